"""Writes tests/golden/peptide_labels.npz: the reference's peptide_simulator.py with several label letters, run molecule by
molecule under the explicit Philox draws of _host_peptide_sim.py (the draw contract of include/fsq_peptide_labels.h).  Data
only: parameters, seeds and recorded results.

The reference is loaded at run time through oracle/refload.py, as tools/gen_peptide_sim_golden.py loads it (which also
asserts, on numpy itself, that lognormal = exp(mean + sigma * z) on the polar normals).  Its module-level `random` is replaced
by an object whose random() reads the current molecule's stream 0 (simulate_dye_counts) or, letter by letter, that channel's
superdye stream (simulate_photometries); its `np` by a stand-in whose random.lognormal is exp(mean + sigma * z) on that
channel's normal stream, starting with an empty cache.

The reference keeps the letters in a set and in dicts, whose order under Python 3 changes from process to process; the
recorded texts put every dict over the letters in sorted-letter order, the order contract of this package.

  python tools/gen_peptide_labels_golden.py [--reference DIR]
"""
import argparse
import math
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_REPR = 25                                  # molecules per case recorded as the reference's own tuples (text)
DDIF7 = [0, 0.3] + [0.3] * 5
CHEM = dict(p=0.9, dd=0.1, u=0.5, s=0.3, sc=3, s2=0.1)

# name, sequence, labels, mocks, edmans, dict(p, dye_destruction, u, s, sc, s2), then one value for all letters or {letter: value}:
# beta, beta_sigma, ddif, rate, factor; seed, first, n
CASES = (
    ("two_letters", "GAKCGAKC", "KC", 2, 4, CHEM, 70000.0, 0.2, DDIF7, 0.0, 1.0, 20240917, 0, 160),
    ("three_interleaved", "KCDAKCDGKCDA", "DKC", 3, 8, dict(p=0.92, dd=0.06, u=0.3, s=0.12, sc=2, s2=0.04),
     {"C": 52000.0, "D": 70000.0, "K": 31000.5}, {"C": 0.2, "D": 0.15, "K": 0.25},
     {"C": DDIF7, "D": [0.0, 0.1, 0.2], "K": [0.0, 0.25, 0.35, 0.4]}, {"C": 0.0, "D": 0.4, "K": 0.0}, {"C": 1.0, "D": 2.5, "K": 1.0},
     0x9e3779b97f4a7c15, 2 ** 32 - 70, 160),
    ("absent_letter", "GAKAGAKC", "YK", 2, 4, CHEM, 70000.0, 0.2, DDIF7, 0.3, 2.0, 5, 10 ** 12, 150),
    ("shorter_than_edmans", "KC", "KC", 0, 6, dict(p=0.8, dd=0.05, u=0.2, s=0.05, sc=100, s2=0.5), {"C": 9000.0, "K": 12000.0}, 0.3,
     [0.0, 0.25], 0.5, 2.0, 2 ** 64 - 1, 5, 150),
    ("mocks_only", "CAKAC", "CK", 3, 0, dict(p=0.9, dd=0.2, u=0.3, s=0.2, sc=1, s2=0.05), 70000.0, 0.2, DDIF7, {"C": 1.0, "K": 0.0}, 1.7,
     99, 0, 150),
    ("one_frame", "AKC", "CK", 0, 0, CHEM, 70000.0, 0.2, DDIF7, 0.0, 1.0, 3, 0, 150),
    ("one_letter", "GAKAGAKC", "K", 2, 4, CHEM, 70000.0, 0.2, DDIF7, 0.0, 1.0, 20240901, 0, 150),     # peptide_sim.npz's case 0
)


class Draws(object):
    """What stands in for the reference's `random` module."""

    def __init__(self):
        self.current = None

    def random(self):
        return self.current()

    def seed(self, *a):
        pass


def per_letter(value, letters):
    return [value[L] for L in letters] if isinstance(value, dict) else [value] * len(letters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("FSQ_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "peptide_labels.npz"))
    a = ap.parse_args()
    os.environ["FSQ_REFERENCE"] = a.reference
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, ROOT)
    import refload
    refload.REF = a.reference
    from fluorosequencingimageanalysis_amd import _host_peptide_sim as T

    import string
    if not hasattr(string, "letters"):
        string.letters = string.ascii_letters
    mc = types.ModuleType("MCsimlib")
    mc._pairwise = lambda seq: zip(seq[:-1], seq[1:])
    sys.modules["MCsimlib"] = mc
    ps = refload.load("peptide_simulator", "peptide_simulator.py")
    draws = Draws()
    ps.random = draws
    state = {}

    class NpRandom(object):
        @staticmethod
        def lognormal(mean, sigma, size):
            return np.array([T.lognormal(state["normals"], mean, sigma) for _ in range(size)])

    class Np(object):
        random = NpRandom

        def __getattr__(self, k):
            return getattr(np, k)
    ps.np = Np()

    out = {"case_names": np.array([c[0] for c in CASES])}
    cause_of = {v: k for k, v in T.CAUSE_NAMES.items()}
    for ci, (name, seq, labels, mocks, edmans, e, beta, sigma, ddif, rate, factor, seed, first, n) in enumerate(CASES):
        letters = sorted(set(labels))
        K = len(letters)
        betas, sigmas, ddifs = per_letter(beta, letters), per_letter(sigma, letters), per_letter(ddif, letters)
        rates, factors = per_letter(rate, letters), per_letter(factor, letters)
        b = -math.log(1.0 - e["dd"])
        pos = [i for i, ch in enumerate(seq) if ch in letters]
        F, L = mocks + edmans + 1, len(pos)
        reserved = "Z"
        counts, inten = np.zeros((K, n, F), np.uint8), np.zeros((K, n, F))
        lcyc, lcause = np.zeros((n, L), np.uint8), np.zeros((n, L), np.uint8)
        fail, cat, nd = np.zeros(n, np.uint64), np.zeros((K, n), np.uint64), np.zeros((n, 1 + 2 * K), np.int32)
        text = []
        for i in range(n):
            mol = first + i
            s0 = T.Stream(seed, mol, 0)
            draws.current = s0
            (dec, dc, ev, tracker), = ps.simulate_dye_counts(seq, labels, mocks, edmans, num_simulations=1, reserved_character=reserved,
                                                             p=e["p"], b=b, u=e["u"], s=e["s"], sc=e["sc"], s2=e["s2"])
            assert sorted(dc) == letters
            nd[i, 0] = s0.j
            categories = {}
            for k, letter in enumerate(letters):
                s1, s2 = T.Stream(seed, mol, T.superdye_stream(k)), T.Stream(seed, mol, T.normal_stream(k))
                draws.current, state["normals"] = s1, T.Normals(s2)
                category, (ints,) = ps.simulate_photometries(dye_counts=dc[letter], beta=betas[k], beta_sigma=sigmas[k], number=1,
                                                             ddif=ddifs[k], dye_position_tracker=tracker, distance_ddif=None,
                                                             superdye_rate=rates[k], superdye_factor=factors[k])
                counts[k, i], inten[k, i] = dc[letter], [float(x) for x in ints]
                cat[k, i] = sum(1 << f for f, c in enumerate(category) if c)
                nd[i, 1 + 2 * k:3 + 2 * k] = (s1.j, s2.j)
                categories[letter] = category
            for x in ev:
                if x.event_name in cause_of:
                    k = pos.index(x.original_position - 1)
                    assert lcause[i, k] == 0 and x.original_amino_acid == seq[pos[k]]
                    lcyc[i, k], lcause[i, k] = x.cycle_number, cause_of[x.event_name]
                elif x.event_name == 'edman failure':
                    fail[i] |= np.uint64(1 << x.cycle_number)
            if i < N_REPR:
                ev = [x._replace(message=dict(sorted(x.message.items()))) if x.event_name == 'dye count' else x for x in ev]
                text.append(repr((dec, dict(sorted(dc.items())), ev, tracker, categories)))
        pre = "c%d_" % ci
        nd_max = max(len(row) for row in ddifs)
        out.update({pre + "sequence": np.array(seq), pre + "labels": np.array(labels), pre + "reserved": np.array(reserved),
                    pre + "ints": np.array([mocks, edmans, e["sc"], n], np.int64), pre + "seed": np.array([seed], np.uint64),
                    pre + "first": np.array([first], np.int64),
                    pre + "floats": np.array([e["p"], b, math.e ** -b, e["u"], e["s"], e["s2"]]),
                    pre + "channel_floats": np.array([betas, sigmas, rates, factors], np.float64),
                    pre + "n_ddif": np.array([len(row) for row in ddifs], np.int64),
                    pre + "ddif": np.array([list(row) + [0.0] * (nd_max - len(row)) for row in ddifs], np.float64),
                    pre + "counts": counts, pre + "loss_cycle": lcyc, pre + "loss_cause": lcause, pre + "edman_fail": fail,
                    pre + "category": cat, pre + "intensity": inten, pre + "n_draws": nd, pre + "tuples": np.array(text)})
        two = sum(1 for i in range(n) for c in range(F)
                  if len({seq[pos[k]] for k in range(L) if lcause[i, k] and lcyc[i, k] == c}) > 1)
        print("%-20s %4d molecules, letters %s, %3d distinct joint count rows, %d (molecule, cycle) pairs losing dyes of two letters" %
              (name, n, "".join(letters), len({tuple(counts[:, i].reshape(-1).tolist()) for i in range(n)}), two))
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
