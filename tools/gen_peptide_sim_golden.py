"""Writes tests/golden/peptide_sim.npz: the reference's peptide_simulator.py run molecule by molecule under the explicit
Philox draws of _host_peptide_sim.py, and what simulate_peptide.py makes of one case (convert_to_oldstyle, the
photometries CSV, molecular_error_signals).  Data only: parameters, seeds and recorded results.

The reference is loaded at run time through oracle/refload.py.  Its module-level `random` is replaced by an object whose
random() reads the current molecule's stream 0 (simulate_dye_counts) or stream 1 (simulate_photometries) and whose seed() does
nothing; its `np` by a stand-in whose random.lognormal is exp(mean + sigma * z) on stream 2's polar normals.  Before that the
generator asserts, on numpy itself, that this is what numpy computes: over 10^4 (mean, sigma, seed) triples
RandomState(seed).lognormal(mean, sigma) has the bits of math.exp(mean + sigma * RandomState(seed).standard_normal()), and the
twin's polar method on RandomState(seed).random_sample() has the bits of RandomState(seed).standard_normal().

It also times the reference with its own `random` (one core, 2 000 molecules) and prints the rate.

  python tools/gen_peptide_sim_golden.py [--reference DIR]
"""
import argparse
import math
import os
import struct
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_REPR = 25                                  # molecules per case recorded as the reference's own tuples (text)
DDIF7 = [0, 0.3] + [0.3] * 5

# name, sequence, label, mocks, edmans, dict(p, dye_destruction, u, s, sc, s2), beta, beta_sigma, ddif, rate, factor, seed, first, n
CASES = (
    ("two_k", "GAKAGAKC", "K", 2, 4, dict(p=0.9, dd=0.1, u=0.5, s=0.3, sc=3, s2=0.1), 70000.0, 0.2, DDIF7, 0.0, 1.0,
     20240901, 0, 300),
    ("default_shape_superdye", "KAKGKAAGKAGC", "K", 3, 8, dict(p=0.9, dd=0.1, u=0.5, s=0.3, sc=3, s2=0.1), 70000.0, 0.2, DDIF7,
     0.3, 2.5, 0x9e3779b97f4a7c15, 2 ** 32 - 100, 300),
    ("fifteen_labels", "KAKGG" * 7 + "AAAAK", "K", 5, 20, dict(p=0.95, dd=0.03, u=0.1, s=0.02, sc=0, s2=0.01), 12345.5, 0.15,
     [0.0] + [0.05 * i for i in range(1, 15)], 0.0, 1.0, 7, 10 ** 12, 150),
    ("shorter_than_edmans", "KK", "K", 0, 6, dict(p=0.8, dd=0.05, u=0.2, s=0.05, sc=100, s2=0.5), 9000.0, 0.3, [0.0, 0.25], 0.5,
     2.0, 2 ** 64 - 1, 5, 200),
    ("mocks_only_first_last", "CAAAC", "C", 3, 0, dict(p=0.9, dd=0.2, u=0.3, s=0.2, sc=1, s2=0.05), 70000.0, 0.2, DDIF7, 1.0, 1.7,
     99, 0, 200),
    ("one_frame", "AKA", "K", 0, 0, dict(p=0.9, dd=0.1, u=0.5, s=0.3, sc=3, s2=0.1), 70000.0, 0.2, DDIF7, 0.0, 1.0, 3, 0, 200),
)


def py2_str(x):
    """str() as Python 2 wrote a float: 12 significant digits."""
    if isinstance(x, (float, np.floating)):
        s = "%.12g" % float(x)
        if s in ("inf", "-inf", "nan"):
            return s
        return s if ("." in s or "e" in s) else s + ".0"
    return str(x)


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def numpy_identities(T):
    rng = np.random.default_rng(11)
    for _ in range(10000):
        mean, sigma, seed = float(rng.uniform(5, 14)), float(rng.uniform(0.01, 0.6)), int(rng.integers(0, 2 ** 32))
        a = np.random.RandomState(seed).lognormal(mean, sigma)
        z = np.random.RandomState(seed).standard_normal()
        assert bits(a) == bits(math.exp(mean + sigma * z)), (mean, sigma, seed)
        assert bits(np.random.RandomState(seed).lognormal(mean, sigma, size=1)[0]) == bits(a)
    for seed in range(300):
        rs = np.random.RandomState(seed)
        g = T.Normals(lambda: float(rs.random_sample()))
        mine = [g() for _ in range(6)]
        theirs = np.random.RandomState(seed).standard_normal(6)
        assert [bits(x) for x in mine] == [bits(x) for x in theirs], seed


class Draws(object):
    """What stands in for the reference's `random` module."""

    def __init__(self):
        self.current = None

    def random(self):
        return self.current()

    def seed(self, *a):
        pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("FSQ_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "peptide_sim.npz"))
    a = ap.parse_args()
    os.environ["FSQ_REFERENCE"] = a.reference
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, ROOT)
    import refload
    refload.REF = a.reference
    from fluorosequencingimageanalysis_amd import _host_peptide_sim as T
    numpy_identities(T)
    print("numpy: lognormal = exp(mean + sigma * z) and the polar normals hold bit for bit")

    import string
    if not hasattr(string, "letters"):
        string.letters = string.ascii_letters
    mc = types.ModuleType("MCsimlib")
    mc._pairwise = lambda seq: zip(seq[:-1], seq[1:])
    sys.modules["MCsimlib"] = mc
    ps = refload.load("peptide_simulator", "peptide_simulator.py")

    # ---- the reference's own rate, with its own random ---------------------------------------------------------------
    kw = dict(p=0.9, b=-math.log(1.0 - 0.1), u=0.5, s=0.3, sc=3, s2=0.1)
    t0 = time.time()
    res = ps.simulate_dye_counts("GAKAGAKC", "K", 2, 4, num_simulations=2000, reserved_character="Z", **kw)
    for dec, dc, ev, tr in res:
        for L, counts in dc.items():
            ps.simulate_photometries(dye_counts=counts, beta=70000.0, beta_sigma=0.2, number=1, ddif=DDIF7)
    dt = time.time() - t0
    print("reference, its own random, one core: 2000 molecules (2 mocks + 4 Edmans) in %.2f s: %.0f molecules/s" % (dt, 2000 / dt))

    # ---- the reference under our draws -------------------------------------------------------------------------------
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
    kept_case = None
    for ci, (name, seq, label, mocks, edmans, e, beta, sigma, ddif, rate, factor, seed, first, n) in enumerate(CASES):
        b = -math.log(1.0 - e["dd"])
        per_cycle_b = math.e ** -b
        pos = [i for i, ch in enumerate(seq) if ch == label]
        F, L = mocks + edmans + 1, len(pos)
        reserved = "Z"
        counts, lcyc, lcause = np.zeros((n, F), np.uint8), np.zeros((n, L), np.uint8), np.zeros((n, L), np.uint8)
        fail, cat, inten, nd = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros((n, F)), np.zeros((n, 3), np.int32)
        text, merged = [], []
        cause_of = {v: k for k, v in T.CAUSE_NAMES.items()}
        for i in range(n):
            mol = first + i
            s0, s1, s2 = T.Stream(seed, mol, 0), T.Stream(seed, mol, 1), T.Stream(seed, mol, 2)
            draws.current = s0
            (dec, dc, ev, tracker), = ps.simulate_dye_counts(seq, label, mocks, edmans, num_simulations=1, reserved_character=reserved,
                                                             p=e["p"], b=b, u=e["u"], s=e["s"], sc=e["sc"], s2=e["s2"])
            draws.current, state["normals"] = s1, T.Normals(s2)
            category, (ints,) = ps.simulate_photometries(dye_counts=dc[label], beta=beta, beta_sigma=sigma, number=1, ddif=ddif,
                                                         dye_position_tracker=tracker, distance_ddif=None, superdye_rate=rate,
                                                         superdye_factor=factor)
            counts[i] = dc[label]
            for x in ev:
                if x.event_name in cause_of:
                    k = pos.index(x.original_position - 1)
                    assert lcause[i, k] == 0
                    lcyc[i, k], lcause[i, k] = x.cycle_number, cause_of[x.event_name]
                elif x.event_name == 'edman failure':
                    fail[i] |= np.uint64(1 << x.cycle_number)
            cat[i] = sum(1 << f for f, c in enumerate(category) if c)
            inten[i] = [float(x) for x in ints]
            nd[i] = (s0.j, s1.j, s2.j)
            if i < N_REPR:
                text.append(repr((dec, dc, ev, tracker, category)))
            merged.append((dec, dc, ev, {label: (category, (tuple(float(x) for x in ints),))}))
        pre = "c%d_" % ci
        out.update({pre + "sequence": np.array(seq), pre + "label": np.array(label), pre + "reserved": np.array(reserved),
                    pre + "ints": np.array([mocks, edmans, e["sc"], n], np.int64), pre + "seed": np.array([seed], np.uint64),
                    pre + "first": np.array([first], np.int64),
                    pre + "floats": np.array([e["p"], b, per_cycle_b, e["u"], e["s"], e["s2"], beta, sigma, rate, factor]),
                    pre + "ddif": np.array(ddif, np.float64), pre + "counts": counts, pre + "loss_cycle": lcyc,
                    pre + "loss_cause": lcause, pre + "edman_fail": fail, pre + "category": cat, pre + "intensity": inten,
                    pre + "n_draws": nd, pre + "tuples": np.array(text)})
        print("%-24s %4d molecules, %3d distinct count rows, stream-0 draws %d .. %d, %d lost a dye to Edman, %d Edman failures" %
              (name, n, len({tuple(r) for r in counts.tolist()}), nd[:, 0].min(), nd[:, 0].max(), int((lcause == 3).any(1).sum()),
               int((fail != 0).sum())))
        if ci == 0:
            kept_case = merged

    # ---- what simulate_peptide.py makes of case 0 (:239-262) ---------------------------------------------------------
    index_of = {id(m[2]): i for i, m in enumerate(kept_case)}
    results = ps.convert_to_oldstyle(kept_case)
    mes, photometries, t, kept, decs = {}, {'ch1': {0: {}}}, 0, [], []
    for dye_decrements, dye_counts, event_buffer, intensities_dict in results:
        kept.append(index_of[id(event_buffer)])
        decs.append(dye_decrements)
        for label, (category, (intensities,)) in intensities_dict.items():
            photometries['ch1'][0].setdefault((t, t), (category, intensities, t))
            t += 1
        (label, seq_), = dye_counts.items()
        key = (dye_decrements, True if seq_[-1] == 0 else False, seq_[0])
        mes[key] = mes.get(key, 0) + 1
    from gen_lognormal_golden import load_functions
    import csv
    ns = load_functions(refload, "MCsimlib.py", ("unwind_photometries", "write_photometries_dict_to_csv"), {"csv": csv, "str": py2_str})
    with tempfile.TemporaryDirectory() as d:
        rows = ns["write_photometries_dict_to_csv"](photometries=photometries, filepath=os.path.join(d, "x.csv"))
        import gc
        gc.collect()                                             # (the reference never closes its writer's file)
        csv_text = open(os.path.join(d, "x.csv"), newline='').read()
    assert rows == len(kept) and csv_text.count("\n") == rows + 1
    out.update(old_kept=np.array(kept, np.int64), old_decrements=np.array(repr(decs)), old_csv=np.frombuffer(csv_text.encode(), np.uint8),
               old_molecular_error_signals=np.array(repr(sorted(mes.items()))))
    print("case 0 through convert_to_oldstyle: %d of %d molecules kept, %d molecular error signals" % (len(kept), len(kept_case), len(mes)))
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
