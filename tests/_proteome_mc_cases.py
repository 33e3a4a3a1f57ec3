"""Inputs shared by tests/test_proteome_mc_host.py and tests/test_gpu_proteome_mc.py: the golden (tests/golden/proteome_mc.npz,
the reference's MCsimlib.py under this library's draws), the peptides, windows and parameter corners of the device tests, the
tally and uniques inputs, the synthetic proteome and one case with more rows than one pass of the kernels' grid.  Expected
values come from the NumPy twin (_host_proteome_mc), which the host file pins to the golden.  Everything is seeded and built
once.  No torch, no GPU."""
import functools
import json
import os

import numpy as np

from fluorosequencingimageanalysis_amd import _host_proteome_mc as H
from _util import GOLD

PMC_BLOCK, PMC_MAX_BLOCKS = 256, 2048           # kpm_signals' and kpm_tally's grid (csrc/simulate/fsq_proteome_mc.hip)
ONE_PASS = PMC_BLOCK * PMC_MAX_BLOCKS           # 524 288 rows

FULL = tuple(range(1, 17))
WINDOWS = {"gapped": {'D': (3, 4, 7), 'K': (7, 8, 9)}, "full": {'D': FULL, 'K': FULL}}
# (p, b, u): p = 0 is the stall path; p = 1, b = 0 and u = 1 are the trivial ones
CORNERS = [(0.9, 0.05, 0.3), (0.5, 5.0, 0.0), (0.0, 0.05, 0.3), (1.0, 0.0, 0.0), (0.9, 0.05, 1.0), (0.5, 0.0, 0.3)]

_H255 = list("A" * 255)
for _x, _c in ((1, 'K'), (2, 'D'), (30, 'K'), (100, 'D'), (254, 'K'), (255, 'D')):
    _H255[_x - 1] = _c
PEPTIDES = {                                                    # 3 proteins, 6 peptides
    "P0": (("AAGA", "CAA"), ("AGA", "CKDK")),                   # no label; tail labels only
    "P1": (("KD" * 20, "C" + "KD" * 12), ("K", "CD")),          # 64 labels; a head of one
    "P2": (("".join(_H255), "CK"), ("AKDAAKDAADKAA", "CKAD")),  # a head of 255; an ordinary peptide
}
SAMPLE_SIZE, SEED = 70, 20261020                                # peptide boundaries fall inside wavefronts, the last wave is partial
CHUNK = (100, 130)
FIRST_SAMPLE_WORD = 2**32 - 50                                  # the item's low word wraps inside the run


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(os.path.join(GOLD, "proteome_mc.npz"))
    out = {k: g[k] for k in ("signal_start", "signal_pos", "signal_acid", "n_draws")}
    for k in ("signal_cases", "preprocessing", "uniques"):
        out[k] = json.loads(str(g[k]))
    return out


def golden_signals(ci):
    """The 300 recorded signals of golden case ci as tuples of (position, acid)."""
    g = golden()
    order = sorted(g["signal_cases"][ci]["windows"])
    n = g["n_draws"].shape[1]
    s = g["signal_start"][ci * n:(ci + 1) * n + 1]
    return [tuple((int(x), order[a]) for x, a in zip(g["signal_pos"][lo:hi], g["signal_acid"][lo:hi])) for lo, hi in zip(s[:-1], s[1:])]


def tupled(x):
    """JSON lists back as the tuples the reference returns."""
    return tuple(tupled(v) for v in x) if isinstance(x, list) else x


@functools.lru_cache(maxsize=None)
def table(which):
    return H.peptide_table(PEPTIDES, WINDOWS[which])


@functools.lru_cache(maxsize=None)
def expected_signals(which, corner, first_sample=0):
    p, b, u = CORNERS[corner]
    keys, draws = H.signals(table(which), p, b, u, SAMPLE_SIZE, SEED, first_sample)
    keys.setflags(write=False), draws.setflags(write=False)
    return keys, draws


# ---- the tally ----

def _rows(keys, proteins, counts, seed):
    k, p = np.repeat(np.asarray(keys, np.uint64), counts), np.repeat(np.asarray(proteins, np.int32), counts)
    order = np.random.default_rng(seed).permutation(len(k))
    return k[order], p[order]


@functools.lru_cache(maxsize=None)
def tally_cases():
    """name -> (keys uint64, proteins int32, signal_slots, pair_slots)."""
    rng = np.random.default_rng(77)
    keys = rng.integers(1, 2**63, 300).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    keys[0], keys[1] = np.uint64(2**64 - 1), np.uint64(1)                   # the all-ones key
    k3, p3 = np.repeat(keys, 3), np.tile(np.arange(3, dtype=np.int32), 300)
    many = _rows(k3, p3, rng.integers(1, 12, 900), 1)
    many = (np.concatenate([many[0], np.zeros(40, np.uint64)]), np.concatenate([many[1], np.full(40, 1, np.int32)]))   # key 0 rows
    few = _rows(keys[:20], np.zeros(20, np.int32), rng.integers(1, 9, 20), 2)
    return {"contention": (np.full(65536, 0x1234, np.uint64), np.full(65536, 2, np.int32), 64, 64),
            "many": many + (512, 1024),
            "overflow": few + (8, 64),
            "one_slot": (np.full(100, 99, np.uint64), np.full(100, 5, np.int32), 1, 1),
            "one_slot_two_keys": (np.array([5, 9] * 50, np.uint64), np.zeros(100, np.int32), 1, 4),
            "one_pair_slot": (np.array([5] * 100, np.uint64), np.array([0, 1] * 50, np.int32), 4, 1)}


# ---- the uniques ----

def golden_triples():
    """The golden's count dicts as sorted triples: case i is key i + 1, protein 'P<k>' is index k."""
    cases = golden()["uniques"]["cases"]
    k = np.concatenate([np.full(len(c), i + 1, np.uint64) for i, (_, _, c) in enumerate(cases)])
    p = np.concatenate([np.arange(len(c), dtype=np.int32) for _, _, c in cases])
    c = np.concatenate([np.array(c, np.int64) for _, _, c in cases])
    return k, p, c


def golden_unique_expected(listed):
    """A recorded find_uniques result as {case index: (best, [second, ties ...], tertiary)} with protein indices (-1: None)."""
    cases = golden()["uniques"]["cases"]
    index = {tupled(sig): i for i, (_, sig, _) in enumerate(cases)}
    num = lambda name: -1 if name is None else int(name[1:])
    return {index[tupled(sig)]: ((num(best[0]), best[1]), [(num(n), c) for n, c in second], tertiary)
            for sig, best, second, tertiary in listed}


def unique_lists(result, triples, demote=False):
    """A uniques result (the twin's or the device's arrays) in the shape of golden_unique_expected."""
    return H.unique_lists(dict(result, segment=H.segments(triples[0])), triples, demote)


@functools.lru_cache(maxsize=None)
def random_triples(n_signals=1000, seed=5):
    """n_signals signals of 1 .. 40 proteins each, small counts (many ties)."""
    rng = np.random.default_rng(seed)
    k, p, c = [], [], []
    for i in range(n_signals):
        m = int(rng.integers(1, 41))
        k.append(np.full(m, 1000 + 3 * i, np.uint64))
        p.append(np.sort(rng.choice(60, m, replace=False)).astype(np.int32))
        c.append(rng.integers(1, 7 if i % 2 else 40, m).astype(np.int64))
    return np.concatenate(k), np.concatenate(p), np.concatenate(c)


UNIQUE_ARGS = [(None, 1, None), (None, 5, None), (2.0, 1, None), (1.0, 3, None), (1.4, 1, 4), (None, 1, 3), (2.0, 6, 2), (1.8, 9, 5)]
ABSOLUTE_ARGS = [(5, 3), (1, 10), (3, 0), (7, 5)]


def top_two(triples):
    """NumPy's answer for demote=True: per signal (best protein, best count, second protein, second count, ties, tertiary)."""
    k, p, c = triples
    seg = H.segments(k)
    out = []
    for lo, hi in zip(seg[:-1], seg[1:]):
        order = np.lexsort((p[lo:hi], -c[lo:hi]))
        pp, cc = p[lo:hi][order], c[lo:hi][order]
        if len(pp) == 1:
            out.append((int(pp[0]), int(cc[0]), -1, 0, 0, 0))
        else:
            rest = cc[2:]
            out.append((int(pp[0]), int(cc[0]), int(pp[1]), int(cc[1]), int((rest == cc[1]).sum()), int(rest[rest < cc[1]].sum())))
    return out


# ---- the synthetic proteome ----

ACIDS, FREQ = "ACDEGKLS", np.array([0.22, 0.06, 0.10, 0.08, 0.16, 0.12, 0.16, 0.10])


@functools.lru_cache(maxsize=None)
def proteome(n=40, length=60, seed=11):
    rng = np.random.default_rng(seed)
    return {"prot%02d" % i: "".join(rng.choice(list(ACIDS), length, p=FREQ)) for i in range(n)}


E2E = dict(p=0.9, b=0.05, u=0.1, windows={'D': tuple(range(1, 11)), 'K': tuple(range(1, 11))}, sample_size=200, seed=424242)
E2E_UNIQUES = dict(worst_ratio=3.0, absolute_min=4, maximum_secondary=None)


@functools.lru_cache(maxsize=None)
def e2e_peptides():
    return H.attach(H.cleave(proteome(), 'E'), 'C')


# ---- more rows than one pass of the grid ----

LIMIT_PEPTIDES = {"Q0": (("AKDAAKDAADKAA", "CKAD"), ("K", "CD")), "Q1": (("DAK", "CK"), ("AAGA", "CAA"), ("KDKD", "C"))}
LIMIT_SAMPLE_SIZE = (ONE_PASS + 333) // 5 + 1                   # 5 peptides: 524 625 rows, 337 beyond one pass
LIMIT = dict(p=0.9, b=0.05, u=0.3, seed=99, first_sample=12345)


@functools.lru_cache(maxsize=None)
def limit_table():
    return H.peptide_table(LIMIT_PEPTIDES, WINDOWS["full"])


@functools.lru_cache(maxsize=None)
def limit_expected():
    """(keys, proteins) of the whole limit case by the vectorised twin, a peptide's 104 925 samples at a time."""
    t = limit_table()
    keys, _ = H.signals(t, LIMIT["p"], LIMIT["b"], LIMIT["u"], LIMIT_SAMPLE_SIZE, LIMIT["seed"], LIMIT["first_sample"])
    return keys, H.row_proteins(t, LIMIT_SAMPLE_SIZE, 0, len(keys))
