"""Inputs shared by tests/test_proteome_sweep_host.py and tests/test_gpu_proteome_sweep.py: the peptides, windows, sample size
and seed of tests/_proteome_mc_cases.py (420 rows a point, peptide boundaries inside wavefronts) at eight (p, b, u) points - its
six corners and two more, so that four distinct p and three distinct b are each shared by several points.  Expected values come
from the single-point NumPy twin (_host_proteome_mc.signals / tally / _uniques), which tests/test_proteome_mc_host.py pins to the
golden.  Everything is seeded and built once.  No torch, no GPU."""
import functools

import numpy as np

from fluorosequencingimageanalysis_amd import _host_proteome_mc as H
import _proteome_mc_cases as C

PEPTIDES, WINDOWS, SAMPLE_SIZE, SEED = C.PEPTIDES, C.WINDOWS, C.SAMPLE_SIZE, C.SEED
ROWS = 6 * SAMPLE_SIZE                                          # 420 rows a point
POINTS = list(C.CORNERS) + [(0.9, 0.05, 0.0), (0.9, 5.0, 0.3)]
STRIDE = 1000
FIRST_SAMPLE_WORD = C.FIRST_SAMPLE_WORD
CHUNKS = (100, 130)                                             # rows a launch: neither divides 420

# the entries of the corners' Edman tables through row d = 3 (rows of 20, 63, 1 and 2 entries): a wrong table index shows
EDMAN_THROUGH_3 = {0.9: 57, 0.5: 177, 0.0: 3, 1.0: 6}

# isolation under overflow: gapped windows, tables of 8 signal slots and 16 pair slots; by the twin the six corners have
OVERFLOW_SLOTS = (8, 16)
CORNER_SIGNALS, CORNER_PAIRS = (45, 6, 51, 2, 0, 17), (62, 10, 66, 2, 0, 26)

GRID_2X2X2 = H.grid_points((0.9, 0.6), (0.05, 0.5), (0.1, 0.4))


@functools.lru_cache(maxsize=None)
def expected_signals(which, k, first_sample=0, stride=0):
    """(keys, n_draws) of point k alone by the single-point twin, its first sample first_sample + k * stride."""
    p, b, u = POINTS[k]
    keys, draws = H.signals(C.table(which), p, b, u, SAMPLE_SIZE, SEED, first_sample + k * stride)
    keys.setflags(write=False), draws.setflags(write=False)
    return keys, draws


def expected_grid(which, first_sample=0, stride=0):
    """(keys [8][420], n_draws [8][420]) stacked from the single-point twin."""
    got = [expected_signals(which, k, first_sample, stride) for k in range(len(POINTS))]
    return np.stack([k for k, _ in got]), np.stack([d for _, d in got])


@functools.lru_cache(maxsize=None)
def expected_triples(which, k, stride=0):
    """The sorted (key, protein, count) triples of point k alone."""
    return H.tally(expected_signals(which, k, 0, stride)[0], H.row_proteins(C.table(which), SAMPLE_SIZE, 0, ROWS))


@functools.lru_cache(maxsize=None)
def e2e_table():
    return H.peptide_table(C.e2e_peptides(), C.E2E["windows"])


@functools.lru_cache(maxsize=None)
def e2e_curve_by_the_loop(stride=0):
    """Per point of GRID_2X2X2: (triples, uniques, identifiable {name: n}) by the single-point twin on e2e_peptides()."""
    t = e2e_table()
    S, seed = C.E2E["sample_size"], C.E2E["seed"]
    proteins = H.row_proteins(t, S, 0, len(t["protein"]) * S)
    out = []
    for k, (p, b, u) in enumerate(GRID_2X2X2):
        triples = H.tally(H.signals(t, p, b, u, S, seed, k * stride)[0], proteins)
        out.append((triples, H.uniques(triples, **C.E2E_UNIQUES)))
    return out


def curve_of_loop(per_point, n_proteins):
    """The five curve columns and the identifiable matrix from e2e_curve_by_the_loop's per-point results, in plain NumPy."""
    out = {name: [] for name in H.CURVE_FIELDS}
    identifiable = np.zeros((len(per_point), n_proteins), np.uint8)
    for i, (triples, uniq) in enumerate(per_point):
        passed = uniq["passed"] != 0
        out["n_signals"].append(len(uniq["key"])), out["n_pairs"].append(len(triples[0]))
        out["samples_detected"].append(int(triples[2].sum())), out["n_passing_signals"].append(int(passed.sum()))
        identifiable[i, np.unique(uniq["best_protein"][passed])] = 1
        out["n_identifiable_proteins"].append(len(np.unique(uniq["best_protein"][passed])))
    out = {k: np.array(v, np.int64) for k, v in out.items()}
    out["identifiable"] = identifiable
    return out
