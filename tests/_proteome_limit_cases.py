"""Inputs and expected values of the proteome Monte-Carlo's limit tests (tests/test_proteome_limits_host.py proves that they
reach the edges named here, tests/test_gpu_proteome_limits.py feeds them to the device).  Everything is seeded and built once.
Expected values come from the NumPy twin (_host_proteome_mc), which tests/test_proteome_mc_host.py pins to the reference's
golden.  No torch, no GPU.

  A  kpm_signals at the key's limits: eight acids of eight observable positions each (64 key bits, bit 63 = (63, 'Y')), window
     positions up to 63, heads of up to 255 residues whose labels are delayed beyond position 64
  B  kpm_uniques over more signals than one pass of its grid, and on one segment of 100 000 proteins between two of one"""
import functools

import numpy as np

from fluorosequencingimageanalysis_amd import _host_proteome_mc as H
from _proteome_mc_cases import ONE_PASS, top_two

# ---- A: the signals at the key's limits ---------------------------------------------------------------------------------------
ACIDS = "CDEKMSTY"
FIRST_WINDOW = (1, 8, 15, 22, 30, 40, 47, 56)                   # the last window ends at 63
WINDOWS = {acid: tuple(range(first, first + 8)) for acid, first in zip(ACIDS, FIRST_WINDOW)}
CORNERS = [(0.9, 0.05, 0.1), (0.5, 0.02, 0.0), (0.97, 0.0, 0.0), (0.6, 5.0, 0.3)]           # (p, b, u)
SAMPLE_SIZE, SEED = 70, 20261020                                # 5 peptides: 350 rows, peptide boundaries inside wavefronts
CHUNK = (100, 130)                                              # rows 100 .. 229: from inside peptide 1 to inside peptide 3
FIRST_SAMPLE_WORD = 2**32 - 50                                  # the item's low word wraps inside the run


def _sequence(rng, length, density):
    """`length` residues, round(density * length) of them one of ACIDS at seeded places, the others 'A'."""
    seq = ["A"] * length
    for at in rng.choice(length, int(round(density * length)), replace=False).tolist():
        seq[at] = ACIDS[int(rng.integers(0, len(ACIDS)))]
    return "".join(seq)


@functools.lru_cache(maxsize=None)
def peptides():
    """Three proteins, five peptides: (head, tail)."""
    rng = np.random.default_rng(6463)
    return {"L0": ((_sequence(rng, 63, 0.5), "CAY"), (_sequence(rng, 90, 0.3), "CK")),
            "L1": ((ACIDS * 7 + "A" * 7, "CY"), ("Y" * 59 + "AAAY", "CYYY")),        # 58 labels; 64 labels, 60 in the head
            "L2": ((_sequence(rng, 255, 0.2), "CT"),)}


@functools.lru_cache(maxsize=None)
def table():
    return H.peptide_table(peptides(), WINDOWS)


@functools.lru_cache(maxsize=None)
def expected_signals(corner, first_sample=0):
    """(keys uint64 [350], n_draws int32 [350]) by the vectorised twin."""
    p, b, u = CORNERS[corner]
    keys, draws = H.signals(table(), p, b, u, SAMPLE_SIZE, SEED, first_sample)
    keys.setflags(write=False), draws.setflags(write=False)
    return keys, draws


def flat_peptides():
    """The (head, tail) pairs in the table's order."""
    return [peptide for name in peptides() for peptide in peptides()[name]]


# ---- B: the scan beyond one pass and on a long segment ------------------------------------------------------------------------
TILES, BLOCK_SIGNALS = 525, 1000                                # 525 000 signals: 712 beyond one pass of 524 288
LONG_PROTEINS, LONG_TIES = 100000, 1000
# (ratio_mode, worst_ratio, absolute_min, has_maximum_secondary, maximum_secondary): no ratio, a ratio with a maximum, absolute
SCAN_MODES = [H.scan_modes(None, 2, None), H.scan_modes(1.4, 1, 4), H.scan_modes(None, 5, 3, absolute=True)]


@functools.lru_cache(maxsize=None)
def block_triples():
    """1 000 signals of 1 .. 6 proteins each with counts 1 .. 6 (many ties): (key, protein, count), keys 1, 2, ..."""
    rng = np.random.default_rng(525)
    k, p, c = [], [], []
    for i in range(BLOCK_SIGNALS):
        m = int(rng.integers(1, 7))
        k.append(np.full(m, i + 1, np.uint64))
        p.append(np.sort(rng.choice(12, m, replace=False)).astype(np.int32))
        c.append(rng.integers(1, 7, m).astype(np.int64))
    return np.concatenate(k), np.concatenate(p), np.concatenate(c)


def tiled_triples(tiles):
    """The block `tiles` times over, tile t's keys BLOCK_SIGNALS * t higher: distinct and ascending."""
    k, p, c = block_triples()
    keys = (k[None, :] + (np.arange(tiles, dtype=np.uint64) * np.uint64(BLOCK_SIGNALS))[:, None]).reshape(-1)
    return keys, np.tile(p, tiles), np.tile(c, tiles)


def tiled_segments(tiles):
    """H.segments(tiled_triples(tiles)[0]) without the keys: the block's starts, shifted tile by tile."""
    seg = H.segments(block_triples()[0])
    starts = (seg[None, :-1] + (np.arange(tiles, dtype=np.int64) * seg[-1])[:, None]).reshape(-1)
    return np.append(starts, tiles * seg[-1]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def block_expected(mode, demote):
    """H._uniques of the block under SCAN_MODES[mode]."""
    return H._uniques(block_triples(), SCAN_MODES[mode], demote)


@functools.lru_cache(maxsize=None)
def long_triples():
    """Three signals: one protein, then 100 000 proteins - counts 1 .. 39, 1 000 of them 40 (the second count) and one 50 at
    seeded places, so that the scan's best is displaced several times -, then one protein."""
    rng = np.random.default_rng(100000)
    c = rng.integers(1, 40, LONG_PROTEINS).astype(np.int64)
    at = rng.choice(LONG_PROTEINS, LONG_TIES + 1, replace=False)
    c[at[:LONG_TIES]] = 40
    c[at[LONG_TIES]] = 50
    k = np.concatenate([[7], np.full(LONG_PROTEINS, 8), [9]]).astype(np.uint64)
    p = np.concatenate([[3], np.arange(LONG_PROTEINS), [5]]).astype(np.int32)
    return k, p, np.concatenate([[4], c, [6]]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def long_expected(mode, demote):
    return H._uniques(long_triples(), SCAN_MODES[mode], demote)


def long_top_two():
    """The independent NumPy answer for demote=True (_proteome_mc_cases.top_two)."""
    return top_two(long_triples())


assert TILES * BLOCK_SIGNALS - ONE_PASS == 712
