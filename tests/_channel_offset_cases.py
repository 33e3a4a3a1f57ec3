"""Shared by the channel-offset tests: a plain-Python restatement of the definition (written from include/fsq_channel_offset.h's
and DESIGN.md 4.31's text, not from the NumPy twin), the votes cases, the peak cases, a generator of two channels with a known
shift, and _colocalize_cases.experiment() with one channel moved.

There is no reference output: the reference stops at one label letter.  The oracle is the plain loops below; the NumPy twin
(_host_channel_offset) is pinned to them on the host, and the kernels to the twin on the GPU."""
import functools
import math

import numpy as np

from _colocalize_cases import BIG, _fuzz_case, _sizes_case, experiment, fuzz_case

MOVED_BY = (3, -4)                                                 # what shifted_experiment() adds to K's positions


# ---- the definition, restated ----

def plain_votes(a_hw, a_field, b_hw, b_field, W):
    """V as a list of lists: V[dh + W][dw + W] = the pairs of one field with a - b = (dh, dw), |dh| <= W and |dw| <= W."""
    V = [[0] * (2 * W + 1) for _ in range(2 * W + 1)]
    for (ah, aw), af in zip(a_hw, a_field):
        for (bh, bw), bf in zip(b_hw, b_field):
            if af != bf:
                continue
            dh, dw = int(ah) - int(bh), int(aw) - int(bw)
            if abs(dh) <= W and abs(dw) <= W:
                V[dh + W][dw + W] += 1
    return V


def plain_score(V, W, tol_sq, oh, ow):
    t = math.isqrt(tol_sq)
    return sum(V[oh + dh + W][ow + dw + W] for dh in range(-t, t + 1) for dw in range(-t, t + 1) if dh * dh + dw * dw <= tol_sq)


def plain_peak(V, R, tol_sq):
    """(record as a list of 16 ints, S as a list of lists) of V (a list of lists, 2W + 1 square)."""
    W, t = len(V) // 2, math.isqrt(tol_sq)
    assert R + t <= W
    S = {(oh, ow): plain_score(V, W, tol_sq, oh, ow) for oh in range(-R, R + 1) for ow in range(-R, R + 1)}
    dh, dw = min(S, key=lambda o: (-S[o], o[0] * o[0] + o[1] * o[1], o[0], o[1]))
    far = [S[o] for o in S if max(abs(o[0] - dh), abs(o[1] - dw)) > 2 * t]
    rec = [dh, dw, S[(dh, dw)], max(far) if far else -1, sum(sum(row) for row in V), int(abs(dh) == R or abs(dw) == R),
           sum(1 for o in S if S[o] == S[(dh, dw)])]
    for h in (dh - 1, dh, dh + 1):
        for w in (dw - 1, dw, dw + 1):
            rec.append(V[h + W][w + W] if abs(h) <= W and abs(w) <= W else 0)
    return rec, [[S[(oh, ow)] for ow in range(-R, R + 1)] for oh in range(-R, R + 1)]


# ---- votes ----

def votes_cases():
    """{name: (a_hw, a_field, b_hw, b_field, W)}: the smallest shapes at which the vote can go wrong.  Small enough for the
    plain loop."""
    far = [(10 + s * 64, 10 + u * 64) for s in (-1, 1) for u in (-1, 1)]
    return {
        "no a": ([], [], [(1, 1), (2, 2), (3, 3)], [0, 0, 1], 2),
        "no b": ([(1, 1), (2, 2)], [0, 1], [], [], 2),
        "nothing": ([], [], [], [], 2),
        "the window's corners": ([(10, 10)], [0], [(7, 7), (7, 13), (13, 7), (13, 13)], [0] * 4, 3),
        # W + 1 in one coordinate only: none of the three votes; the fourth b stands at (3, -3)
        "one past the window": ([(0, 0)], [0], [(-4, 0), (0, 4), (3, -4), (-3, 3)], [0] * 4, 3),
        "W = 0": ([(5, 5), (5, 5), (8, 8)], [0, 0, 0], [(5, 5), (8, 8), (8, 8), (8, 9)], [0, 0, 0, 0], 0),
        "W = 64": ([(10, 10), (300, 300)], [0, 0], far + [(10, 10), (75, 10), (10, -55), (300 - 64, 300 + 64)], [0] * 8, 64),
        "a field in one channel only": ([(0, 0), (9, 9), (0, 0)], [0, 1, 1], [(0, 0), (9, 9), (0, 0)], [1, 2, 2], 2),
        "unsorted fields": ([(0, 0), (0, 0), (1, 1), (2, 2)], [7, 2, 7, 2], [(2, 2), (1, 1), (0, 0), (0, 0)], [2, 7, 2, 7], 2),
        "field sizes": _sizes_case()[:4] + (5,),
        "one bin from two blocks": ([(4, -4)] * 300, [3] * 300, [(4, -4)] * 300, [3] * 300, 1),
        # the correct answer is no vote; a difference taken in int32 wraps to (-2, 2) and votes
        "the coordinate corners": ([(BIG, -BIG)], [0], [(-BIG, BIG)], [0], 2),
        "negative positions": ([(-5, -5), (-9, 4), (3, -7)], [0, 0, 0], [(-6, -5), (-9, 5), (4, -8), (-100, -100)], [0, 0, 0, 0], 2),
        "small fuzz": _fuzz_case(3, 3, 150, side=14)[:4] + (6,),
    }


def votes_fuzz_case():
    """_colocalize_cases.fuzz_case(): 3 300 tracks on a 40 x 40 lattice, every bin of W = 18 hit many times.  (Too many for the
    plain loop: twin and kernel.)"""
    return fuzz_case()[:4] + (18,)


# ---- peaks ----

def histogram(W, bins):
    """V int64 [2W + 1, 2W + 1] with V[dh + W, dw + W] = v for {(dh, dw): v}."""
    V = np.zeros((2 * W + 1, 2 * W + 1), np.int64)
    for (dh, dw), v in bins.items():
        V[dh + W, dw + W] = v
    return V


def peak_cases():
    """{name: (V, R, tol_sq)}."""
    rng = np.random.default_rng(31)
    busy = lambda W: rng.integers(0, 50, (2 * W + 1, 2 * W + 1)).astype(np.int64)        # noqa: E731
    sparse = np.where(rng.random((129, 129)) < 0.02, rng.integers(1, 9, (129, 129)), 0).astype(np.int64)
    sparse[64 + 57, 64 - 60] = 40
    return {
        "all zero": (histogram(4, {}), 3, 1),
        "all zero, no far offset": (histogram(3, {}), 2, 1),
        "equal peaks at (1, 0) and (0, 1)": (histogram(3, {(1, 0): 5, (0, 1): 5}), 2, 0),
        "equal peaks at (-1, 0) and (0, -1)": (histogram(3, {(-1, 0): 5, (0, -1): 5}), 2, 0),
        "equal peaks at (0, 2) and (1, 1)": (histogram(3, {(0, 2): 5, (1, 1): 5}), 2, 0),
        "a peak on the edge": (histogram(2, {(2, -1): 7, (1, -1): 3, (2, 0): 2, (0, 0): 1}), 2, 0),
        "a peak at the corner": (histogram(2, {(-2, 2): 7, (-1, 1): 3, (-2, 1): 2, (1, 1): 4}), 2, 0),
        "tol_sq 0": (busy(6), 3, 0),
        "tol_sq 1": (busy(6), 3, 1),
        "tol_sq 4": (busy(6), 3, 4),
        "tol_sq 6": (busy(6), 3, 6),
        "tol_sq 6 counts 21 taps": (np.ones((11, 11), np.int64), 3, 6),
        # (2, 1) is a tap of tol_sq 6, (2, 2) is not: the one offset scores 5 + 3 of the 12 votes
        "tol_sq 6, (2, 1) in and (2, 2) out": (histogram(6, {(0, 0): 5, (2, 1): 3, (-2, -2): 4}), 0, 6),
        "R = 0": (busy(2), 0, 4),
        "W = R + t": (busy(4), 2, 4),
        "W larger": (busy(6), 2, 4),
        # every offset of the window stands within 2t of a peak at its centre: no runner-up
        "R <= 2t": (histogram(6, {(0, 0): 9}), 4, 4),
        "bins of 2^45": (busy(5) << 45, 3, 4),
        "R = 60, t = 4, W = 64": (sparse, 60, 16),
    }


# ---- two channels with a known shift ----

def shifted_channels(seed, n, fields, side, offset):
    """(a_hw, a_field, b_hw, b_field): n base positions uniform in side^2 over `fields` fields; each channel keeps 85 % of them;
    B is jittered by +-1, gets 10 % spurious tracks, is shifted by -offset - so `offset` is what has to be added to B to land on
    A - and permuted."""
    rng = np.random.default_rng(seed)
    base, field = rng.integers(0, side, (n, 2)), rng.integers(0, fields, n) * 3 + 1
    keep_a, keep_b = rng.random(n) < 0.85, rng.random(n) < 0.85
    b = base[keep_b] + rng.integers(-1, 2, (int(keep_b.sum()), 2))
    extra = len(b) // 10
    b = np.concatenate([b, rng.integers(0, side, (extra, 2))]) - np.array(offset)
    b_field = np.concatenate([field[keep_b], rng.integers(0, fields, extra) * 3 + 1])
    order = rng.permutation(len(b))
    return base[keep_a].astype(np.int64), field[keep_a].astype(np.int64), b[order].astype(np.int64), b_field[order].astype(np.int64)


SHIFT_SIZES = ((600, 3, 100), (200, 2, 64))                        # (n, fields, side)
SHIFT_OFFSETS = ((0, 0), (5, -7), (-9, 12), (-16, 16), (16, -16))
SHIFT_RADII = (math.sqrt(2), 2)


@functools.lru_cache(maxsize=None)
def shifted_experiment(n=240):
    """experiment()'s tables (or those of a smaller one of n molecules) with K's positions moved by MOVED_BY: the offset of K
    is its negative."""
    tables, _ = experiment(n) if n != 240 else experiment()
    tables = dict(tables)
    intensity, words, field, hw, row = tables["K"]
    tables["K"] = (intensity, words, field, hw + np.array(MOVED_BY), row)
    return tables
