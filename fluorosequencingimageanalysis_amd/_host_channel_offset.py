"""NumPy twin of the estimate of the integer offset between two colour channels (include/fsq_channel_offset.h): the votes, the
scores, the peak's record and the centroid that colocalize derives from it - the same integers, without a GPU."""
import math

import numpy as np

from . import _host_colocalize as HC

MAX_W = 64
RECORD = 16
MAX_SEGMENT_B = 1 << 24

NOT_WELL_FORMED = "a_seg or the offsets are not well formed, or a field holds 2^24 or more tracks of the channel to move"


def window(max_shift, tol_sq):
    """(W, R, t) of a search range max_shift and a tolerance tol_sq: t = isqrt(tol_sq), W = R + t.  ValueError for a negative
    one and for max_shift + isqrt(tol_sq) > 64."""
    R, tol_sq = int(max_shift), int(tol_sq)
    if R < 0 or tol_sq < 0:
        raise ValueError("max_shift and tol_sq must not be negative")
    t = math.isqrt(tol_sq)
    if R + t > MAX_W:
        raise ValueError("max_shift=%d + isqrt(tol_sq) = %d exceed the histogram's half-width %d" % (R, t, MAX_W))
    return R + t, R, t


def votes(a_hw, a_seg, a_off, b_hw, b_off, W):
    """fsq_channel_offset_votes with NumPy: V int64 [2W + 1, 2W + 1], V[dh + W, dw + W] = the pairs (a, b) of one segment with
    a - b = (dh, dw).  What the kernel flags raises ValueError."""
    a_hw, b_hw = HC.check_positions(a_hw, "a_hw"), HC.check_positions(b_hw, "b_hw")
    a_off, b_off = (np.asarray(x, np.int64).reshape(-1) for x in (a_off, b_off))
    W = int(W)
    if not 0 <= W <= MAX_W:
        raise ValueError("W must be 0 .. %d" % MAX_W)
    if HC.bad_lanes(a_seg, a_off, b_off, len(a_hw), len(b_hw))[1]:
        raise ValueError(NOT_WELL_FORMED)
    side = 2 * W + 1
    V = np.zeros(side * side, np.int64)
    for s in range(len(a_off) - 1):
        a0, a1, b0, b1 = int(a_off[s]), int(a_off[s + 1]), int(b_off[s]), int(b_off[s + 1])
        if a0 == a1:
            continue
        if b1 - b0 >= MAX_SEGMENT_B:
            raise ValueError(NOT_WELL_FORMED)
        d = a_hw[a0:a1, None, :] - b_hw[None, b0:b1, :]              # (int64: a difference reaches 2^31 - 2)
        inside = (np.abs(d) <= W).all(axis=2)
        d = d[inside]
        V += np.bincount((d[:, 0] + W) * side + d[:, 1] + W, minlength=side * side)
    return V.reshape(side, side)


def taps(tol_sq):
    """The (dh, dw) with dh^2 + dw^2 <= tol_sq."""
    t = math.isqrt(int(tol_sq))
    return [(dh, dw) for dh in range(-t, t + 1) for dw in range(-t, t + 1) if dh * dh + dw * dw <= tol_sq]


def _checked_votes(V, R, tol_sq):
    V = np.asarray(V)
    if V.dtype != np.int64 or V.ndim != 2 or V.shape[0] != V.shape[1] or not V.shape[0] & 1 or V.shape[0] > 2 * MAX_W + 1:
        raise ValueError("votes are int64 [2W + 1, 2W + 1] with W <= %d" % MAX_W)
    W, R, tol_sq = V.shape[0] // 2, int(R), int(tol_sq)
    if R < 0 or tol_sq < 0 or R + math.isqrt(tol_sq) > W:
        raise ValueError("0 <= R, 0 <= tol_sq and R + isqrt(tol_sq) <= W = %d are needed" % W)
    return V, W, R, tol_sq


def scores(V, R, tol_sq):
    """S int64 [2R + 1, 2R + 1]: S[oh + R, ow + R] = the sum of V[o + d] over |d|^2 <= tol_sq."""
    V, W, R, tol_sq = _checked_votes(V, R, tol_sq)
    S = np.zeros((2 * R + 1, 2 * R + 1), np.int64)
    for dh, dw in taps(tol_sq):
        S += V[W - R + dh:W + R + dh + 1, W - R + dw:W + R + dw + 1]
    return S


def peak(V, R, tol_sq):
    """fsq_channel_offset_peak with NumPy: the record int64 [16] (dh, dw, score, runner_up, total, at_edge, n_ties and the
    3 x 3 of V around the peak)."""
    V, W, R, tol_sq = _checked_votes(V, R, tol_sq)
    t = math.isqrt(tol_sq)
    S = scores(V, R, tol_sq)
    oh, ow = np.meshgrid(np.arange(-R, R + 1), np.arange(-R, R + 1), indexing="ij")
    # the largest S, then the smallest (d2, dh, dw): lexsort's last key is the first one compared
    at = np.lexsort((ow.ravel(), oh.ravel(), (oh * oh + ow * ow).ravel(), -S.ravel()))[0]
    dh, dw = int(oh.ravel()[at]), int(ow.ravel()[at])
    best = S[dh + R, dw + R]
    far = np.maximum(np.abs(oh - dh), np.abs(ow - dw)) > 2 * t
    rec = np.zeros(RECORD, np.int64)
    rec[:7] = (dh, dw, best, S[far].max() if far.any() else -1, V.sum(), int(abs(dh) == R or abs(dw) == R), (S == best).sum())
    around = np.zeros((2 * W + 3, 2 * W + 3), np.int64)               # (V with a border of zeros)
    around[1:-1, 1:-1] = V
    rec[7:] = around[dh + W:dh + W + 3, dw + W:dw + W + 3].ravel()
    return rec


def centroid(record):
    """(h, w) float64: the peak plus the mean displacement of the 3 x 3 of V around it, or the peak itself when those bins are
    empty.  Integers up to one division per coordinate: the host and device routes agree bit for bit."""
    rec = [int(x) for x in np.asarray(record).reshape(-1)]
    dh, dw, v = rec[0], rec[1], rec[7:16]
    n = sum(v)
    if n == 0:
        return (float(dh), float(dw))
    mh = sum((k // 3 - 1) * x for k, x in enumerate(v))
    mw = sum((k % 3 - 1) * x for k, x in enumerate(v))
    return (dh + mh / n, dw + mw / n)


def estimate_of(record, V):
    """The dict that colocalize's estimate_* functions return, of a record and its votes."""
    rec = [int(x) for x in np.asarray(record).reshape(-1)]
    return {"offset": (rec[0], rec[1]), "score": rec[2], "runner_up": rec[3], "total": rec[4], "at_edge": bool(rec[5]),
            "n_ties": rec[6], "centroid": centroid(rec), "votes": V}
