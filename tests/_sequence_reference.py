"""NumPy restatement of what fsq_sequence_photometry / fsq_sequence_category_counts write (include/fsq_sequence.h): the
closed form of SequenceExperiment.fill_in_trace + interpolate_spots (flexlibrary.py:1842-2032), Spot.valid_slice, the two
photometry metrics and the categories.  Plain Python floats: every operation is one fp64 rounding, as on the device."""
import math

import numpy as np

DETECTED, INTERPOLATED, WINDOW_INSIDE = 1, 2, 4
COORD_LIMIT = 1 << 29


def _round_half_away(x):
    # exact: floor / ceil of x itself, then one comparison of the exact remainder (x - floor(x) is exact for |x| < 2^52)
    if not math.isfinite(x) or abs(x) >= 2.0 ** 52:
        return x
    f = math.floor(x)
    d = x - f
    if x >= 0:
        return float(f + 1) if d >= 0.5 else float(f)
    return float(f + 1) if d > 0.5 else float(f)


def accumulate(offsets):
    """Experiment.accumulate_offsets: Python's sum, left to right from 0, for every frame."""
    cum, ah, aw = [], 0.0, 0.0
    for o in offsets:
        ah = ah + float(o[0])
        aw = aw + float(o[1])
        cum.append((ah, aw))
    return cum


def fill_positions(hw, cum, H, W, spot_size, interpolate):
    """One trace: hw int [F, 2] ((-1, -1) = no Spot) -> (positions [(h, w) or None] * F, detected [bool] * F)."""
    F = len(hw)
    det = [bool(hw[f][0] >= 0 and hw[f][1] >= 0) for f in range(F)]
    r = (spot_size - 1) // 2
    out = []
    for i in range(F):
        if det[i]:
            out.append((int(hw[i][0]), int(hw[i][1])))
            continue
        if not interpolate or not any(det):
            out.append(None)
            continue
        before = [f for f in range(i) if det[f]]
        after = [f for f in range(i + 1, F) if det[f]]
        a = before[-1] if before else 0
        b = after[0] if after else F - 1
        p = []
        for c in (0, 1):
            if after:
                stop = float(hw[b][c]) + (cum[a][c] - cum[b][c])
            if before:
                start = float(hw[a][c])
            else:
                start = stop
            if not after:
                stop = start
            inc = (stop - start) / float(b - a)
            v = start + inc * float(i - a)
            v = v + (cum[i][c] - cum[a][c])
            p.append(_round_half_away(v))
        if all(-COORD_LIMIT < v < COORD_LIMIT for v in p) and r <= p[0] < H - r and r <= p[1] < W - r:
            out.append((int(p[0]), int(p[1])))
        else:
            out.append(None)
    return out, det


def window(img, h, w, radius):
    """Spot.image_slice: the (2 radius + 1)^2 window clipped at the borders."""
    H, W = img.shape
    return img[max(0, h - radius):max(0, min(H, h + radius + 1)), max(0, w - radius):max(0, min(W, w + radius + 1))]


def mexican_hat(img, h, w, brim, radius):
    """Spot.mexican_hat_photometry_metric (flexlibrary.py:172-210) on int64 pixels."""
    sl = window(img, h, w, radius).astype(np.int64)
    d = 2 * radius + 1
    hh, ww = np.meshgrid(np.arange(sl.shape[0]), np.arange(sl.shape[1]), indexing="ij")
    crown = (brim <= hh) & (hh < d - brim) & (brim <= ww) & (ww < d - brim)
    brim_px = sl[~crown]
    med = float(np.median(brim_px)) if brim_px.size else math.nan
    return float(int(sl[crown].sum())) - float(int(crown.sum())) * med


def simple(img, h, w, spot_size):
    return float(int(window(img, h, w, (spot_size - 1) // 2).astype(np.int64).sum()))


def records(frames, trace_hw, trace_seq, offsets, method="mexican_hat", radius=9, brim_size=6, spot_size=5, interpolate=True):
    """The outputs of sequencing.sequence_photometry_records (without `counts`), computed with NumPy."""
    frames = np.asarray(frames)
    n_seq, F, H, W = frames.shape
    hw_in = np.asarray(trace_hw).reshape(-1, F, 2)
    n = len(hw_in)
    cums = [accumulate(offsets[s]) for s in range(n_seq)]
    hw = np.full((n, F, 2), -1, np.int32)
    phot = np.full((n, F), np.nan)
    flags = np.zeros((n, F), np.uint8)
    category = np.zeros(n, np.uint64)
    valid = np.zeros(n, bool)
    wr = radius if method == "mexican_hat" else (spot_size - 1) // 2
    for t in range(n):
        s = int(trace_seq[t])
        pos, det = fill_positions(hw_in[t], cums[s], H, W, spot_size, interpolate)
        cat, ok = 0, True
        for f in range(F):
            if det[f]:
                cat |= 1 << f
            if pos[f] is None:
                ok = False
                continue
            h, w = pos[f]
            hw[t, f] = (h, w)
            inside = h - wr >= 0 and h + wr < H and w - wr >= 0 and w + wr < W
            ok = ok and inside
            flags[t, f] = (DETECTED if det[f] else INTERPOLATED) | (WINDOW_INSIDE if inside else 0)
            img = frames[s, f]
            phot[t, f] = mexican_hat(img, h, w, brim_size, radius) if method == "mexican_hat" else simple(img, h, w, spot_size)
        category[t] = cat
        valid[t] = ok
    return {"hw": hw, "photometry": phot, "flags": flags, "category": category, "trace_valid": valid}


def category_counts(category, trace_seq, select=None):
    """(seq, pattern, count, first) per group in order of first appearance."""
    groups = {}
    for i, (c, s) in enumerate(zip(np.asarray(category).tolist(), np.asarray(trace_seq).tolist())):
        if select is not None and not select[i]:
            continue
        g = groups.setdefault((int(s), int(c)), [0, i])
        g[0] += 1
    keys = list(groups)
    return {"seq": np.array([k[0] for k in keys], np.int32), "pattern": np.array([k[1] for k in keys], np.uint64),
            "count": np.array([groups[k][0] for k in keys], np.int32), "first": np.array([groups[k][1] for k in keys], np.int32)}


def category_counts_unique(category, trace_seq, select=None):
    """category_counts for millions of traces: the same groups, counts and first (= smallest) indices from one stable sort,
    in order of first appearance."""
    cat = np.asarray(category, dtype=np.uint64).reshape(-1)
    seq = np.asarray(trace_seq).reshape(-1).astype(np.int64)
    idx = np.arange(len(cat)) if select is None else np.flatnonzero(np.asarray(select).reshape(-1))
    c, s = cat[idx], seq[idx]
    o = np.lexsort((c, s))                                          # stable: equal keys stay in index order
    cs, ss = c[o], s[o]
    new = np.ones(len(o), bool)
    new[1:] = (cs[1:] != cs[:-1]) | (ss[1:] != ss[:-1])
    starts = np.flatnonzero(new)
    first = idx[o[starts]]
    count = np.diff(np.append(starts, len(o)))
    order = np.argsort(first, kind="stable")
    return {"seq": ss[starts][order].astype(np.int32), "pattern": cs[starts][order].astype(np.uint64),
            "count": count[order].astype(np.int32), "first": first[order].astype(np.int32)}
