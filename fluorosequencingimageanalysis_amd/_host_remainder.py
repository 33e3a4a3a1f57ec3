"""The remainder correction with numpy on the host: what fsq_remainder_adjust (include/fsq_remainder.h) computes, the
`device=None` route of remainder.py."""
import numpy as np

from ._native_remainder import MODE_RATIO


def _median(values):
    """np.median of a 1-D float64 array, NaN for an empty one (numpy warns and gives NaN)."""
    return np.float64(np.nan) if len(values) == 0 else np.median(values)


def adjust(rows, cats, seg_off, mode, minimum):
    """rows float64 [n, F], cats uint64 [n], seg_off int64 [S + 1] -> the dict of remainder.remainder_adjust_device, as arrays."""
    n, F = rows.shape
    S = len(seg_off) - 1
    all_on = np.uint64((1 << F) - 1)
    remainder = (cats & all_on) == all_on
    adjusted, adjustment = np.zeros((n, F)), np.empty((S, F))
    n_remainders, kept = np.zeros(S, np.int32), np.zeros(S, np.uint8)
    with np.errstate(all='ignore'):
        for s in range(S):
            a, b = int(seg_off[s]), int(seg_off[s + 1])
            block = rows[a:b]
            rem = block[remainder[a:b]]
            R = len(rem)
            if mode == MODE_RATIO:
                m = np.median(rem, axis=1)[:, None] if R else np.zeros((0, 1))
                values = (rem - m) / m
            else:
                values = rem
            med = np.array([_median(values[:, f]) for f in range(F)])
            adjustment[s] = med if mode == MODE_RATIO else med - med[0]
            n_remainders[s] = R
            kept[s] = R >= minimum and (mode == MODE_RATIO or R >= 1)
            if kept[s]:
                adjusted[a:b] = block * (1.0 - adjustment[s]) if mode == MODE_RATIO else block - adjustment[s]
    return {"adjusted": adjusted, "adjustment": adjustment, "n_remainders": n_remainders, "kept": kept}
