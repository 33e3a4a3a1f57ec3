"""Plain-numpy restatement of the remainder correction (include/fsq_remainder.h; MCsimlib._remainder_adjust_2 :3434-3472 and
_remainder_adjust :3398-3431).  Medians are taken from a full sort, so nothing here shares code with the library's host route
(np.median) or with the kernels (rank counting and a radix select)."""
import numpy as np

RATIO, ADDITIVE = "ratio", "additive"


def median(values):
    """np.median of a 1-D array: NaN for none or with a NaN among them, else the middle of the sorted values or the mean of
    the two middle ones.  np.mean adds the first value to the sum of the others, and that sum starts from +0.0: a median of
    -0.0 comes out as +0.0 (and so the order of -0.0 and +0.0 in the sort never shows)."""
    a = np.sort(np.asarray(values, dtype=np.float64))              # (NaN sorts last)
    n = len(a)
    if n == 0 or np.isnan(a[-1]):
        return np.float64(np.nan)
    with np.errstate(all="ignore"):
        zero = np.float64(0.0)
        return a[n // 2] + zero if n % 2 else (a[n // 2 - 1] + (zero + a[n // 2])) / np.float64(2.0)


def is_remainder(word, F):
    return (int(word) & ((1 << F) - 1)) == (1 << F) - 1


def adjust_arrays(rows, cats, seg_off, mode=RATIO, minimum=5):
    """rows float64 [n, F], cats [n] category words, seg_off [S + 1] -> the dict fsq_remainder_adjust fills."""
    rows = np.asarray(rows, dtype=np.float64)
    n, F = rows.shape
    S = len(seg_off) - 1
    adjusted, adjustment = np.zeros((n, F)), np.full((S, F), np.nan)
    n_remainders, kept = np.zeros(S, np.int32), np.zeros(S, np.uint8)
    with np.errstate(all="ignore"):
        for s in range(S):
            a, b = int(seg_off[s]), int(seg_off[s + 1])
            values = [[] for _ in range(F)]
            for t in range(a, b):
                if not is_remainder(cats[t], F):
                    continue
                m = median(rows[t])
                for f in range(F):
                    values[f].append((rows[t, f] - m) / m if mode == RATIO else rows[t, f])
            R = len(values[0])
            med = np.array([median(v) for v in values])
            adjustment[s] = med if mode == RATIO else med - med[0]
            n_remainders[s] = R
            kept[s] = 1 if (R >= minimum and (mode == RATIO or R >= 1)) else 0
            if kept[s]:
                for t in range(a, b):
                    adjusted[t] = rows[t] * (1.0 - adjustment[s]) if mode == RATIO else rows[t] - adjustment[s]
    return {"adjusted": adjusted, "adjustment": adjustment, "n_remainders": n_remainders, "kept": kept}


def adjust_records(rows, cats, segments, mode=RATIO, minimum=5):
    """adjust_arrays for one segment id per track in any order: `adjusted` in the caller's order, the rest per ascending id."""
    rows, cats, ids = np.asarray(rows, dtype=np.float64), np.asarray(cats), np.asarray(segments).reshape(-1)
    order = np.argsort(ids, kind="stable")
    unique, counts = np.unique(ids, return_counts=True)
    seg_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    out = adjust_arrays(rows[order], cats[order], seg_off, mode, minimum)
    adjusted = np.empty_like(out["adjusted"])
    adjusted[order] = out["adjusted"]
    out["adjusted"], out["segment_ids"] = adjusted, unique
    return out


def adjust_dict(photometries, num_frames, minimum=5, mode=RATIO):
    """(adjusted_photometries, medians) of the nested dict, as the two MCsimlib functions return them."""
    F = num_frames
    adjusted, medians = {}, {}
    for channel, cdict in photometries.items():
        for field, fdict in cdict.items():
            tracks = list(fdict.items())
            rows = np.array([t[1][1] for t in tracks], dtype=np.float64).reshape(len(tracks), F)
            cats = [sum(1 << f for f, c in enumerate(t[1][0]) if c) for t in tracks]
            out = adjust_arrays(rows, cats, [0, len(tracks)], mode, minimum)
            if not out["kept"][0]:
                continue
            medians.setdefault(channel, {})[field] = list(out["adjustment"][0])
            fd = adjusted.setdefault(channel, {}).setdefault(field, {})
            for i, (hw, (category, _, row)) in enumerate(tracks):
                fd[hw] = (category, list(out["adjusted"][i]), row)
    return adjusted, medians
