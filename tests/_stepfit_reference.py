"""NumPy restatement of the step-fit path (Trace.stepfit_photometries of the reference), written from the specification in
DESIGN.md section 4.10 for tests on machines without the reference.

The plateau boundaries, heights and CK-filtered values follow the reference's arithmetic (np.mean, Python sums, pow), so
they are compared bit for bit; p-values come from scipy.special.stdtr.  `near` flags a trace whose decisions are not
well defined under a 1e-10 p tolerance (a p within 1e-8 of the threshold, or two sorted p within 1e-8 of each other)."""
import math

import numpy as np
from scipy.special import stdtr

REL = 1e-8


class Flags:
    def __init__(self):
        self.near = False
        self.unsupported = False
        self.p_slide = []      # (radius index, frame, p)
        self.p_pairs = []      # p of every t-filter pair test, in order


def _near(a, b):
    return np.isfinite(a) and np.isfinite(b) and abs(a - b) <= REL * max(abs(a), abs(b))


def welch_p(a, b):
    """scipy.stats.ttest_ind(a, b, equal_var=False).pvalue."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    n1, n2 = len(a), len(b)
    if n1 == 0 or n2 == 0:
        return math.nan
    with np.errstate(all="ignore"):
        m1, m2 = np.mean(a), np.mean(b)
        v1 = np.mean((a - m1) ** 2) * np.divide(n1, n1 - 1)
        v2 = np.mean((b - m2) ** 2) * np.divide(n2, n2 - 1)
        vn1, vn2 = v1 / np.float64(n1), v2 / np.float64(n2)
        df = (vn1 + vn2) ** 2 / (vn1 ** 2 / np.float64(n1 - 1) + vn2 ** 2 / np.float64(n2 - 1))
        if np.isnan(df):
            df = np.float64(1.0)
        t = (m1 - m2) / np.sqrt(vn1 + vn2)
        if np.isnan(t):
            return math.nan
        return float(2.0 * stdtr(df, -abs(t)))


def cpython_sort_desc(keys):
    """Indices of keys in the order of CPython's sorted(range(n), key=keys.__getitem__, reverse=True), for n < 64:
    reverse, count_run, binary insertion sort with `<`, reverse."""
    n = len(keys)
    idx = list(range(n))[::-1]
    if n >= 2:
        run = 2
        if keys[idx[1]] < keys[idx[0]]:
            while run < n and keys[idx[run]] < keys[idx[run - 1]]:
                run += 1
            idx[:run] = idx[:run][::-1]
        else:
            while run < n and not (keys[idx[run]] < keys[idx[run - 1]]):
                run += 1
        for st in range(run, n):
            pv = idx[st]
            lo, hi = 0, st
            while True:
                p = lo + ((hi - lo) >> 1)
                if keys[pv] < keys[idx[p]]:
                    hi = p
                else:
                    lo = p + 1
                if not lo < hi:
                    break
            idx[lo + 1:st + 1] = idx[lo:st]
            idx[lo] = pv
    return idx[::-1]


def ck_filter(lum, window_lengths=(2, 4, 8, 16), M=10):
    """chung_kennedy_filter with p = 2 (weights pow(x, -2.0) through Python floats: glibc's pow)."""
    lum = [float(v) for v in lum]
    n = len(lum)
    if not n > 2:
        raise ValueError("luminosities must have len(luminosities) > 2")
    arr = np.asarray(lum, dtype=np.float64)
    fp, bp = {}, {}
    for w in window_lengths:
        fp[w] = [None] + [np.mean(arr[max(L - w - 1, 0):L]) for L in range(1, n)]
        bp[w] = [np.mean(arr[L + 1:L + w + 1]) for L in range(n - 1)] + [None]
    out = []
    for L in range(n):
        fws, bws = [], []
        for w in window_lengths:
            if L == 0:
                fw, bw = 0, 1
            elif L == n - 1:
                fw, bw = 1, 0
            else:
                r0 = max(L - M + 1, 1)
                fe = min(L + M, n) - (1 if L + M >= n - 1 else 0)
                bd = 0
                for j in range(r0, L + 1):
                    d = lum[j] - float(fp[w][j])
                    bd = bd + d * d
                fd = 0
                for j in range(L, fe):
                    d = lum[j] - float(bp[w][j])
                    fd = fd + d * d
                if bd != 0 and fd != 0:
                    fw, bw = bd ** -2, fd ** -2
                elif bd == 0 and fd != 0:
                    fw, bw = 1, 0
                elif bd != 0 and fd == 0:
                    fw, bw = 0, 1
                else:
                    fw, bw = 1, 0
            fws.append(fw)
            bws.append(bw)
        tot = sum(fws) + sum(bws)
        s = 0
        for k, w in enumerate(window_lengths):
            if L == 0:
                s = s + (float(bws[k]) / tot) * float(bp[w][L])
            elif L == n - 1:
                s = s + (float(fws[k]) / tot) * float(fp[w][L])
            else:
                s = s + ((float(fws[k]) / tot) * float(fp[w][L]) + (float(bws[k]) / tot) * float(bp[w][L]))
        out.append(float(s))
    return out


def sliding_steps(seq, window_radius, p_threshold, flags):
    seq = np.asarray(seq, dtype=np.float64)
    n = len(seq)
    radii = list(range(5, window_radius))
    steps = []
    for f in range(n):
        ok = len(radii) > 0
        for k, r in enumerate(radii):
            p = welch_p(seq[f - r:f] if f - r >= -n else seq[0:f], seq[f:f + r])
            flags.p_slide.append((k, f, p))
            if _near(p, p_threshold):
                flags.near = True
            ok = ok and (p < p_threshold)
        if ok:
            steps.append(f)
    kept = [f for f in steps if f + 1 not in set(steps)]
    return kept


def plateaus_from_steps(steps, n, lum):
    lum = np.asarray(lum, dtype=np.float64)
    bounds = [0] + list(steps) + [n]
    return [(bounds[i], bounds[i + 1] - 1, np.mean(lum[bounds[i]:bounds[i + 1]])) for i in range(len(bounds) - 1)]


def t_test_filter(lum, plateaus, p_threshold, drop_sort=True, no_merge_start=0, flags=None, tie_reverse=False):
    """tie_reverse=True is NOT the reference's order: equal p are visited last pair first (the order an unstable sort could
    give).  The limit tests use it to prove that a case with tied p depends on the tie order."""
    flags = flags or Flags()
    lum = np.asarray(lum, dtype=np.float64)
    pl = list(plateaus)

    def merged(a, b):
        return (a[0], b[1], np.mean(lum[a[0]:b[1] + 1]))

    for _ in range(len(plateaus) - 1):
        if len(pl) < 2:
            break
        out = []
        any_merge = False
        if drop_sort:
            ps = []
            for r in range(len(pl) - 1):
                p = welch_p(lum[pl[r][0]:pl[r][1] + 1], lum[pl[r + 1][0]:pl[r + 1][1] + 1])
                flags.p_pairs.append(p)
                if _near(p, p_threshold):
                    flags.near = True
                ps.append(p)
            if any(math.isnan(p) for p in ps) and len(ps) >= 64:
                flags.unsupported = True
                return None
            order = cpython_sort_desc(ps) if any(math.isnan(p) for p in ps) else sorted(range(len(ps)), key=ps.__getitem__, reverse=True)
            if tie_reverse and not any(math.isnan(p) for p in ps):
                order = sorted(range(len(ps)), key=lambda r: (ps[r], r), reverse=True)
            fin = sorted(p for p in ps if np.isfinite(p))
            if any(_near(fin[i], fin[i + 1]) and fin[i] != fin[i + 1] for i in range(len(fin) - 1)):
                flags.near = True
            mark = [ps[r] >= p_threshold and pl[r][1] >= no_merge_start for r in range(len(ps))]
            done = [False] * len(ps)
            for r in order:
                done[r] = True
                if mark[r]:
                    for q in (r - 1, r + 1):
                        if 0 <= q < len(ps) and not done[q]:
                            mark[q] = False
            r = 0
            while r < len(pl):
                if r < len(ps) and mark[r]:
                    out.append(merged(pl[r], pl[r + 1]))
                    any_merge = True
                    r += 2
                else:
                    out.append(pl[r])
                    r += 1
        else:
            r = 0
            while r < len(pl):
                merge = False
                if r + 1 < len(pl) and pl[r][1] >= no_merge_start:
                    p = welch_p(lum[pl[r][0]:pl[r][1] + 1], lum[pl[r + 1][0]:pl[r + 1][1] + 1])
                    flags.p_pairs.append(p)
                    if _near(p, p_threshold):
                        flags.near = True
                    merge = p >= p_threshold
                if merge:
                    out.append(merged(pl[r], pl[r + 1]))
                    any_merge = True
                    r += 2
                else:
                    out.append(pl[r])
                    r += 1
        pl = out
        if not any_merge:
            break
    return pl


def unmirror_plateaus(plateaus, m):
    out = []
    for a, o, h in plateaus:
        a, o = a - m, o - m
        if o < 0:
            continue
        out.append((max(a, 0), o, h))
    return out


def stepfit(photometries, mirror_start=0, chung_kennedy=0, p_threshold=0.01, photometry_min=None, window_radius=6,
            drop_sort=True, window_lengths=(2, 4, 8, 16), M=10):
    """Returns (photometries, ck_filtered, plateaus, t_filtered_plateaus, flags) for one trace (unmirrored lists)."""
    ph = [0.0 if v is None else float(v) for v in photometries]
    if photometry_min is not None:
        ph = [max(photometry_min, v) for v in ph]
    elif any(math.isnan(v) for v in ph):
        raise ValueError("NaN photometry without photometry_min")
    m = mirror_start
    mir = [x for x in reversed(ph[:m])] + list(ph)
    flags = Flags()
    ck = ck_filter(mir, window_lengths=window_lengths, M=M) if chung_kennedy > 0 else mir
    steps = sliding_steps(ck, window_radius, p_threshold, flags)
    pl = plateaus_from_steps(steps, len(mir), mir)
    tf = t_test_filter(mir, pl, p_threshold, drop_sort=drop_sort, no_merge_start=m, flags=flags)
    if tf is None:
        return ph, ck[m:], unmirror_plateaus(pl, m), None, flags
    return ph, ck[m:], unmirror_plateaus(pl, m), unmirror_plateaus(tf, m), flags
