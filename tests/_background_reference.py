"""Restatement of MCsimlib.iterative_peak_finding_v3 (:5932-6019) for the tests, written from the reference's rules and not
from the package's host twin: keys become rows of arrays once, `max` is a sequential scan with `>`, every total is a
sequential sum (np.cumsum along a row adds left to right), pow is libm's.  Dicts are walked in insertion order.

`iterate` is the array form (seconds at 1 100 keys).  `iterate_dicts` is the shape of the reference's loop: one dict copy, one
renormalisation and one z-score table per trial; it is what tools/bench_background.py times as the reference-shaped loop, and
the tests hold the two against each other at small sizes."""
import itertools
import math

import numpy as np

STOP_NO_DEFINED, STOP_THRESHOLD, STOP_NO_IMPROVEMENT, STOP_CONVERGED, STOP_MAX_ITERATIONS = 1, 2, 3, 4, 5


def py2_round(x):
    return math.floor(x + 0.5) if x >= 0 else math.ceil(x - 0.5)


def seq_sum(values):
    total = 0
    for v in values:
        total = total + v
    return total


def scan_max(values):
    """Index of Python's max over a sequence: replaced only by a strictly greater value."""
    best = 0
    for i in range(1, len(values)):
        if values[i] > values[best]:
            best = i
    return best


def z_of(bp, ap, sp):
    d = bp - ap
    try:
        m = math.pow(float(d), 2.0) / math.pow(float(sp), 2.0)
    except OverflowError:
        m = math.inf
    return math.copysign(math.sqrt(m), d) if m == m else math.nan


def passes_filter(key, num_cycles, include_multidrop):
    pos = [p for _, p in key[0]]
    return bool(key[1]) and (include_multidrop or len(set(pos)) == len(pos)) and max(pos) <= num_cycles


def neighbours(key, num_cycles, include_multidrop):
    """The keys interpolate_signal reads for `key`, in order."""
    letter = key[0][0][0]
    pos = [p for _, p in key[0]]
    out = []
    for e in itertools.product((-1, 0, 1), repeat=len(pos)):
        if not any(e):
            continue
        q = [p + s for p, s in zip(pos, e)]
        if not include_multidrop and len(set(q)) < len(q):
            continue
        if all(0 < p <= num_cycles for p in q):
            out.append((tuple((letter, p) for p in q), key[1], key[2]))
    return out


def np_mean(values):
    with np.errstate(all='ignore'):
        return np.float64(np.nan) if len(values) == 0 else np.mean(np.asarray(values, dtype=np.float64))


def iterate(boc_raw, boc_percent, ac_average, ac_std, num_cycles, sigma_threshold=3, include_multidrop=False, max_iterations=None):
    """-> dict: keys (in order), counts (float), updated_boc_raw, updated_boc_percent, undefined_peaks, stop, passes, accepted
    (the key of every accepting pass)."""
    keys = list(boc_raw.keys())
    row = {k: i for i, k in enumerate(keys)}
    und_ac = [k for k in ac_average if ac_std[k] == 0]
    for k in und_ac:                                                # (all of them are written in the first pass, in this order)
        if k not in row:
            row[k] = len(keys)
            keys.append(k)
    n = len(keys)
    count = np.zeros(n)
    for k, v in boc_raw.items():
        count[row[k]] = v
    percent = np.zeros(n)
    for k, v in boc_percent.items():
        percent[row[k]] = v
    keep = np.array([passes_filter(k, num_cycles, include_multidrop) for k in keys], dtype=bool)
    kept = np.flatnonzero(keep)
    where = np.full(n, -1)
    where[kept] = np.arange(len(kept))
    nb = [np.array([row.get(q, -1) for q in neighbours(k, num_cycles, include_multidrop)], dtype=np.int64) for k in keys]
    defined = [k for k in ac_average if ac_std[k] != 0]
    d_row = np.array([row.get(k, -1) for k in defined], dtype=np.int64)
    d_ap = [float(ac_average[k]) for k in defined]
    d_sp = [float(ac_std[k]) for k in defined]

    def interpolated(r):
        return np_mean([count[j] if j >= 0 else 0.0 for j in nb[r]])

    undefined_peaks, accepted = [], []
    passes, prior, stop = 0, None, None
    with np.errstate(all='ignore'):
        while True:
            if max_iterations is not None and passes >= max_iterations:
                stop = STOP_MAX_ITERATIONS
                break
            passes += 1
            z = [z_of(percent[r] if r >= 0 else 0, a, s) for r, a, s in zip(d_row, d_ap, d_sp)]
            order = und_ac + ([k for k in boc_percent if k not in ac_average] if passes == 1 else
                              [keys[r] for r in kept if keys[r] not in ac_average])
            for k in order:
                r = row[k]
                undefined_peaks.append((k[0], k[1], k[2], boc_percent.get(k, 0) if passes == 1 else percent[r], ac_average.get(k, 0),
                                        ac_std.get(k, 0)))
                count[r] = interpolated(r)
            sums = np.cumsum(np.concatenate([[0.0], count[kept]]))
            total = sums[-1]
            if len(kept) and total == 0:
                raise ZeroDivisionError("float division by zero")
            percent = np.where(keep, count / total, 0.0)
            if not z:
                stop = STOP_NO_DEFINED
                break
            if z[scan_max(z)] <= sigma_threshold:
                stop = STOP_THRESHOLD
                break
            trials = [i for i in range(len(z)) if not z[i] <= sigma_threshold]
            assert all(d_row[i] >= 0 for i in trials), "a key that boc lacks would be chosen"
            rows = d_row[trials]
            values = np.array([interpolated(r) for r in rows])
            totals = np.full(len(trials), total)
            inside = np.flatnonzero(keep[rows])
            for a in range(0, len(inside), 256):
                part = inside[a:a + 256]
                table = np.tile(np.concatenate([[0.0], count[kept]]), (len(part), 1))
                table[np.arange(len(part)), where[rows[part]] + 1] = values[part]
                totals[part] = np.cumsum(table, axis=1)[:, -1]
            if (totals[inside] == 0).any():
                raise ZeroDivisionError("float division by zero")
            diffs = [z[i] - z_of(values[t] / totals[t] if keep[d_row[i]] else 0, d_ap[i], d_sp[i]) for t, i in enumerate(trials)]
            b = scan_max(diffs)
            if diffs[b] <= 0:
                stop = STOP_NO_IMPROVEMENT
                break
            count[rows[b]] = values[b]
            accepted.append(keys[rows[b]])
            if prior is not None:
                changes = list(np.abs(count - prior))
                if changes[scan_max(changes)] < 0.001:
                    stop = STOP_CONVERGED
                    break
            prior = count.copy()
            percent = np.where(keep, count / seq_sum(count[kept]), 0.0)
    rounded = None
    if not np.isnan(count).any():
        rounded = {k: int(py2_round(c)) for k, c in zip(keys, count)}
    return dict(keys=keys, counts=count, updated_boc_raw=rounded,
                updated_boc_percent={k: float(percent[i]) for i, k in enumerate(keys) if keep[i]},
                undefined_peaks=undefined_peaks, stop=stop, passes=passes, accepted=accepted)


# ---- the reference-shaped loop ----

def percent_of(signals, num_cycles, include_multidrop):
    kept = {k: c for k, c in signals.items() if passes_filter(k, num_cycles, include_multidrop)}
    total = seq_sum(kept.values())
    return {k: float(c) / total for k, c in kept.items()}


def z_table(boc, ac_average, ac_std):
    z, und = {}, {}
    for k in list(ac_average) + list(boc):
        bp, ap, sp = boc.get(k, 0), ac_average.get(k, 0), ac_std.get(k, 0)
        if sp == 0:
            und.setdefault(k, (bp, ap, sp))
        else:
            z.setdefault(k, z_of(bp, ap, sp))
    return z, und


def dict_max(d):
    ks = list(d)
    return ks[scan_max([d[k] for k in ks])]


def iterate_dicts(boc_raw, boc_percent, ac_average, ac_std, num_cycles, sigma_threshold=3, include_multidrop=False):
    """The same result as `iterate`, with the cost of the reference: per trial one dict copy, one renormalisation of all
    keys and one z-score table."""
    def interpolated(raw, k):
        return np_mean([raw.get(q, 0) for q in neighbours(k, num_cycles, include_multidrop)])
    raw, percent = dict(boc_raw), dict(boc_percent)
    undefined_peaks, accepted, prior, passes = [], [], None, 0
    while True:
        passes += 1
        z, und = z_table(percent, ac_average, ac_std)
        for k, (bp, ap, sp) in und.items():
            raw[k] = interpolated(raw, k)
            undefined_peaks.append((k[0], k[1], k[2], bp, ap, sp))
        percent = percent_of(raw, num_cycles, include_multidrop)
        if not z:
            stop = STOP_NO_DEFINED
            break
        if z[dict_max(z)] <= sigma_threshold:
            stop = STOP_THRESHOLD
            break
        values = {k: interpolated(raw, k) for k in z}
        diffs = {}
        for k, v in values.items():
            if z[k] <= sigma_threshold:
                continue
            trial = dict(raw)
            trial[k] = v
            tz, _ = z_table(percent_of(trial, num_cycles, include_multidrop), ac_average, ac_std)
            diffs[k] = z[k] - tz[k]
        best = dict_max(diffs)
        if diffs[best] <= 0:
            stop = STOP_NO_IMPROVEMENT
            break
        raw[best] = values[best]
        accepted.append(best)
        if prior is not None:
            changes = [abs(raw[k] - prior[k]) for k in prior]
            if changes[scan_max(changes)] < 0.001:
                stop = STOP_CONVERGED
                break
        prior = dict(raw)
        percent = percent_of(raw, num_cycles, include_multidrop)
    return dict(keys=list(raw), counts=np.array([float(v) for v in raw.values()]),
                updated_boc_raw={k: int(py2_round(c)) for k, c in raw.items()}, updated_boc_percent=percent,
                undefined_peaks=undefined_peaks, stop=stop, passes=passes, accepted=accepted)
