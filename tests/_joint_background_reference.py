"""Restatement of MCsimlib.iterative_peak_finding_v3 (:5932-6019) for joint signals (decrements, zeros, starts) of several label
letters, written from the package's four rules for them and not from its host twin, in the shape of the reference's loop: plain
dicts, per trial one copy, one renormalisation and one z-score table.  Dicts are walked in insertion order.

The rules: a key is a remainder when not all(zeros); it is multidrop when a cycle repeats, whatever the letters; it passes the
filter when all(zeros), multidrop is included or it is not multidrop, and its largest cycle is <= num_cycles; its neighbours are
its own tuple with the cycles perturbed by itertools.product((-1, 0, 1), repeat=d) without the all-zero one, kept when every
0 < cycle <= num_cycles and (multidrop excluded) all cycles differ, and looked up as they stand."""
import itertools

import _background_reference as R


def is_remainder(key):
    return not all(key[1])


def is_multidrop(key):
    cycles = [c for _, c in key[0]]
    return len(set(cycles)) < len(cycles)


def passes_filter(key, num_cycles, include_multidrop):
    return (not is_remainder(key)) and (include_multidrop or not is_multidrop(key)) and max(c for _, c in key[0]) <= num_cycles


def neighbours(key, num_cycles, include_multidrop):
    out = []
    for e in itertools.product((-1, 0, 1), repeat=len(key[0])):
        if all(x == 0 for x in e):
            continue
        cand = tuple((letter, c + x) for (letter, c), x in zip(key[0], e))
        if not all(0 < c <= num_cycles for _, c in cand):
            continue
        if not include_multidrop and len(set(c for _, c in cand)) < len(cand):
            continue
        out.append((cand, key[1], key[2]))
    return out


def percent_of(signals, num_cycles, include_multidrop):
    kept = {k: c for k, c in signals.items() if passes_filter(k, num_cycles, include_multidrop)}
    total = R.seq_sum(kept.values())
    return {k: float(c) / total for k, c in kept.items()}


def iterate(boc_raw, boc_percent, ac_average, ac_std, num_cycles, sigma_threshold=3, include_multidrop=False, max_iterations=None):
    """-> dict: keys (in order), counts, updated_boc_raw, updated_boc_percent, undefined_peaks, stop, passes, accepted."""
    def interpolated(raw, k):
        return R.np_mean([raw.get(q, 0) for q in neighbours(k, num_cycles, include_multidrop)])
    raw, percent = dict(boc_raw), dict(boc_percent)
    undefined_peaks, accepted, prior, passes = [], [], None, 0
    while True:
        if max_iterations is not None and passes >= max_iterations:
            stop = R.STOP_MAX_ITERATIONS
            break
        passes += 1
        z, und = R.z_table(percent, ac_average, ac_std)
        for k, (bp, ap, sp) in und.items():
            raw[k] = interpolated(raw, k)
            undefined_peaks.append((k[0], k[1], k[2], bp, ap, sp))
        percent = percent_of(raw, num_cycles, include_multidrop)
        if not z:
            stop = R.STOP_NO_DEFINED
            break
        if z[R.dict_max(z)] <= sigma_threshold:
            stop = R.STOP_THRESHOLD
            break
        values = {k: interpolated(raw, k) for k in z}
        diffs = {}
        for k, v in values.items():
            if z[k] <= sigma_threshold:
                continue
            trial = dict(raw)
            trial[k] = v
            tz, _ = R.z_table(percent_of(trial, num_cycles, include_multidrop), ac_average, ac_std)
            diffs[k] = z[k] - tz[k]
        best = R.dict_max(diffs)
        if diffs[best] <= 0:
            stop = R.STOP_NO_IMPROVEMENT
            break
        raw[best] = values[best]
        accepted.append(best)
        if prior is not None:
            changes = [abs(raw[k] - prior[k]) for k in prior]
            if changes[R.scan_max(changes)] < 0.001:
                stop = R.STOP_CONVERGED
                break
        prior = dict(raw)
        percent = percent_of(raw, num_cycles, include_multidrop)
    return dict(keys=list(raw), counts=[float(v) for v in raw.values()],
                updated_boc_raw={k: int(R.py2_round(c)) for k, c in raw.items()}, updated_boc_percent=percent,
                undefined_peaks=undefined_peaks, stop=stop, passes=passes, accepted=accepted)
