"""Writes tests/golden/signal_sweep.npz: the reference's signal_correlation (jupyter_development.py:279-578) recorded for the
ten metrics fsq_signal_scores builds, under the three normalisations, on pairs of signal dicts.  Data only: the dicts as key
arrays (include/fsq_signal_sweep.h's 64-bit keys) in their dict order - the order the reference sums in - with their counts,
the options, and per (case, metric, normalisation) the status, the result, the factor and the contributions.

The reference function is loaded at run time through oracle/refload.py (never written anywhere), with np, sqrt and log
injected as its module imports them.  Checked for Python-2 integer division in the ten metrics: every fit count is a float
after `fit_count * float(normalization_factor)` (:362), every divisor is a float() or a sqrt, and the factor is
float(...) / ...; `observed_count * (n - observed_count) / float(n)` divides by a float.  None is left.

  python tools/gen_signal_sweep_golden.py
"""
import os
import sys
from math import log, sqrt

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")]

from fluorosequencingimageanalysis_amd import _host_signal_sweep as H          # noqa: E402
from fluorosequencingimageanalysis_amd import signal_sweep as SW               # noqa: E402

NORMALIZATIONS = ((False, False), (True, False), (False, True))                # (normalize_counts, heatmap_normalize_counts)
STATUS_OF = {ZeroDivisionError: H.SCORE_DIVZERO, ValueError: H.SCORE_DOMAIN}


def sig(start, *cycles):
    """The signal of a row that starts at `start` dyes and drops one at each of `cycles`."""
    return H.signal_of_key(H.key_of(start, cycles))


def twin_cases():
    """Two pairs from the seeded host twin at different points: the fits of one point against those of another, and the
    molecular signals of the two."""
    sweep = SW.sweep_records('GAKAGAKC', 'K', 2, 4, [(0.9, 0.05, 0.1), (0.7, 0.2, 0.4)], 300, seed=7, host=True, quench_factors=[0, 0.3] + [0.3] * 5,
                             s=0.1, sc=3, s2=0.05, beta=70000.0, beta_sigma=0.2, ddif=[0, 0.3] + [0.3] * 5)
    (sa, ma), (sb, mb) = (sweep["all_simulations"][k] for k in sweep["points"])
    wide = dict(zero_only=False, heatmap_only=False, allow_multidrop=True)
    return [("twin_fits_defaults", sa, sb, {}), ("twin_fits_wide", sa, sb, wide), ("twin_molecular_wide", mb, ma, wide)]


def hand_cases():
    obs = {sig(1, 1): 120, sig(1, 3): 80, sig(2, 1, 4): 40, sig(2, 2, 2): 9, sig(2, 3): 31, sig(1): 200, sig(3, 1, 2, 5): 12,
           sig(0): 7, sig(2, 1, 2): 3}
    fit = {sig(1, 3): 60, sig(1, 1): 150, sig(2, 1, 4): 44, sig(1, 2): 17, sig(2, 2, 2): 4, sig(1): 260, sig(2, 5): 21,
           sig(3, 1, 2, 5): 2, sig(3, 3, 3, 3): 5, sig(2, 1, 2): 30}
    wide = dict(zero_only=False, heatmap_only=False, allow_multidrop=True)
    off = {sig(2, 3): 10, sig(1): 50, sig(3, 1): 4}                          # no key ends at zero
    return [("hand_defaults", obs, fit, {}),
            ("hand_wide", obs, fit, wide),
            ("hand_zero_multidrop", obs, fit, dict(heatmap_only=False, allow_multidrop=True)),
            ("hand_cutoff", obs, fit, dict(wide, small_count_cutoff=5)),
            ("hand_select", obs, fit, dict(wide, select_signals={sig(1, 1), sig(1, 2), sig(2, 1, 4), sig(1), sig(3, 3, 3, 3)})),
            ("hand_exclude", obs, fit, dict(wide, exclude_signals={sig(1, 1), sig(2, 5), sig(0)})),
            ("nothing_pairs", off, {sig(2, 3): 3, sig(2, 4): 8}, {}),
            ("heatmap_total_zero", off, {sig(2, 3): 3, sig(2, 4): 8}, dict(zero_only=False, heatmap_only=False)),
            ("one_observed_signal", {sig(1, 2): 50}, {sig(1, 2): 40, sig(1, 3): 10}, {}),
            ("observed_only", obs, {}, wide)]


def main():
    import refload
    from gen_lognormal_golden import load_functions
    ref = load_functions(refload, "jupyter_development.py", ["signal_correlation"], {"np": np, "sqrt": sqrt, "log": log})
    cases = twin_cases() + hand_cases()
    keys = lambda signals: np.array([H.key_of_signal(s) for s in signals], np.uint64)      # noqa: E731
    out = {"metrics": np.array(H.METRICS), "normalizations": np.array(NORMALIZATIONS), "names": np.array([c[0] for c in cases])}
    shape = (len(cases), len(H.METRICS), len(NORMALIZATIONS))
    status, result, factor = np.zeros(shape, np.int32), np.full(shape, np.nan), np.full(shape, np.nan)
    c_off, c_keys, c_vals = [0], [], []
    for ci, (name, obs, fit, opts) in enumerate(cases):
        out["%s_observed_keys" % name], out["%s_observed_counts" % name] = keys(obs), np.array(list(obs.values()), np.int64)
        out["%s_fit_keys" % name], out["%s_fit_counts" % name] = keys(fit), np.array(list(fit.values()), np.int64)
        out["%s_flags" % name] = np.array([opts.get("zero_only", True), opts.get("heatmap_only", True), opts.get("allow_multidrop", False)])
        out["%s_cutoff" % name] = np.float64(opts.get("small_count_cutoff", np.nan))
        for what in ("select_signals", "exclude_signals"):
            if opts.get(what) is not None:
                out["%s_%s" % (name, what)] = keys(sorted(opts[what]))
        for mi, metric in enumerate(H.METRICS):
            for ni, (nc, hn) in enumerate(NORMALIZATIONS):
                contrib = {}
                try:
                    r, (nf, contrib) = ref["signal_correlation"](obs, fit, metric=metric, normalize_counts=nc, heatmap_normalize_counts=hn, **opts)
                    factor[ci, mi, ni] = nf
                    if r is None:
                        status[ci, mi, ni] = H.SCORE_EMPTY
                    else:
                        result[ci, mi, ni] = r
                except (ZeroDivisionError, ValueError) as e:
                    status[ci, mi, ni], contrib = STATUS_OF[type(e)], {}
                c_keys += [H.key_of_signal(s) for s in contrib]
                c_vals += [float(v) for v in contrib.values()]
                c_off.append(len(c_keys))
    out.update(status=status, result=result, factor=factor, contribution_offsets=np.array(c_off, np.int64),
               contribution_keys=np.array(c_keys, np.uint64), contribution_values=np.array(c_vals, np.float64))
    path = os.path.join(ROOT, "tests", "golden", "signal_sweep.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d runs, %d bytes; statuses %s" % (path, len(cases), status.size, os.path.getsize(path),
                                                            np.bincount(status.reshape(-1)).tolist()))


if __name__ == "__main__":
    main()
