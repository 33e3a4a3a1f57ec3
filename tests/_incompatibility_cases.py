"""The recorded runs of the reference's incompatibility loop (tests/golden/incompatibility.npz,
tools/gen_incompatibility_golden.py) as dicts, and what the host and the GPU tests of the pair kernels share."""
import math
import os

import numpy as np

from fluorosequencingimageanalysis_amd import _host_signal_sweep as H

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "incompatibility.npz")
OUTPUTS = ("best_point", "result", "factor", "dist", "error_point", "error_status")

_cache = {}


def golden():
    if not _cache:
        with np.load(GOLDEN) as z:
            _cache.update({k: z[k] for k in z.files})
    return _cache


def case_names():
    return [str(n) for n in golden()["names"]]


def case(name):
    """(observed dict, sweep_records' dict of the eight points, the candidate list, the cutoff or None) of a recorded case."""
    g = golden()
    sigs = lambda keys: [H.signal_of_key(k) for k in keys.tolist()]                  # noqa: E731
    observed = dict(zip(sigs(g[name + "_observed_keys"]), g[name + "_observed_counts"].tolist()))
    off = g[name + "_fit_offsets"].tolist()
    fit_keys, fit_counts = sigs(g[name + "_fit_keys"]), g[name + "_fit_counts"].tolist()
    fits = [dict(zip(fit_keys[a:b], fit_counts[a:b])) for a, b in zip(off, off[1:])]
    sweep = {"points": list(range(len(fits))), "all_simulations": {k: (d, None) for k, d in enumerate(fits)}}
    cutoff = float(g[name + "_cutoff"])
    return observed, sweep, sigs(g[name + "_candidates"]), None if math.isnan(cutoff) else cutoff


def runs(name):
    """(metric, normalize_counts, heatmap_normalize_counts, reverse_order, best_point [K], factor [K], dist [K, 2],
    dist_is_none [K, 2]) of every recorded run of a case."""
    g = golden()
    for mi, metric in enumerate(g["metrics"].tolist()):
        for ni, (nc, hn) in enumerate(g["normalizations"].tolist()):
            for ri, reverse_order in enumerate((False, True)):
                yield (str(metric), bool(nc), bool(hn), reverse_order) + tuple(
                    g["%s_%s" % (name, what)][mi, ni, ri] for what in ("best_point", "factor", "dist", "dist_is_none"))


def host_inputs(observed, sweep, candidates, **opts):
    """(key table, candidate rows, fit [S, P], fit_total [P]) as incompatibility_records(host=True) builds them."""
    dicts = [sweep["all_simulations"][k][0] for k in sweep["points"]]
    signals = H.ordered_signals(set(observed).union(*dicts))
    fit, fit_total = H.fit_matrix(signals, dicts)
    index = {s: i for i, s in enumerate(signals)}
    return H.key_table(observed, signals, **opts), np.array([index.get(s, -1) for s in candidates], np.int32), fit, fit_total


def same_bits(a, b):
    """Equal float64 arrays bit for bit, every NaN counted as one pattern."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint64),
                                                                                              b[~np.isnan(b)].view(np.uint64))


def assert_same_outputs(got, want, what):
    for k in OUTPUTS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if w.dtype == np.float64:
            assert same_bits(g, w), (what, k, g, w)
        else:
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, k, g, w)


def synthetic(S, P, seed):
    """A key table over S made-up heat-map keys and a count matrix [S, P] with every situation in it: keys that are observed
    only, fit only, in neither, not admitted, observed with a count of zero, small counts around a cutoff of 3, and points at
    which nothing of a key stands."""
    rng = np.random.default_rng(seed)
    observed = rng.integers(0, 60, S).astype(np.int64)
    in_observed = (rng.random(S) < 0.8).astype(np.uint8)
    observed[in_observed == 0] = 0
    observed[::5] = np.minimum(observed[::5], 4)
    fit = rng.integers(0, 60, (S, P)).astype(np.int64)
    fit[rng.random((S, P)) < 0.3] = 0
    fit[1::4] = np.minimum(fit[1::4], 5)
    if S > 2:
        fit[2] = 0                                                                   # a key in no fit
    admitted = (rng.random(S) < 0.9).astype(np.uint8)
    heatmap = np.ones(S, np.uint8)
    table = {"signals": list(range(S)), "observed": observed, "in_observed": in_observed, "admitted": admitted, "heatmap": heatmap,
             "n_observed": int(observed.sum()) + 50}
    return table, fit, fit.sum(axis=0) + 100
