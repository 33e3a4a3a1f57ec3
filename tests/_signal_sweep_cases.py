"""The recorded runs of the reference's signal_correlation (tests/golden/signal_sweep.npz, tools/gen_signal_sweep_golden.py)
as dicts, and the comparison the host and the GPU tests make against them."""
import math
import os

import numpy as np

from fluorosequencingimageanalysis_amd import _host_signal_sweep as H

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "signal_sweep.npz")
U = 2.0 ** -53                                  # the unit roundoff of float64
SUMS = ('naive', 'my_canberra')
ROOTS = ('my_euclidean', 'normalized_euclidean', 'my_std_normalized_euclidean', 'my_sim_std_normalized_euclidean', 'log_rmsd')
MAXIMA = ('my_chebyshev', 'my_normalized_chebyshev', 'my_std_normalized_chebyshev')
assert set(SUMS + ROOTS + MAXIMA) == set(H.METRICS)

_cache = {}


def golden():
    if not _cache:
        with np.load(GOLDEN) as z:
            _cache.update({k: z[k] for k in z.files})
    return _cache


def case_names():
    return [str(n) for n in golden()["names"]]


def case(name):
    """(observed dict, fit dict, signal_correlation's option keywords) of a recorded case, the dicts in their recorded order."""
    g = golden()
    d = lambda what: {H.signal_of_key(k): int(n) for k, n in zip(g["%s_%s_keys" % (name, what)].tolist(),      # noqa: E731
                                                                 g["%s_%s_counts" % (name, what)].tolist())}
    zero_only, heatmap_only, allow_multidrop = (bool(x) for x in g["%s_flags" % name])
    opts = dict(zero_only=zero_only, heatmap_only=heatmap_only, allow_multidrop=allow_multidrop)
    if not math.isnan(float(g["%s_cutoff" % name])):
        opts["small_count_cutoff"] = float(g["%s_cutoff" % name])
    for what in ("select_signals", "exclude_signals"):
        if "%s_%s" % (name, what) in g:
            opts[what] = {H.signal_of_key(k) for k in g["%s_%s" % (name, what)].tolist()}
    return d("observed"), d("fit"), opts


def runs(name):
    """(metric, normalize_counts, heatmap_normalize_counts, status, result, factor, {signal: contribution}) of every recorded
    run of a case."""
    g = golden()
    ci = case_names().index(name)
    n_norm = len(g["normalizations"])
    for mi, metric in enumerate(g["metrics"].tolist()):
        for ni, (nc, hn) in enumerate(g["normalizations"].tolist()):
            r = (ci * len(g["metrics"]) + mi) * n_norm + ni
            a, b = g["contribution_offsets"][r:r + 2]
            contrib = {H.signal_of_key(k): v for k, v in zip(g["contribution_keys"][a:b].tolist(), g["contribution_values"][a:b].tolist())}
            yield (str(metric), bool(nc), bool(hn), int(g["status"][ci, mi, ni]), float(g["result"][ci, mi, ni]),
                   float(g["factor"][ci, mi, ni]), contrib)


def outcome(call):
    """(status, result, factor, contributions) of a signal_correlation call, exceptions as the kernel's statuses."""
    try:
        result, (factor, contrib) = call()
    except ZeroDivisionError:
        return H.SCORE_DIVZERO, None, None, {}
    except ValueError:
        return H.SCORE_DOMAIN, None, None, {}
    return (H.SCORE_EMPTY if result is None else H.SCORE_OK), result, factor, contrib


def bits(x):
    return np.float64(x).view(np.uint64)


def check_against_golden(what, metric, got, recorded):
    """The comparison with the reference.

    The status, the factor (a quotient of two integer sums: no order to differ in), every contribution (the same operations on
    the same operands) and the maxima are the reference's bits.  A sum is not: the reference adds its S contributions in dict
    order, we add them in key order.  Every contribution t_i is non-negative, and a recursive float64 sum of S terms in any
    order is sum(t_i * (1 + d_i)) with |d_i| <= (S - 1) u (to first order in u = 2^-53; Higham, Accuracy and Stability of
    Numerical Algorithms, 4.2), so it lies within (S - 1) u * T of the exact T = sum(t_i), and two orders lie within
    2 (S - 1) u T < 2 S u T of each other: a relative 2 S 2^-53.  A square root halves a relative error and rounds once on
    either side, which is within one more ulp (2^-52 relative); log_rmsd's division by S before the root rounds once on either
    side too, 2 u on the root's argument and so u on the root, still inside 2 S u + 2^-52 for S >= 1."""
    status, result, factor, contrib = got
    r_status, r_result, r_factor, r_contrib = recorded
    assert status == r_status, (what, status, r_status)
    if status in (H.SCORE_OK, H.SCORE_EMPTY):
        assert bits(factor) == bits(r_factor), (what, factor, r_factor)
    if status != H.SCORE_OK:
        return
    assert set(contrib) == set(r_contrib), what
    for s, v in r_contrib.items():
        assert bits(contrib[s]) == bits(v), (what, s, contrib[s], v)
    if metric in MAXIMA:
        assert bits(result) == bits(r_result), (what, result, r_result)
    else:
        S = len(r_contrib)
        bound = 2 * S * U + (2.0 ** -52 if metric in ROOTS else 0.0)
        assert abs(result - r_result) <= bound * abs(r_result), (what, result, r_result, S)
