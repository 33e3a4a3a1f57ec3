"""The lognormal chain of lognormal_fitter_v2.main on a track table with numpy on the host: what lognormal.chain_device
computes on the GPU (include/fsq_lognormal_chain.h, fsq_binsearch.h, fsq_lognormal.h), the `host=True` route of
lognormal.chain_records.  Tracks are rows of arrays; no Python object is made per track but the fit's own
(_host_lognormal.fit, one call per track).

Also the pieces both routes share once a histogram is on the host: alpha from the histogram of all photometries
(`alpha_of_hist`, MCsimlib._get_m0Dm1 :3942-3979), beta and its sigma from the histogram of the last-drop values
(`beta_of_hist`, MCsimlib.last_drop_method_v2 :5357-5384), and the tally of the winning sequences (`tally_rows`)."""
import math

import numpy as np

from . import _host_lognormal
from . import _host_lognormal_dp
from . import _tracks

MAX_FRAMES = 64
STATUS_FOUND, STATUS_NONE, STATUS_OVER_BUDGET = 0, 1, 2


# ---- what both routes share ----

def alpha_of_hist(hist, n_bins, lo, hi):
    """_get_m0Dm1's [7] of the histogram `hist` of n_bins bins over lo .. hi: the left edge of the highest bin before the
    deepest valley.  The valley's depth at a bin is the lower of the highest bins to its left and to its right minus the bin,
    where the bin exceeds neither.  Where no bin stands before the valley, np.argmax raises its ValueError."""
    hist = np.asarray(hist)
    depth = np.zeros_like(hist)
    if len(hist) > 2:
        left = np.maximum.accumulate(hist)[:-2]                    # the highest of hist[:g], g = 1 .. len - 2
        right = np.maximum.accumulate(hist[::-1])[::-1][2:]        # the highest of hist[g + 1:]
        inner = hist[1:-1]
        depth[1:-1] = np.where((inner > left) | (inner > right), 0, np.minimum(left, right) - inner)
    gamma_index = np.argmax(depth)
    alpha_index = np.argmax(hist[:gamma_index])
    np.argmax(hist[gamma_index + 1:])                              # (beta_index of :3975: raises as there for an empty right side)
    mapping_factor = float(hi - lo) / n_bins
    return lo + mapping_factor * alpha_index


def beta_of_hist(hist, bins):
    """last_drop_method_v2's (beta, beta_sigma) of the histogram of the last-drop values and its n + 1 edges."""
    hist_max, hist_argmax = np.amax(hist), np.argmax(hist)
    if hist_argmax < len(bins) - 1:
        hist_max_logP = np.mean([bins[hist_argmax], bins[hist_argmax + 1]])
    else:
        hist_max_logP = bins[hist_argmax]
    hwhm = hist_max_logP / 2.0
    for i in range(int(hist_argmax) - 1, -1, -1):
        if hist[i] > hist_max / 2.0:
            continue
        hwhm = hist_max_logP - np.mean([bins[i], bins[i + 1]])
        break
    beta = math.e**hist_max_logP
    beta_sigma = hwhm / math.sqrt(2.0 * math.log(2.0))
    return beta, beta_sigma


def alpha_of_values(values):
    """(alpha, the bin count) of all photometries, searched on the host."""
    from . import lognormal as _ln
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    n_bins = _ln.optimal_bin_count(values, 10, 10000)
    hist, _ = np.histogram(a=values, bins=n_bins)
    return alpha_of_hist(hist, n_bins, values.min(), values.max()), n_bins


def beta_of_values(values):
    """(beta, beta_sigma) of the last-drop values, searched on the host; ValueError for none."""
    from . import lognormal as _ln
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    if values.size == 0:
        raise ValueError("min() arg is an empty sequence")         # (optimal_bin_size's min() of an empty last-drop list)
    hist, bins = np.histogram(a=values, bins=_ln.optimal_bin_count(values))
    return beta_of_hist(hist, bins)


def tally_rows(rows, first, counts, total):
    """(signals, total_count, none_count) of the unique winning sequences `rows` (lists of counts), the index of each one's
    first track and how often each stands, among `total` tracks: the keys in the order of their first track, as
    _tracks.tally_signals leaves them when it walks the tracks."""
    order = sorted(range(len(rows)), key=lambda k: first[k])
    signals, none = _tracks.tally_signals((_host_lognormal.signal_of(tuple(rows[k])) for k in order), [counts[k] for k in order])
    return signals, int(total), int(total) - sum(counts) + none


def tally(status, best_seq):
    """tally_rows of a fit's arrays."""
    found = np.flatnonzero(np.asarray(status) == STATUS_FOUND)
    if len(found) == 0:
        return {}, len(status), len(status)
    rows, first, counts = np.unique(np.asarray(best_seq)[found], axis=0, return_index=True, return_counts=True)
    return tally_rows(rows.tolist(), found[first].tolist(), counts.tolist(), len(status))


def check_frames(F, allow_multidrop):
    if F < 1:
        raise ValueError("at least one frame is needed")
    if F > MAX_FRAMES:
        raise NotImplementedError("tracks are limited to %d frames" % MAX_FRAMES)
    if not allow_multidrop and F == 1:
        raise ValueError("max() arg is an empty sequence")        # (max(seq_diff) of a one-frame sequence, :5442)


def check_status(status, what):
    """NotImplementedError for a track over the budget, ValueError for one of an invalid length."""
    status = np.asarray(status)
    if (status == STATUS_OVER_BUDGET).any():
        raise NotImplementedError("%s: track %d has more surviving sequences than the budget"
                                  % (what, int(np.flatnonzero(status == STATUS_OVER_BUDGET)[0])))
    if (status > STATUS_OVER_BUDGET).any():
        raise ValueError("%s: invalid length" % what)


# ---- the chain on arrays ----

def category_bits(cats, F):
    """bool [n, F]: frame f of track t is ON."""
    return ((np.asarray(cats, dtype=np.uint64)[:, None] >> np.arange(F, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)


def on_then_off(bits):
    """bool [n, F - 1]: frame f is ON and frame f + 1 is OFF."""
    return bits[:, :-1] & ~bits[:, 1:]


def last_drops(rows, bits, truncate=0):
    """log(I) of every frame f >= truncate with frame f ON, frame f + 1 OFF and I > 0, in (track, frame) order."""
    F = rows.shape[1]
    take = on_then_off(bits) & (np.arange(F - 1) >= truncate)[None, :] & (rows[:, :-1] > 0)
    return np.array([math.log(x) for x in rows[:, :-1][take].tolist()], dtype=np.float64)


def fit_rows(rows, bits, log_fluor_means, beta_sigma, max_possible, allow_multidrop, max_deviation, budget, solver='enumerate'):
    """lognormal.lognormal_device's dict as arrays, with _host_lognormal.fit, or with solver='dp' _host_lognormal_dp.fit
    (no track over the budget)."""
    n, F = rows.shape
    out = {"status": np.zeros(n, np.int32), "best_seq": np.zeros((n, F), np.uint8), "best_score": np.full(n, -1.0),
           "frame_score": np.zeros((n, F)), "n_surviving": np.zeros(n, np.int64)}
    if solver == 'dp':
        _host_lognormal_dp.check_overflow(beta_sigma, F)
    for t, (I, c) in enumerate(zip(rows.tolist(), bits.tolist())):
        if solver == 'dp':
            seq, score, scores, out["n_surviving"][t] = _host_lognormal_dp.fit(I, c, log_fluor_means, beta_sigma, max_possible,
                                                                               allow_multidrop, max_deviation)
            if seq is None:
                out["status"][t] = STATUS_NONE
            else:
                out["best_seq"][t], out["best_score"][t], out["frame_score"][t] = seq, score, scores
            continue
        ok, _ = _host_lognormal.tables(I, c, log_fluor_means, beta_sigma, max_possible, max_deviation)
        out["n_surviving"][t] = min(_host_lognormal.count_surviving(ok, max_possible, allow_multidrop), np.iinfo(np.int64).max)
        if out["n_surviving"][t] > budget:
            out["status"][t] = STATUS_OVER_BUDGET
            continue
        seq, score, scores, _ = _host_lognormal.fit(I, c, log_fluor_means, beta_sigma, max_possible, allow_multidrop, max_deviation)
        if seq is None:
            out["status"][t] = STATUS_NONE
        else:
            out["best_seq"][t], out["best_score"][t], out["frame_score"][t] = seq, score, scores
    return out


def _median(values):
    return np.float64(np.nan) if len(values) == 0 else np.median(values)


def on_off_medians(rows, bits, seg_off, found, alpha):
    """(m float64 [S, F - 1], counts int32 [S, F - 1], M): the medians of I - alpha over the ON -> OFF entries of the tracks
    with a sequence per (segment, frame), NaN without entries, and the median of the medians that exist, NaN without any."""
    n, F = rows.shape
    S = len(seg_off) - 1
    take = on_then_off(bits) & np.asarray(found, dtype=bool)[:, None]
    values = rows[:, :-1] - alpha
    m, counts = np.full((S, F - 1), np.nan), np.zeros((S, F - 1), np.int32)
    for s in range(S):
        a, b = int(seg_off[s]), int(seg_off[s + 1])
        for f in range(F - 1):
            entries = values[a:b, f][take[a:b, f]]
            counts[s, f] = len(entries)
            m[s, f] = _median(entries)
    return m, counts, float(_median(m[counts > 0]))


def on_off_adjust(rows, seg_off, alpha, m, counts, M):
    """(I - alpha) * M / m[(segment, f)] where f < F - 1 and the key has entries, else the raw I."""
    seg = np.repeat(np.arange(len(seg_off) - 1), np.diff(seg_off))
    adjusted = rows.copy()
    with np.errstate(all='ignore'):
        adjusted[:, :-1] = np.where(counts[seg] > 0, (rows[:, :-1] - alpha) * M / m[seg], rows[:, :-1])
    return adjusted


def chain(rows, cats, seg_off, beta_sigma, max_possible=5, ddif=0.30, allow_multidrop=True, truncate=0, beta=None,
          no_adjustment=False, budget=1 << 22, solver='enumerate'):
    """lognormal.chain_device's dict as NumPy arrays and Python scalars: rows float64 [n, F], cats uint64 [n], seg_off int64
    [S + 1], the tracks of a field contiguous.  solver: 'enumerate' or 'dp', the fit of fit_rows."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    n, F = rows.shape
    check_frames(F, allow_multidrop)
    seg_off = np.asarray(seg_off, dtype=np.int64)
    bits = category_bits(cats, F)
    quench = tuple([0.0] + [ddif] * (max_possible + 1))
    fit_kw = dict(beta_sigma=beta_sigma, max_possible=max_possible, allow_multidrop=allow_multidrop, max_deviation=3, budget=budget, solver=solver)

    alpha, n_bins = alpha_of_values(rows)
    original_beta, original_beta_sigma = beta_of_values(last_drops(rows, bits, truncate))
    if beta is not None:
        original_beta = beta
    alpha_adjusted = rows - alpha
    if not np.isfinite(alpha_adjusted).all():
        raise ValueError("intensities must be finite")
    fit0 = fit_rows(alpha_adjusted, bits, _tracks.log_fluor_means(original_beta, quench, max_possible), **fit_kw)
    check_status(fit0["status"], "the first fit")
    m, counts, M = on_off_medians(rows, bits, seg_off, fit0["status"] == STATUS_FOUND, alpha)
    adjusted = alpha_adjusted if no_adjustment else on_off_adjust(rows, seg_off, alpha, m, counts, M)
    if not np.isfinite(adjusted).all():
        raise ValueError("an adjusted intensity is not finite")
    adj_beta, adj_beta_sigma = beta_of_values(last_drops(adjusted, bits))
    if beta is not None:
        adj_beta = beta
    fit1 = fit_rows(adjusted, bits, _tracks.log_fluor_means(adj_beta, quench, max_possible), **fit_kw)
    check_status(fit1["status"], "the second fit")
    return dict(alpha=alpha, n_bins=n_bins, original_beta=original_beta, original_beta_sigma=original_beta_sigma, adj_beta=adj_beta,
                adj_beta_sigma=adj_beta_sigma, alpha_adjusted=alpha_adjusted, adjusted=adjusted, on_off_median=m,
                on_off_count=counts, last_beta_median=M, fit0=fit0, fit1=fit1)
