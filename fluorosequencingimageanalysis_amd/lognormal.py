"""Lognormal fluor-count fitting of track photometries on the GPU: the reference's lognormal_fitter_v2 chain.

The fit itself - MCsimlib._intensities_to_signal_lognormal_v8 (:5387-5493), the most expensive per-track step of the chain -
runs on the device, one wavefront per track and one launch for a whole experiment (`lognormal_device`, `lognormal_records`,
`photometries_lognormal_fit`; include/fsq_lognormal.h).  The host pieces of the chain (the CSV reader, the histogram bin
search, alpha, beta, the ON/OFF adjustment) are restated here with the reference's own numpy calls.  The bin search, 9 991
histograms of all photometries for alpha alone, also runs on the device with numpy's bits (`histogram_costs_device`,
`bin_search_records`, `histogram_counts`; include/fsq_binsearch.h): `optimal_bin_size`, `optimal_bin_count`, `_get_m0Dm1` and
`last_drop_method_v2` take it with `device=...` and stay on the host with `device=None`.

The whole chain also runs on a track table that stays on the device (`chain_device`, `chain_records`,
`track_table_from_photometries`, `track_table_from_records`; include/fsq_lognormal_chain.h): the last-drop lists, the ON/OFF
medians and the adjustment are kernels, only scalars and histograms cross to the host between the steps, and no Python object
is made per track.  `chain_records(host=True)` is its NumPy twin (_host_lognormal_chain.py).

Limits of the device fit, each raised on the host before anything is launched: 1 .. 64 frames per track
(NotImplementedError above 64, ValueError for none), max_possible in 1 .. 15 (NotImplementedError above), beta_sigma finite
and > 0, max_deviation not NaN, finite intensities and finite log_fluor_means (ValueError).  With the default solver='enumerate' allow_upsteps=True raises
NotImplementedError (the command line never passes it), and a track with more surviving sequences than `budget` (default 2^22)
is not enumerated: it comes back with STATUS_OVER_BUDGET from the array interfaces and raises NotImplementedError naming the
track from the dict interfaces.

solver='dp' (include/fsq_lognormal_dp.h, _host_lognormal_dp.py) finds the same winner, bit for bit and with the reference's tie
rule, by an exact dynamic programme in O(frames * max_possible^2) per track: no track is over a budget (`budget` is accepted
and unused) and allow_upsteps=True is served.  It refuses (ValueError, before any launch) a beta_sigma so small that a product
of max_frames densities could overflow: 1 / (sqrt(2 pi) * beta_sigma) > 1 and max_frames * log of it >= 700.

Limits of the device bin search, each raised as ValueError on the host before anything is launched: at least one value, finite
values, integers of magnitude at most 2^53 (beyond it float64 does not hold them), bin counts in 1 .. 10 000
(FSQ_BINSEARCH_MAX_BINS), fewer than 2^31 values.  Where all values are equal the search runs on the host whatever `device` is,
and ends as it ends there."""
import ctypes
import math
from math import log, sqrt

import numpy as np

from . import _host_lognormal_chain as HC
from . import _host_lognormal_dp as HD
from . import _native_binsearch as NB
from . import _native_lognormal as NL
from . import _native_lognormal_chain as NC
from . import _native_lognormal_dp as ND
from . import _tracks
from . import engine as _engine
from ._tracks import category_word                                # noqa: F401  (its old place)
from .pflib import _py2_round

STATUS_FOUND, STATUS_NONE, STATUS_OVER_BUDGET = NL.STATUS_FOUND, NL.STATUS_NONE, NL.STATUS_OVER_BUDGET
DEFAULT_BUDGET = NL.DEFAULT_BUDGET
MAX_BINS = NB.MAX_BINS


# ---- the device fit ----

SOLVERS = ('enumerate', 'dp')


def _no_upsteps(allow_upsteps):
    if allow_upsteps:
        raise NotImplementedError("allow_upsteps=True is not built with solver='enumerate': pass solver='dp'")


def _check_solver(solver, allow_upsteps=False):
    if solver not in SOLVERS:
        raise ValueError("solver must be 'enumerate' or 'dp', not %r" % (solver,))
    if solver == 'enumerate':
        _no_upsteps(allow_upsteps)


def _solver_kw(solver, allow_upsteps=False):
    """The keywords that choose the dynamic programme; none for the default solver."""
    return {} if solver == 'enumerate' else {"solver": solver, "allow_upsteps": bool(allow_upsteps)}


def fit_params(log_fluor_means, beta_sigma, max_possible, allow_multidrop, max_deviation, budget):
    """FsqLognormalParams after the checks the module docstring names."""
    if log_fluor_means is None:
        raise ValueError("v8+ requires log_fluor_means to be passed manually")
    max_possible = int(max_possible)
    if max_possible < 1:
        raise ValueError("max_possible must be at least 1")
    if max_possible > NL.MAX_POSSIBLE:
        raise NotImplementedError("max_possible is limited to %d" % NL.MAX_POSSIBLE)
    means = [float(x) for x in log_fluor_means]
    if len(means) < max_possible + 1:
        raise IndexError("list index out of range")                # (norm_function_cache reads log_fluor_means[max_possible], :5433)
    if not all(math.isfinite(x) for x in means[:max_possible + 1]):
        raise ValueError("log_fluor_means must be finite")
    beta_sigma, max_deviation = float(beta_sigma), float(max_deviation)
    if not (math.isfinite(beta_sigma) and beta_sigma > 0):
        raise ValueError("beta_sigma must be finite and > 0")
    if math.isnan(max_deviation):
        raise ValueError("max_deviation must not be NaN")
    budget = int(budget)
    if not 1 <= budget <= NL.MAX_BUDGET:
        raise ValueError("budget must be in 1 .. 2^59")
    prm = NL.FsqLognormalParams()
    for i, x in enumerate(means[:NL.MAX_POSSIBLE + 2]):
        prm.log_fluor_means[i] = x
    prm.beta_sigma, prm.max_deviation, prm.budget = beta_sigma, max_deviation, budget
    prm.max_possible, prm.allow_multidrop = max_possible, 1 if allow_multidrop else 0
    return prm


def lognormal_device(d_intensity, d_category, d_len, log_fluor_means, beta_sigma, max_possible=5, allow_multidrop=True,
                     max_deviation=3, budget=DEFAULT_BUDGET, prm=None, solver='enumerate', allow_upsteps=False):
    """fsq_lognormal_fit on device tensors: float64 [n, max_frames] intensities, int64 [n] categories (bit f set when frame f
    is ON, the uint64 word of sequencing.py) and int32 [n] lengths.  Returns a dict of device tensors: status int32 [n], best_seq
    uint8 [n, max_frames], best_score float64 [n], frame_score float64 [n, max_frames], n_surviving int64 [n].  Enqueued on the
    current stream, not synchronised.  Lengths and intensities are not checked here: a track whose length is not in
    1 .. max_frames comes back with status 3.  `prm`: the parameters already built by fit_params (the other arguments are then unused).
    solver='dp': fsq_lognormal_fit_dp, the same dict; no status is STATUS_OVER_BUDGET, and allow_upsteps is served."""
    torch = _engine._torch()
    _check_solver(solver, allow_upsteps)
    if prm is None:
        prm = fit_params(log_fluor_means, beta_sigma, max_possible, allow_multidrop, max_deviation, budget)
    dev = d_intensity.device
    n, max_frames = int(d_intensity.shape[0]), int(d_intensity.shape[1])
    if max_frames > NL.MAX_FRAMES:
        raise NotImplementedError("tracks are limited to %d frames" % NL.MAX_FRAMES)
    dp = solver == 'dp'
    if dp:
        HD.check_overflow(prm.beta_sigma, max_frames)
    L = ND.lib() if dp else NL.lib()
    ws_bytes = (L.fsq_lognormal_dp_workspace_bytes if dp else L.fsq_lognormal_workspace_bytes)(n, max_frames)
    if ws_bytes < 0:
        raise ValueError("fsq_lognormal_workspace_bytes: invalid shape")
    if not (d_intensity.is_contiguous() and d_category.is_contiguous() and d_len.is_contiguous()):
        raise ValueError("contiguous tensors are needed")
    if d_intensity.dtype != torch.float64 or d_len.dtype != torch.int32 or d_category.element_size() != 8:
        raise ValueError("float64 intensities, 64-bit categories and int32 lengths are needed")
    out = {"status": torch.empty(n, dtype=torch.int32, device=dev),
           "best_seq": torch.empty((n, max_frames), dtype=torch.uint8, device=dev),
           "best_score": torch.empty(n, dtype=torch.float64, device=dev),
           "frame_score": torch.empty((n, max_frames), dtype=torch.float64, device=dev),
           "n_surviving": torch.empty(n, dtype=torch.int64, device=dev)}
    _engine.launch(L.fsq_lognormal_fit_dp if dp else L.fsq_lognormal_fit, "fsq_lognormal_fit_dp" if dp else "fsq_lognormal_fit", dev,
                   d_intensity.data_ptr(), d_category.data_ptr(), d_len.data_ptr(), n, max_frames, ctypes.byref(prm),
                   out["status"].data_ptr(), out["best_seq"].data_ptr(), out["best_score"].data_ptr(), out["frame_score"].data_ptr(),
                   out["n_surviving"].data_ptr(), *((1 if allow_upsteps else 0,) if dp else ()), None, 0)
    return out


def log_device(d_x):
    """fsq_lognormal_log: glibc 2.35's log of a float64 device tensor, bit for bit."""
    torch = _engine._torch()
    if d_x.dtype != torch.float64 or not d_x.is_contiguous():
        raise ValueError("a contiguous float64 tensor is needed")
    out = torch.empty_like(d_x)
    _engine.launch(NL.lib().fsq_lognormal_log, "fsq_lognormal_log", d_x.device, d_x.data_ptr(), out.data_ptr(), int(d_x.numel()))
    return out


def _rows(intensities, categories, lengths):
    """(float64 [n, max_frames], uint64 [n], int32 [n]) of ragged host sequences, or of a 2-D array with lengths."""
    rows, lens = _tracks.pack_rows(intensities, lengths, min_frames=1,
                                   short_error="max() arg is an empty sequence")   # (max(intensities) of a track without frames, :5413)
    if len(lens) and lens.max() > rows.shape[1]:
        raise ValueError("a length exceeds the width of the rows")
    if len(lens) and lens.max() > NL.MAX_FRAMES:
        raise NotImplementedError("tracks are limited to %d frames" % NL.MAX_FRAMES)
    if not (isinstance(categories, np.ndarray) and categories.ndim == 1 and categories.dtype.kind in "iu"):
        categories = list(categories)
        if any(len(c) < T for c, T in zip(categories, lens)):
            raise IndexError("tuple index out of range")          # (categories[i] of a frame beyond the category, :5436)
    cats = _tracks.category_words(categories, None)
    if not (len(rows) == len(cats) == len(lens)):
        raise ValueError("one category and one length per track")
    valid = np.arange(rows.shape[1])[None, :] < lens[:, None]
    if not np.isfinite(rows[valid]).all():
        raise ValueError("intensities must be finite")
    return rows, cats, lens


def lognormal_records(intensities, categories, log_fluor_means, beta_sigma, max_possible=5, allow_multidrop=True,
                      max_deviation=3, budget=DEFAULT_BUDGET, lengths=None, device=None, solver='enumerate', allow_upsteps=False):
    """The fit for many tracks in one launch, as arrays.

    intensities  ragged sequences, a float64 [n, max_frames] array or a CUDA tensor of that shape (with `lengths`, or every
                 row full); categories  tuples of booleans, or the uint64 / int64 words as an array or CUDA tensor.
    Returns a dict of NumPy arrays: status (STATUS_FOUND / STATUS_NONE / STATUS_OVER_BUDGET), best_seq uint8 [n, max_frames],
    best_score, frame_score [n, max_frames], n_surviving int64 and lengths.  Rows beyond a track's length, and the rows of
    a track without a winner, hold count 0, score 0 and best_score -1.  solver, allow_upsteps: as lognormal_device."""
    _check_solver(solver, allow_upsteps)
    prm = fit_params(log_fluor_means, beta_sigma, max_possible, allow_multidrop, max_deviation, budget)
    if hasattr(intensities, "is_cuda"):                            # a torch tensor
        torch = _engine._torch()
        d_int = intensities.contiguous()
        n, F = int(d_int.shape[0]), int(d_int.shape[1])
        if solver == 'dp':
            HD.check_overflow(prm.beta_sigma, F)
        dev = d_int.device
        d_len = (torch.full((n,), F, dtype=torch.int32, device=dev) if lengths is None
                 else torch.as_tensor(lengths, dtype=torch.int32, device=dev).contiguous())
        d_cat = categories if torch.is_tensor(categories) else torch.from_numpy(np.asarray(categories).astype(np.uint64).view(np.int64))
        d_cat = d_cat.to(dev).contiguous()
        lens = d_len.cpu().numpy()
        if n and (int(lens.min()) < 1 or int(lens.max()) > min(F, NL.MAX_FRAMES)):
            raise ValueError("lengths must be in 1 .. max_frames (at most %d)" % NL.MAX_FRAMES)
        if n and not bool(torch.isfinite(torch.where(torch.arange(F, device=dev)[None, :] < d_len[:, None], d_int,
                                                     torch.zeros_like(d_int))).all()):
            raise ValueError("intensities must be finite")
    else:
        rows, cats, lens = _rows(intensities, categories, lengths)
        n = len(lens)
        if solver == 'dp':
            HD.check_overflow(prm.beta_sigma, rows.shape[1])
        if n:
            torch = _engine._torch()
            dev = torch.device(device or "cuda")
            d_int, d_len = torch.from_numpy(rows).to(dev), torch.from_numpy(lens).to(dev)
            d_cat = torch.from_numpy(cats.view(np.int64)).to(dev)
    if n == 0:
        return {"status": np.zeros(0, np.int32), "best_seq": np.zeros((0, 1), np.uint8), "best_score": np.zeros(0),
                "frame_score": np.zeros((0, 1)), "n_surviving": np.zeros(0, np.int64), "lengths": np.zeros(0, np.int32)}
    out = lognormal_device(d_int, d_cat, d_len, None, None, prm=prm, **_solver_kw(solver, allow_upsteps))
    host = _engine.to_host(out)
    host["lengths"] = np.asarray(lens, dtype=np.int32)
    return host


# ---- the histogram bin search on the device ----

def _checked_bin_counts(bin_counts):
    """int32 bin counts after the checks the module docstring names."""
    b = np.asarray(bin_counts)
    if b.ndim != 1 or b.size == 0 or b.dtype.kind not in "iu":
        raise ValueError("bin counts: a non-empty 1-D array of integers is needed")
    if int(b.min()) < 1 or int(b.max()) > MAX_BINS:
        raise ValueError("bin counts must be in 1 .. %d" % MAX_BINS)
    return np.ascontiguousarray(b, dtype=np.int32)


def _checked_values(values):
    """float64 values after the checks the module docstring names."""
    a = np.asarray(values).reshape(-1)
    if a.size == 0:
        raise ValueError("at least one value is needed")
    if a.dtype.kind in "iub":
        if int(a.min()) < -(1 << 53) or int(a.max()) > (1 << 53):
            raise ValueError("integers are limited to a magnitude of 2^53")
    elif a.dtype.kind != "f":
        raise ValueError("finite real values are needed (integers of a magnitude of at most 2^53)")
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not np.isfinite(a).all():
        raise ValueError("values must be finite")
    return a


def _sorted(d_values):
    torch = _engine._torch()
    if not d_values.is_cuda or d_values.dtype != torch.float64 or d_values.dim() != 1:
        raise ValueError("a 1-D float64 CUDA tensor is needed")
    if d_values.numel() < 1:
        raise ValueError("at least one value is needed")
    return torch.sort(d_values).values.contiguous()


def histogram_costs_device(d_values, bin_counts, lo=None, hi=None):
    """fsq_histogram_costs on a 1-D float64 CUDA tensor of values in any order: Shimazaki & Shinomoto's cost of every bin
    count, as optimal_bin_size computes it, a float64 CUDA tensor.  bin_counts: integers on the host (checked here), or an
    int32 CUDA tensor (not checked: a count outside 1 .. 10 000 comes back as NaN).  The values are sorted with torch.sort.
    Enqueued on the current stream; nothing is read back and the result is not synchronised.

    Without lo and hi the kernel takes the least and the greatest value from the sorted data (fsq_histogram_costs_sorted);
    the host cannot see the values then, so non-finite or all-equal values give NaN in every cost instead of an error.  With
    lo and hi (both) the caller vouches that they are the least and the greatest of finite values; bounds that cannot be
    (hi <= lo, non-finite) raise ValueError."""
    torch = _engine._torch()
    if (lo is None) != (hi is None):
        raise ValueError("lo and hi are given together or not at all")
    d_sorted = _sorted(d_values)
    dev = d_sorted.device
    if torch.is_tensor(bin_counts):
        if bin_counts.dtype != torch.int32 or bin_counts.dim() != 1 or bin_counts.device != dev:
            raise ValueError("bin counts: a 1-D int32 tensor on the values' device is needed")
        d_counts = bin_counts.contiguous()
    else:
        d_counts = torch.from_numpy(_checked_bin_counts(bin_counts)).to(dev)
    d_cost = torch.empty(int(d_counts.numel()), dtype=torch.float64, device=dev)
    bounds = () if lo is None else (float(lo), float(hi))
    _engine.launch(NB.lib().fsq_histogram_costs_sorted if lo is None else NB.lib().fsq_histogram_costs, "fsq_histogram_costs", dev,
                   d_sorted.data_ptr(), int(d_sorted.numel()), *bounds, d_counts.data_ptr(), int(d_counts.numel()), d_cost.data_ptr())
    return d_cost


def histogram_counts_device(d_values, n_bins, lo=None, hi=None):
    """fsq_histogram_counts: np.histogram(values, bins=np.linspace(lo, hi, n_bins + 1))[0] as an int64 CUDA tensor, enqueued
    on the current stream.  lo and hi are the least and the greatest value; where they are not given they are read back from
    the device (one small synchronising copy).  Bounds that cannot be (equal, non-finite) raise ValueError."""
    torch = _engine._torch()
    n_bins = int(n_bins)
    if not 1 <= n_bins <= MAX_BINS:
        raise ValueError("bin counts must be in 1 .. %d" % MAX_BINS)
    d_sorted = _sorted(d_values)
    if lo is None or hi is None:
        lo, hi = d_sorted[[0, -1]].tolist()
    lo, hi = float(lo), float(hi)
    dev = d_sorted.device
    d_hist = torch.empty(n_bins, dtype=torch.int64, device=dev)
    _engine.launch(NB.lib().fsq_histogram_counts, "fsq_histogram_counts", dev, d_sorted.data_ptr(), int(d_sorted.numel()), lo, hi,
                   n_bins, d_hist.data_ptr())
    return d_hist


def histogram_costs(values, bin_counts, device=None):
    """histogram_costs_device for host values: the costs as a float64 array."""
    a, b = _checked_values(values), _checked_bin_counts(bin_counts)
    torch = _engine._torch()
    d_values = torch.from_numpy(a).to(torch.device(device or "cuda"))
    return histogram_costs_device(d_values, b, float(a.min()), float(a.max())).cpu().numpy()


def bin_search_records(values, min_n_bins, max_n_bins, device=None):
    """The search of optimal_bin_size over min_n_bins .. max_n_bins on the device, as a dict of NumPy values: cost (float64,
    one per bin count), n_bins (the first bin count of least cost, optimal_bin_count's rule), lo and hi."""
    a = _checked_values(values)
    cost = histogram_costs(a, np.arange(int(min_n_bins), int(max_n_bins) + 1), device)
    where = np.where(cost == np.amin(cost))
    return {"cost": cost, "n_bins": np.int64(int(where[0][0]) + int(min_n_bins)), "lo": np.float64(a.min()), "hi": np.float64(a.max())}


def histogram_counts(values, n_bins, device=None):
    """np.histogram(values, bins=np.linspace(min, max, n_bins + 1))[0] on the device: an int64 array."""
    a = _checked_values(values)
    if not 1 <= int(n_bins) <= MAX_BINS:
        raise ValueError("bin counts must be in 1 .. %d" % MAX_BINS)
    torch = _engine._torch()
    d_values = torch.from_numpy(a).to(torch.device(device or "cuda"))
    return histogram_counts_device(d_values, n_bins, float(a.min()), float(a.max())).cpu().numpy()


# ---- the reference's call surface ----

def signal_of(best_seq):
    """(signal, is_zero, starting_intensity) of a winning sequence (:5467-5491)."""
    drops = [best_seq[f] - fc for f, fc in enumerate(best_seq[1:])]
    signal = []
    for i, tf in enumerate(drops):
        if tf > 0:
            signal += [('A', i + 1)] * tf
        elif tf < 0:
            return None, None, best_seq[0]
    signal = tuple(signal) if len(signal) else (('A', 0),)
    return signal, best_seq[-1] == 0, best_seq[0]


def _fit_tuples(host, max_possible, what):
    """The reference's 7-tuple for every track of lognormal_records' output."""
    status = host["status"]
    if (status == STATUS_OVER_BUDGET).any():
        i = int(np.flatnonzero(status == STATUS_OVER_BUDGET)[0])
        raise NotImplementedError("%s: %d sequences pass the rules, more than the budget" % (what(i), int(host["n_surviving"][i])))
    if (status > STATUS_OVER_BUDGET).any():
        raise ValueError("%s: invalid length" % what(int(np.flatnonzero(status > STATUS_OVER_BUDGET)[0])))
    seqs, fscores, scores, lens = host["best_seq"].tolist(), host["frame_score"].tolist(), host["best_score"].tolist(), host["lengths"].tolist()
    out = []
    for st, seq, fs, score, T in zip(status.tolist(), seqs, fscores, scores, lens):
        if st == STATUS_FOUND:
            best_seq = tuple(seq[:T])
            signal, is_zero, start = signal_of(best_seq)
            out.append((signal, is_zero, best_seq, max_possible, score, fs[:T], start))
        else:
            out.append((None, None, None, max_possible, -1, None, None))
    return out


def intensities_to_signal_lognormal(intensities, beta, beta_sigma, max_possible=5, allow_multidrop=True, allow_upsteps=False,
                                    max_deviation=3, quench_factor=0, categories=None, log_fluor_boundaries=None,
                                    log_fluor_means=None, budget=DEFAULT_BUDGET, device=None, solver='enumerate'):
    """MCsimlib._intensities_to_signal_lognormal_v8 on the GPU: (signal, is_zero, best_seq, lmii, best_score,
    best_intensity_scores, starting_intensity).  beta, quench_factor and log_fluor_boundaries are accepted and, as in the
    reference's v8, unused once log_fluor_means is given.  allow_upsteps needs solver='dp'; a winner that steps up comes
    back as (None, None, best_seq, lmii, best_score, best_intensity_scores, best_seq[0]), as there."""
    if categories is None:
        raise ValueError("categories required in v7+")
    if log_fluor_means is None:
        raise ValueError("v8+ requires log_fluor_means to be passed manually")
    _check_solver(solver, allow_upsteps)
    if not allow_multidrop and len(intensities) == 1:
        raise ValueError("max() arg is an empty sequence")        # (max(seq_diff) of a one-frame sequence, :5442)
    host = lognormal_records([intensities], [categories], log_fluor_means, beta_sigma, max_possible, allow_multidrop,
                             max_deviation, budget, device=device, **_solver_kw(solver, allow_upsteps))
    return _fit_tuples(host, max_possible, lambda i: "the track")[0]


def unwind_photometries(photometries):
    """(channel, field, h, w, category, intensities, row) of every track, in the dicts' order (:5560-5564)."""
    for channel, cdict in photometries.items():
        for field, fdict in cdict.items():
            for (h, w), (category, intensities, row) in fdict.items():
                yield (channel, field, h, w, category, intensities, row)


def write_photometries_dict_to_csv(photometries, filepath, dialect='excel'):
    """MCsimlib.write_photometries_dict_to_csv (:5566-5586): one row per track in the dicts' order, the header's frame count
    taken from the first track; returns the number of rows.  Floats are written as Python 2's str() wrote them."""
    import csv
    from .pflib import _py2_str
    with open(filepath, 'w', newline='') as f:
        output_writer = csv.writer(f, dialect=dialect)
        cdict = next(iter(photometries.values()))
        fdict = next(iter(cdict.values()))
        category, intensities, row = next(iter(fdict.values()))
        output_writer.writerow(['CHANNEL', 'FIELD', 'H', 'W', 'CATEGORY'] + ['FRAME ' + str(i) for i in range(len(category))])
        row_counter = 0
        for channel, field, h, w, category, intensities, row in unwind_photometries(photometries):
            output_writer.writerow([str(channel), str(field), str(h), str(w), str(category)] + [_py2_str(i) for i in intensities])
            row_counter += 1
    return row_counter


def photometries_lognormal_fit(photometries, beta, beta_sigma, max_possible=5, num_processes=None, allow_upsteps=False,
                               allow_multidrop=True, max_deviation=3, quench_factor=0, quench_factors=None,
                               budget=DEFAULT_BUDGET, device=None, solver='enumerate'):
    """MCsimlib._photometries_lognormal_fit_MP_v8 (:5496-5558) in one launch: (signals, total_count, none_count, all_fit_info),
    tracks in the nested dict's iteration order (insertion order; Python 2's hash order is not reproduced).  num_processes is
    accepted and unused.  A track over `budget` raises NotImplementedError naming it (never with solver='dp', which allow_upsteps
    needs; a winner that steps up has no signal and counts towards none_count)."""
    if len(photometries) > 1:
        raise NotImplementedError("Currently puts all photometries together, can't handle multiple channels at once.")
    log_fluor_means = _tracks.log_fluor_means(beta, quench_factors, max_possible)
    tracks = list(unwind_photometries(photometries))
    _check_solver(solver, allow_upsteps)
    if not allow_multidrop and any(len(t[5]) == 1 for t in tracks):
        raise ValueError("max() arg is an empty sequence")
    host = lognormal_records([t[5] for t in tracks], [t[4] for t in tracks], log_fluor_means, beta_sigma, max_possible,
                             allow_multidrop, max_deviation, budget, device=device, **_solver_kw(solver, allow_upsteps))
    fits = _fit_tuples(host, max_possible, lambda i: "track %s field %s (%s, %s)" % tracks[i][:4])
    all_fit_info = [(channel, field, h, w, row, category, intensities) + fit
                    for (channel, field, h, w, category, intensities, row), fit in zip(tracks, fits)]
    signals, none_count = _tracks.tally_signals((f[0], f[1], f[6]) for f in fits)
    return signals, len(tracks), none_count, all_fit_info


# ---- host pieces of the chain, with the reference's numpy calls ----

def read_track_photometries_csv(path, downstep_filtered=False, head_truncate=0, tail_truncate=0, omit_header=True, channels=None):
    """MCsimlib.read_track_photometries_csv (:2534-2575): ({channel: {field: {(h, w): (category, frames, row)}}}, {row: ...}).
    Coordinates and intensities are rounded as Python 2 rounds (half away from zero); a frame that reads 'None' raises
    ValueError as float('None') does there."""
    import csv
    d, d2 = {}, {}
    with open(path, newline='') as f:
        for r, row in enumerate(csv.reader(f)):
            if r == 0 and omit_header:
                continue
            (channel, field, h, w, category), frames = row[:5], row[5:]
            if channels is not None and channel not in channels:
                continue
            if h == 'None' or w == 'None':
                continue
            field, h, w = (int(_py2_round(float(x))) for x in (field, h, w))
            cat = tuple(c in ('True,', 'True') for c in category[1:-1].split(' '))
            cat = cat[head_truncate:-tail_truncate] if tail_truncate > 0 else cat[head_truncate:]
            if downstep_filtered and not (tuple(sorted(cat, reverse=True)) == cat and cat[0]):
                continue
            vals = [int(_py2_round(float(x))) for x in frames]
            vals = tuple(vals[head_truncate:-tail_truncate] if tail_truncate > 0 else vals[head_truncate:])
            d.setdefault(channel, {}).setdefault(field, {}).setdefault((h, w), (cat, vals, r))
            d2.setdefault(r, (channel, field, h, w, cat, vals))
    return d, d2


def photometries_from_records(records, channel, downstep_filtered=True, channels=None):
    """The nested dict of read_track_photometries_csv(..., downstep_filtered=..., channels=[channel])[0] straight from
    experiment.sequence_experiment_records' output: what the reader gives on the file experiment.write_track_photometries_csv
    (save_averages=False) writes from the same records.  `channels` renames the channels as there."""
    from . import experiment as _ex
    from . import _native_sequence as NQ
    from . import sequencing as _sq
    names = _ex.channel_names(records, channels)
    F = int(records["shape"][2])
    flags, hw, phot = records["flags"], records["hw"], records["photometry"]
    as_int = str(records["photometry_method"]) == 'simple'
    d, r = {}, 0
    for c, e, members in _ex._ordered_traces(records):
        for t in members:
            r += 1                                                  # (the header is row 0)
            if names[c] != channel:
                continue
            have = (flags[t] & (NQ.DETECTED | NQ.INTERPOLATED)) != 0
            f0 = int(np.flatnonzero(have)[0])
            cat = tuple(bool(x) for x in _sq.pattern_to_tuple(records["category"][t], F))
            if downstep_filtered and not (tuple(sorted(cat, reverse=True)) == cat and cat[0]):
                continue
            vals = tuple(int(_py2_round(int(v) if as_int else v)) if ok else 0
                         for v, ok in zip(phot[t].tolist(), have.tolist()))
            d.setdefault(names[c], {}).setdefault(e, {}).setdefault((int(hw[t, f0, 0]), int(hw[t, f0, 1])), (cat, vals, r))
    return d


def optimal_bin_size(raw_photometries, bin_array=None, device=None):
    """MCsimlib.optimal_bin_size (:3888-3909), Shimazaki & Shinomoto's histogram cost: (min_cost, where, cost_array).  With a
    `device` the costs are computed there, bit for bit the same."""
    lo, hi = min(raw_photometries), max(raw_photometries)
    if bin_array is None:
        bin_array = np.array(range(10, 101))
    if device is not None:
        values = _checked_values(raw_photometries)
        if values.min() != values.max():                           # (all equal: the host route, to end as it always has)
            cost_array = histogram_costs(values, bin_array, device).reshape(-1, 1)
            min_cost = np.amin(cost_array)
            return min_cost, np.where(cost_array == min_cost), cost_array
    bin_size_vector = float(hi - lo) / bin_array
    cost_array = np.zeros(shape=(bin_size_vector.size, 1))
    for i, bin_size in enumerate(bin_size_vector):
        hist, _ = np.histogram(a=raw_photometries, bins=np.linspace(lo, hi, bin_array[i] + 1))
        cost_array[i] = (2.0 * np.mean(hist) - np.var(hist, ddof=0)) / bin_size**2
    min_cost = np.amin(cost_array)
    return min_cost, np.where(cost_array == min_cost), cost_array


def optimal_bin_count(raw_photometries, min_n_bins=10, max_n_bins=1000, device=None):
    """The bin count optimal_bin_size_MP (:3912-3939) settles on, searched in this process: the first bin count with the
    least cost.  (The reference splits the range over its workers and takes the first share with the least cost; it raises
    TypeError where two bin counts of one share tie.)"""
    _, where, _ = optimal_bin_size(raw_photometries, np.array(range(min_n_bins, max_n_bins + 1)), device=device)
    return int(where[0][0]) + min_n_bins


def _get_m0Dm1(raw_photometries, optimal_bin_number=None, device=None):
    """MCsimlib._get_m0Dm1 (:3942-3979): the two highest histogram peaks and the valley between them; [7] is alpha.  `device`:
    where the bin search runs (None: on the host)."""
    n_bins = optimal_bin_count(raw_photometries, 10, 10000, device=device) if optimal_bin_number is None else optimal_bin_number
    hist, bins = np.histogram(a=raw_photometries, bins=n_bins)
    depth_array = np.zeros_like(hist)
    for (gi,), gv in np.ndenumerate(hist):
        if gi == 0 or gi == hist.shape[0] - 1:
            continue
        L_max, R_max = np.amax(hist[:gi]), np.amax(hist[gi + 1:])
        if gv > L_max or gv > R_max:
            continue
        depth_array[gi] = min(L_max, R_max) - gv
    gamma_index, gamma = np.argmax(depth_array), np.amax(depth_array)
    alpha_index, alpha = np.argmax(hist[:gamma_index]), np.amax(hist[:gamma_index])
    beta_index, beta = gamma_index + 1 + np.argmax(hist[gamma_index + 1:]), np.amax(hist[gamma_index + 1:])
    lo, hi = min(raw_photometries), max(raw_photometries)
    mapping_factor = float(hi - lo) / n_bins
    return (n_bins, alpha, alpha_index, beta, beta_index, gamma, gamma_index, lo + mapping_factor * alpha_index,
            lo + mapping_factor * beta_index, lo + mapping_factor * gamma_index)


def _pairwise(seq):
    return zip(seq[:-1], seq[1:])


def last_drop_method_v2(photometries, device=None):
    """MCsimlib.last_drop_method_v2 (:5357-5384): (beta, beta_sigma) from the histogram of log(intensity) at every last ON frame.
    `device`: where the bin search runs (None: on the host)."""
    if len(photometries) > 1:
        raise NotImplementedError("Currently puts all photometries together, can't handle multiple channels at once.")
    last_drop_list = [log(iON) for _, _, _, _, category, intensities, _ in unwind_photometries(photometries)
                      for i, (iON, iOFF) in enumerate(_pairwise(intensities)) if category[i] and not category[i + 1] and iON > 0]
    obn = optimal_bin_count(last_drop_list, device=device)
    hist, bins = np.histogram(a=last_drop_list, bins=obn)
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
    beta_sigma = hwhm / sqrt(2.0 * log(2.0))
    return beta, beta_sigma


def grab_ON_OFFS(all_fit_info, allow_bad_fits=False, alpha_adjust=None):
    """jupyter_development.grab_ON_OFFS (:63-84): {(cycle, field): ((iON, fluors dropped), ...)} of every ON -> OFF step.  As
    there, the alpha_adjust branches are swapped: iON is adjusted only when alpha_adjust is None (and then fails) with good
    fits, and only when it is given with allow_bad_fits."""
    on_offs = {}
    for (channel, field, h, w, row, category, intensities, signal, is_zero, dye_sequence, lmii, total_score, per_frame_scores,
         starting_intensity) in all_fit_info:
        if not allow_bad_fits and dye_sequence is None:
            continue
        for i, (iON, iOFF) in enumerate(_pairwise(intensities)):
            if not (category[i] and not category[i + 1]):
                continue
            if not allow_bad_fits:
                entry = ((iON if alpha_adjust is not None else iON - alpha_adjust), dye_sequence[i] - dye_sequence[i + 1])
            else:
                entry = ((iON - alpha_adjust if alpha_adjust is not None else iON), None)
            on_offs.setdefault((i, field), []).append(entry)
    return {key: tuple(drops) for key, drops in on_offs.items()}


def ON_OFF_adjust_photometries(photometries, ON_OFFS, alpha):
    """jupyter_development.ON_OFF_adjust_photometries (:262-276): every frame but a track's last scaled so that its (cycle,
    field)'s median last-ON intensity becomes the median over all of them."""
    last_beta_dict = {key: np.median([iON for iON, ddiff in drops]) for key, drops in ON_OFFS.items()}
    last_beta_median = float(np.median(list(last_beta_dict.values())))
    adjusted = {}
    for channel, field, h, w, category, intensities, row in unwind_photometries(photometries):
        vals = [(intensity - alpha) * last_beta_median / last_beta_dict[(i, field)]
                if i < len(intensities) - 1 and (i, field) in last_beta_dict else intensity
                for i, intensity in enumerate(intensities)]
        adjusted.setdefault(channel, {}).setdefault(field, {}).setdefault((h, w), (category, tuple(vals), row))
    return adjusted


# ---- the whole chain on a track table: the records route of lognormal_fitter_v2 ----

def _bin_search_device(d_values, min_n_bins, max_n_bins):
    """(the first bin count of least cost over min_n_bins .. max_n_bins, its histogram as an int64 array, lo, hi) of a 1-D
    float64 CUDA tensor, sorted once for both launches; None where all values are equal (the host's case)."""
    torch = _engine._torch()
    d_sorted = _sorted(d_values)
    dev = d_sorted.device
    lo, hi = d_sorted[[0, -1]].tolist()
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError("values must be finite")
    if lo == hi:
        return None
    n = int(d_sorted.numel())
    d_counts = torch.arange(int(min_n_bins), int(max_n_bins) + 1, dtype=torch.int32, device=dev)
    d_cost = torch.empty(int(d_counts.numel()), dtype=torch.float64, device=dev)
    _engine.launch(NB.lib().fsq_histogram_costs, "fsq_histogram_costs", dev, d_sorted.data_ptr(), n, lo, hi, d_counts.data_ptr(),
                   int(d_counts.numel()), d_cost.data_ptr())
    n_bins = int(torch.nonzero(d_cost == d_cost.min())[0]) + int(min_n_bins)
    d_hist = torch.empty(n_bins, dtype=torch.int64, device=dev)
    _engine.launch(NB.lib().fsq_histogram_counts, "fsq_histogram_counts", dev, d_sorted.data_ptr(), n, lo, hi, n_bins, d_hist.data_ptr())
    return n_bins, d_hist.cpu().numpy(), lo, hi


def _beta_device(d_values):
    """last_drop_method_v2's (beta, beta_sigma) of the last-drop values on the device: ValueError for none."""
    if int(d_values.numel()) == 0:
        raise ValueError("min() arg is an empty sequence")         # (optimal_bin_size's min() of an empty last-drop list)
    found = _bin_search_device(d_values, 10, 1000)
    if found is None:
        return HC.beta_of_values(d_values.cpu().numpy())
    n_bins, hist, lo, hi = found
    return HC.beta_of_hist(hist, np.linspace(lo, hi, n_bins + 1))


def _check_chain_tensors(d_intensity, d_category, d_seg_off=None):
    torch = _engine._torch()
    if d_intensity.dim() != 2 or d_category.dim() != 1 or int(d_category.numel()) != int(d_intensity.shape[0]):
        raise ValueError("[n, F] intensities and [n] categories are needed")
    F = int(d_intensity.shape[1])
    if F < 1:
        raise ValueError("at least one frame is needed")
    if F > NC.MAX_FRAMES:
        raise NotImplementedError("tracks are limited to %d frames" % NC.MAX_FRAMES)
    if int(d_intensity.shape[0]) >= 1 << 31:
        raise ValueError("fewer than 2^31 tracks are needed")
    tensors = [d_intensity, d_category] + ([] if d_seg_off is None else [d_seg_off])
    if d_intensity.dtype != torch.float64 or d_category.element_size() != 8 or not all(t.is_contiguous() for t in tensors):
        raise ValueError("contiguous float64 intensities and 64-bit categories are needed")
    if not d_intensity.is_cuda or any(t.device != d_intensity.device for t in tensors):
        raise ValueError("tensors on one GPU are needed")
    if d_seg_off is not None:
        if d_seg_off.dim() != 1 or d_seg_off.numel() < 1 or d_seg_off.dtype != torch.int64:
            raise ValueError("[S + 1] int64 offsets are needed")
        if (int(d_seg_off.numel()) - 1) * max(F - 1, 1) >= 1 << 31:
            raise ValueError("fewer than 2^31 (segment, frame) pairs are needed")


def last_drops_device(d_intensity, d_category, truncate=0):
    """fsq_chain_last_drops on device tensors (float64 [n, F] intensities, 64-bit [n] category words): (values, track_count),
    the float64 log(I) of every frame f >= truncate that is ON before an OFF frame with I > 0, in (track, frame) order, and
    the int64 [n] number of them per track.  Two launches with torch.cumsum between them; the total crosses to the host to size
    `values`."""
    torch = _engine._torch()
    _check_chain_tensors(d_intensity, d_category)
    truncate = int(truncate)
    if truncate < 0:
        raise ValueError("truncate must not be negative")
    truncate = min(truncate, NC.MAX_FRAMES)
    n, F = int(d_intensity.shape[0]), int(d_intensity.shape[1])
    dev = d_intensity.device
    L = NC.lib()
    d_count = torch.empty(n, dtype=torch.int64, device=dev)
    if n == 0:
        return torch.empty(0, dtype=torch.float64, device=dev), d_count
    _engine.launch(L.fsq_chain_last_drops, "fsq_chain_last_drops", dev, d_intensity.data_ptr(), d_category.data_ptr(), n, F, truncate,
                   None, d_count.data_ptr(), None, 0, None, 0)
    d_incl = torch.cumsum(d_count, 0)
    total = int(d_incl[-1])
    d_values = torch.empty(total, dtype=torch.float64, device=dev)
    if total:
        d_off = (d_incl - d_count).contiguous()
        _engine.launch(L.fsq_chain_last_drops, "fsq_chain_last_drops", dev, d_intensity.data_ptr(), d_category.data_ptr(), n, F,
                       truncate, d_off.data_ptr(), None, d_values.data_ptr(), total, None, 0)
    return d_values, d_count


def on_off_medians_device(d_intensity, d_category, d_seg_off, d_status, alpha):
    """fsq_chain_on_off_medians on device tensors: a dict of on_off_median float64 [S, F - 1] (NaN for a key without entries),
    on_off_count int32 [S, F - 1] and last_beta_median float64 [1].  d_status: int32 [n], the first fit's status.  Enqueued on
    the current stream, not synchronised."""
    torch = _engine._torch()
    _check_chain_tensors(d_intensity, d_category, d_seg_off)
    n, F, S = int(d_intensity.shape[0]), int(d_intensity.shape[1]), int(d_seg_off.numel()) - 1
    dev = d_intensity.device
    if d_status.dtype != torch.int32 or d_status.dim() != 1 or int(d_status.numel()) != n or not d_status.is_contiguous() or d_status.device != dev:
        raise ValueError("one contiguous int32 status per track is needed")
    L = NC.lib()
    ws_bytes = L.fsq_chain_on_off_medians_workspace_bytes(n, F, S)
    if ws_bytes < 0:
        raise ValueError("fsq_chain_on_off_medians_workspace_bytes: invalid shape")
    out = {"on_off_median": torch.empty((S, F - 1), dtype=torch.float64, device=dev),
           "on_off_count": torch.empty((S, F - 1), dtype=torch.int32, device=dev),
           "last_beta_median": torch.empty(1, dtype=torch.float64, device=dev)}
    ws = _engine.workspace(dev, ws_bytes)
    _engine.launch(L.fsq_chain_on_off_medians, "fsq_chain_on_off_medians", dev, d_intensity.data_ptr(), d_category.data_ptr(),
                   d_seg_off.data_ptr(), d_status.data_ptr(), n, F, S, float(alpha), out["on_off_median"].data_ptr(),
                   out["on_off_count"].data_ptr(), out["last_beta_median"].data_ptr(), ws.data_ptr(), ws_bytes)
    return out


def on_off_adjust_device(d_intensity, d_seg_off, alpha, medians):
    """fsq_chain_on_off_adjust on device tensors: the adjusted float64 [n, F] of on_off_medians_device's dict."""
    torch = _engine._torch()
    n, F, S = int(d_intensity.shape[0]), int(d_intensity.shape[1]), int(d_seg_off.numel()) - 1
    dev = d_intensity.device
    d_adjusted = torch.empty((n, F), dtype=torch.float64, device=dev)
    _engine.launch(NC.lib().fsq_chain_on_off_adjust, "fsq_chain_on_off_adjust", dev, d_intensity.data_ptr(), d_seg_off.data_ptr(), n, F, S,
                   float(alpha), medians["on_off_median"].data_ptr(), medians["on_off_count"].data_ptr(),
                   medians["last_beta_median"].data_ptr(), d_adjusted.data_ptr(), None, 0)
    return d_adjusted


def _check_fit_status(fit, what):
    """NotImplementedError for a track over the budget (one scalar crosses to the host)."""
    worst = int(fit["status"].max()) if int(fit["status"].numel()) else 0
    if worst >= STATUS_OVER_BUDGET:
        HC.check_status(fit["status"].cpu().numpy(), what)


def chain_device(d_intensity, d_category, d_seg_off, d_field, beta_sigma, max_possible=5, ddif=0.30, allow_multidrop=True,
                 truncate=0, beta=None, no_adjustment=False, budget=DEFAULT_BUDGET, solver='enumerate'):
    """lognormal_fitter_v2.main's computation on a track table on the device: float64 [n, F] intensities, 64-bit [n] category
    words, int64 [S + 1] offsets of the fields' contiguous tracks (d_field, the field number per track, is accepted and not
    needed: the segments say it).  Returns a dict: the scalars alpha, n_bins, original_beta, original_beta_sigma, adj_beta and
    adj_beta_sigma, and the device tensors alpha_adjusted [n, F], adjusted [n, F] (the second fit's input), on_off_median and
    on_off_count [S, F - 1], last_beta_median [1] and fit0, fit1 (lognormal_device's dicts).  Only scalars and histograms of at
    most 10 000 bins cross to the host; where all values of a bin search are equal, that search's values do too.  solver='dp':
    both fits by fsq_lognormal_fit_dp, the same outputs and no track over a budget."""
    torch = _engine._torch()
    _check_solver(solver)
    _check_chain_tensors(d_intensity, d_category, d_seg_off)
    n, F = int(d_intensity.shape[0]), int(d_intensity.shape[1])
    HC.check_frames(F, allow_multidrop)
    if solver == 'dp':
        HD.check_overflow(beta_sigma, F)
    dev = d_intensity.device
    if n == 0:
        raise ValueError("min() arg is an empty sequence")         # (optimal_bin_size's min() of no photometries)
    if not bool(torch.isfinite(d_intensity).all()):
        raise ValueError("intensities must be finite")
    quench = tuple([0.0] + [ddif] * (max_possible + 1))
    d_len = torch.full((n,), F, dtype=torch.int32, device=dev)

    def fit(d_rows, beta_now, what):
        prm = fit_params(_tracks.log_fluor_means(beta_now, quench, max_possible), beta_sigma, max_possible, allow_multidrop, 3, budget)
        out = lognormal_device(d_rows, d_category, d_len, None, None, prm=prm, **_solver_kw(solver))
        _check_fit_status(out, what)
        return out

    found = _bin_search_device(d_intensity.reshape(-1), 10, 10000)
    if found is None:
        alpha, n_bins = HC.alpha_of_values(d_intensity.cpu().numpy())
    else:
        n_bins, hist, lo, hi = found
        alpha = HC.alpha_of_hist(hist, n_bins, np.float64(lo), np.float64(hi))
    original_beta, original_beta_sigma = _beta_device(last_drops_device(d_intensity, d_category, truncate)[0])
    if beta is not None:
        original_beta = beta
    d_alpha_adjusted = d_intensity - float(alpha)
    if not bool(torch.isfinite(d_alpha_adjusted).all()):
        raise ValueError("intensities must be finite")
    fit0 = fit(d_alpha_adjusted, original_beta, "the first fit")
    medians = on_off_medians_device(d_intensity, d_category, d_seg_off, fit0["status"], alpha)
    d_adjusted = d_alpha_adjusted if no_adjustment else on_off_adjust_device(d_intensity, d_seg_off, alpha, medians)
    if not bool(torch.isfinite(d_adjusted).all()):
        raise ValueError("an adjusted intensity is not finite")
    adj_beta, adj_beta_sigma = _beta_device(last_drops_device(d_adjusted, d_category, 0)[0])
    if beta is not None:
        adj_beta = beta
    fit1 = fit(d_adjusted, adj_beta, "the second fit")
    return dict(alpha=alpha, n_bins=n_bins, original_beta=original_beta, original_beta_sigma=original_beta_sigma, adj_beta=adj_beta,
                adj_beta_sigma=adj_beta_sigma, alpha_adjusted=d_alpha_adjusted, adjusted=d_adjusted, fit0=fit0, fit1=fit1, **medians)


def tally_device(fit, d_order=None):
    """(signals, total_count, none_count) of a fit on the device, the keys in the order of each one's first track
    (_tracks.tally_signals' insertion order): torch.unique over the winning rows and the first index of every unique row;
    only the unique rows reach Python.  d_order: the caller's index of every track (default: as they stand)."""
    torch = _engine._torch()
    status, best_seq = fit["status"], fit["best_seq"]
    total = int(status.numel())
    where = torch.nonzero(status == STATUS_FOUND).reshape(-1)
    if int(where.numel()) == 0:
        return {}, total, total
    rows, inverse, counts = torch.unique(best_seq[where], dim=0, return_inverse=True, return_counts=True)
    index = where if d_order is None else d_order[where]
    first = torch.full((int(rows.shape[0]),), total, dtype=torch.int64, device=status.device)
    first.scatter_reduce_(0, inverse.reshape(-1), index.to(torch.int64), reduce="amin")
    return HC.tally_rows(rows.cpu().tolist(), first.cpu().tolist(), counts.cpu().tolist(), total)


def _grouped_by_first_appearance(fields):
    """(order, field ids, seg_off, segment per track) of one field per track: a stable grouping, the fields in the order of
    their first track."""
    fields = np.asarray(fields).reshape(-1)
    ids, first, inverse = np.unique(fields, return_index=True, return_inverse=True)
    by_first = np.argsort(first, kind='stable')
    rank = np.empty(len(ids), np.int64)
    rank[by_first] = np.arange(len(ids))
    segment = rank[inverse.reshape(-1)]
    order = np.argsort(segment, kind='stable')
    seg_off = np.zeros(len(ids) + 1, np.int64)
    np.cumsum(np.bincount(segment, minlength=len(ids)), out=seg_off[1:])
    return order, ids[by_first], seg_off, segment


def chain_records(intensities, categories, fields, beta_sigma, max_possible=5, ddif=0.30, allow_multidrop=True, truncate=0,
                  beta=None, no_adjustment=False, budget=DEFAULT_BUDGET, device=None, host=False, solver='enumerate'):
    """The chain for a track table on the host, as arrays: intensities, sequences of one length or a [n, F] array; categories,
    tuples of F booleans or the uint64 words; fields, one integer per track.  Tracks may come in any order: they are grouped by
    field, stably, the fields in the order of their first track, and everything per track comes back in the caller's order.
    Returns chain_device's dict as NumPy arrays (fit0 and fit1 dicts of arrays) with field_ids (one per row of on_off_median
    and on_off_count), segment (the row of every track's field), signals, total_count and none_count of the second fit.
    host=True: with numpy on the host (_host_lognormal_chain), no GPU needed.  solver='dp': both fits by the dynamic programme
    (on the host by its twin), the same outputs and no track over a budget."""
    _check_solver(solver)
    two_d = isinstance(intensities, np.ndarray) and intensities.ndim == 2
    seqs = intensities if two_d else [np.asarray(s, dtype=np.float64).reshape(-1) for s in intensities]
    F = seqs.shape[1] if two_d else len(seqs[0]) if len(seqs) else 1
    HC.check_frames(F, allow_multidrop)
    if solver == 'dp':
        HD.check_overflow(beta_sigma, F)
    rows, _ = _tracks.pack_rows(seqs, width=F, width_error="every track needs exactly %d intensities" % F)
    n = len(rows)
    if not np.isfinite(rows).all():
        raise ValueError("intensities must be finite")
    cats = _tracks.category_words(categories, n, F)
    order, field_ids, seg_off, segment = _grouped_by_first_appearance(fields)
    if len(segment) != n:
        raise ValueError("one field per track")
    if n == 0:
        raise ValueError("min() arg is an empty sequence")         # (optimal_bin_size's min() of no photometries)
    kw = dict(beta_sigma=beta_sigma, max_possible=max_possible, ddif=ddif, allow_multidrop=allow_multidrop, truncate=truncate,
              beta=beta, no_adjustment=no_adjustment, budget=budget, **({} if solver == 'enumerate' else {"solver": solver}))
    g_rows, g_cats = np.ascontiguousarray(rows[order]), np.ascontiguousarray(cats[order])
    if host:
        out = HC.chain(g_rows, g_cats, seg_off, **kw)
        signals = None
    else:
        torch = _engine._torch()
        dev = torch.device(device or "cuda")
        d_out = chain_device(torch.from_numpy(g_rows).to(dev), torch.from_numpy(g_cats.view(np.int64)).to(dev),
                             torch.from_numpy(seg_off).to(dev), None, **kw)
        signals = tally_device(d_out["fit1"], torch.from_numpy(order).to(dev))
        out = {k: (_engine.to_host(v) if isinstance(v, dict) else v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in d_out.items()}
        out["last_beta_median"] = float(out["last_beta_median"][0])

    def back(a):
        b = np.empty_like(a)
        b[order] = a
        return b
    for k in ("alpha_adjusted", "adjusted"):
        out[k] = back(out[k])
    for k in ("fit0", "fit1"):
        out[k] = {name: back(a) for name, a in out[k].items()}
    if signals is None:
        signals = HC.tally(out["fit1"]["status"], out["fit1"]["best_seq"])
    out["signals"], out["total_count"], out["none_count"] = signals
    out["field_ids"], out["segment"] = field_ids, segment
    return out


def track_table_from_photometries(photometries):
    """The nested dict of one channel as a track table in unwind_photometries' order: (intensity float64 [n, F], category
    uint64 [n], field int64 [n], hw int64 [n, 2], row int64 [n]).  Every track needs the first one's number of frames
    (ValueError)."""
    if len(photometries) > 1:
        raise NotImplementedError("Currently puts all photometries together, can't handle multiple channels at once.")
    tracks = list(unwind_photometries(photometries))
    n = len(tracks)
    F = len(tracks[0][5]) if n else 0
    if any(len(t[5]) != F or len(t[4]) != F for t in tracks):
        raise ValueError("every track needs exactly %d intensities and category entries" % F)
    intensity = np.array([t[5] for t in tracks], dtype=np.float64).reshape(n, F)
    return (intensity, _tracks.category_words([t[4] for t in tracks], n), np.array([t[1] for t in tracks], dtype=np.int64),
            np.array([(t[2], t[3]) for t in tracks], dtype=np.int64).reshape(n, 2), np.array([t[6] for t in tracks], dtype=np.int64))


def track_table_from_records(records, channel, downstep_filtered=True, channels=None):
    """track_table_from_photometries(photometries_from_records(records, channel, downstep_filtered, channels)) without the
    dict: the same table straight from experiment.sequence_experiment_records' output, with array operations only."""
    from . import experiment as _ex
    from . import _native_sequence as NQ
    names = _ex.channel_names(records, channels)
    C, F = int(records["shape"][1]), int(records["shape"][2])
    seq, cat = np.asarray(records["trace_seq"]).astype(np.int64), np.asarray(records["category"]).astype(np.uint64)
    t = np.flatnonzero(_ex._staying(records))
    # the order of the written file: channels, fields ascending, categories in order of first appearance, traces as tracked
    _, group = np.unique(np.stack([seq[t].astype(np.uint64), cat[t]]), axis=1, return_inverse=True)
    group = group.reshape(-1)
    first = np.full(int(group.max()) + 1 if len(t) else 0, len(seq), np.int64)
    np.minimum.at(first, group, t)
    t = t[np.lexsort((t, first[group], seq[t] // C, seq[t] % C))]
    row = np.arange(1, len(t) + 1, dtype=np.int64)                  # (the header is row 0)
    mask = np.uint64(0xFFFFFFFFFFFFFFFF) if F >= 64 else np.uint64((1 << F) - 1)
    word = cat[t] & mask
    keep = np.isin(seq[t] % C, [c for c in range(C) if names[c] == channel])
    if downstep_filtered:
        keep &= ((word & (word + np.uint64(1))) == 0) & ((word & np.uint64(1)) == 1)       # ON in a prefix of the frames, from frame 0
    t, row, word = t[keep], row[keep], word[keep]
    have = (np.asarray(records["flags"])[t] & (NQ.DETECTED | NQ.INTERPOLATED)) != 0
    if len(t) and not have.any(axis=1).all():
        raise IndexError("index 0 is out of bounds for axis 0 with size 0")      # (a trace without a frame, as the dict route)
    f0 = np.argmax(have, axis=1)
    hw = np.asarray(records["hw"])[t, f0].astype(np.int64).reshape(len(t), 2)
    v = np.where(have, np.asarray(records["photometry"], dtype=np.float64)[t], 0.0)
    if str(records["photometry_method"]) == 'simple':
        v = np.trunc(v)
    intensity = np.where(have, np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5)), 0.0)         # (_py2_round)
    field = seq[t] // C
    # a later track at a (field, h, w) that an earlier one holds is dropped, as the dict's setdefault drops it
    _, first_at = np.unique(np.stack([field, hw[:, 0], hw[:, 1]]), axis=1, return_index=True)
    sel = np.sort(first_at)
    return intensity[sel].reshape(len(sel), F), word[sel], field[sel], hw[sel], row[sel]
