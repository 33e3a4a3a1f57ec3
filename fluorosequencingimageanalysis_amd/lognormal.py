"""Lognormal fluor-count fitting of track photometries on the GPU: the reference's lognormal_fitter_v2 chain.

The fit itself - MCsimlib._intensities_to_signal_lognormal_v8 (:5387-5493), the most expensive per-track step of the chain -
runs on the device, one wavefront per track and one launch for a whole experiment (`lognormal_device`, `lognormal_records`,
`photometries_lognormal_fit`; include/fsq_lognormal.h).  The host pieces of the chain (the CSV reader, the histogram bin
search, alpha, beta, the ON/OFF adjustment) are restated here with the reference's own numpy calls.  The bin search, 9 991
histograms of all photometries for alpha alone, also runs on the device with numpy's bits (`histogram_costs_device`,
`bin_search_records`, `histogram_counts`; include/fsq_binsearch.h): `optimal_bin_size`, `optimal_bin_count`, `_get_m0Dm1` and
`last_drop_method_v2` take it with `device=...` and stay on the host with `device=None`.

Limits of the device fit, each raised on the host before anything is launched: 1 .. 64 frames per track
(NotImplementedError above 64, ValueError for none), max_possible in 1 .. 15 (NotImplementedError above), beta_sigma finite
and > 0, max_deviation not NaN, finite intensities and finite log_fluor_means (ValueError); allow_upsteps=True is not built
(NotImplementedError; the command line never passes it).  A track with more surviving sequences than `budget` (default 2^22)
is not enumerated: it comes back with STATUS_OVER_BUDGET from the array interfaces and raises NotImplementedError naming the
track from the dict interfaces.

Limits of the device bin search, each raised as ValueError on the host before anything is launched: at least one value, finite
values, integers of magnitude at most 2^53 (beyond it float64 does not hold them), bin counts in 1 .. 10 000
(FSQ_BINSEARCH_MAX_BINS), fewer than 2^31 values.  Where all values are equal the search runs on the host whatever `device` is,
and ends as it ends there."""
import ctypes
import math
from math import log, sqrt

import numpy as np

from . import _native_binsearch as NB
from . import _native_lognormal as NL
from . import _tracks
from . import engine as _engine
from ._tracks import category_word                                # noqa: F401  (its old place)
from .pflib import _py2_round

STATUS_FOUND, STATUS_NONE, STATUS_OVER_BUDGET = NL.STATUS_FOUND, NL.STATUS_NONE, NL.STATUS_OVER_BUDGET
DEFAULT_BUDGET = NL.DEFAULT_BUDGET
MAX_BINS = NB.MAX_BINS


# ---- the device fit ----

def _no_upsteps(allow_upsteps):
    if allow_upsteps:
        raise NotImplementedError("allow_upsteps=True is not built")


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
                     max_deviation=3, budget=DEFAULT_BUDGET, prm=None):
    """fsq_lognormal_fit on device tensors: float64 [n, max_frames] intensities, int64 [n] categories (bit f set when frame f
    is ON, the uint64 word of sequencing.py) and int32 [n] lengths.  Returns a dict of device tensors: status int32 [n], best_seq
    uint8 [n, max_frames], best_score float64 [n], frame_score float64 [n, max_frames], n_surviving int64 [n].  Enqueued on the
    current stream, not synchronised.  Lengths and intensities are not checked here: a track whose length is not in
    1 .. max_frames comes back with status 3.  `prm`: the parameters already built by fit_params (the other arguments are then unused)."""
    torch = _engine._torch()
    if prm is None:
        prm = fit_params(log_fluor_means, beta_sigma, max_possible, allow_multidrop, max_deviation, budget)
    dev = d_intensity.device
    n, max_frames = int(d_intensity.shape[0]), int(d_intensity.shape[1])
    if max_frames > NL.MAX_FRAMES:
        raise NotImplementedError("tracks are limited to %d frames" % NL.MAX_FRAMES)
    L = NL.lib()
    ws_bytes = L.fsq_lognormal_workspace_bytes(n, max_frames)
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
    _engine.launch(L.fsq_lognormal_fit, "fsq_lognormal_fit", dev, d_intensity.data_ptr(), d_category.data_ptr(), d_len.data_ptr(), n,
                   max_frames, ctypes.byref(prm), out["status"].data_ptr(), out["best_seq"].data_ptr(), out["best_score"].data_ptr(),
                   out["frame_score"].data_ptr(), out["n_surviving"].data_ptr(), None, 0)
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
                      max_deviation=3, budget=DEFAULT_BUDGET, lengths=None, device=None):
    """The fit for many tracks in one launch, as arrays.

    intensities  ragged sequences, a float64 [n, max_frames] array or a CUDA tensor of that shape (with `lengths`, or every
                 row full); categories  tuples of booleans, or the uint64 / int64 words as an array or CUDA tensor.
    Returns a dict of NumPy arrays: status (STATUS_FOUND / STATUS_NONE / STATUS_OVER_BUDGET), best_seq uint8 [n, max_frames],
    best_score, frame_score [n, max_frames], n_surviving int64 and lengths.  Rows beyond a track's length, and the rows of
    a track without a winner, hold count 0, score 0 and best_score -1."""
    prm = fit_params(log_fluor_means, beta_sigma, max_possible, allow_multidrop, max_deviation, budget)
    if hasattr(intensities, "is_cuda"):                            # a torch tensor
        torch = _engine._torch()
        d_int = intensities.contiguous()
        n, F = int(d_int.shape[0]), int(d_int.shape[1])
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
        if n:
            torch = _engine._torch()
            dev = torch.device(device or "cuda")
            d_int, d_len = torch.from_numpy(rows).to(dev), torch.from_numpy(lens).to(dev)
            d_cat = torch.from_numpy(cats.view(np.int64)).to(dev)
    if n == 0:
        return {"status": np.zeros(0, np.int32), "best_seq": np.zeros((0, 1), np.uint8), "best_score": np.zeros(0),
                "frame_score": np.zeros((0, 1)), "n_surviving": np.zeros(0, np.int64), "lengths": np.zeros(0, np.int32)}
    out = lognormal_device(d_int, d_cat, d_len, None, None, prm=prm)
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
                                    log_fluor_means=None, budget=DEFAULT_BUDGET, device=None):
    """MCsimlib._intensities_to_signal_lognormal_v8 on the GPU: (signal, is_zero, best_seq, lmii, best_score,
    best_intensity_scores, starting_intensity).  beta, quench_factor and log_fluor_boundaries are accepted and, as in the
    reference's v8, unused once log_fluor_means is given."""
    if categories is None:
        raise ValueError("categories required in v7+")
    if log_fluor_means is None:
        raise ValueError("v8+ requires log_fluor_means to be passed manually")
    _no_upsteps(allow_upsteps)
    if not allow_multidrop and len(intensities) == 1:
        raise ValueError("max() arg is an empty sequence")        # (max(seq_diff) of a one-frame sequence, :5442)
    host = lognormal_records([intensities], [categories], log_fluor_means, beta_sigma, max_possible, allow_multidrop,
                             max_deviation, budget, device=device)
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
                               budget=DEFAULT_BUDGET, device=None):
    """MCsimlib._photometries_lognormal_fit_MP_v8 (:5496-5558) in one launch: (signals, total_count, none_count, all_fit_info),
    tracks in the nested dict's iteration order (insertion order; Python 2's hash order is not reproduced).  num_processes is
    accepted and unused.  A track over `budget` raises NotImplementedError naming it."""
    if len(photometries) > 1:
        raise NotImplementedError("Currently puts all photometries together, can't handle multiple channels at once.")
    log_fluor_means = _tracks.log_fluor_means(beta, quench_factors, max_possible)
    tracks = list(unwind_photometries(photometries))
    _no_upsteps(allow_upsteps)
    if not allow_multidrop and any(len(t[5]) == 1 for t in tracks):
        raise ValueError("max() arg is an empty sequence")
    host = lognormal_records([t[5] for t in tracks], [t[4] for t in tracks], log_fluor_means, beta_sigma, max_possible,
                             allow_multidrop, max_deviation, budget, device=device)
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
