"""Step fitting of spot photometry traces on the GPU (include/fsq_stepfit.h): the live path of the reference's
Trace.stepfit_photometries (flexlibrary.py:1380-1462) through stepfitting_library, for many traces in one launch.

stepfit_records is the fast path (flat arrays, no Python object per plateau); stepfit_photometries returns the reference's
4-tuple per trace.  sliding_t_fitter, chung_kennedy_filter, t_test_filter, refit_plateaus and the mirror helpers are
drop-ins with the reference's names and defaults.

chi_squared_step_fitter, filter_upsteps, filter_small_steps and stepfit_r_squared (include/fsq_chisq.h) are drop-ins as well;
chisq_records / chisq_device fit many traces in one launch.

Trace and the plateau / step list helpers (plateau_value, plateaus_to_steps, last_step_info, frame_plateau, plateau_starts)
are the host-side surface save_experiment_as_csv is written against; timetrace.py computes the same table for whole
experiments on the GPU."""
import ctypes
import math

import numpy as np

from . import _native_chisq as NC
from . import _native_stepfit as NS
from . import _tracks
from . import engine as _engine

CK_WINDOW_LENGTHS = (2, 4, 8, 16)     # the live path's CK windows (flexlibrary.py:1436)
LIVE_WINDOW_RADIUS = 6                 # flexlibrary.py:1439


def _pow2(v):
    """`v ** 2` of the reference's Python 2 / numpy scalars: libm's pow(v, 2.0), inf where that overflows."""
    try:
        return math.pow(v, 2.0)
    except OverflowError:
        return math.inf


class Trace(object):
    """flexlibrary.Trace (flexlibrary.py:1320-1514) without the step fit itself (stepfit_photometries above takes whole
    batches): what TimetraceExperiment.save_experiment_as_csv asks of a trace.  Subclasses define photometry(frame)."""

    def photometry(self, **kwargs):
        raise AttributeError("Every Trace subclass must implement its own photometry() method")

    def photometries(self, photometry_min=None, photometry_method='mexican_hat', **kwargs):
        """The photometries of every Spot of self.trace as a tuple; a None counts the int 0; values below photometry_min
        are raised to it."""
        out = [spot.photometry(method=photometry_method, **kwargs) if spot is not None else 0 for spot in self.trace]
        if photometry_min is not None:
            out = [max(photometry_min, v) for v in out]
        return tuple(out)

    def frame_output(self, frame, **kwargs):
        return self.photometry(frame, **kwargs)

    @staticmethod
    def trace_comparison_rss(trace_A, trace_B, photometry_method='mexican_hat', **kwargs):
        """Left-to-right sum over the frames of (A.photometry(f) - B.photometry(f)) ** 2."""
        if trace_A.num_frames != trace_B.num_frames:
            raise Exception("trace_A and trace_B must cover an identical number of frames for comparison to be valid.")
        return sum([_pow2(trace_A.photometry(frame=f, photometry_method=photometry_method, **kwargs) -
                          trace_B.photometry(frame=f, photometry_method=photometry_method, **kwargs))
                    for f in range(trace_A.num_frames)])

    def total_sum_squares(self, photometry_method='mexican_hat', **kwargs):
        photometries = self.photometries(photometry_min=None, photometry_method=photometry_method, **kwargs)
        photometry_mean = float(np.mean(photometries))
        return sum(_pow2(p - photometry_mean) for p in photometries)

    @staticmethod
    def coefficient_of_determination(trace_A, trace_B, photometry_method='mexican_hat', **kwargs):
        """1 - rss / tss of trace_B's photometries as a fit of trace_A's (ZeroDivisionError for a constant trace_A)."""
        rss = float(Trace.trace_comparison_rss(trace_A, trace_B, photometry_method=photometry_method, **kwargs))
        tss = float(trace_A.total_sum_squares(photometry_method=photometry_method, **kwargs))
        return 1.0 - rss / tss


class PhotometryTrace(Trace):
    """flexlibrary.PhotometryTrace (flexlibrary.py:1595-1611): a sequence of photometries at (h, w)."""

    def __init__(self, trace, h, w):
        self.trace = trace
        self.h, self.w = h, w
        self.num_frames = len(trace)

    def photometry(self, frame, **kwargs):
        return self.trace[frame]

    def plateau_starts(self):
        return set(range(self.num_frames))


class PlateauTrace(Trace):
    """flexlibrary.PlateauTrace (flexlibrary.py:1630-1662): a list of (start, stop, height) plateaus at (h, w)."""

    def __init__(self, trace, h, w):
        self.trace = trace
        self.h, self.w = h, w
        self.num_frames = trace[-1][1] + 1 if len(trace) > 0 else 0

    def photometry(self, frame, **kwargs):
        return plateau_value(self.trace, frame)

    def last_step_info(self, frame):
        """stepfitting_library.last_step_info of the PLATEAUS, as the reference calls it (flexlibrary.py:1652): in plateau
        k >= 1 that is (k - 1, start_{k-1}, h_{k-1}), not a step's number and magnitude."""
        return last_step_info(self.trace, frame)

    def frame_plateau(self, frame):
        return frame_plateau(self.trace, frame)

    def plateau_starts(self):
        return plateau_starts(self.trace)


# ---- plateau and step lists (stepfitting_library.py:508-529, :594-676, :1749) --------------------------------------------
def plateau_value(plateaus, frame):
    """Height of the first plateau that holds frame; ValueError when none does."""
    for start, stop, height in plateaus:
        if start <= frame <= stop:
            return height
    raise ValueError("frame " + str(frame) + " is outside of plateaus " + str(plateaus))


def plateaus_to_steps(plateaus):
    """[(stop_A, start_B, height_B - height_A)] for every pair of neighbouring plateaus."""
    return [(a[1], b[0], b[2] - a[2]) for a, b in zip(plateaus[:-1], plateaus[1:])]


def last_step_info(steps, frame):
    """(number, pre-step frame, magnitude) of the last step (pre_frame, post_frame, magnitude) before frame: the first step
    whose post_frame <= frame <= the next step's pre_frame, else the last step if frame >= its pre_frame, else three Nones."""
    if frame < 0:
        raise ValueError("frame must be a positive integer.")
    for s in range(len(steps) - 1):
        if steps[s][1] <= frame <= steps[s + 1][0]:
            return s, steps[s][0], steps[s][2]
    if len(steps) and frame >= steps[-1][0]:
        return len(steps) - 1, steps[-1][0], steps[-1][2]
    return None, None, None


def frame_plateau(plateaus, frame):
    """((start, stop, height), index) of the first plateau that holds frame, else ((None, None, None), None)."""
    for p, (start, stop, height) in enumerate(plateaus):
        if start <= frame <= stop:
            return (start, stop, height), p
    return (None, None, None), None


def plateau_starts(plateaus):
    return set(start for start, _stop, _height in plateaus)


def _as_rows(photometries, photometry_min):
    """Photometry sequences -> (float64 [n, max_frames] host rows, int32 lengths).  None frames count 0."""
    # (the reference's plateau comparisons depend on object identity with NaN heights: no pinnable result)
    return _tracks.pack_rows(photometries, none_is_zero=True, min_frames=1,
                             short_error="every photometry trace needs at least one frame",
                             nan_error="trace %d holds a NaN photometry; pass photometry_min to clamp it" if photometry_min is None else None)


def _params(mirror_start, chung_kennedy, p_threshold, photometry_min, window_radius=LIVE_WINDOW_RADIUS, drop_sort=True,
            window_lengths=CK_WINDOW_LENGTHS, M=10, p=2):
    if int(mirror_start) < 0:
        raise ValueError("mirror_size must be greater than 0.")
    if p != 2:
        raise NotImplementedError("chung_kennedy_filter: only p = 2 is built")
    wl = tuple(int(w) for w in window_lengths)
    if chung_kennedy > 0 and not (1 <= len(wl) <= NS.MAX_WINDOWS and all(1 <= w <= 64 for w in wl) and 1 <= M <= 64):
        raise NotImplementedError("chung_kennedy_filter: at most %d window lengths in 1..64 and M in 1..64" % NS.MAX_WINDOWS)
    if not 0 <= int(window_radius) <= 64:
        raise NotImplementedError("sliding_t_fitter: window_radius above 64 is not built")
    prm = NS.FsqStepfitParams()
    prm.mirror_start = int(mirror_start)
    prm.chung_kennedy = int(chung_kennedy)
    prm.n_windows = len(wl)
    for k, w in enumerate(wl[:NS.MAX_WINDOWS]):
        prm.window_lengths[k] = w
    prm.M, prm.p = int(M), int(p)
    prm.window_radius = int(window_radius)
    prm.drop_sort = 1 if drop_sort else 0
    prm.p_threshold = float(p_threshold)
    prm.has_photometry_min = 0 if photometry_min is None else 1
    prm.photometry_min = 0.0 if photometry_min is None else float(photometry_min)
    return prm


def _check_lengths(lens, prm):
    mirrored = lens + np.minimum(lens, prm.mirror_start)
    if len(lens) and mirrored.max() > NS.MAX_MIRRORED:
        raise ValueError("traces are limited to %d frames after mirroring" % NS.MAX_MIRRORED)
    if prm.chung_kennedy > 0 and len(lens) and mirrored.min() <= 2:
        raise ValueError("luminosities must have len(luminosities) > 2 for the Chung-Kennedy filter")


def _plateau_out(n, max_frames, dev, zero, keys=("start", "stop", "height", "count")):
    """The output tensors of one plateau list per trace under `keys`: zeros, or uninitialised where every row is written."""
    torch = _engine._torch()
    alloc = torch.zeros if zero else torch.empty
    rows = [alloc((n, max_frames), dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.float64)]
    return dict(zip(keys, rows + [alloc(n, dtype=torch.int32, device=dev)]))


def run_device(d_phot, d_len, max_frames, prm, want_p=False, pair_cap=0):
    """fsq_stepfit_traces on device tensors (float64 [n, max_frames], int32 [n]); returns a dict of device tensors:
    ck, pl_start, pl_stop, pl_h, pl_n, tf_start, tf_stop, tf_h, tf_n, status (and p when want_p; pair_p [n, pair_cap] and
    pair_n, the t-filter pair tests, when pair_cap > 0).  Enqueued on the current stream, not synchronised.  Lengths are not
    checked here: invalid traces come back with status 2."""
    torch = _engine._torch()
    dev = d_phot.device
    n = int(d_phot.shape[0])
    L = NS.lib()
    ws_bytes = L.fsq_stepfit_workspace_bytes(n, int(max_frames), ctypes.byref(prm))
    if ws_bytes < 0:
        raise ValueError("fsq_stepfit_workspace_bytes: invalid parameters")
    Lmax = max_frames + min(prm.mirror_start, max_frames)
    n_radii = max(prm.window_radius - 5, 0)
    out = {"ck": torch.empty((n, max_frames), dtype=torch.float64, device=dev)}
    for pre in ("pl", "tf"):
        out.update(_plateau_out(n, max_frames, dev, False, (pre + "_start", pre + "_stop", pre + "_h", pre + "_n")))
    out["status"] = torch.empty(n, dtype=torch.int32, device=dev)
    if want_p:
        out["p"] = torch.empty((n, n_radii, Lmax), dtype=torch.float64, device=dev)
    if pair_cap > 0:
        out["pair_p"] = torch.empty((n, pair_cap), dtype=torch.float64, device=dev)
        out["pair_n"] = torch.empty(n, dtype=torch.int32, device=dev)
    ws = _engine.workspace(dev, ws_bytes)
    o = out
    _engine.launch(L.fsq_stepfit_traces, "fsq_stepfit_traces", dev, d_phot.data_ptr(), d_len.data_ptr(), n, int(max_frames),
                   ctypes.byref(prm), o["ck"].data_ptr(), o["pl_start"].data_ptr(), o["pl_stop"].data_ptr(), o["pl_h"].data_ptr(),
                   o["pl_n"].data_ptr(), o["tf_start"].data_ptr(), o["tf_stop"].data_ptr(), o["tf_h"].data_ptr(), o["tf_n"].data_ptr(),
                   o["status"].data_ptr(), o["p"].data_ptr() if want_p else None, o["pair_p"].data_ptr() if pair_cap > 0 else None,
                   o["pair_n"].data_ptr() if pair_cap > 0 else None, int(pair_cap), ws.data_ptr(), int(ws_bytes))
    out["_ws"] = ws                   # (kept alive until the caller has read the outputs)
    return out


def raise_for_fit_status(st):
    """run_device's status words as the exception of the first trace that has one."""
    if (st == NS.STATUS_UNSUPPORTED).any():
        raise NotImplementedError("trace %d: a t-filter pass sorts >= 64 plateau pairs with a NaN p (CPython's merge sort order "
                                  "is not restated)" % int(np.flatnonzero(st == NS.STATUS_UNSUPPORTED)[0]))
    if (st != NS.STATUS_OK).any():
        raise ValueError("trace %d: invalid length" % int(np.flatnonzero(st != NS.STATUS_OK)[0]))


def _run(photometries, mirror_start, chung_kennedy, p_threshold, photometry_min, want_p=False, device=None, **kw):
    prm = _params(mirror_start, chung_kennedy, p_threshold, photometry_min, **kw)
    rows, lens = _as_rows(photometries, photometry_min)
    _check_lengths(lens, prm)
    if len(lens) == 0:
        return None, lens, prm
    torch = _engine._torch()
    dev = torch.device(device or "cuda")
    host = _engine.to_host(run_device(torch.from_numpy(rows).to(dev), torch.from_numpy(lens).to(dev), rows.shape[1], prm, want_p=want_p))
    raise_for_fit_status(host["status"])
    host["rows"], host["lens"] = rows, lens
    return host, lens, prm


def _flat(start, stop, height, count):
    """Plateau rows [n, max_frames] and counts [n] -> one entry per plateau, in trace order."""
    cnt = count.astype(np.int64)
    mask = np.arange(start.shape[1])[None, :] < cnt[:, None]
    return {"trace": np.nonzero(mask)[0].astype(np.int64), "start": start[mask], "stop": stop[mask], "height": height[mask],
            "counts": cnt}


def _flat_empty():
    return _flat(np.zeros((0, 1), np.int32), np.zeros((0, 1), np.int32), np.zeros((0, 1)), np.zeros(0, np.int32))


def _plateau_tuples(start, stop, height):
    """The reference's (start, stop, height) plateaus: Python ints and np.float64 heights."""
    return [(s, o, np.float64(h)) for s, o, h in zip(start.tolist(), stop.tolist(), height)]


def stepfit_records(photometries, mirror_start=0, chung_kennedy=0, p_threshold=0.01, photometry_min=None, device=None):
    """Trace.stepfit_photometries for many traces, as flat arrays.

    Returns a dict: "plateaus" and "t_filtered_plateaus", each {"trace", "start", "stop", "height", "counts"} (one entry per
    plateau, in trace order; counts per trace), "ck_filtered" (float64 [n, max_frames], row t valid for its own length)
    and "lengths"."""
    host, lens, prm = _run(photometries, mirror_start, chung_kennedy, p_threshold, photometry_min, device=device)
    if host is None:
        return {"plateaus": _flat_empty(), "t_filtered_plateaus": _flat_empty(), "ck_filtered": np.zeros((0, 1)), "lengths": lens}
    flat = {pre: _flat(host[pre + "_start"], host[pre + "_stop"], host[pre + "_h"], host[pre + "_n"]) for pre in ("pl", "tf")}
    return {"plateaus": flat["pl"], "t_filtered_plateaus": flat["tf"], "ck_filtered": host["ck"], "lengths": lens}


def _plateau_lists(host, pre, i):
    n = int(host[pre + "_n"][i])
    return _plateau_tuples(host[pre + "_start"][i, :n], host[pre + "_stop"][i, :n], host[pre + "_h"][i, :n])


def stepfit_photometries(photometries, mirror_start=0, chung_kennedy=0, p_threshold=0.01, photometry_min=None, keys=None,
                         device=None):
    """Trace.stepfit_photometries (flexlibrary.py:1380-1462) for every sequence of `photometries` (a 2-D array or a list of
    ragged sequences).  Returns one (photometries, ck_filtered_photometries, plateaus, t_filtered_plateaus) tuple per trace:
    PhotometryTrace, PhotometryTrace, PlateauTrace, PlateauTrace, at keys[i] = (h, w) (None when keys is None)."""
    host, lens, prm = _run(photometries, mirror_start, chung_kennedy, p_threshold, photometry_min, device=device)
    if host is None:
        return []
    if keys is not None and len(keys) != len(lens):
        raise ValueError("keys must hold one (h, w) per trace")
    res = []
    rows, ck = host["rows"], host["ck"]
    m = int(mirror_start)
    for i, n in enumerate(lens.tolist()):
        h, w = keys[i] if keys is not None else (None, None)
        ph = rows[i, :n]
        if photometry_min is not None:
            ph = np.where(ph > photometry_min, ph, photometry_min)
        nck = max(n + min(m, n) - m, 0)
        res.append((PhotometryTrace(tuple(ph.tolist()), h, w), PhotometryTrace(ck[i, :nck].tolist(), h, w),
                    PlateauTrace(_plateau_lists(host, "pl", i), h, w), PlateauTrace(_plateau_lists(host, "tf", i), h, w)))
    return res


# ---- drop-ins of stepfitting_library ----------------------------------------------------------------------------------
def sliding_t_fitter(luminosity_sequence, window_radius=20, p_threshold=0.001, median_filter_size=None, downsteps_only=False,
                     min_step_magnitude=None):
    """stepfitting_library.sliding_t_fitter (:929-1078) on the GPU."""
    if median_filter_size is not None or downsteps_only or min_step_magnitude is not None:
        raise NotImplementedError("sliding_t_fitter: median_filter_size, downsteps_only and min_step_magnitude are not built")
    host, _, _ = _run([luminosity_sequence], 0, 0, p_threshold, None, window_radius=window_radius)
    return _plateau_lists(host, "pl", 0)


def chung_kennedy_filter(luminosities, window_lengths=range(2, 17), M=10, p=2):
    """stepfitting_library.chung_kennedy_filter (:1081-1274) on the GPU."""
    if not len(luminosities) > 2:
        raise ValueError("luminosities must have len(luminosities) > 2; currently len(luminosities) = " + str(len(luminosities)))
    host, lens, _ = _run([luminosities], 0, 1, 0.01, None, window_lengths=tuple(window_lengths), M=M, p=p, window_radius=0)
    return host["ck"][0, :int(lens[0])].tolist()


def t_test_filter(luminosities, plateaus, p_threshold, drop_sort=True, no_merge_start=0):
    """stepfitting_library.t_test_filter (:1441-1480) on the GPU (fsq_stepfit_ttest_filter): merges adjacent plateaus whose
    Welch t-test p >= p_threshold, len(plateaus) - 1 passes, both the drop_sort and the left-to-right branch.  Plateaus
    must be consecutive (stop + 1 == next start) within the luminosities; unmerged plateaus keep their given heights."""
    d = _plateau_rows(luminosities, plateaus, "t_test_filter", lenient=True)
    if d is None:
        return list(plateaus)
    torch = _engine._torch()
    dev, n = d["lum"].device, int(d["lum"].shape[1])
    L = NS.lib()
    ws_bytes = L.fsq_stepfit_ttest_filter_workspace_bytes(1, n)
    out = _plateau_out(1, n, dev, False)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = _engine.workspace(dev, ws_bytes)
    _engine.launch(L.fsq_stepfit_ttest_filter, "fsq_stepfit_ttest_filter", dev, d["lum"].data_ptr(), d["len"].data_ptr(), 1, n,
                   d["s"].data_ptr(), d["o"].data_ptr(), d["h"].data_ptr(), d["n"].data_ptr(), float(p_threshold), 1 if drop_sort else 0,
                   int(no_merge_start), out["start"].data_ptr(), out["stop"].data_ptr(), out["height"].data_ptr(),
                   out["count"].data_ptr(), status.data_ptr(), None, None, 0, ws.data_ptr(), int(ws_bytes))
    st = int(status.cpu()[0])
    if st == NS.STATUS_UNSUPPORTED:
        raise NotImplementedError("t_test_filter: a pass sorts >= 64 plateau pairs with a NaN p (CPython's merge sort order "
                                  "is not restated)")
    if st != NS.STATUS_OK:
        raise ValueError("t_test_filter: invalid plateaus")
    return _first_plateaus(out)


def refit_plateaus(luminosities, plateaus):
    """stepfitting_library.refit_plateaus (:1322): np.mean of each plateau's frames."""
    lum = np.asarray(luminosities, dtype=np.float64)
    out = []
    for start, stop, height in plateaus:
        if not 0 <= start <= stop < len(lum):
            raise ValueError("Invalid (starting_frame, stopping_frame): " + str((start, stop)))
        out.append((start, stop, np.mean(lum[start:stop + 1])))
    return out


def mirror_photometries(photometries, mirror_size):
    if mirror_size < 0:
        raise ValueError("mirror_size must be greater than 0.")
    return [x for x in reversed(photometries[:mirror_size])] + list(photometries)


def unmirror_photometries(photometries, mirror_size):
    if mirror_size < 0:
        raise ValueError("mirror_size must be greater than 0.")
    return photometries[mirror_size:]


def unmirror_plateaus(plateaus, mirror_size):
    if mirror_size < 0:
        raise ValueError("mirror_size must be greater than 0.")
    out = []
    for a, o, h in plateaus:
        a, o = a - mirror_size, o - mirror_size
        if a < 0 and o < 0:
            continue
        out.append((max(a, 0), o, h))
    return out


# ---- chi-squared step fitter, plateau merge filters, R^2 (include/fsq_chisq.h) --------------------------------------------
def _chisq_params(num_steps_multiplier, num_steps, min_step_length, min_step_magnitude, ignore_counterfits):
    """FsqChisqParams after the reference's own argument check (:433-435)."""
    if not 0 < num_steps_multiplier <= 1:
        raise ValueError("num_steps_multiplier has an invalid value of " + str(num_steps_multiplier))
    if num_steps is not None and not 0 < num_steps:
        raise ValueError("num_steps has an invalid value of " + str(num_steps))
    prm = NC.FsqChisqParams()
    prm.num_steps = 0 if num_steps is None else int(num_steps)
    prm.min_step_length = max(int(min_step_length), 0)
    prm.ignore_counterfits = 1 if ignore_counterfits else 0
    prm.num_steps_multiplier = float(num_steps_multiplier)
    prm.min_step_magnitude = float(min_step_magnitude)
    return prm


def chisq_device(d_lum, d_len, num_steps_multiplier=1, num_steps=None, min_step_length=2, min_step_magnitude=0.0,
                 ignore_counterfits=False, fit_cap=0):
    """fsq_chisq_step_fit on device tensors (float64 [n, max_frames], int32 [n]); returns a dict of device tensors:
    start, stop, height [n, max_frames], count, n_fits, status [n] and, when fit_cap > 0, best_res, counter_res, S
    (float64 [n, fit_cap]) and counter_n (int32).  Enqueued on the current stream, not synchronised.  Lengths are not
    checked here: a trace the device refuses comes back with a status other than 0 and its rows as allocated (zeros)."""
    torch = _engine._torch()
    prm = _chisq_params(num_steps_multiplier, num_steps, min_step_length, min_step_magnitude, ignore_counterfits)
    dev = d_lum.device
    n, max_frames = int(d_lum.shape[0]), int(d_lum.shape[1])
    L = NC.lib()
    ws_bytes = L.fsq_chisq_workspace_bytes(n, max_frames)
    if ws_bytes < 0:
        raise ValueError("fsq_chisq_workspace_bytes: invalid shape")
    out = _plateau_out(n, max_frames, dev, True)
    out["n_fits"], out["status"] = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    if fit_cap > 0:
        for k in ("best_res", "counter_res", "S"):
            out[k] = torch.zeros((n, fit_cap), dtype=torch.float64, device=dev)
        out["counter_n"] = torch.zeros((n, fit_cap), dtype=torch.int32, device=dev)
    ws = _engine.workspace(dev, ws_bytes)
    opt = [out[k].data_ptr() for k in ("best_res", "counter_res", "counter_n", "S")] if fit_cap > 0 else [None] * 4
    _engine.launch(L.fsq_chisq_step_fit, "fsq_chisq_step_fit", dev, d_lum.data_ptr(), d_len.data_ptr(), n, max_frames,
                   ctypes.byref(prm), out["start"].data_ptr(), out["stop"].data_ptr(), out["height"].data_ptr(), out["count"].data_ptr(),
                   out["n_fits"].data_ptr(), *opt, int(fit_cap), out["status"].data_ptr(), ws.data_ptr(), int(ws_bytes))
    out["_ws"] = ws                   # (kept alive until the caller has read the outputs)
    return out


def chisq_records(photometries, num_steps_multiplier=1, num_steps=None, min_step_length=2, min_step_magnitude=0.0,
                  ignore_counterfits=False, fit_cap=0, device=None):
    """chi_squared_step_fitter for many traces in one launch, as arrays.

    Returns a dict: "trace", "start", "stop", "height" (one entry per plateau, in trace order), "counts" and "n_fits" per
    trace, "lengths" and, when fit_cap > 0, "best_res", "counter_res", "S", "counter_n" ([n, fit_cap], row t valid up to
    n_fits[t]).  Raises the reference's errors for the first trace that has one."""
    rows, lens = _tracks.pack_rows(photometries, none_is_zero=False, nan_error="trace %d holds a NaN luminosity")   # (no pinnable result)
    _chisq_params(num_steps_multiplier, num_steps, min_step_length, min_step_magnitude, ignore_counterfits)
    if len(lens) and lens.max() > NC.MAX_FRAMES:
        raise ValueError("chi_squared_step_fitter: traces are limited to %d frames" % NC.MAX_FRAMES)
    for n in lens.tolist():
        if num_steps is not None and not 0 < num_steps < n:
            raise ValueError("num_steps has an invalid value of " + str(num_steps) + " vs len(luminosity_sequence) = " + str(n))
        if num_steps is None and n < 2:
            raise IndexError("list index out of range")            # (the reference sorts an empty list of fits, :502)
    if len(lens) == 0:
        return dict(_flat_empty(), n_fits=np.zeros(0, np.int32), lengths=lens)
    torch = _engine._torch()
    dev = torch.device(device or "cuda")
    host = _engine.to_host(chisq_device(torch.from_numpy(rows).to(dev), torch.from_numpy(lens).to(dev), num_steps_multiplier, num_steps,
                                        min_step_length, min_step_magnitude, ignore_counterfits, fit_cap))
    st = host["status"]
    if (st == NS.STATUS_UNSUPPORTED).any():
        i = int(np.flatnonzero(st == NS.STATUS_UNSUPPORTED)[0])
        raise ValueError("num_plateaus = " + str(int(lens[i]) + 1) + " is greater than len(luminosities) = " + str(int(lens[i])))
    if (st != NS.STATUS_OK).any():
        raise ValueError("trace %d: invalid length or num_steps" % int(np.flatnonzero(st != NS.STATUS_OK)[0]))
    res = dict(_flat(host["start"], host["stop"], host["height"], host["count"]), n_fits=host["n_fits"], lengths=lens)
    for k in ("best_res", "counter_res", "S", "counter_n"):
        if k in host:
            res[k] = host[k]
    return res


def chi_squared_step_fitter(luminosity_sequence, num_steps_multiplier=1, num_steps=None, min_step_length=2,
                            min_step_magnitude=0.0, ignore_counterfits=False):
    """stepfitting_library.chi_squared_step_fitter (:342-505) on the GPU: a list of (start, stop, height) plateaus."""
    r = chisq_records([luminosity_sequence], num_steps_multiplier, num_steps, min_step_length, min_step_magnitude,
                      ignore_counterfits)
    return _plateau_tuples(r["start"], r["stop"], r["height"])


def _plateau_rows(luminosities, plateaus, what, lenient=False):
    """One trace and its plateaus as the device rows of the filter kernels: {"lum", "len", "s", "o", "h", "n"}.  lenient
    (t_test_filter): None luminosities count 0, NaN ones pass, and fewer than two plateaus give None (nothing to merge)."""
    conv = (lambda v: 0.0 if v is None else float(v)) if lenient else float
    lum = np.array([conv(v) for v in luminosities], dtype=np.float64)
    if not lenient and np.isnan(lum).any():
        raise ValueError(what + ": a NaN luminosity")
    pls = [(int(a), int(o), float(h)) for a, o, h in plateaus]
    if lenient and len(pls) < 2:
        return None
    n = len(lum)
    if n > NS.MAX_MIRRORED:
        raise ValueError(what + ": at most %d luminosities" % NS.MAX_MIRRORED)
    if not (len(pls) >= 1 and 0 <= pls[0][0] and pls[-1][1] < n and all(a <= o for a, o, _ in pls) and
            all(pls[i][1] + 1 == pls[i + 1][0] for i in range(len(pls) - 1))):
        raise ValueError("Merged plateaus must be consecutive and lie within the luminosities")
    st = np.zeros((1, n), np.int32); so = np.zeros((1, n), np.int32); hh = np.zeros((1, n))
    st[0, :len(pls)] = [a for a, _, _ in pls]; so[0, :len(pls)] = [o for _, o, _ in pls]; hh[0, :len(pls)] = [h for _, _, h in pls]
    torch = _engine._torch()
    dev = torch.device("cuda")
    return {k: torch.from_numpy(v).to(dev) for k, v in (("lum", lum[None]), ("len", np.array([n], np.int32)), ("s", st), ("o", so),
                                                          ("h", hh), ("n", np.array([len(pls)], np.int32)))}


def _first_plateaus(out):
    """Trace 0 of the "start", "stop", "height", "count" device tensors as the reference's plateau tuples."""
    k = int(out["count"].cpu()[0])
    return _plateau_tuples(*(out[key][0, :k].cpu().numpy() for key in ("start", "stop", "height")))


def merge_filter_device(d_lum, d_len, d_start, d_stop, d_h, d_n, mode, min_magnitude=None, min_noise_ratio=None):
    """fsq_stepfit_merge_filter on device tensors (rows of [n, max_frames]); mode 0 filter_upsteps, 1 filter_small_steps.
    Returns {"start", "stop", "height", "count", "status"} device tensors; enqueued on the current stream."""
    torch = _engine._torch()
    dev = d_lum.device
    n, mf = int(d_lum.shape[0]), int(d_lum.shape[1])
    out = _plateau_out(n, mf, dev, True)
    out["status"] = torch.zeros(n, dtype=torch.int32, device=dev)
    _engine.launch(NC.lib().fsq_stepfit_merge_filter, "fsq_stepfit_merge_filter", dev, d_lum.data_ptr(), d_len.data_ptr(), n, mf,
                   d_start.data_ptr(), d_stop.data_ptr(), d_h.data_ptr(), d_n.data_ptr(), int(mode), 0 if min_magnitude is None else 1,
                   0.0 if min_magnitude is None else float(min_magnitude), 0 if min_noise_ratio is None else 1,
                   0.0 if min_noise_ratio is None else float(min_noise_ratio), out["start"].data_ptr(), out["stop"].data_ptr(),
                   out["height"].data_ptr(), out["count"].data_ptr(), out["status"].data_ptr(), None, 0)
    return out


def r_squared_device(d_lum, d_len, d_start, d_stop, d_h, d_n):
    """fsq_stepfit_r_squared on device tensors; returns {"r2", "status"} device tensors."""
    torch = _engine._torch()
    dev = d_lum.device
    n, mf = int(d_lum.shape[0]), int(d_lum.shape[1])
    out = {"r2": torch.zeros(n, dtype=torch.float64, device=dev), "status": torch.zeros(n, dtype=torch.int32, device=dev)}
    _engine.launch(NC.lib().fsq_stepfit_r_squared, "fsq_stepfit_r_squared", dev, d_lum.data_ptr(), d_len.data_ptr(), n, mf,
                   d_start.data_ptr(), d_stop.data_ptr(), d_h.data_ptr(), d_n.data_ptr(), out["r2"].data_ptr(), out["status"].data_ptr(),
                   None, 0)
    return out


def _merge_filter(luminosities, plateaus, mode, min_magnitude, min_noise_ratio, what):
    if len(plateaus) < 2:
        return list(plateaus)
    d = _plateau_rows(luminosities, plateaus, what)
    out = merge_filter_device(d["lum"], d["len"], d["s"], d["o"], d["h"], d["n"], mode, min_magnitude, min_noise_ratio)
    if int(out["status"].cpu()[0]) != NS.STATUS_OK:
        raise ValueError(what + ": invalid plateaus")
    return _first_plateaus(out)


def filter_upsteps(luminosities, plateaus):
    """stepfitting_library.filter_upsteps (:773-799) on the GPU: merges plateaus until no upstep remains."""
    return _merge_filter(luminosities, plateaus, 0, None, None, "filter_upsteps")


def filter_small_steps(luminosities, plateaus, min_magnitude=None, min_noise_ratio=None):
    """stepfitting_library.filter_small_steps (:881-926) on the GPU: merges steps below min_magnitude, or below
    min_noise_ratio * max(sqrt(residuals)) of their two plateaus; a criterion that is None is not applied."""
    if min_magnitude is not None and min_magnitude < 0:
        raise ValueError("min_step_magnitude < 0 makes no sense. min_magnitude = " + str(min_magnitude))
    if min_noise_ratio is not None and min_noise_ratio < 0:
        raise ValueError("min_step_noise_ratio < 0 makes no sense. min_noise_ratio = " + str(min_noise_ratio))
    return _merge_filter(luminosities, plateaus, 1, min_magnitude, min_noise_ratio, "filter_small_steps")


def stepfit_r_squared(luminosities, plateaus):
    """stepfitting_library.stepfit_r_squared (:1483-1503) on the GPU: 1 - SS_res / SS_tot over the frames the plateaus span."""
    d = _plateau_rows(luminosities, plateaus, "stepfit_r_squared")
    out = r_squared_device(d["lum"], d["len"], d["s"], d["o"], d["h"], d["n"])
    if int(out["status"].cpu()[0]) != NS.STATUS_OK:
        raise ValueError("stepfit_r_squared: invalid plateaus")
    return np.float64(out["r2"].cpu().numpy()[0])
