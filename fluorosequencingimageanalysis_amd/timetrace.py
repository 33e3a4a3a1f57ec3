"""Timetrace experiments on the GPU (include/fsq_timetrace.h): the table TimetraceExperiment.save_experiment_as_csv writes
(flexlibrary.py:3550-3709) for whole experiments in one launch, and a frame stack -> table path that stays on the device.

table_device      device tensors in, device tensors out (fsq_timetrace_table)
timetrace_table   host convenience for ragged lists; raises what the reference raises
timetrace_records frames + first-frame spots -> tracking, photometry, step fit and table, uploaded once, downloaded once
write_csv         the records as the reference's CSV (Python 2's text, as pflib.save_psfs_csv writes it)

DESIGN.md 4.13 states the table's rules, among them the reference's own reading of `Step #` / `Step Size`."""
import csv

import numpy as np

from . import _native as N
from . import _native_stepfit as NS
from . import _native_timetrace as NT
from . import _tracks
from . import engine as _engine
from . import stepfitting as _sf
from .pflib import _py2_str

HEADER = ['Trace #', 'Hcoord', 'Wcoord', 'Frame #', 'Photometry']
STEP_FIT_HEADER = ['Step #', 'Plateau Height', 'Step Size', 'Plateau Length', 'Overall Fit R^2']
INTERMEDIATES = ('ck_filtered_photometries', 'photometries', 'plateaus', 't_filtered_plateaus')     # (sorted() order)
TABLE_KEYS = ("plateau_index", "plateau_height", "plateau_length", "step_num", "step_size", "rss", "tss", "r2", "status")


def table_out(n, max_frames, dev):
    """Zeroed output tensors of table_device."""
    torch = _engine._torch()
    i32, f64 = torch.int32, torch.float64
    out = {k: torch.zeros((n, max_frames), dtype=dt, device=dev)
           for k, dt in (("plateau_index", i32), ("plateau_height", f64), ("plateau_length", i32), ("step_num", i32), ("step_size", f64))}
    out.update({k: torch.zeros(n, dtype=f64, device=dev) for k in ("rss", "tss", "r2")})
    out["status"] = torch.zeros(n, dtype=i32, device=dev)
    return out


def table_device(d_phot, d_len, d_start, d_stop, d_h, d_n, out=None):
    """fsq_timetrace_table on device tensors (float64 / int32 rows of [n, max_frames], int32 [n]); returns a dict of device
    tensors under TABLE_KEYS (`out`, when given, is written in place).  Enqueued on the current stream, not synchronised.
    A trace the device refuses comes back with status 2 and its rows as they were (zeros)."""
    dev = d_phot.device
    n, mf = int(d_phot.shape[0]), int(d_phot.shape[1])
    out = table_out(n, mf, dev) if out is None else out
    _engine.launch(NT.lib().fsq_timetrace_table, "fsq_timetrace_table", dev, d_phot.data_ptr(), d_len.data_ptr(), n, mf,
                   d_start.data_ptr(), d_stop.data_ptr(), d_h.data_ptr(), d_n.data_ptr(), *[out[k].data_ptr() for k in TABLE_KEYS])
    return out


def plateau_values_device(d_start, d_stop, d_h, d_n, want_index=False):
    """fsq_plateau_values: per frame the height (and index) of the plateau that holds it -> {"height", "index", "status"}
    device tensors; frames beyond a trace's last stop stay 0."""
    torch = _engine._torch()
    dev = d_start.device
    n, mf = int(d_start.shape[0]), int(d_start.shape[1])
    out = {"height": torch.zeros((n, mf), dtype=torch.float64, device=dev), "status": torch.zeros(n, dtype=torch.int32, device=dev),
           "index": torch.zeros((n, mf), dtype=torch.int32, device=dev) if want_index else None}
    _engine.launch(NT.lib().fsq_plateau_values, "fsq_plateau_values", dev, d_start.data_ptr(), d_stop.data_ptr(), d_h.data_ptr(),
                   d_n.data_ptr(), n, mf, out["height"].data_ptr(), out["index"].data_ptr() if want_index else None,
                   out["status"].data_ptr())
    return out


def raise_for_status(status, lens, sf_stop, sf_n):
    """The reference's exception for the first trace whose status word is not 0: Exception for a step fit that covers another
    number of frames than the trace (flexlibrary.py:1484), ValueError for a frame that lies in no plateau
    (stepfitting_library.py:527), ZeroDivisionError for a total sum of squares of 0 (:1514)."""
    status = np.asarray(status)
    for t in np.flatnonzero(status != NS.STATUS_OK).tolist():
        if status[t] == NT.STATUS_ZERO_TSS:
            raise ZeroDivisionError("float division by zero")
        k = int(sf_n[t])
        covered = int(sf_stop[t][k - 1]) + 1 if 1 <= k <= len(sf_stop[t]) else 0
        if covered != int(lens[t]):
            raise Exception("trace_A and trace_B must cover an identical number of frames for comparison to be valid.")
        raise ValueError("trace " + str(t) + ": a frame is outside of its plateaus")


def plateau_rows(plateaus, max_frames):
    """A list of plateau lists -> int32 start / stop, float64 height rows [n, max_frames] and int32 counts."""
    n = len(plateaus)
    if any(len(p) > max_frames for p in plateaus):
        raise ValueError("a trace has more plateaus than frames")
    st, so, hh = np.zeros((n, max_frames), np.int32), np.zeros((n, max_frames), np.int32), np.zeros((n, max_frames))
    for i, pls in enumerate(plateaus):
        k = len(pls)
        st[i, :k] = [p[0] for p in pls]; so[i, :k] = [p[1] for p in pls]; hh[i, :k] = [float(p[2]) for p in pls]
    return st, so, hh, np.array([len(p) for p in plateaus], np.int32)


def timetrace_table(photometries, plateaus, device=None):
    """The table of many traces: photometries is a 2-D array or a list of ragged sequences (None counts 0), plateaus one list
    of (start, stop, height) per trace.  Returns a dict of numpy arrays under TABLE_KEYS (rows [n, max_frames], row t valid
    for its own length) and "lengths"; raises what save_experiment_as_csv raises for the first trace it would fail on."""
    rows, lens = _tracks.pack_rows(photometries, none_is_zero=True)
    if len(plateaus) != len(lens):
        raise ValueError("plateaus must hold one list per trace")
    if len(lens) == 0:
        return dict({k: np.zeros((0, 1)) for k in TABLE_KEYS}, lengths=lens)
    mf = rows.shape[1]
    if mf > NS.MAX_MIRRORED:
        raise ValueError("traces are limited to %d frames" % NS.MAX_MIRRORED)
    st, so, hh, cnt = plateau_rows(plateaus, mf)
    torch = _engine._torch()
    dev = torch.device(device or "cuda")
    host = _engine.to_host(table_device(*(torch.from_numpy(a).to(dev) for a in (rows, lens, st, so, hh, cnt))))
    raise_for_status(host["status"], lens, so, cnt)
    host["lengths"] = lens
    return host


def timetrace_records(frames, init_hw, search_radius=3, s_n_cutoff=3.0, photometry_min=None, mirror_start=0, chung_kennedy=0,
                      p_threshold=0.01, brim_size=6, radius=9, include_intermediates=True, device=None):
    """One filmed field from frames to the experiment table without leaving the device: TimetraceExperiment's
    lc_create_traces + stepfit_tracks + the numbers of save_experiment_as_csv.

    frames integer [F, H, W] (values below 2^31; beyond 65 535 the _u32 entries run); init_hw int [T, 2], the Spots of frame 0.
    The stack is uploaded once; fsq_centroid_tracking, fsq_timetrace_spot_rows, fsq_mexican_hat,
    fsq_timetrace_photometry_rows, fsq_stepfit_traces and fsq_timetrace_table run on it, then everything is downloaded once.
    Returns a dict of numpy arrays: hw [T, F, 2], present [T, F], photometry [T, F] (raw, 0 where absent), photometries (the
    `photometries` intermediate: the same numbers, since photometry_min does not reach the step fit), ck_filtered, pl_* / tf_* plateau rows with "plateaus" / "t_filtered_plateaus" as stepfit_records lays
    them out, the table under TABLE_KEYS, r_squared (= r2), lengths, params and, with include_intermediates, plateaus_height (the
    `plateaus` column).  Raises what the object path raises."""
    torch = _engine._torch()
    dev = torch.device(device or ("cuda:%d" % torch.cuda.current_device()))
    fr, fmt = _engine.as_integer_fields(frames)
    if fr.ndim != 3:
        raise ValueError("frames must have shape (F, H, W)")
    F, H, W = fr.shape
    hw0 = np.ascontiguousarray(np.asarray(init_hw, dtype=np.int32).reshape(-1, 2))
    T = len(hw0)
    if len(set(map(tuple, hw0.tolist()))) != T:
        raise Exception("Two tracks have initial Spots with identical (h, w).")
    # (photometry_min is accepted and unused, as in TimetraceExperiment.stepfit_tracks: the reference drops it on the way to
    # the step fit, flexlibrary.py:3499-3508)
    prm = _sf._params(mirror_start, chung_kennedy, p_threshold, None)
    _sf._check_lengths(np.full(T, F, np.int32), prm)
    params = {"photometry_min": photometry_min, "mirror_start": int(mirror_start), "chung_kennedy": int(chung_kennedy)}
    if T == 0:
        return {"hw": np.zeros((0, F, 2), np.int32), "present": np.zeros((0, F), bool), "lengths": np.zeros(0, np.int32),
                "photometry": np.zeros((0, F)), "params": params}
    L, LT = N.lib(), NT.lib()
    u32 = fmt == N.PIXELS_U32
    d_fr = _engine.to_device_pixels(fr, fmt, dev)
    d_hw0 = torch.from_numpy(hw0).to(dev)
    d_field = torch.zeros(T, dtype=torch.int32, device=dev)
    d_hw = torch.empty((T, F, 2), dtype=torch.int32, device=dev)
    d_pres = torch.empty((T, F), dtype=torch.uint8, device=dev)
    d_err = torch.zeros(1, dtype=torch.int32, device=dev)
    _engine.launch(L.fsq_centroid_tracking_u32 if u32 else L.fsq_centroid_tracking, "fsq_centroid_tracking", dev, d_fr.data_ptr(), 1, F,
                   H, W, d_hw0.data_ptr(), d_field.data_ptr(), T, int(search_radius), float(s_n_cutoff), None, d_hw.data_ptr(),
                   d_pres.data_ptr(), d_err.data_ptr())
    if int(d_err.item()):                                              # (before the positions are used as pixel addresses)
        raise ValueError("cannot convert float NaN to integer")
    d_fhw = torch.empty((T * F, 3), dtype=torch.int32, device=dev)
    _engine.launch(LT.fsq_timetrace_spot_rows, "fsq_timetrace_spot_rows", dev, d_hw.data_ptr(), d_pres.data_ptr(), T, F, d_fhw.data_ptr())
    d_val = torch.empty(T * F, dtype=torch.float64, device=dev)
    _engine.launch(L.fsq_mexican_hat_u32 if u32 else L.fsq_mexican_hat, "fsq_mexican_hat", dev, d_fr.data_ptr(), F, H, W,
                   d_fhw.data_ptr(), T * F, int(brim_size), int(radius), d_val.data_ptr())
    d_rows = torch.empty((T, F), dtype=torch.float64, device=dev)
    d_len = torch.empty(T, dtype=torch.int32, device=dev)
    _engine.launch(LT.fsq_timetrace_photometry_rows, "fsq_timetrace_photometry_rows", dev, d_val.data_ptr(), d_pres.data_ptr(), T, F,
                   d_rows.data_ptr(), d_len.data_ptr())
    fit = _sf.run_device(d_rows, d_len, F, prm)
    tab = table_device(d_rows, d_len, fit["tf_start"], fit["tf_stop"], fit["tf_h"], fit["tf_n"])
    dev_out = {"hw": d_hw, "present": d_pres, "photometry": d_rows, "ck_filtered": fit["ck"]}
    dev_out.update({k: fit[k] for k in fit if k[:3] in ("pl_", "tf_")})
    dev_out["fit_status"] = fit["status"]
    dev_out.update(tab)
    if include_intermediates:
        pv = plateau_values_device(fit["pl_start"], fit["pl_stop"], fit["pl_h"], fit["pl_n"])
        dev_out["plateaus_height"], dev_out["plateaus_status"] = pv["height"], pv["status"]
    host = _engine.to_host(dev_out)
    _sf.raise_for_fit_status(host.pop("fit_status"))
    lens = np.full(T, F, np.int32)
    raise_for_status(host["status"], lens, host["tf_stop"], host["tf_n"])
    if include_intermediates:
        raise_for_status(host.pop("plateaus_status"), lens, host["pl_stop"], host["pl_n"])
    host["present"] = host["present"].astype(bool)
    host["photometries"] = host["photometry"]
    for pre, name in (("pl", "plateaus"), ("tf", "t_filtered_plateaus")):
        host[name] = _sf._flat(host[pre + "_start"], host[pre + "_stop"], host[pre + "_h"], host[pre + "_n"])
    host["r_squared"], host["lengths"], host["params"] = host["r2"], lens, params
    return host


def _cells(values, mask=None, masked="None"):
    """Python 2's str() of a row of floats, cached per distinct neighbour as the reference caches per plateau."""
    out, last, text = [], None, None
    for i, v in enumerate(values.tolist()):
        if mask is not None and mask[i]:
            out.append(masked)
            continue
        if v != last or text is None:
            last, text = v, _py2_str(float(v))
        out.append(text)
    return out


def write_csv(path, records, include_step_fits=True, include_intermediates=True, dialect='excel'):
    """timetrace_records' result as the CSV TimetraceExperiment.save_experiment_as_csv writes; returns the number of rows
    written including the header.  Floats are Python 2's str() ('%.12g'), the Photometry cell repr(float), a None Spot's
    photometry the int 0 - also in the `photometries` column (and in `ck_filtered_photometries` when no filter ran), as in the
    reference."""
    hw, present, lens = records["hw"], records["present"], records["lengths"]
    prm = records["params"]
    header = list(HEADER) + (STEP_FIT_HEADER if include_step_fits else []) + (list(INTERMEDIATES) if include_intermediates else [])
    if include_intermediates and len(lens) and "plateaus_height" not in records:
        raise KeyError("records were made without include_intermediates")
    n_rows = 1
    with open(path, 'w', newline='') as f:
        wr = csv.writer(f, dialect=dialect)
        wr.writerow(header)
        for t in range(len(lens)):
            n = int(lens[t])
            base = [str(t), str(int(hw[t, 0, 0])), str(int(hw[t, 0, 1]))]
            absent = ~present[t, :n]
            cols = [[repr(float(v)) if p else '0' for v, p in zip(records["photometry"][t, :n].tolist(), present[t, :n].tolist())]]
            if include_step_fits:
                none = records["step_num"][t, :n] < 0
                r2 = _py2_str(float(records["r2"][t]))
                cols += [['None' if m else str(v) for v, m in zip(records["step_num"][t, :n].tolist(), none.tolist())],
                         _cells(records["plateau_height"][t, :n]), _cells(records["step_size"][t, :n], none),
                         [str(v) for v in records["plateau_length"][t, :n].tolist()], [r2] * n]
            if include_intermediates:
                int0 = absent
                cols += [_cells(records["ck_filtered"][t, :n], int0 if prm["chung_kennedy"] == 0 else None, '0'),
                         _cells(records["photometries"][t, :n], int0, '0'), _cells(records["plateaus_height"][t, :n]),
                         _cells(records["plateau_height"][t, :n])]
            for fi in range(n):
                wr.writerow(base + [str(fi)] + [c[fi] for c in cols])
            n_rows += n
    return n_rows
