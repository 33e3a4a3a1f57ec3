"""Sequence experiments on the GPU (include/fsq_sequence.h): the step of the reference's basic_experiment_script after
tracking.  Every track of every field and channel is reduced to where its Spot is in each frame (detected, or filled in as
SequenceExperiment.fill_in_trace / interpolate_spots do, flexlibrary.py:1842-2032), whether it counts
(discard_invalid_traces, :2034-2063), its photometry per frame (binary_trace_categories_photometry, :2065-2129) and its
ON/OFF category; categories are counted per sequence on the device.  One *sequence* is one field of one channel.

sequence_photometry_records / category_counts are the records surface (flat NumPy arrays, no Python object per Spot);
run_device / category_counts_device work on device tensors.  flexlibrary's sequence classes are built on these."""
import numpy as np

from . import _native as N
from . import _native_sequence as NQ
from . import engine as _engine
from ._tracks import pattern_to_tuple                             # noqa: F401  (its old place)

METHODS = {"mexican_hat": NQ.METHOD_MEXICAN_HAT, "simple": NQ.METHOD_SIMPLE}
FIRST_OFFSET_ERROR = "The first image's offset must be (0, 0) by definiton."          # flexlibrary.py:581-583


def check_arguments(frames_shape, trace_hw, trace_seq, offsets, method="mexican_hat", radius=9, brim_size=6, spot_size=5):
    """Validates and normalises the host arguments of sequence_photometry_records (no GPU needed).
    -> (trace_hw int32 [N, F, 2], trace_seq int32 [N], offsets float64 [n_seq, F, 2], method code).  Raises before anything
    is launched: ValueError on mismatched shapes, a sequence index out of range, a first offset that is not (0, 0) (the
    reference's text) or an unknown method (the reference's text); NotImplementedError beyond 64 frames."""
    if method not in METHODS:
        if method in ("sextractor", "maximum", "sigmas", "gaussian_volume"):
            raise NotImplementedError("photometry method %r is not computed on the device" % (method,))
        raise ValueError("Uknown method specified.")                                 # flexlibrary.py:315
    if len(frames_shape) != 4:
        raise ValueError("frames must have shape (n_seq, F, H, W)")
    n_seq, F, H, W = (int(x) for x in frames_shape)
    if n_seq < 1 or F < 1 or H < 1 or W < 1:
        raise ValueError("frames must have shape (n_seq, F, H, W) with no empty axis")
    if F > NQ.MAX_FRAMES:
        raise NotImplementedError("sequences of more than %d frames are not built (the category is one bit per frame)"
                                  % NQ.MAX_FRAMES)
    hw = np.asarray(trace_hw)
    if hw.size == 0:
        hw = np.zeros((0, F, 2), np.int32)
    if hw.ndim != 3 or hw.shape[1] != F or hw.shape[2] != 2:
        raise ValueError("trace_hw must have shape (n_traces, %d, 2)" % F)
    if hw.dtype.kind not in "iu":
        if not np.array_equal(hw, np.rint(hw)):
            raise ValueError("trace_hw must hold whole numbers")
    if hw.size and (hw.min() < -1 or hw.max() >= 2 ** 29):
        raise ValueError("trace_hw must hold pixel coordinates, or (-1, -1) where the trace has no Spot")
    hw = np.ascontiguousarray(hw.astype(np.int32))
    seq = np.ascontiguousarray(np.asarray(trace_seq).reshape(-1).astype(np.int32)) if len(hw) else np.zeros(0, np.int32)
    if len(seq) != len(hw):
        raise ValueError("trace_seq must name a sequence for every trace")
    if len(seq) and (seq.min() < 0 or seq.max() >= n_seq):
        raise ValueError("trace_seq out of range")
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.float64))
    if off.shape != (n_seq, F, 2):
        raise ValueError("offsets must have shape (%d, %d, 2)" % (n_seq, F))
    if np.any(off[:, 0, :] != 0):
        raise ValueError(FIRST_OFFSET_ERROR)
    if int(radius) != radius or int(brim_size) != brim_size or radius < 0 or brim_size < 0 or radius > 16383:
        raise ValueError("radius and brim_size must be whole numbers >= 0")
    if int(spot_size) != spot_size or spot_size < 1 or spot_size % 2 == 0 or spot_size > 32767:
        raise ValueError("Spot.size must be odd.")
    return hw, seq, off, METHODS[method]


def run_device(d_frames, d_trace_hw, d_trace_seq, d_offsets, wide=False, method=NQ.METHOD_MEXICAN_HAT, radius=9, brim_size=6,
               spot_size=5, interpolate=True):
    """fsq_sequence_photometry on device tensors: d_frames [n_seq, F, H, W] (16-bit words, or 32-bit with wide=True),
    d_trace_hw int32 [N, F, 2], d_trace_seq int32 [N], d_offsets float64 [n_seq, F, 2].  Returns a dict of device tensors: hw
    int32 [N, F, 2], photometry float64 [N, F], flags uint8 [N, F], category int64 [N] (the 64 bits of the uint64 pattern),
    trace_valid uint8 [N].  Enqueued on the current stream, not synchronised; the arguments are not checked here."""
    torch = _engine._torch()
    dev = d_frames.device
    n_seq, F, H, W = (int(x) for x in d_frames.shape)
    n = int(d_trace_hw.shape[0])
    L = NQ.lib()
    ws_bytes = L.fsq_sequence_workspace_bytes(n_seq, F)
    if ws_bytes < 0:
        raise ValueError("fsq_sequence_workspace_bytes: invalid shape")
    m = max(n, 1)
    out = {"hw": torch.empty((m, F, 2), dtype=torch.int32, device=dev),
           "photometry": torch.empty((m, F), dtype=torch.float64, device=dev),
           "flags": torch.empty((m, F), dtype=torch.uint8, device=dev),
           "category": torch.empty(m, dtype=torch.int64, device=dev),
           "trace_valid": torch.empty(m, dtype=torch.uint8, device=dev)}
    ws = _engine.workspace(dev, ws_bytes)
    _engine.launch(L.fsq_sequence_photometry_u32 if wide else L.fsq_sequence_photometry, "fsq_sequence_photometry", dev,
                   d_frames.data_ptr(), n_seq, F, H, W, d_trace_hw.data_ptr(), d_trace_seq.data_ptr(), n, d_offsets.data_ptr(),
                   int(radius), int(brim_size), int(spot_size), int(method), 1 if interpolate else 0, out["hw"].data_ptr(),
                   out["photometry"].data_ptr(), out["flags"].data_ptr(), out["category"].data_ptr(), out["trace_valid"].data_ptr(),
                   ws.data_ptr(), int(ws_bytes))
    for k in out:
        out[k] = out[k][:n]
    out["_ws"] = ws                   # (kept alive until the caller has read the outputs)
    return out


def category_counts_device(d_category, d_trace_seq, d_select=None):
    """fsq_sequence_category_counts on device tensors (category int64 [N], trace_seq int32 [N], select uint8 [N] or None).
    Returns device tensors (seq int32, pattern int64, count int32, first int32, n_groups int32 [1]); rows beyond n_groups are
    not written.  Not synchronised."""
    torch = _engine._torch()
    dev = d_category.device
    n = int(d_category.shape[0])
    L = NQ.lib()
    ws_bytes = L.fsq_sequence_category_counts_workspace_bytes(n)
    if ws_bytes < 0:
        raise ValueError("fsq_sequence_category_counts: too many traces")
    m = max(n, 1)
    g_seq = torch.empty(m, dtype=torch.int32, device=dev)
    g_pat = torch.empty(m, dtype=torch.int64, device=dev)
    g_cnt = torch.empty(m, dtype=torch.int32, device=dev)
    g_first = torch.empty(m, dtype=torch.int32, device=dev)
    g_n = torch.empty(1, dtype=torch.int32, device=dev)
    ws = _engine.workspace(dev, ws_bytes)
    _engine.launch(L.fsq_sequence_category_counts, "fsq_sequence_category_counts", dev, d_category.data_ptr(), d_trace_seq.data_ptr(),
                   d_select.data_ptr() if d_select is not None else None, n, g_seq.data_ptr(), g_pat.data_ptr(), g_cnt.data_ptr(),
                   g_first.data_ptr(), g_n.data_ptr(), ws.data_ptr(), int(ws_bytes))
    return g_seq, g_pat, g_cnt, g_first, g_n, ws


def _counts_to_host(g_seq, g_pat, g_cnt, g_first, g_n):
    k = int(g_n.item())
    first = g_first[:k].cpu().numpy()
    order = np.argsort(first, kind="stable")          # order of first appearance (the table itself comes in no particular order)
    return {"seq": g_seq[:k].cpu().numpy()[order], "pattern": g_pat[:k].cpu().numpy().view(np.uint64)[order],
            "count": g_cnt[:k].cpu().numpy()[order], "first": first[order]}


def category_counts(category, trace_seq, select=None, device=None):
    """Counts of traces per (sequence, pattern), counted on the device: dict of flat arrays seq int32, pattern uint64 (bit f =
    ON in frame f), count int32, first int32 (smallest trace index of the group), in order of first appearance.  select
    (bool [N]) restricts the count to some traces."""
    torch = _engine._torch()
    dev = torch.device(device or ("cuda:%d" % torch.cuda.current_device()))
    cat = np.ascontiguousarray(np.asarray(category, dtype=np.uint64).reshape(-1))
    seq = np.ascontiguousarray(np.asarray(trace_seq).reshape(-1).astype(np.int32))
    if len(cat) != len(seq):
        raise ValueError("category and trace_seq must have one entry per trace")
    d_sel = None
    if select is not None:
        sel = np.ascontiguousarray(np.asarray(select).reshape(-1).astype(np.uint8))
        if len(sel) != len(cat):
            raise ValueError("select must have one entry per trace")
        d_sel = torch.from_numpy(sel).to(dev)
    res = category_counts_device(torch.from_numpy(cat.view(np.int64)).to(dev), torch.from_numpy(seq).to(dev), d_sel)
    return _counts_to_host(*res[:5])


def sequence_photometry_records(frames, trace_hw, trace_seq, offsets, method='mexican_hat', radius=9, brim_size=6, spot_size=5,
                                interpolate=True, device=None, counts=True):
    """All traces of all sequences of an experiment in one launch.

    frames    integer [n_seq, F, H, W] (values < 2^31; beyond 65 535 the uint32 kernel runs), F <= 64
    trace_hw  int [N, F, 2]: (h, w) of the detected Spot of every trace in every frame, (-1, -1) where there is none
    trace_seq int [N]: the sequence of every trace
    offsets   float [n_seq, F, 2]: (d_h, d_w) of every frame relative to the one before; offsets[:, 0] must be (0, 0)
    method    'mexican_hat' (radius, brim_size) or 'simple' (sum of the spot_size^2 window)
    interpolate  False: an undetected frame is None; True: it is filled in as SequenceExperiment.fill_in_trace does

    Returns a dict of NumPy arrays: hw int32 [N, F, 2] ((-1, -1) = None), photometry float64 [N, F] (NaN where None), flags
    uint8 [N, F] (1 detected, 2 interpolated, 4 window fully inside the frame = Spot.valid_slice), category uint64 [N] (bit f =
    detected in frame f), trace_valid bool [N] (every frame holds a Spot and every window is inside: what
    discard_invalid_traces keeps when interpolate is True), and, with counts=True, `counts`: category_counts of all traces."""
    fr, fmt = _engine.as_integer_fields(frames)
    hw, seq, off, code = check_arguments(fr.shape, trace_hw, trace_seq, offsets, method, radius, brim_size, spot_size)
    torch = _engine._torch()
    dev = torch.device(device or ("cuda:%d" % torch.cuda.current_device()))
    d_fr = _engine.to_device_pixels(fr, fmt, dev)
    d_hw, d_seq, d_off = torch.from_numpy(hw).to(dev), torch.from_numpy(seq).to(dev), torch.from_numpy(off).to(dev)
    if len(hw) == 0:
        d_hw = torch.zeros((0, fr.shape[1], 2), dtype=torch.int32, device=dev)
    o = run_device(d_fr, d_hw, d_seq, d_off, wide=(fmt == N.PIXELS_U32), method=code, radius=radius, brim_size=brim_size,
                   spot_size=spot_size, interpolate=interpolate)
    res = None
    if counts:
        res = category_counts_device(o["category"], d_seq)
    out = {"hw": o["hw"].cpu().numpy(), "photometry": o["photometry"].cpu().numpy(), "flags": o["flags"].cpu().numpy(),
           "category": o["category"].cpu().numpy().view(np.uint64), "trace_valid": o["trace_valid"].cpu().numpy().astype(bool)}
    if counts:
        out["counts"] = _counts_to_host(*res[:5])
    return out
