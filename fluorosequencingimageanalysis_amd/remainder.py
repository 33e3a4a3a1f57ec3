"""Remainder correction of track photometries: the reference's remainder_correction step, on the GPU.

MCsimlib._remainder_adjust_2 (:3434-3472, method 4 of remainder_correction.py) corrects per-field, per-cycle illumination drift
with the peptides that never lose a fluor, the remainders (category ON in every frame): per remainder the ratios (I_f - m) / m
against its median m over frames, per (channel, field) and frame the median of those ratios, and every track of a field with
at least `minimum_r_per_field` remainders scaled by 1 - median.  MCsimlib._remainder_adjust (:3398-3431) is the additive
sibling: medians of the raw intensities, and median_f - median_0 subtracted.  Both run on the device as one call of
fsq_remainder_adjust (include/fsq_remainder.h; `remainder_adjust_device`, `remainder_adjust_records`) with numpy's bits, and
as plain numpy on the host with `device=None`.  `remainder_adjust_2` and `remainder_adjust` are drop-ins on the nested dict of
lognormal.read_track_photometries_csv; dicts are walked in insertion order (Python 2's hash order is not reproduced).

A segment is one (channel, field).  `adjustment` is computed for every segment, kept or not (NaN for one without a remainder);
the `adjusted` rows of a segment that is not kept are 0.  A median of -0.0 comes out as +0.0, as np.median's does (np.mean's
sum starts from +0.0), so the order of -0.0 and +0.0 within one (segment, frame) never shows.

Checks, each raised on the host before anything is launched, on either route: every track has exactly `num_frames`
intensities and category entries (ValueError); at least one frame (ValueError) and at most 64, the category word
(NotImplementedError); finite intensities of a magnitude of at most 2^52, beyond which the mean of two middle integers is no
longer exact (ValueError); fewer than 2^31 tracks (ValueError).  `remainder_adjust_device` takes device tensors as they are
and checks their shapes and types only."""
import ctypes

import numpy as np

from . import _host_remainder
from . import _native_remainder as NR
from . import _tracks
from . import engine as _engine
from .lognormal import unwind_photometries
from .pflib import _py2_round, _py2_str

MAX_FRAMES = NR.MAX_FRAMES
LDS_MAX = NR.LDS_MAX
MAX_MAGNITUDE = float(1 << 52)
_MODES = {"ratio": NR.MODE_RATIO, "additive": NR.MODE_ADDITIVE}


def _mode(mode):
    if mode not in _MODES:
        raise ValueError("mode is 'ratio' or 'additive'")
    return _MODES[mode]


def _check_frames(F):
    if F < 1:
        raise ValueError("at least one frame is needed")
    if F > MAX_FRAMES:
        raise NotImplementedError("tracks are limited to %d frames" % MAX_FRAMES)


# ---- the device route ----

def remainder_adjust_device(d_intensity, d_category, d_seg_off, mode='ratio', minimum_r_per_field=5):
    """fsq_remainder_adjust on device tensors: float64 [n, F] intensities, 64-bit [n] category words (bit f set when frame f
    is ON) and int64 [S + 1] segment offsets, the tracks of a segment contiguous.  Returns a dict of device tensors: adjusted
    float64 [n, F], adjustment float64 [S, F], n_remainders int32 [S], kept uint8 [S].  Enqueued on the current stream, not
    synchronised; the values of the tensors are not checked."""
    torch = _engine._torch()
    prm = NR.FsqRemainderParams(_mode(mode), max(-(1 << 31), min(int(minimum_r_per_field), (1 << 31) - 1)))
    if d_intensity.dim() != 2 or d_category.dim() != 1 or d_seg_off.dim() != 1 or d_seg_off.numel() < 1:
        raise ValueError("[n, F] intensities, [n] categories and [S + 1] offsets are needed")
    n, F, S = int(d_intensity.shape[0]), int(d_intensity.shape[1]), int(d_seg_off.numel()) - 1
    _check_frames(F)
    if n >= 1 << 31 or S * F >= 1 << 31:
        raise ValueError("fewer than 2^31 tracks and (segment, frame) pairs are needed")
    if int(d_category.numel()) != n:
        raise ValueError("one category per track")
    if not (d_intensity.is_contiguous() and d_category.is_contiguous() and d_seg_off.is_contiguous()):
        raise ValueError("contiguous tensors are needed")
    if d_intensity.dtype != torch.float64 or d_category.element_size() != 8 or d_seg_off.dtype != torch.int64:
        raise ValueError("float64 intensities, 64-bit categories and int64 offsets are needed")
    dev = d_intensity.device
    if not d_intensity.is_cuda or d_category.device != dev or d_seg_off.device != dev:
        raise ValueError("tensors on one GPU are needed")
    L = NR.lib()
    ws_bytes = L.fsq_remainder_workspace_bytes(n, F, S)
    if ws_bytes < 0:
        raise ValueError("fsq_remainder_workspace_bytes: invalid shape")
    out = {"adjusted": torch.empty((n, F), dtype=torch.float64, device=dev),
           "adjustment": torch.empty((S, F), dtype=torch.float64, device=dev),
           "n_remainders": torch.empty(S, dtype=torch.int32, device=dev),
           "kept": torch.empty(S, dtype=torch.uint8, device=dev)}
    ws = _engine.workspace(dev, ws_bytes)
    _engine.launch(L.fsq_remainder_adjust, "fsq_remainder_adjust", dev, d_intensity.data_ptr(), d_category.data_ptr(),
                   d_seg_off.data_ptr(), n, F, S, ctypes.byref(prm), out["adjustment"].data_ptr(), out["n_remainders"].data_ptr(),
                   out["kept"].data_ptr(), out["adjusted"].data_ptr(), ws.data_ptr(), ws_bytes)
    return out


# ---- arrays ----

def _checked_rows(intensities, num_frames=None):
    """float64 [n, F] after the checks the module docstring names."""
    two_d = isinstance(intensities, np.ndarray) and intensities.ndim == 2
    seqs = intensities if two_d else [np.asarray(s).reshape(-1) for s in intensities]
    F = int(num_frames) if num_frames is not None else seqs.shape[1] if two_d else len(seqs[0]) if seqs else 1
    if any(s.dtype.kind not in "fiub" for s in ([seqs] if two_d else seqs)):
        raise ValueError("finite real intensities are needed")
    rows, _ = _tracks.pack_rows(seqs, width=F, width_error="every track needs exactly %d intensities" % F)
    _check_frames(F)
    if rows.shape[0] >= 1 << 31:
        raise ValueError("fewer than 2^31 tracks are needed")
    if not np.isfinite(rows).all():
        raise ValueError("intensities must be finite")
    if rows.size and np.abs(rows).max() > MAX_MAGNITUDE:
        raise ValueError("intensities are limited to a magnitude of 2^52")
    return rows


def _grouped(ids):
    """(order, unique ids, seg_off) of one segment id per track: a stable grouping by ascending id."""
    ids = np.asarray(ids).reshape(-1)
    order = np.argsort(ids, kind='stable')
    unique, counts = np.unique(ids, return_counts=True)
    seg_off = np.zeros(len(unique) + 1, np.int64)
    np.cumsum(counts, out=seg_off[1:])
    return order, unique, seg_off


def _adjust(rows, cats, seg_off, mode, minimum_r_per_field, device):
    """remainder_adjust_device's dict as arrays for grouped host arrays: with numpy for device=None, else on that GPU."""
    if device is None:
        return _host_remainder.adjust(rows, cats, seg_off, _mode(mode), int(minimum_r_per_field))
    torch = _engine._torch()
    dev = torch.device(device)
    return _engine.to_host(remainder_adjust_device(torch.from_numpy(rows).to(dev), torch.from_numpy(cats.view(np.int64)).to(dev),
                                                   torch.from_numpy(seg_off).to(dev), mode, minimum_r_per_field))


def remainder_adjust_records(intensities, categories, segments, mode='ratio', minimum_r_per_field=5, device="cuda"):
    """The correction of many tracks in one call, as arrays.

    intensities  sequences of one length, a [n, F] array or a float64 CUDA tensor of that shape; categories  tuples of F
    booleans, or the uint64 / int64 words as an array or CUDA tensor; segments  one integer id per track, in any order: the
    tracks are grouped stably by ascending id.  device  where it runs; None: with numpy on the host.
    Returns a dict of NumPy arrays: adjusted float64 [n, F] in the caller's order, segment_ids (ascending), and per segment id
    adjustment float64 [S, F], n_remainders int32 [S] and kept uint8 [S]."""
    _mode(mode)
    if hasattr(intensities, "is_cuda"):                            # a torch tensor
        torch = _engine._torch()
        d_int = intensities.contiguous()
        if d_int.dim() != 2 or d_int.dtype != torch.float64:
            raise ValueError("a float64 [n, F] tensor is needed")
        n, F = int(d_int.shape[0]), int(d_int.shape[1])
        _check_frames(F)
        if n >= 1 << 31:
            raise ValueError("fewer than 2^31 tracks are needed")
        dev = d_int.device
        if n and not bool(torch.isfinite(d_int).all()):
            raise ValueError("intensities must be finite")
        if n and float(d_int.abs().max()) > MAX_MAGNITUDE:
            raise ValueError("intensities are limited to a magnitude of 2^52")
        d_cat = categories if torch.is_tensor(categories) else torch.from_numpy(_tracks.category_words(categories, n, F).view(np.int64))
        d_cat = d_cat.to(dev).contiguous()
        d_ids = (segments if torch.is_tensor(segments) else torch.from_numpy(np.asarray(segments).astype(np.int64))).to(dev).reshape(-1)
        if int(d_cat.numel()) != n or int(d_ids.numel()) != n:
            raise ValueError("one category and one segment per track")
        d_sorted, d_order = torch.sort(d_ids, stable=True)
        d_unique, d_counts = torch.unique_consecutive(d_sorted, return_counts=True)
        d_off = torch.zeros(int(d_unique.numel()) + 1, dtype=torch.int64, device=dev)
        d_off[1:] = torch.cumsum(d_counts, 0)
        out = remainder_adjust_device(d_int[d_order].contiguous(), d_cat[d_order].contiguous(), d_off, mode, minimum_r_per_field)
        d_adjusted = torch.empty_like(out["adjusted"])
        d_adjusted[d_order] = out["adjusted"]
        host = _engine.to_host(out)
        host["adjusted"], host["segment_ids"] = d_adjusted.cpu().numpy(), d_unique.cpu().numpy()
        return host
    rows = _checked_rows(intensities)
    n, F = rows.shape
    cats = _tracks.category_words(categories, n, F)
    ids = np.asarray(segments).reshape(-1)
    if len(ids) != n:
        raise ValueError("one segment per track")
    order, unique, seg_off = _grouped(ids)
    host = _adjust(np.ascontiguousarray(rows[order]), np.ascontiguousarray(cats[order]), seg_off, mode, minimum_r_per_field, device)
    adjusted = np.empty_like(host["adjusted"])
    adjusted[order] = host["adjusted"]
    host["adjusted"], host["segment_ids"] = adjusted, unique
    return host


# ---- the reference's call surface ----

def _unwound(photometries, num_frames):
    """(segment keys, one segment index per track, tracks) of the nested dict, after the checks on every track."""
    F = int(num_frames)
    _check_frames(F)
    keys, seg, tracks = [], [], []
    for channel, cdict in photometries.items():
        for field, fdict in cdict.items():
            keys.append((channel, field))
            for hw, (category, intensities, row) in fdict.items():
                if len(intensities) != F or len(category) != F:
                    raise ValueError("channel %s field %s %s: %d frames are needed in intensities and category"
                                     % (channel, field, hw, F))
                seg.append(len(keys) - 1)
                tracks.append((hw, category, intensities, row))
    return keys, seg, tracks


def _adjust_dict(photometries, num_frames, minimum_r_per_field, mode, device):
    keys, seg, tracks = _unwound(photometries, num_frames)
    F = int(num_frames)
    rows = _checked_rows([t[2] for t in tracks], F)
    cats = _tracks.category_words([t[1] for t in tracks], len(tracks))
    seg_off = np.searchsorted(np.asarray(seg, dtype=np.int64), np.arange(len(keys) + 1)).astype(np.int64)
    host = _adjust(rows, cats, seg_off, mode, minimum_r_per_field, device)
    adjusted, medians = {}, {}
    for s, (channel, field) in enumerate(keys):
        if not host["kept"][s]:
            continue
        medians.setdefault(channel, {})[field] = list(host["adjustment"][s])
        fdict = adjusted.setdefault(channel, {}).setdefault(field, {})
        for t in range(int(seg_off[s]), int(seg_off[s + 1])):
            hw, category, _, row = tracks[t]
            fdict[hw] = (category, list(host["adjusted"][t]), row)
    return adjusted, medians


def remainder_adjust_2(photometries, num_frames, minimum_r_per_field=5, device=None):
    """MCsimlib._remainder_adjust_2 (:3434-3472): (adjusted_photometries, adjustment_ratio_medians).  A channel without a
    kept field is in neither.  device=None: numpy on the host; else the GPU to use."""
    return _adjust_dict(photometries, num_frames, minimum_r_per_field, 'ratio', device)


def remainder_adjust(photometries, num_frames, minimum_r_per_field=5, device=None):
    """MCsimlib._remainder_adjust (:3398-3431): (adjusted_photometries, remainder_adjustments), the additive variant."""
    return _adjust_dict(photometries, num_frames, minimum_r_per_field, 'additive', device)


def adjusted_photometries_as_read(adjusted):
    """The nested dict lognormal.read_track_photometries_csv(path, downstep_filtered=False)[0] gives on the file
    write_adjusted_csv writes from `adjusted`, without the file: every value through Python 2's str() and the reader's
    int(round(float(text))), rows numbered as written.  (A value that is not finite raises as the reader does.)"""
    d = {}
    for r, (channel, field, h, w, category, intensities, _) in enumerate(unwind_photometries(adjusted), 1):   # (the header is row 0)
        vals = tuple(int(_py2_round(float(_py2_str(np.float64(v))))) for v in intensities)
        d.setdefault(str(channel), {}).setdefault(int(field), {}).setdefault((int(h), int(w)), (tuple(bool(c) for c in category), vals, r))
    return d


def write_adjusted_csv(adjusted, num_frames, path):
    """remainder_correction.py:200-210: CHANNEL, FIELD, H, W, CATEGORY and the frames of every track, floats as Python 2 wrote
    them, lines ended as the csv module ends them."""
    import csv
    with open(path, 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(["CHANNEL", "FIELD", "H", "W", "CATEGORY"] + ["FRAME " + str(frame) for frame in range(num_frames)])
        for channel, field, h, ww, category, intensities, _ in unwind_photometries(adjusted):
            w.writerow([str(channel), str(field), str(h), str(ww), str(category)] + [_py2_str(np.float64(v)) for v in intensities])
    return path
