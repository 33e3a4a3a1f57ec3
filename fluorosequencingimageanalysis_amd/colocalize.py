"""Joint observed signals of an experiment with several colour channels: which tracks of the channels are the same molecule,
decided on the GPU, every channel fitted with the lognormal chain, and the joint signals tallied - the observed side of
signal_sweep's joint sweeps (sweep_peptide SEQUENCE KC --observed JOINT.pkl), from a track table.

The reference stops at one label letter; like the joint signal itself this is a definition of this package
(include/fsq_colocalize.h), in exact integers:

  a track's position is its (h, w) plus its channel's integer offset (dh, dw); positions are compared as given;
  two tracks of one field match when each is the other's nearest (smallest (d2, index), d2 = dh^2 + dw^2 <= floor(radius^2)):
  mutual nearest neighbours, ties to the lowest index, no second choice;
  the molecules start as the first channel's tracks; every further channel's tracks are matched against them, a matched track
  becomes its molecule's member and the others are appended as new molecules in track order; at the end the molecules are
  sorted stably by field.  A molecule keeps its first member's position.

joint_observed_records then fits the downstep-filtered tracks of every channel with lognormal.chain_records, unchanged - each
channel's alpha, beta and fits are what lognormal_fitter_v2 gives for it alone - and tallies one joint signal per molecule by
signal_sweep.joint_signals_of_fits' rule: a channel without a member is dark (a row of zeros), a molecule with a member that
fails the downstep filter is rejected (on_filtered='dark': that channel counts as dark; a molecule left with no lit channel is
rejected all the same), a molecule with a lit channel whose second fit found nothing counts into none_count.

The channels' integer offsets are an input, or estimated from the tracks themselves (include/fsq_channel_offset.h;
estimate_offset_device, estimate_offset_records, estimate_offsets_records, joint_observed_records(offsets='estimate')): all pairs
of one field vote for their displacement a - b within a window, every offset of [-max_shift, max_shift]^2 is scored by the
pairs it brings within the match's radius, and the largest score wins, ties to the smallest (dh^2 + dw^2, dh, dw).  Every
further channel is estimated against the first one, whose tracks the molecules start from.

Limits: at most 4 letters, tables of one frame count of at most 64, |coordinate| < 2^30 after the offset (ValueError), and the
joint key's (signal_sweep: NotImplementedError naming the drop limit, ValueError naming table_slots=)."""
import math
import re

import numpy as np

from . import _host_channel_offset as HO
from . import _host_colocalize as H
from . import _native_channel_offset as NCO
from . import _native_colocalize as NCL
from . import engine as _engine

ON_FILTERED = ('reject', 'dark')
ESTIMATE = 'estimate'


# ---- one match ----

def _segment_sizes(d_a_hw, d_a_seg, d_a_off, d_b_hw, d_b_off):
    """(n_a, n_b, n_seg) of the five tensors that fsq_colocalize_match and fsq_channel_offset_votes share, after their checks."""
    torch = _engine._torch()
    n_a, n_b, n_seg = int(d_a_hw.shape[0]), int(d_b_hw.shape[0]), int(d_a_off.numel()) - 1
    tensors = (d_a_hw, d_a_seg, d_a_off, d_b_hw, d_b_off)
    if d_a_hw.dim() != 2 or d_b_hw.dim() != 2 or d_a_hw.shape[1] != 2 or d_b_hw.shape[1] != 2 \
            or d_a_hw.dtype != torch.int32 or d_b_hw.dtype != torch.int32:
        raise ValueError("int32 positions [n, 2] are needed")
    if d_a_seg.dtype != torch.int32 or tuple(d_a_seg.shape) != (n_a,):
        raise ValueError("one int32 segment per a is needed")
    if d_a_off.dtype != torch.int64 or d_b_off.dtype != torch.int64 or d_a_off.dim() != 1 or n_seg < 0 \
            or tuple(d_b_off.shape) != tuple(d_a_off.shape):
        raise ValueError("int64 offsets [n_seg + 1] are needed for a and for b")
    if not all(t.is_contiguous() for t in tensors) or not d_a_hw.is_cuda or any(t.device != d_a_hw.device for t in tensors):
        raise ValueError("contiguous tensors on one GPU are needed")
    if max(n_a, n_b, n_seg) >= 1 << 31:
        raise ValueError("fewer than 2^31 positions and segments are needed")
    return n_a, n_b, n_seg


def _launch_match(d_a_hw, d_a_seg, d_a_off, d_b_hw, d_b_off, radius_sq):
    """fsq_colocalize_match on device tensors: (match_of_a, match_of_b, dist_sq_of_a, bad int32 [1]).  Enqueued on the current
    stream, not synchronised."""
    torch = _engine._torch()
    n_a, n_b, n_seg = _segment_sizes(d_a_hw, d_a_seg, d_a_off, d_b_hw, d_b_off)
    radius_sq = int(radius_sq)
    if not 0 <= radius_sq < 1 << 63:
        raise ValueError("radius_sq must not be negative")
    dev = d_a_hw.device
    match_of_a = torch.empty(n_a, dtype=torch.int32, device=dev)
    match_of_b = torch.empty(n_b, dtype=torch.int32, device=dev)
    dist_sq_of_a = torch.empty(n_a, dtype=torch.int64, device=dev)
    d_bad = torch.empty(1, dtype=torch.int32, device=dev)
    ptr = lambda t: t.data_ptr() if t.numel() else None                                  # noqa: E731
    _engine.launch(NCL.lib().fsq_colocalize_match, "fsq_colocalize_match", dev, ptr(d_a_hw), ptr(d_a_seg), d_a_off.data_ptr(),
                   d_b_off.data_ptr(), ptr(d_b_hw), radius_sq, n_a, n_b, n_seg, ptr(match_of_a), ptr(match_of_b), ptr(dist_sq_of_a),
                   d_bad.data_ptr())
    return match_of_a, match_of_b, dist_sq_of_a, d_bad


def _check_device_positions(d_hw, what="positions"):
    if d_hw.numel() and int(d_hw.abs().max()) >= NCL.COORD_LIMIT:
        raise ValueError("%s need |coordinate| < 2^30" % what)


def match_device(d_a_hw, d_a_seg, d_a_off, d_b_hw, d_b_off, radius_sq):
    """One match of A against B on the device: int32 positions [n, 2] (|coordinate| < 2^30), d_a_seg int32 [n_a], the
    contiguous per-field ranges d_a_off and d_b_off int64 [n_seg + 1].  Returns the CUDA tensors (match_of_a int32 [n_a],
    match_of_b int32 [n_b], dist_sq_of_a int64 [n_a]), -1 where unmatched.  Segments or offsets that are not well formed raise
    ValueError (the kernel's flag and the largest coordinate cross to the host)."""
    _check_device_positions(d_a_hw, "a_hw")
    _check_device_positions(d_b_hw, "b_hw")
    match_of_a, match_of_b, dist_sq_of_a, d_bad = _launch_match(d_a_hw, d_a_seg, d_a_off, d_b_hw, d_b_off, radius_sq)
    if int(d_bad):
        raise ValueError("a_seg or the offsets are not well formed")
    return match_of_a, match_of_b, dist_sq_of_a


def match_records(a_hw, a_seg, a_off, b_hw, b_off, radius_sq, host=False, device=None):
    """match_device for NumPy arrays, as NumPy arrays; host=True: the NumPy twin, without a GPU."""
    if host:
        return H.match(a_hw, a_seg, a_off, b_hw, b_off, radius_sq)
    torch = _engine._torch()
    dev = torch.device(device or "cuda")
    a_hw, b_hw = H.check_positions(a_hw, "a_hw"), H.check_positions(b_hw, "b_hw")
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).to(dev)           # noqa: E731
    out = match_device(up(a_hw, np.int32), up(np.asarray(a_seg).reshape(-1), np.int32), up(np.asarray(a_off).reshape(-1), np.int64),
                       up(b_hw, np.int32), up(np.asarray(b_off).reshape(-1), np.int64), radius_sq)
    return tuple(t.cpu().numpy() for t in out)


# ---- the offset between two channels (include/fsq_channel_offset.h) ----

def _launch_votes(d_a_hw, d_a_seg, d_a_off, d_b_hw, d_b_off, W):
    """fsq_channel_offset_votes on device tensors: (votes int64 [2W + 1, 2W + 1], bad int32 [1]).  Enqueued on the current
    stream, not synchronised."""
    torch = _engine._torch()
    n_a, n_b, n_seg = _segment_sizes(d_a_hw, d_a_seg, d_a_off, d_b_hw, d_b_off)
    W = int(W)
    if not 0 <= W <= NCO.MAX_W:
        raise ValueError("W must be 0 .. %d" % NCO.MAX_W)
    dev = d_a_hw.device
    d_votes = torch.empty((2 * W + 1, 2 * W + 1), dtype=torch.int64, device=dev)
    d_bad = torch.empty(1, dtype=torch.int32, device=dev)
    ptr = lambda t: t.data_ptr() if t.numel() else None                                  # noqa: E731
    _engine.launch(NCO.lib().fsq_channel_offset_votes, "fsq_channel_offset_votes", dev, ptr(d_a_hw), ptr(d_a_seg), d_a_off.data_ptr(),
                   d_b_off.data_ptr(), ptr(d_b_hw), W, n_a, n_b, n_seg, d_votes.data_ptr(), d_bad.data_ptr())
    return d_votes, d_bad


def offset_votes_device(d_a_hw, d_a_seg, d_a_off, d_b_hw, d_b_off, W):
    """The votes of A against B on the device, tensors as for match_device: the CUDA tensor V int64 [2W + 1, 2W + 1],
    V[dh + W, dw + W] = the pairs (a, b) of one field with a - b = (dh, dw), 0 <= W <= 64.  Segments or offsets that are not
    well formed, or a field of 2^24 or more b's, raise ValueError."""
    _check_device_positions(d_a_hw, "a_hw")
    _check_device_positions(d_b_hw, "b_hw")
    d_votes, d_bad = _launch_votes(d_a_hw, d_a_seg, d_a_off, d_b_hw, d_b_off, W)
    if int(d_bad):
        raise ValueError(HO.NOT_WELL_FORMED)
    return d_votes


def offset_peak_device(d_votes, R, tol_sq, scores=False):
    """fsq_channel_offset_peak on a CUDA tensor of votes int64 [2W + 1, 2W + 1]: the record int64 [16] as a CUDA tensor (dh,
    dw, score, runner_up, total, at_edge, n_ties, the 3 x 3 of V around the peak); scores=True: (record, S int64 [2R + 1,
    2R + 1]).  0 <= R, 0 <= tol_sq and R + isqrt(tol_sq) <= W are needed (ValueError).  Not synchronised."""
    torch = _engine._torch()
    if d_votes.dtype != torch.int64 or d_votes.dim() != 2 or d_votes.shape[0] != d_votes.shape[1] or not d_votes.shape[0] & 1 \
            or d_votes.shape[0] > 2 * NCO.MAX_W + 1 or not d_votes.is_cuda or not d_votes.is_contiguous():
        raise ValueError("votes are a contiguous int64 CUDA tensor [2W + 1, 2W + 1] with W <= %d" % NCO.MAX_W)
    W, R, tol_sq = int(d_votes.shape[0]) // 2, int(R), int(tol_sq)
    if R < 0 or tol_sq < 0 or R + math.isqrt(tol_sq) > W:
        raise ValueError("0 <= R, 0 <= tol_sq and R + isqrt(tol_sq) <= W = %d are needed" % W)
    dev = d_votes.device
    d_record = torch.empty(NCO.RECORD, dtype=torch.int64, device=dev)
    d_scores = torch.empty((2 * R + 1, 2 * R + 1), dtype=torch.int64, device=dev) if scores else None
    _engine.launch(NCO.lib().fsq_channel_offset_peak, "fsq_channel_offset_peak", dev, d_votes.data_ptr(), W, R, tol_sq,
                   d_record.data_ptr(), d_scores.data_ptr() if scores else None)
    return (d_record, d_scores) if scores else d_record


def estimate_offset_device(d_a_hw, d_a_seg, d_a_off, d_b_hw, d_b_off, max_shift=16, tol_sq=4):
    """The integer offset to add to B's positions so that they land on A's, tensors as for match_device: the offset of
    [-max_shift, max_shift]^2 under which the most pairs of one field lie within tol_sq of each other (ties to the smallest
    (dh^2 + dw^2, dh, dw)).  Returns a dict: offset (dh, dw), score, runner_up (the best score further than 2 isqrt(tol_sq)
    from the peak, -1 without such an offset), total (all votes), at_edge (the peak stands on the window's edge: the true
    offset may lie outside), n_ties, centroid (float64 (h, w), from the 3 x 3 of votes around the peak; informational) and
    votes (the CUDA tensor int64 [2W + 1, 2W + 1], W = max_shift + isqrt(tol_sq) <= 64, else ValueError).  Two launches; the
    128-byte record and the error flags cross to the host."""
    W, R, _ = HO.window(max_shift, tol_sq)
    d_votes = offset_votes_device(d_a_hw, d_a_seg, d_a_off, d_b_hw, d_b_off, W)
    return HO.estimate_of(offset_peak_device(d_votes, R, tol_sq).cpu().numpy(), d_votes)


def estimate_offset_records(a_hw, a_field, b_hw, b_field, max_shift=16, radius=2, host=False, device=None):
    """estimate_offset_device for NumPy positions [n, 2] and one field per position, the tolerance being the match's own
    radius_sq_of(radius); `votes` comes back as a NumPy array.  host=True: the NumPy twin, without a GPU."""
    tol_sq = H.radius_sq_of(radius)
    W, R, _ = HO.window(max_shift, tol_sq)
    a_hw, b_hw = H.check_positions(a_hw, "a_hw"), H.check_positions(b_hw, "b_hw")
    a_field, b_field = (np.asarray(f).reshape(-1) for f in (a_field, b_field))
    if len(a_field) != len(a_hw) or len(b_field) != len(b_hw) or any(f.size and f.dtype.kind not in "iu" for f in (a_field, b_field)):
        raise ValueError("one integer field per position is needed")
    ids = np.unique(np.concatenate([a_field.astype(np.int64), b_field.astype(np.int64)]))
    a_order, a_seg, a_off = H.grouped(a_field, ids)
    b_order, _, b_off = H.grouped(b_field, ids)
    if host:
        V = HO.votes(a_hw[a_order], a_seg, a_off, b_hw[b_order], b_off, W)
        return HO.estimate_of(HO.peak(V, R, tol_sq), V)
    torch = _engine._torch()
    dev = torch.device(device or "cuda")
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).to(dev)           # noqa: E731
    out = estimate_offset_device(up(a_hw[a_order], np.int32), up(a_seg, np.int32), up(a_off, np.int64), up(b_hw[b_order], np.int32),
                                 up(b_off, np.int64), max_shift, tol_sq)
    out["votes"] = out["votes"].cpu().numpy()
    return out


def estimate_offsets_records(tables_hw_field, radius, max_shift=16, offsets=None, min_score=1, host=False, device=None):
    """The offsets of K channels for molecules_*: tables_hw_field per channel (hw [n, 2], field [n]); offsets: None, or per
    channel (dh, dw) or None for a channel to estimate (channel 0: None is (0, 0)).  Every channel k >= 1 without an offset is
    estimated against channel 0 - a molecule keeps its first member's position, so channel 0 is the anchor - after channel 0's
    own offset was applied: K - 1 vote launches at the most.  Returns (offsets [K] of (dh, dw), estimates [K]:
    estimate_offset_records' dict of an estimated channel, None for the others).  A score below min_score raises ValueError
    naming the channel and max_shift=."""
    tables = list(tables_hw_field)
    K = len(tables)
    offsets = [None] * K if offsets is None else list(offsets)
    if len(offsets) != K:
        raise ValueError("one (dh, dw) offset, or None, per channel is needed")
    given = [(0, 0) if o is None else o for o in offsets]
    checked = H.checked_tables(tables, given)                          # (the given offsets are applied here, exactly)
    out, estimates = list(given), [None] * K
    for k in range(1, K):
        if offsets[k] is not None:
            continue
        est = estimate_offset_records(checked[0][0], checked[0][1], checked[k][0], checked[k][1], max_shift, radius, host=host,
                                      device=device)
        if est["score"] < int(min_score):
            raise ValueError("channel %d: the best offset within max_shift=%d pairs %d tracks, fewer than min_score=%d"
                             % (k, int(max_shift), est["score"], int(min_score)))
        out[k], estimates[k] = est["offset"], est
    return out, estimates


# ---- the merge over K channels ----

def _grouped_device(d_field, d_field_ids):
    """_host_colocalize.grouped on the device: (order, int32 segment per sorted element, int64 offsets [n_seg + 1])."""
    torch = _engine._torch()
    d_sorted, d_order = torch.sort(d_field, stable=True)
    d_seg = torch.searchsorted(d_field_ids, d_sorted)
    d_off = torch.searchsorted(d_seg, torch.arange(int(d_field_ids.numel()) + 1, dtype=torch.int64, device=d_field.device))
    return d_order, d_seg.to(torch.int32), d_off.contiguous()


def molecules_device(tables_hw_field, radius, offsets=None):
    """The merge over K channels on the device.  tables_hw_field: per channel (hw [n, 2], field [n]) as integer CUDA tensors;
    offsets: per channel (dh, dw) integers.  Returns the CUDA tensors {member int32 [K, M] (the track of every channel in that
    channel's table, or -1), field int64 [M], hw int64 [M, 2]}.  K - 1 launches of fsq_colocalize_match; the append and the
    stable sorts are torch operations on the device, and only sizes (and the error flags) cross to the host."""
    torch = _engine._torch()
    r2 = H.radius_sq_of(radius)
    tables = list(tables_hw_field)
    K = len(tables)
    if not 1 <= K <= NCL.MAX_CHANNELS:
        raise ValueError("1 .. %d channels are needed, not %d" % (NCL.MAX_CHANNELS, K))
    offsets = [(0, 0)] * K if offsets is None else [tuple(int(x) for x in o) for o in offsets]
    if len(offsets) != K or any(len(o) != 2 for o in offsets):
        raise ValueError("one (dh, dw) offset per channel is needed")
    dev = tables[0][0].device
    chans = []
    for k, ((d_hw, d_field), off) in enumerate(zip(tables, offsets)):
        if d_hw.is_floating_point() or d_field.is_floating_point() or d_hw.dim() != 2 or d_hw.shape[1] != 2 \
                or tuple(d_field.shape) != (int(d_hw.shape[0]),) or not d_hw.is_cuda or d_hw.device != dev or d_field.device != dev:
            raise ValueError("integer positions [n, 2] and fields [n] on one GPU are needed")
        if max(abs(off[0]), abs(off[1])) >= 1 << 31:
            raise ValueError("channel %d: positions need |coordinate| < 2^30 after the offset" % k)
        d_hw = d_hw.to(torch.int64) + torch.tensor(off, dtype=torch.int64, device=dev)
        _check_device_positions(d_hw, "channel %d: after the offset, positions" % k)
        chans.append((d_hw, d_field.to(torch.int64)))
    d_field_ids = torch.unique(torch.cat([f for _, f in chans]))
    d_hw0, d_f0 = chans[0]
    d_order, _, _ = _grouped_device(d_f0, d_field_ids)
    mol_hw, mol_field = d_hw0[d_order], d_f0[d_order]
    member = torch.full((K, int(d_order.numel())), -1, dtype=torch.int32, device=dev)
    member[0] = d_order.to(torch.int32)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    for k in range(1, K):
        d_hw, d_field = chans[k]
        b_order, _, b_off = _grouped_device(d_field, d_field_ids)
        _, a_seg, a_off = _grouped_device(mol_field, d_field_ids)      # (the molecules stand sorted: their order is the identity)
        match_of_a, match_of_b, _, d_bad = _launch_match(mol_hw.to(torch.int32).contiguous(), a_seg.contiguous(), a_off,
                                                         d_hw[b_order].to(torch.int32).contiguous(), b_off, r2)
        bad |= d_bad
        if int(b_order.numel()):
            paired = match_of_a >= 0
            member[k] = torch.where(paired, b_order[match_of_a.clamp(min=0).to(torch.int64)].to(torch.int32),
                                    torch.full_like(match_of_a, -1))
        new = torch.sort(b_order[match_of_b < 0]).values               # the unmatched tracks, in track order
        more = torch.full((K, int(new.numel())), -1, dtype=torch.int32, device=dev)
        more[k] = new.to(torch.int32)
        member = torch.cat([member, more], dim=1)
        mol_hw, mol_field = torch.cat([mol_hw, d_hw[new]]), torch.cat([mol_field, d_field[new]])
        order = torch.sort(mol_field, stable=True).indices
        member, mol_hw, mol_field = member[:, order], mol_hw[order], mol_field[order]
    if int(bad):
        raise RuntimeError("fsq_colocalize_match refused segments that molecules_device built (a bug)")
    return {"member": member.contiguous(), "field": mol_field, "hw": mol_hw}


def molecules_records(tables_hw_field, radius, offsets=None, host=False, device=None):
    """molecules_device for NumPy arrays, as NumPy arrays: {member int32 [K, M], field int64 [M], hw int64 [M, 2]}.  host=True:
    the NumPy twin (_host_colocalize.molecules), without a GPU."""
    if host:
        return H.molecules(tables_hw_field, radius, offsets)
    torch = _engine._torch()
    dev = torch.device(device or "cuda")
    H.radius_sq_of(radius)
    tables = H.checked_tables(tables_hw_field, offsets)                # (the offsets are applied here, exactly)
    out = molecules_device([(torch.from_numpy(hw).to(dev), torch.from_numpy(field).to(dev)) for hw, field in tables], radius)
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- joint observed signals ----

def downstep_filtered(words, F):
    """bool [n]: the category words (bit f: ON at frame f) that are ON in a prefix of the F frames, from frame 0 - the tracks
    read_track_photometries_csv(downstep_filtered=True) keeps."""
    words = np.asarray(words).astype(np.uint64)
    word = words & (np.uint64(0xFFFFFFFFFFFFFFFF) if F >= 64 else np.uint64((1 << F) - 1))
    return ((word & (word + np.uint64(1))) == 0) & ((word & np.uint64(1)) == 1)


def _per_letter(value, name, letters):
    from .peptide_simulator import _per_letter as per
    return per({name: value}, name, letters, None)


def _letter_offsets(offsets, letters):
    if offsets is None:
        return [(0, 0)] * len(letters)
    unknown = sorted(set(offsets) - set(letters))
    if unknown:
        raise ValueError("offsets name the letters %s, which have no table" % unknown)
    return [tuple(offsets.get(L, (0, 0))) for L in letters]


def _offsets_to_estimate(offsets, letters):
    """(offsets per letter with None where one is to be estimated, whether any is): offsets='estimate' asks for every letter
    but the first, a dict may ask with the value 'estimate' letter by letter."""
    if isinstance(offsets, str):
        if offsets != ESTIMATE:
            raise ValueError("offsets must be a dict {letter: (dh, dw)}, None or 'estimate'")
        return [(0, 0)] + [None] * (len(letters) - 1), True
    asked = {L for L, o in (offsets or {}).items() if isinstance(o, str)}
    if not asked:
        return _letter_offsets(offsets, letters), False
    if any(offsets[L] != ESTIMATE for L in asked) or letters[0] in asked:
        raise ValueError("an offset is (dh, dw) or, for a letter other than the first, 'estimate'")
    per = _letter_offsets({L: ((0, 0) if L in asked else o) for L, o in offsets.items()}, letters)
    return [None if L in asked else o for L, o in zip(letters, per)], True


def joint_observed_records(tables, beta_sigma, radius=2, offsets=None, max_possible=5, ddif=0.30, allow_multidrop=True, truncate=0,
                           beta=None, no_adjustment=False, solver='enumerate', on_filtered='reject', table_slots=1024, device=None,
                           host=False, max_shift=16, min_score=1):
    """The joint observed signals of {letter: track table}, a table being lognormal.track_table_from_photometries' or
    track_table_from_records' 5-tuple with downstep_filtered=False: (intensity [n, F], category words [n], field [n], hw [n, 2],
    row [n]).  offsets: {letter: (dh, dw)} integers, (0, 0) where absent; or 'estimate': every letter but the first is estimated
    against the first (estimate_offsets_records: the window is max_shift, the tolerance the call's radius, a score below min_score
    raises ValueError), or a dict with the value 'estimate' for the letters to estimate.  Only then does the returned dict gain
    offsets {letter: (dh, dw)} and offset_estimates {estimated letter: estimate_offset_records' dict}.  beta_sigma, ddif, truncate and beta are one value
    for all letters or a dict {letter: value}.  Returns a dict:

      signals       {joint_signal: n}, what sweep_peptide --observed and signal_sweep.score_records take
      n_molecules, n_rejected, total_count (= n_molecules - n_rejected = the signals' sum + none_count), none_count
      labels        the sorted letters
      molecules     {member int32 [K, M], field int64 [M], hw int64 [M, 2]} as NumPy arrays
      rejected      bool [M]
      kept          {letter: the indices of the channel's downstep-filtered tracks in its table}
      fit_index     int64 [K, M]: the row of the member in channels[letter]'s per-track arrays, -1 for a dark channel
      channels      {letter: lognormal.chain_records' dict of the channel's downstep-filtered tracks}

    A channel without a downstep-filtered track raises chain_records' ValueError.  On the device the molecules come from
    molecules_device and the [K][M][F] rows and flags are gathered from the channels' second fits by torch indexing; there is no
    Python loop over molecules.  host=True: the twins and chain_records(host=True) end to end, without a GPU."""
    from . import _host_lognormal_chain as HC
    from . import lognormal as LN
    from . import signal_sweep as SW
    letters = tuple(sorted(tables))
    K = len(letters)
    if not 1 <= K <= H.MAX_CHANNELS or any(not isinstance(L, str) or len(L) != 1 for L in letters):
        raise ValueError("1 .. %d label letters are needed, one table each" % H.MAX_CHANNELS)
    if on_filtered not in ON_FILTERED:
        raise ValueError("on_filtered must be 'reject' or 'dark'")
    slots = int(table_slots)
    if slots < 1 or slots & (slots - 1) or slots > SW.NS.MAX_SLOTS:
        raise ValueError("table_slots=%d must be a power of two up to 2^24" % slots)
    H.radius_sq_of(radius)
    tabs = []
    for L in letters:
        intensity, words, field, hw, row = tables[L]
        intensity = np.ascontiguousarray(intensity, dtype=np.float64)
        if intensity.ndim != 2:
            raise ValueError("letter %s: intensities [n, F] are needed" % L)
        n = len(intensity)
        words, field, row = (np.asarray(x).reshape(-1) for x in (words, field, row))
        if not len(words) == len(field) == len(row) == n or np.asarray(hw).size != 2 * n:
            raise ValueError("letter %s: one category word, field, position and row per track are needed" % L)
        tabs.append((intensity, words.astype(np.uint64), field, np.asarray(hw).reshape(n, 2), row))
    F = tabs[0][0].shape[1]
    if any(t[0].shape[1] != F for t in tabs):
        raise ValueError("every channel needs the same number of frames, not %s" % sorted({t[0].shape[1] for t in tabs}))
    HC.check_frames(F, allow_multidrop)
    sigmas, ddifs, truncs, betas = (_per_letter(v, name, letters) for v, name in
                                    ((beta_sigma, 'beta_sigma'), (ddif, 'ddif'), (truncate, 'truncate'), (beta, 'beta')))
    hw_field, (offs, estimated) = [(t[3], t[2]) for t in tabs], _offsets_to_estimate(offsets, letters)
    if estimated:
        try:
            offs, estimates = estimate_offsets_records(hw_field, radius, max_shift, offs, min_score, host=host, device=device)
        except ValueError as e:                                        # (a channel by its letter)
            k = re.match(r"channel (\d+): ", str(e))
            raise ValueError("letter %s: %s" % (letters[int(k.group(1))], str(e)[k.end():])) if k else e
    if host:
        mols = H.molecules(hw_field, radius, offs)
    else:
        torch = _engine._torch()
        dev = torch.device(device or "cuda")
        checked = H.checked_tables(hw_field, offs)
        d_mols = molecules_device([(torch.from_numpy(hw).to(dev), torch.from_numpy(field).to(dev)) for hw, field in checked], radius)
        mols = {k: v.cpu().numpy() for k, v in d_mols.items()}
    channels, kept = {}, {}
    for k, L in enumerate(letters):
        intensity, words, field, _, _ = tabs[k]
        at = np.flatnonzero(downstep_filtered(words, F))
        kept[L] = at
        channels[L] = LN.chain_records(intensity[at], words[at], field[at], sigmas[k], max_possible=max_possible, ddif=ddifs[k],
                                       allow_multidrop=allow_multidrop, truncate=truncs[k], beta=betas[k], no_adjustment=no_adjustment,
                                       device=device, host=host, solver=solver)
    # per channel: where a track stands among the fitted ones (-1: it failed the filter), and the second fit's rows
    where = []
    for k, L in enumerate(letters):
        w = np.full(len(tabs[k][0]) + 1, -1, np.int64)                 # (one spare entry: the index -1 of a missing member reads -1)
        w[kept[L]] = np.arange(len(kept[L]))
        where.append(w)
    if host:
        xp, member = np, mols["member"].astype(np.int64)
        stack, as_x = np.stack, lambda a: a                                             # noqa: E731
    else:
        xp, member = torch, d_mols["member"].to(torch.int64)
        stack, as_x = torch.stack, lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    index = stack([as_x(where[k])[member[k]] for k in range(K)])        # [K, M]
    has = member >= 0
    lit = has & (index >= 0)
    failed = has & (index < 0)
    rejected = ~lit.any(0) | failed.any(0) if on_filtered == 'reject' else ~lit.any(0)
    best, found = [], []
    for k, L in enumerate(letters):
        fit1 = channels[L]["fit1"]
        rows, status = as_x(fit1["best_seq"])[:, :F], as_x(fit1["status"])
        at = index[k].clip(0) if host else index[k].clamp(min=0)
        best.append(xp.where(lit[k][:, None], rows[at], xp.zeros_like(rows[at])))
        found.append(lit[k] & (status[at] == LN.STATUS_FOUND))
    best, found = stack(best), stack(found)
    keep = ~rejected
    none_count = int(((lit & ~found).any(0) & keep).sum())
    uint8 = np.uint8 if host else torch.uint8
    cast = (lambda a: a.astype(uint8)) if host else (lambda a: a.to(uint8))
    signals = SW.joint_signals_of_fits(letters, best[:, keep], cast(found[:, keep]), cast(lit[:, keep]), host=host, table_slots=slots,
                                       device=device)
    to_np = (lambda a: a) if host else (lambda a: a.cpu().numpy())
    M, n_rejected = int(member.shape[1]), int(rejected.sum())
    out = {"signals": signals, "n_molecules": M, "n_rejected": n_rejected, "total_count": M - n_rejected, "none_count": none_count,
           "labels": letters, "molecules": mols, "rejected": to_np(rejected), "kept": kept,
           "fit_index": to_np(xp.where(lit, index, xp.full_like(index, -1))), "channels": channels}
    if estimated:
        out["offsets"] = dict(zip(letters, offs))
        out["offset_estimates"] = {L: e for L, e in zip(letters, estimates) if e is not None}
    return out
