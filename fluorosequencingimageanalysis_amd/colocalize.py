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

Limits: at most 4 letters, tables of one frame count of at most 64, |coordinate| < 2^30 after the offset (ValueError), and the
joint key's (signal_sweep: NotImplementedError naming the drop limit, ValueError naming table_slots=)."""
import numpy as np

from . import _host_colocalize as H
from . import _native_colocalize as NCL
from . import engine as _engine

ON_FILTERED = ('reject', 'dark')


# ---- one match ----

def _launch_match(d_a_hw, d_a_seg, d_a_off, d_b_hw, d_b_off, radius_sq):
    """fsq_colocalize_match on device tensors: (match_of_a, match_of_b, dist_sq_of_a, bad int32 [1]).  Enqueued on the current
    stream, not synchronised."""
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


def joint_observed_records(tables, beta_sigma, radius=2, offsets=None, max_possible=5, ddif=0.30, allow_multidrop=True, truncate=0,
                           beta=None, no_adjustment=False, solver='enumerate', on_filtered='reject', table_slots=1024, device=None,
                           host=False):
    """The joint observed signals of {letter: track table}, a table being lognormal.track_table_from_photometries' or
    track_table_from_records' 5-tuple with downstep_filtered=False: (intensity [n, F], category words [n], field [n], hw [n, 2],
    row [n]).  offsets: {letter: (dh, dw)} integers, (0, 0) where absent.  beta_sigma, ddif, truncate and beta are one value
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
    hw_field, offs = [(t[3], t[2]) for t in tabs], _letter_offsets(offsets, letters)
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
    return {"signals": signals, "n_molecules": M, "n_rejected": n_rejected, "total_count": M - n_rejected, "none_count": none_count,
            "labels": letters, "molecules": mols, "rejected": to_np(rejected), "kept": kept,
            "fit_index": to_np(xp.where(lit, index, xp.full_like(index, -1))), "channels": channels}
