"""Sequence experiments from frames to the two CSV files without a Python object per Spot: the reference's
basic_experiment_script (fit every cycle's image, load the fits as Spots, register consecutive cycles, track, fill holes,
measure, count) as one chain of library calls on the device.

    fsq_find_peptides            every frame of every field and channel           (engine.PathRunner)
    fsq_experiment_spot_table    peak records -> Spot tables                      (include/fsq_experiment.h)
    fsq_phase_correlate          consecutive frames of every field                (phase_correlate.Registrar)
    fsq_greedy_tracking          one "field" per sequence
    fsq_experiment_trace_rows    traces -> rows of (h, w)                         (include/fsq_experiment.h)
    fsq_sequence_photometry      positions, validity, photometries, categories    (sequencing.run_device)
    fsq_sequence_category_counts all traces / the valid ones                      (sequencing.category_counts_device)

One *sequence* is one field of one channel; sequence s = field * channels + channel.  sequence_experiment_records returns flat
NumPy arrays; write_track_photometries_csv / write_category_counts_csv / summary_text turn them into the bytes the classes of
flexlibrary write (they share the text formatting with them)."""
import numpy as np

from . import _native as N
from . import _native_experiment as NX
from . import _native_sequence as NQ
from . import engine as _engine
from . import flexlibrary as _fl
from . import sequencing as _sq

CANDIDATE_RADIUS, SPOT_RADIUS = 2, 0            # SequenceExperiment.trace_existing_spots' arguments (flexlibrary.py:1770-1809)


def spot_table_device(d_records, d_peaks, H, W, spot_size=NX.SPOT_SIZE):
    """fsq_experiment_spot_table on device tensors: d_records uint8 [k, 378 | 428], d_peaks int32 [n_frames].  -> dict of device
    tensors hw int32 [k, 2], spot_record int32 [k] (the first n_spots rows are written), counts, discarded, status int32
    [n_frames], n_spots int32 [1].  Enqueued on the current stream, not synchronised."""
    torch = _engine._torch()
    dev = d_peaks.device
    k, n_frames = int(d_records.shape[0]), int(d_peaks.shape[0])
    L = NX.lib()
    ws_bytes = L.fsq_experiment_spot_table_workspace_bytes(k, n_frames)
    if ws_bytes < 0:
        raise ValueError("fsq_experiment_spot_table: invalid sizes")
    i32 = dict(dtype=torch.int32, device=dev)
    out = {"hw": torch.empty((max(k, 1), 2), **i32), "spot_record": torch.empty(max(k, 1), **i32),
           "counts": torch.empty(max(n_frames, 1), **i32), "discarded": torch.empty(max(n_frames, 1), **i32),
           "status": torch.empty(max(n_frames, 1), **i32), "n_spots": torch.empty(1, **i32)}
    ws = _engine.workspace(dev, ws_bytes)
    _engine.launch(L.fsq_experiment_spot_table, "fsq_experiment_spot_table", dev, d_records.data_ptr() if k else None, k,
                   int(d_records.shape[1]), d_peaks.data_ptr(), n_frames, int(H), int(W), int(spot_size), out["hw"].data_ptr(),
                   out["spot_record"].data_ptr(), out["counts"].data_ptr(), out["discarded"].data_ptr(), out["status"].data_ptr(),
                   out["n_spots"].data_ptr(), ws.data_ptr(), int(ws_bytes))
    out["hw"], out["spot_record"] = out["hw"][:k], out["spot_record"][:k]
    for name in ("counts", "discarded", "status"):
        out[name] = out[name][:n_frames]
    out["_ws"] = ws                   # (kept alive until the caller has read the outputs)
    return out


def trace_starts_device(d_n_traces):
    """fsq_experiment_trace_starts: int32 [n_seq] -> int32 [n_seq + 1] (exclusive scan; the last word is N).  Not synchronised."""
    torch = _engine._torch()
    n_seq = int(d_n_traces.shape[0])
    d_start = torch.empty(n_seq + 1, dtype=torch.int32, device=d_n_traces.device)
    _engine.launch(NX.lib().fsq_experiment_trace_starts, "fsq_experiment_trace_starts", d_n_traces.device,
                   d_n_traces.data_ptr() if n_seq else None, n_seq, d_start.data_ptr())
    return d_start


def trace_rows_device(d_traces, d_seq_start, d_field_start, d_hw, n_frames, n_rows):
    """fsq_experiment_trace_rows on device tensors (n_rows: the last word of d_seq_start, read back by the caller).  -> device
    tensors trace_hw int32 [N, F, 2], trace_spot int32 [N, F], trace_seq int32 [N].  Not synchronised."""
    torch = _engine._torch()
    dev = d_traces.device
    n_seq, F, n = int(d_seq_start.shape[0]) - 1, int(n_frames), int(n_rows)
    i32 = dict(dtype=torch.int32, device=dev)
    t_hw, t_spot, t_seq = torch.empty((max(n, 1), F, 2), **i32), torch.empty((max(n, 1), F), **i32), torch.empty(max(n, 1), **i32)
    _engine.launch(NX.lib().fsq_experiment_trace_rows, "fsq_experiment_trace_rows", dev, d_traces.data_ptr(), d_seq_start.data_ptr(),
                   d_field_start.data_ptr(), d_hw.data_ptr(), n_seq, F, n, t_hw.data_ptr(), t_spot.data_ptr(), t_seq.data_ptr())
    return t_hw[:n], t_spot[:n], t_seq[:n]


def _fit_device(torch, dev, d_frames3, fmt, pixel_max, params):
    """fsq_find_peptides on the uploaded frames [n, H, W] -> (runner, records view, peaks per frame int32 [n] on the device).  The
    records are a view of the cached runner's buffer: the caller holds runner.lock until it has read them."""
    from . import pflib as _pf
    p = dict(median_filter_size=5, correlation_matrix=_pf.default_correlation_matrix, c_std=2, r_2_threshold=0.7,
             consolidation_radius=4, solver='reference')
    unknown = set(params) - set(p) - {"fit_type", "candidate_pixels", "N_iter"}
    if unknown:
        raise TypeError("find_peptides got an unexpected keyword argument %r" % sorted(unknown)[0])
    p.update({k: v for k, v in params.items() if k in p})
    if params.get("fit_type", "gauss") != "gauss":
        raise NotImplementedError("fit_type='monte_carlo' draws from an unseeded RNG in the reference and is not reproduced")
    if params.get("candidate_pixels") is not None:
        raise NotImplementedError("candidate_pixels is not taken by the records route")
    mode = _pf._solver_mode(p["solver"])
    wide = fmt == N.PIXELS_U32
    if wide and mode == N.MODE_TEXTBOOK_F32:
        raise NotImplementedError("solver='textbook_f32' takes 16-bit pixels only")
    if p["consolidation_radius"] < 2:
        raise ValueError("consolidation_radius must be at least 2")
    prm = _engine.detect_params(p["median_filter_size"], p["correlation_matrix"], p["c_std"], fmt, pixel_max if wide else None)
    n, H, W = (int(x) for x in d_frames3.shape)
    per = min(n, max(1, _pf.CHUNK_PIXELS // (H * W)))              # frames per library call

    def build():
        import threading
        r = _engine.PathRunner(per, H, W, record_bytes=_engine.peak_record_bytes(fmt))
        r.lock = threading.Lock()
        return r
    runner = _pf._cached(("experiment", _pf._device_key(), per, H, W, wide), build)
    runner.lock.acquire()
    try:
        if per == n:
            rec, _, nk, _ = runner.run(d_frames3, prm, p["r_2_threshold"], p["consolidation_radius"], mode, _pf.PY2_ROUND)
            return runner, rec, nk[:n].contiguous()
        recs, peaks = [], []                                       # (a stack beyond one chunk: the runner's buffer is copied out chunk by chunk)
        for a in range(0, n, per):
            part = d_frames3[a:a + per]
            rec, _, nk, _ = runner.run(part, prm, p["r_2_threshold"], p["consolidation_radius"], mode, _pf.PY2_ROUND)
            recs.append(rec.clone())
            peaks.append(nk[:len(part)].clone())
    except BaseException:
        runner.lock.release()
        raise
    runner.lock.release()
    return None, torch.cat(recs), torch.cat(peaks)


def _offsets_device(torch, dev, d_align, is_u16, n_fields, F, H, W, upsample_factor):
    """phase_correlate.offsets_from_frames for every field in one fsq_phase_correlate call: d_align [n_fields, F, H, W] (16-bit
    words, or float64) -> float64 [n_fields, F, 2] on the device, [.., 0] = (0, 0), [.., f + 1] = the shift of frame f + 1
    relative to frame f."""
    from . import phase_correlate as _pc
    off = torch.zeros((n_fields, F, 2), dtype=torch.float64, device=dev)
    if F < 2:
        return off
    ref = d_align[:, :-1].reshape(n_fields * (F - 1), H, W).contiguous()
    reg = d_align[:, 1:].reshape(n_fields * (F - 1), H, W).contiguous()
    reg_out = _pc.Registrar(n_fields * (F - 1), H, W, upsample_factor, N.DTYPE_U16 if is_u16 else N.DTYPE_F64, dev).register(ref, reg)
    off[:, 1:] = reg_out[:, :2].reshape(n_fields, F - 1, 2)
    return off


def _track_device(torch, dev, d_hw, d_field_start, d_counts, d_off, n_seq, F, H, W, total, max_count):
    """fsq_greedy_tracking with everything left on the device; track_fields' capacity loop on FSQ_ERANGE reads the status words
    (and, in the same download, the number of trace rows).  -> (traces, n_traces, n_discarded, seq_start, status (host), N)."""
    L = N.lib()
    i32 = dict(dtype=torch.int32, device=dev)
    pair_cap = max(4096, 8 * int(max_count))
    d_prev, d_next = torch.empty(max(total, 1), **i32), torch.empty(max(total, 1), **i32)
    d_kept = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    d_traces = torch.empty(max(total, 1) * F, **i32)
    d_nt, d_nd, d_st = torch.empty(n_seq, **i32), torch.empty(n_seq, **i32), torch.empty(n_seq, **i32)
    while True:
        ws_bytes = L.fsq_track_workspace_bytes(n_seq, F, H, W, pair_cap)
        if ws_bytes < 0:
            raise ValueError("invalid tracking shape")
        ws = _engine.workspace(dev, ws_bytes)
        _engine.launch(L.fsq_greedy_tracking, "fsq_greedy_tracking", dev, d_hw.data_ptr(), d_field_start.data_ptr(), d_counts.data_ptr(),
                       d_off.data_ptr(), n_seq, F, H, W, CANDIDATE_RADIUS, float(SPOT_RADIUS), d_prev.data_ptr(), d_next.data_ptr(),
                       d_kept.data_ptr(), d_traces.data_ptr(), d_nt.data_ptr(), d_nd.data_ptr(), d_st.data_ptr(), pair_cap, ws.data_ptr(),
                       ws_bytes)
        # (a sequence that failed has no traces: its count is not read)
        d_start = trace_starts_device(torch.where(d_st == 0, d_nt, torch.zeros_like(d_nt)))
        word = torch.cat([d_st, d_start[-1:]]).cpu().numpy()
        st = word[:n_seq]
        if not (st == N.FSQ_ERANGE).any() or pair_cap >= (1 << 28):
            break
        pair_cap *= 4
    return d_traces, d_nt, d_nd, d_start, st, int(word[n_seq])


def _spots_argument(spots, n_fields, C, F):
    """spots[field][channel][frame] -> (hw int32 [k, 2], counts int32 [n_seq * F]) in sequence order."""
    parts, counts = [], np.zeros(n_fields * C * F, np.int32)
    if len(spots) != n_fields:
        raise ValueError("spots must hold one entry per field")
    i = 0
    for e in range(n_fields):
        if len(spots[e]) != C:
            raise ValueError("spots[%d] must hold one entry per channel" % e)
        for c in range(C):
            if len(spots[e][c]) != F:
                raise ValueError("spots[%d][%d] must hold one (h, w) table per frame" % (e, c))
            for f in range(F):
                a = np.asarray(spots[e][c][f])
                if a.size and not np.array_equal(a, np.rint(a)):
                    raise NotImplementedError("Spot.h / Spot.w must be whole numbers (flexlibrary.py:449 makes them so)")
                a = a.astype(np.int32).reshape(-1, 2)
                parts.append(a)
                counts[i] = len(a)
                i += 1
    hw = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, 2), np.int32)
    return hw, counts


def sequence_experiment_records(frames, alignment_frames=None, self_align=True, spots=None, find_peptides_parameters=None,
                                upsample_factor=20, method='mexican_hat', keep_invalid=False, device=None, stage_times=None,
                                **photometry_kwargs):
    """A whole sequence experiment in one call.

    frames            integer [fields, channels, F, H, W], F <= 64, values below 2^31 (beyond 65 535 the uint32 entries run)
    alignment_frames  [fields, F, H, W] or None; None with self_align: channel 0 of every field aligns all its channels
                      (basic_experiment_script.py:273-278, 429-439); None without self_align: all offsets are (0, 0)
    spots             optional spots[field][channel][frame] = int [n, 2] tables of (h, w) already loaded (from the pkl files): the
                      fit and the spot-table kernel are skipped
    find_peptides_parameters  keyword arguments of pflib.find_peptides
    method, **photometry_kwargs  as Spot.photometry: 'mexican_hat' (radius, brim_size), 'simple', 'gaussian_volume' (scaling,
                      default; needs the fits, so not with spots=)
    keep_invalid      False: the summary numbers and filtered_counts leave out the traces discard_invalid_traces drops
    stage_times       a dict that receives the device time of every stage in ms (HIP events; for measurements)

    Returns a dict of NumPy arrays.  Per sequence: offsets float64 [n_seq, F, 2], n_dropouts int32 [n_seq] (discard_dropouts),
    seq_start int32 [n_seq + 1], spot_count, trace_count, singleton_count int64 [n_seq].  Per frame: spot_counts, spots_discarded
    int32 [n_seq, F].  Spot table: spot_hw int32 [k', 2], spot_record int32 [k'] (with spots=: 0 .. k'-1).  Per trace (tracking
    order, sequences ascending): trace_hw int32 [N, F, 2] (detected Spots, (-1, -1) = none), trace_spot int32 [N, F], trace_seq
    int32 [N], hw, photometry, flags, category, trace_valid as sequencing.sequence_photometry_records (interpolate=True; for
    'gaussian_volume' photometry holds the volumes, `default` where the Spot is interpolated), trace_appended int32 [N] (the
    Spots one fill_in_trace pass appends to the frames for this trace).  counts / filtered_counts: sequencing.category_counts of
    all traces / of the traces that stay (all of them with keep_invalid).  trace_count and singleton_count count the traces that
    stay, spot_count the fitted Spots (summary_counts adds what the script's passes append).

    Raises NotImplementedError for F > 64 and for the photometry methods that are not built (before anything is launched),
    AssertionError naming the frame whose fit ended in the re-key assertion, the reference's AssertionError for two Spots of a
    frame in one tracking bin."""
    plan = _fl._photometry_plan(method, photometry_kwargs)
    a = np.asarray(frames)
    if a.ndim != 5:
        raise ValueError("frames must have shape (fields, channels, F, H, W)")
    n_fields, C, F, H, W = (int(x) for x in a.shape)
    if min(n_fields, C, F, H, W) < 1:
        raise ValueError("frames must have shape (fields, channels, F, H, W) with no empty axis")
    if F > NQ.MAX_FRAMES:
        raise NotImplementedError("sequences of more than %d frames are not built (the category is one bit per frame)" % NQ.MAX_FRAMES)
    if plan['method'] == 'gaussian_volume' and spots is not None:
        raise NotImplementedError("gaussian_volume needs the fits: not with spots=")
    radius = plan['radius'] if plan['radius'] is not None else (NX.SPOT_SIZE - 1) // 2
    n_seq = n_fields * C
    _sq.check_arguments((n_seq, F, H, W), np.zeros((0, F, 2), np.int32), [], np.zeros((n_seq, F, 2)), plan['device'], radius,
                        plan['brim_size'], NX.SPOT_SIZE)
    align, align_u16 = None, False
    if alignment_frames is not None:
        align = np.asarray(alignment_frames)
        if align.shape != (n_fields, F, H, W):
            raise ValueError("alignment_frames must have shape (fields, F, H, W)")
        align_u16 = align.dtype == np.uint16
    fr, fmt = _engine.as_integer_fields(a)
    wide = fmt == N.PIXELS_U32
    torch = _engine._torch()
    dev = torch.device(device or ("cuda:%d" % torch.cuda.current_device()))
    i32 = dict(dtype=torch.int32, device=dev)
    if spots is not None:
        host_hw, host_counts = _spots_argument(spots, n_fields, C, F)

    marks = []

    def mark(name):
        if stage_times is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            marks.append((name, ev))

    with torch.cuda.device(dev):
        mark("start")
        d_fr = _engine.to_device_pixels(fr, fmt, dev)                                     # the one upload of the stack
        mark("upload")
        d_seq_frames = d_fr.reshape(n_seq, F, H, W)

        # ---- Spots ----
        d_volume = None
        if spots is None:
            runner, d_rec, d_peaks = _fit_device(torch, dev, d_fr.reshape(n_seq * F, H, W), fmt, int(fr.max()) if wide else None,
                                                 dict(find_peptides_parameters or {}))
            try:
                mark("fit")
                tab = spot_table_device(d_rec, d_peaks, H, W)
                if plan['method'] == 'gaussian_volume' and int(d_rec.shape[0]):
                    fits = d_rec[:, 24:48].contiguous().view(torch.float64)                # A, sigma_h, sigma_w of every record
                    d_volume = float(plan['scaling']) * fits[:, 0] * fits[:, 1] * fits[:, 2]   # multiplied left to right
                small = torch.cat([tab["status"], tab["counts"], tab["discarded"], tab["n_spots"]]).cpu().numpy()
            finally:
                if runner is not None:
                    runner.lock.release()
            n_frames = n_seq * F
            status, counts, discarded, total = small[:n_frames], small[n_frames:2 * n_frames], small[2 * n_frames:3 * n_frames], int(small[-1])
            bad = np.flatnonzero(status != NX.STATUS_OK)
            if len(bad):
                s, f = divmod(int(bad[0]), F)
                if status[bad[0]] == NX.STATUS_REKEY_ASSERT:
                    raise AssertionError("field %d, channel %d, frame %d: re-keyed peak collides with an existing key (pflib.py:518)"
                                         % (s // C, s % C, f))
                raise RuntimeError("fsq_experiment_spot_table: frame %d: invalid peak count" % int(bad[0]))
            d_hw, d_spot_record, d_counts = tab["hw"][:total], tab["spot_record"][:total], tab["counts"]
        else:
            counts, discarded, total = host_counts, np.zeros_like(host_counts), len(host_hw)
            d_hw, d_counts = torch.from_numpy(host_hw).to(dev), torch.from_numpy(host_counts).to(dev)
            d_spot_record = torch.arange(total, **i32)
        if total == 0:
            d_hw = torch.zeros((1, 2), **i32)[:0]
        mark("spot_table")
        per_seq = counts.reshape(n_seq, F).sum(axis=1)
        d_field_start = torch.from_numpy(np.concatenate([[0], np.cumsum(per_seq)]).astype(np.int32)).to(dev)

        # ---- offsets ----
        if align is not None:
            if align_u16:
                d_align = _engine.to_device_u16(align, dev)
            else:
                d_align = torch.from_numpy(np.ascontiguousarray(align, dtype=np.float64)).to(dev)
            d_off_field = _offsets_device(torch, dev, d_align, align_u16, n_fields, F, H, W, upsample_factor)
        elif self_align:
            chan0 = d_fr.reshape(n_fields, C, F, H, W)[:, 0]
            is_u16 = a.dtype == np.uint16                                                   # (as offsets_from_frames: anything else through float64)
            if not is_u16:
                chan0 = chan0.to(torch.float64) if wide else (chan0.to(torch.int32) & 0xffff).to(torch.float64)
            d_off_field = _offsets_device(torch, dev, chan0, is_u16, n_fields, F, H, W, upsample_factor)
        else:
            d_off_field = torch.zeros((n_fields, F, 2), dtype=torch.float64, device=dev)
        d_off = d_off_field[:, None].expand(n_fields, C, F, 2).reshape(n_seq, F, 2).contiguous()
        mark("registration")

        # ---- tracking, trace rows ----
        d_traces, d_nt, d_nd, d_seq_start, st, n_rows = _track_device(torch, dev, d_hw, d_field_start, d_counts, d_off, n_seq, F, H, W,
                                                                      total, int(counts.max()) if counts.size else 0)
        for s in range(n_seq):
            if st[s] == N.FSQ_EASSERT:
                raise AssertionError("field %d: two spots of one frame round to the same bin of frame_bins (flexlibrary.py:851)" % s)
            N.check(int(st[s]), "fsq_greedy_tracking (field %d)" % s)
        mark("tracking")
        d_trace_hw, d_trace_spot, d_trace_seq = trace_rows_device(d_traces, d_seq_start, d_field_start, d_hw, F, n_rows)
        mark("trace_rows")

        # ---- positions, photometries, categories, counts ----
        o = _sq.run_device(d_seq_frames, d_trace_hw, d_trace_seq, d_off, wide=wide, method=_sq.METHODS[plan['device']], radius=radius,
                           brim_size=plan['brim_size'], spot_size=NX.SPOT_SIZE, interpolate=True)
        d_phot = o["photometry"]
        if plan['method'] == 'gaussian_volume':
            have, fitted = (o["flags"] & 3) != 0, d_trace_spot >= 0
            vol = torch.full_like(d_phot, float(plan['default']))
            if d_volume is not None and n_rows:
                vol = torch.where(fitted, d_volume[d_spot_record[d_trace_spot.clamp(min=0).long()].long()], vol)
            d_phot = torch.where(have, vol, torch.full_like(vol, float("nan")))
        mark("photometry")
        d_select = None if keep_invalid else o["trace_valid"]
        all_counts = _sq.category_counts_device(o["category"], d_trace_seq)
        kept_counts = _sq.category_counts_device(o["category"], d_trace_seq, d_select)

        mark("counts")
        # ---- the one download ----
        dev_out = {"offsets": d_off, "n_dropouts": d_nd, "seq_start": d_seq_start, "spot_hw": d_hw, "spot_record": d_spot_record,
                   "trace_hw": d_trace_hw, "trace_spot": d_trace_spot, "trace_seq": d_trace_seq, "hw": o["hw"], "photometry": d_phot,
                   "flags": o["flags"], "category": o["category"], "trace_valid": o["trace_valid"]}
        host = _engine.to_host(dev_out)
        host["counts"] = _sq._counts_to_host(*all_counts[:5])
        host["filtered_counts"] = _sq._counts_to_host(*kept_counts[:5])
        mark("download")
        if stage_times is not None:
            torch.cuda.synchronize(dev)
            for (_, e0), (name, e1) in zip(marks[:-1], marks[1:]):
                stage_times[name] = stage_times.get(name, 0.0) + e0.elapsed_time(e1)
    host["spot_counts"] = counts.reshape(n_seq, F).astype(np.int32)
    host["spots_discarded"] = discarded.reshape(n_seq, F).astype(np.int32)
    return finish_records(host, (n_fields, C, F, H, W), keep_invalid, plan['method'])


def finish_records(host, shape, keep_invalid, photometry_method):
    """The host side of sequence_experiment_records: from the downloaded arrays (offsets, n_dropouts, seq_start, spot_counts,
    trace_hw, trace_seq, hw, photometry, flags, category, trace_valid, counts, filtered_counts) the summary numbers and the
    settings the writers read."""
    n_fields, C, F, H, W = (int(x) for x in shape)
    n_seq = n_fields * C
    host["category"] = np.ascontiguousarray(host["category"]).view(np.uint64)
    host["trace_valid"] = np.asarray(host["trace_valid"]).astype(bool)
    host["trace_appended"] = _trace_appended(host["flags"], host["trace_hw"], H, W)
    stay = np.ones(len(host["trace_seq"]), bool) if keep_invalid else host["trace_valid"]
    detected = (host["flags"] & NQ.DETECTED) != 0
    host["spot_count"] = host["spot_counts"].reshape(n_seq, F).sum(axis=1).astype(np.int64)
    host["trace_count"] = np.bincount(host["trace_seq"][stay], minlength=n_seq).astype(np.int64)
    host["singleton_count"] = np.bincount(host["trace_seq"][stay & (detected.sum(axis=1) == 1)], minlength=n_seq).astype(np.int64)
    host["keep_invalid"] = np.bool_(keep_invalid)
    host["shape"] = np.array([n_fields, C, F, H, W], np.int64)
    host["photometry_method"] = np.str_(photometry_method)
    return host


def _trace_appended(flags, trace_hw, H, W, spot_size=NX.SPOT_SIZE):
    """The number of Spots one fill_in_trace pass appends to the frames for every trace (flexlibrary.py:1842-2032): for every
    hole of the trace, interpolate_spots makes a new Spot for every position of the span that lies inside its frame - the
    filled-in frames and, on every call, the detected frames on either side of the hole."""
    r = (spot_size - 1) // 2
    detected, interpolated = (flags & NQ.DETECTED) != 0, (flags & NQ.INTERPOLATED) != 0
    hole = ~detected
    beside = np.zeros(flags.shape, np.int32)
    beside[:, 1:] += hole[:, :-1]
    beside[:, :-1] += hole[:, 1:]
    h, w = trace_hw[..., 0], trace_hw[..., 1]
    inside = detected & (r <= h) & (h < H - r) & (r <= w) & (w < W - r)
    return (interpolated.sum(axis=1) + (inside * beside).sum(axis=1)).astype(np.int32)


# ---- the records as the reference's texts ----

def channel_names(records, channels=None):
    C = int(records["shape"][1])
    names = list(channels) if channels is not None else ["ch%d" % (c + 1) for c in range(C)]      # basic_experiment_script.py:434-441
    if len(names) != C:
        raise ValueError("one name per channel")
    return names


def _staying(records):
    n = len(records["trace_seq"])
    return np.ones(n, bool) if bool(records["keep_invalid"]) else np.asarray(records["trace_valid"], bool)


def _ordered_traces(records):
    """Trace indices in the order track_photometries_as_csv writes them: channels, fields ascending, categories in order of first
    appearance among the sequence's staying traces, traces in tracking order.  -> list of (channel, field, [trace indices])."""
    n_fields, C = int(records["shape"][0]), int(records["shape"][1])
    stay, seq, cat = _staying(records), records["trace_seq"], records["category"]
    out = []
    for c in range(C):
        for e in range(n_fields):
            rows = np.flatnonzero(stay & (seq == e * C + c))
            first = {}
            for t in rows.tolist():
                first.setdefault(int(cat[t]), []).append(t)
            out.append((c, e, [t for members in first.values() for t in members]))
    return out


def write_track_photometries_csv(path, records, save_averages, channels=None, dialect='excel'):
    """The bytes of MultifieldMultichannelSequenceExperiment.track_photometries_as_csv (after discard_invalid_traces unless the
    records were made with keep_invalid) from sequence_experiment_records' output.  Returns the number of rows."""
    import csv
    names = channel_names(records, channels)
    F = int(records["shape"][2])
    flags, hw, phot = records["flags"], records["hw"], records["photometry"]
    as_int = str(records["photometry_method"]) == 'simple'
    use_bit = NQ.DETECTED if save_averages else (NQ.DETECTED | NQ.INTERPOLATED)       # (averages: interpolate=False)
    rows = 0
    with open(path, 'w') as output_file:
        writer = csv.writer(output_file, dialect=dialect)
        writer.writerow(_fl._track_photometries_header(save_averages, F))
        for c, e, members in _ordered_traces(records):
            for t in members:
                have = (flags[t] & use_bit) != 0
                f0 = int(np.flatnonzero(have)[0])
                vals = phot[t].tolist()
                values = [(int(v) if as_int else v) if ok else None for v, ok in zip(vals, have.tolist())]
                writer.writerow(_fl._track_photometries_row(names[c], e, int(hw[t, f0, 0]), int(hw[t, f0, 1]),
                                                            _sq.pattern_to_tuple(records["category"][t], F), values, save_averages))
                rows += 1
    return rows


def category_stats(records, channels=None, filtered=False, include_first_frame_only=True):
    """{channel: {field: {pattern: count}}} of the traces that stay: count_binary_trace_categories()[0], or with filtered the
    result of filtered_binary_trace_category_counts, in the reference's dict order."""
    names = channel_names(records, channels)
    n_fields, C, F = (int(x) for x in records["shape"][:3])
    k = records["filtered_counts"]
    by_seq = {}
    for s, p, n in zip(k["seq"].tolist(), k["pattern"].tolist(), k["count"].tolist()):      # (order of first appearance)
        by_seq.setdefault(s, {})[_sq.pattern_to_tuple(p, F)] = n
    out = {}
    for e in range(n_fields):                                   # (the classes merge field by field: channels appear in that order)
        for c in range(C):
            if e * C + c in by_seq:
                counts = by_seq[e * C + c]
                out.setdefault(names[c], {})[e] = _fl._filtered_counts(counts, include_first_frame_only) if filtered else counts
    return out


def write_category_counts_csv(path, records, collate_fields, channels=None, dialect='excel'):
    """The bytes of category_counts_as_csv(filtered=True) from the records.  Returns path."""
    return _fl._write_category_counts_csv(path, category_stats(records, channels, filtered=True), collate_fields, dialect)


def offsets_by_frame(records, channels=None):
    """get_offsets_by_frame: {frame: {field: {channel: (d_h, d_w)}}}."""
    names = channel_names(records, channels)
    n_fields, C, F = (int(x) for x in records["shape"][:3])
    off = records["offsets"]
    out = {}
    for e in range(n_fields):
        for c in range(C):
            for f in range(F):
                d_h, d_w = (0, 0) if f == 0 else (off[e * C + c, f, 0], off[e * C + c, f, 1])
                out.setdefault(f, {}).setdefault(e, {}).setdefault(names[c], (d_h, d_w))
    return out


def summary_counts(records, save_averages, channels=None):
    """What basic_experiment_script prints at its end, per channel: spot_count (the fitted Spots plus those its fill-in passes have
    appended to the frames: discard_invalid_traces over all traces unless keep_invalid, then track_photometries_as_csv over the
    staying traces unless save_averages), count_discarded_spots, trace_count, singleton_count."""
    names = channel_names(records, channels)
    C = int(records["shape"][1])
    n_seq = len(records["spot_count"])
    stay, seq, app = _staying(records), records["trace_seq"], records["trace_appended"].astype(np.int64)
    spots = records["spot_count"].astype(np.int64).copy()
    if not bool(records["keep_invalid"]):
        spots += np.bincount(seq, weights=app, minlength=n_seq).astype(np.int64)
    if not save_averages:
        spots += np.bincount(seq[stay], weights=app[stay], minlength=n_seq).astype(np.int64)
    out = {}
    for key, per_seq in (("spot_count", spots), ("count_discarded_spots", records["n_dropouts"]), ("trace_count", records["trace_count"]),
                         ("singleton_count", records["singleton_count"])):
        out[key] = {}
        for s in range(n_seq):                                  # (field by field, as _summed does)
            out[key][names[s % C]] = out[key].get(names[s % C], 0) + int(per_seq[s])
    return out


def summary_text(records, save_averages, collate_fields=False, channels=None):
    """The "Summary stats" block of basic_experiment_script.py:627-644, as the lines it prints."""
    s = summary_counts(records, save_averages, channels)
    return "\n".join(["", "", "Summary stats", "-------------", "Stage drift offsets:",
                      _fl._offsets_string(offsets_by_frame(records, channels)),
                      "Total spots found in all peptide frames: " + str(s["spot_count"]),
                      "Number of spots discarded due to stage drift: " + str(s["count_discarded_spots"]),
                      "Total number of traced spots: " + str(s["trace_count"]),
                      "Singleton count: " + str(s["singleton_count"]),
                      "Basic track breakdown:",
                      _fl._category_counts_string(category_stats(records, channels, filtered=True), collate_fields)]) + "\n"
