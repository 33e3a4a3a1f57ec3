"""The simulate family on the GPU at its limits and at sweep scale (include/fsq_peptide_sim.h, fsq_montecarlo.h,
fsq_signal_sweep.h): the inputs of tests/_simulate_limit_cases.py, whose corners tests/test_simulate_limits_host.py proves
without a GPU, against the NumPy twins and the single-point kernel.  Every output buffer starts as a byte pattern; nothing is
compared with a tolerance, NaNs are one pattern.

  A  more rows than one pass of the grid: fsq_peptide_simulate_points, fsq_signal_tally, fsq_mc_fit_rois, and sweep_device at
     its default chunk_rows
  B  fsq_peptide_simulate_points at 1 and at 64 frames with extreme parameters side by side in a wavefront
  C  table edges: one slot, a full table, the keys 0 and all ones, 1000 points, nothing to do
  D  fsq_signal_scores over 1 .. 1000 points with every status among neighbouring lanes
  E  the argument rules of the sweep's C ABI
  F  the Monte-Carlo fit on images that are not square, off the image, and on float ROIs without a finite maximum

Run time of this file on an MI355X: 6 s for its 40 tests, 2.2 s of them the points kernel over two passes;
test_monte_carlo_fit_over_more_rois_than_one_pass alone 0.10 s (the launch of 4 194 455 ROIs x 2 iterations 0.055 s)."""
import contextlib
import ctypes
import time

import numpy as np
import pytest

import _simulate_limit_cases as LC
from _montecarlo_cases import same_tables
from fluorosequencingimageanalysis_amd import _host_signal_sweep as H

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _prefilled():
    """Every output tensor a binding allocates starts as a byte pattern, not as zeros: what a kernel leaves unwritten shows."""
    import torch
    real = torch.empty

    def filled(*a, **k):
        t = real(*a, **k)
        if t.is_cuda:
            t.view(torch.uint8).fill_(0xA5)
        return t
    torch.empty = filled
    try:
        yield
    finally:
        torch.empty = real


def _prm(kw, seed, first):
    from fluorosequencingimageanalysis_amd import _native_peptide_sim as NP
    prm = NP.FsqPeptideSimParams()
    for k in ("label_mask", "p", "per_cycle_b", "u", "s", "s2", "log_beta", "beta_sigma", "superdye_rate", "superdye_factor", "length",
              "num_mocks", "num_edmans", "sc"):
        setattr(prm, k, kw[k])
    prm.seed, prm.first_molecule, prm.n_ddif = seed, first, min(len(kw["ddif"]), 15)
    for i, x in enumerate(kw["ddif"][:15]):
        prm.ddif[i] = x
    return prm


def _same_rows(got, exp, what):
    """(counts, intensity, category) as host arrays, bit for bit."""
    assert np.array_equal(got[0], exp[0]), what
    assert LC.same(got[1], exp[1]), what
    assert np.array_equal(np.asarray(got[2]).view(np.uint64), np.asarray(exp[2]).view(np.uint64)), what


# ---- A: more rows than one pass of the grid --------------------------------------------------------------------------------
def test_points_kernel_over_more_rows_than_two_passes():
    """16 384 blocks of 64 rows are launched at most: every block goes twice round its loop here and the first two a third time,
    and every point boundary falls inside a wavefront."""
    import torch
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS, signal_sweep as SW
    base = _prm(LC.sim_kw(LC.A1_SHAPE, LC.A1_POINTS[0]), LC.A1_SEED, LC.A1_FIRST_MOLECULE)
    with _prefilled():
        got = SW.simulate_points_device(base, torch.from_numpy(LC.A1_POINTS).cuda(), len(LC.A1_POINTS), LC.A1_PER, LC.A1_STRIDE,
                                        LC.A1_FIRST_ROW, LC.A1_ROWS)
        assert got["counts"].shape == (LC.A1_ROWS, 4)
        for k, lo, hi, first in LC.a1_point_ranges():
            one = PS.simulate_device_prm(_prm(LC.sim_kw(LC.A1_SHAPE, LC.A1_POINTS[k]), LC.A1_SEED, first), hi - lo)
            assert torch.equal(got["counts"][lo:hi], one["counts"]), k
            assert torch.equal(got["intensity"][lo:hi].view(torch.int64), one["intensity"].view(torch.int64)), k
            assert torch.equal(got["category"][lo:hi], one["category"]), k
            assert bool(one["counts"].any())
    for (lo, hi), exp in LC.a1_expected().items():
        _same_rows([got[k][lo:hi].cpu().numpy() for k in ("counts", "intensity", "category")], exp, (lo, hi))


def _decode(tables):
    """([{key: count}] of the occupied slots per point, none, unkeyed, overflow); a key sits in one slot."""
    keys, counts = tables["keys"].cpu().numpy().view(np.uint64), tables["counts"].cpu().numpy()
    assert ((keys == H.EMPTY) == (counts == 0)).all()
    got = []
    for k in range(keys.shape[0]):
        at = np.flatnonzero(keys[k] != H.EMPTY)
        assert len(set(keys[k][at].tolist())) == len(at)
        got.append(dict(zip(keys[k][at].tolist(), counts[k][at].tolist())))
    return got, tables["none"].cpu().tolist(), tables["unkeyed"].cpu().tolist(), tables["overflow"].cpu().tolist()


@pytest.mark.parametrize("few", [False, True], ids=["251_shapes", "13_shapes"])
def test_tally_over_more_rows_than_one_pass(few):
    """16 384 blocks of 256 rows: the first 70 001 rows' blocks go round twice, with other shapes (251 is prime).  251 shapes
    overfill the LDS sub-tables (the direct global path), 13 stay in them."""
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    dev = torch.device("cuda")
    base = LC.tally_few() if few else LC.tally_base()
    i = torch.arange(LC.A2_N, device=dev)
    d_rows = torch.from_numpy(base).to(dev)[i % len(base)].contiguous()
    d_point = torch.div(i, LC.A2_PER, rounding_mode="floor").to(torch.int32)
    valid = LC.tally_valid()
    d_valid = torch.from_numpy(valid).to(dev)
    exp = LC.tally_expected(base, 0, LC.A2_N, valid) + ([0] * LC.A2_POINTS,)
    whole = SW.new_tables(LC.A2_POINTS, LC.A2_SLOTS, dev)
    SW.tally_device(whole, d_rows, d_point, d_valid)
    assert _decode(whole) == exp
    halves, cut = SW.new_tables(LC.A2_POINTS, LC.A2_SLOTS, dev), 1234567
    SW.tally_device(halves, d_rows[:cut], d_point[:cut], d_valid[:cut])
    SW.tally_device(halves, d_rows[cut:], d_point[cut:], d_valid[cut:])
    assert _decode(halves) == exp


def test_monte_carlo_fit_over_more_rois_than_one_pass():
    """2^20 blocks of 4 ROIs: the first 151 ROIs' waves go round twice.  The draws are counter-based, so ROI i is ROI i mod 251
    in every byte; the first 251 are the twin's.  Measured on an MI355X: 0.055 s for the launch, 0.10 s for the test."""
    import torch
    from fluorosequencingimageanalysis_amd import _native as N
    from fluorosequencingimageanalysis_amd import _native_montecarlo as NM
    dev = torch.device("cuda:%d" % torch.cuda.current_device())
    rois, ids = LC.mc_base()
    n = LC.A3_N
    idx = torch.arange(n, device=dev) % LC.A3_BASE
    d_rois = torch.from_numpy(rois).to(dev)[idx].contiguous()
    d_ids = torch.from_numpy(ids.view(np.int32)).to(dev)[idx].contiguous()
    out = {"rows": torch.empty((n, 16), dtype=torch.int64, device=dev), "fit": torch.empty((n, 25), dtype=torch.float64, device=dev),
           "rms": torch.empty(n, dtype=torch.float64, device=dev), "status": torch.empty(n, dtype=torch.int32, device=dev)}
    for t in out.values():
        t.view(torch.uint8).fill_(0xA5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = NM.lib().fsq_mc_fit_rois(d_rois.data_ptr(), d_ids.data_ptr(), n, LC.A3_N_ITER, LC.A3_SEED, out["rows"].data_ptr(),
                                  out["fit"].data_ptr(), out["rms"].data_ptr(), out["status"].data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    print("fsq_mc_fit_rois of %d ROIs x %d iterations: %.3f s" % (n, LC.A3_N_ITER, time.perf_counter() - t0))
    assert rc == N.FSQ_OK
    for k in ("rows", "status", "rms", "fit"):
        t = out[k] if out[k].dtype != torch.float64 else out[k].view(torch.int64)
        assert torch.equal(t, t[:LC.A3_BASE][idx]), k
    got = {k: v[:LC.A3_BASE].cpu().numpy() for k, v in out.items()}
    got["rows"] = got["rows"].view(N.ROW_DTYPE).reshape(-1)
    same_tables(got, LC.mc_base_expected())


def test_sweep_at_the_default_chunk_rows():
    """8 points x 140 000 molecules are one chunk of 1.12 M rows: more than one pass of the points kernel."""
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS, signal_sweep as SW
    with _prefilled():
        sweep = SW.sweep_device(*LC.SHAPE7, LC.GRID, LC.A4_PER, seed=21, first_molecule=3, fit=False, **LC.FIXED)
    records = SW.records_of_sweep(sweep)
    assert records["points"] == LC.GRID
    for p, b, u in LC.GRID:
        sim = PS.simulate_device(*LC.SHAPE7, LC.A4_PER, 21, 3, p=p, b=b, u=u, **LC.FIXED)
        mes, _, total, _ = PS.signals_from_device(sim)
        assert records["all_simulations"][(p, b, u)] == (None, mes) and records["total_count"][(p, b, u)] == total, (p, b, u)
        assert len(mes) > 20 and total > LC.A4_PER // 2


# ---- B: the points kernel at the shape and parameter limits ----------------------------------------------------------------
@pytest.mark.parametrize("stride", [0, 5])
@pytest.mark.parametrize("shape", sorted(LC.B_SHAPES))
def test_points_at_the_shape_and_parameter_limits(shape, stride):
    import torch
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS, signal_sweep as SW
    pts, kw = LC.limit_points(), LC.B_SHAPES[shape]
    F = kw["num_mocks"] + kw["num_edmans"] + 1
    with _prefilled():
        out = SW.simulate_points_device(_prm(LC.sim_kw(kw, pts[0]), LC.B_SEED, LC.B_FIRST_MOLECULE), torch.from_numpy(pts).cuda(),
                                        LC.B_POINTS, LC.B_PER, stride)
        got = [out[k].cpu().numpy() for k in ("counts", "intensity", "category")]
        assert got[0].shape == (LC.B_POINTS * LC.B_PER, F)
        for k in range(LC.B_POINTS):
            one = PS.simulate_device_prm(_prm(LC.sim_kw(kw, pts[k]), LC.B_SEED, LC.B_FIRST_MOLECULE + k * stride), LC.B_PER)
            rows = slice(k * LC.B_PER, (k + 1) * LC.B_PER)
            _same_rows([g[rows] for g in got], [one[x].cpu().numpy() for x in ("counts", "intensity", "category")], (shape, stride, k))
    _same_rows(got, LC.limit_points_expected(shape, stride), (shape, stride))


# ---- C: table edges ------------------------------------------------------------------------------------------------------------
def _tally_into(tables, rows, points=None):
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    rows = np.ascontiguousarray(rows, np.uint8)
    points = np.zeros(len(rows), np.int32) if points is None else points
    SW.tally_device(tables, torch.from_numpy(rows).cuda(), torch.from_numpy(np.ascontiguousarray(points, np.int32)).cuda())


def _lookup(tables, keys):
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    with _prefilled():
        return SW.lookup_device(tables, torch.from_numpy(np.array(keys, np.uint64).view(np.int64)).cuda()).cpu().numpy()


def test_a_table_of_one_slot():
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    tables = SW.new_tables(1, 1, torch.device("cuda"))
    first, second = H.key_of(3, [2, 4, 4]), H.key_of(1, [1])
    _tally_into(tables, np.tile(np.array([[3, 3, 2, 2, 0]], np.uint8), (1000, 1)))
    assert _decode(tables) == ([{first: 1000}], [0], [0], [0])
    _tally_into(tables, np.tile(np.array([[1, 0, 0, 0, 0]], np.uint8), (5, 1)))
    assert _decode(tables) == ([{first: 1000}], [0], [0], [1])
    assert _lookup(tables, [first, second, H.NEVER]).tolist() == [[1000], [0], [0]]


def test_a_table_that_is_exactly_full():
    """8 keys in 8 slots: table_add's probes run to `slots` without an overflow, and the lookup of an absent key meets no
    empty slot, so that only the bound of kss_lookup's loop ends it."""
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    rows, keys, absent = LC.full_table_case()
    exp, _, _ = H.tally_rows(rows, np.zeros(len(rows), np.int32), None, 1)
    tables = SW.new_tables(1, 8, torch.device("cuda"))
    _tally_into(tables, rows)
    assert _decode(tables) == (exp, [0], [0], [0]) and not bool((tables["keys"] == H.EMPTY).any())
    assert _lookup(tables, keys + [absent, H.NEVER]).tolist() == [[exp[0][k]] for k in keys] + [[0], [0]]


def test_the_extreme_keys_in_one_table():
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    tables = SW.new_tables(1, 4, torch.device("cuda"))
    _tally_into(tables, [LC.C_ROW_ZERO] * 5 + [LC.C_ROW_ONES] * 7 + [LC.C_ROW_FLAT] * 11 + [LC.C_ROW_ONES] * 2)
    exp = {0: 5, LC.ALL_ONES: 9, H.key_of(15, []): 11}
    assert _decode(tables) == ([exp], [0], [0], [0])
    assert _lookup(tables, [LC.ALL_ONES, 0, H.NEVER, H.key_of(15, [])]).tolist() == [[9], [5], [0], [11]]


def test_a_thousand_points_of_four_slots():
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    rows, points = LC.many_points_case()
    exp, e_none, e_unkeyed = H.tally_rows(rows, points, None, 1000)
    tables = SW.new_tables(1000, 4, torch.device("cuda"))
    _tally_into(tables, rows, points)
    assert _decode(tables) == (exp, e_none, e_unkeyed, [0] * 1000)
    wanted = sorted(set().union(*exp)) + [H.NEVER]
    assert np.array_equal(_lookup(tables, wanted), np.array([[t.get(w, 0) for t in exp] for w in wanted]))


def _pattern_buffer():
    import torch
    buf = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device="cuda")
    return buf, buf.data_ptr(), torch.cuda.current_stream().cuda_stream


def test_nothing_to_do_is_ok_and_writes_nothing():
    import torch
    from fluorosequencingimageanalysis_amd import _native as N
    from fluorosequencingimageanalysis_amd import _native_signal_sweep as NS
    L = NS.lib()
    buf, p, s = _pattern_buffer()
    assert L.fsq_signal_tally(p, 5, p, p, 0, 2, 8, p, p, p, p, p, s) == N.FSQ_OK
    assert L.fsq_signal_tally(p, 5, p, None, 0, 2, 8, p, p, p, p, p, s) == N.FSQ_OK
    assert L.fsq_signal_tally(None, 5, None, None, 0, 2, 8, p, p, p, p, p, s) == N.FSQ_OK
    assert L.fsq_signal_lookup(p, p, 2, 8, p, 0, p, s) == N.FSQ_OK
    assert L.fsq_signal_lookup(p, p, 2, 8, None, 0, None, s) == N.FSQ_OK
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all())


# ---- D: the scores over many points --------------------------------------------------------------------------------------------
def _scores_equal_the_twin(S, P, n_observed):
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    table, fit, total = LC.score_case(S, P, n_observed)
    d_fit, d_total = torch.from_numpy(fit).cuda(), torch.from_numpy(total).cuda()
    for (metric, norm, cutoff), (score, factor, status, contrib) in LC.score_expected(S, P, n_observed).items():
        for contributions in (True, False):
            with _prefilled():
                out = SW._scores_on_device(table, d_fit, d_total, metric, norm, cutoff, contributions)
                got = {k: out[k].cpu().numpy() for k in ("score", "factor", "status")}
                got_contrib = out["contributions"].cpu().numpy() if contributions else None
            what = (S, P, metric, norm, cutoff, contributions)
            assert np.array_equal(got["status"], status), what
            assert LC.same(got["score"], score) and LC.same(got["factor"], factor), what
            assert out["contributions"] is None if not contributions else LC.same(got_contrib, contrib), what


@pytest.mark.parametrize("S,P", LC.SCORE_SHAPES, ids=["%dx%d" % sp for sp in LC.SCORE_SHAPES])
def test_scores_over_many_points(S, P):
    """All ten metrics x normalisation 0 .. 3 x cutoff none and 3, with and without contributions: points of every status in
    neighbouring lanes, P at and round the block size and in sixteen blocks."""
    _scores_equal_the_twin(S, P, LC.N_OBS_SMALL)


def test_scores_at_the_largest_count():
    """observed = fit = n_observed = 2^31 - 1, and an observed count of 2^30: oi * (n_observed - oi) needs 61 bits."""
    _scores_equal_the_twin(60, 130, LC.BIG)


# ---- E: the argument rules of the sweep's C ABI --------------------------------------------------------------------------------
def test_argument_rules_of_the_sweep_c_abi():
    import torch
    from fluorosequencingimageanalysis_amd import _native as N
    from fluorosequencingimageanalysis_amd import _native_signal_sweep as NS
    L = NS.lib()
    buf, p, s = _pattern_buffer()
    EINVAL = N.FSQ_EINVAL
    # tally: (rows, frames, point, valid, n_rows, n_points, slots, keys, counts, none, unkeyed, overflow)
    for frames in (0, 65):
        assert L.fsq_signal_tally(p, frames, p, None, 4, 1, 8, p, p, p, p, p, s) == EINVAL, frames
    for slots in (0, 3, 2 ** 25):
        assert L.fsq_signal_tally(p, 5, p, None, 4, 1, slots, p, p, p, p, p, s) == EINVAL, slots
        assert L.fsq_signal_lookup(p, p, 1, slots, p, 2, p, s) == EINVAL, slots
    assert L.fsq_signal_tally(p, 5, p, None, 4, 0, 8, p, p, p, p, p, s) == EINVAL
    assert L.fsq_signal_tally(p, 5, p, None, -1, 1, 8, p, p, p, p, p, s) == EINVAL
    assert L.fsq_signal_tally(p, 5, p, None, 4, 1, 8, None, p, p, p, p, s) == EINVAL
    assert L.fsq_signal_tally(p, 5, p, None, 4, 1, 8, p, None, p, p, p, s) == EINVAL
    # lookup: (keys, counts, n_points, slots, wanted, n_wanted, out)
    assert L.fsq_signal_lookup(p, p, 0, 8, p, 2, p, s) == EINVAL
    assert L.fsq_signal_lookup(None, p, 1, 8, p, 2, p, s) == EINVAL
    assert L.fsq_signal_lookup(p, None, 1, 8, p, 2, p, s) == EINVAL
    assert L.fsq_signal_lookup(p, p, 1, 8, p, -1, p, s) == EINVAL

    # scores: (observed, in_observed, admitted, heatmap, fit, fit_total, n_keys, n_points, prm, score, factor, status, contrib)
    def score_prm(**change):
        prm = NS.FsqScoreParams()
        prm.n_observed, prm.small_count_cutoff, prm.has_cutoff, prm.normalization, prm.metric = 100, 3.0, 0, 0, 0
        for k, v in change.items():
            setattr(prm, k, v)
        return ctypes.byref(prm)

    def scores(prm, n_points=3):
        return L.fsq_signal_scores(p, p, p, p, p, p, 2, n_points, prm, p, p, p, p, s)
    for change in (dict(metric=-1), dict(metric=10), dict(normalization=4), dict(n_observed=-1),
                   dict(has_cutoff=1, small_count_cutoff=float("nan")), dict(n_observed=2 ** 31), dict(n_observed=2 ** 62)):
        assert scores(score_prm(**change)) == EINVAL, change
    assert scores(score_prm(), n_points=0) == EINVAL and scores(None) == EINVAL

    # simulate_points: (base, points, n_points, n_per_point, molecule_stride, first_row, n_rows, counts, intensity, category)
    def base(first_molecule=0):
        return ctypes.byref(_prm(LC.sim_kw(LC.A1_SHAPE, LC.A1_POINTS[0]), 9, first_molecule))
    d_points = torch.from_numpy(LC.A1_POINTS[:3].copy()).cuda()
    q = d_points.data_ptr()
    assert L.fsq_peptide_simulate_points(base(), q, 3, 130, 0, 380, 20, p, p, p, s) == EINVAL
    assert L.fsq_peptide_simulate_points(base(), q, 3, 130, 0, -1, 5, p, p, p, s) == EINVAL
    assert L.fsq_peptide_simulate_points(base(), q, 3, 130, -1, 0, 5, p, p, p, s) == EINVAL
    assert L.fsq_peptide_simulate_points(base(2 ** 63 - 100), q, 3, 130, 0, 0, 5, p, p, p, s) == EINVAL
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all())                        # nothing was launched on the refused calls


# ---- F: the Monte-Carlo fit on oblong images, off the image, on float ROIs -----------------------------------------------------
def test_candidates_on_an_oblong_stack_and_off_it():
    """2 fields of 23 x 41 from field 2^32 - 2: pixel = h * W + w, the corners, and candidates without a 5x5 neighbourhood
    inside the stack (an all-NaN ROI: status 2 under their own h, w and field)."""
    from fluorosequencingimageanalysis_amd import montecarlo
    img, inside, outside = LC.candidates_case()
    with _prefilled():
        got = montecarlo.fit_candidates(img, np.concatenate([inside, outside]), LC.F1_N_ITER, LC.F1_SEED, LC.F1_FIRST_FIELD)
    same_tables(got, LC.candidates_case_expected())
    img5, cand5 = LC.tiny_case()
    with _prefilled():
        got = montecarlo.fit_candidates(img5, cand5, LC.F1_N_ITER, LC.F1_SEED, 0)
    same_tables(got, LC.candidates_expected(img5, cand5, LC.F1_N_ITER, LC.F1_SEED, 0))


@pytest.mark.parametrize("name", ["96x64", "64x96"])
def test_records_of_an_oblong_field(name):
    """find_peptides_records on the cropped golden field, upside down as field 0 and as it is as field 1: every record is the
    twin's fit of its own (h, w) - the row, the last iteration's image - and holds the image's own 25 pixels."""
    from fluorosequencingimageanalysis_amd import engine, pflib
    from _montecarlo_cases import FLOAT_FIELDS
    img, kw = LC.crop_fields()[name], LC.crop_kwargs()
    stack = np.stack([img[::-1], img])
    with _prefilled():
        rec, counts, fmt = pflib.find_peptides_records(stack, **kw)
    print("records per field of %s: %s" % (name, counts.tolist()))
    assert (counts >= 10).all() and len(rec) == counts.sum()
    rows, fit, sub = engine.split_peak_records(rec, fmt)
    assert rows["field"].tolist() == [0] * counts[0] + [1] * counts[1]
    for r in range(len(rows)):
        f, h, w = int(rows["field"][r]), int(rows["h"][r]), int(rows["w"][r])
        exp = LC.record_expected(stack[f], h, w, f, kw)
        for k in FLOAT_FIELDS:
            assert LC.same(rows[k][r], exp["row"][k]), (r, k)
        for k in ("status", "niter", "nfev"):
            assert rows[k][r] == exp["row"][k], (r, k)
        assert rows["key_h"][r] >= 0 and rows["key_w"][r] >= 0          # (the re-key is the consolidation's, not the fit's)
        assert LC.same(fit[r].reshape(25), exp["fit"]), r
        assert np.array_equal(sub[r], stack[f][h - 2:h + 3, w - 2:w + 3]), r


@pytest.mark.parametrize("n_iter", LC.F3_N_ITERS)
def test_float_rois_without_a_finite_maximum(n_iter):
    """+inf, -inf, a negative maximum, zeros, -0.0, a denormal maximum and a NaN, at 1 .. 7 ROIs (3, 2, 1 idle waves a block)."""
    from fluorosequencingimageanalysis_amd import montecarlo
    for n in LC.F3_NS:
        rois, ids = LC.float_case(n_iter, n)
        with _prefilled():
            got = montecarlo.fit_rois(rois, ids, n_iter, LC.F3_SEED)
        same_tables(got, LC.float_expected(n_iter, n), (n_iter, n))
