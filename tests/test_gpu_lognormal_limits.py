"""The lognormal family at its limits on the GPU: the enumerating fit and the dynamic programme (include/fsq_lognormal.h,
fsq_lognormal_dp.h), the logarithm, the remainder correction (fsq_remainder.h) and the chain's steps (fsq_lognormal_chain.h),
through the device-tensor routes that check no value.  Inputs and expected values: tests/_lognormal_limit_cases.py
(tests/test_lognormal_limits_host.py proves that they reach the paths named here); the expected values are the Python twins'
and the numpy restatement's.  Every output tensor and the workspace start as a byte pattern.  Every comparison is bit for
bit, NaN equal to NaN.

  A  2 x 16 384 + 77 tracks, a base of 257 tiled: three trips of the block stride of kln_fit and kln_fit_dp over LDS tables
     left by another track, rows of an invalid length among them; enumerate, dp, dp with upsteps, enumerate under a small
     budget (OVER_BUDGET rows between the trips); 4 096 x 256 + 3 values through kln_log
  B  the 495-survivor track at budget 495 and 494; tracks of exactly 1, 2, 63, 64, 65, 127, 128 and 129 survivors (lanes with
     no share, one survivor each, the remainder split), with and without multi-drop, against the twin and the other solver
  C  0, -0.0, -5, NaN, +inf, -inf, 5e-324 and 1.7e308 at ON and at OFF frames, max_deviation 3, 1e9 and +inf
  D  remainder tracks with NaN, +inf and (-inf, +inf) in segments of 9 and 600 remainders (a NaN among a track's intensities
     is a NaN median: in RATIO mode these fail without the ballot in krm_tracks); malformed offsets; 66 000 segments
  E  the values of C through last_drops_device, a NaN entry in one key of on_off_medians_device

Measured durations on the MI355X (--durations): the enumerating fit over the tiled base 1.9 s (its first launch in the
process), the survivor targets 0.3 s, the chain steps over 66 000 segments 0.3 s, every other test 0.1 s or less; the whole
file 3.6 s.  The slowest test of the existing limits files in the same kind of run is the pow sweep of
test_gpu_chisq_limits.py at 2.9 s.  On the library built from the commit before the ballot, the four RATIO cases of
test_remainder_tracks_with_nan_and_infinities fail and the four ADDITIVE cases pass; with it all eight pass.
"""
import contextlib

import numpy as np
import pytest

import _lognormal_limit_cases as LC
import _remainder_reference as RR
from _lognormal_chain_cases import same_bits
from _remainder_cases import same_arrays

pytestmark = pytest.mark.gpu

PATTERN64 = np.frombuffer(b"\xa5" * 8, dtype=np.uint64)[0]
PATTERN32 = np.frombuffer(b"\xa5" * 4, dtype=np.int32)[0]


@contextlib.contextmanager
def _prefilled():
    """Every tensor the bindings allocate (outputs, and the workspace of engine.workspace) starts as a byte pattern, not as
    zeros: what a kernel leaves unwritten, or reads before it writes, shows."""
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


def _cuda(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def _fit(rows, words, lens, dev, solver, ups, budget=1 << 22, multi=True):
    from fluorosequencingimageanalysis_amd import lognormal as LN
    with _prefilled():
        out = LN.lognormal_device(_cuda(rows), _cuda(np.asarray(words, np.uint64)), _cuda(np.asarray(lens, np.int32)), LC.MEANS, LC.SIGMA,
                                  LC.M, multi, dev, budget, solver=solver, allow_upsteps=ups)
        return {k: v.cpu().numpy() for k, v in out.items()}


def _fit_lists(I, C, dev, solver, ups, budget=1 << 22, multi=True, F=None):
    return _fit(LC.rows_of(I, F), LC.words_of(C), [len(v) for v in I], dev, solver, ups, budget, multi)


def _same_fit(h, e, what, count=True):
    for k in LC.FIT_KEYS:
        if k != "n_surviving" or count:
            same_bits(h[k], e[k], (what, k))


# ---- A ---------------------------------------------------------------------------------------------------------------------
STRIDE_RUNS = [("enumerate", False, 1 << 22), ("dp", False, 1 << 22), ("dp", True, 1 << 22), ("enumerate", False, LC.SMALL_BUDGET)]


@pytest.mark.parametrize("solver,ups,budget", STRIDE_RUNS, ids=["enumerate", "dp", "dp_upsteps", "enumerate_small_budget"])
def test_block_stride_over_a_tiled_base(solver, ups, budget):
    rows, words, lens, _, _, _ = LC.stride_base()
    idx = LC.stride_index()
    h = _fit(rows[idx], words[idx], lens[idx], 3, solver, ups, budget)
    e = LC.stride_expected(solver, ups, budget)
    _same_fit(h, {k: v[idx] for k, v in e.items()}, (solver, ups, budget))


def test_log_beyond_its_grid():
    from fluorosequencingimageanalysis_amd import lognormal as LN
    x, e = LC.log_stride()
    with _prefilled():
        got = LN.log_device(_cuda(x)).cpu().numpy()
    same_bits(got, e, "log")


# ---- B ---------------------------------------------------------------------------------------------------------------------
def test_budget_boundary_of_the_495_survivor_track():
    I, C, dev, n = LC.BUDGET_TRACK
    at = _fit_lists([I], [C], dev, "enumerate", False, budget=n)
    _same_fit(at, LC.twin_fit([I], [C], LC.MEANS, LC.SIGMA, LC.M, True, dev, "enumerate", False, budget=n), "at the budget")
    assert at["status"][0] == LC.FOUND and at["n_surviving"][0] == n
    below = _fit_lists([I], [C], dev, "enumerate", False, budget=n - 1)
    assert below["status"][0] == LC.OVER_BUDGET and below["n_surviving"][0] == n and below["best_score"][0] == -1.0
    assert not below["best_seq"].any() and not below["frame_score"].any()


def test_survivor_counts_around_the_lanes_shares():
    found = LC.survivor_tracks()
    for n in LC.SURVIVOR_TARGETS:
        I, C, dev = found[n]
        for multi in (True, False):
            e = LC.twin_fit([I], [C], LC.MEANS, LC.SIGMA, LC.M, multi, dev, "enumerate", False)
            k = _fit_lists([I], [C], dev, "enumerate", False, multi=multi)
            d = _fit_lists([I], [C], dev, "dp", False, multi=multi)
            _same_fit(k, e, (n, multi, "enumerate"))
            _same_fit(d, LC.twin_fit([I], [C], LC.MEANS, LC.SIGMA, LC.M, multi, dev, "dp", False), (n, multi, "dp"))
            _same_fit(k, d, (n, multi, "solvers"))
            assert not multi or k["n_surviving"][0] == n


# ---- C ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", LC.DEVIATIONS, ids=["3", "1e9", "inf"])
def test_values_the_record_routes_refuse(dev):
    I, C, _ = LC.value_tracks()
    for solver, ups in LC.LAUNCHES:
        _same_fit(_fit_lists(I, C, dev, solver, ups, F=6), LC.value_expected(dev, solver, ups), (dev, solver, ups))


# ---- D ---------------------------------------------------------------------------------------------------------------------
def _remainder(rows, cats, seg_off, mode, minimum):
    from fluorosequencingimageanalysis_amd import remainder as RM
    with _prefilled():
        out = RM.remainder_adjust_device(_cuda(np.asarray(rows, np.float64)), _cuda(np.asarray(cats, np.uint64)),
                                         _cuda(np.asarray(seg_off, np.int64)), mode, minimum)
        return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("mode", [RR.RATIO, RR.ADDITIVE])
@pytest.mark.parametrize("F", LC.NAN_FRAMES)
def test_remainder_tracks_with_nan_and_infinities(F, mode):
    """D1.  In RATIO mode the medians of a segment with a NaN track are NaN at every frame, not at the NaN's frame alone."""
    rows, cats, seg_off, meta = LC.nan_table(F)
    got = _remainder(rows, cats, seg_off, mode, 5)
    same_arrays(got, LC.nan_expected(F, mode), (F, mode))
    if mode == RR.RATIO:
        for s, name, frames in meta:
            if name is not None and any(v != v for v in frames.values()):
                assert np.isnan(got["adjustment"][s]).all(), (F, s, name)


def test_remainder_malformed_seg_off_stays_in_bounds():
    """D2.  Offsets that the host cannot vouch for leave every output written and nothing out of bounds (checked by the
    outputs: a well-formed segment of an ascending list comes out as its table alone, a track that no well-formed segment
    holds as zeros)."""
    rows, cats, _ = LC.malformed_table()
    n, F = rows.shape
    for off in LC.MALFORMED_OFFSETS:
        seg_off = np.array(off, dtype=np.int64)
        held = np.zeros(n, bool)
        for s in range(3):
            if LC.well_formed(off, s, n):
                held[off[s]:off[s + 1]] = True
        for mode in (RR.RATIO, RR.ADDITIVE):
            for minimum in (0, 5):
                got = _remainder(rows, cats, seg_off, mode, minimum)
                what = (off, mode, minimum)
                for k in ("adjustment", "adjusted"):
                    assert not (got[k].view(np.uint64) == PATTERN64).any(), (what, k)
                assert not (got["n_remainders"] == PATTERN32).any() and (got["n_remainders"] >= 0).all(), what
                assert np.isin(got["kept"], (0, 1)).all(), what
                assert not got["adjusted"][~held].any() and not np.signbit(got["adjusted"][~held]).any(), what
                for s in range(3):
                    a, b = off[s], off[s + 1]
                    assert got["n_remainders"][s] <= max(b - a, 0), what
                    if LC.well_formed(off, s, n) and (np.diff(seg_off) >= 0).all():
                        with np.errstate(all="ignore"):
                            alone = RR.adjust_arrays(rows[a:b], cats[a:b], [0, b - a], mode, minimum)
                        same_arrays({"adjustment": got["adjustment"][s:s + 1], "adjusted": got["adjusted"][a:b],
                                     "n_remainders": got["n_remainders"][s:s + 1], "kept": got["kept"][s:s + 1]}, alone, (what, s))


@pytest.mark.parametrize("mode,minimum", [(RR.RATIO, 0), (RR.RATIO, 2), (RR.ADDITIVE, 0), (RR.ADDITIVE, 2)])
def test_remainder_over_66000_segments(mode, minimum):
    """D3.  krm_finish beyond one block, S * F median blocks, a 17-step search of the offsets."""
    rows, cats, seg_off, _ = LC.many_segments(2)
    same_arrays(_remainder(rows, cats, seg_off, mode, minimum), LC.many_remainder_expected(mode, minimum), (mode, minimum))


def _steps(rows, cats, seg_off, status, alpha, what):
    """fsq_chain_on_off_medians and fsq_chain_on_off_adjust against the twin's steps."""
    from fluorosequencingimageanalysis_amd import _host_lognormal_chain as HC, lognormal as LN
    F = rows.shape[1]
    with _prefilled():
        d_rows, d_off = _cuda(rows), _cuda(seg_off)
        med = LN.on_off_medians_device(d_rows, _cuda(cats), d_off, _cuda(status), alpha)
        adjusted = LN.on_off_adjust_device(d_rows, d_off, alpha, med).cpu().numpy()
        med = {k: v.cpu().numpy() for k, v in med.items()}
    m, counts, M = HC.on_off_medians(rows, HC.category_bits(cats, F), seg_off, status == 0, alpha)
    same_bits(med["on_off_count"], counts, what)
    same_bits(med["on_off_median"], m, what)
    same_bits(med["last_beta_median"], [M], what)
    same_bits(adjusted, HC.on_off_adjust(rows, seg_off, alpha, m, counts, M), what)
    return m, counts, M


def test_chain_steps_over_66000_segments():
    rows, cats, seg_off, status = LC.many_segments(3)
    _steps(rows, cats, seg_off, status, 3.5, "66000 segments")


# ---- E ---------------------------------------------------------------------------------------------------------------------
def test_chain_steps_with_refused_values():
    from fluorosequencingimageanalysis_amd import _host_lognormal_chain as HC, lognormal as LN
    rows, cats = LC.value_table()
    with _prefilled():
        values, count = LN.last_drops_device(_cuda(rows), _cuda(cats))
        values, count = values.cpu().numpy(), count.cpu().numpy()
    bits = HC.category_bits(cats, 4)
    same_bits(values, HC.last_drops(rows, bits), "last drops")
    assert np.array_equal(count, (HC.on_then_off(bits) & (rows[:, :-1] > 0)).sum(axis=1))
    assert np.isinf(values).sum() >= 2 and not np.isnan(values).any()
    rows, cats, seg_off, status, (s, f) = LC.nan_key_table()
    m, counts, M = _steps(rows, cats, seg_off, status, 3.5, "a NaN entry")
    assert np.isnan(m[s, f]) and np.isnan(M)
