"""The simulation parameter sweep on the GPU (include/fsq_signal_sweep.h): the batched simulation bit for bit against the
single-point kernel, the tally against the host twin and np.unique, the sweep against simulate_and_fit_records point by point,
the scores bit for bit against the NumPy twin and within the reordering bound of the reference's recorded runs."""
import contextlib

import numpy as np
import pytest

from fluorosequencingimageanalysis_amd import _host_signal_sweep as H
from _signal_sweep_cases import case, case_names, check_against_golden, outcome, runs

pytestmark = pytest.mark.gpu

DDIF = [0, 0.3] + [0.3] * 5
FIXED = dict(s=0.1, sc=3, s2=0.05, beta=70000.0, beta_sigma=0.2, ddif=DDIF)
SHAPE = ('GAKAGAKC', 'K', 2, 4)                  # 2 mocks + 4 Edmans: 7 frames
POINTS3 = [(0.9, 0.05, 0.1), (0.7, 0.2, 0.4), (0.95, 0.1, 0.25)]
GRID = [(p, b, u) for p in (0.8, 0.95) for b in (0.05, 0.15) for u in (0.1, 0.4)]


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


# ---- the batched simulation ----

def _points_run(points, n, stride, first_molecule=17, seed=9, first_row=0, n_rows=None):
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    base, values, _ = SW._point_params(*SHAPE, seed, first_molecule, points, FIXED)
    with _prefilled():
        out = SW.simulate_points_device(base, torch.from_numpy(values).cuda(), len(points), n, stride, first_row, n_rows)
        return {k: v.cpu().numpy() for k, v in out.items()}


def _single(point, n, first_molecule, seed=9):
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS
    p, b, u = point
    out = PS.simulate_device(*SHAPE, n, seed, first_molecule, p=p, b=b, u=u, **FIXED)
    return {k: out[k].cpu().numpy() for k in ("counts", "intensity", "category")}


@pytest.mark.parametrize("points, n, stride", [(POINTS3, 130, 0), (POINTS3, 130, 1000), (POINTS3, 1, 0), (POINTS3, 1, 5), (POINTS3[1:2], 130, 0)],
                         ids=["3x130", "3x130_stride", "3x1", "3x1_stride", "1x130"])
def test_points_are_the_single_point_kernel_bit_for_bit(points, n, stride):
    got = _points_run(points, n, stride)
    assert got["counts"].shape == (len(points) * n, 7) and got["counts"].dtype == np.uint8
    for k, point in enumerate(points):
        exp = _single(point, n, 17 + k * stride)
        rows = slice(k * n, (k + 1) * n)
        assert np.array_equal(got["counts"][rows], exp["counts"]), k
        assert np.array_equal(got["intensity"][rows].view(np.uint64), exp["intensity"].view(np.uint64)), k
        assert np.array_equal(got["category"][rows], exp["category"]), k
    if n > 1:
        assert got["counts"].max() > 0 and len({got["counts"][k * n:(k + 1) * n].tobytes() for k in range(len(points))}) == len(points)


def test_a_chunk_is_a_slice_of_the_whole():
    whole = _points_run(POINTS3, 130, 1000)
    part = _points_run(POINTS3, 130, 1000, first_row=100, n_rows=150)                    # rows 100 .. 249: parts of points 0 and 1
    for k in ("counts", "intensity", "category"):
        assert np.array_equal(part[k], whole[k][100:250]), k


def test_invalid_sweep_shapes_are_refused():
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    base, values, _ = SW._point_params(*SHAPE, 9, 0, POINTS3, FIXED)
    d_points = torch.from_numpy(values).cuda()
    for bad in (dict(first_row=380, n_rows=20), dict(first_row=-1, n_rows=5), dict(molecule_stride=-1)):
        with pytest.raises(ValueError):
            SW.simulate_points_device(base, d_points, 3, 130, **bad)
    base.first_molecule = 2 ** 63 - 100
    with pytest.raises(ValueError):
        SW.simulate_points_device(base, d_points, 3, 130)


# ---- the tally ----

def _tally(rows, points, valid, n_points, slots):
    """fsq_signal_tally of host arrays: ([{key: count}] of the occupied slots, none, unkeyed, overflow)."""
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    tables = SW.new_tables(n_points, slots, torch.device("cuda"))
    SW.tally_device(tables, torch.from_numpy(np.ascontiguousarray(rows, np.uint8)).cuda(),
                    torch.from_numpy(np.ascontiguousarray(points, np.int32)).cuda(),
                    None if valid is None else torch.from_numpy(np.ascontiguousarray(valid, np.uint8)).cuda())
    keys, counts = tables["keys"].cpu().numpy().view(np.uint64), tables["counts"].cpu().numpy()
    assert ((keys == H.EMPTY) == (counts == 0)).all()
    got = []
    for k in range(n_points):
        at = np.flatnonzero(keys[k] != H.EMPTY)
        assert len(set(keys[k][at].tolist())) == len(at)                                 # a key sits in one slot
        got.append(dict(zip(keys[k][at].tolist(), counts[k][at].tolist())))
    return got, tables["none"].cpu().tolist(), tables["unkeyed"].cpu().tolist(), tables["overflow"].cpu().tolist()


def _distinct_rows(n, frames, rng, start=5):
    rows = set()
    while len(rows) < n:
        rows.add(tuple(sorted(rng.integers(0, start + 1, frames).tolist(), reverse=True)))
    return np.array(sorted(rows), np.uint8)


def test_tally_full_contention():
    rows = np.tile(np.array([[3, 3, 2, 2, 0]], np.uint8), (65536, 1))
    got, none, unkeyed, overflow = _tally(rows, np.zeros(65536, np.int32), None, 1, 16)
    assert got == [{H.key_of(3, [2, 4, 4]): 65536}] and (none, unkeyed, overflow) == ([0], [0], [0])


def test_tally_300_keys_in_512_slots_over_three_points():
    rng = np.random.default_rng(1)
    shapes = _distinct_rows(300, 8, rng)
    rows = shapes[rng.integers(0, 300, 5000)]
    rows[:300] = shapes                                                                  # every key stands at least once
    points = np.sort(rng.integers(0, 3, 5000)).astype(np.int32)                          # point boundaries inside blocks
    points[:300] = 1
    exp, e_none, e_unkeyed = H.tally_rows(rows, points, None, 3)
    assert len(exp[1]) == 300
    uniq, n = np.unique(rows[points == 1], axis=0, return_counts=True)
    assert sorted(exp[1].values()) == sorted(n.tolist())
    got, none, unkeyed, overflow = _tally(rows, points, None, 3, 512)
    assert got == exp and (none, unkeyed, overflow) == (e_none, e_unkeyed, [0, 0, 0])


def test_tally_does_not_depend_on_the_rows_order_or_the_points_order():
    rng = np.random.default_rng(2)
    shapes = _distinct_rows(40, 6, rng)
    rows, points = shapes[rng.integers(0, 40, 3000)], rng.integers(0, 9, 3000).astype(np.int32)     # unsorted: beyond 4 points a block
    exp, _, _ = H.tally_rows(rows, points, None, 9)
    assert _tally(rows, points, None, 9, 64)[0] == exp


def test_tally_overflow_is_flagged_and_costs_only_counts():
    rng = np.random.default_rng(3)
    shapes = _distinct_rows(20, 6, rng)
    rows = shapes[rng.integers(0, 20, 4000)]
    rows[:20] = shapes
    points = (np.arange(4000) % 2).astype(np.int32)
    points[:20] = 0
    rows[1::2][10:] = shapes[0]                                                          # point 1 keeps to a few keys
    exp, _, _ = H.tally_rows(rows, points, None, 2)
    assert len(exp[0]) == 20 and len(exp[1]) <= 8
    got, none, unkeyed, overflow = _tally(rows, points, None, 2, 8)
    assert overflow == [1, 0] and got[1] == exp[1]
    assert len(got[0]) == 8 and all(exp[0][k] == n for k, n in got[0].items())           # what found a slot is counted in full


def test_tally_rows_without_key_or_signal_and_the_mask():
    rng = np.random.default_rng(4)
    rows = _distinct_rows(30, 5, rng)[rng.integers(0, 30, 1000)]
    rows[::7] = [11, 6, 0, 0, 0]                                                         # 11 drops
    rows[3::7] = [2, 1, 2, 1, 0]                                                         # an upstep
    rows[5::50] = [16, 16, 0, 0, 0]                                                      # starts above 15
    points = (np.arange(1000) * 3 // 1000).astype(np.int32)
    points[10], points[20] = -1, 3                                                       # not a point: left out
    valid = (rng.random(1000) < 0.7).astype(np.uint8)
    exp = H.tally_rows(rows, points, valid, 3)
    assert min(exp[1]) > 0 and min(exp[2]) > 0
    got, none, unkeyed, overflow = _tally(rows, points, valid, 3, 64)
    assert (got, none, unkeyed) == exp and overflow == [0, 0, 0]
    assert _tally(rows, points, np.zeros(1000, np.uint8), 3, 64)[:3] == ([{}, {}, {}], [0, 0, 0], [0, 0, 0])


@pytest.mark.parametrize("frames", [1, 64])
def test_tally_at_the_frame_limits(frames):
    rng = np.random.default_rng(frames)
    if frames == 1:
        rows = rng.integers(0, 18, (700, 1)).astype(np.uint8)                            # 16 and 17 have no key
    else:
        rows = _distinct_rows(50, 64, rng, start=10)[rng.integers(0, 50, 700)]
        rows[0], rows[1] = [15] * 63 + [5], [15] + [4] * 63                              # 10 drops at cycle 63; 11 drops
    points = (np.arange(700) // 350).astype(np.int32)
    exp = H.tally_rows(rows, points, None, 2)
    got, none, unkeyed, overflow = _tally(rows, points, None, 2, 128)
    assert (got, none, unkeyed) == exp and overflow == [0, 0] and sum(unkeyed) > 0


def test_lookup_gives_the_dense_matrix():
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    rng = np.random.default_rng(6)
    shapes = _distinct_rows(60, 6, rng)
    rows, points = shapes[rng.integers(0, 60, 2000)], rng.integers(0, 5, 2000).astype(np.int32)
    tables = SW.new_tables(5, 64, torch.device("cuda"))
    SW.tally_device(tables, torch.from_numpy(rows).cuda(), torch.from_numpy(points).cuda())
    exp, _, _ = H.tally_rows(rows, points, None, 5)
    wanted = sorted(set().union(*exp)) + [H.NEVER, H.key_of(15, [63] * 10)]
    with _prefilled():
        got = SW.lookup_device(tables, torch.from_numpy(np.array(wanted, np.uint64).view(np.int64)).cuda()).cpu().numpy()
    assert np.array_equal(got, np.array([[exp[k].get(w, 0) for k in range(5)] for w in wanted]))


# ---- the sweep ----

_sweeps = {}


def _grid_sweep(**kw):
    """sweep_device over the 2 x 2 x 2 grid x 500 molecules, once per keyword set."""
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    key = tuple(sorted(kw.items()))
    if key not in _sweeps:
        sweep = SW.sweep_device(*SHAPE, GRID, 500, seed=21, first_molecule=3, quench_factors=DDIF, **kw, **FIXED)
        _sweeps[key] = (sweep, SW.records_of_sweep(sweep))
    return _sweeps[key]


def _single_points():
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS
    if "single" not in _sweeps:
        _sweeps["single"] = [PS.simulate_and_fit_records(*SHAPE, 500, 21, 3, quench_factors=DDIF, p=p, b=b, u=u, **FIXED) for p, b, u in GRID]
    return _sweeps["single"]


def test_sweep_is_simulate_and_fit_records_point_by_point():
    _, records = _grid_sweep()
    assert records["points"] == GRID == list(records["all_simulations"])
    for point, exp in zip(GRID, _single_points()):
        signals, molecular = records["all_simulations"][point]
        assert signals == exp["signals"] and molecular == exp["molecular_error_signals"], point
        assert (records["total_count"][point], records["none_count"][point]) == (exp["total_count"], exp["none_count"]), point
        assert exp["total_count"] > 300 and len(signals) > 10


def test_sweep_does_not_depend_on_chunk_rows():
    assert _grid_sweep(chunk_rows=100)[1] == _grid_sweep()[1]


def test_sweep_with_a_stride_and_without_the_fit():
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS, signal_sweep as SW
    records = SW.sweep_records(*SHAPE, POINTS3, 130, seed=4, first_molecule=8, molecule_stride=1000, fit=False, **FIXED)
    for k, (p, b, u) in enumerate(POINTS3):
        sim = PS.simulate_device(*SHAPE, 130, 4, 8 + 1000 * k, p=p, b=b, u=u, **FIXED)
        mes, _, total, _ = PS.signals_from_device(sim)
        assert records["all_simulations"][(p, b, u)] == (None, mes) and records["total_count"][(p, b, u)] == total


def test_a_table_too_small_raises_naming_table_slots():
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    with pytest.raises(ValueError, match="table_slots=4"):
        SW.sweep_device(*SHAPE, POINTS3, 300, seed=4, table_slots=4, quench_factors=DDIF, **FIXED)
    with pytest.raises(ValueError, match="table_slots=48"):
        SW.sweep_device(*SHAPE, POINTS3, 300, seed=4, table_slots=48, quench_factors=DDIF, **FIXED)


# ---- the scores ----

def _same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint64),
                                                                                              b[~np.isnan(b)].view(np.uint64))


@pytest.mark.parametrize("name", case_names())
def test_scores_against_the_twin_and_the_reference(name):
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    observed, fit, opts = case(name)
    for metric, nc, hn, status, result, factor, contrib in runs(name):
        kw = dict(metric=metric, normalize_counts=nc, heatmap_normalize_counts=hn, **opts)
        got = outcome(lambda: SW.signal_correlation(observed, fit, **kw))
        twin = outcome(lambda: SW.signal_correlation(observed, fit, host=True, **kw))
        assert got[0] == twin[0] and list(got[3]) == list(twin[3]), (name, metric, nc, hn)
        if got[0] in (H.SCORE_OK, H.SCORE_EMPTY):
            assert _same_bits(got[2], twin[2]), (name, metric, nc, hn)
        if got[0] == H.SCORE_OK:
            assert _same_bits(got[1], twin[1]) and _same_bits(list(got[3].values()), list(twin[3].values())), (name, metric, nc, hn, got[1], twin[1])
        check_against_golden((name, metric, nc, hn), metric, got, (status, result, factor, contrib))


@pytest.mark.parametrize("molecular", [False, True])
def test_scores_of_a_sweep_are_the_twins_bit_for_bit(molecular):
    """Eight points at once, from the tables on the device (lookup) and from the dicts (upload): both are the twin's arrays."""
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    sweep, records = _grid_sweep()
    observed = dict(records["all_simulations"][GRID[5]][1 if molecular else 0])
    observed[((('A', 1),) * 12, False, 13)] = 4                                          # an observed signal without a key
    opts = dict(heatmap_only=False, zero_only=False, allow_multidrop=True)
    dicts = [records["all_simulations"][p][1 if molecular else 0] for p in GRID]
    signals = H.ordered_signals(set(observed).union(*dicts))
    fit, fit_total = H.fit_matrix(signals, dicts)
    for metric in H.METRICS:
        for norm, cutoff in ((0, None), (1, 3), (2, None)):
            exp = H.scores(H.key_table(observed, signals, **opts), fit, fit_total, metric, norm, cutoff)
            for source in (sweep, records):
                with _prefilled():
                    out = SW.score_device(observed, source, metric, bool(norm & 1), bool(norm & 2), cutoff, molecular=molecular, **opts)
                assert out["signals"] == signals
                assert np.array_equal(out["status"].cpu().numpy(), exp[2]), (metric, norm)
                for got, want in zip((out["score"], out["factor"], out["contributions"]), (exp[0], exp[1], exp[3])):
                    assert _same_bits(got.cpu().numpy(), want), (metric, norm)
            assert (exp[2] == H.SCORE_OK).any()


def test_best_point_is_the_point_the_observed_signals_came_from():
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    sweep, records = _grid_sweep()
    observed = records["all_simulations"][GRID[6]][0]
    scores = SW.score_records(observed, sweep, metric='my_euclidean', heatmap_only=False, zero_only=False, allow_multidrop=True)
    assert list(scores) == GRID
    point, result, factor, contrib = SW.best_point(scores)
    assert point == GRID[6] and result == 0.0 and factor == 1.0 and set(contrib) == set(observed)
    assert min(r for p, (r, _) in scores.items() if p != GRID[6]) > 0.0
    assert SW.best_point(SW.score_records(observed, sweep, metric='naive', normalize_counts=True), reverse_order=True)[0] in GRID
