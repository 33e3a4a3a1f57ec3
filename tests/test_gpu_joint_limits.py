"""The joint-signal sweep and the multi-letter simulation on the GPU at their limits (include/fsq_signal_sweep.h,
fsq_peptide_labels.h): the inputs of tests/_joint_limit_cases.py, whose edges tests/test_joint_limits_host.py proves without a
GPU, against the NumPy twins and the single-point kernel.  Every output buffer starts as a byte pattern; nothing is compared
with a tolerance, NaNs are one pattern.

  C  fsq_signal_tally_joint and fsq_signal_lookup on the joint key's extreme values (bit 63 and all below it) for K = 1 .. 4,
     a joint tally of more rows than one pass of the grid, whole and in two uneven calls, and one whose channel stride does
     not fit 32 bits
  D  fsq_peptide_simulate_labels_points against the twin with extreme parameters side by side in a wavefront at 1 and at 64
     frames, and over more than two passes of its grid
  E  fsq_signal_pair_best and fsq_signal_pair_extremes over a thousand points, and a sweep whose keys carry bit 63 through the
     records, the scores, the pair loop and match_diagnostic

Run time of this file on an MI355X: 5 s for its 19 tests, 1.7 s of them the first test (it starts the device); the pair kernel
over a thousand points 0.37 s a metric with its host twin, the tally over one pass 0.3 s, the tally of 8.6 GB of rows 0.10 s,
the points kernel over two passes 0.11 s."""
import contextlib

import numpy as np
import pytest

import _joint_limit_cases as LC
import _simulate_limit_cases as SL
from _incompatibility_cases import OUTPUTS, assert_same_outputs, same_bits
from _joint_sweep_cases import GRID4, LETTERS
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


# ---- C: the joint key's extreme values -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_the_extreme_joint_keys_through_tally_lookup_and_codec(K):
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    rows, keyed = LC.extreme_molecules(K)
    n = rows.shape[1]
    tables = SW.new_tables(1, 4, torch.device("cuda"))
    order = np.random.default_rng(K).permutation(n)                            # the three molecules mixed among the lanes
    SW.tally_joint_device(tables, torch.from_numpy(np.ascontiguousarray(rows[:, order])).cuda(), torch.zeros(n, dtype=torch.int32, device="cuda"))
    exp = dict(keyed)
    assert exp[LC.EXTREME_KEYS[K]] == LC.EXTREME_COPIES[0] and exp[0] == LC.EXTREME_COPIES[1]
    assert _decode(tables) == ([exp], [0], [0], [0])
    wanted = [k for k, _ in keyed] + [H.EMPTY, H.NEVER]
    with _prefilled():
        got = SW.lookup_device(tables, torch.from_numpy(np.array(wanted, np.uint64).view(np.int64)).cuda()).cpu().numpy()
    assert got.tolist() == [[c] for _, c in keyed] + [[0], [0]]
    letters = LETTERS[K]
    decoded = SW._decode_tables(tables, letters)                               # joint_signals_of_keys on the table's own keys
    assert decoded == [{H.joint_signal_of_key(letters, k): c for k, c in keyed}]
    occupied = tables["keys"][tables["keys"] != H.EMPTY]                       # the int64 view, as _counts_on_device reads it
    assert sorted(int(k) & LC.ALL_ONES for k in torch.unique(occupied).cpu().tolist()) == sorted(exp)
    one_more = np.array(LC.extreme_rows(K, more=1), np.uint8)[:, None, :]
    SW.tally_joint_device(tables, torch.from_numpy(np.ascontiguousarray(one_more)).cuda(), torch.zeros(1, dtype=torch.int32, device="cuda"))
    assert _decode(tables) == ([exp], [0], [1], [0])


def test_joint_tally_over_more_rows_than_one_pass():
    """16 384 blocks of 256 rows: the first 300 rows' blocks go round twice, with other molecules (997 is prime), and channel
    1 lies 12.6 M bytes beyond channel 0."""
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    dev = torch.device("cuda")
    i = torch.arange(LC.T_N, device=dev)
    d_rows = torch.from_numpy(LC.tally_base()).to(dev)[:, i % LC.T_BASE].contiguous()
    d_point = torch.div(i, LC.T_PER, rounding_mode="floor").to(torch.int32)
    valid = LC.tally_valid()
    d_valid = torch.from_numpy(valid).to(dev)
    assert tuple(d_rows.shape) == (LC.T_K, LC.T_N, LC.T_FRAMES)
    exp = LC.tally_expected(0, LC.T_N, valid) + ([0] * LC.T_POINTS,)
    whole = SW.new_tables(LC.T_POINTS, LC.T_SLOTS, dev)
    SW.tally_joint_device(whole, d_rows, d_point, d_valid)
    assert _decode(whole) == exp
    halves, cut = SW.new_tables(LC.T_POINTS, LC.T_SLOTS, dev), LC.T_CUT
    SW.tally_joint_device(halves, d_rows[:, :cut].contiguous(), d_point[:cut], d_valid[:cut])
    SW.tally_joint_device(halves, d_rows[:, cut:].contiguous(), d_point[cut:], d_valid[cut:])
    assert _decode(halves) == exp


def test_joint_tally_with_channels_more_than_four_gibibytes_apart():
    """2^26 + 300 molecules of 64 frames: channel 1 lies 2^32 + 19 200 bytes beyond channel 0, so the channel stride needs 64
    bits.  8.6 GB of rows, gathered on the device from 101 molecules and given back afterwards."""
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    dev = torch.device("cuda")
    d_base = torch.from_numpy(LC.wide_base()).to(dev)
    d_rows = torch.empty((LC.W_K, LC.W_N, LC.W_FRAMES), dtype=torch.uint8, device=dev)
    d_point = torch.empty(LC.W_N, dtype=torch.int32, device=dev)
    for lo in range(0, LC.W_N, 1 << 24):                                       # (2^30 elements a copy)
        i = torch.arange(lo, min(lo + (1 << 24), LC.W_N), device=dev)
        d_point[lo:lo + len(i)] = torch.div(i, LC.W_PER, rounding_mode="floor")
        i.remainder_(LC.W_BASE)
        for k in range(LC.W_K):
            d_rows[k, lo:lo + len(i)] = d_base[k][i]
    del i
    tables = SW.new_tables(LC.W_POINTS, LC.W_SLOTS, dev)
    SW.tally_joint_device(tables, d_rows, d_point)
    got = _decode(tables)
    del d_rows, d_point
    torch.cuda.empty_cache()
    assert got == LC.wide_expected() + ([0] * LC.W_POINTS,)


# ---- D: the multi-letter points kernel -----------------------------------------------------------------------------------------
def _same_rows(got, exp, what):
    """(counts, intensity, category) as host arrays, bit for bit."""
    assert got[0].shape == exp[0].shape and np.array_equal(got[0], exp[0]), what
    assert SL.same(got[1], exp[1]), what
    assert np.array_equal(np.asarray(got[2]).view(np.uint64), np.asarray(exp[2]).view(np.uint64)), what


@pytest.mark.parametrize("stride", [0, 5])
@pytest.mark.parametrize("shape_name", sorted(LC.D_SHAPES))
def test_labels_points_with_extreme_parameters_in_neighbouring_lanes(shape_name, stride):
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    shape, fixed = LC.D_SHAPES[shape_name]
    prm, values, letters = LC.labels_params(shape, fixed, SL.limit_points(), LC.D_SEED, LC.D_FIRST_MOLECULE)
    with _prefilled():
        out = SW.simulate_labels_points_device(prm, torch.from_numpy(values).cuda(), SL.B_POINTS, SL.B_PER, stride)
        got = [out[k].cpu().numpy() for k in ("counts", "intensity", "category")]
    assert got[0].shape == (len(letters), SL.B_POINTS * SL.B_PER, shape[2] + shape[3] + 1) and got[0].dtype == np.uint8
    _same_rows(got, LC.extreme_points_expected(shape_name, stride), (shape_name, stride))


def test_labels_points_over_more_rows_than_two_passes():
    """16 384 blocks of 64 rows are launched at most: every block goes twice round its loop here and the first three a third
    time, from a first row inside a wavefront, and every point boundary falls inside a wavefront."""
    import torch
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS, signal_sweep as SW
    prm, values, _ = LC.labels_params(LC.P_SHAPE, LC.P_FIXED, LC.P_POINTS, LC.P_SEED, LC.P_FIRST_MOLECULE)
    with _prefilled():
        got = SW.simulate_labels_points_device(prm, torch.from_numpy(values).cuda(), len(LC.P_POINTS), LC.P_PER, LC.P_STRIDE,
                                               LC.P_FIRST_ROW, LC.P_ROWS)
        assert tuple(got["counts"].shape) == (2, LC.P_ROWS, 2)
        for k, lo, hi, first in LC.p_point_ranges():
            p, per_cycle_b, u, s, s2 = LC.P_POINTS[k].tolist()
            one = PS.multilabel_device(*LC.P_SHAPE, hi - lo, LC.P_SEED, first, p=p, per_cycle_b=per_cycle_b, u=u, s=s, s2=s2, **LC.P_FIXED)
            assert torch.equal(got["counts"][:, lo:hi], one["counts"]), k
            assert torch.equal(got["intensity"][:, lo:hi].view(torch.int64), one["intensity"].view(torch.int64)), k
            assert torch.equal(got["category"][:, lo:hi], one["category"]), k
            assert bool(one["counts"][0].any()) and bool(one["counts"][1].any())
    for (lo, hi), exp in LC.p_expected().items():
        _same_rows([got[k][:, lo:hi].cpu().numpy() for k in ("counts", "intensity", "category")], exp, (lo, hi))


# ---- E: the pair kernel over a sweep-sized grid --------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", LC.E_METRICS)
def test_pair_best_over_a_thousand_points(metric):
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    table, fit, total = SL.score_case(LC.E_S, LC.E_P)
    d_fit, d_total = torch.from_numpy(fit).cuda(), torch.from_numpy(total).cuda()
    for (norm, reverse), (want, (want_score, want_n)) in LC.pair_expected(metric).items():
        with _prefilled():
            out = SW.pair_best_device(table, LC.E_ROWS, d_fit, d_total, metric, norm, None, reverse)
            score, n = SW.pair_extremes_device(out["dist"], len(LC.E_ROWS), reverse)
            got = {k: out[k].cpu().numpy() for k in OUTPUTS}
        assert_same_outputs(got, want, (metric, norm, reverse))
        assert same_bits(score.cpu().numpy(), want_score) and np.array_equal(n.cpu().numpy(), want_n), (metric, norm, reverse)
        assert n.cpu().numpy().dtype == want_n.dtype


# ---- E: a sweep whose keys carry bit 63 ----------------------------------------------------------------------------------------
def _bits(x):
    return None if x is None else np.float64(x).view(np.uint64)


def test_a_sweep_with_top_bit_keys_is_its_host_twin():
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    host = LC.top_bit_sweep()
    with _prefilled():
        got = SW.joint_sweep_records(*LC.TOP_SHAPE, GRID4, LC.TOP_N, **LC.TOP_KW)
    assert got == host
    assert all(sum(LC.has_top_bit(s) for s in got["all_simulations"][key][j]) >= 5 for key in GRID4 for j in (0, 1))


@pytest.mark.parametrize("metric, norm", [("my_euclidean", {}), ("my_canberra", dict(normalize_counts=True)),
                                          ("my_std_normalized_chebyshev", {})])
def test_scores_and_pairs_over_top_bit_keys_are_their_host_twins_bit_for_bit(metric, norm):
    """(No molecule of eight lysines gives a heat-map signal, so heatmap_normalize_counts would end every point in the
    reference's ZeroDivisionError: the normalisations here are none and normalize_counts.)"""
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    host, observed, cand = LC.top_bit_sweep(), LC.top_bit_observed(), LC.top_bit_candidates()
    dev = SW.joint_sweep_device(*LC.TOP_SHAPE, GRID4, LC.TOP_N, **LC.TOP_KW)
    opts = dict(metric=metric, on_error="none", heatmap_only=False, zero_only=False, allow_multidrop=True, **norm)
    for molecular in (False, True):
        exp = SW.score_records(observed, host, host=True, molecular=molecular, **opts)
        for sweep in (dev, host):                                              # the tables where they are, and uploaded dicts
            with _prefilled():
                got = SW.score_records(observed, sweep, molecular=molecular, **opts)
            assert list(got) == GRID4 == list(exp)
            for key in GRID4:
                (r, (f, c)), (er, (ef, ec)) = got[key], exp[key]
                assert _bits(r) == _bits(er) and _bits(f) == _bits(ef) and set(c) == set(ec), key
                assert all(_bits(c[s]) == _bits(ec[s]) for s in c), key
        assert any(LC.has_top_bit(s) for _, (_, c) in exp.values() for s in c)            # top-bit keys contribute to the scores
    assert sum(r is not None for r, _ in exp.values()) >= 3
    with _prefilled():
        got = SW.incompatibility_records(observed, dev, cand, **opts)
    exp = SW.incompatibility_records(observed, host, cand, host=True, **opts)
    assert set(got["scores"]) == set(exp["scores"]) and sum(LC.has_top_bit(s) for s in exp["scores"]) >= 4
    assert all(_bits(got["scores"][s]) == _bits(exp["scores"][s]) for s in exp["scores"])
    assert list(got["pairs"]) == list(exp["pairs"]) and len(exp["pairs"]) == 190
    for pair, (point, dist, factor) in exp["pairs"].items():
        g = got["pairs"][pair]
        assert g[0] == point and [_bits(x) for x in g[1]] == [_bits(x) for x in dist] and _bits(g[2]) == _bits(factor), pair


def test_match_diagnostic_of_a_sweep_with_top_bit_keys():
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    host, observed = LC.top_bit_sweep(), LC.top_bit_observed()
    dev = SW.joint_sweep_device(*LC.TOP_SHAPE, GRID4, LC.TOP_N, **LC.TOP_KW)
    # metric, reverse_order, normalize_counts, heatmap_normalize_counts, heatmap_only, zero_only, allow_multidrop, small_count_cutoff,
    # matching_p, split_cycle, incompatibility_threshold, compute_incompatibility_scores, num_mocks, num_mocks_omitted, num_edmans
    args = (observed, "my_euclidean", False, True, False, False, False, False, None, 0.1, 2, 1e9, True, 1, 0, 3)
    got, exp = SW.match_diagnostic(dev, *args, on_error="none"), SW.match_diagnostic(host, *args, host=True, on_error="none")
    for k in ("optimal_pbu", "normalized_plot_signals", "normalized_plot_molecular_signals", "exclude_signals", "tables", "labels"):
        assert got[k] == exp[k], k
    assert _bits(got["result"]) == _bits(exp["result"]) and _bits(got["normalization_factor"]) == _bits(exp["normalization_factor"])
    assert {s: _bits(v) for s, v in got["incompatibility_scores"].items()} == {s: _bits(v) for s, v in exp["incompatibility_scores"].items()}
    assert {s: _bits(v) for s, v in got["diff_plot_signals"].items()} == {s: _bits(v) for s, v in exp["diff_plot_signals"].items()}
    assert {s: _bits(v) for s, v in got["optimal_contributions"].items()} == {s: _bits(v) for s, v in exp["optimal_contributions"].items()}
    assert sum(LC.has_top_bit(s) for s in exp["normalized_plot_signals"]) >= 5 and any(LC.has_top_bit(s) for s in exp["optimal_contributions"])
