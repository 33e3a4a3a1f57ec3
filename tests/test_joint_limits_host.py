"""Host twin of test_gpu_joint_limits.py (no GPU): the inputs of tests/_joint_limit_cases.py reach the edges they are meant to
reach, so that the GPU tests cannot pass vacuously, and the vectorised expectation of the large tally equals the plain twin on
its prefix.  The counts are floors on the inputs.

  C  for K = 1 .. 4 the extreme molecule is a signal with the key 0xffffffffffffffff (0xff0bfbfbfbfbfbff for K = 3), one lost
     dye more has no key, and the keys round-trip through the codec; 16 384 x 256 + 300 rows of 997 base molecules over three
     points, whose np.add.at expectation equals H.tally_joint_rows on the first 50 000 rows; 2^26 + 300 rows of 64 frames,
     whose channel stride is 2^32 + 19 200 bytes, with a closed-form expectation that equals H.tally_joint_rows on 20 000 rows
  D  70 points x 3 molecules of three letters at 1 frame and four letters at 64 frames with the extremes of
     _simulate_limit_cases.B_EXTREMES: all duds, nothing cut, everything lost at cycle 1; 2 x 1 048 576 + 130 rows of five
     points from row 100, every window round a seam or a point boundary holding a count in both channels
  E  the twelve candidates of the thousand-point pair run give best points, errors of both kinds and pairs without a result;
     every point of the eight-lysine sweep has at least 5 molecular and 5 fitted signals whose key has bit 63 set

Run time of this file on the host: 5 s."""
import numpy as np

import _joint_limit_cases as LC
import _simulate_limit_cases as SL
from _joint_sweep_cases import GRID4, LETTERS
from fluorosequencingimageanalysis_amd import _host_peptide_sim as PSIM
from fluorosequencingimageanalysis_amd import _host_signal_sweep as H


# ---- C ---------------------------------------------------------------------------------------------------------------------
def test_the_extreme_molecules_have_the_extreme_keys():
    for K in (1, 2, 3, 4):
        letters = LETTERS[K]
        what, key = H.classify_joint_rows(LC.extreme_rows(K))
        assert (what, key) == (H.ROW_SIGNAL, LC.EXTREME_KEYS[K]) and key & LC.TOP_BIT, K
        assert H.classify_joint_rows(LC.extreme_rows(K, more=1)) == (H.ROW_UNKEYED, None), K
        signal = H.joint_signal_of_key(letters, key)
        assert signal == (((letters[K - 1], 63),) * H.JOINT_MAX_DROPS[K], (False,) * K, (15,) * K), K
        assert H.joint_key_of_signal(letters, signal) == key and H.joint_signals_of_keys(letters, np.array([key], np.uint64)) == [signal]
        assert H.joint_signal_of_key(letters, np.array([key], np.uint64).view(np.int64)[0]) == signal     # as an int64 tensor holds it
        rows, keyed = LC.extreme_molecules(K)
        assert rows.shape == (K, sum(LC.EXTREME_COPIES), 64) and [n for _, n in keyed] == list(LC.EXTREME_COPIES)
        keys = [k for k, _ in keyed]
        assert keys[0] == key and keys[1] == 0 and 0 < keys[2] and not keys[2] & LC.TOP_BIT and len(set(keys)) == 3
        assert all(H.joint_key_of_signal(letters, H.joint_signal_of_key(letters, k)) == k for k in keys)
        assert H.EMPTY not in keys and H.NEVER not in keys
        for reserved in (H.EMPTY, H.NEVER):
            try:
                H.joint_signal_of_key(letters, reserved)
            except ValueError:
                continue
            raise AssertionError("a reserved pattern decodes to a signal")
    assert H.classify_joint_rows(LC.extreme_rows(1)) == (H.ROW_SIGNAL, H.classify_row(LC.extreme_rows(1)[0])[1])


def test_the_large_joint_tally_and_its_vectorised_count():
    base = LC.tally_base()
    kinds = [H.classify_joint_rows(base[:, j].tolist())[0] for j in range(LC.T_BASE)]
    assert base.shape == (2, 997, 3) and LC.T_N == 16384 * 256 + 300 and LC.T_PER * 2 < LC.T_N <= LC.T_PER * 3
    assert kinds.count(H.ROW_NONE) >= 20 and kinds.count(H.ROW_UNKEYED) == 0 and kinds.count(H.ROW_SIGNAL) >= 900
    assert (16384 * 256) % 997 != 0 and LC.T_PER % 256 != 0                    # a block's second pass meets other molecules; points change inside blocks
    valid = LC.tally_valid()
    assert 0.88 < valid.mean() < 0.92
    for lo, hi, v in ((0, 50000, None), (0, 50000, valid), (LC.T_PER - 2500, LC.T_PER + 2500, valid)):
        rows, points = LC.tally_rows_of(lo, hi)
        assert LC.tally_expected(lo, hi, v) == H.tally_joint_rows(rows, points, None if v is None else v[lo:hi], LC.T_POINTS), lo
    tables, none, unkeyed = LC.tally_expected(0, LC.T_N, valid)
    assert sum(sum(t.values()) for t in tables) + sum(none) == int(valid.sum()) and min(none) > 0 and unkeyed == [0, 0, 0]
    assert all(50 < len(t) <= LC.T_SLOTS // 2 for t in tables)
    a, b = LC.tally_expected(0, LC.T_CUT, valid), LC.tally_expected(LC.T_CUT, LC.T_N, valid)
    assert [{k: a[0][p].get(k, 0) + b[0][p].get(k, 0) for k in set(a[0][p]) | set(b[0][p])} for p in range(3)] == tables


def test_the_wide_joint_tally_has_a_channel_stride_beyond_32_bits():
    stride = LC.W_N * LC.W_FRAMES
    assert stride == (1 << 32) + 64 * LC.W_SHIFT and stride & 0xffffffff == 64 * LC.W_SHIFT and LC.W_SHIFT % LC.W_BASE
    assert LC.W_K * stride < 10 * 10 ** 9                                      # 8.6 GB of rows
    base = LC.wide_base()
    kinds = [H.classify_joint_rows(base[:, j].tolist()) for j in range(LC.W_BASE)]
    assert base.shape == (2, 101, 64) and sum(k[0] == H.ROW_SIGNAL for k in kinds) >= 90 and all(k[0] != H.ROW_UNKEYED for k in kinds)
    assert len({k[1] for k in kinds} - {None}) >= 90                           # (and a block's distinct keys fit its LDS sub-tables)
    for lo, hi in ((0, 20000), (LC.W_PER - 3000, LC.W_PER + 3000), (12345, 12346), (7, 7)):
        n = np.zeros((LC.W_POINTS, LC.W_BASE), np.int64)
        i = np.arange(lo, hi)
        np.add.at(n, (i // LC.W_PER, i % LC.W_BASE), 1)
        assert np.array_equal(LC.wide_counts(lo, hi), n), (lo, hi)
        rows, points = LC.wide_rows_of(lo, hi)
        assert LC.wide_expected(lo, hi) == H.tally_joint_rows(rows, points, None, LC.W_POINTS), (lo, hi)
    whole = LC.wide_counts(0, LC.W_N)
    assert whole.sum() == LC.W_N and whole.min() > 200000 and LC.W_PER * 2 < LC.W_N <= LC.W_PER * 3
    tables, none, unkeyed = LC.wide_expected()
    assert sum(sum(t.values()) for t in tables) + sum(none) == LC.W_N and unkeyed == [0, 0, 0]
    # channel 1 read through a stride of 32 bits gives other tables: the case tells the two apart
    rows, points = LC.wide_rows_of(0, 20000, shift=LC.W_SHIFT)
    assert H.tally_joint_rows(rows, points, None, LC.W_POINTS)[0] != LC.wide_expected(0, 20000)[0]


# ---- D ---------------------------------------------------------------------------------------------------------------------
def test_the_extremes_do_what_they_say_in_every_channel():
    pts = SL.limit_points()
    where = {(name, value): k for k, (name, value) in SL.B_EXTREMES.items()}
    keys = ("counts", "intensity", "category", "loss_cause", "edman_fail")
    for name, ((sequence, labels, mocks, edmans), _) in LC.D_SHAPES.items():
        K, F = len(labels), mocks + edmans + 1
        for stride in (0, 5):
            counts, intensity, category, cause, fail = LC.extreme_points_expected(name, stride, keys)
            assert counts.shape == (K, 210, F) and category.shape == (K, 210)
            per = counts.reshape(K, 70, SL.B_PER, F)
            point = lambda x, k: x[3 * k:3 * k + 3]                                              # noqa: E731
            duds = where[("u", 1.0)]
            assert pts[duds, 2] == 1.0 and not per[:, duds].any() and (point(cause, duds) == PSIM.CAUSE_DUD).all()       # all duds
            assert not intensity.reshape(K, 70, -1)[:, duds].any() and not category.reshape(K, 70, -1)[:, duds].any()
            assert all(per[k, duds - 1].any() and per[k, duds + 1].any() for k in range(K)), (name, stride)               # its neighbours are not
            assert not (point(cause, where[("u", 0.0)]) == PSIM.CAUSE_DUD).any()
            if edmans:
                edman_cycles = sum(1 << c for c in range(mocks + 1, F))
                assert (point(fail, where[("p", 0.0)]) == edman_cycles).all()                    # nothing cut
                assert not (point(cause, where[("p", 0.0)]) == PSIM.CAUSE_EDMAN).any()
                assert (point(fail, where[("p", 1.0)]) == 0).all()
                lost = where[("s", 1.0)]
                assert (per[:, lost, :, 1:] == 0).all() and per[:, lost, :, 0].any()             # everything lost at cycle 1
                assert (per[:, where[("s2", 1.0)], :, 5:] == 0).all()                            # nothing survives the cycle after sc
                assert (counts[:, :, 63] > 0).any() and (category >> np.uint64(63)).any()        # a dye is kept to frame 63
                assert counts[:, :, 0].max() == 6
            assert (per[:, where[("per_cycle_b", 0.0)]] == 0).all()                              # nothing survives the first exposure
            assert not (point(cause, where[("per_cycle_b", 1.0)]) == PSIM.CAUSE_DESTRUCTION).any()
        a, b = LC.extreme_points_expected(name, 0, keys)[0], LC.extreme_points_expected(name, 5, keys)[0]
        assert np.array_equal(a[:, :3], b[:, :3]) and not np.array_equal(a, b)                  # the stride moves every point but the first
    assert 21 * SL.B_PER <= 63 < 22 * SL.B_PER                                                   # the u = 1 point lies across the first wavefront's end


def test_the_rows_of_more_than_two_passes():
    assert LC.P_ROWS == 2 * 1048576 + 130 and LC.P_PER % 64 and LC.P_FIRST_ROW % 64
    assert LC.P_FIRST_ROW + LC.P_ROWS <= len(LC.P_POINTS) * LC.P_PER
    lanes = {(k * LC.P_PER - LC.P_FIRST_ROW) % 64 for k in range(1, 5)}
    assert len(lanes) == 4 and 0 not in lanes                                  # point boundaries inside wavefronts, at four lanes
    ranges = LC.p_point_ranges()
    assert [r[0] for r in ranges] == [0, 1, 2, 3, 4] and ranges[0][1] == 0 and ranges[-1][2] == LC.P_ROWS
    assert all(a[2] == b[1] for a, b in zip(ranges, ranges[1:])) and ranges[0][3] == LC.P_FIRST_MOLECULE + LC.P_FIRST_ROW
    exp, windows = LC.p_expected(), LC.p_windows()
    assert len(windows) == 8 and windows[1][1] == LC.P_ROWS and windows[3][1] < LC.P_ROWS
    for (lo, hi), (counts, intensity, category) in exp.items():
        assert counts.shape == (2, hi - lo, 2) and intensity.shape == counts.shape and category.shape == (2, hi - lo)
        assert all(counts[k].any() and (intensity[k] > 0).any() and category[k].any() for k in range(2)), (lo, hi)
    sides = []
    for k in range(1, 5):                                                      # the 70 rows before and after a point boundary
        counts = exp[windows[3 + k]][0]
        sides += [counts[:, :70].tobytes(), counts[:, 70:].tobytes()]
    assert len(set(sides)) == 8


# ---- E ---------------------------------------------------------------------------------------------------------------------
def test_the_pair_run_over_a_thousand_points_holds_every_outcome():
    table, fit, total = SL.score_case(LC.E_S, LC.E_P)
    n_sel = len(LC.E_ROWS)
    assert fit.shape == (60, 1000) and n_sel == 12 and LC.E_ROWS.count(-1) == 1 and not table["admitted"][6]
    statuses, best_points = set(), set()
    for metric in LC.E_METRICS:
        for (norm, reverse), (best, (score, n)) in LC.pair_expected(metric).items():
            assert best["best_point"].shape == (66,) and score.shape == (12,) and n.dtype == np.int32
            assert (best["best_point"] >= 0).sum() >= 20 and (best["best_point"] < 0).any(), (metric, norm, reverse)
            statuses |= set(best["error_status"].tolist())
            best_points |= set(best["best_point"].tolist())
            assert np.isnan(score).any() and not np.isnan(score).all()
    assert statuses == {0, H.SCORE_DIVZERO, H.SCORE_DOMAIN}
    assert max(best_points) >= 64 * 8 and len(best_points) >= 10               # best points far beyond the first blocks
    for metric in LC.E_METRICS:                                                # the two orders are told apart
        runs = LC.pair_expected(metric)
        assert not np.array_equal(runs[(1, False)][0]["best_point"], runs[(1, True)][0]["best_point"])


def test_every_point_of_the_sweep_has_keys_with_bit_63():
    sweep = LC.top_bit_sweep()
    assert sweep["points"] == GRID4 and sweep["labels"] == LC.TOP_LETTERS
    for key in GRID4:
        fitted, molecular = sweep["all_simulations"][key]
        assert sum(LC.has_top_bit(s) for s in molecular) >= 5 and sum(LC.has_top_bit(s) for s in fitted) >= 5, key
        assert max(s[2][1] for s in molecular) == 8 and sweep["total_count"][key] > 150
    observed, cand = LC.top_bit_observed(), LC.top_bit_candidates()
    assert len(cand) == 20 == len(set(cand)) and sum(LC.has_top_bit(s) for s in cand) == 8 and all(s in observed for s in cand[12:])
