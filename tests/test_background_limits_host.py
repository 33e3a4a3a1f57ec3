"""Host twin of test_gpu_background_limits.py (no GPU): the problems of tests/_background_limit_cases.py reach the paths they
are meant to reach, and the host twin of the package (_host_background, background_records(device=None)) equals the
restatement (tests/_background_reference.py) on them, bit for bit, NaN equal to NaN.

  F  the full key set of up to 6 drops over 5 cycles: 28 keys with 728 neighbours (MAX_NEIGHBOURS, three levels of the
     pairwise sum) and 21 with 242; the undefined keys, chosen by hand, have 728 and 242 neighbours, an accepted key has 728;
     without multi-drop an interpolated key has fewer than 3^d - 1 neighbours; a one-cycle trial with the mean of nothing
  G  zero totals: the reference's ZeroDivisionError in the restatement, FSQ_BACKGROUND_ZERO_TOTAL in the twin and through
     iterative_peak_finding_v3(device=None): the only trial's total, the head's total, the head's total after the undefined
     key is interpolated (one pass each), and a trial of the second pass, after one acceptance
  H  first_argmax's NaN rule (a NaN in first place stays, elsewhere never wins): a NaN control average in first place gives
     CONVERGED after 2 passes and 2 acceptances, in third and last place NO_IMPROVEMENT after 3 passes and 2 acceptances; at
     entries 255, 256 and 300 of 398 defined keys the NaN is a trial of every pass and the outcome is that of the problem
     without it; infinite and tied infinite z-scores, the first in order accepted first
  I  300 problems, of which two need more than 16 passes and three stop on a zero total

Run time of this file on the host: 5 s (tests/test_chisq_limits_host.py in the same run: 30 s)."""
import numpy as np
import pytest

import _background_limit_cases as BL
import _background_reference as R
from _background_cases import key
from _util import bits_equal
from fluorosequencingimageanalysis_amd import _native_background as NB, background as BG


def _host(args, **kw):
    (res,) = BG.background_records([BG.pack_problem(*args)], device=None, **kw)
    return res


def _twin_equals_restatement(args, what, cap=None):
    """background_records(device=None) against R.iterate: counts, percents, stop, passes and the accepted keys."""
    prob = BG.pack_problem(*args)
    kw = {} if cap is None else {"max_iterations": cap}
    r = R.iterate(*args, **kw)
    res = _host(args, accepted_cap=1024, undefined_cap=4096, **kw)
    assert prob["keys"] == r["keys"], what
    assert bits_equal(res["count"], r["counts"]).all(), what
    pct = np.array([r["updated_boc_percent"].get(k, 0.0) for k in r["keys"]])
    assert bits_equal(res["percent"], pct).all(), what
    assert (res["stop_reason"], res["n_passes"], res["overflow"]) == (r["stop"], r["passes"], 0), what
    assert [prob["keys"][i] for i in res["accepted_key"]] == r["accepted"], what
    assert bits_equal(res["undefined_bp"][len(prob["und_first"]):], [u[3] for u in r["undefined_peaks"]][len(prob["und_first"]):]).all(), what
    return r, res


# ---- F ---------------------------------------------------------------------------------------------------------------------
def test_six_drop_keys_reach_the_full_neighbour_list():
    assert NB.MAX_DROPS >= 6
    args = BL.six_drop_problem(True)
    boc, C = args[0], args[4]
    count = {k: len(R.neighbours(k, C, True)) for k in boc}
    assert len(boc) == 461 and sum(1 for v in count.values() if v == 728) == 28 and sum(1 for v in count.values() if v == 242) == 21
    assert max(count.values()) == 728 == 3 ** 6 - 1
    lacking = BL.LACKING[True]
    assert [count[k] for k in lacking[:2]] == [728, 242] and all(k not in args[2] for k in lacking)
    r, res = _twin_equals_restatement(args, "six drops", BL.SIX_DROP_CAP)
    assert (r["stop"], r["passes"], len(r["accepted"])) == (R.STOP_THRESHOLD, 25, 24)
    assert sum(1 for k in r["accepted"] if count[k] == 728) >= 1 and r["passes"] > 16
    assert {u[:3] for u in r["undefined_peaks"]} == set(lacking)
    # without multi-drop
    args = BL.six_drop_problem(False)
    boc = args[0]
    assert len(boc) == 31 and not any(BG.is_multidrop(k[0]) for k in boc)
    r, res = _twin_equals_restatement(args, "six drops, no multi-drop", BL.SIX_DROP_CAP)
    assert (r["stop"], r["passes"]) == (R.STOP_MAX_ITERATIONS, BL.SIX_DROP_CAP) and len(r["accepted"]) == BL.SIX_DROP_CAP
    interpolated = {u[:3] for u in r["undefined_peaks"]}
    assert interpolated == set(BL.LACKING[False])
    assert any(len(R.neighbours(k, 5, False)) < 3 ** len(k[0]) - 1 and all(1 < p < 5 for _, p in k[0]) for k in interpolated)


def test_one_cycle_trial_has_the_mean_of_nothing():
    args = BL.no_neighbour_problem()
    assert R.neighbours(key(3), 1, True) == [] and not R.passes_filter(key(3), 1, True)
    r, res = _twin_equals_restatement(args, "one cycle", 50)
    assert (r["stop"], r["passes"], r["accepted"]) == (R.STOP_THRESHOLD, 2, [key(3)])
    assert np.isnan(r["counts"][1]) and r["counts"][0] == 100.0 and np.isnan(res["count"][1])


# ---- G ---------------------------------------------------------------------------------------------------------------------
def test_zero_totals_stop_the_twin_where_the_reference_divides_by_zero():
    problems = BL.zero_total_problems()
    assert set(problems) == set(BL.ZERO_TOTAL_OUTCOMES)
    for name, args in problems.items():
        with pytest.raises(ZeroDivisionError):
            R.iterate(*args)
        res = _host(args)
        assert (res["stop_reason"], res["n_passes"], res["n_accepted"]) == (NB.ZERO_TOTAL,) + BL.ZERO_TOTAL_OUTCOMES[name], name
        with pytest.raises(ZeroDivisionError):
            BG.iterative_peak_finding_v3(*args, device=None)
    head = BG.pack_problem(*problems["zero head"])
    assert head["count"].sum() == 0 and len(head["und_first"]) == 0
    late = BG.pack_problem(*problems["zero after interpolation"])
    assert late["count"].sum() != 0 and late["und_first"].tolist() == [0]
    second = _host(problems["zero trial in the second pass"])
    assert second["accepted_key"].tolist() == [0] and second["count"].tolist() == [10.0, 10.0, -10.0, 20.0]
    assert second["count"][[0, 1, 2]].sum() + second["count"][2] == 0       # key(4)'s trial: its count replaced by key(3)'s


# ---- H ---------------------------------------------------------------------------------------------------------------------
def test_nan_and_infinite_scores_follow_the_first_argmax_rule():
    want = {"nan first": (R.STOP_CONVERGED, 2, [key(2), key(2)]), "nan third": (R.STOP_NO_IMPROVEMENT, 3, [key(2), key(4)]),
            "nan last": (R.STOP_NO_IMPROVEMENT, 3, [key(2), key(4)]), "infinite z": (R.STOP_CONVERGED, 3, [key(2), key(4), key(2)]),
            "tied infinite z": (R.STOP_CONVERGED, 3, [key(2), key(4), key(2)])}   # (key(2) stands before key(4): the first in order decides)
    clean, _ = _twin_equals_restatement(BL.nan_lane_problem(None), "clean", 100)
    assert (clean["stop"], clean["passes"], len(clean["accepted"])) == (R.STOP_NO_IMPROVEMENT, 8, 7)
    for name, args in BL.score_problems().items():
        r, res = _twin_equals_restatement(args, name, 100)
        if name in want:
            assert (r["stop"], r["passes"], r["accepted"]) == want[name], name
        else:                                                       # the NaN in another lane and round never wins
            assert (r["stop"], r["passes"], r["accepted"]) == (clean["stop"], clean["passes"], clean["accepted"]), name
    boc, pct, avg, std = BL.five_keys(0)[:4]
    z = [R.z_of(pct[k], avg[k], std[k]) for k in avg]
    assert z[0] != z[0] and z[1] > 2.0                             # the NaN leads the list; the next score would win without it
    tied = BL.score_problems()["tied infinite z"]
    z = [R.z_of(tied[1][k], tied[2][k], tied[3][k]) for k in tied[2]]
    assert z[0] == z[1] == BL.INF
    for e in BL.NAN_ENTRIES:
        boc, pct, avg, std = BL.nan_lane_problem(e)[:4]
        defined = [k for k in avg if std[k] != 0]
        assert len(defined) == 398 and avg[defined[e]] != avg[defined[e]] and sum(1 for k in defined if avg[k] != avg[k]) == 1
        z = R.z_of(pct[defined[e]], avg[defined[e]], std[defined[e]])
        assert z != z and not z <= 2.0                             # a trial of every pass, whose difference is NaN
    assert BL.NAN_ENTRIES[0] // 256 == 0 and BL.NAN_ENTRIES[1] // 256 == 1 and BL.NAN_ENTRIES[0] % 64 == 63 and BL.NAN_ENTRIES[1] % 64 == 0


# ---- I ---------------------------------------------------------------------------------------------------------------------
def test_many_problems_hold_long_runs_and_zero_totals():
    problems = [BG.pack_problem(*args) for args in BL.many_problems()]
    assert len(problems) == 300 and {len(p["keys"]) for p in problems} >= set(range(1, 41))
    res = BG.background_records(problems, max_iterations=BL.MANY_CAP, accepted_cap=64, undefined_cap=256, device=None)
    assert sum(1 for r in res if r["n_passes"] > 16) >= 2 and sum(1 for r in res if r["stop_reason"] == NB.ZERO_TOTAL) == 3
    assert all(r["overflow"] == 0 for r in res) and len({r["stop_reason"] for r in res}) >= 4
    assert sum(1 for r in res if r["n_accepted"] > 0) >= 50
