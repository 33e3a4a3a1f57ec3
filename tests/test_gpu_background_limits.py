"""The iterative background correction at its limits on the GPU (include/fsq_background.h): the problems of
tests/_background_limit_cases.py (tests/test_background_limits_host.py proves that they reach the paths named here), every
output and the workspace pre-filled, bit for bit against the restatement (tests/_background_reference.py) and the host twin,
NaN equal to NaN.

  F  keys of six drops: 728 neighbours (the whole MAX_NEIGHBOURS list, the head's full LDS gather, three levels of the pairwise
     sum in a trial lane) and 242, with and without multi-drop; a one-cycle trial with the mean of nothing
  G  FSQ_BACKGROUND_ZERO_TOTAL from the head, from a trial, after the interpolation and from a trial of the second pass, alone
     and in a batch between two ordinary problems whose results equal their results alone; ZeroDivisionError through
     iterative_peak_finding_v3
  H  first_argmax's NaN rule in the 256-lane reduction: a NaN control average in first, third and last place of five keys and
     at entries 255, 256 and 300 of 398 (another lane, another round); infinite and tied infinite z-scores
  I  300 problems in one call, two of more than 16 passes and three zero totals among them: each equals its run alone on the
     host twin, overflow 0

Measured durations on the MI355X (--durations): six drops with multi-drop 2.1 s (1.4 s of it the restatement's 25 passes over
461 keys on the host, and the first launch of the process), 300 problems 0.7 s, every other test below 0.1 s; the whole file
3.5 s.  The slowest test of the existing limits files in the same kind of run is the pow sweep of test_gpu_chisq_limits.py at
2.9 s.
"""
import contextlib

import numpy as np
import pytest

import _background_limit_cases as BL
import _background_reference as R
from fluorosequencingimageanalysis_amd import _native_background as NB

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _prefilled():
    """Every tensor the binding allocates (outputs and workspace) starts as a byte pattern, not as zeros."""
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


def _records(problems, device="cuda", **kw):
    from fluorosequencingimageanalysis_amd import background as BG
    kw = dict(dict(accepted_cap=64, undefined_cap=64), **kw)
    with _prefilled():
        return BG.background_records(problems, device=device, **kw)


def _same_bits(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and ((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all(), what


def _same(got, exp, what):
    for k in ("stop_reason", "n_passes", "n_accepted", "overflow"):
        assert got[k] == exp[k], (what, k, got[k], exp[k])
    for k in ("count", "percent", "undefined_bp"):
        _same_bits(got[k], exp[k], (what, k))
    assert got["rounded"].tolist() == exp["rounded"].tolist() and got["accepted_key"].tolist() == exp["accepted_key"].tolist(), what


def _same_as_restatement(got, prob, r, what):
    """The device's records against R.iterate's result: counts, percents, stop, passes, accepted keys."""
    assert prob["keys"] == r["keys"], what
    _same_bits(got["count"], r["counts"], (what, "count"))
    _same_bits(got["percent"], [r["updated_boc_percent"].get(k, 0.0) for k in r["keys"]], (what, "percent"))
    assert (got["stop_reason"], got["n_passes"], got["overflow"]) == (r["stop"], r["passes"], 0), what
    assert [prob["keys"][i] for i in got["accepted_key"]] == r["accepted"], what


def _against_restatement(args, what, cap):
    from fluorosequencingimageanalysis_amd import background as BG
    prob = BG.pack_problem(*args)
    kw = dict(max_iterations=cap, accepted_cap=128, undefined_cap=512)
    (got,) = _records([prob], **kw)
    r = R.iterate(*args, max_iterations=cap)
    _same_as_restatement(got, prob, r, what)
    (twin,) = _records([prob], device=None, **kw)
    _same(got, twin, what)
    return got, r


# ---- F ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("multidrop", [True, False])
def test_keys_of_six_drops(multidrop):
    got, r = _against_restatement(BL.six_drop_problem(multidrop), ("six drops", multidrop), BL.SIX_DROP_CAP)
    assert got["n_passes"] == (25 if multidrop else BL.SIX_DROP_CAP) and got["n_accepted"] >= 24


def test_one_cycle_trial_with_the_mean_of_nothing():
    got, r = _against_restatement(BL.no_neighbour_problem(), "one cycle", 50)
    assert np.isnan(got["count"][1]) and got["n_accepted"] == 1 and got["stop_reason"] == NB.THRESHOLD


# ---- G ---------------------------------------------------------------------------------------------------------------------
def test_zero_totals_alone_and_in_a_batch():
    from fluorosequencingimageanalysis_amd import background as BG
    zero = {name: BG.pack_problem(*args) for name, args in BL.zero_total_problems().items()}
    for name, prob in zero.items():
        (got,) = _records([prob])
        (exp,) = _records([prob], device=None)
        assert (got["stop_reason"], got["n_passes"], got["n_accepted"]) == (NB.ZERO_TOTAL,) + BL.ZERO_TOTAL_OUTCOMES[name], name
        assert got["overflow"] == 0, name
        _same(got, exp, name)
        with pytest.raises(ZeroDivisionError):
            with _prefilled():
                BG.iterative_peak_finding_v3(*BL.zero_total_problems()[name], device="cuda")
    first, last = (BG.pack_problem(*args) for args in BL.ordinary_problems())
    batch = _records([first] + list(zero.values()) + [last])
    exp = _records([first] + list(zero.values()) + [last], device=None)
    for p, (got, e) in enumerate(zip(batch, exp)):
        _same(got, e, p)
    for p, (prob, args) in ((0, (first, BL.ordinary_problems()[0])), (len(batch) - 1, (last, BL.ordinary_problems()[1]))):
        (alone,) = _records([prob])
        _same(batch[p], alone, ("alone", p))
        _same_as_restatement(batch[p], prob, R.iterate(*args), ("restatement", p))
        assert batch[p]["stop_reason"] != NB.ZERO_TOTAL


# ---- H ---------------------------------------------------------------------------------------------------------------------
def test_nan_and_infinite_scores():
    from fluorosequencingimageanalysis_amd import background as BG
    for name, args in BL.score_problems().items():
        _against_restatement(args, name, 100)
    probs = [BG.pack_problem(*args) for args in BL.score_problems().values()]
    for p, (got, e) in enumerate(zip(_records(probs), _records(probs, device=None))):
        _same(got, e, ("batch", p))


# ---- I ---------------------------------------------------------------------------------------------------------------------
def test_300_problems_in_one_call():
    from fluorosequencingimageanalysis_amd import background as BG
    problems = [BG.pack_problem(*args) for args in BL.many_problems()]
    kw = dict(max_iterations=BL.MANY_CAP, accepted_cap=64, undefined_cap=256)
    batch = _records(problems, **kw)
    alone = _records(problems, device=None, **kw)                   # (the host twin runs every problem on its own)
    assert len(batch) == BL.MANY
    for p, (got, e) in enumerate(zip(batch, alone)):
        _same(got, e, p)
        assert got["overflow"] == 0, p
    assert sum(1 for r in batch if r["n_passes"] > 16) >= 2 and sum(1 for r in batch if r["stop_reason"] == NB.ZERO_TOTAL) == 3
