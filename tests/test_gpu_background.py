"""Iterative background correction on the GPU (include/fsq_background.h): bit for bit against the reference's recorded outputs
(tests/golden/background_signals.npz) and, at shapes the fixture does not hold, against the numpy restatement
(tests/_background_reference.py).  Nothing is compared with a tolerance; NaN equals NaN."""
import contextlib
import os

import numpy as np
import pytest

import _background_reference as R
from _background_cases import bits, case, case_names, key, problem, same_dict, same_peaks, tiny_problem

pytestmark = pytest.mark.gpu

TRIAL_THREADS, HEAD_THREADS, TILE = 64, 256, 1024


@contextlib.contextmanager
def _prefilled():
    """Every output tensor the binding allocates starts as a byte pattern, not as zeros: what a kernel leaves unwritten shows."""
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


def _v3_args(c):
    return (c["boc_experiment"], c["boc_percent"], c["averaged_ac"], c["ac_stds"], c["num_cycles"], c["sigma"], not c["omit_multidrop"])


def _device_v3(args):
    from fluorosequencingimageanalysis_amd import background as BG
    info = {}
    with _prefilled():
        peak_list, undefined_peaks, raw, pct = BG.iterative_peak_finding_v3(*args, device="cuda", info=info)
    assert peak_list == []
    return undefined_peaks, raw, pct, info


def _check_against_restatement(args, what):
    r = R.iterate(*args)
    undefined_peaks, raw, pct, info = _device_v3(args)
    same_dict(raw, r["updated_boc_raw"], what)
    same_dict(pct, r["updated_boc_percent"], what)
    same_peaks(undefined_peaks, r["undefined_peaks"], what)
    assert (info["stop_reason"], info["n_passes"], info["accepted_keys"]) == (r["stop"], r["passes"], r["accepted"]), what
    return r


def _records(problems, **kw):
    from fluorosequencingimageanalysis_amd import background as BG
    with _prefilled():
        return BG.background_records(problems, device="cuda", **kw)


def _same_records(got, exp, what=None):
    for k in ("stop_reason", "n_passes", "n_accepted", "overflow"):
        assert got[k] == exp[k], (what, k, got[k], exp[k])
    for k in ("count", "percent", "undefined_bp"):
        assert bits(got[k]) == bits(exp[k]) or (np.isnan(got[k]) == np.isnan(exp[k])).all() and \
            bits(np.nan_to_num(got[k])) == bits(np.nan_to_num(exp[k])), (what, k)
    assert got["rounded"].tolist() == exp["rounded"].tolist() and got["accepted_key"].tolist() == exp["accepted_key"].tolist(), what


@pytest.mark.parametrize("name", case_names())
def test_fixture_cases_equal_golden(name):
    c = case(name)
    undefined_peaks, raw, pct, info = _device_v3(_v3_args(c))
    same_dict(raw, c["updated_boc_raw"], name)
    assert all(type(v) is int for v in raw.values())
    same_dict(pct, c["updated_boc_percent"], name)
    same_peaks(undefined_peaks, c["undefined_peaks"], name)
    assert (info["stop_reason"], info["n_passes"], info["accepted_keys"]) == (c["stop"], c["passes"], c["accepted"])


@pytest.mark.parametrize("n,multidrop", [(1, True), (2, True), (63, True), (64, True), (65, False), (HEAD_THREADS - 1, True),
                                         (HEAD_THREADS + 1, False), (TILE - 1, True), (TILE + 1, True), (1100, True)])
def test_sizes_against_restatement(n, multidrop):
    """Around the trial workgroup (64 trials), the head workgroup (256 lanes) and the LDS tile of the base sum (1 024 counts)."""
    args = tiny_problem(n) if n < 3 else problem(n, 100 + n, include_multidrop=multidrop)
    assert len(args[0]) == n or not multidrop
    r = _check_against_restatement(args, n)
    assert n < 100 or (r["accepted"] and r["undefined_peaks"])


def test_trial_counts_around_the_trial_workgroup():
    """63, 64, 65 and 130 trials in the first pass: every key is planted far above its controls."""
    for trials in (TRIAL_THREADS - 1, TRIAL_THREADS, TRIAL_THREADS + 1, 2 * TRIAL_THREADS + 2):
        boc, pct, avg, std, C, sigma, md = problem(trials, 7, peaks=0, undefined=0)
        avg = {k: v * (0.5 if i % 2 else 0.6) for i, (k, v) in enumerate(avg.items())}
        std = {k: 1e-4 for k in std}
        args = (boc, pct, avg, std, C, 0.5, md)
        assert len(avg) == trials
        r = R.iterate(*args, max_iterations=40)
        from fluorosequencingimageanalysis_amd import background as BG
        prob = BG.pack_problem(*args)
        z0 = R.z_of(pct[next(iter(avg))], avg[next(iter(avg))], 1e-4)
        assert z0 > 0.5 and r["passes"] >= 2
        (got,) = _records([prob], max_iterations=40, accepted_cap=64)
        (exp,) = BG.background_records([prob], max_iterations=40, accepted_cap=64, device=None)
        _same_records(got, exp, trials)
        assert [prob["keys"][i] for i in got["accepted_key"]] == r["accepted"] and got["n_passes"] == r["passes"]


@pytest.mark.parametrize("where", ["first", "last"])
def test_single_trial_at_the_ends_of_the_order(where):
    boc, pct, avg, std, C, sigma, md = problem(150, 11, peaks=0, undefined=0)
    k = list(boc)[0 if where == "first" else -1]
    boc[k] *= 3
    from fluorosequencingimageanalysis_amd import background as BG
    avg, pct = dict(pct), BG.counts_to_percent(boc)                # (the controls are the experiment before the peak)
    std = {q: 0.05 * v for q, v in avg.items()}
    r = _check_against_restatement((boc, pct, avg, std, C, 30.0, md), where)
    assert r["accepted"][0] == k
    z = [R.z_of(pct[q], avg[q], std[q]) for q in avg]
    assert sum(1 for v in z if not v <= 30.0) == 1                 # one trial in the first pass


def test_equal_scores_and_equal_differences_first_in_order_decides():
    boc = {key(1): 10, key(2): 100, key(3): 10, key(4): 100, key(5): 10}
    total = float(sum(boc.values()))
    pct = {k: v / total for k, v in boc.items()}
    for first, second in ((2, 4), (4, 2)):
        order = [key(first), key(second), key(1), key(3), key(5)]
        avg = {k: (0.1 if k in (key(2), key(4)) else pct[k]) for k in order}
        std = {k: 0.01 for k in order}
        r = _check_against_restatement((boc, pct, avg, std, 5, 2.0, True), first)
        assert r["accepted"][:2] == [key(first), key(second)]
        assert R.z_of(pct[key(2)], 0.1, 0.01) == R.z_of(pct[key(4)], 0.1, 0.01)


def test_batch_of_five_equals_each_alone_and_the_host():
    from fluorosequencingimageanalysis_amd import background as BG
    two_ac = case("two_ac")
    assert two_ac["passes"] > 4 * 16                               # more passes than one host batch
    many = [BG.pack_problem(*_v3_args(two_ac)),
            BG.pack_problem(*problem(300, 21)),
            BG.pack_problem(*problem(40, 22, sigma=1e6)),          # stops in its first pass
            BG.pack_problem(*tiny_problem(2)),
            BG.pack_problem(*_v3_args(case("one_ac")))]
    kw = dict(accepted_cap=2048, undefined_cap=4096)
    batch = _records(many, **kw)
    assert batch[2]["n_passes"] == 1 and batch[2]["stop_reason"] == R.STOP_THRESHOLD and batch[0]["stop_reason"] == R.STOP_CONVERGED
    assert batch[4]["stop_reason"] == R.STOP_NO_DEFINED and len(batch[4]["count"]) > len(two_ac["boc_experiment"])
    for p, prob in enumerate(many):
        (alone,) = _records([prob], **kw)
        _same_records(batch[p], alone, p)
        (host,) = BG.background_records([prob], device=None, **kw)
        _same_records(batch[p], host, p)
        assert batch[p]["overflow"] == 0


def test_max_iterations_and_history_overflow():
    from fluorosequencingimageanalysis_amd import _native_background as NB, background as BG
    c = case("two_ac")
    prob = BG.pack_problem(*_v3_args(c))
    for cap in (0, 3, 16, 17, 40):
        (got,) = _records([prob], max_iterations=cap, accepted_cap=64, undefined_cap=64)
        (exp,) = BG.background_records([prob], max_iterations=cap, accepted_cap=64, undefined_cap=64, device=None)
        _same_records(got, exp, cap)
        assert got["stop_reason"] == NB.MAX_ITERATIONS and got["n_passes"] == cap
        assert [prob["keys"][i] for i in got["accepted_key"]] == c["accepted"][:cap]
    with pytest.raises(RuntimeError, match="max_iterations"):
        BG.iterative_peak_finding_v3(*_v3_args(c), device="cuda", max_iterations=5)
    (full,) = _records([prob], accepted_cap=2048, undefined_cap=2048)
    (small,) = _records([prob], accepted_cap=2, undefined_cap=3)
    assert full["overflow"] == 0 and small["overflow"] == NB.OVERFLOW_ACCEPTED | NB.OVERFLOW_UNDEFINED
    assert small["accepted_key"].tolist() == full["accepted_key"][:2].tolist()
    assert bits(small["undefined_bp"]) == bits(full["undefined_bp"][:3])
    for k in ("count", "percent"):
        assert bits(small[k]) == bits(full[k])
    assert (small["rounded"].tolist(), small["stop_reason"], small["n_passes"], small["n_accepted"]) == \
        (full["rounded"].tolist(), full["stop_reason"], full["n_passes"], full["n_accepted"])
    (none,) = _records([prob], accepted_cap=0, undefined_cap=0)      # no history at all: undefined_bp is NULL
    assert none["overflow"] == NB.OVERFLOW_ACCEPTED and bits(none["count"]) == bits(full["count"])


def test_device_tensors_are_checked():
    import torch
    from fluorosequencingimageanalysis_amd import background as BG
    prob = BG.pack_problem(*tiny_problem(2))
    a, max_defined = BG.concatenate_problems([prob])
    tensors = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).cuda() for k, v in a.items()}
    out = BG.background_device(dict(tensors), max_defined, int(a["nb_off"][-1]))
    assert int(out["stop_reason"][0]) == R.STOP_THRESHOLD and out["count"].data_ptr() == tensors["count"].data_ptr()
    for name, bad in (("count", tensors["count"].float()), ("def_key", tensors["def_key"].long()), ("key_off", tensors["key_off"][:1]),
                      ("filter", tensors["filter"][:1]), ("percent", tensors["percent"].cpu())):
        with pytest.raises(ValueError):
            BG.background_device(dict(tensors, **{name: bad}), max_defined, int(a["nb_off"][-1]))
    with pytest.raises(ValueError):
        BG.background_device(dict(tensors), max_defined + 5, int(a["nb_off"][-1]))
    assert BG.background_records([], device="cuda") == []


def test_command_line_equals_its_host_route_file_by_file(tmp_path):
    from fluorosequencingimageanalysis_amd import iterative_background_v2 as CL
    from test_background_host import _argv, _write_inputs
    for name in ("three_ac_no_multidrop", "eight_cycles"):
        c = case(name)
        work = tmp_path / name
        work.mkdir()
        boc_path, csv_path = _write_inputs(work, c)
        host = _argv(c, boc_path, csv_path, str(work / "host"))
        gpu = [a for a in _argv(c, boc_path, csv_path, str(work / "gpu")) if a != "--host"]
        CL.main(host, timestamp_epoch=1500000000)
        with _prefilled():
            res = CL.main(gpu, timestamp_epoch=1500000000, device="cuda")
        names = sorted(os.listdir(str(work / "host")))
        assert names == sorted(os.listdir(str(work / "gpu"))) and len(names) == 4
        for f in names:
            assert open(str(work / "host" / f), "rb").read() == open(str(work / "gpu" / f), "rb").read(), f
        same_dict(res["updated_boc_raw"], c["updated_boc_raw"])
