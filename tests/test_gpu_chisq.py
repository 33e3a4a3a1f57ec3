"""Chi-squared step fitter, plateau merge filters and R^2 on the GPU (include/fsq_chisq.h): bit for bit against the
reference's recorded outputs (tests/golden/chisq_traces.npz) and, for random batches, against the NumPy restatement
(tests/_chisq_reference.py).  Nothing is compared with a tolerance."""
import numpy as np
import pytest

import _chisq_reference as R
from _chisq_cases import BATCH_PARAMS, filter_cases, fit_cases, random_batch
from _util import _bits, same_plateaus

pytestmark = pytest.mark.gpu

FIT_CAP = 64


def _fit_batch(traces, num_steps, mult, L, mag, ignore, max_frames=None, lens=None, fit_cap=FIT_CAP, fill=None):
    """fsq_chisq_step_fit through chisq_device on host rows; returns host arrays.  `lens` overrides the row lengths (to hand
    the device lengths a Python list cannot have); `fill` pre-fills every output with a pattern."""
    import torch
    from fluorosequencingimageanalysis_amd import stepfitting as S
    mf = max_frames or max(max(len(t) for t in traces), 1)
    rows = np.zeros((len(traces), mf))
    for i, t in enumerate(traces):
        rows[i, :min(len(t), mf)] = np.asarray(t, dtype=np.float64)[:mf]
    ln = np.array([len(t) for t in traces] if lens is None else lens, dtype=np.int32)
    if fill is None:
        out = S.chisq_device(torch.from_numpy(rows).cuda(), torch.from_numpy(ln).cuda(), mult, num_steps, L, mag, ignore, fit_cap)
    else:
        real = torch.zeros

        def filled(*a, **k):
            t = real(*a, **k)
            return t.fill_(fill) if t.is_cuda else t
        torch.zeros = filled
        try:
            out = S.chisq_device(torch.from_numpy(rows).cuda(), torch.from_numpy(ln).cuda(), mult, num_steps, L, mag, ignore, fit_cap)
        finally:
            torch.zeros = real
    return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}


def _check_row(h, t, fit, recs, what):
    assert h["status"][t] == 0, what
    k = int(h["count"][t])
    same_plateaus(list(zip(h["start"][t, :k], h["stop"][t, :k], h["height"][t, :k])), fit, what)
    nf = int(h["n_fits"][t])
    assert nf == len(recs), what
    m = min(nf, h["S"].shape[1])
    assert np.array_equal(_bits(h["best_res"][t, :m]), _bits([r[0] for r in recs[:m]])), what
    assert np.array_equal(_bits(h["counter_res"][t, :m]), _bits([r[1] for r in recs[:m]])), what
    assert h["counter_n"][t, :m].tolist() == [int(r[2]) for r in recs[:m]], what
    assert np.array_equal(_bits(h["S"][t, :m]), _bits([r[3] for r in recs[:m]])), what


def test_golden_through_c_abi():
    """Every recorded case: boundaries, heights, residual sums, S and counter-fit counts, bit for bit."""
    for i, c in enumerate(fit_cases()):
        h = _fit_batch([c["lum"]], c["num_steps"], c["mult"], c["L"], c["mag"], c["ignore"])
        recs = list(zip(c["best"], c["counter"], c["counter_n"], c["S"]))
        assert len(recs) <= FIT_CAP
        _check_row(h, 0, c["fit"], recs, (i, c["name"]))


def test_golden_in_one_launch_per_parameter_set():
    """The same cases batched: traces of different lengths side by side in one launch give what they give alone."""
    cases = fit_cases()
    groups = {}
    for i, c in enumerate(cases):
        groups.setdefault((c["num_steps"], c["mult"], c["L"], c["mag"], c["ignore"]), []).append(i)
    for key, idx in groups.items():
        if key[0] is not None and any(not key[0] < len(cases[i]["lum"]) for i in idx):
            continue
        h = _fit_batch([cases[i]["lum"] for i in idx], *key)
        for t, i in enumerate(idx):
            c = cases[i]
            _check_row(h, t, c["fit"], list(zip(c["best"], c["counter"], c["counter_n"], c["S"])), i)


def test_random_ragged_batch_equals_restatement():
    traces = random_batch(20240, 3000)
    n_par = len(BATCH_PARAMS)
    for k, (ns, mult, L, mag, ign) in enumerate(BATCH_PARAMS):
        sub = [t for j, t in enumerate(traces) if j % n_par == k and (ns is None or ns < len(t) - 1)]
        assert len(sub) > 300
        h = _fit_batch(sub, ns, mult, L, mag, ign)
        assert (h["status"] == 0).all()
        for t, v in enumerate(sub):
            fit, recs = R.chi_squared(v.tolist(), mult, ns, L, mag, ign)
            _check_row(h, t, fit, recs, (k, t, len(v)))


def test_limits_and_invalid_rows():
    """1023 and 1024 frames next to a 1025-frame row and rows of length 0 and -3 in one launch: the invalid rows get status 2
    and keep their outputs, their neighbours are bit-identical to a launch without them."""
    cases = {len(c["lum"]): c for c in fit_cases() if len(c["lum"]) in (1023, 1024, 200)}
    a, b, s = cases[1023], cases[1024], cases[200]
    assert (a["num_steps"], a["L"]) == (b["num_steps"], b["L"]) == (3, 2)
    long_row = np.concatenate([b["lum"], [1.0]])
    traces = [a["lum"], long_row, b["lum"], s["lum"], s["lum"], a["lum"][:300]]
    lens = [1023, 1025, 1024, 0, -3, 300]
    FILL = -77
    h = _fit_batch(traces, 3, 1, 2, 0.0, False, max_frames=1025, lens=lens, fill=FILL)
    assert h["status"].tolist() == [0, 2, 0, 2, 2, 0]
    for t in (1, 3, 4):
        for k in ("start", "stop", "height", "count", "n_fits", "best_res", "counter_res", "S", "counter_n"):
            assert (h[k][t] == FILL).all(), (t, k)
    clean = _fit_batch([a["lum"], b["lum"], a["lum"][:300]], 3, 1, 2, 0.0, False, max_frames=1025, fill=FILL)
    for t_all, t_clean in ((0, 0), (2, 1), (5, 2)):
        for k in ("start", "stop", "count", "n_fits", "counter_n"):
            assert np.array_equal(h[k][t_all], clean[k][t_clean]), (t_all, k)
        for k in ("height", "best_res", "counter_res", "S"):
            assert np.array_equal(_bits(h[k][t_all]), _bits(clean[k][t_clean])), (t_all, k)
    for t, c in ((0, a), (2, b)):
        _check_row(h, t, c["fit"], list(zip(c["best"], c["counter"], c["counter_n"], c["S"])), t)
    # an explicit num_steps outside 0 < num_steps < len is invalid per trace; a full-length fit is where the reference raises
    h = _fit_batch([[1.0, 5.0, 2.0, 7.0], [1.0, 5.0, 2.0], [3.0, 9.0]], 3, 1, 2, 0.0, False)
    assert h["status"].tolist() == [0, 2, 2]
    h = _fit_batch([[1.0, 5.0, 2.0]], 2, 1, 0, 0.0, False)
    assert h["status"].tolist() == [1]
    h = _fit_batch([[4.0], [4.0, 6.0]], None, 1, 2, 0.0, False, max_frames=2)
    assert h["status"].tolist() == [2, 0] and h["count"][1] == 1 and h["height"][1, 0] == 5.0


def _rows_of(cases, mf):
    n = len(cases)
    lum, ln = np.zeros((n, mf)), np.zeros(n, np.int32)
    st, so, hh, cn = np.zeros((n, mf), np.int32), np.zeros((n, mf), np.int32), np.zeros((n, mf)), np.zeros(n, np.int32)
    for i, c in enumerate(cases):
        ln[i] = len(c["lum"]); lum[i, :ln[i]] = c["lum"]
        cn[i] = len(c["pin"])
        st[i, :cn[i]] = [p[0] for p in c["pin"]]; so[i, :cn[i]] = [p[1] for p in c["pin"]]; hh[i, :cn[i]] = [p[2] for p in c["pin"]]
    return lum, ln, st, so, hh, cn


def test_merge_filter_and_r_squared_golden():
    """Both modes and every has_ combination, batched per criterion set in one launch."""
    import torch
    from fluorosequencingimageanalysis_amd import stepfitting as S
    cases = filter_cases()
    combos = {(c["mode"], c["mag"] is not None, c["ratio"] is not None) for c in cases}
    assert combos == {(0, False, False), (1, False, False), (1, True, False), (1, False, True), (1, True, True)}
    groups = {}
    for c in cases:
        groups.setdefault((c["mode"], c["mag"], c["ratio"]), []).append(c)
    for (mode, mag, ratio), grp in groups.items():
        mf = max(len(c["lum"]) for c in grp)
        d = [torch.from_numpy(x).cuda() for x in _rows_of(grp, mf)]
        out = {k: v.cpu().numpy() for k, v in S.merge_filter_device(*d, mode, mag, ratio).items()}
        r2 = {k: v.cpu().numpy() for k, v in S.r_squared_device(*d).items()}
        assert (out["status"] == 0).all() and (r2["status"] == 0).all()
        for i, c in enumerate(grp):
            k = int(out["count"][i])
            same_plateaus(list(zip(out["start"][i, :k], out["stop"][i, :k], out["height"][i, :k])), c["pout"], (mode, mag, ratio, i))
            assert np.array_equal(_bits(r2["r2"][i:i + 1]), _bits([c["r2"]])), (mode, mag, ratio, i)


def test_merge_filter_and_r_squared_random_equals_restatement():
    import torch
    from fluorosequencingimageanalysis_amd import stepfitting as S
    rng = np.random.default_rng(99)
    traces = random_batch(777, 600)
    cases = []
    for v in traces:
        n = len(v)
        cuts = np.sort(rng.choice(np.arange(1, n), int(rng.integers(0, min(n - 1, 12) + 1)), replace=False)).tolist()
        lo = int(rng.integers(0, 2)) if n > 3 and cuts and cuts[0] > 1 else 0          # (some lists start after frame 0)
        bounds = [lo] + cuts + [n]
        pin = []
        for a, b in zip(bounds[:-1], bounds[1:]):
            h = float(np.mean(v[a:b])) if rng.random() < 0.8 else float(np.round(rng.normal(np.mean(v[a:b]), 2000.0)))
            pin.append((a, b - 1, h))
        cases.append(dict(lum=v, pin=pin))
    mf = max(len(v) for v in traces)
    d = [torch.from_numpy(x).cuda() for x in _rows_of(cases, mf)]
    r2 = S.r_squared_device(*d)["r2"].cpu().numpy()
    exp = np.array([R.r_squared(c["lum"].tolist(), c["pin"]) for c in cases])
    assert np.array_equal(_bits(r2), _bits(exp))
    for mode, mag, ratio in ((0, None, None), (1, None, None), (1, 6000.0, None), (1, None, 0.4), (1, 3000.0, 0.25), (1, 0.0, 0.0)):
        out = {k: v.cpu().numpy() for k, v in S.merge_filter_device(*d, mode, mag, ratio).items()}
        assert (out["status"] == 0).all()
        for i, c in enumerate(cases):
            lum = c["lum"].tolist()
            e = R.filter_upsteps(lum, c["pin"]) if mode == 0 else R.filter_small_steps(lum, c["pin"], mag, ratio)
            k = int(out["count"][i])
            same_plateaus(list(zip(out["start"][i, :k], out["stop"][i, :k], out["height"][i, :k])), e, (mode, mag, ratio, i))
    # invalid plateau rows: status 2, neighbours untouched by them
    lum, ln, st, so, hh, cn = _rows_of(cases[:4], mf)
    so[1, 0] += 1                                                  # overlaps / leaves a gap
    cn[2] = 0
    d2 = [torch.from_numpy(x).cuda() for x in (lum, ln, st, so, hh, cn)]
    out = {k: v.cpu().numpy() for k, v in S.merge_filter_device(*d2, 0).items()}
    assert out["status"].tolist()[1:3] == [2, 2] and out["status"][0] == 0 and out["status"][3] == 0
    assert S.r_squared_device(*d2)["status"].cpu().numpy().tolist()[1:3] == [2, 2]


def test_drop_ins_return_the_reference_shapes():
    from fluorosequencingimageanalysis_amd import stepfitting as S
    c = [x for x in fit_cases() if x["name"] == "n200"][1]
    lum = c["lum"].tolist()
    fit = S.chi_squared_step_fitter(lum, num_steps=c["num_steps"], min_step_length=c["L"])
    assert isinstance(fit, list) and all(isinstance(p, tuple) and len(p) == 3 for p in fit)
    assert all(type(p[0]) is int and type(p[1]) is int and isinstance(p[2], float) for p in fit)
    same_plateaus(fit, c["fit"])
    rec = S.chisq_records([lum, lum[:50]], num_steps=c["num_steps"], min_step_length=c["L"], fit_cap=16)
    assert rec["counts"].tolist()[0] == len(c["fit"]) and rec["n_fits"][0] == len(c["best"])
    assert np.array_equal(_bits(rec["S"][0, :len(c["S"])]), _bits(c["S"]))
    for f in filter_cases()[:10]:
        lum = f["lum"].tolist()
        got = S.filter_upsteps(lum, f["pin"]) if f["mode"] == 0 else S.filter_small_steps(lum, f["pin"], f["mag"], f["ratio"])
        assert all(type(p[0]) is int and type(p[1]) is int and isinstance(p[2], float) for p in got)
        same_plateaus(got, f["pout"])
        r2 = S.stepfit_r_squared(lum, f["pin"])
        assert isinstance(r2, float) and np.array_equal(_bits([r2]), _bits([f["r2"]]))
    with pytest.raises(ValueError, match="is greater than len"):
        S.chi_squared_step_fitter([1.0, 5.0, 2.0], num_steps=2, min_step_length=0)
    assert S.chi_squared_step_fitter([1.0, 3.0]) == [(0, 1, 2.0)]
