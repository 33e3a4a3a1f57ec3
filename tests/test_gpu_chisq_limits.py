"""The chi-squared step fitter, the merge filters and R^2 at their limits and at scale (include/fsq_chisq.h), through the C
ABI with every output pre-filled with a sentinel.  Inputs: tests/_chisq_limit_cases.py (tests/test_chisq_limits_host.py
proves that they reach the paths named here).  Expected values: the restatement (tests/_chisq_reference.py) and the
reference's records (tests/golden/chisq_limits.npz).  Every comparison is bit for bit; a NaN is compared by the bits of the
x86 one.

  A  3 x 8192 + 101 two-frame traces [x, -x]: glibc's pow(x, 2.0) over the whole double range, three block-stride trips
  B  2 x 8192 + 777 ragged rows of 3 - 60 frames on a dirty workspace and a non-default stream, invalid rows among them
  C  traces scaled by 1e-165 .. 1e154, on 2^52 and 1e15 offsets, with -0.0 and +0.0 levels
  D  129 - 1 024 frames with up to 129 plateaus, more fits than fit_cap
  E  merge filter and R^2 on rows of 8 191 and 8 192 frames
  F  FSQ_STEPFIT_UNSUPPORTED rows and every FSQ_EINVAL return

The restatement's CPU time for group D is 6 s on the host (2.7 s as this module's fixture on the MI355X box).  Measured
durations on the MI355X (--durations): pow sweep 2.9 s, block stride 1.7 s and 0.7 s, long traces 2.1 s (+ 2.7 s fixture),
merge filter 0.1 - 0.5 s per configuration, every other test below 0.1 s.
"""
import ctypes

import numpy as np
import pytest

import _chisq_limit_cases as CL
import _chisq_reference as R
from _util import _bits, same_plateaus

pytestmark = pytest.mark.gpu

SENT_I, SENT_F = -777, -777.25
INVALID, UNSUPPORTED = 2, 1


def _prm(num_steps, mult, L, mag, ign):
    from fluorosequencingimageanalysis_amd import _native_chisq as NC
    p = NC.FsqChisqParams()
    p.num_steps, p.min_step_length, p.ignore_counterfits = num_steps or 0, L, 1 if ign else 0
    p.num_steps_multiplier, p.min_step_magnitude = float(mult), float(mag)
    return p


def _rows(traces, max_frames=None):
    lens = np.array([len(t) for t in traces], np.int32)
    rows = np.zeros((len(traces), max_frames or int(lens.max())))
    for i, t in enumerate(traces):
        rows[i, :len(t)] = t
    return rows, lens


def _launch(rows, lens, params, fit_cap=CL.FIT_CAP, optional=True, stream=None, dirty_ws=False, expect_rc=0, mutate=None):
    """fsq_chisq_step_fit through the C ABI with every output pre-filled with a sentinel -> (rc, host arrays).  `mutate`
    edits the argument list before the call (the FSQ_EINVAL cases)."""
    import torch
    from fluorosequencingimageanalysis_amd import _native_chisq as NC
    n, mf = rows.shape
    L = NC.lib()
    ws_bytes = int(L.fsq_chisq_workspace_bytes(n, mf))
    assert ws_bytes > 0
    prm = params if isinstance(params, ctypes.Structure) else _prm(*params)
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
        def full(shape, dt):
            return torch.full(shape, SENT_F if dt == torch.float64 else SENT_I, dtype=dt, device="cuda")
        o = {"start": full((n, mf), torch.int32), "stop": full((n, mf), torch.int32), "height": full((n, mf), torch.float64),
             "count": full((n,), torch.int32), "n_fits": full((n,), torch.int32), "status": full((n,), torch.int32)}
        cap = max(fit_cap, 1)
        o.update(best_res=full((n, cap), torch.float64), counter_res=full((n, cap), torch.float64),
                 counter_n=full((n, cap), torch.int32), S=full((n, cap), torch.float64))
        ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device="cuda") if dirty_ws else \
            torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        d_lum, d_len = torch.from_numpy(rows).cuda(), torch.from_numpy(lens).cuda()
        s = torch.cuda.current_stream()
        opt = [o[k].data_ptr() if optional else None for k in ("best_res", "counter_res", "counter_n", "S")]
        args = [d_lum.data_ptr(), d_len.data_ptr(), n, mf, ctypes.byref(prm), o["start"].data_ptr(), o["stop"].data_ptr(),
                o["height"].data_ptr(), o["count"].data_ptr(), o["n_fits"].data_ptr()] + opt + \
               [int(fit_cap), o["status"].data_ptr(), ws.data_ptr(), ws_bytes, s.cuda_stream]
        if mutate:
            mutate(args)
        rc = L.fsq_chisq_step_fit(*args)
        s.synchronize()
    assert rc == expect_rc
    return {k: v.cpu().numpy() for k, v in o.items()}


def _untouched(h, t=None):
    for k, v in h.items():
        row = v if t is None else v[t]
        assert (row == (SENT_F if v.dtype.kind == "f" else SENT_I)).all(), (t, k)


def _check_row(h, t, fit, recs, what, optional=True):
    """Row t equals (fit, records): plateaus, counts, the records below fit_cap, and sentinels everywhere else."""
    assert h["status"][t] == 0, what
    k = int(h["count"][t])
    same_plateaus(list(zip(h["start"][t, :k], h["stop"][t, :k], h["height"][t, :k])), fit, what)
    assert (h["start"][t, k:] == SENT_I).all() and (h["stop"][t, k:] == SENT_I).all() and (h["height"][t, k:] == SENT_F).all(), what
    assert int(h["n_fits"][t]) == len(recs), what
    m = min(len(recs), h["S"].shape[1]) if optional else 0
    assert np.array_equal(_bits(h["best_res"][t, :m]), _bits([r[0] for r in recs[:m]])), what
    assert np.array_equal(_bits(h["counter_res"][t, :m]), _bits([r[1] for r in recs[:m]])), what
    assert h["counter_n"][t, :m].tolist() == [int(r[2]) for r in recs[:m]], what
    assert np.array_equal(_bits(h["S"][t, :m]), CL.nan_to_x86([r[3] for r in recs[:m]])), what
    for key in ("best_res", "counter_res", "S"):
        assert (h[key][t, m:] == SENT_F).all(), (what, key)
    assert (h["counter_n"][t, m:] == SENT_I).all(), what


def _same_bytes(a, b):
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# ---- A ---------------------------------------------------------------------------------------------------------------------
def test_pow_sweep_in_three_block_stride_trips():
    x, _ = CL.pow_sweep()
    res, S = CL.sweep_expected(x)
    rows = np.stack([x, -x], axis=1)
    h = _launch(rows, np.full(len(x), 2, np.int32), (None, 1, 2, 0.0, False), fit_cap=2)
    assert (h["status"] == 0).all() and (h["count"] == 1).all() and (h["n_fits"] == 1).all()
    assert np.array_equal(_bits(h["best_res"][:, 0]), _bits(res))
    assert np.array_equal(_bits(h["counter_res"][:, 0]), _bits(res))
    assert (h["counter_n"][:, 0] == 1).all() and np.array_equal(_bits(h["S"][:, 0]), S)
    assert (h["start"][:, 0] == 0).all() and (h["stop"][:, 0] == 1).all() and (_bits(h["height"][:, 0]) == 0).all()
    assert (h["start"][:, 1] == SENT_I).all() and (h["height"][:, 1] == SENT_F).all() and (h["S"][:, 1] == SENT_F).all()


# ---- B ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(CL.STRIDE_PARAMS)))
def test_block_stride_on_ragged_rows(k):
    """Long traces followed by short ones in the same block and the reverse, invalid rows between the trips, 0xFF bytes in
    the workspace, a stream of its own; and the same rows in chunks of one trip give identical bytes."""
    import torch
    pool = CL.stride_pool()
    idx, lens = CL.stride_rows()
    exp = CL.stride_expected(k)
    mf = max(len(v) for v in pool)
    rows = _rows(pool, mf)[0][idx]
    stream = torch.cuda.Stream()
    h = _launch(rows, lens, CL.STRIDE_PARAMS[k], stream=stream, dirty_ws=True)
    true_len = np.array([len(pool[i]) for i in idx])
    for t in range(len(idx)):
        if lens[t] != true_len[t]:
            assert h["status"][t] == INVALID, t
            _untouched({key: v for key, v in h.items() if key != "status"}, t)
        else:
            _check_row(h, t, exp[idx[t]][0], exp[idx[t]][1], (k, t, int(idx[t])))
    parts = [_launch(rows[a:a + CL.MAX_BLOCKS], lens[a:a + CL.MAX_BLOCKS], CL.STRIDE_PARAMS[k]) for a in range(0, len(idx), CL.MAX_BLOCKS)]
    _same_bytes(h, {key: np.concatenate([p[key] for p in parts]) for key in h})


# ---- C ---------------------------------------------------------------------------------------------------------------------
def test_extreme_scales_equal_reference_records():
    """Subnormal residual sums, sums that are all inf (one fit, S the x86 NaN), luminosities on 2^52 and 1e15, -0.0 levels:
    one launch per num_steps, every row against the reference's record and the restatement."""
    gold = {(g["name"], g["num_steps"]): g for g in CL.golden()}
    for ns in (5, None):
        cases = [c for c in CL.extreme_cases() if c[2] == ns]
        rows, lens = _rows([c[1] for c in cases])
        h = _launch(rows, lens, (ns, 1, 2, 0.0, False))
        for t, (name, v, _) in enumerate(cases):
            g = gold[(name, ns)]
            assert np.array_equal(_bits(g["lum"]), _bits(v))
            _check_row(h, t, g["fit"], list(zip(g["best"], g["counter"], g["counter_n"], g["S"])), (name, ns))
            with np.errstate(all="ignore"):
                fit, recs = R.chi_squared(v.tolist(), 1, ns, 2)
            _check_row(h, t, fit, recs, (name, ns))


# ---- D ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_expected():
    return {c[0]: R.chi_squared(CL.long_trace(c).tolist(), c[5], c[4], c[6]) for c in CL.LONG_CASES}


def test_long_traces_with_many_plateaus(long_expected):
    """More than 64 list nodes in the best fit and in the counter-fit, refits of 129 - 1 023 frames, n_fits > fit_cap: n_fits
    reports the full count, the first fit_cap columns equal the records and nothing past them is written (the row's tail and
    the row after it, an invalid one, keep their sentinels).  With the four optional pointers NULL the fits are identical."""
    groups = {}
    for c in CL.LONG_CASES:
        groups.setdefault(c[4:], []).append(c)
    over_cap = 0
    for (ns, mult, L), grp in groups.items():
        traces = []
        for c in grp:
            traces += [CL.long_trace(c), np.zeros(3)]
        rows, lens = _rows(traces, 1024)
        lens[1::2] = 0                                              # the row after each long one is invalid: all sentinels
        h = _launch(rows, lens, (ns, mult, L, 0.0, False))
        bare = _launch(rows, lens, (ns, mult, L, 0.0, False), optional=False)
        for j, c in enumerate(grp):
            fit, recs = long_expected[c[0]]
            over_cap += len(recs) > CL.FIT_CAP
            _check_row(h, 2 * j, fit, recs, c[0])
            _check_row(bare, 2 * j, fit, recs, c[0], optional=False)
            for hh in (h, bare):
                assert hh["status"][2 * j + 1] == INVALID
                _untouched({key: v for key, v in hh.items() if key != "status"}, 2 * j + 1)
    assert over_cap >= 4
    gold = {g["name"]: g for g in CL.golden()}
    for c in CL.LONG_CASES:                                         # the full sizes the reference finished
        if c[0] in gold:
            g = gold[c[0]]
            same_plateaus(long_expected[c[0]][0], g["fit"], c[0])


def test_reduced_long_cases_equal_reference_records():
    gold = {g["name"]: g for g in CL.golden()}
    for c in CL.LONG_CASES_RECORDED:
        g = gold[c[0]]
        rows, lens = _rows([g["lum"]])
        h = _launch(rows, lens, (c[4], c[5], c[6], 0.0, False))
        _check_row(h, 0, g["fit"], list(zip(g["best"], g["counter"], g["counter_n"], g["S"])), c[0])


# ---- E ---------------------------------------------------------------------------------------------------------------------
def _filter_rows(cases, mf):
    n = len(cases)
    lum, ln = np.zeros((n, mf)), np.zeros(n, np.int32)
    st, so, hh, cn = np.zeros((n, mf), np.int32), np.zeros((n, mf), np.int32), np.zeros((n, mf)), np.zeros(n, np.int32)
    for i, c in enumerate(cases):
        ln[i] = len(c["lum"]); lum[i, :ln[i]] = c["lum"]
        cn[i] = len(c["pin"])
        st[i, :cn[i]] = [p[0] for p in c["pin"]]; so[i, :cn[i]] = [p[1] for p in c["pin"]]; hh[i, :cn[i]] = [p[2] for p in c["pin"]]
    return lum, ln, st, so, hh, cn


def _filter_launch(arrs, mode, mag, ratio):
    import torch
    from fluorosequencingimageanalysis_amd import _native_chisq as NC
    d = [torch.from_numpy(a).cuda() for a in arrs]
    n, mf = arrs[0].shape
    o = {"start": torch.full((n, mf), SENT_I, dtype=torch.int32, device="cuda"),
         "stop": torch.full((n, mf), SENT_I, dtype=torch.int32, device="cuda"),
         "height": torch.full((n, mf), SENT_F, dtype=torch.float64, device="cuda"),
         "count": torch.full((n,), SENT_I, dtype=torch.int32, device="cuda"),
         "status": torch.full((n,), SENT_I, dtype=torch.int32, device="cuda"),
         "r2": torch.full((n,), SENT_F, dtype=torch.float64, device="cuda"),
         "r2_status": torch.full((n,), SENT_I, dtype=torch.int32, device="cuda")}
    L = NC.lib()
    s = torch.cuda.current_stream().cuda_stream
    rc = L.fsq_stepfit_merge_filter(d[0].data_ptr(), d[1].data_ptr(), n, mf, d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                                    d[5].data_ptr(), int(mode), int(mag is not None), float(mag or 0.0), int(ratio is not None),
                                    float(ratio or 0.0), o["start"].data_ptr(), o["stop"].data_ptr(), o["height"].data_ptr(),
                                    o["count"].data_ptr(), o["status"].data_ptr(), None, 0, s)
    assert rc == 0
    rc = L.fsq_stepfit_r_squared(d[0].data_ptr(), d[1].data_ptr(), n, mf, d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                                 d[5].data_ptr(), o["r2"].data_ptr(), o["r2_status"].data_ptr(), None, 0, s)
    assert rc == 0
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


@pytest.mark.parametrize("cfg", range(len(CL.FILTER_CONFIGS)))
def test_merge_filter_and_r_squared_at_8192_frames(cfg):
    """Rows of 8 191 and 8 192 frames beside short ones: thousands of single-frame plateaus, merges that refit 3 100 - 8 192
    frames (the deep levels of the pairwise sum), R^2 of the same lists and of a flat row (the x86 NaN); a row that claims
    8 193 frames is refused and keeps its sentinels."""
    mode, mag, ratio = CL.FILTER_CONFIGS[cfg]
    cases = CL.filter_limit_cases()
    arrs = _filter_rows(cases + [cases[-1]], CL.FILTER_FRAMES)
    bad = len(cases)
    arrs[1][bad] = CL.FILTER_FRAMES + 1
    h = _filter_launch(arrs, mode, mag, ratio)
    exp = CL.filter_expected(cases, mode, mag, ratio)
    for i, c in enumerate(cases):
        assert h["status"][i] == 0 and h["r2_status"][i] == 0, i
        k = int(h["count"][i])
        same_plateaus(list(zip(h["start"][i, :k], h["stop"][i, :k], h["height"][i, :k])), exp[i], (cfg, i))
        assert (h["stop"][i, k:] == SENT_I).all(), i              # (start and height rows are the filter's working rows)
        with np.errstate(all="ignore"):
            r2 = R.r_squared(c["lum"].tolist(), c["pin"])
        assert _bits([h["r2"][i]])[0] == CL.nan_to_x86([r2])[0], (cfg, i)
    assert h["status"][bad] == INVALID and h["r2_status"][bad] == INVALID
    assert (h["start"][bad] == SENT_I).all() and (h["stop"][bad] == SENT_I).all() and (h["height"][bad] == SENT_F).all()
    assert h["r2"][bad] == SENT_F and h["count"][bad] == 0         # (a refused row's count is 0, as in the t-test filter)


# ---- F ---------------------------------------------------------------------------------------------------------------------
def test_unsupported_rows_keep_their_fit_rows():
    for lum, ns in CL.UNSUPPORTED_CASES:
        recs = CL.records_until_raise(lum, ns)
        rows, lens = _rows([lum, [4.0] * len(lum)])
        h = _launch(rows, lens, (ns, 1, 0, 0.0, False))
        assert h["status"].tolist() == [UNSUPPORTED, 0]
        _untouched({k: h[k] for k in ("start", "stop", "height", "count", "n_fits")}, 0)
        m = len(recs)
        assert np.array_equal(_bits(h["best_res"][0, :m]), _bits([r[0] for r in recs]))
        assert np.array_equal(_bits(h["counter_res"][0, :m]), _bits([r[1] for r in recs]))
        assert h["counter_n"][0, :m].tolist() == [r[2] for r in recs]
        assert np.array_equal(_bits(h["S"][0, :m]), CL.nan_to_x86([r[3] for r in recs]))
        assert (h["S"][0, m:] == SENT_F).all() and (h["counter_n"][0, m:] == SENT_I).all()
        fit, frecs = R.chi_squared([4.0] * len(lum), 1, ns, 0)
        assert len(frecs) == 1
        _check_row(h, 1, fit, frecs, "flat")


def test_einval_returns_launch_nothing():
    from fluorosequencingimageanalysis_amd import _native as N
    from fluorosequencingimageanalysis_amd import _native_chisq as NC
    einval = N.FSQ_EINVAL
    rows, lens = _rows([[1.0, 5.0, 2.0, 7.0, 3.0]])
    good = (None, 1, 2, 0.0, False)
    _launch(rows, lens, good)                                       # (the same call is accepted unmutated)

    def refused(params=good, mutate=None, fit_cap=4):
        _untouched(_launch(rows, lens, params, fit_cap=fit_cap, expect_rc=einval, mutate=mutate))

    def setter(i, v):
        def f(args):
            args[i] = v
        return f
    refused(mutate=setter(4, None))                                 # NULL prm
    for i in (0, 1, 5, 6, 7, 8, 9, 15, 16):                         # a NULL required pointer
        refused(mutate=setter(i, None))
    for keep in ((10,), (10, 11), (10, 11, 12), (13,), (11, 13)):   # 1 - 3 of the 4 optional pointers

        def some(args, keep=keep):
            for i in (10, 11, 12, 13):
                if i not in keep:
                    args[i] = None
        refused(mutate=some)

    def short(args):
        args[17] -= 1
    refused(mutate=short)                                           # ws_bytes one byte short
    for mult in (0.0, 1.5, float("nan")):
        refused(params=(None, mult, 2, 0.0, False))
    refused(params=(None, 1, 2, float("nan"), False))
    refused(fit_cap=-1)
    refused(params=(-1, 1, 2, 0.0, False))
    refused(mutate=setter(3, 0))                                    # max_frames = 0
    L = NC.lib()
    prm = _prm(*good)
    z = [None] * 9
    assert L.fsq_chisq_step_fit(None, None, 0, 5, ctypes.byref(prm), *z, 0, None, None, 0, None) == 0       # n_traces = 0
    # the filter entries
    assert L.fsq_stepfit_merge_filter_workspace_bytes(4, 8193) == -1 and L.fsq_stepfit_r_squared_workspace_bytes(4, 8193) == -1
    f = [None] * 4
    o = [None] * 5
    assert L.fsq_stepfit_merge_filter(None, None, 0, 8, *f, 0, 0, 0.0, 0, 0.0, *o, None, 0, None) == 0
    assert L.fsq_stepfit_r_squared(None, None, 0, 8, *f, None, None, None, 0, None) == 0
    assert L.fsq_stepfit_merge_filter(None, None, 0, 8193, *f, 0, 0, 0.0, 0, 0.0, *o, None, 0, None) == einval
    assert L.fsq_stepfit_r_squared(None, None, 0, 8193, *f, None, None, None, 0, None) == einval
    assert L.fsq_stepfit_merge_filter(None, None, 0, 8, *f, 2, 0, 0.0, 0, 0.0, *o, None, 0, None) == einval           # mode 2
    for bad in (-1.0, float("nan")):
        assert L.fsq_stepfit_merge_filter(None, None, 0, 8, *f, 1, 1, bad, 0, 0.0, *o, None, 0, None) == einval
        assert L.fsq_stepfit_merge_filter(None, None, 0, 8, *f, 1, 0, 0.0, 1, bad, *o, None, 0, None) == einval
        assert L.fsq_stepfit_merge_filter(None, None, 0, 8, *f, 1, 0, bad, 0, bad, *o, None, 0, None) == 0           # flags clear
    assert L.fsq_stepfit_merge_filter(None, None, 3, 8, *f, 0, 0, 0.0, 0, 0.0, *o, None, 0, None) == einval           # NULL buffers
    assert L.fsq_stepfit_r_squared(None, None, 3, 8, *f, None, None, None, 0, None) == einval


def test_chisq_records_raises_for_the_first_offending_trace():
    from fluorosequencingimageanalysis_amd import stepfitting as S
    ok = [1.0, 5.0, 2.0, 7.0, 3.0, 9.0]
    with pytest.raises(ValueError, match=r"num_steps has an invalid value of 4 vs len\(luminosity_sequence\) = 4"):
        S.chisq_records([ok, ok[:4], ok[:2]], num_steps=4)
    with pytest.raises(IndexError, match="list index out of range"):
        S.chisq_records([ok, [3.0], []])
    with pytest.raises(ValueError, match=r"num_plateaus = 4 is greater than len\(luminosities\) = 3"):
        S.chisq_records([ok, [1.0, 5.0, 2.0], [7.0, 1.0, 3.0, 9.0]], num_steps=2, min_step_length=0)
