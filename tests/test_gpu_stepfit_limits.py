"""The step-fit kernels at their documented limits (include/fsq_stepfit.h): traces of 8191 / 8192 mirrored frames, p over the
whole (t, df) plane, window_radius 64, 16 CK windows, M = 1 and 64, the two sort paths of the t-filter with tied and NaN p,
and FSQ_STEPFIT_INVALID rows next to valid ones.  The inputs come from tests/_limits_cases.py; tests/test_limits_host.py
checks the same inputs against the restatement alone.

Expected values: the reference's records (tests/golden/stepfit_limits.npz) for the long traces, the restatement
(tests/_stepfit_reference.py) bit for bit elsewhere, scipy.stats.ttest_ind and mpmath (50 digits) for p, at the project's
bar of 1e-10 relative.

Measured on the MI355X (largest relative deviation of the device's p; the tests print the figures of every run):
    p sweep, 6000 points, df 1 - 8190, |t| 1e-9 - 1e4:  5.58e-13 against scipy, 5.58e-13 against mpmath (2000 points);
                                                         35 points with a true p below 1e-300 compared absolutely
    sliding-window p, window_radius 64 (33 593 finite p): 7.22e-14;  window_radius 7 (3 755 finite p): 1.11e-14
"""
import ctypes
import math

import numpy as np
import pytest

import _limits_cases as LC
import _stepfit_reference as R
from _util import _bits, same_plateaus
from test_limits_host import param_limit_expected
from test_stepfit_host import check_pair_p

pytestmark = pytest.mark.gpu

INVALID = 2
SENT_I, SENT_F = -777, -777.25


def _rows(traces, max_frames=None):
    lens = np.array([len(t) for t in traces], np.int32)
    rows = np.zeros((len(traces), max_frames or int(lens.max())))
    for i, t in enumerate(traces):
        rows[i, :len(t)] = t
    return rows, lens


def _launch(rows, lens, prm, want_p=False, pair_cap=0):
    """fsq_stepfit_traces through the C ABI with every output pre-filled with a sentinel -> host arrays."""
    import torch
    from fluorosequencingimageanalysis_amd import _native as N
    from fluorosequencingimageanalysis_amd import _native_stepfit as NS
    n, mf = rows.shape
    L = NS.lib()
    ws_bytes = L.fsq_stepfit_workspace_bytes(n, mf, ctypes.byref(prm))
    assert ws_bytes > 0
    Lmax = mf + min(prm.mirror_start, mf)
    nr = max(prm.window_radius - 5, 0)

    def full(shape, dt):
        return torch.full(shape, SENT_F if dt == torch.float64 else SENT_I, dtype=dt, device="cuda")
    o = {"ck": full((n, mf), torch.float64), "status": full((n,), torch.int32)}
    for pre in ("pl", "tf"):
        o[pre + "_start"], o[pre + "_stop"] = full((n, mf), torch.int32), full((n, mf), torch.int32)
        o[pre + "_h"], o[pre + "_n"] = full((n, mf), torch.float64), full((n,), torch.int32)
    if want_p:
        o["p"] = full((n, nr, Lmax), torch.float64)
    if pair_cap:
        o["pair_p"], o["pair_n"] = full((n, pair_cap), torch.float64), full((n,), torch.int32)
    ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device="cuda")
    d_phot, d_len = torch.from_numpy(rows).cuda(), torch.from_numpy(lens).cuda()
    rc = L.fsq_stepfit_traces(d_phot.data_ptr(), d_len.data_ptr(), n, mf, ctypes.byref(prm), o["ck"].data_ptr(),
                              o["pl_start"].data_ptr(), o["pl_stop"].data_ptr(), o["pl_h"].data_ptr(), o["pl_n"].data_ptr(),
                              o["tf_start"].data_ptr(), o["tf_stop"].data_ptr(), o["tf_h"].data_ptr(), o["tf_n"].data_ptr(),
                              o["status"].data_ptr(), o["p"].data_ptr() if want_p else None,
                              o["pair_p"].data_ptr() if pair_cap else None, o["pair_n"].data_ptr() if pair_cap else None,
                              int(pair_cap), ws.data_ptr(), int(ws_bytes), torch.cuda.current_stream().cuda_stream)
    N.check(rc, "fsq_stepfit_traces")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _plateaus(h, pre, j):
    k = int(h[pre + "_n"][j])
    return list(zip(h[pre + "_start"][j, :k], h[pre + "_stop"][j, :k], h[pre + "_h"][j, :k]))


def _tfilter_batch(lums, plateaus, thr, drop_sort, nms, pair_cap=0, max_frames=None):
    """fsq_stepfit_ttest_filter for many traces in one launch -> host arrays (s, o, h, n, st, pair_p, pair_n)."""
    import torch
    from fluorosequencingimageanalysis_amd import _native as N
    from fluorosequencingimageanalysis_amd import _native_stepfit as NS
    n = len(lums)
    rows, lens = _rows(lums, max_frames)
    mf = rows.shape[1]
    kmax = max(len(p) for p in plateaus)
    st, so, hh = np.zeros((n, kmax), np.int32), np.zeros((n, kmax), np.int32), np.zeros((n, kmax))
    for i, pl in enumerate(plateaus):
        st[i, :len(pl)], so[i, :len(pl)], hh[i, :len(pl)] = [a for a, _, _ in pl], [o for _, o, _ in pl], [h for _, _, h in pl]
    d_s, d_o = (torch.zeros((n, mf), dtype=torch.int32, device="cuda") for _ in range(2))
    d_h = torch.zeros((n, mf), dtype=torch.float64, device="cuda")
    d_s[:, :kmax], d_o[:, :kmax], d_h[:, :kmax] = torch.from_numpy(st).cuda(), torch.from_numpy(so).cuda(), torch.from_numpy(hh).cuda()
    d_n = torch.from_numpy(np.array([len(p) for p in plateaus], np.int32)).cuda()
    out = {"s": torch.full((n, mf), SENT_I, dtype=torch.int32, device="cuda"),
           "o": torch.full((n, mf), SENT_I, dtype=torch.int32, device="cuda"),
           "h": torch.full((n, mf), SENT_F, dtype=torch.float64, device="cuda"),
           "n": torch.full((n,), SENT_I, dtype=torch.int32, device="cuda"),
           "st": torch.full((n,), SENT_I, dtype=torch.int32, device="cuda")}
    if pair_cap:
        out["pair_p"] = torch.full((n, pair_cap), SENT_F, dtype=torch.float64, device="cuda")
        out["pair_n"] = torch.full((n,), SENT_I, dtype=torch.int32, device="cuda")
    L = NS.lib()
    ws_bytes = L.fsq_stepfit_ttest_filter_workspace_bytes(n, mf)
    assert ws_bytes > 0
    ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device="cuda")
    d_lum, d_len = torch.from_numpy(rows).cuda(), torch.from_numpy(lens).cuda()
    rc = L.fsq_stepfit_ttest_filter(d_lum.data_ptr(), d_len.data_ptr(), n, mf, d_s.data_ptr(), d_o.data_ptr(), d_h.data_ptr(),
                                    d_n.data_ptr(), float(thr), 1 if drop_sort else 0, int(nms), out["s"].data_ptr(),
                                    out["o"].data_ptr(), out["h"].data_ptr(), out["n"].data_ptr(), out["st"].data_ptr(),
                                    out["pair_p"].data_ptr() if pair_cap else None, out["pair_n"].data_ptr() if pair_cap else None,
                                    int(pair_cap), ws.data_ptr(), int(ws_bytes), torch.cuda.current_stream().cuda_stream)
    N.check(rc, "fsq_stepfit_ttest_filter")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- A1 ------------------------------------------------------------------------------------------------------------------------
def test_length_limits_equal_reference_records():
    """8188 / 8189 frames with mirror 3 and 8192 frames with mirror 0 (8191 and 8192 mirrored frames), with and without CK,
    drop_sort on and off, one case whose t-filter starts with more than 64 pairs: CK values, plateau bounds and heights bit
    for bit against the reference's records, every pair p within 1e-10 of scipy's.  With mirror 3 the same launch holds a row
    of 8190 frames (8193 mirrored): FSQ_STEPFIT_INVALID, outputs untouched."""
    from fluorosequencingimageanalysis_amd import stepfitting as S
    for i, c in enumerate(LC.length_limit_cases()):
        prm = S._params(c["mirror"], c["ck"], c["thr"], None, drop_sort=c["drop_sort"])
        n = len(c["phot"])
        extra = c["mirror"] > 0
        traces = [c["phot"]] + ([np.resize(c["phot"], 8193 - c["mirror"])] if extra else [])      # 8193 mirrored frames
        rows, lens = _rows(traces)
        cap = max(len(c["p_pairs"]), 1)
        h = _launch(rows, lens, prm, pair_cap=cap)
        assert h["status"][0] == 0, i
        if c["ck"]:
            assert np.array_equal(_bits(h["ck"][0, :n]), _bits(c["ck_out"])), i
        else:
            assert np.array_equal(_bits(h["ck"][0, :n]), _bits(c["phot"])), i
        same_plateaus(_plateaus(h, "pl", 0), c["pl"])
        same_plateaus(_plateaus(h, "tf", 0), c["tf"])
        k = int(h["pair_n"][0])
        assert k >= 1
        check_pair_p(h["pair_p"][0, :k], c["p_pairs"])
        if extra:
            assert int(lens[1]) + c["mirror"] == 8193
            assert h["status"][1] == INVALID and h["pl_n"][1] == 0 and h["tf_n"][1] == 0 and h["pair_n"][1] == 0, i
            assert (h["ck"][1] == SENT_F).all() and (h["tf_h"][1] == SENT_F).all() and (h["pl_start"][1] == SENT_I).all(), i


def test_long_merges_pin_the_pairwise_recursion():
    """48 traces of 7689 - 8192 frames whose two plateaus merge: the height is np.mean of all frames, whose bits depend on the
    depth of the pairwise recursion for about a fifth of them (test_limits_host.py counts them).  Through the t-filter entry,
    one launch; the full path runs the same traces as one plateau each (window_radius 0 finds no step)."""
    from fluorosequencingimageanalysis_amd import stepfitting as S
    cases = LC.long_merge_cases()
    out = _tfilter_batch([c[0] for c in cases], [c[1] for c in cases], 0.01, True, 0, max_frames=8192)
    for j, (lum, pl) in enumerate(cases):
        assert out["st"][j] == 0 and out["n"][j] == 1, j
        assert (out["s"][j, 0], out["o"][j, 0]) == (0, len(lum) - 1), j
        assert _bits([out["h"][j, 0]])[0] == _bits([np.mean(lum)])[0], j
    rows, lens = _rows([c[0] for c in cases], 8192)
    h = _launch(rows, lens, S._params(0, 0, 0.01, None, window_radius=0))
    for j, (lum, pl) in enumerate(cases):
        assert h["status"][j] == 0 and h["pl_n"][j] == 1 and h["tf_n"][j] == 1, j
        assert _bits([h["pl_h"][j, 0]])[0] == _bits([h["tf_h"][j, 0]])[0] == _bits([np.mean(lum)])[0], j


# ---- A2 ------------------------------------------------------------------------------------------------------------------------
def _rel_dev(got, exp):
    """Largest relative deviation over the points with exp >= P_TINY; the others must lie in [0, 1e-299]."""
    tiny = exp < LC.P_TINY
    assert ((got[tiny] >= 0) & (got[tiny] <= 1e-299)).all()
    rel = np.abs(got[~tiny] - exp[~tiny]) / exp[~tiny]
    return float(rel.max()), int(tiny.sum())


def test_p_sweep_against_scipy_and_mpmath(capsys):
    """6000 two-plateau traces through fsq_stepfit_ttest_filter (pair_cap 1), bucketed by length into four launches: the
    device's p of every pair against scipy.stats.ttest_ind(equal_var=False) and, on 2000 of them, against mpmath at 50
    digits: 1e-10 relative.  Points whose true p is below 1e-300 (at most 5 %, test_limits_host.py) must give 0 <= p <= 1e-299."""
    pts = LC.p_sweep()
    exp, t, df = LC.sweep_scipy(pts)
    got = np.full(len(pts), np.nan)
    size = np.array([len(a) + len(b) for a, b in pts])
    for lo, hi in ((0, 64), (64, 512), (512, 2048), (2048, 8192)):
        idx = np.flatnonzero((size > lo) & (size <= hi))
        assert len(idx) > 100
        lums = [np.concatenate(pts[i]) for i in idx]
        pls = [[(0, len(pts[i][0]) - 1, 0.0), (len(pts[i][0]), size[i] - 1, 0.0)] for i in idx]
        out = _tfilter_batch(lums, pls, 2.0, True, 0, pair_cap=1, max_frames=hi)        # threshold 2: nothing merges
        assert (out["st"] == 0).all() and (out["pair_n"] == 1).all() and (out["n"] == 2).all()
        got[idx] = out["pair_p"][:, 0]
    assert np.isfinite(got).all()
    dev_scipy, n_tiny = _rel_dev(got, exp)
    sub = LC.mp_subsample(len(pts))
    mp = np.array([LC.mp_p(t[i], df[i]) for i in sub])
    dev_mp, _ = _rel_dev(got[sub], mp)
    with capsys.disabled():
        print("\n[p sweep] largest relative deviation of the device's p: %.3g against scipy (%d points, %d below 1e-300), "
              "%.3g against mpmath (%d points)" % (dev_scipy, len(pts), n_tiny, dev_mp, len(sub)))
    assert n_tiny <= LC.MAX_TINY_SHARE * len(pts)
    assert dev_scipy <= 1e-10 and dev_mp <= 1e-10


def test_p_special_cases_are_exact():
    """A one-frame plateau: NaN.  Two constant plateaus: p == 0 where the values differ, NaN where they are equal.  Equal
    means (t == 0): p == 1."""
    cases = [([5.0, 1.0, 2.0, 4.0], 1, lambda p: math.isnan(p)), ([1.0, 2.0, 4.0, 5.0], 3, lambda p: math.isnan(p)),
             ([3.0] * 4 + [7.0] * 5, 4, lambda p: p == 0.0), ([3.0] * 4 + [3.0] * 5, 4, lambda p: math.isnan(p)),
             ([1.0, 2.0, 3.0, 1.0, 2.0, 3.0], 3, lambda p: p == 1.0), ([1.0, 3.0, 0.0, 2.0, 4.0], 2, lambda p: p == 1.0),
             ([3.0] * 4000 + [7.0] * 4192, 4000, lambda p: p == 0.0)]
    lums = [np.array(c[0]) for c in cases]
    pls = [[(0, c[1] - 1, 0.0), (c[1], len(c[0]) - 1, 0.0)] for c in cases]
    for ds in (True, False):
        out = _tfilter_batch(lums, pls, 2.0, ds, 0, pair_cap=2)
        assert (out["st"] == 0).all() and (out["pair_n"] == 1).all()
        for j, c in enumerate(cases):
            assert c[2](float(out["pair_p"][j, 0])), (j, out["pair_p"][j, 0])
            assert out["pair_p"][j, 1] == SENT_F


@pytest.mark.parametrize("wr", [64, 7])
def test_sliding_window_p_against_scipy(wr, capsys):
    """want_p at window_radius 64 (59 radii) and 7 on ragged random traces: every finite p within 1e-10 of scipy's, NaN where
    scipy gives NaN (empty or one-frame windows)."""
    from fluorosequencingimageanalysis_amd import stepfitting as S
    traces = LC.sliding_p_traces(wr)
    rows, lens = _rows(traces)
    h = _launch(rows, lens, S._params(0, 0, 0.01, None, window_radius=wr), want_p=True)
    worst, n_fin = 0.0, 0
    exps = LC.sliding_p_scipy(traces, wr)
    for j, tr in enumerate(traces):
        exp = exps[j]
        got = h["p"][j][:, :len(tr)]
        assert np.array_equal(np.isnan(got), np.isnan(exp)), j
        assert (h["p"][j][:, len(tr):] == SENT_F).all(), j
        assert np.array_equal(got == 0, exp == 0), j
        f = np.isfinite(exp) & (exp != 0)
        n_fin += int(f.sum())
        if f.any():
            worst = max(worst, float((np.abs(got[f] - exp[f]) / exp[f]).max()))
    with capsys.disabled():
        print("\n[sliding p, window_radius %d] %d finite p, largest relative deviation %.3g" % (wr, n_fin, worst))
    assert n_fin > (20000 if wr == 64 else 1500)
    assert worst <= 1e-10


# ---- A3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s[0] for s in LC.PARAM_LIMIT_SETS])
def test_parameter_limits_equal_restatement(name):
    """window_radius 64; 16 CK windows from 1 to 64 frames with M = 64 and M = 1; ragged traces that include 3, 4, 64, 65, 127,
    128 and 129 frames: CK values, plateaus and heights bit for bit.  At most a tenth of the traces is `near` (none of the
    boundary lengths; test_limits_host.py)."""
    from fluorosequencingimageanalysis_amd import stepfitting as S
    (_, seed, mirror, ck, wr, ds, wl, M), = [s for s in LC.PARAM_LIMIT_SETS if s[0] == name]
    traces, exp = param_limit_expected(name)
    prm = S._params(mirror, ck, 0.01, None, window_radius=wr, drop_sort=ds, window_lengths=wl, M=M)
    rows, lens = _rows(traces)
    h = _launch(rows, lens, prm)
    assert (h["status"] == 0).all()
    checked = 0
    for j, e in enumerate(exp):
        if e is None:
            continue
        ckf, pl, tf = e
        assert np.array_equal(_bits(h["ck"][j, :len(ckf)]), _bits(ckf)), j
        same_plateaus(_plateaus(h, "pl", j), pl)
        same_plateaus(_plateaus(h, "tf", j), tf)
        checked += 1
    assert checked >= (1.0 - LC.MAX_SKIPPED_SHARE) * len(traces)


# ---- A4 ------------------------------------------------------------------------------------------------------------------------
def test_sort_paths_with_ties_and_nan():
    """63, 64, 65, 400 and 700 pairs in the first pass with exactly tied p (the stable merge sort from 64 pairs on, CPython's
    insertion sort below), and NaN mixed with finite p below 64 pairs: plateaus and heights bit for bit through the C ABI
    (all cases in one launch per drop_sort) and through stepfitting.t_test_filter.  Nothing is skipped."""
    from fluorosequencingimageanalysis_amd import stepfitting as S
    cases = LC.sort_cases()
    names = sorted(cases)
    for nms in sorted(set(c[2] for c in cases.values())):
        group = [k for k in names if cases[k][2] == nms]
        for ds in (True, False):
            cap = 4096
            out = _tfilter_batch([cases[k][0] for k in group], [cases[k][1] for k in group], LC.SORT_THR, ds, nms, pair_cap=cap)
            for j, k in enumerate(group):
                lum, pl, _, tied = cases[k]
                fl = R.Flags()
                exp = R.t_test_filter(lum, pl, LC.SORT_THR, drop_sort=ds, no_merge_start=nms, flags=fl)
                assert not fl.near and not fl.unsupported and out["st"][j] == 0, k
                m = int(out["n"][j])
                same_plateaus(list(zip(out["s"][j, :m], out["o"][j, :m], out["h"][j, :m])), exp)
                assert (out["h"][j, m:] == SENT_F).all(), k
                q = min(int(out["pair_n"][j]), cap)
                assert int(out["pair_n"][j]) == len(fl.p_pairs), k
                check_pair_p(out["pair_p"][j, :q], fl.p_pairs[:q])
                same_plateaus(S.t_test_filter(lum.tolist(), pl, LC.SORT_THR, drop_sort=ds, no_merge_start=nms), exp)


# ---- A5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ck", [0, 1])
def test_invalid_rows_leave_their_neighbours_alone(ck):
    """Rows of length 0, -5, max_frames + 1 and (CK on) 1 frame (2 mirrored) between valid rows, through
    stepfitting.run_device (which checks no length) and through the C ABI with sentinel-filled outputs: status
    FSQ_STEPFIT_INVALID, counts 0, output rows untouched, and every valid row equal to the launch without the invalid ones."""
    import torch
    from fluorosequencingimageanalysis_amd import stepfitting as S
    rng = np.random.default_rng(50 + ck)
    valid = LC.random_traces(rng, [3, 200, 64, 129, 7, 300, 300])
    mf = 300
    bad_lens = [0, -5, mf + 1, -2 ** 31] + ([1] if ck else [])
    rows_v, lens_v = _rows(valid, mf)
    order = []                                                     # interleave: v b v b ...
    for i in range(len(valid)):
        order.append(("v", i))
        if i < len(bad_lens):
            order.append(("b", i))
    rows = np.stack([rows_v[i] if kind == "v" else rng.normal(1e4, 3e3, mf) for kind, i in order])
    lens = np.array([lens_v[i] if kind == "v" else bad_lens[i] for kind, i in order], np.int32)
    prm = S._params(1, ck, 0.01, None)
    clean = _launch(rows_v, lens_v, prm, want_p=True, pair_cap=8)
    mixed = _launch(rows, lens, prm, want_p=True, pair_cap=8)
    dev = S.run_device(torch.from_numpy(rows).cuda(), torch.from_numpy(lens).cuda(), mf, prm, pair_cap=8)
    dev = {k: v.cpu().numpy() for k, v in dev.items() if not k.startswith("_")}
    assert (clean["status"] == 0).all()
    for j, (kind, i) in enumerate(order):
        if kind == "b":
            for h in (mixed, dev):
                assert h["status"][j] == INVALID and h["pl_n"][j] == 0 and h["tf_n"][j] == 0 and h["pair_n"][j] == 0, j
            for k in ("ck", "pl_h", "tf_h", "pair_p"):
                assert (mixed[k][j] == SENT_F).all(), (j, k)
            for k in ("pl_start", "pl_stop", "tf_start", "tf_stop"):
                assert (mixed[k][j] == SENT_I).all(), (j, k)
            assert (mixed["p"][j] == SENT_F).all(), j
        else:
            for k in clean:                                        # sentinels included: the same cells are written
                assert np.array_equal(mixed[k][j].view(np.uint8 if mixed[k].dtype.kind != "f" else np.uint64).reshape(-1),
                                      clean[k][i].view(np.uint8 if clean[k].dtype.kind != "f" else np.uint64).reshape(-1)) \
                    if mixed[k].ndim > 1 else mixed[k][j] == clean[k][i], (j, k)
            n = int(lens[j])
            assert np.array_equal(_bits(dev["ck"][j, :n]), _bits(clean["ck"][i, :n])), j
            for pre in ("pl", "tf"):
                same_plateaus(_plateaus(dev, pre, j), _plateaus(clean, pre, i))
