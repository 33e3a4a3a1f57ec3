"""GPU tests (-m gpu) of the single-precision PSF solver (FSQ_MODE_TEXTBOOK_F32, csrc/fsq_fit_f32.h) at its limits, against float64
references.  Inputs: tests/_f32_limit_cases.py; host twin (which proves that the inputs reach their edges and measures the
restatement's constants used here): tests/test_f32_limits_host.py; DESIGN 4.9, "Limits that tests stand on".

  a  f32_eval through fsq_selftest_f32_eval against a float64 evaluation of the same formulas on E, in batches of 1, 63, 64, 65
     and all 4 157: |N - N64| <= c 2^-24 sum m_a m_b, |g - g64| <= c 2^-24 sum m_a m_r, |chi2 - chi2_64| <= c 2^-24 chi2_64 with the
     cancellation-free magnitudes m of _f32_limit_cases.eval_reference and c = 16 x (1, 3, 6), sixteen times what the float32
     restatement reaches (never taken from the kernel's own error)
  b  the solver on S against the fp64 oracle, all seven parameters: share within 1e-3 >= the restatement's - 0.03, share with
     float64 chi2 <= (1 + 1e-4) x the oracle's >= 0.99, median of niter <= the restatement's + 2, 99th percentile <= + 6, no exit 5
  c  lane refill: 2 x 12 x 64 x CUs + 65 fits of 257 distinct ROIs into a row buffer of 0xFF bytes, every row byte for byte the
     row of the same ROI from a stand-alone batch of the 257; batches of 0, 1, 63, 64, 65
  d  B, S, the exit-code ROIs and the textbook fixtures: every parameter a float32 value inside the box, the named parameter of a
     bound case exactly on its bound, exit codes in {1, 2, 4, 5} and each reached where the restatement reaches it, rmse / r2 / h0
     / w0 of the row bit for bit the oracle's fp64 metrics of the row's own parameters, flat ROIs fitted to 1e-3 (value + 1)"""
import ctypes

import numpy as np
import pytest

import _f32_limit_cases as C
from _util import TEXTBOOK_NAMES, bits_equal, load_field, rois_of

pytestmark = pytest.mark.gpu
PARAMS = ("H", "A", "p2", "p3", "sigma_h", "sigma_w", "theta")
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def env():
    import torch
    from fluorosequencingimageanalysis_amd import _native
    import oracle as O
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    O.build()
    return torch, _native, O


def params_of(rows):
    return np.stack([rows[k] for k in PARAMS], axis=1)


def fit_device(torch, N, rois, n=None):
    """fsq_fit_rois in the single-precision mode into a row buffer of 0xFF bytes -> the device tensor uint8 [n + 1, 128]; the row
    behind the last one is a guard that must stay 0xFF"""
    rois = np.ascontiguousarray(rois, dtype=np.uint16).reshape(-1, 25)
    n = len(rois) if n is None else n
    d = torch.from_numpy(rois.view(np.int16)).cuda() if len(rois) else torch.zeros(25, dtype=torch.int16, device="cuda")
    rows = torch.full((n + 1, 128), 255, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(max(int(N.lib().fsq_fit_workspace_bytes(n)), 8), dtype=torch.uint8, device="cuda")
    N.check(N.lib().fsq_fit_rois(d.data_ptr(), n, N.MODE_TEXTBOOK_F32, rows.data_ptr(), ws.data_ptr(), ws.numel(),
                                 torch.cuda.current_stream().cuda_stream), "fsq_fit_rois")
    torch.cuda.synchronize()
    assert bool((rows[n] == 255).all()), "a row behind the batch was written"
    return rows


def fit_rows(torch, N, rois):
    return fit_device(torch, N, rois)[:-1].cpu().numpy().view(N.ROW_DTYPE).reshape(-1)


def eval_device(torch, N, x, rois):
    """fsq_selftest_f32_eval -> (chi2 [n], N [n, 28], g [n, 7]) float32; the outputs are allocated 64 entries longer, filled with
    0xFF bytes, and the surplus must stay as it was"""
    n = len(x)
    dx = torch.from_numpy(np.ascontiguousarray(x, dtype=f32).reshape(-1)).cuda() if n else torch.zeros(7, device="cuda")
    dr = torch.from_numpy(np.ascontiguousarray(rois, dtype=np.uint16).reshape(-1).view(np.int16)).cuda() if n else torch.zeros(25, dtype=torch.int16, device="cuda")
    out = [torch.full(((n + 64) * k * 4,), 255, dtype=torch.uint8, device="cuda") for k in (1, 28, 7)]
    N.check(N.lib().fsq_selftest_f32_eval(dx.data_ptr(), dr.data_ptr(), n, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                          torch.cuda.current_stream().cuda_stream), "fsq_selftest_f32_eval")
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in out]
    for h, k in zip(host, (1, 28, 7)):
        assert (h[n * k * 4:] == 255).all(), "written behind the last point"
    return tuple(h[:n * k * 4].view(f32).reshape((n, k) if k > 1 else (n,)) for h, k in zip(host, (1, 28, 7)))


# ---- a ------------------------------------------------------------------------------------------------------------------------
def test_f32_eval_against_float64(env):
    torch, N, O = env
    x, rois = C.eval_points()
    ref = C.eval_reference(x, rois)
    chi2, Nn, g = eval_device(torch, N, x, rois)
    eN, eg, ec = C.eval_units(chi2, Nn, g, ref)
    c = {k: C.KERNEL_FACTOR * v for k, v in C.RESTATEMENT_UNITS.items()}
    print("f32_eval on E in units of 2^-24 x magnitudes: N %.3f (allowed %g), g %.3f (%g), chi2 %.3f (%g)"
          % (eN.max(), c["N"], eg.max(), c["g"], ec.max(), c["chi2"]))
    assert np.isfinite(chi2).all() and np.isfinite(Nn).all() and np.isfinite(g).all()
    assert eN.max() <= c["N"], (eN.max(), int(eN.argmax()), x[eN.argmax()])
    assert eg.max() <= c["g"], (eg.max(), int(eg.argmax()), x[eg.argmax()])
    assert ec.max() <= c["chi2"], (ec.max(), int(ec.argmax()), x[ec.argmax()])
    # every LDS column, a partial block, one lane: a point's result does not depend on the lane that evaluates it
    for k, b in enumerate(C.BATCHES + (0,)):
        at = 37 * (k + 1)
        cb, Nb, gb = eval_device(torch, N, x[at:at + b], rois[at:at + b])
        assert cb.shape == (b,) and Nb.shape == (b, 28) and gb.shape == (b, 7)
        assert np.array_equal(cb.view(np.uint32), chi2[at:at + b].view(np.uint32)), b
        assert np.array_equal(Nb.view(np.uint32), Nn[at:at + b].view(np.uint32)), b
        assert np.array_equal(gb.view(np.uint32), g[at:at + b].view(np.uint32)), b


# ---- b ------------------------------------------------------------------------------------------------------------------------
def test_solver_on_conditioned_spots_against_the_fp64_oracle(env):
    torch, N, O = env
    truth, rois = C.spots()
    ref = O.fit_rois(rois, mode=1, n_threads=16)["p"]
    xr, sr, nr, _ = C.restatement_on_spots()
    base = C.solver_figures(xr, nr, sr, ref, rois)
    rows = fit_rows(torch, N, rois)
    fig = C.solver_figures(params_of(rows), rows["niter"], rows["status"], ref, rois)
    print("S (%d spots), all seven parameters against the fp64 oracle:\n   kernel      %s\n   restatement %s" % (len(rois), fig, base))
    assert C.spot_conditions(base, base) == []
    assert C.spot_conditions(fig, base) == [], (fig, base)


# ---- c ------------------------------------------------------------------------------------------------------------------------
def test_lane_refill(env):
    torch, N, O = env
    rois = C.refill_rois()
    alone = fit_device(torch, N, rois)[:-1]
    host = alone.cpu().numpy().view(N.ROW_DTYPE).reshape(-1)
    assert np.isin(host["status"], (1, 2, 4, 5)).all() and np.isfinite(params_of(host)).all()
    assert not bool((alone == 255).all(dim=1).any())
    assert host["niter"].min() <= 4 and host["niter"].max() >= 50                  # short and long fits side by side
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = C.refill_count(cus)
    assert n > 2 * 12 * 64 * cus and n % 64 == 1
    idx = np.arange(n) % C.N_REFILL
    rows = fit_device(torch, N, rois[idx])[:-1]
    want = alone[torch.from_numpy(idx).cuda()]
    same = (rows == want).all(dim=1)
    assert bool(same.all()), "%d of %d refilled rows differ from the stand-alone rows, the first at %d" % (
        int((~same).sum()), n, int(torch.nonzero(~same)[0]))
    lanes = {int(i) % 64 for i in np.flatnonzero(idx == 0)}                        # (257 is coprime to 64)
    assert len(lanes) == 64
    for b in (0, 1, 63, 64, 65):
        small = fit_device(torch, N, rois[:b])
        assert small.shape == (b + 1, 128) and bool((small[:b] == alone[:b]).all()), b


# ---- d ------------------------------------------------------------------------------------------------------------------------
def check_rows(N, O, rows, rois, what):
    """what holds for every row of the single-precision solver"""
    p = params_of(rows)
    assert np.isfinite(p).all(), what
    assert np.array_equal(p.astype(f32).astype(f64), p), what                     # o.x[k] = (double) x[k]
    floor = C.amplitude_floor(rois)
    assert (p[:, 0] >= 0).all() and (p[:, 1] >= floor).all(), what
    assert ((p[:, 2:4] >= 2) & (p[:, 2:4] <= 3)).all() and ((p[:, 4:6] >= 0.75) & (p[:, 4:6] <= 2)).all(), what
    assert ((p[:, 6] >= 0) & (p[:, 6] <= 360)).all(), what
    assert np.isin(rows["status"], (1, 2, 4, 5)).all() and (rows["niter"] >= 1).all() and (rows["nfev"] >= rows["niter"] + 1).all(), what
    assert (rows["niter"] <= 200).all() and (rows["nfev"] <= 401).all(), what
    exp = np.zeros(1, O.ROW_DTYPE)                  # the oracle's metrics (its model, pflib.py:461-473) of the row's own parameters
    for i in range(len(rows)):                      # kfinish is the fp64 path's: bit for bit
        roi = np.ascontiguousarray(rois[i].astype(np.int64))
        pi = np.ascontiguousarray(p[i])
        O.lib().fsq_o_fit_metrics(roi.ctypes.data_as(ctypes.c_void_p), pi.ctypes.data_as(ctypes.c_void_p), 2, 2,
                                  exp.ctypes.data_as(ctypes.c_void_p))
        for k in ("h0", "w0", "rmse", "r2"):
            assert bits_equal(rows[k][i], exp[k][0]).all(), (what, k, i, rows[k][i], exp[k][0])
    return p


def test_bound_cases_end_on_their_bounds(env):
    torch, N, O = env
    cases, rois = C.bound_cases(), C.bound_rois()
    rows = fit_rows(torch, N, rois)
    p = check_rows(N, O, rows, rois, "B")
    floor = C.amplitude_floor(rois)
    missed = [(name, k, p[i, k]) for i, (name, _, k, bound) in enumerate(cases)
              if k is not None and p[i, k] != (floor[i] if bound is None else bound)]
    assert not missed, missed
    flat = np.flatnonzero((rois == rois[:, :1]).all(1))
    assert len(flat) >= 3 and {0, 1, 65535} <= set(rois[flat, 0].tolist())
    assert (rows["rmse"][flat] <= 1e-3 * (rois[flat, 0].astype(f64) + 1)).all(), (rois[flat, 0], rows["rmse"][flat])


def test_exit_codes_are_reached(env):
    torch, N, O = env
    found = C.exit_code_rois()
    for code in C.EXIT_CODES:
        rows = fit_rows(torch, N, found[code])
        check_rows(N, O, rows, found[code], "exit %d" % code)
        print("exit %d of the restatement: the kernel's exits %s" % (code, rows["status"].tolist()))
        assert (rows["status"] == code).any(), (code, rows["status"].tolist())


@pytest.mark.parametrize("name", ["S"] + TEXTBOOK_NAMES)
def test_rows_are_float32_inside_the_box_with_fp64_metrics(env, name):
    torch, N, O = env
    if name == "S":
        rois = C.spots()[1]
    else:
        g, img = load_field(name, prefix="textbook_")
        rois = rois_of(img, g["candidates"])
    rows = fit_rows(torch, N, rois)
    check_rows(N, O, rows, rois, name)
