"""GPU tests (-m gpu) of the per-evaluation range predicate of csrc/fsq_evalguard.h: the fast fit kernels no longer check
operand ranges on every model pixel, so fits that SIT ON the predicate's edges - theta pegged at 0 and 360 and driven towards
90 degrees (c or s zero or tiny), centres and sigmas pegged at both bounds, background / amplitude pegged at 0 on ROIs with
zero pixels, flat and saturated ROIs - must still equal the oracle bit for bit, in both solver modes, at batch sizes that leave
partial quads and partial waves, through the exact path as well, and whatever the workspace held."""
import ctypes

import numpy as np
import pytest

from _util import bits_equal

pytestmark = pytest.mark.gpu

P7 = ("H", "A", "p2", "p3", "sigma_h", "sigma_w", "theta")
SIZES = (1, 15, 17, 63, 65)


def _spot(H, A, ch, cw, sh, sw, theta_deg, noise=0, seed=0):
    """The fit's own model (gaussfitter.py:100-136) sampled on the 5x5 grid, rounded to integers, clipped to 16 bits."""
    t = np.pi / 180.0 * theta_deg
    x, y = np.indices((5, 5)).astype(np.float64)
    c, s = np.cos(t), np.sin(t)
    rcx, rcy = cw * c - ch * s, cw * s + ch * c
    xp, yp = x * c - y * s, x * s + y * c
    g = H + A * np.exp(-(((rcx - xp) / sh) ** 2 + ((rcy - yp) / sw) ** 2) / 2.0)
    if noise:
        g = g + np.random.default_rng(seed).normal(0.0, noise, g.shape)
    return np.clip(np.rint(g), 0, 65535).astype(np.int64).reshape(25)


def edge_rois():
    """65 ROIs; the first ones are the sharpest edge cases so that every batch size above holds some of them."""
    r = []
    r.append(_spot(0, 40000, 2.5, 2.5, 0.8, 0.8, 0))                   # zero pixels all round: background pegged at 0, theta at 0
    r.append(_spot(300, 9000, 2.4, 2.6, 0.9, 1.8, 90))                  # long axis at 90 degrees: cos tiny
    r.append(_spot(300, 9000, 2.5, 2.5, 1.9, 0.8, 358))                 # towards theta's upper bound
    r.append(_spot(200, 30000, 1.2, 1.4, 1.0, 1.0, 0))                  # centre beyond the lower bound of both coordinates
    r.append(_spot(200, 30000, 3.8, 3.6, 1.0, 1.0, 0))                  # ... and beyond the upper bound
    r.append(_spot(100, 50000, 2.5, 2.5, 0.4, 0.4, 0))                  # narrower than sigma's lower bound
    r.append(_spot(100, 5000, 2.5, 2.5, 6.0, 5.0, 0))                   # wider than its upper bound
    r.append(np.zeros(25, np.int64))                                    # all zero: amplitude and background pegged at 0
    r.append(np.full(25, 1234, np.int64))                               # flat
    r.append(np.full(25, 65535, np.int64))                              # saturated
    r.append(_spot(60000, 60000, 2.5, 2.5, 1.2, 1.2, 0))                # saturated plateau
    one = np.zeros(25, np.int64); one[12] = 65535; r.append(one)        # a single pixel on zeros
    corner = np.zeros(25, np.int64); corner[0] = 5000; corner[24] = 4000; r.append(corner)
    r.append(_spot(0, 3000, 2.0, 3.0, 0.75, 2.0, 0))                    # truth on four bounds at once
    r.append(_spot(0, 20000, 2.5, 2.5, 0.9, 1.7, 89.99))
    r.append(_spot(0, 20000, 2.5, 2.5, 0.9, 1.7, 270))
    r.append(_spot(500, 20000, 2.3, 2.7, 1.7, 0.9, 180))
    k = 0
    for theta in (0, 1, 45, 89, 90, 91, 135, 179, 180, 181, 269, 270, 271, 359, 360):
        for sh, sw in ((0.8, 1.9), (1.9, 0.8), (1.3, 1.3), (0.76, 2.0)):
            if len(r) < 65:
                k += 1
                r.append(_spot((0, 150, 700)[k % 3], (800, 6000, 40000)[k % 3], 2.0 + 0.07 * (k % 15), 3.0 - 0.06 * (k % 17), sh, sw, theta,
                               noise=(0, 3, 40)[k % 3], seed=k))
    assert len(r) == 65
    return np.stack(r)


@pytest.fixture(scope="module")
def env():
    import torch
    from fluorosequencingimageanalysis_amd import _native
    import oracle as O
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    O.build()
    return torch, _native, O


@pytest.fixture(scope="module")
def case(env):
    """The ROIs and the oracle's fits of them in both solver modes (computed once, shared, never modified)."""
    torch, N, O = env
    rois = edge_rois()
    ref = {mode: O.fit_rois(rois.astype(np.uint16), mode=mode, n_threads=8) for mode in (0, 1)}
    for v in ref.values():
        v.setflags(write=False)
    return rois, ref


def _fit(torch, N, rois, mode=0, ws_fill=None):
    d = torch.from_numpy(np.ascontiguousarray(rois.astype(np.uint16)).view(np.int16)).cuda()
    rows = torch.zeros(len(rois) * 128, dtype=torch.uint8, device="cuda")
    nbytes = N.lib().fsq_fit_workspace_bytes(len(rois))
    if ws_fill is None:
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    else:
        ws = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(ws_fill))
    N.check(N.lib().fsq_fit_rois(d.data_ptr(), len(rois), mode, rows.data_ptr(), ws.data_ptr(), ws.numel(),
                                 torch.cuda.current_stream().cuda_stream), "fsq_fit_rois")
    torch.cuda.synchronize()
    return rows.cpu().numpy().view(N.ROW_DTYPE)


def _same(got, ref, n, what):
    p = np.stack([got[k] for k in P7], axis=1)
    bad = np.flatnonzero(~bits_equal(p, ref["p"][:n]).all(axis=1))
    assert len(bad) == 0, "%s: parameters differ from the oracle in fits %s" % (what, bad.tolist())
    for k in ("status", "niter", "nfev"):
        assert np.array_equal(got[k], ref[k][:n]), (what, k)


def test_the_rois_sit_on_the_guard_edges(case):
    """The oracle's own results (not the code under test): the batch does peg every bound the predicate is built around."""
    rois, ref = case
    p = ref[0]["p"]
    assert (p[:, 6] == 0.0).any() and (p[:, 6] == 360.0).any(), "theta pegged at both bounds"
    assert (np.abs(p[:, 6] % 180.0 - 90.0) < 0.3).any(), "theta driven near 90 / 270 degrees (cos small)"
    assert 0 < np.abs(np.sin(np.pi / 180.0 * 360.0)) < 1e-15           # (and pegged at 360 the sine is tiny, not zero)
    for col in (2, 3):
        assert (p[:, col] == 2.0).any() and (p[:, col] == 3.0).any(), "centre coordinate %d pegged at both bounds" % col
    sig = p[:, 4:6]
    assert (sig == 0.75).any() and (sig == 2.0).any(), "sigma pegged at both bounds"
    assert ((p[:, 0] == 0.0) & (rois == 0).any(axis=1)).any(), "background pegged at 0 on a ROI with zero pixels"
    assert (p[:, 1] == 0.0).any(), "amplitude pegged at 0"
    for n in SIZES:                 # the smallest batch still holds an edge case, the larger ones several kinds
        assert (p[:n, 0] == 0.0).any()


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("n", SIZES)
def test_edge_fits_equal_the_oracle(env, case, n, mode):
    torch, N, O = env
    rois, ref = case
    _same(_fit(torch, N, rois[:n], mode), ref[mode], n, "n=%d mode=%d" % (n, mode))


@pytest.mark.parametrize("mode", (0, 1))
def test_edge_fits_through_the_exact_path_and_on_a_dirty_workspace(env, case, mode, monkeypatch):
    """Every second fit forced through the FAST = false kernels (FSQ_DEBUG_FORCE_SLOW), on zeroed and on random workspace bits:
    both paths give the oracle's bits.  Without forcing, the predicate must add no slow-path fit: it rejects nothing inside the box
    (tests/test_evalguard_host.py), so the fits that leave the fast path are those that qrfac's own guards send, exactly as before
    the predicate existed.  The parent commit sends 18 (reference solver) and 19 (textbook solver) of these 65 fits through the slow
    kernel (measured with the parent's library on this batch; the headline fields: 77 091 of 1 089 660 with and without the
    predicate, profiles/r06_summary.md) - those counts are the bound."""
    torch, N, O = env
    rois, ref = case
    monkeypatch.setenv("FSQ_DEBUG_FORCE_SLOW", "2")
    _same(_fit(torch, N, rois, mode), ref[mode], len(rois), "forced slow")
    assert N.lib().fsq_fit_last_slow_count() > 0
    _same(_fit(torch, N, rois, mode, ws_fill=5), ref[mode], len(rois), "forced slow, random workspace")
    monkeypatch.delenv("FSQ_DEBUG_FORCE_SLOW")
    _same(_fit(torch, N, rois, mode, ws_fill=6), ref[mode], len(rois), "random workspace")
    slow = int(N.lib().fsq_fit_last_slow_count())
    print("unforced: %d of %d fits through the slow kernel" % (slow, len(rois)))
    assert slow <= {0: 18, 1: 19}[mode]


def test_wide_pixel_edge_fits_equal_the_oracle(env, case):
    """The same ROIs scaled beyond 16 bits, tiled into one uint32 frame (fsq_fit_candidates | FSQ_PIXELS_U32_FLAG: the P32
    instantiations of both kernels)."""
    torch, N, O = env
    rois, _ = case
    wide = rois * np.array([1, 17, 4001, 30000])[np.arange(len(rois)) % 4][:, None]        # up to 65535 * 30000 < 2^31
    assert wide.max() > 65535 and wide.max() < 2 ** 31
    ref = O.fit_rois(wide.astype(np.int64), mode=0, n_threads=8)
    per_row = 9
    H, W = 6 * ((len(wide) + per_row - 1) // per_row) + 1, 6 * per_row + 1
    img = np.zeros((H, W), np.uint32)
    cand = np.zeros((len(wide), 3), np.int32)
    for i, roi in enumerate(wide):
        h, w = 3 + 6 * (i // per_row), 3 + 6 * (i % per_row)
        img[h - 2:h + 3, w - 2:w + 3] = roi.reshape(5, 5)
        cand[i] = (0, h, w)
    d_img = torch.from_numpy(img.view(np.int32)).cuda()
    d_cand = torch.from_numpy(cand).cuda()
    rows = torch.zeros(len(wide) * 128, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(N.lib().fsq_fit_workspace_bytes(len(wide)), dtype=torch.uint8, device="cuda")
    N.check(N.lib().fsq_fit_candidates(d_img.data_ptr(), 1, H, W, d_cand.data_ptr(), len(wide), N.MODE_REF | N.PIXELS_U32_FLAG,
                                       rows.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream),
            "fsq_fit_candidates")
    torch.cuda.synchronize()
    _same(rows.cpu().numpy().view(N.ROW_DTYPE), ref, len(wide), "wide pixels")


def test_unchecked_forms_equal_division_and_exp_inside_the_proved_ranges(env):
    """fsq_selftest_evalguard on 2^22 operands inside the ranges fsq_evalguard.h proves: numerators 0 or 2^-452 <= |n| <= 16 (dense
    where the model lives, log-uniform down to the floor, both zeros), divisors 0.75 <= |d| < 2^250 (dense in the box [0.75, 2]),
    exp arguments in [-455.2, 0] - zero differences in the square of the quotient and in exp's bits."""
    torch, N, O = env
    rng = np.random.default_rng(2024)
    n = 1 << 22
    k = 1 << 20
    num = rng.uniform(-16.0, 16.0, n)
    num[:k] = rng.choice([-1.0, 1.0], k) * np.ldexp(rng.random(k) + 1.0, rng.integers(-452, 3, k))
    num[k:k + (1 << 18)] = rng.integers(-16, 17, 1 << 18).astype(np.float64)                 # exact quotients and ties
    den = rng.uniform(0.75, 2.0, n) * rng.choice([-1.0, 1.0], n)
    den[2 * k:3 * k] = rng.choice([-1.0, 1.0], k) * np.ldexp(rng.random(k) + 1.0, rng.integers(0, 249, k))
    x = -rng.uniform(0.0, 455.2, n)
    x[:k] = -rng.uniform(0.0, 40.0, k)
    x[k:k + (1 << 18)] = -np.ldexp(rng.random(1 << 18) + 1.0, rng.integers(-1074, 8, 1 << 18))
    sp_n = [0.0, -0.0, 16.0, -16.0, 2.0 ** -452, -2.0 ** -452, 1.0, 3.0]
    sp_d = [0.75, -0.75, 2.0, np.nextafter(0.75, 1), np.nextafter(2.0 ** 250, 0), 1.0, 1.5, 3.0]
    sp_x = [0.0, -0.0, -455.2, -2.0 ** -54, -2.0 ** -55, -5e-324, -1.0, -0.5]
    num[-8:], den[-8:], x[-8:] = sp_n, sp_d, sp_x
    x = np.where(x < -455.2, -455.2, x)
    assert (np.abs(num) <= 16).all() and ((num == 0) | (np.abs(num) >= 2.0 ** -452)).all()
    assert (np.abs(den) >= 0.75).all() and (np.abs(den) < 2.0 ** 250).all() and (x <= 0).all() and (x >= -455.2).all()
    dn, dd, dx = (torch.from_numpy(a).cuda() for a in (num, den, x))
    bad_sq, bad_exp = ctypes.c_int64(-1), ctypes.c_int64(-1)
    N.check(N.lib().fsq_selftest_evalguard(dn.data_ptr(), dd.data_ptr(), dx.data_ptr(), n, ctypes.byref(bad_sq), ctypes.byref(bad_exp),
                                           torch.cuda.current_stream().cuda_stream), "selftest")
    assert bad_sq.value == 0 and bad_exp.value == 0
