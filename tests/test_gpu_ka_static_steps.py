"""GPU parity tests (-m gpu) of the Jacobian round's static qrfac steps: the fast four-lane kernel compiles each Householder
step with its index as a constant, so every step is code of its own whose row loops stop at 25 - j.  A Jacobian column that is all
zero (a pegged parameter) makes ajnorm == 0 and breaks qrfac at step 7 - k, k being the number of zero columns: k = 1 .. 4 ends
the factorisation in each of the steps 3 .. 6.  The sample therefore holds as many fits with k = 0, 1, 2, 3 and 4 parameters on a
bound, interleaved so that every 16-fit wave and every position in it sees every k.  Every case asks for BIT equality with the
oracle: the 7 parameters, status, niter and nfev."""
import numpy as np
import pytest

from _util import DEGEN_NAMES, bits_equal, load_field, rois_of

pytestmark = pytest.mark.gpu

PARAMS = ("H", "A", "p2", "p3", "sigma_h", "sigma_w", "theta")
MODE_REF, MODE_TEXTBOOK = 0, 1
PER_BUCKET = 64


@pytest.fixture(scope="module")
def env():
    import torch
    from fluorosequencingimageanalysis_amd import _native
    import oracle as O
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    O.build()
    return torch, _native, O


def gpu_fit(torch, N, rois, mode=MODE_REF, ws_fill=None):
    d = torch.from_numpy(np.ascontiguousarray(rois.astype(np.uint16)).view(np.int16)).cuda()
    rows = torch.zeros(len(rois) * 128, dtype=torch.uint8, device="cuda")
    nbytes = N.lib().fsq_fit_workspace_bytes(len(rois))
    if ws_fill == "random":
        ws = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(11))
    else:
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    N.check(N.lib().fsq_fit_rois(d.data_ptr(), len(rois), mode, rows.data_ptr(), ws.data_ptr(), ws.numel(),
                                 torch.cuda.current_stream().cuda_stream), "fsq_fit_rois")
    torch.cuda.synchronize()
    return rows.cpu().numpy().view(N.ROW_DTYPE)


def assert_equals_oracle(got, ref, what=""):
    p = np.stack([got[k] for k in PARAMS], axis=1)
    nbad = int((~bits_equal(p, ref["p"]).all(axis=1)).sum())
    assert nbad == 0, "%s: parameters differ from the oracle's in %d of %d fits" % (what, nbad, len(got))
    for k in ("status", "niter", "nfev"):
        assert np.array_equal(got[k], ref[k]), (what, k)


def n_on_bound(rois, p):
    """How many of a fit's final parameters sit exactly on a bound (pflib's limits: H >= 0, A >= (max - mean) / 3, the centre
    in [2, 3], the sigmas in [0.75, 2], theta in [0, 360])."""
    r = rois.astype(np.int64)
    llim1 = (r.max(axis=1).astype(np.float64) - r.sum(axis=1) / 25.0) / 3.0
    k = (p[:, 0] == 0).astype(int) + (p[:, 1] == llim1)
    for i, (lo, hi) in ((2, (2., 3.)), (3, (2., 3.)), (4, (0.75, 2.)), (5, (0.75, 2.)), (6, (0., 360.))):
        k = k + ((p[:, i] == lo) | (p[:, i] == hi))
    return k


@pytest.fixture(scope="module")
def ladder(env):
    """320 ROIs of the headline workload (synth.make_field seeds 0 and 1, 512 x 512, 500 spots): the first 64 with k = 0, 1, 2, 3
    and 4 parameters on a bound, in the order k = 0, 1, 2, 3, 4, 0, 1, ... - 16 and 4 are prime to 5, so every wave of 16 fits
    and every quad position meets every k.  With them the oracle's fits in the reference mode."""
    torch, N, O = env
    from fluorosequencingimageanalysis_amd import synth
    parts = []
    for seed in (0, 1):
        img = synth.make_field(seed, (512, 512), 500)
        parts.append(rois_of(img, O.candidates(img)))
    rois = np.concatenate(parts)
    ref = O.fit_rois(rois, mode=MODE_REF, n_threads=16)
    k = n_on_bound(rois, ref["p"])
    buckets = [np.flatnonzero(k == kk) for kk in range(5)]
    sizes = [len(b) for b in buckets]
    assert min(sizes) >= PER_BUCKET, "a bucket of pegged-parameter counts is short of %d fits: %r" % (PER_BUCKET, sizes)
    sel = np.stack([b[:PER_BUCKET] for b in buckets], axis=1).reshape(-1)       # k = 0, 1, 2, 3, 4, 0, 1, ...
    assert np.array_equal(k[sel][:10], [0, 1, 2, 3, 4, 0, 1, 2, 3, 4])
    rois, ref = np.ascontiguousarray(rois[sel]), ref[sel].copy()
    rois.setflags(write=False)
    ref.setflags(write=False)
    return rois, ref


@pytest.fixture(scope="module")
def ladder_textbook(env, ladder):
    torch, N, O = env
    ref = O.fit_rois(ladder[0], mode=MODE_TEXTBOOK, n_threads=16)
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("mode", [MODE_REF, MODE_TEXTBOOK])
@pytest.mark.parametrize("n", [1, 15, 17, 320])
def test_ladder(env, ladder, ladder_textbook, mode, n):
    """All 320, and their first 1, 15 and 17 (one quad, a wave one quad short, a wave and one quad), in both solver modes."""
    torch, N, O = env
    rois, ref = ladder
    if mode == MODE_TEXTBOOK:
        ref = ladder_textbook
    got = gpu_fit(torch, N, rois[:n], mode=mode)
    if n == 320:
        assert N.lib().fsq_fit_last_slow_count() < 0.2 * n, "ordinary data must (nearly) never leave the fast kernel"
    assert_equals_oracle(got, ref[:n], "mode=%d n=%d" % (mode, n))


def test_forced_norm_recomputation(env, ladder, monkeypatch):
    """The re-computation of a down-dated norm forced on both sides, so that it runs in every static step that has one."""
    torch, N, O = env
    rois, ref0 = ladder
    monkeypatch.setenv("FSQ_DEBUG_FORCE_NORM_RECOMPUTE", "1")
    O.lib().fsq_o_set_force_norm_recompute(1)
    try:
        got = gpu_fit(torch, N, rois)
        ref = O.fit_rois(rois, mode=MODE_REF, n_threads=16)
    finally:
        O.lib().fsq_o_set_force_norm_recompute(0)
        monkeypatch.delenv("FSQ_DEBUG_FORCE_NORM_RECOMPUTE")
    assert_equals_oracle(got, ref, "forced recomputation")
    assert not bits_equal(ref["p"], ref0["p"]).all(), "the forced branch should change some trajectories"


def test_forced_slow_queue(env, ladder, monkeypatch):
    """Every third fit through the plain-division instantiation, which keeps the rolled steps: records of both kernels in one
    batch."""
    torch, N, O = env
    rois, ref = ladder
    monkeypatch.setenv("FSQ_DEBUG_FORCE_SLOW", "3")
    try:
        got = gpu_fit(torch, N, rois)
        assert N.lib().fsq_fit_last_slow_count() >= len(rois) // 3
    finally:
        monkeypatch.delenv("FSQ_DEBUG_FORCE_SLOW")
    assert_equals_oracle(got, ref, "FSQ_DEBUG_FORCE_SLOW=3")


def test_degenerate_frames_in_one_batch(env):
    """Flat, saturated, dim, noise, hot-pixel and all-zero frames, 16 copies of each in one batch on a workspace of random bits:
    columns that are all zero from the start, the break at step 0 and at every step after it."""
    torch, N, O = env
    parts = []
    for name in DEGEN_NAMES:
        g, img = load_field(name, prefix="degen_")
        parts += [rois_of(img, g["candidates"])] * 16
    rois = np.concatenate(parts)
    got = gpu_fit(torch, N, rois, ws_fill="random")
    assert_equals_oracle(got, O.fit_rois(rois, mode=MODE_REF, n_threads=16), "degenerate frames")
