"""GPU tests (-m gpu) of frame registration at the limits of csrc/fsq_register.hip, against the reference's own answers
recorded in tests/golden/registration_limits.npz: upsample factors at which the MFMA row product ends on a single 16-row
tile (Mp = 16, 48, 80) or carries padded rows, shapes on both sides of the path predicate and on its boundaries (Mp == H,
Mp == W, H % 4 == 0 with H % 16 != 0), odd and even grids, blank frames, shifts of exactly half the size, images down to
1 x 1.  Which (shape, factor) runs which path, the comparison rule and why no case can leave a buffer:
_register_limit_cases.py; that the fixture reaches every branch: test_register_limits_host.py."""
import builtins

import numpy as np
import pytest

import _register_limit_cases as C

pytestmark = pytest.mark.gpu

ALL_SHAPES = C.SHAPES + C.TINY
MFMA_CASES = [(H, W, uf) for H, W in C.SHAPES for uf in C.FACTORS if C.layout(H, W, uf)[2]]


@pytest.fixture(scope="module")
def pc():
    import torch
    assert torch.cuda.is_available()
    from fluorosequencingimageanalysis_amd import phase_correlate as m
    return m


@pytest.fixture(scope="module")
def fx():
    return C.fixture()


_SINGLE = {}


def single(pc, fx, name, uf):
    """One pair through phase_correlate as uint16 (computed once per pair and factor; the reference of the batched tests)."""
    if (name, uf) not in _SINGLE:
        a, b = fx.pairs[name]
        _SINGLE[name, uf] = np.array([float(x) for x in pc.phase_correlate(a, b, upsample_factor=uf)])
    return _SINGLE[name, uf]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def stack(fx, names):
    return np.stack([fx.pairs[n][0] for n in names]), np.stack([fx.pairs[n][1] for n in names])


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "%dx%d" % s)
def test_fixture_single_calls(pc, fx, shape):
    """Every pair at every factor, as uint16 and as float64: the recorded tuple, and the same bits from both dtypes.  The
    tiny shapes are here too: the port returns what the reference returned, NaN for NaN, and raises what it raised."""
    for name in fx.of_shape(*shape):
        a, b = fx.pairs[name]
        for uf in C.FACTORS:
            exp, exc, kw = fx.expected(name, uf)
            if exc:
                with pytest.raises(getattr(builtins, exc)):
                    pc.phase_correlate(a, b, upsample_factor=uf)
                continue
            r16 = single(pc, fx, name, uf)
            r64 = pc.phase_correlate(a.astype(np.float64), b.astype(np.float64), upsample_factor=uf)
            print(name, uf, C.layout(*shape, uf)[1:], r16.tolist(), exp.tolist())
            C.assert_matches(r16, exp, (name, uf), **kw)
            assert np.array_equal(bits(r16), bits([float(x) for x in r64])), (name, uf, r16, r64)
            assert isinstance(r64[0], np.int64 if uf == 1 else np.float64)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "%dx%d" % s)
def test_fixture_batched(pc, fx, shape):
    """All pairs of a shape in one call per factor (the blank pair between real ones): the single calls' bits."""
    names = fx.of_shape(*shape)
    if len(names) == 3:
        names = [names[1], names[0], names[2]]          # (roll, blank, rand)
    if len(names) >= 3:
        assert not names[0].endswith("_blank") and not names[-1].endswith("_blank")
    if len(names) > 3:
        assert names[0].endswith("_int") and names[-1].startswith("%dx%d_sub" % shape) and any(n.endswith("_blank") for n in names[1:-1])
    ref, reg = stack(fx, names)
    for uf in C.FACTORS:
        out = pc.phase_correlate_batch(ref, reg, uf)
        exp = np.stack([single(pc, fx, n, uf) for n in names])
        assert np.array_equal(bits(out), bits(exp)), (shape, uf, out, exp)


@pytest.mark.parametrize("n_pairs", (1, 63, 64, 65))
def test_batch_sizes_around_one_block_of_k6_fine(pc, fx, n_pairs):
    names = fx.of_shape(16, 16)
    names = [names[i % len(names)] for i in range(n_pairs)]
    ref, reg = stack(fx, names)
    for uf in C.FACTORS:
        out = pc.phase_correlate_batch(ref, reg, uf)
        exp = np.stack([single(pc, fx, n, uf) for n in names])
        assert np.array_equal(bits(out), bits(exp)), (n_pairs, uf, np.argwhere(bits(out) != bits(exp)))


@pytest.mark.parametrize("env", (("FSQ_REGISTER_Z2Z",), ("FSQ_REGISTER_NO_MFMA",), ("FSQ_REGISTER_Z2Z", "FSQ_REGISTER_NO_MFMA")),
                         ids=("z2z", "no_mfma", "z2z_no_mfma"))
def test_forced_paths(pc, fx, env, monkeypatch):
    """Every (shape, factor) that the predicate sends to the matrix cores, through the full-spectrum form (rkT and T in
    the slots of F and G: Mp == H, Mp == W), on the vector-ALU DFT, and both: the default path's shifts, error and
    diffphase within the bounds."""
    assert len(MFMA_CASES) == 23
    for H, W, uf in MFMA_CASES:
        names = fx.of_shape(H, W)
        ref, reg = stack(fx, names)
        base = pc.phase_correlate_batch(ref, reg, uf)
        for e in env:
            monkeypatch.setenv(e, "1")
        out = pc.phase_correlate_batch(ref, reg, uf)
        for e in env:
            monkeypatch.delenv(e)
        for k, n in enumerate(names):
            assert np.array_equal(out[k, :2], base[k, :2], equal_nan=True), (n, uf, env, out[k], base[k])
            C.assert_matches(out[k], fx.expected(n, uf)[0], (n, uf, env))
            C.assert_matches(out[k], base[k], (n, uf, env, "against the default path"))


def test_dirty_workspace(pc, fx):
    """48 x 64 at uf = 22 (up = 33, Mp = 48: fifteen padded columns of rkT, a single-tile last block): whatever the
    workspace held before - zeros, all ones, random bytes (NaNs and infinities as doubles) - the output bits are the same."""
    import torch
    from fluorosequencingimageanalysis_amd import engine as E
    names = fx.of_shape(48, 64)
    ref, reg = stack(fx, names)
    d_ref, d_reg = E.to_device_u16(ref), E.to_device_u16(reg)
    exp = np.stack([single(pc, fx, n, 22) for n in names])
    gen = torch.Generator(device="cuda").manual_seed(7)
    for fill in ("zeros", "ones", "random"):
        R = pc.Registrar(len(names), 48, 64, 22)
        ws = R._workspace(torch.cuda.current_stream().cuda_stream)
        if fill == "random":
            ws.copy_(torch.randint(0, 256, (ws.numel(),), dtype=torch.uint8, device=ws.device, generator=gen))
        else:
            ws.fill_(0 if fill == "zeros" else 255)
        out = R.register(d_ref, d_reg).cpu().numpy()
        assert np.array_equal(bits(out), bits(exp)), (fill, out, exp)


@pytest.mark.parametrize("shape", ((16, 16), (48, 64)), ids=lambda s: "%dx%d" % s)
def test_registrars_of_several_factors_share_a_stream(pc, fx, shape):
    """Factors 10, 11, 22 and 1 in turn on one shape and one stream: the transform plans are cached without the factor
    and handed each Registrar's own work area call by call; every result is that of a fresh Registrar."""
    from fluorosequencingimageanalysis_amd import engine as E
    names = fx.of_shape(*shape)
    ref, reg = stack(fx, names)
    d_ref, d_reg = E.to_device_u16(ref), E.to_device_u16(reg)
    regs = {uf: pc.Registrar(len(names), shape[0], shape[1], uf) for uf in (10, 11, 22, 1)}
    outs = [(uf, R.register(d_ref, d_reg)) for _ in range(3) for uf, R in regs.items()]       # (enqueued back to back)
    for uf, out in outs:
        fresh = pc.Registrar(len(names), shape[0], shape[1], uf).register(d_ref, d_reg).cpu().numpy()
        assert np.array_equal(bits(out.cpu().numpy()), bits(fresh)), (shape, uf)
        assert np.array_equal(bits(fresh), bits(np.stack([single(pc, fx, n, uf) for n in names]))), (shape, uf)
