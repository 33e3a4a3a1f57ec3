"""GPU tests (-m gpu) of candidate detection at the limits of csrc/fsq_detect.hip, against the reference's own answers
recorded in tests/golden/detect_limits.npz: asymmetric correlation matrices of side 1..9 across the block seams of
k1_response5<false> (uint16, binary16 and uint32 pixels; the older K1 behind FSQ_DETECT_R03 as well), matrices one entry away
from ring symmetry, responses that sum to just below and to 2^53, a response exactly on the threshold, c_std of 0, -1, inf and
NaN, every class of ragged last chunk of the variance, more than 256 fields, empty fields between full ones, more than 256 tiles
in a field, and a candidate buffer smaller than the total through the C ABI.  Candidates are compared exactly and in order,
thresholds as bit patterns (any NaN for a NaN), counts and offsets per field.  Which case runs which kernel, and that the
fixture reaches every branch: _detect_limit_cases.py, test_detect_limits_host.py.  Every buffer the Engine owns is filled with
random bytes before a run; every refusal is checked by its return code or exception, with the output buffers unchanged."""
import ctypes

import numpy as np
import pytest

import _detect_limit_cases as C
from _util import bits_equal

pytestmark = pytest.mark.gpu

ENGINE_CASES = [c.name for c in C.cases() if not c.abi_only and c.name != "seam_k5_floatK"]
OLD_ROUTE = [n for n in ENGINE_CASES if n.split("_")[0] in ("seam", "lowent", "ring") and C.route(C.case(n))["kernel"].startswith("k1_response5")]


@pytest.fixture(scope="module")
def fx():
    return C.fixture()


@pytest.fixture(scope="module")
def E():
    import torch
    assert torch.cuda.is_available()
    from fluorosequencingimageanalysis_amd import engine
    return engine


def params(E, c):
    words, fmt = E.as_pixel_fields(c.images)
    prm = E.detect_params(c.med, c.K, c.c_std, fmt, int(c.images.max()) if c.fmt == "u32" else None)
    return E.to_device_pixels(words, fmt), prm


def dirty(tensors, seed):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    for t in tensors:
        raw = t.view(torch.uint8)
        raw.copy_(torch.randint(0, 256, (raw.numel(),), dtype=torch.uint8, device="cuda", generator=gen).reshape(raw.shape))


def run_engine(E, c, seed=11):
    """One Engine.detect of a case with all of the Engine's buffers holding random bytes -> (triples, counts, offsets, thr)."""
    n, (H, W) = len(c.images), c.shape
    d_img, prm = params(E, c)
    eng = E.Engine(n, H, W, fit_workspace=False)
    dirty((eng.ws, eng.rows, eng.cand, eng.keep, eng.counts, eng.offsets, eng.nkeep, eng.thr), seed)
    total = eng.detect(d_img, prm)
    cand, counts, offsets = eng.candidates(total)
    return cand, counts, offsets, eng.thr.cpu().numpy()


def assert_case(fx, c, got, what):
    cand, counts, offsets, thr = got
    e_cand, e_counts, e_thr, _ = fx.expected(c.name)
    n = len(c.images)
    print(what, "candidates", len(cand), "recorded", len(e_cand), "thr", thr[:3], e_thr[:3].view(np.float64))
    assert np.array_equal(counts[:n], e_counts) and counts[n] == e_counts.sum(), (what, counts, e_counts)
    assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(e_counts)])), (what, offsets)
    assert np.array_equal(cand, C.triples(e_cand, e_counts)), what
    assert bits_equal(thr, e_thr.view(np.float64)).all(), (what, thr, e_thr.view(np.float64))


@pytest.mark.parametrize("name", ENGINE_CASES)
def test_engine_matches_the_reference(E, fx, name):
    c = C.case(name)
    if "refuse" in c.expect:
        with pytest.raises(NotImplementedError, match=r"2\^53"):
            run_engine(E, c)
        return
    assert_case(fx, c, run_engine(E, c), name)


@pytest.mark.parametrize("name", OLD_ROUTE)
def test_old_k1_agrees(E, fx, name, monkeypatch):
    """The same cases through round 3's K1 (FSQ_DETECT_R03: the generic tile kernel with the forgetful-selection median)."""
    c = C.case(name)
    assert C.route(c, r03=True)["kernel"] == "k1_response<true,u16>" != C.route(c)["kernel"]
    monkeypatch.setenv("FSQ_DETECT_R03", "1")
    got = run_engine(E, c, seed=12)
    monkeypatch.delenv("FSQ_DETECT_R03")
    assert_case(fx, c, got, name + " (FSQ_DETECT_R03)")


def test_psf_candidates_matches_the_reference(E, fx):
    """pflib._psf_candidates, the drop-in entry, on every single-field case: the reference's list, its refusals."""
    from fluorosequencingimageanalysis_amd import pflib
    for c in C.cases():
        if len(c.images) != 1 or c.abi_only:
            continue
        args = (c.images[0], c.med, c.K, c.c_std)
        if c.name == "seam_k5_floatK":
            with pytest.raises(NotImplementedError, match="integer correlation matrices"):
                pflib._psf_candidates(*args)
            continue
        if "refuse" in c.expect:
            with pytest.raises(NotImplementedError, match=r"2\^53"):
                pflib._psf_candidates(*args)
            continue
        got = pflib._psf_candidates(*args)
        assert got == [tuple(x) for x in fx.expected(c.name)[0].tolist()], c.name
        assert all(type(h) is int and type(w) is int for h, w in got)


class Raw:
    """fsq_detect through the C ABI on buffers of the test's own, every output pre-filled with the byte 0xA5."""
    FILL = 0xA5

    def __init__(self, E, c, cap, cand_rows=None):
        import torch
        from fluorosequencingimageanalysis_amd import _native as N
        self.torch, self.L = torch, N.lib()
        self.n, (self.H, self.W) = len(c.images), c.shape
        self.d_img, self.prm = params(E, c)
        nbytes = self.L.fsq_detect_workspace_bytes(self.n, self.H, self.W)
        assert nbytes > 0
        mk = lambda shape, dt: torch.full(shape, self.FILL, dtype=torch.uint8, device="cuda").view(dt)      # noqa: E731
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        self.cand = mk((max(cand_rows if cand_rows is not None else cap, 1) * 12,), torch.int32).reshape(-1, 3)
        self.counts, self.offsets = mk((4 * (self.n + 1),), torch.int32), mk((4 * (self.n + 1),), torch.int32)
        self.thr = mk((8 * self.n,), torch.float64)
        self.cap = cap

    def call(self, prm=None, cand="own", ws_bytes=None, n_fields=None):
        rc = self.L.fsq_detect(self.d_img.data_ptr(), self.n if n_fields is None else n_fields, self.H, self.W, ctypes.byref(prm or self.prm),
                               self.cand.data_ptr() if cand == "own" else cand, self.cap, self.counts.data_ptr(), self.offsets.data_ptr(),
                               self.thr.data_ptr(), self.ws.data_ptr(), self.ws.numel() if ws_bytes is None else ws_bytes,
                               self.torch.cuda.current_stream().cuda_stream)
        self.torch.cuda.synchronize()
        return rc

    def host(self):
        return self.cand.cpu().numpy(), self.counts.cpu().numpy(), self.offsets.cpu().numpy(), self.thr.cpu().numpy()

    def untouched(self, a):
        return bool((np.ascontiguousarray(a).view(np.uint8) == self.FILL).all())


def test_cap_smaller_than_the_total(E, fx):
    """cap = total - 1, 1 and 0 (with a NULL candidate pointer) on a seam case: the first `cap` triples are the prefix of the
    full list, the buffer beyond them keeps its bytes, counts and offsets report the full totals."""
    c = C.case("seam_k7_u16")
    e_cand, e_counts, e_thr, _ = fx.expected(c.name)
    full = C.triples(e_cand, e_counts)
    total = len(full)
    assert total > 8
    for cap, null in ((total - 1, False), (1, False), (0, True), (total, False), (total + 5, False)):
        r = Raw(E, c, cap, cand_rows=total + 8)
        assert r.call(cand=None if null else "own") == 0, cap
        cand, counts, offsets, thr = r.host()
        k = min(cap, total)
        assert np.array_equal(cand[:k], full[:k]) and r.untouched(cand[k:]), cap
        assert counts.tolist() == [total, total] and offsets.tolist() == [0, total], (cap, counts, offsets)
        assert bits_equal(thr, e_thr.view(np.float64)).all()


def test_one_row_frame_through_the_c_abi(E, fx):
    """1 x 7 (the Python entries return before any launch: no pixel has a 5 x 5 neighbourhood): no candidate, nothing written
    to the candidate buffer, the reference's threshold."""
    c = C.case("abi_1x7")
    r = Raw(E, c, 4)
    assert r.call() == 0
    cand, counts, offsets, thr = r.host()
    assert counts.tolist() == [0, 0] and offsets.tolist() == [0, 0] and r.untouched(cand)
    assert bits_equal(thr, fx.expected(c.name)[2].view(np.float64)).all(), thr


def test_sum_of_2_53_is_reported_through_the_c_abi(E, fx):
    """fsq_detect itself returns FSQ_OK and a total of -1 for the field whose response sums to 2^53; per-field counts and the
    last offset still hold the count.  Its neighbour, below 2^53, is an ordinary call."""
    for name, refused in (("sum_below", False), ("sum_reach", True)):
        c = C.case(name)
        e_cand, e_counts, _, _ = fx.expected(name)
        r = Raw(E, c, 400)
        assert r.call() == 0
        cand, counts, offsets, thr = r.host()
        assert counts[1] == (-1 if refused else e_counts[0]), (name, counts)
        if not refused:
            assert counts[0] == e_counts[0] and offsets.tolist() == [0, e_counts[0]]
            assert np.array_equal(cand[:counts[0]], C.triples(e_cand, e_counts))


def test_refusals_leave_the_buffers_alone(E):
    """Every refusal of fsq_detect comes back as a return code before anything is launched: all outputs keep their bytes."""
    from fluorosequencingimageanalysis_amd import _native as N
    c = C.case("seam_k7_u16")

    def prm(**kw):
        p = N.FsqDetectParams()
        ctypes.memmove(ctypes.byref(p), ctypes.byref(r.prm), ctypes.sizeof(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    r = Raw(E, c, 64)
    big = prm()
    big.K[3] = 2 ** 31
    wide = prm(ksz=15)
    for i in range(225):
        wide.K[i] = 2 ** 31 - 1                          # 225 (2^31 - 1) 65535 H W >= 2^64: the response sum could wrap
    calls = [(dict(prm=prm(ksz=4)), N.FSQ_EINVAL), (dict(prm=prm(ksz=17)), N.FSQ_ENOTIMPL), (dict(prm=prm(median_filter_size=16)), N.FSQ_ENOTIMPL),
             (dict(prm=prm(median_filter_size=0)), N.FSQ_ENOTIMPL), (dict(prm=prm(pixel_format=7)), N.FSQ_EINVAL), (dict(prm=big), N.FSQ_ENOTIMPL),
             (dict(prm=wide), N.FSQ_ENOTIMPL), (dict(cand=None), N.FSQ_EINVAL), (dict(ws_bytes=r.ws.numel() - 1), N.FSQ_ENOMEM),
             (dict(n_fields=0), N.FSQ_EINVAL)]
    for kw, want in calls:
        assert r.call(**kw) == want, (kw, want)
        assert all(r.untouched(a) for a in r.host()), kw
    assert r.call() == 0 and not r.untouched(r.host()[1])       # ... and the same buffers take an ordinary call
