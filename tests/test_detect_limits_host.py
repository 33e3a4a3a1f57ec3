"""CPU checks that tests/golden/detect_limits.npz is not vacuous and that the oracle stands where the reference stands: read
from the recorded reference output and from the route restated in _detect_limit_cases.route, never from the code under
test, the fixture holds a case for every branch of csrc/fsq_detect.hip that the older detection tests leave unrun or run
inside one block only; oracle/fsq_oracle.c gives the reference's list and threshold on every field of every case and refuses
exactly the one whose response sums to 2^53; engine.detect_params refuses what the GPU path cannot reproduce."""
import os

import numpy as np
import pytest

import _detect_limit_cases as C
from _util import bits_equal

KERNELS = {"k1_response5<true>", "k1_response5<false>", "k1_response<true,u16>", "k1_response<false,u16>",
           "k1_response<true,u32>", "k1_response<false,u32>"}
# the route every case has to keep (kernel, blocks per field, tiles, last chunk)
ROUTES = {
    "seam_k1": ("k1_response5<false>", (2, 3)), "seam_k3": ("k1_response5<false>", (2, 3)), "seam_k5": ("k1_response5<false>", (2, 3)),
    "seam_k7": ("k1_response5<false>", (3, 3)), "seam_k9": ("k1_response5<false>", (3, 3)),
    "seam_default_u16": ("k1_response5<true>", (2, 3)), "seam_k11_u16": ("k1_response<true,u16>", (2, 3)),
    "seam_med3_k3_u16": ("k1_response<false,u16>", (2, 3)), "seam_med4_k3_u32": ("k1_response<false,u32>", (2, 3)),
    "lowent_k5_u16": ("k1_response5<false>", (2, 3)), "lowent_k9_u16": ("k1_response5<false>", (3, 3)), "lowent_k5_u32": ("k1_response<true,u32>", (2, 3)),
    "ring_corner": ("k1_response5<false>", (2, 3)), "ring_inner": ("k1_response5<false>", (2, 3)),
    "ring_corner_default": ("k1_response5<true>", (2, 3)), "ring_inner_default": ("k1_response5<true>", (2, 3)),
    "sum_below": ("k1_response<true,u16>", (2, 1)), "sum_reach": ("k1_response<true,u16>", (2, 1)),
    "tie_c0": ("k1_response<false,u16>", (1, 1)), "tie_c1e-9": ("k1_response<false,u16>", (1, 1)),
}


@pytest.fixture(scope="module")
def fx():
    return C.fixture()


def in_interior(c, cand):
    H, W = c.shape
    return len(cand) == 0 or ((cand[:, 0] >= 2) & (cand[:, 0] < H - 2) & (cand[:, 1] >= 2) & (cand[:, 1] < W - 2)).all()


def test_fixture_holds_every_case(fx):
    assert os.path.getsize(C.FIXTURE) < 200_000
    assert fx.names == [c.name for c in C.cases()]
    assert not any(fx.exc)                      # the reference raised nowhere: every refusal is the port's own
    for i, c in enumerate(C.cases()):
        assert int(fx.n_fields[i]) == len(c.images) and int(fx.crc[i]) == c.crc(), c.name
        assert (c.name in fx.pixels) == c.crafted, c.name
        if c.crafted:
            assert np.array_equal(fx.pixels[c.name], c.images), c.name
        cand, counts, thr, _ = fx.expected(c.name)
        assert len(cand) == counts.sum() and in_interior(c, cand), c.name
        for f, (want, n) in enumerate(zip(c.expect, counts)):
            assert want == "refuse" or n == {"all": C.interior(c), "none": 0}.get(want, n), (c.name, f, want, n)
            assert want != "some" or 0 < n < C.interior(c), (c.name, f, n)
    assert set(fx.orient) == set(C.ORIENTED) and len(C.ORIENTED) == 12


def test_every_route_is_reached():
    """Every K1 instantiation on a frame of several blocks (with and without FSQ_DETECT_R03), every class of last chunk, tile
    and field counts on both sides of 256, both sides of 2^53."""
    cases = [c for c in C.cases() if c.name != "seam_k5_floatK"]
    routes = {c.name: C.route(c) for c in cases}
    for name, r in routes.items():
        key = name if name in ROUTES else name.rsplit("_", 1)[0]
        if key in ROUTES:
            want = ROUTES[key]
            if name.endswith("_u32") and key.startswith("seam_k"):
                want = ("k1_response<true,u32>", (2, 3))
            assert (r["kernel"], r["blocks"]) == want, (name, r)
    multi = {r["kernel"] for r in routes.values() if r["blocks"][0] > 1 and r["blocks"][1] > 1}
    assert multi == KERNELS, multi
    for s, tile in zip(C.SEAM_SIDES, ((16, 64), (14, 62), (12, 60), (10, 58), (8, 56))):
        for fmt in ("u16", "f16"):
            r = routes["seam_k%d_%s" % (s, fmt)]
            assert r["tile"] == tile and r["blocks"][0] >= 2 and r["blocks"][1] >= 3
            assert C.SEAM_SHAPE[0] % tile[0] and C.SEAM_SHAPE[1] % tile[1]
            assert C.route(C.case("seam_k%d_%s" % (s, fmt)), r03=True)["kernel"] == "k1_response<true,u16>"
    assert {C.chunk_class(r["last_chunk"]) for r in routes.values()} == {"<8", "8", "(8,128]", "(128,8192)", "full"}
    assert [routes["chunk_%dx%d" % s]["last_chunk"] for s in C.CHUNK_SHAPES] == [3, 8, 128, 129, 8191, 8192]
    assert routes["chunk_127x129"]["chunks"] == 2 and routes["abi_1x7"]["last_chunk"] == 7
    assert {r["tiles"] for r in routes.values()} >= {1, 2, 257} and routes["flat33"]["tiles"] == 2
    assert routes["tiles257_513x512"]["tiles"] == 257 and routes["tiles258_2052x128"]["tiles"] == 257
    assert routes["fields257_8x8"]["fields"] == 257 and routes["fields3_24x40"]["fields"] == 3
    below, reach = C.case("sum_below"), C.case("sum_reach")
    assert 2 ** 52 <= C.SUMS[2] < 2 ** 53 <= C.SUMS[3]
    assert int(C.response_int(below.images[0], 5, below.K).sum()) == C.SUMS[2] and int(C.response_int(reach.images[0], 5, reach.K).sum()) == C.SUMS[3]
    assert int((reach.images != below.images).sum()) == 1            # one more hot pixel
    assert C.static_checks(below) and C.static_checks(reach) and all(C.static_checks(c) for c in cases)


def test_recorded_structure(fx):
    """What the cases are chosen for, read off the recorded lists."""
    # candidates in the second round of k2_scan_field (tiles 256 and up) - and none there in the 513 x 512 frame
    cand = fx.expected("tiles258_2052x128")[0]
    assert ((cand[:, 0] * 128 + cand[:, 1]) >= 256 * C.TILE).sum() >= 2 and ((cand[:, 0] * 128 + cand[:, 1]) < 256 * C.TILE).sum() > 100
    cand = fx.expected("tiles257_513x512")[0]
    assert not ((cand[:, 0] * 512 + cand[:, 1]) >= 256 * C.TILE).any() and len(cand) > 100
    # candidates on both sides of every block seam of the seam cases
    for s in C.SEAM_SIDES:
        c = C.case("seam_k%d_u16" % s)
        r = C.route(c)
        cand = fx.expected(c.name)[0]
        assert len(set((cand[:, 0] // r["tile"][0]).tolist())) == r["blocks"][0], c.name
        assert len(set((cand[:, 1] // r["tile"][1]).tolist())) == r["blocks"][1], c.name
    # fields without candidates between fields with some, beyond field 256 too
    counts = fx.expected("fields257_8x8")[1]
    assert counts[254] == 0 and counts[255] > 0 and counts[256] > 0 and (counts == 0).sum() > 40 and (counts > 0).sum() > 150
    assert [bool(n) for n in fx.expected("fields3_24x40")[1]] == [True, False, True]
    # one entry off by one changes the list
    for which in ("corner", "inner"):
        assert not C.is_ring(C.almost_ring(which)) and C.is_ring(C.DEFAULT_K)
        a, b = fx.expected("ring_%s" % which), fx.expected("ring_%s_default" % which)
        assert not np.array_equal(a[0], b[0]) and a[2][0] != b[2][0], which
    # pixel formats: the binary16 frame holds the uint16 frame's values wherever binary16 can
    assert fx.expected("seam_k5_f16")[1] == fx.expected("seam_k5_u16")[1]


def test_threshold_edges(fx):
    cand, counts, thr, _ = fx.expected("tie_c0")
    assert thr.view(np.float64)[0] == 3.0 and cand.tolist() == [[3, 3], [3, 11], [11, 4], [12, 12]]      # `not cm < thr`: the tie is a candidate
    cand, counts, thr, _ = fx.expected("tie_c1e-9")
    assert thr.view(np.float64)[0] > 3.0 and cand.tolist() == [[3, 3], [3, 11], [11, 4]]
    assert np.isposinf(fx.expected("cstd_inf")[2].view(np.float64)[0])
    assert np.isnan(fx.expected("cstd_nan")[2].view(np.float64)[0])
    assert np.isnan(fx.expected("flat_cstd_inf")[2].view(np.float64)[0])          # inf * 0
    assert fx.expected("flat33")[2].view(np.float64)[0] == 0.0
    assert fx.expected("cstd_neg1")[2].view(np.float64)[0] < 0.0
    assert np.isfinite(fx.expected("abi_1x7")[2].view(np.float64)[0]) and fx.expected("abi_1x7")[1].tolist() == [0]


def oracle_image(c, f):
    return c.images[f].astype(np.int64).astype(np.uint16) if c.fmt == "f16" else c.images[f]


def test_orientation_is_pinned(fx):
    """The reference's list under the flipped and under the transposed matrix (recorded as checksums) differs from the recorded
    list, and the oracle gives each of the three."""
    import oracle as O
    for name in C.ORIENTED:
        c = C.case(name)
        base = C.cand_crc(fx.expected(name)[0])
        flip, transp = fx.orient[name]
        assert len({base, flip, transp}) == 3, name
        for K, want in ((c.K, base), (C.oriented(c)["flip"], flip), (C.oriented(c)["transp"], transp)):
            assert C.cand_crc(O.candidates(oracle_image(c, 0), c.med, K, c.c_std)) == want, name


def test_oracle_agrees_with_the_reference(fx):
    import oracle as O
    refused = []
    for c in C.cases():
        if c.name == "seam_k5_floatK":          # (the oracle takes integer matrices, like the GPU path)
            continue
        cand, counts, thr, _ = fx.expected(c.name)
        off = np.concatenate([[0], np.cumsum(counts)])
        for f in range(len(c.images)):
            try:
                hw, cm, t = O.candidates(oracle_image(c, f), c.med, c.K, c.c_std, return_cm=True)
            except ValueError as e:
                assert str(e) == "oracle candidates error -3", (c.name, e)
                refused.append(c.name)
                continue
            assert np.array_equal(hw, cand[off[f]:off[f + 1]]), (c.name, f)
            assert bits_equal(t, thr[f:f + 1].view(np.float64)).all(), (c.name, f, t, thr[f])
            if c.name.startswith("sum_"):
                assert sum(int(v) for v in cm.ravel()) == C.SUMS[2]
    assert refused == ["sum_reach"] == [c.name for c in C.cases() if "refuse" in c.expect]


def test_detect_params_takes_integer_matrices_only(fx):
    """The reference correlates a floating-point matrix in floating point and truncates the response; the GPU path works on
    integers.  A matrix with a fractional entry used to be truncated silently (0.5 -> 0); recorded on the seam frame, even an
    integral-valued float64 matrix does not give the reference the integer matrix's answer (scipy takes the FFT route), so
    every floating-point matrix is refused before anything is launched."""
    from fluorosequencingimageanalysis_amd import engine as E
    a, b = fx.expected("seam_k5_floatK"), fx.expected("seam_k5_u16")
    assert C.case("seam_k5_floatK").K.dtype == np.float64 and np.array_equal(C.case("seam_k5_floatK").K, C.case("seam_k5_u16").K)
    assert not (np.array_equal(a[0], b[0]) and a[2][0] == b[2][0])
    half = C.DEFAULT_K.astype(np.float64)
    half[2, 2] += 0.5
    for K in (half, C.DEFAULT_K.astype(np.float64), C.DEFAULT_K.astype(np.float32), C.DEFAULT_K + 0j,
              np.full((3, 3), np.nan), [[0.5]]):
        with pytest.raises(NotImplementedError, match="integer correlation matrices"):
            E.detect_params(5, K, 2)
    for K in (C.DEFAULT_K, C.DEFAULT_K.astype(np.int16), C.DEFAULT_K.tolist(), np.ones((3, 3), bool), C.DEFAULT_K.astype(np.uint32) % 7):
        p = E.detect_params(5, K, 2)
        assert [int(p.K[i]) for i in range(p.ksz ** 2)] == np.asarray(K).astype(np.int64).ravel().tolist()
    with pytest.raises(ValueError):
        E.detect_params(5, np.ones((4, 4)), 2)          # (the reference's own check comes first, pflib.py:236-239)
