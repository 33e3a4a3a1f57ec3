"""Cases of the candidate-detection limit tests: tests/golden/detect_limits.npz (oracle/gen_golden.py --only detect_limits:
the reference's own _psf_candidates on every field of every case, the threshold recomputed by the reference's expressions)
and the route a case takes through fsq_detect (csrc/fsq_detect.hip), restated here from its dispatch so that the tests can
say which kernel, how many blocks, tiles and chunks a case runs without asking the code under test.  No torch, no GPU.

A case is a stack of same-shaped frames (most hold one), a median window, a correlation matrix, c_std and a pixel format;
`expect` says, per field, whether the case is meant to have some candidates ("some": at least one, fewer than all interior
pixels), every interior pixel ("all"), none ("none"), or to be refused by the GPU path ("refuse": the response sums to 2^53 or
more, where numpy.mean is no longer the exact integer mean).

What the groups are for:
  seam_*      23 x 131: not a multiple of any K1 tile (16x64, 14x62, 12x60, 10x58, 8x56) and 2 x 3 blocks of each; asymmetric
              matrices of side 1..9 at the default median through k1_response5<false> (uint16 and binary16 pixels) and
              through the generic kernel (uint32 pixels); one case for each other instantiation of K1.  For sides 3..9 the
              fixture also holds checksums of the reference's lists for the matrix flipped in both axes and transposed: they
              differ from the recorded list, so a convolution or a transposed index fails.  (A 1 x 1 matrix has no orientation.)
  lowent_*    pixel values 0..3: both median networks see mostly ties.
  ring_*      the default matrix with one entry off by one: not ring-symmetric, so it must take k1_response5<false>; c_std is chosen
              so that the candidate list differs from the default matrix's on the same frame (RING_CSTD).
  sum_*       20 x 20 zero frames with isolated saturated pixels under a constant 15 x 15 matrix: the response sums into
              [2^52, 2^53) and, with one more hot pixel, to 2^53 or more (SUMS, computed in Python integers below).
  tie_*, cstd_*, flat*   the threshold compare: a response exactly on the threshold, c_std of 0, -1, inf, NaN, NaN thresholds.
  chunk_*, abi_1x7       last chunks of the variance's 8192-element blocks of 3, 8, 128, 129, 8191 elements and none ragged.
  fields*, tiles*        more than 256 fields, an empty field between full ones, more than 256 tiles in a field.  In a
              513 x 512 frame tile 256 is the last image row, which holds no interior pixel: the second round of k2_scan_field
              runs there on a count of zero.  tiles258_2052x128 has the same number of pixels and two spots in tile 256.
"""
import os
import zlib

import numpy as np

from fluorosequencingimageanalysis_amd import synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLD, "detect_limits.npz")

DEFAULT_K = np.array([[-5935, -5935, -5935, -5935, -5935],
                      [-5935, 8027, 8027, 8027, -5935],
                      [-5935, 8027, 30742, 8027, -5935],
                      [-5935, 8027, 8027, 8027, -5935],
                      [-5935, -5935, -5935, -5935, -5935]], dtype=np.int64)
SEAM_SHAPE = (23, 131)
SEAM_SIDES = (1, 3, 5, 7, 9)
# c_std at which the seam frame's list differs between the default matrix and the one with an entry off by one: the
# threshold is put a quarter of the way between the two responses of the pixel the changed entry moves most
RING_CSTD = {"corner": 5.53604951978246, "inner": 8.48511418559302}
CHUNK_SHAPES = ((5, 1639), (8, 1025), (64, 130), (53, 157), (127, 129), (64, 128))
CHUNK, TILE = 8192, 1024


class Case:
    def __init__(self, name, images, med=5, K=DEFAULT_K, c_std=2.0, fmt="u16", expect="some", crafted=False, abi_only=False):
        images = np.asarray(images)
        if images.ndim == 2:
            images = images[None]
        assert images.dtype == {"u16": np.uint16, "f16": np.float16, "u32": np.uint32}[fmt], name
        self.name, self.images, self.med, self.K, self.c_std, self.fmt = name, np.ascontiguousarray(images), int(med), np.asarray(K), c_std, fmt
        self.expect = [expect] * len(images) if isinstance(expect, str) else list(expect)
        self.crafted, self.abi_only = crafted, abi_only
        assert len(self.expect) == len(images)

    @property
    def shape(self):
        return self.images.shape[1:]

    def integer_images(self):
        """What the reference's image.astype(np.int64) sees."""
        return self.images.astype(np.int64)

    def crc(self):
        return zlib.crc32(self.images.tobytes())


def seam_frame():
    return synth.make_hard_field(305, SEAM_SHAPE, 20)      # (candidates in every block row and column of every tile shape)


def seam_matrix(side):
    """Asymmetric random integers with a dominant centre (so that spots, not noise, are found)."""
    if side == 1:
        return np.array([[7]], dtype=np.int64)
    rng = np.random.default_rng(9100 + side)
    K = rng.integers(-3000, 5000, (side, side)).astype(np.int64)
    K[side // 2, side // 2] = 30000
    return K


def almost_ring(which):
    K = DEFAULT_K.copy()
    if which == "corner":
        K[4, 4] += 1
    else:
        K[1, 2] -= 1
    return K


SUM_K = np.full((15, 15), 2 ** 28, dtype=np.int64)
SUM_HOT = ((6, 6), (13, 13), (6, 13))               # the first two: below 2^53; all three: at or above


def sum_frame(n_hot):
    img = np.zeros((20, 20), np.uint16)
    for h, w in SUM_HOT[:n_hot]:
        img[h, w] = 65535
    return img


def response_int(img, med, K):
    """The int64 response image of pflib.py:241-248 for an odd median window, in exact integer arithmetic (numpy only):
    used for the sums of the 2^53 cases, never as the expected answer of a test."""
    img = np.asarray(img, dtype=np.int64)
    assert med % 2 == 1
    r = med // 2
    pad = np.pad(img, r, mode="symmetric")                   # (numpy's 'symmetric' is scipy.ndimage's 'reflect')
    win = np.lib.stride_tricks.sliding_window_view(pad, (med, med)).reshape(img.shape + (med * med,))
    m = np.sort(win, axis=-1)[..., med * med // 2]
    mf = img - np.minimum(m, img)
    c = K.shape[0] // 2
    zp = np.pad(mf, c)
    cm = np.zeros(img.shape, dtype=object)
    for a in range(K.shape[0]):
        for b in range(K.shape[1]):
            cm = cm + zp[a:a + img.shape[0], b:b + img.shape[1]].astype(object) * int(K[a, b])
    return np.maximum(cm, 0)


def static_checks(case):
    """The two static domain checks of fsq_detect, restated: one pixel's window sum fits an int64, a field's response sum
    fits an unsigned 64-bit word.  True = the call is let through to the kernels."""
    K = [int(v) for v in case.K.ravel()]
    kabs, kmax = sum(abs(v) for v in K), sum(v for v in K if v > 0)
    bits = 16 if case.fmt != "u32" else max(1, int(case.images.max()).bit_length())
    pmax = 2 ** bits - 1
    H, W = case.shape
    return kabs * pmax < 2 ** 63 - 1 and kmax * pmax * H * W < 2 ** 64 - 1


SUMS = {n: int(response_int(sum_frame(n), 5, SUM_K).sum()) for n in (2, 3)}
assert SUMS[2] == 2 * 196 * 2 ** 28 * 65535 and SUMS[3] == 3 * 196 * 2 ** 28 * 65535
assert 2 ** 52 <= SUMS[2] < 2 ** 53 <= SUMS[3]


def tie_frame():
    img = np.full((16, 16), 100, np.uint16)
    for (h, w), e in zip(((3, 3), (3, 11), (11, 4), (12, 12)), (255, 255, 255, 3)):
        img[h, w] += e
    return img


def spot_frame():
    return synth.make_field(77, (32, 48), 5)


def fields257():
    """257 frames of 8 x 8.  Most hold one bright interior pixel on noise; every fifth (and the last but two) holds a
    saturated corner pixel instead, whose response lifts the threshold above everything inside."""
    rng = np.random.default_rng(257)
    imgs = rng.integers(90, 130, (257, 8, 8)).astype(np.uint16)
    expect = []
    for f in range(257):
        if f % 5 == 2 or f == 254:
            imgs[f, 0, 0] = 65535
            expect.append("none")
        else:
            imgs[f, rng.integers(2, 6), rng.integers(2, 6)] = 4000
            expect.append("some")
    return imgs, expect


def fields3():
    a, c = synth.make_hard_field(311, (24, 40), 8), synth.make_hard_field(312, (24, 40), 8)
    b = np.full((24, 40), 100, np.uint16)
    b[0, 0] = 65535
    return np.stack([a, b, c]), ["some", "none", "some"]


def tall_frame():
    """2052 x 128 (as many pixels as 513 x 512): spots all over and two in rows 2048 and 2049, which lie in tile 256."""
    img = synth.make_field(88, (2052, 128), 40).astype(np.int64)
    yy, xx = np.mgrid[0:2052, 0:128]
    for h, w in ((2048.3, 30.2), (2049.1, 97.6)):
        img += np.rint(2500 * np.exp(-((yy - h) ** 2 + (xx - w) ** 2) / (2 * 1.1 ** 2))).astype(np.int64)
    return np.minimum(img, 65535).astype(np.uint16)


_CASES = None


def cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    S = seam_frame()
    S16 = np.minimum(S, 65504).astype(np.float16)            # integer-valued: binary16 holds every integer up to 2048, and only integers above 1024
    S32 = S.astype(np.uint32) * 37 + 70000
    assert np.array_equal(S16.astype(np.float64), np.rint(S16.astype(np.float64)))
    for s in SEAM_SIDES:
        out.append(Case("seam_k%d_u16" % s, S, 5, seam_matrix(s)))
        out.append(Case("seam_k%d_f16" % s, S16, 5, seam_matrix(s), fmt="f16"))
        out.append(Case("seam_k%d_u32" % s, S32, 5, seam_matrix(s), fmt="u32"))
    out.append(Case("seam_default_u16", S))
    out.append(Case("seam_k11_u16", S, 5, np.pad(seam_matrix(9), 1, constant_values=-200)))
    out.append(Case("seam_med3_k3_u16", S, 3, seam_matrix(3)))
    out.append(Case("seam_med4_k3_u32", S32, 4, seam_matrix(3), fmt="u32"))
    out.append(Case("seam_k5_floatK", S, 5, seam_matrix(5).astype(np.float64)))
    low = np.random.default_rng(4).integers(0, 4, SEAM_SHAPE).astype(np.uint16)
    out.append(Case("lowent_k5_u16", low, 5, seam_matrix(5)))
    out.append(Case("lowent_k9_u16", low, 5, seam_matrix(9)))
    out.append(Case("lowent_k5_u32", low.astype(np.uint32), 5, seam_matrix(5), fmt="u32"))
    for which in ("corner", "inner"):
        out.append(Case("ring_%s" % which, S, 5, almost_ring(which), RING_CSTD[which]))
        out.append(Case("ring_%s_default" % which, S, c_std=RING_CSTD[which]))
    out.append(Case("sum_below", sum_frame(2), 5, SUM_K, 1.0, crafted=True))
    out.append(Case("sum_reach", sum_frame(3), 5, SUM_K, 1.0, expect="refuse", crafted=True))
    one = np.array([[1]], dtype=np.int64)
    out.append(Case("tie_c0", tie_frame(), 3, one, 0.0, crafted=True))
    out.append(Case("tie_c1e-9", tie_frame(), 3, one, 1e-9, crafted=True))
    out.append(Case("cstd_neg1", spot_frame(), c_std=-1.0, expect="all"))        # (sparse spots: the deviation exceeds the mean)
    out.append(Case("cstd_inf", spot_frame(), c_std=float("inf"), expect="none"))
    out.append(Case("cstd_nan", spot_frame(), c_std=float("nan"), expect="all"))
    out.append(Case("flat_cstd_inf", np.full((16, 16), 100, np.uint16), c_std=float("inf"), expect="all", crafted=True))
    out.append(Case("flat33", np.full((33, 33), 100, np.uint16), expect="all", crafted=True))
    for k, (H, W) in enumerate(CHUNK_SHAPES):
        out.append(Case("chunk_%dx%d" % (H, W), synth.make_hard_field(400 + k, (H, W), max(6, H * W // 400))))
    out.append(Case("abi_1x7", np.array([[100, 104, 900, 101, 99, 100, 103]], np.uint16), expect="none", crafted=True, abi_only=True))
    imgs, expect = fields257()
    out.append(Case("fields257_8x8", imgs, expect=expect))
    imgs, expect = fields3()
    out.append(Case("fields3_24x40", imgs, expect=expect))
    out.append(Case("tiles257_513x512", synth.make_field(87, (513, 512), 50)))
    out.append(Case("tiles258_2052x128", tall_frame()))
    assert len({c.name for c in out}) == len(out)
    _CASES = out
    return out


def case(name):
    return next(c for c in cases() if c.name == name)


def oriented(c):
    """The matrices whose lists must differ from the recorded one: flipped in both axes (a convolution), transposed."""
    return {"flip": c.K[::-1, ::-1], "transp": c.K.T}


ORIENTED = tuple("seam_k%d_%s" % (s, f) for s in SEAM_SIDES if s > 1 for f in ("u16", "f16", "u32"))


def is_ring(K):
    K = np.asarray(K)
    return K.shape == (5, 5) and all(K[a, b] == (K[0, 0], K[1, 1], K[2, 2])[2 - max(abs(a - 2), abs(b - 2))] for a in range(5) for b in range(5))


def route(c, r03=False):
    """fsq_detect's dispatch for a case (r03: with FSQ_DETECT_R03 set): the K1 instantiation, its grid of blocks per field,
    the tiles of 1024 pixels and the 8192-element chunks of a field, the length of the last chunk, the fields."""
    H, W = c.shape
    ksz, kc = c.K.shape[0], (c.K.shape[0] - 1) // 2
    th, tw = 16, 64
    if c.fmt == "u32":
        kernel = "k1_response<%s,u32>" % ("true" if c.med == 5 else "false")
    elif c.med == 5 and ksz <= 9 and not r03:
        kernel = "k1_response5<%s>" % ("true" if is_ring(c.K) else "false")
        th, tw = 16 - 2 * kc, 64 - 2 * kc
    else:
        kernel = "k1_response<%s,u16>" % ("true" if c.med == 5 else "false")
    N = H * W
    chunks = -(-N // CHUNK)
    return dict(kernel=kernel, tile=(th, tw), blocks=(-(-H // th), -(-W // tw)), tiles=-(-N // TILE), chunks=chunks,
                last_chunk=N - CHUNK * (chunks - 1), fields=len(c.images))


def chunk_class(n):
    return "<8" if n < 8 else "8" if n == 8 else "(8,128]" if n <= 128 else "(128,8192)" if n < CHUNK else "full"


def interior(c):
    H, W = c.shape
    return max(H - 4, 0) * max(W - 4, 0)


class Fixture:
    def __init__(self):
        g = np.load(FIXTURE)
        self.names = [str(n) for n in g["names"]]
        self.n_fields = g["n_fields"]
        self.counts, self.thr_bits, self.cand = g["counts"], g["thr_bits"], g["cand"]
        self.exc, self.crc = [str(e) for e in g["exc"]], g["crc"]
        self.f0 = np.concatenate([[0], np.cumsum(self.n_fields)])
        self.c0 = np.concatenate([[0], np.cumsum(self.counts)])
        self.orient = {str(n): (int(a), int(b)) for n, a, b in zip(g["orient_names"], g["flip_crc"], g["transp_crc"])}
        off = np.concatenate([[0], np.cumsum(np.prod(g["pixel_shapes"], axis=1))])
        self.pixels = {str(n): g["pixels"][off[i]:off[i + 1]].reshape(g["pixel_shapes"][i]) for i, n in enumerate(g["pixel_names"])}

    def expected(self, name):
        """(candidates int32[total, 2] field after field, counts int32[n_fields], thresholds as uint64 bit patterns[n_fields],
        name of the exception class the reference raised or '')."""
        i = self.names.index(name)
        f0, f1 = self.f0[i], self.f0[i + 1]
        return (self.cand[self.c0[f0]:self.c0[f1]].astype(np.int32), self.counts[f0:f1].astype(np.int32), self.thr_bits[f0:f1], self.exc[i])


_FIX = None


def fixture():
    global _FIX
    if _FIX is None:
        _FIX = Fixture()
    return _FIX


def cand_crc(cand):
    return zlib.crc32(np.ascontiguousarray(cand, dtype=np.int16).tobytes())


def triples(cand, counts):
    """(h, w) lists field after field -> the (field, h, w) triples fsq_detect writes."""
    f = np.repeat(np.arange(len(counts), dtype=np.int32), counts)
    return np.column_stack([f, np.asarray(cand, dtype=np.int32).reshape(-1, 2)]).astype(np.int32)
