"""Cases of the registration limit tests: tests/golden/registration_limits.npz (oracle/gen_golden.py --only reg_limits, the
reference's own phase_correlate on every pair at every factor, the oracle's answer next to it) and the path the port takes
for a shape and a factor, restated from reg_layout (csrc/fsq_register.hip) so that the tests can say which branch a case
runs without asking the code under test.

Comparison rule (tests/test_gpu_register.py): shifts equal exactly, NaN where NaN; diffphase within 1e-9 absolute; error
within 1e-9 absolute where the recorded error is >= 1e-4, else error^2 within 1e-12 absolute (the error of an exact shift
is the square root of rounding noise).  The reference and the oracle - two fp64 implementations, neither under test -
differ over the whole fixture by at most 1.3e-16 in diffphase, 7.3e-13 in error and 1.2e-14 in error^2, so those bounds
leave two to seven orders of magnitude of room and none had to be derived from the spread.

Pairs flagged `fragile` (one row or one column of non-blank content at upsample_factor > 1, 32 of 855): the reference
divides the upsampled grid by mid_row * mid_col = 0, every element becomes +-inf or NaN, numpy's argmax takes the first NaN,
and NaN stands exactly where a part of the undivided grid is exactly zero.  At the correlation peak the imaginary part is
zero in exact arithmetic and a rounding residue in floating point, so whether it is 0.0 or 1e-13 decides the answer along
the long axis: the reference and the oracle already disagree on 8x1_rand (0 against -0.5).  What does not hang on the
residue is held: error is NaN; the shift along the axis of length 1 is exact (all rows resp. columns of the grid are equal,
the first wins: -dftshift / uf); the shift along the long axis is either the whole-pixel shift (the peak's own index, when
the NaN is there or when the residue makes it the first (+inf, +inf)) or `alt`, computed at generation from the signs of
the grid without the peak (the reference's and the oracle's answers are each one of the two); diffphase is NaN or an odd
multiple of pi / 4 (atan2 of two infinities).

No load or store of a new shape leaves its buffer - read off the index expressions of csrc/fsq_register.hip:

  kernel                 index                                   bound                      holds because
  k6_dft_mfma(_half)     r = r0 + lane / 16, r0 += 4             r < rows                   rows % 4 == 0 (16, 36, 48, 80)
    (16x16 36x48         c = 16 bx + lane % 16                   c < cols                   cols % 16 == 0 (16, 48, 64, 96), grid.x = cols / 16
     48x64 80x96,        rkT[r][m0 + lane % 16], m0 = 32 by      m0 + 15 < Mp               Mp % 16 == 0, grid.y = ceil(Mp / 32) => m0 < Mp
     Mp <= H, W)         rkT[r][m0 + 16 + lane % 16]             only if m0 + 16 < Mp       `two`; then m0 + 31 < Mp
                         T[m0 + lane / 16 + 4 g (+ 16)][c]       row < Mp                   as above; T holds Mp x cols per pair
                         half spectra: r Wh + c (c < Wh) or      < H Wh                     1 <= W - c <= W - Wh < Wh
                           ((H - r) % H) Wh + (W - c)
    full-spectrum form   rkT in F's slots: pairs H Mp elements   <= pairs H W               Mp <= W (equality at 16x16, Mp = 16)
    (FSQ_REGISTER_Z2Z)   T in G's slots: pairs Mp W elements     <= pairs H W               Mp <= H (equality at 16x16, 48x64 Mp = 48,
                                                                                            80x96 Mp = 80)
  k6_rowkernel           i = r Mp + u < rows Mp                  guard `i >= rows * Mp`
  k6_dft_cols            T[u][c], u < up <= Mp, c < cols         strided loops
  k6_expand_gf           i < H W                                 guard; spectra as above    every shape, W = 1 included (Wh = 1: c < Wh always)
                         out[pair][i]: T holds pairs H W         reg_layout sizes T by      ... FSQ_REGISTER_NO_MFMA included: until this suite the
                         complex                                 the path it will run       layout still kept Mp x W there and the expansion ran
                                                                                            over rkT, U, the sums and the offsets (found by
                                                                                            test_forced_paths[no_mfma]; the layout now reads the switch)
  k6_dftups              Wr[r], r < min(rows, 1536); T[c],       LDS of 1536 + 1536         rows, cols <= 96 < 256: one row chunk, T in LDS,
    (every other shape)  c < cols <= 1536; data[r][c]; out[u][v] complex, fixed             Tg never touched
  k6_argmax_real_part    lo = n part / 16, hi = n (part + 1)/16  i < hi <= n                n < 16: parts with lo == hi read nothing and hand on
                                                                                            (-inf, idx n); part 15 always holds pixel n - 1, so
                                                                                            k6_coarse ends on idx < n (the sentinel loses to any
                                                                                            number), and idx / W < H
  k6_argmax, k6_fine     i < up up; p < n_pairs                  strided loop; guard        n_pairs = 63, 64, 65: one resp. two blocks of 64
  hipFFT, length 1       D2Z of H x 1 / 1 x W / 1 x 1: in H W    buffers sized H W and      Wh = W / 2 + 1 >= 1; a shape hipFFT has no plan for
                         doubles, out H Wh complex               H Wh by reg_layout         comes back as FSQ_ENOTIMPL before any launch
"""
import math
import os

import numpy as np

from _util import GOLD

SHAPES = ((16, 16), (36, 48), (48, 64), (80, 96), (50, 48), (30, 50), (47, 61))
TINY = ((1, 1), (1, 8), (8, 1), (2, 8), (3, 7), (2, 2), (3, 3), (4, 4), (5, 5))
FACTORS = (1, 2, 3, 10, 11, 21, 22, 32, 43)


def layout(H, W, uf):
    """reg_layout's path choice: (up, Mp, mfma, M-tiles of 16 rows per column of blocks)."""
    up = math.ceil(uf * 1.5)
    Mp = 16 * ((up + 15) // 16)
    mfma = uf > 1 and W % 16 == 0 and H % 4 == 0 and Mp <= W and Mp <= H
    return up, Mp, mfma, Mp // 16


class Fixture:
    def __init__(self):
        g = np.load(os.path.join(GOLD, "registration_limits.npz"))
        self.names = [str(n) for n in g["names"]]
        self.factors = tuple(int(f) for f in g["factors"])
        self.out, self.spread, self.fragile, self.alt = g["out"], g["spread"], g["fragile"], g["alt"]
        self.exc, self.spread_exc = g["exc"], g["spread_exc"]
        off = np.concatenate([[0], np.cumsum(np.prod(g["img_shapes"], axis=1))])
        self.images = {str(k): g["pixels"][off[i]:off[i + 1]].reshape(g["img_shapes"][i]) for i, k in enumerate(g["img_keys"])}
        self.pairs = {n: (self.images[str(a)], self.images[str(b)]) for n, a, b in zip(self.names, g["ref_keys"], g["reg_keys"])}
        assert self.factors == FACTORS

    def shape(self, name):
        return self.pairs[name][0].shape

    def of_shape(self, H, W):
        return [n for n in self.names if self.shape(n) == (H, W)]

    def expected(self, name, uf):
        """(recorded tuple, name of the exception class the reference raised or '', keywords of assert_matches)."""
        i, k = self.names.index(name), self.factors.index(uf)
        kw = {}
        if self.fragile[i, k]:
            kw = dict(fragile=True, whole=self.out[i, 0, :2], alt=self.alt[i, k], unit_axis=0 if self.shape(name)[0] == 1 else 1)
        return self.out[i, k], str(self.exc[i, k]), kw


_FIX = None


def fixture():
    global _FIX
    if _FIX is None:
        _FIX = Fixture()
    return _FIX


def _same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def assert_matches(got, exp, what, fragile=False, whole=None, alt=None, unit_axis=None):
    """The comparison rule of the module docstring; `got`, `exp` = (row_shift, col_shift, error, diffphase).  For a
    fragile pair, `whole` holds its recorded whole-pixel shifts, `alt` the other candidate and `unit_axis` is the axis of
    length 1."""
    got, exp = [float(x) for x in got], [float(x) for x in exp]
    if fragile:
        assert np.isnan(exp[2]) and np.isnan(got[2]), (what, got, exp)
        assert got[unit_axis] == exp[unit_axis], (what, got, exp)
        long_axis = 1 - unit_axis
        assert got[long_axis] in (float(alt[long_axis]), float(whole[long_axis])), (what, got, exp, whole, alt)
        assert np.isnan(got[3]) or abs(abs(got[3]) / (math.pi / 4) % 2 - 1) < 1e-12, (what, got, exp)
        return
    assert _same(got[0], exp[0]) and _same(got[1], exp[1]), (what, got, exp)
    assert _same(got[3], exp[3]) or abs(got[3] - exp[3]) <= 1e-9, (what, got, exp)
    if np.isnan(exp[2]) or np.isnan(got[2]):
        assert np.isnan(exp[2]) and np.isnan(got[2]), (what, got, exp)
    elif exp[2] >= 1e-4:
        assert abs(got[2] - exp[2]) <= 1e-9, (what, got, exp)
    else:
        assert abs(got[2] ** 2 - exp[2] ** 2) <= 1e-12, (what, got, exp)
