"""CPU checks that tests/golden/registration_limits.npz is not vacuous: read from the recorded reference output and from
the path predicate restated in _register_limit_cases.layout, never from the code under test, it holds a case for every
branch of csrc/fsq_register.hip that the three factors of registration.npz (1, 20, 100) leave unrun; and the oracle
(oracle/fsq_register_oracle.c) is pinned to the reference at the new factors, as test_oracle_golden.py pins it at the old."""
import os

import numpy as np
import pytest

import _register_limit_cases as C
from _util import GOLD


@pytest.fixture(scope="module")
def fx():
    return C.fixture()


def test_fixture_holds_every_case_at_every_factor(fx):
    assert os.path.getsize(os.path.join(GOLD, "registration_limits.npz")) < 200_000
    assert fx.out.shape == (len(fx.names), len(C.FACTORS), 4) == fx.spread.shape
    for H, W in C.SHAPES:
        kinds = {n.split("_", 1)[1] for n in fx.of_shape(H, W)}
        want = {"int", "zero", "blank", "blankref", "blankreg", "sub0", "sub1", "sub2", "sub3"}
        if H % 2 == 0 and W % 2 == 0:
            want.add("half")
        assert kinds == want, ((H, W), kinds)
    for H, W in C.TINY:
        kinds = {n.split("_", 1)[1] for n in fx.of_shape(H, W)}
        assert kinds == ({"blank", "7v9"} if H * W == 1 else {"blank", "roll", "rand"}), ((H, W), kinds)
    for n in fx.names:
        a, b = fx.pairs[n]
        assert a.dtype == np.uint16 and b.dtype == np.uint16 and a.shape == b.shape
        kind = n.split("_", 1)[1]
        assert (kind == "blank") == (not a.any() and not b.any()), n
        if kind == "zero":
            assert np.array_equal(a, b)
    # the reference raised nowhere (one-row and one-column images divide by zero quietly): nothing to refuse
    assert not fx.exc.any() and not fx.spread_exc.any()


def test_recorded_answers_at_the_edges(fx):
    """What the issue of these tests reads off the reference, as recorded: blank pairs answer (0, 0, nan, 0) at factor 1 and
    (-dftshift / uf, -dftshift / uf, nan, -+0) above it - (-0.75, -0.75) at 10 and 22 and 32, where `up` is even, less where
    it is odd; a shift of exactly half the size keeps its sign (`row_max > mid_row` is strict); H or W in {2, 3} zeroes
    that axis at uf > 1; one-row and one-column images give a NaN error at uf > 1."""
    for n in fx.names:
        H, W = fx.shape(n)
        kind = n.split("_", 1)[1]
        for uf in C.FACTORS:
            e, _, _ = fx.expected(n, uf)
            up = C.layout(H, W, uf)[0]
            if kind in ("blank", "blankref", "blankreg"):
                want = [0.0, 0.0] if uf == 1 else [0.0 if d // 2 == 1 else -(up // 2) / uf for d in (H, W)]
                assert e[:2].tolist() == want and np.isnan(e[2]), (n, uf, e)
                assert (e[3] == 0 and (uf == 1 or np.signbit(e[3]))) or (np.isnan(e[3]) and min(H, W) == 1 and uf > 1), (n, uf, e)
            if kind == "half":
                assert e[0] == H // 2 and e[1] == W // 2, (n, uf, e)
            if uf > 1 and kind != "blank":
                assert (H // 2 != 1 or e[0] == 0) and (W // 2 != 1 or e[1] == 0), (n, uf, e)
            if uf > 1 and min(H, W) == 1:
                assert np.isnan(e[2]), (n, uf, e)
            assert fx.expected(n, uf)[2].get("fragile", False) == (uf > 1 and min(H, W) == 1 and H * W > 1 and kind != "blank")
    assert any(C.layout(1, 1, uf)[0] % 2 for uf in C.FACTORS) and any(C.layout(1, 1, uf)[0] % 2 == 0 for uf in C.FACTORS[1:])


def test_path_coverage():
    """Every branch named by the path predicate has a (shape, factor) in the table, and each of those shapes stands on the
    vector-ALU side at another factor."""
    cases = [((H, W), uf) + C.layout(H, W, uf) for H, W in C.SHAPES + C.TINY for uf in C.FACTORS if uf > 1]
    mfma = [c for c in cases if c[4]]
    valu = {c[0] for c in cases if not c[4]}
    assert {c[3] for c in cases} == {16, 32, 48, 80}
    assert [(c[2], c[3]) for c in cases if c[0] == (80, 96)] == [(3, 16), (5, 16), (15, 16), (17, 32), (32, 32), (33, 48), (48, 48), (65, 80)]

    def covered(pred, other_side=True):
        hit = [c for c in mfma if pred(c)]
        assert hit, "no MFMA case"
        assert not other_side or any(c[0] in valu for c in hit), "no such shape on the vector-ALU side"
        return hit

    for Mp in (16, 48, 80):                                     # a single-tile last block: Mp / 16 odd
        # (Mp = 80 fits 80 x 96 alone, which the predicate sends to the matrix cores at every factor up to 43: its
        # vector-ALU side is the forced one, FSQ_REGISTER_NO_MFMA, in test_gpu_register_limits)
        covered(lambda c, Mp=Mp: c[3] == Mp and c[5] % 2 == 1, other_side=Mp != 80)
    covered(lambda c: c[5] % 2 == 0)                            # ... and only full blocks
    covered(lambda c: c[3] == c[0][0])                          # Mp == H
    covered(lambda c: c[3] == c[0][1])                          # Mp == W
    covered(lambda c: c[3] == c[0][0] and c[3] < c[0][1] and c[5] % 2 == 1)
    covered(lambda c: c[2] == c[3])                             # no padded row of rkT
    covered(lambda c: c[2] % 16 == 1)                           # fifteen padded rows next to one live row
    covered(lambda c: c[2] < c[3] and c[5] % 2 == 1)            # padded rows in the single tile of the last block
    covered(lambda c: c[0][0] % 4 == 0 and c[0][0] % 16 != 0)   # H % 4 == 0, H % 16 != 0
    assert {c[2] % 2 for c in mfma} == {0, 1} and {c[2] % 2 for c in cases if not c[4]} == {0, 1}     # odd and even `up`
    # the vector-ALU side for each reason: H % 4, W % 16, Mp > H, Mp > W, and shapes that fit nothing
    by = {s: [c for c in cases if c[0] == s] for s in C.SHAPES}
    assert not any(c[4] for s in ((50, 48), (30, 50), (47, 61)) for c in by[s])
    assert [c[1] for c in by[(16, 16)] if c[4]] == [2, 3, 10] and [c[1] for c in by[(36, 48)] if c[4]] == [2, 3, 10, 11, 21]
    assert [c[1] for c in by[(48, 64)] if not c[4]] == [43] and all(c[4] for c in by[(80, 96)])
    assert not any(c[4] for c in cases if c[0] in C.TINY)


def test_reachability(fx):
    """The upsampled peak of the recorded answers, dftshift + (shift - whole-pixel shift) * uf, lies in the first and in the
    last 16-row tile at uf = 32 (rows and columns alike) on each MFMA shape of that factor: rows 32-47 are the single tile
    of the last block (up = Mp = 48).  (At uf = 22 and 43 the single tile holds one live row, 32 resp. 64, more than half a
    pixel from the centre: the peak cannot stand there, a wrong value there can only win by being large; at uf <= 10 the
    single tile is the whole grid.)"""
    uf = 32
    up, k = C.layout(80, 96, uf)[0], C.FACTORS.index(uf)
    assert up == 48
    for H, W in ((48, 64), (80, 96)):
        assert C.layout(H, W, uf)[1:] == (48, True, 3)
        idx = [fx.names.index(n) for n in fx.of_shape(H, W) if "_sub" in n]
        for ax in (0, 1):
            peak = up // 2 + (fx.out[idx, k, ax] - fx.out[idx, 0, ax]) * uf
            assert np.array_equal(peak, np.rint(peak)) and (peak >= 0).all() and (peak < up).all()
            assert (peak < 16).any() and (peak >= 32).any() and ((peak >= 16) & (peak < 32)).any(), ((H, W), ax, peak)


def test_oracle_agrees_with_the_reference(fx):
    import oracle as O
    worst = np.zeros(3)
    for i, n in enumerate(fx.names):
        a, b = fx.pairs[n]
        for k, uf in enumerate(C.FACTORS):
            e, exc, kw = fx.expected(n, uf)
            r = O.phase_correlate(a, b, uf)
            C.assert_matches(r, e, (n, uf), **kw)
            C.assert_matches(r, fx.spread[i, k], (n, uf, "spread"), **kw)      # the recorded spread is this oracle's
            if not kw and not np.isnan(e[2]):
                worst = np.maximum(worst, [abs(r[3] - e[3]), abs(r[2] - e[2]) if e[2] >= 1e-4 else 0.0,
                                           abs(r[2] ** 2 - e[2] ** 2) if e[2] < 1e-4 else 0.0])
    # (measured 1.3e-16, 7.3e-13, 1.2e-14, quoted in _register_limit_cases: a tenth of each bound is room enough)
    print("reference against oracle: diffphase %.3g, error %.3g, error^2 %.3g" % tuple(worst))
    assert worst[0] < 1e-10 and worst[1] < 1e-10 and worst[2] < 1e-13, worst
