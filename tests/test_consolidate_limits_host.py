"""CPU tests of the consolidation limit cases (tests/_consolidate_limit_cases.py): the Python restatement and the C oracle's
fsq_o_consolidate against tests/golden/consolidate_limits.npz - what the reference's own loops (pflib.py:441-520) did with every
field, in both rounding modes - and proofs that every case reaches what its name claims.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

import _consolidate_limit_cases as C

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import oracle as O  # noqa: E402

MODES = (("py2", True), ("py3", False))


@pytest.fixture(scope="module")
def fx():
    return C.Fixture()


def oracle_consolidate(c, f, py2):
    h0, w0 = f.centres()
    try:
        keep, key = O.consolidate(f.h, f.w, h0, w0, f.r2(), c.H, c.W, c.thr, c.radius, py2)
    except AssertionError:
        return None
    return keep.tolist(), [tuple(k) for k in key.tolist()]


def test_the_fixture_holds_every_recorded_case(fx):
    want = [c.name for c in C.cases() if c.recorded]
    assert fx.names == want
    assert list(fx.g["n_fields"]) == [len(c.fields) for c in C.cases() if c.recorded]
    assert os.path.getsize(C.FIXTURE) < 100 * 1024


@pytest.mark.parametrize("case", [c for c in C.cases() if c.recorded], ids=lambda c: c.name)
def test_restatement_and_oracle_equal_the_reference(case, fx):
    """Centres and r_2 as the reference held them, bit for bit; the kept candidates in dict order and their keys, or the assert, in
    both rounding modes - from the Python restatement and from fsq_o_consolidate."""
    for u, f in enumerate(case.fields):
        h0, w0 = f.centres()
        hb, wb, rb = fx.field(case.name, u)
        assert np.array_equal(h0.view(np.uint64), hb) and np.array_equal(w0.view(np.uint64), wb), (case.name, u)
        r2, nan = f.r2(), np.isnan(rb.view(np.float64))           # (0 / 0 is a NaN of either sign: its sign is not part of the contract)
        assert np.array_equal(np.isnan(r2), nan) and np.array_equal(r2.view(np.uint64)[~nan], rb[~nan]), (case.name, u)
    for mode, py2 in MODES:
        ref = fx.expected(case.name, py2)
        assert case.expected(py2) == ref, (case.name, mode)
        if case.name == "outside_collision":
            continue                    # (the documented deviation: test_two_keys_outside_the_frame_that_collide)
        assert [oracle_consolidate(case, f, py2) for f in case.fields] == ref, (case.name, mode)


@pytest.mark.parametrize("case", [c for c in C.cases() if not c.recorded], ids=lambda c: c.name)
def test_oracle_equals_the_restatement_where_the_reference_cannot_go(case):
    """r_2 = +inf and -0.0 are no values of pflib.py:463-465; the two restatements must still agree on them."""
    assert all(f.forced for f in case.fields)
    for mode, py2 in MODES:
        assert [oracle_consolidate(case, f, py2) for f in case.fields] == case.expected(py2), (case.name, mode)


def test_two_keys_outside_the_frame_that_collide(fx):
    """The documented deviation (include/fsq.h): the reference's assert fires, the oracle - and the library - keep both."""
    case = C.by_name("outside_collision")
    for mode, py2 in MODES:
        assert fx.expected(case.name, py2) == [None, None]
        for f in case.fields:
            keep, keys = oracle_consolidate(case, f, py2)
            assert keep == [0, 1] and keys[0] == keys[1]
            assert not (0 <= keys[0][0] < case.H and 0 <= keys[0][1] < case.W)


def test_no_other_case_has_a_collision_outside_the_frame():
    """The condition on the generator: in every case the GPU test runs, the entries alive at the re-key whose rounded centre lies
    outside the frame have distinct rounded centres, in both rounding modes."""
    n_outside = 0
    for case in C.cases():
        if not case.gpu:
            continue
        for f in case.fields:
            h0, w0 = f.centres()
            alive = list(C.consolidated_bins(f.h, f.w, h0, w0, f.r2(), case.H, case.W, case.thr, case.radius).values())
            for rnd in (C.py2_round, C.py3_round):
                keys = [(rnd(h0[i]), rnd(w0[i])) for i in alive]
                outside = [k for k in keys if not (0 <= k[0] < case.H and 0 <= k[1] < case.W)]
                assert len(set(outside)) == len(outside), case.name
                n_outside += len(outside)
    assert n_outside > 100


@pytest.mark.parametrize("name", list(C.STOPS))
def test_stopping_rival_sits_at_the_cell_the_case_names(name, fx):
    case = C.by_name(name)
    H, W, radius, ch, cw, _ = C.STOPS[name]
    rw = radius + 2
    ncell = (min(ch + rw + 1, H) - max(0, ch - rw)) * (min(cw + rw + 1, W) - max(0, cw - rw))
    assert (ncell > 64 * C.NGW) == (name in ("stop_r5_full", "stop_r5_top"))      # two passes of the scan
    seen = set()
    for u, (f, cell) in enumerate(zip(case.fields, C.stop_cells(name))):
        turns = C.stopping_turns(f, H, W, case.thr, radius)
        cand = int(np.flatnonzero((f.h == ch) & (f.w == cw))[0])
        assert cand == 0                                                          # (nothing raster-earlier: its turn is the first)
        assert len(turns) == 1 and turns[0][:2] == (cand, cell), (name, u, turns)
        _, _, killed, behind = turns[0]
        centre = (ch - max(0, ch - rw)) * (min(cw + rw + 1, W) - max(0, cw - rw)) + (cw - max(0, cw - rw))
        assert killed >= 1 or cell == centre + 1, (name, u)
        assert behind >= 1 or cell == ncell - 1, (name, u)
        h0, w0 = f.centres()
        for mode, py2 in MODES:
            kept, _ = fx.expected(name, py2)[u]
            # the candidate and the rivals it deleted are gone; the stopping rival and every rival behind it survive
            assert sorted(kept) == list(range(1 + killed, len(f))), (name, u, mode)
        seen.add(cell)
    assert seen == set(C.STOPS[name][5])
    # the seams: the last lane of a 64-lane group and the first of the next, the last cell of a pass and the first of the next
    if name == "stop_r5_full":
        assert {127, 128, 191, 192, ncell - 1} <= seen


def test_turn_cases_are_what_their_names_claim(fx):
    def components(f, radius):
        D = 2 * (radius + 2)
        parent = list(range(len(f)))

        def find(x):
            while parent[x] != x:
                x = parent[x]
            return x
        for i in range(len(f)):
            for j in range(i):
                if abs(int(f.h[i]) - int(f.h[j])) <= D and abs(int(f.w[i]) - int(f.w[j])) <= D:
                    a, b = find(i), find(j)
                    parent[max(a, b)] = min(a, b)
        roots = [find(i) for i in range(len(f))]
        return {r: [i for i in range(len(f)) if roots[i] == r] for r in set(roots)}
    for name, n in (("turn_row_63", 63), ("turn_row_64", 64), ("turn_row_65", 65), ("turn_col_63", 63), ("turn_col_64", 64),
                    ("turn_col_65", 65), ("turn_rows_130", 130), ("turn_snake_130", 130)):
        case = C.by_name(name)
        for f in case.fields:
            assert len(f) == n and list(components(f, case.radius)) == [0]        # one component: root 0, last n - 1
    strips = C.by_name("turn_strips")
    for f in strips.fields:
        assert set((f.w // ((strips.W + 7) // 8)).tolist()) == set(range(8)) and list(components(f, 4)) == [0]
    for f in C.by_name("turn_interleaved").fields:
        comp = components(f, 4)
        assert len(comp) == 2
        a, b = sorted(comp.values())
        assert a[0] < b[0] < a[-1] < b[-1]                                         # the index ranges root .. last interleave
    # every chain both keeps and deletes, and the patterns give different tables
    for name in ("turn_row_65", "turn_col_65", "turn_rows_130", "turn_snake_130", "turn_strips"):
        exp = fx.expected(name, True)
        assert all(e is not None and 0 < len(e[0]) < len(f) for e, f in zip(exp, C.by_name(name).fields))
        assert len({tuple(e[0]) for e in exp}) >= 4


def test_radius_cases_sit_on_both_sides_of_the_circle(fx):
    exp = fx.expected("radius_345", True)
    assert [len(e[0]) for e in exp] == [1, 2, 1, 1, 2]          # on the circle: a rival; one ulp beyond: none; one ulp inside: one
    assert exp[0][0] == [0] and exp[3][0] == [1]
    on, off = C.by_name("radius_345").fields[:2]
    assert off.centres()[0][1] == np.nextafter(on.centres()[0][1], np.inf) == np.nextafter(5.0, np.inf)
    n = [len(e[0]) for e in fx.expected("radius_mantissa", True)]
    assert set(n) == {1, 2} and min(n.count(1), n.count(2)) >= 10
    case = C.by_name("radius_mantissa")
    frac = np.concatenate([np.concatenate(f.centres()) for f in case.fields])
    assert (np.frexp(frac)[0] * 2.0 ** 53 % 2 ** 20 != 0).mean() > 0.9       # full mantissas


def test_r2_cases_are_what_their_names_claim(fx):
    zoo = C.by_name("r2_thr_half").fields
    r2 = [f.r2() for f in zoo]
    assert r2[0][0] == r2[0][1] and np.isnan(r2[2][0]) and np.isnan(r2[3][1]) and r2[5][0] == -np.inf and r2[10][0] == 0.0
    assert np.signbit(C.by_name("r2_forced_thr_zero").fields[6].r2()[0])
    half = fx.expected("r2_thr_half", True)
    assert half[0][0] == [1] and half[1][0] == [1, 2]            # a tie: the one whose turn it is dies (the two others are 5 apart)
    assert half[2][0] == [1] and half[3][0] == [1] and half[4][0] == [1]     # NaN passes the filter and loses every comparison, on either side
    assert half[5][0] == [1] and half[6][0] == [0]               # -inf is filtered at 0.5 ...
    ninf = fx.expected("r2_thr_ninf", True)
    assert ninf[5][0] == [1] and ninf[6][0] == [0] and ninf[7][0] == [1] and ninf[8][0] == [1]       # ... and passes at -inf
    # r_2 equal to the threshold passes; the threshold one ulp above it filters it
    at = C.by_name("r2_thr_equal")
    assert at.thr == at.fields[12].r2()[0] == at.fields[13].r2()[1]
    assert fx.expected("r2_thr_equal", True)[13][0] == [1] and fx.expected("r2_thr_ulp_above", True)[13][0] == []
    assert fx.expected("r2_thr_ulp_below", True)[13][0] == [1]
    assert fx.expected("r2_thr_equal", True)[12][0] != fx.expected("r2_thr_ulp_above", True)[12][0]
    # NaN threshold: nothing is filtered; +inf: only NaN passes
    assert all(len(e[0]) >= 1 for e in fx.expected("r2_thr_nan", True))
    pinf = fx.expected("r2_thr_pinf", True)
    assert pinf[0][0] == [] and pinf[2][0] == [0] and pinf[3][0] == [1] and pinf[4][0] == [1]


def test_rekey_cases_are_what_their_names_claim(fx):
    names = list(C.REKEY_NAMES)
    case = C.by_name("rekey_each")
    H, W = case.H, case.W
    for mode, py2 in MODES:
        exp = dict(zip(names, fx.expected("rekey_each", py2)))
        # which fields assert
        for n in names:
            if n in C.ASSERTING:
                assert exp[n] is None, (n, mode)
            elif n not in C.HALF_INTEGER:
                assert exp[n] is not None, (n, mode)
        # keys outside the frame on all four sides, the negative row among them, kept with their key
        assert exp["out_top"] == ([1, 0], [(7, 7), (-1, 2)])
        assert exp["out_top_far"][1][-1] == (-3, 7) and exp["out_left"][1][-1] == (7, -1)
        assert exp["out_bottom"][1][-1] == (H, 7) and exp["out_right"][1][-1] == (7, W) and exp["out_corner"][1][-1] == (-1, -1)
        keys = exp["out_all_sides"][1]
        assert {(-1, 7), (7, -1), (7, W), (H, 7)} <= set(keys) and len(keys) == 5
        assert exp["only_negative_rows"] == ([0, 1, 2], [(-1, 2), (-2, 7), (-1, 12)])
        # the moves that are allowed
        assert exp["into_empty"] == ([1, 0], [(7, 7), (3, 4)])
        assert exp["into_filtered"] == ([2, 0], [(7, 7), (2, 7)])
        assert exp["into_deleted"] == ([2, 0], [(7, 7), (2, 4)])
        assert exp["into_left_by_earlier"] == ([0, 1], [(7, 2), (2, 2)])
        assert exp["into_left_for_negative_row"] == ([0, 1], [(-1, 2), (2, 2)])
        assert exp["into_left_for_right_of_frame"] == ([0, 1], [(2, W), (2, 12)])
        assert exp["chain_of_three"] ==([0, 1, 2], [(7, 2), (2, 2), (2, 7)])
        assert exp["just_below_half"] == ([1, 0], [(7, 7), (0, 2)])
    assert math.floor(0.49999999999999994 + 0.5) == 1            # (what a rounding by floor(x + 0.5) would make of it)
    # the half-integer cases differ between the two rounding modes
    py2, py3 = (dict(zip(names, fx.expected("rekey_each", m))) for m in (True, False))
    for n in C.HALF_INTEGER:
        assert py2[n] != py3[n], n
    assert py2["minus_half"][1] == [(2, 7), (-1, 2), (7, -1)] and py3["minus_half"][1] == [(2, 7), (0, 2), (7, 0)]
    assert py2["out_half"][1][-1] == (-1, -1) and py3["out_half"][1][-1] == (0, 0)
    for n in names:
        if n not in C.HALF_INTEGER:
            assert py2[n] == py3[n], n
    # embedded: every one of them sits between two ordinary fields
    emb = C.by_name("rekey_embedded")
    assert emb.layout[0] == emb.layout[-1] == 0 and sorted(emb.layout[1::2]) == list(range(1, len(names))) and set(emb.layout[::2]) == {0}


def test_layout_cases_are_what_their_names_claim(fx):
    assert [len(f) for f in C.by_name("layout_5x5").fields] == [1, 1, 1, 1, 1, 0]
    assert [len(e[0]) for e in fx.expected("layout_5x5", True)] == [1, 0, 1, 1, 1, 0]
    assert fx.expected("layout_5x5", True)[2][1] == [(3, 3)] and fx.expected("layout_5x5", False)[2][1] == [(2, 2)]
    assert fx.expected("layout_5x5", True)[3][1] == [(-1, 2)] and fx.expected("layout_5x5", True)[4][1] == [(2, 5)]
    for name, H, W in (("layout_5x64", 5, 64), ("layout_64x5", 64, 5), ("layout_every_pixel", 20, 20), ("layout_every_pixel_r2", 12, 12)):
        case = C.by_name(name)
        assert (case.H, case.W) == (H, W)
        for f in case.fields:
            assert len(f) == (H - 4) * (W - 4) and not (f.r2() < case.thr).any()        # every pixel a survivor
    assert fx.expected("layout_one_field_filtered", True) == [([], [])] and fx.expected("layout_one_field_empty", True) == [([], [])]
    e = C.by_name("layout_empties")
    assert len(e.fields[0]) == 0 and e.layout[0] == 0 and e.layout[-1] == 0 and 0 in e.layout[1:-1]
    for n in (257, 1023, 1024):
        case = C.by_name("layout_%d_fields" % n)
        assert len(case.layout) == n and case.default_form and set(case.layout) == set(range(len(case.fields)))
    # the library's switch between its two forms: n_fields * 8 waves >= 8 192 (frames of up to a megapixel)
    assert 1023 * 8 < 8192 <= 1024 * 8
    assert max(max(c.H, c.W) for c in C.cases()) <= 69


def test_wild_cases_reach_all_four_sides_and_the_assert(fx):
    sides = {"top": 0, "left": 0, "bottom": 0, "right": 0}
    n_assert = 0
    for name in ("wild_40x56", "wild_33x47_r2"):
        case = C.by_name(name)
        for e in fx.expected(name, True):
            if e is None:
                n_assert += 1
                continue
            for kh, kw in e[1]:
                sides["top"] += kh < 0
                sides["left"] += kw < 0
                sides["bottom"] += kh >= case.H
                sides["right"] += kw >= case.W
    assert min(sides.values()) >= 2 and n_assert >= 2, (sides, n_assert)


def test_py2_round_is_the_c_library_s_round():
    import ctypes
    libm = ctypes.CDLL("libm.so.6")
    libm.round.restype, libm.round.argtypes = ctypes.c_double, [ctypes.c_double]
    libm.rint.restype, libm.rint.argtypes = ctypes.c_double, [ctypes.c_double]
    xs = [0.49999999999999994, -0.49999999999999994, 0.5, -0.5, 1.5, 2.5, -1.5, -2.5, 0.0, -0.0, 3.4999999999999996, 1e15 + 0.5, -7.5, 7.25]
    for x in xs:
        assert C.py2_round(x) == int(libm.round(x)), x
        assert C.py3_round(x) == int(libm.rint(x)), x
