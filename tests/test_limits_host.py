"""Host twins of the limit tests (no GPU): what test_gpu_stepfit_limits.py and test_gpu_sequence_limits.py feed to the device
is checked here against the restatements alone - the new fixtures equal the restatements bit for bit, every tied-p case
depends on the tie order, scipy agrees with mpmath on the p sweep's subsample, the sweep covers what it claims, and the share
of traces a GPU test may leave out stays inside its cap."""
import math
import os

import numpy as np
import pytest

import _limits_cases as LC
import _sequence_reference as Q
import _stepfit_reference as R
from _util import _bits, same_plateaus


# ---- A1 ------------------------------------------------------------------------------------------------------------------------
def test_length_limit_fixture_equals_restatement():
    """The reference's recorded CK values, plateaus and heights of the 8191 / 8192-frame traces == the restatement's, and the
    cases stand where they claim: a final plateau of more than 7689 frames whose mean a pairwise sum with one level of
    recursion too few would round differently."""
    cases = LC.length_limit_cases()
    assert sorted(set(len(c["phot"]) + min(c["mirror"], len(c["phot"])) for c in cases)) == [8191, 8192]
    assert any(c["ck"] for c in cases) and any(not c["ck"] for c in cases) and any(not c["drop_sort"] for c in cases)
    assert any(c["first_pass_pairs"] >= 64 for c in cases)
    for i, c in enumerate(cases):
        ph, ck, pl, tf, fl = R.stepfit(c["phot"].tolist(), c["mirror"], c["ck"], c["thr"], None, drop_sort=c["drop_sort"])
        assert not fl.near and not fl.unsupported, i
        if c["ck"]:
            assert np.array_equal(_bits(ck), _bits(c["ck_out"])), i
        same_plateaus(pl, c["pl"])
        same_plateaus(tf, c["tf"])
        if c["thr"] < 0.01:
            lens = [o - s + 1 for s, o, _ in c["tf"]]
            assert max(lens) > 7689 and sum(1 for x in lens if 129 < x <= 7689) >= 3, i
            s, o, h = c["tf"][int(np.argmax(lens))]
            m = c["mirror"]
            mir = np.concatenate([c["phot"][:m][::-1], c["phot"]])
            seg = mir[s if s > 0 else 0:o + m + 1]                  # the plateau in mirrored frames (it starts inside the mirror)
            assert _bits([LC.pairwise_sum(seg) / len(seg)])[0] == _bits([h])[0] == _bits([np.mean(seg)])[0], i


def test_long_merge_cases_see_a_recursion_that_is_too_shallow():
    """Every case merges into one plateau whose height is np.mean of all frames, and for a good share of them a pairwise sum
    with 6 instead of 7 levels of recursion gives other bits (the shallow recursion adds one block of 129 - 136 frames in one
    go; its 8 accumulators see the same frames in the same order, so only the way they are combined differs and about one
    case in five shows it)."""
    cases = LC.long_merge_cases()
    n_sensitive = 0
    for lum, pl in cases:
        fl = R.Flags()
        (s, o, h), = R.t_test_filter(lum, pl, 0.01, flags=fl)
        assert not fl.near and (s, o) == (0, len(lum) - 1)
        assert _bits([h])[0] == _bits([LC.pairwise_sum(lum) / len(lum)])[0]
        n_sensitive += int(_bits([LC.pairwise_sum(lum, depth=6) / len(lum)])[0] != _bits([h])[0])
    print("sensitive to the recursion depth:", n_sensitive, "of", len(cases))
    assert n_sensitive >= 8


def test_pairwise_sum_restatement():
    rng = np.random.default_rng(1)
    for n in (0, 1, 7, 8, 9, 127, 128, 129, 136, 1000, 7689, 8191, 8192):
        a = rng.normal(0, 1e4, n)
        assert LC.pairwise_sum(a) == float(np.sum(a)), n


# ---- A2 ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    pts = LC.p_sweep()
    return pts, LC.sweep_scipy(pts)


def test_p_sweep_covers_the_plane(sweep):
    pts, (p, t, df) = sweep
    assert len(pts) >= 6000 and max(len(a) + len(b) for a, b in pts) <= 8192
    assert np.isfinite(p).all()
    assert df.min() < 1.2 and df.max() > 7000
    edges = np.exp(np.linspace(0.0, math.log(8190.0), 41))                        # 40 bins on the log scale
    assert (np.histogram(df, edges)[0] >= 40).all()
    for lo, hi in ((38, 39), (39, 39.8), (39.8, 40), (40, 40.2), (40.2, 41), (41, 42)):      # both sides of a = 20
        assert ((df >= lo) & (df < hi)).sum() >= 10, (lo, hi)
    at = np.abs(t)
    assert at.min() < 1e-8 and at.max() > 5e3
    assert (np.histogram(np.log10(at), np.arange(-9, 5))[0] >= 150).all()         # every decade of |t|
    swap = 3.0 * df / (df + 2.0)                                                   # x < (a + 1) / (a + b + 2)  <=>  t^2 > swap
    for d in range(4):                                                             # every df decade, both branches
        m = (df >= 10.0 ** d) & (df < 10.0 ** (d + 1))
        assert (m & (t * t > swap)).sum() >= 100 and (m & (t * t < swap)).sum() >= 100, d
        assert (m & (np.abs(t * t / swap - 1.0) < 5e-3)).sum() >= 20, d
    assert (p < LC.P_TINY).mean() <= LC.MAX_TINY_SHARE
    assert (p < LC.P_TINY).sum() >= 20                                             # (and the underflow corner is visited)


def test_scipy_agrees_with_mpmath_on_the_subsample(sweep):
    """The two host references of the sweep are independent of each other and agree far inside the 1e-10 bar."""
    pts, (p, t, df) = sweep
    idx = LC.mp_subsample(len(pts))
    assert len(idx) >= 2000
    worst = 0.0
    for i in idx:
        e = LC.mp_p(t[i], df[i])
        if e < LC.P_TINY:
            assert 0.0 <= p[i] <= 1e-299
            continue
        worst = max(worst, abs(p[i] - e) / e)
    print("scipy against mpmath, largest relative deviation: %.3g" % worst)
    assert worst <= 1e-11


def test_sliding_p_scipy_equals_restatement_windows():
    """The vectorised scipy reference of the sliding-window p against one ttest_ind call per window."""
    from scipy import stats
    seq = LC.sliding_p_traces(7)[-2]
    got, = LC.sliding_p_scipy([seq], 9)
    n = len(seq)
    for k, r in enumerate(range(5, 9)):
        for f in range(0, n, 7):
            a, b = seq[f - r:f] if f - r >= -n else seq[0:f], seq[f:f + r]
            e = stats.ttest_ind(a, b, equal_var=False).pvalue if len(a) and len(b) else math.nan
            assert (math.isnan(e) and math.isnan(got[k, f])) or abs(got[k, f] - e) <= 1e-13 * e, (r, f)


# ---- A3 ------------------------------------------------------------------------------------------------------------------------
def param_limit_expected(name):
    """(traces, [restatement result or None where it flags near / unsupported])."""
    (_, seed, mirror, ck, wr, ds, wl, M), = [s for s in LC.PARAM_LIMIT_SETS if s[0] == name]
    traces = LC.param_limit_traces(seed, wr)
    out = []
    for t in traces:
        ph, ckf, pl, tf, fl = R.stepfit(t.tolist(), mirror, ck, 0.01, None, window_radius=wr, drop_sort=ds, window_lengths=wl, M=M)
        out.append(None if fl.near or fl.unsupported else (ckf, pl, tf))
    return traces, out


@pytest.mark.parametrize("name", [s[0] for s in LC.PARAM_LIMIT_SETS])
def test_param_limit_sets_skip_at_most_a_tenth(name):
    traces, exp = param_limit_expected(name)
    assert set(LC.BOUNDARY_LENGTHS) <= set(len(t) for t in traces)
    skipped = sum(e is None for e in exp)
    print(name, "skipped", skipped, "of", len(exp))
    assert skipped <= LC.MAX_SKIPPED_SHARE * len(exp)
    assert all(e is not None for t, e in zip(traces, exp) if len(t) in LC.BOUNDARY_LENGTHS)


# ---- A4 ------------------------------------------------------------------------------------------------------------------------
def test_sort_cases_are_deterministic_and_tie_sensitive():
    cases = LC.sort_cases()
    first = {name: len(pl) - 1 for name, (lum, pl, nms, tied) in cases.items()}
    assert {63, 64, 65} <= set(first.values()) and max(first.values()) >= 300
    for name, (lum, pl, nms, tied) in cases.items():
        fl = R.Flags()
        exp = R.t_test_filter(lum, pl, LC.SORT_THR, drop_sort=True, no_merge_start=nms, flags=fl)
        assert exp is not None and not fl.near and not fl.unsupported, name
        assert len(exp) < len(pl), name                             # at least one pass merges
        ps = np.array(fl.p_pairs[:len(pl) - 1])
        if tied:
            fin = ps[np.isfinite(ps)]
            assert len(fin) == len(ps) and len(np.unique(fin)) < len(fin) / 4, name
            ties = fin[fin >= LC.SORT_THR]
            assert len(ties) - len(np.unique(ties)) >= 20, name     # exactly tied p at or above the threshold
            rev = R.t_test_filter(lum, pl, LC.SORT_THR, drop_sort=True, no_merge_start=nms, tie_reverse=True)
            assert [(s, o) for s, o, _ in rev] != [(s, o) for s, o, _ in exp], name + ": insensitive to the tie order"
        else:
            assert len(pl) - 1 < 64 and np.isnan(ps).any() and np.isfinite(ps).any(), name
        fl2 = R.Flags()
        assert R.t_test_filter(lum, pl, LC.SORT_THR, drop_sort=False, no_merge_start=nms, flags=fl2) is not None and not fl2.near


# ---- B ---------------------------------------------------------------------------------------------------------------------------
def test_category_counts_unique_equals_dict_loop():
    rng = np.random.default_rng(3)
    for n in (1, 2, 50, 3000):
        cat = rng.integers(0, 6, n).astype(np.uint64) | (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63))
        seq = rng.integers(0, 3, n).astype(np.int32)
        for sel in (None, rng.random(n) < 0.6):
            a, b = Q.category_counts(cat, seq, sel), Q.category_counts_unique(cat, seq, sel)
            for k in ("seq", "pattern", "count", "first"):
                assert np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype, (n, k)


def test_hash_restatement_crafts_colliding_keys():
    import _sequence_limit_cases as SC
    keys = SC.keys_in_slot(63, 64, 12)
    assert len(set(keys)) == 12 and all(SC.hash_key(p, s) & 63 == 63 for p, s in keys)
    keys = SC.keys_in_slot(5, 8192, 50)
    assert all(SC.hash_key(p, s) & 8191 == 5 for p, s in keys)


def test_sequence_limit_fixture_equals_restatement():
    """The reference's mexican hat values at radii 12 - 17 (tests/golden/sequence_limits.npz) == the restatement's."""
    import _sequence_limit_cases as SC
    g = SC.load_fixture()
    n_big = 0
    for case in SC.hat_cases(g):
        img = case["frame"].astype(np.int64)
        for (h, w), e in zip(case["hw"], case["phot"]):
            v = Q.mexican_hat(img, int(h), int(w), case["brim"], case["radius"])
            assert (math.isnan(v) and math.isnan(e)) or _bits([v])[0] == _bits([e])[0], (case["name"], h, w)
            n_big += int(Q.window(img, int(h), int(w), case["radius"]).size > 960)
    assert n_big >= 5


def test_round_half_cases_of_the_restatement():
    assert [Q._round_half_away(x) for x in (-0.5, 0.5, 2.5, -2.5, 1.4999999999999998)] == [-1.0, 1.0, 3.0, -3.0, 1.0]
