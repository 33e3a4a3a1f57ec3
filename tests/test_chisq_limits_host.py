"""Host twin of test_gpu_chisq_limits.py (no GPU): the inputs of tests/_chisq_limit_cases.py reach the corners they are meant
to reach, so that the GPU test cannot pass vacuously, and the restatement (tests/_chisq_reference.py) equals every record of
tests/golden/chisq_limits.npz (tools/gen_chisq_golden.py --limits) bit for bit.  The counts are floors on the inputs."""
import math

import numpy as np

import _chisq_limit_cases as CL
import _chisq_reference as R
from _limits_cases import pairwise_sum
from _util import _bits, same_plateaus


def _fit(v, ns, mult=1, L=2, mag=0.0, ign=False):
    with np.errstate(all="ignore"):
        return R.chi_squared(np.asarray(v).tolist(), mult, ns, L, mag, ign)


# ---- A ---------------------------------------------------------------------------------------------------------------------
def test_pow_sweep_reaches_every_path_of_the_power():
    x, band = CL.pow_sweep()
    assert len(x) == 3 * 8192 + 101
    p = CL.pow2_array(x)
    assert int(((p > 0) & (p < CL.DBL_MIN)).sum()) >= 2000             # a subnormal result (exp's special case)
    assert int((p == 0).sum()) >= 500 and int(np.isinf(p).sum()) >= 500
    assert int(((np.abs(x) < CL.DBL_MIN) & (x != 0)).sum()) >= 1500     # a subnormal x (the normalise branch)
    assert int((x == 0).sum()) >= 2 and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    with np.errstate(all="ignore"):
        differs = _bits(p) != _bits(x * x)
    assert int(differs.sum()) >= 200
    ax = np.abs(x)
    assert int((differs & (ax >= 2.0 ** -10) & (ax <= 2.0 ** 20)).sum()) >= 100
    assert int((differs & (p > 0) & (p < CL.DBL_MIN)).sum()) >= 50
    for t in (2.0 ** -537, CL.SQRT_MAX):                                # both sides of the two thresholds
        assert (ax == t).any() and (ax == math.nextafter(t, 0.0)).any() and (ax == math.nextafter(t, math.inf)).any()
    # no block of the three-trip launch sees one band only: the bands are shuffled over the batch
    assert (band[:8192] != band[8192:16384]).mean() > 0.5 and (band[8192:16384] != band[16384:24576]).mean() > 0.5
    assert all(len(set(band[k * 8192:(k + 1) * 8192].tolist())) == 8 for k in range(3)) and len(band) > 3 * 8192
    # the stated expectation is the restatement's, on a subsample
    res, S = CL.sweep_expected(x)
    for i in range(0, len(x), 61):
        fit, recs = _fit([x[i], -x[i]], None)
        same_plateaus(fit, [(0, 1, 0.0)], i)
        assert len(recs) == 1 and recs[0][2] == 1, i
        assert _bits([recs[0][0]])[0] == _bits([recs[0][1]])[0] == _bits([res[i]])[0], i
        assert CL.nan_to_x86([recs[0][3]])[0] == S[i], i


# ---- B ---------------------------------------------------------------------------------------------------------------------
def test_stride_rows_change_length_in_both_directions():
    pool = CL.stride_pool()
    idx, lens = CL.stride_rows()
    assert len(pool) <= 512 and len(idx) == 2 * 8192 + 777
    plen = np.array([len(v) for v in pool])
    assert plen.min() == 3 and (plen[:480] <= 40).all()
    assert sum(1 for v in pool if np.ptp(v) == 0) >= 5                                     # flat
    assert sum(1 for v in pool if np.ptp(v) > 0 and len(np.unique(v)) <= 5 and len(v) > 8) >= 5   # exact staircases
    true_len = plen[idx]
    a, b, c = true_len[:8192], true_len[8192:16384], true_len[16384:]
    assert int((b < a).sum()) >= 2000 and int((b > a).sum()) >= 2000
    assert int((c < b[:777]).sum()) >= 100 and int((c > b[:777]).sum()) >= 100
    bad = lens != true_len
    assert set(lens[bad].tolist()) == {0, -3, 1, int(plen.max()) + 1} and 200 <= int(bad.sum()) <= 400
    assert len(set(idx[~bad].tolist())) == len(pool)                                       # every pool trace runs
    for k in range(len(CL.STRIDE_PARAMS)):
        exp = CL.stride_expected(k)
        for fit, recs in exp:
            CL.check_no_unpinned_nan(recs)
        assert sum(1 for _, recs in exp if len(recs) > 1) > 300
    # the second parameter set rejects steps and keeps the longest fit
    assert sum(1 for (f0, _), (f1, _) in zip(CL.stride_expected(0), CL.stride_expected(1)) if len(f0) != len(f1)) > 100


# ---- C ---------------------------------------------------------------------------------------------------------------------
def test_extreme_scales_reach_subnormal_sums_and_the_x86_nan():
    n_sub = n_nan = 0
    for name, v, ns in CL.extreme_cases():
        assert 40 <= len(v) <= 60
        fit, recs = _fit(v, ns)
        CL.check_no_unpinned_nan(recs)
        sums = np.array([r[:2] for r in recs])
        n_sub += int(len(recs) > 1 and ((sums > 0) & (sums < CL.DBL_MIN)).all())
        n_nan += int(CL.nan_to_x86([recs[0][3]])[0] == CL.X86_NAN)
    assert n_sub >= 2 and n_nan >= 2
    names = {c[0] for c in CL.extreme_cases()}
    assert len(names) == 9 and {ns for _, _, ns in CL.extreme_cases()} == {5, None}
    z = [v for n, v, _ in CL.extreme_cases() if n == "zeros"][0]
    assert np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()
    fit, _ = _fit(z, 5)
    assert sum(1 for a, b, _ in fit if b - a + 1 >= 8 and np.signbit(z[a:b + 1]).all()) >= 1   # a long plateau of -0.0 alone


# ---- D ---------------------------------------------------------------------------------------------------------------------
def test_long_cases_exceed_64_plateaus_and_fit_cap():
    big_fit = big_counter = big_nfits = 0
    longest = 0
    for c in CL.LONG_CASES:
        v = CL.long_trace(c)
        assert len(np.unique(np.frexp(v)[0] * 2.0 ** 53 % 2 ** 20)) > len(v) // 2     # full mantissas
        fit, recs = _fit(v, c[4], c[5], c[6])
        CL.check_no_unpinned_nan(recs)
        big_fit += len(fit) > 64
        big_counter += max(r[2] for r in recs) > 64
        big_nfits += len(recs) > CL.FIT_CAP
        longest = max([longest] + [b - a + 1 for a, b, _ in fit])
    assert big_fit >= 1 and big_counter >= 1 and big_nfits >= 1
    lengths = {len(CL.long_trace(c)) for c in CL.LONG_CASES}
    assert lengths >= {129, 136, 257, 520, 1023, 1024}
    # the candidates of a whole trace of n frames refit 1 .. n - 1 frames on the left and on the right (at every offset), so a
    # trace just above an edge of the pairwise sum and one far above it put sub-plateaus on both sides of that edge
    for edge in (128, 256, 512):
        assert any(edge < n <= edge + 8 for n in lengths) and any(n > 2 * edge - 1 for n in lengths), edge
    assert longest > 128                                            # and a returned height is the mean of more than one leaf


# ---- E ---------------------------------------------------------------------------------------------------------------------
def test_filter_limit_cases_need_the_deep_pairwise_levels():
    cases = CL.filter_limit_cases()
    assert len(cases) % 64 and {len(c["lum"]) for c in cases} >= {8191, 8192}
    assert sum(1 for c in cases if len(c["pin"]) == len(c["lum"]) >= 8191) == 2
    up = CL.filter_expected(cases[:2], 0, None, None)
    assert all(1 < len(p) < 100 for p in up)
    one = CL.filter_expected(cases[:14], 1, 1e9, None)
    assert all(len(p) == 1 for p in one)
    # a pairwise sum with 4 instead of 7 levels gives other bits for a good share of the merged heights
    sens = sum(int(_bits([pairwise_sum(c["lum"], depth=4) / len(c["lum"])])[0] != _bits([p[0][2]])[0]) for c, p in zip(cases[:14], one))
    assert sens >= 4, sens
    with np.errstate(all="ignore"):
        assert CL.nan_to_x86([R.r_squared(cases[14]["lum"].tolist(), cases[14]["pin"])])[0] == CL.X86_NAN


# ---- F ---------------------------------------------------------------------------------------------------------------------
def test_unsupported_cases_raise_after_their_records():
    for lum, ns in CL.UNSUPPORTED_CASES:
        recs = CL.records_until_raise(lum, ns)
        assert len(recs) == len(lum) - 1
    fit, recs = _fit([4.0, 4.0, 4.0], 2, L=0)
    assert fit == [(0, 2, 4.0)] and len(recs) == 1


# ---- the fixture -----------------------------------------------------------------------------------------------------------
def test_restatement_equals_every_limit_record():
    gold = CL.golden()
    want = CL.recorded_cases()
    assert [g["name"] for g in gold] == [w[0] for w in want]
    assert sum(1 for g in gold if len(g["lum"]) >= 129) >= 5 and max(len(g["fit"]) for g in gold) >= 30
    for i, (g, (_, v, ns, mult, L)) in enumerate(zip(gold, want)):
        assert np.array_equal(_bits(g["lum"]), _bits(v)), "the seeded trace generator drifted from the fixture"
        assert (g["num_steps"], g["mult"], g["L"]) == (ns, float(mult), L), i
        fit, recs = _fit(v, ns, mult, L)
        same_plateaus(fit, g["fit"], i)
        assert len(recs) == len(g["best"]), i
        assert np.array_equal(_bits([r[0] for r in recs]), _bits(g["best"])), i
        assert np.array_equal(_bits([r[1] for r in recs]), _bits(g["counter"])), i
        assert [r[2] for r in recs] == g["counter_n"].tolist(), i
        assert np.array_equal(CL.nan_to_x86([r[3] for r in recs]), CL.nan_to_x86(g["S"])), i
