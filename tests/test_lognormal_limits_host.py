"""Host twin of test_gpu_lognormal_limits.py (no GPU): the inputs of tests/_lognormal_limit_cases.py reach the paths they are
meant to reach, so that the GPU tests cannot pass vacuously, and the expected values come from code that is not the kernels'
(the Python twins of the package and tests/_remainder_reference.py).  The counts are floors on the inputs.

  A  257 base rows tiled to 2 x 16 384 + 77: at least 20 each of FOUND, NONE and INVALID, at least 5 OVER_BUDGET under the
     small budget, a period that is no divisor of the grid; 4 096 x 256 + 3 values for the logarithm
  B  the 495-survivor track on both sides of its budget; tracks of exactly 1, 2, 63, 64, 65, 127, 128 and 129 survivors
  C  0, -0.0, -5, NaN, +inf, -inf, 5e-324 and 1.7e308 at an ON and at an OFF frame: -10000 for what has no logarithm, +inf
     admissible at an infinite deviation alone, with density 0 and the first sequence in order at score 0.0
  D  remainder tracks with a NaN (median NaN: every frame of the segment's RATIO medians is NaN, one frame of the ADDITIVE
     ones), +inf and (-inf, +inf), in segments on both selection paths; malformed offsets; 66 000 segments, whose vectorised
     expectation equals the restatement on the first 2 000
  E  the values of C at a last drop; a NaN entry in one ON/OFF key

Run time of this file on the host: 7 s (tests/test_chisq_limits_host.py in the same run: 30 s)."""
import math

import numpy as np

import _lognormal_limit_cases as LC
import _remainder_reference as RR
from _remainder_cases import same_arrays
from _util import bits_equal
from fluorosequencingimageanalysis_amd import _host_lognormal as R
from fluorosequencingimageanalysis_amd import _host_lognormal_chain as HC
from fluorosequencingimageanalysis_amd import _host_remainder as HR
from fluorosequencingimageanalysis_amd import _native_remainder as NR


def _same_fit(a, b, what):
    for k in ("status", "best_seq"):
        assert np.array_equal(a[k], b[k]), (what, k)
    for k in ("best_score", "frame_score"):
        assert bits_equal(a[k], b[k]).all(), (what, k)


# ---- A ---------------------------------------------------------------------------------------------------------------------
def test_stride_base_holds_every_status_and_no_block_repeats_a_track():
    rows, words, lens, I, C, valid = LC.stride_base()
    assert rows.shape == (LC.PERIOD, LC.F_STRIDE) and LC.MAX_BLOCKS % LC.PERIOD and math.gcd(LC.MAX_BLOCKS, LC.PERIOD) == 1
    assert LC.N_STRIDE == 2 * 16384 + 77 and {len(v) for v in I} == set(range(1, 14))
    assert sorted(set(lens[~valid].tolist())) == [-1, 0, LC.F_STRIDE + 1] and (~valid).sum() == 21
    idx = LC.stride_index()
    # block b meets base tracks idx[b], idx[b + 16384], idx[b + 32768]: all different, and of different lengths for most
    first, second = idx[:LC.MAX_BLOCKS], idx[LC.MAX_BLOCKS:2 * LC.MAX_BLOCKS]
    assert (first != second).all() and (lens[first] != lens[second]).mean() > 0.8
    assert (lens[first] > lens[second]).sum() > 4000 and (lens[first] < lens[second]).sum() > 4000
    assert set(idx[2 * LC.MAX_BLOCKS:].tolist()) != set(idx[:77].tolist())
    for solver, ups in LC.LAUNCHES:
        e = LC.stride_expected(solver, ups)
        for status in (LC.FOUND, LC.NONE, LC.INVALID):
            assert int((e["status"] == status).sum()) >= 20, (solver, ups, status)
        assert not (e["status"] == LC.OVER_BUDGET).any()
    _same_fit(LC.stride_expected("enumerate", False), LC.stride_expected("dp", False), "two twins")
    assert np.array_equal(LC.stride_expected("enumerate", False)["n_surviving"], LC.stride_expected("dp", False)["n_surviving"])
    up = LC.stride_expected("dp", True)
    rising = sum(1 for s, seq, T in zip(up["status"], up["best_seq"], lens) if s == 0 and (np.diff(seq[:T].astype(int)) > 0).any())
    assert rising >= 20
    small = LC.stride_expected("enumerate", False, LC.SMALL_BUDGET)
    over = small["status"] == LC.OVER_BUDGET
    assert int(over.sum()) >= 5 and int((small["status"] == LC.FOUND).sum()) >= 20
    assert (small["n_surviving"][over] > LC.SMALL_BUDGET).all() and (small["best_score"][over] == -1.0).all()
    assert not small["best_seq"][over].any() and not small["frame_score"][over].any()


def test_log_values_exceed_the_grid():
    x, e = LC.log_stride()
    assert len(x) == 4096 * 256 + 3 > LC.LOG_BLOCKS * LC.LOG_THREADS and len(LC.golden()["c_x"]) > 3500
    with np.errstate(all="ignore"):
        assert (np.abs(np.log(x) - e) <= 1e-12 * np.abs(e))[np.isfinite(e)].all()       # (the recorded bits are the fixture's)


# ---- B ---------------------------------------------------------------------------------------------------------------------
def test_budget_track_and_survivor_targets():
    I, C, dev, n = LC.BUDGET_TRACK
    ok, _ = R.tables(I, C, LC.MEANS, LC.SIGMA, LC.M, dev)
    assert R.count_surviving(ok, LC.M, True) == n == 495
    at = LC.twin_fit([I], [C], LC.MEANS, LC.SIGMA, LC.M, True, dev, "enumerate", False, budget=495)
    below = LC.twin_fit([I], [C], LC.MEANS, LC.SIGMA, LC.M, True, dev, "enumerate", False, budget=494)
    assert at["status"][0] == LC.FOUND and below["status"][0] == LC.OVER_BUDGET and below["best_score"][0] == -1.0
    found = LC.survivor_tracks()
    assert sorted(found) == sorted(LC.SURVIVOR_TARGETS)
    for n, (I, C, dev) in found.items():
        ok, _ = R.tables(I, C, LC.MEANS, LC.SIGMA, LC.M, dev)
        assert R.count_surviving(ok, LC.M, True) == n and len(I) >= 2
        for multi in (True, False):
            a = LC.twin_fit([I], [C], LC.MEANS, LC.SIGMA, LC.M, multi, dev, "enumerate", False)
            b = LC.twin_fit([I], [C], LC.MEANS, LC.SIGMA, LC.M, multi, dev, "dp", False)
            _same_fit(a, b, (n, multi))
            assert a["n_surviving"][0] == b["n_surviving"][0] and (not multi or a["n_surviving"][0] == n)


# ---- C ---------------------------------------------------------------------------------------------------------------------
def test_refused_values_take_the_paths_named():
    I, C, meta = LC.value_tracks()
    assert len(I) == 2 * 4 * len(LC.VALUES) and {len(v) for v in I} == {3, 4, 5, 6}
    assert {(vi, on) for vi, on, _ in meta} == {(vi, on) for vi in range(len(LC.VALUES)) for on in (True, False)}
    for v, c, (vi, on, f) in zip(I, C, meta):
        assert c[f] == on and (v[f] == LC.VALUES[vi] or (v[f] != v[f] and LC.VALUES[vi] != LC.VALUES[vi]))
        assert math.copysign(1.0, v[f]) == math.copysign(1.0, LC.VALUES[vi])
    logs = R.log_intensities(list(LC.VALUES))
    assert logs[:4] == [-10000] * 4 and logs[4] == math.inf and logs[5] == -10000 and logs[6] < -744 and logs[7] > 709
    inf_on = [t for t, (vi, on, _) in enumerate(meta) if on and LC.VALUES[vi] == math.inf]
    no_log_on = [t for t, (vi, on, _) in enumerate(meta) if on and logs[vi] == -10000]
    for solver, ups in LC.LAUNCHES:
        narrow, wide, infinite = (LC.value_expected(dev, solver, ups) for dev in LC.DEVIATIONS)
        on_rows = [t for t, m in enumerate(meta) if m[1]]
        assert (narrow["status"][on_rows] == LC.NONE).all()         # none of the values is within 3 sigma of a count
        assert int((narrow["status"] == LC.FOUND).sum()) >= 20      # at an OFF frame the value is not looked at
        assert (wide["status"][inf_on] == LC.NONE).all() and (wide["status"][no_log_on] == LC.FOUND).all()
        assert (wide["best_score"][no_log_on] == 0.0).all()
        assert (infinite["status"] == LC.FOUND).all() and (infinite["best_score"][inf_on] == 0.0).all()
        for t in inf_on:                                            # density 0 at the infinite frame; score 0.0: the first in order
            f = meta[t][2]
            assert infinite["frame_score"][t, f] == 0.0
            if not ups:
                first = LC.twin_fit([I[t]], [C[t]], LC.MEANS, LC.SIGMA, LC.M, True, math.inf, "enumerate", False, F=6)
                assert np.array_equal(first["best_seq"][0], infinite["best_seq"][t])
                assert infinite["best_seq"][t, 0] == LC.M           # (the largest count first: every total is 0.0)


# ---- D ---------------------------------------------------------------------------------------------------------------------
def test_nan_tracks_make_every_ratio_median_nan():
    assert NR.LDS_MAX == 512 and LC.SMALL_R <= NR.LDS_MAX < LC.LARGE_R
    for F in LC.NAN_FRAMES:
        rows, cats, seg_off, meta = LC.nan_table(F)
        names = {name for _, name, _ in meta}
        assert {"nan first", "nan middle", "nan last", "inf", "-inf, inf", None} <= names and ("two nans" in names) == (F == 5)
        ratio, additive = LC.nan_expected(F, RR.RATIO), LC.nan_expected(F, RR.ADDITIVE)
        assert set(ratio["n_remainders"].tolist()) == {LC.SMALL_R, LC.LARGE_R}
        for s, name, frames in meta:
            a, b = int(seg_off[s]), int(seg_off[s + 1])
            special = [t for t in range(a, b) if not np.isfinite(rows[t]).all()]
            assert len(special) == (0 if name is None else 1), (F, s)
            if name is None:
                assert np.isfinite(ratio["adjustment"][s]).all() and np.isfinite(additive["adjustment"][s]).all()
                continue
            t = special[0]
            assert RR.is_remainder(cats[t], F)
            nan_at = sorted(f for f, v in frames.items() if v != v)
            assert np.flatnonzero(np.isnan(rows[t])).tolist() == nan_at
            if nan_at:                                              # the median rule for a NaN track
                assert np.isnan(RR.median(rows[t])) and np.isnan(np.median(rows[t]))
                assert np.isfinite(np.sort(rows[t])[(F - 1) // 2]) and np.isfinite(np.sort(rows[t])[F // 2]) or F == 5 and len(nan_at) == 2
                assert np.isnan(ratio["adjustment"][s]).all(), (F, s, name)
                want = set(range(F)) if 0 in nan_at else set(nan_at)
                assert set(np.flatnonzero(np.isnan(additive["adjustment"][s])).tolist()) == want, (F, s, name)
            else:
                assert np.isfinite(RR.median(rows[t])) and np.isfinite(ratio["adjustment"][s]).all(), (F, s, name)
        # the host twin of the package says the same
        for mode, e in ((RR.RATIO, ratio), (RR.ADDITIVE, additive)):
            with np.errstate(all="ignore"):
                same_arrays(HR.adjust(rows, cats, seg_off, {RR.RATIO: NR.MODE_RATIO, RR.ADDITIVE: NR.MODE_ADDITIVE}[mode], 5), e, (F, mode))


def test_malformed_offsets_and_their_well_formed_segments():
    rows, cats, good = LC.malformed_table()
    n = len(rows)
    assert good.tolist() == LC.MALFORMED_OFFSETS[0] and n == 100
    ascending = [off for off in LC.MALFORMED_OFFSETS if (np.diff(off) >= 0).all()]
    assert len(ascending) == 3 and len(LC.MALFORMED_OFFSETS) == 8
    kinds = set()
    for off in LC.MALFORMED_OFFSETS:
        for s in range(3):
            a, b = off[s], off[s + 1]
            kinds.add("ok" if LC.well_formed(off, s, n) else "descending" if b < a else "negative" if a < 0 else "beyond")
    assert kinds == {"ok", "descending", "negative", "beyond"}
    e = RR.adjust_arrays(rows, cats, good, RR.RATIO, 5)
    assert e["n_remainders"].tolist() == [10, 30, 7] and e["kept"].all()


def test_many_segments_shortcut_equals_the_restatement():
    rows, cats, seg_off, _ = LC.many_segments(2)
    sizes = np.diff(seg_off)
    assert len(sizes) == 66000 and set(sizes.tolist()) == {0, 1, 2, 3} and 0.3 < (sizes == 0).mean() < 0.37
    assert len(sizes) > 256 * 256 and len(sizes) * 2 > 1 << 17        # krm_finish beyond one block of blocks, S * F median blocks
    assert math.ceil(math.log2(len(sizes) + 1)) == 17               # the depth of segment_of's search
    count = LC.many_remainder_expected(RR.RATIO, 1)["n_remainders"]
    assert all(int((count == c).sum()) > 3000 for c in (0, 1, 2, 3))
    for mode in (RR.RATIO, RR.ADDITIVE):
        for minimum in (0, 2):
            short = LC.many_remainder_expected(mode, minimum, 2000)
            n = int(seg_off[2000])
            with np.errstate(all="ignore"):
                same_arrays(short, RR.adjust_arrays(rows[:n], cats[:n], seg_off[:2001], mode, minimum), (mode, minimum))
            full = LC.many_remainder_expected(mode, minimum)
            same_arrays({k: v[:n if k == "adjusted" else 2000] for k, v in full.items()}, short, (mode, minimum, "prefix"))
    rows, cats, seg_off, status = LC.many_segments(3)
    m, counts, M = HC.on_off_medians(rows, HC.category_bits(cats, 3), seg_off, status == 0, 3.5)
    assert all(int((counts == c).sum()) >= 50 for c in (0, 1, 2, 3)) and np.isfinite(M) and int((counts > 0).sum()) > 512


# ---- E ---------------------------------------------------------------------------------------------------------------------
def test_chain_steps_with_refused_values():
    rows, cats = LC.value_table()
    bits = HC.category_bits(cats, 4)
    drops = HC.last_drops(rows, bits)
    step = HC.on_then_off(bits)
    at_step = rows[:, :-1][step]
    assert int(np.isinf(drops).sum()) == int((at_step == np.inf).sum()) >= 2                 # +inf gives +inf
    assert len(drops) == int((at_step > 0).sum()) < len(at_step) and not np.isnan(drops).any()
    for v in LC.VALUES:
        assert any((x == v and math.copysign(1, x) == math.copysign(1, v)) or (x != x and v != v) for x in at_step.tolist())
    assert (drops == math.log(5e-324)).any() and (drops == math.log(1.7e308)).any()
    rows, cats, seg_off, status, (s, f) = LC.nan_key_table()
    m, counts, M = HC.on_off_medians(rows, HC.category_bits(cats, 4), seg_off, status == 0, 3.5)
    assert np.isnan(M) and np.isnan(m[s, f]) and counts[s, f] == 40
    clean = rows.copy()
    clean[np.isnan(rows)] = 1000.0
    m0, counts0, M0 = HC.on_off_medians(clean, HC.category_bits(cats, 4), seg_off, status == 0, 3.5)
    keep = np.ones(m.shape, bool)
    keep[s, f] = False
    assert np.array_equal(counts, counts0) and np.isfinite(M0) and bits_equal(m[keep], m0[keep]).all()
    assert np.isnan(m[:, 1]).all() and np.isfinite(m[:, [0, 2]][keep[:, [0, 2]]]).all()
