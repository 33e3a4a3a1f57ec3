"""Inputs of the chi-squared limit tests (test_chisq_limits_host.py, test_gpu_chisq_limits.py) and the loader of
tests/golden/chisq_limits.npz (tools/gen_chisq_golden.py --limits): generated here once, seeded, so that the host twin
checks exactly what the GPU test runs.  Nothing here needs a GPU or reads a file outside tests/golden/."""
import functools
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
X86_NAN = 0xfff8000000000000    # the NaN an invalid operation makes on x86-64
MAX_BLOCKS = 8192               # blocks of kcs_split_scan: a launch of more traces strides
DBL_MIN = 2.0 ** -1022
FIT_CAP = 64


def scalar_pow2(v):
    """glibc's pow(v, 2.0) (math.pow raises where libm returns inf)."""
    try:
        return math.pow(v, 2.0)
    except OverflowError:
        return math.inf


def pow2_array(x):
    return np.array([scalar_pow2(float(v)) for v in x], dtype=np.float64)


def nan_to_x86(v):
    """Expected bits of a float64 array: every NaN is the x86 one."""
    b = np.array(v, dtype=np.float64).view(np.uint64).copy()
    b[np.isnan(np.asarray(v, dtype=np.float64))] = X86_NAN
    return b


# ---- A: pow sweep ----------------------------------------------------------------------------------------------------------
def _differs_from_multiply(x):
    with np.errstate(all="ignore"):
        return pow2_array(x).view(np.uint64) != (x * x).view(np.uint64)


def _search_differing(rng, lo, hi, want):
    """Full-mantissa |x| in [2^lo, 2^hi] whose pow(x, 2.0) is not x * x (about one in a thousand): drawn until `want` are found."""
    found = []
    n_found = 0
    for _ in range(200):
        x = np.exp2(rng.uniform(lo, hi, 40000))
        d = x[_differs_from_multiply(x)]
        found.append(d)
        n_found += len(d)
        if n_found >= want:
            break
    assert n_found >= want, "no pow-sensitive points found"
    return np.concatenate(found)[:want]


SWEEP_N = 3 * MAX_BLOCKS + 101
SQRT_MAX = math.sqrt(sys.float_info.max)


@functools.lru_cache(maxsize=None)
def pow_sweep():
    """SWEEP_N values x for the two-frame traces [x, -x]: the bands of the issue, shuffled.  -> (x, band) with band the
    index into SWEEP_BANDS."""
    rng = np.random.default_rng(9001)
    sign = lambda n: np.where(rng.random(n) < 0.5, -1.0, 1.0)
    bands = []
    # 0: log-uniform over the whole double range (normal exponents), full mantissas
    bits = (rng.integers(1, 2047, 6000, dtype=np.uint64) << np.uint64(52)) | rng.integers(0, 1 << 52, 6000, dtype=np.uint64)
    bands.append(bits.view(np.float64) * sign(6000))
    # 1: the result is subnormal or barely normal
    bands.append(np.exp2(rng.uniform(-538.0, -510.0, 6000)) * sign(6000))
    # 2: subnormal x
    bands.append(rng.integers(1, 1 << 52, 2000, dtype=np.uint64).view(np.float64) * sign(2000))
    # 3: around sqrt(DBL_MAX)
    bands.append(np.exp2(rng.uniform(510.0, 513.0, 3000)) * sign(3000))
    # 4: the working range
    bands.append(np.exp2(rng.uniform(-10.0, 20.0, 6000)) * sign(6000))
    # 5, 6: searched points where pow is not a multiply, in the working range and in the subnormal-result band
    bands.append(_search_differing(rng, -10.0, 20.0, 150) * sign(150))
    bands.append(_search_differing(rng, -537.0, -511.0, 150) * sign(150))
    # 7: specials
    sp = [0.0, -0.0, 2.0 ** -537, -2.0 ** -537, SQRT_MAX, -SQRT_MAX, 2.0 ** -1074, 2.0 ** -1022, 2.0 ** 511, 2.0 ** 512,
          sys.float_info.max, -sys.float_info.max, 1.0, -1.0, 2.0 ** -511, 2.0 ** -538]
    for base in (2.0 ** -537, 2.0 ** -538, 2.0 ** -511, SQRT_MAX, 2.0 ** 512, 2.0 ** -1022, 1.0):
        up = dn = base
        for _ in range(6):
            up, dn = math.nextafter(up, math.inf), math.nextafter(dn, 0.0)
            sp += [up, dn, -up, -dn]
    sp += [2.0 ** k for k in range(-1074, 1024, 7)] + [-(2.0 ** k) for k in range(-1070, 1024, 11)]
    rest = SWEEP_N - sum(len(b) for b in bands) - len(sp)
    assert rest >= 0
    sp += np.exp2(rng.uniform(-539.0, -536.0, rest)).tolist()       # (the fill: around the underflow threshold)
    bands.append(np.array(sp))
    x = np.concatenate(bands)
    band = np.concatenate([np.full(len(b), i) for i, b in enumerate(bands)])
    assert len(x) == SWEEP_N and not np.isnan(x).any() and np.isfinite(x).all()
    perm = rng.permutation(SWEEP_N)
    return x[perm], band[perm]


def sweep_expected(x):
    """Per trace [x, -x]: (best_res == counter_res, S bits)."""
    p = pow2_array(x)
    with np.errstate(all="ignore"):
        res = p + p
    S = np.where(res == 0.0, 1e10, 1.0).view(np.uint64).copy()
    S[np.isinf(res)] = X86_NAN
    return res, S


# ---- traces ---------------------------------------------------------------------------------------------------------------
def stair_noise(seed, n, steps, step=20000.0, noise=2500.0, min_len=1):
    """Full-mantissa values on `steps` + 1 levels that go down and sometimes up (the style of unrounded_trace of
    tools/gen_chisq_golden.py): the sum of such doubles depends on the order of the additions."""
    rng = np.random.default_rng(seed)
    # plateau lengths: min_len each, the remaining frames dealt out at random
    assert (steps + 1) * min_len <= n
    extra = np.bincount(rng.integers(0, steps + 1, n - (steps + 1) * min_len), minlength=steps + 1)
    cuts = np.cumsum(min_len + extra)[:-1]
    level = np.zeros(n)
    cur = float(steps)
    prev = 0
    for c in list(cuts) + [n]:
        level[prev:c] = cur
        cur += 1.0 if rng.random() < 0.25 else -1.0
        prev = c
    return level * step + 5000.0 + rng.normal(0.0, noise, n)


# ---- C: extreme scales -----------------------------------------------------------------------------------------------------
SCALES = (1e-165, 1e-158, 1e-150, 1e150, 1e154)


@functools.lru_cache(maxsize=None)
def extreme_cases():
    """[(name, trace, num_steps)] with the default multiplier 1, min_step_length 2, min_step_magnitude 0."""
    out = []
    for i, s in enumerate(SCALES):
        v = stair_noise(700 + i, 40 + 5 * i, 4, min_len=4) * s
        out += [("scale%g" % s, v, 5), ("scale%g" % s, v, None)]
    v = stair_noise(710, 48, 4, min_len=4)
    out += [("off2^52", v + 2.0 ** 52, 5), ("off2^52", v + 2.0 ** 52, None), ("off1e15", v + 1e15, 5), ("off1e15", v + 1e15, None)]
    z = np.array([-0.0] * 12 + [2.5] * 9 + [0.0] * 10 + [-0.0] * 11 + [-1.5] * 8)
    zn = z.copy()
    zn[z != 0.0] += np.random.default_rng(711).normal(0.0, 0.2, int((z != 0.0).sum()))
    out += [("zeros", z, 5), ("zeros", z, None), ("zeros_noise", zn, 5), ("zeros_noise", zn, None)]
    return out


# ---- D: long traces, many plateaus -----------------------------------------------------------------------------------------
# (name, seed, frames, steps of the staircase, num_steps, multiplier, min_step_length)
LONG_CASES = (("n1024_none", 801, 1024, 110, None, 0.1, 2),
              ("n700_none_L0", 802, 700, 101, None, 0.15, 0),
              ("n300_none", 803, 300, 60, None, 1, 2),
              ("n130_none_L0", 804, 130, 40, None, 1, 0),
              ("n1023_80", 805, 1023, 90, 80, 1, 0),
              ("n1024_80", 806, 1024, 90, 80, 1, 0),
              ("n129_8", 807, 129, 3, 8, 1, 2),
              ("n136_8", 808, 136, 3, 8, 1, 2),
              ("n257_8", 809, 257, 3, 8, 1, 2),
              ("n520_8", 810, 520, 3, 8, 1, 2))
# the sizes the pure-Python reference finishes: recorded in chisq_limits.npz, the restatement pinned to them
LONG_CASES_RECORDED = (("r129_8", 807, 129, 3, 8, 1, 2),
                       ("r136_8", 808, 136, 3, 8, 1, 2),
                       ("r257_8", 809, 257, 3, 8, 1, 2),
                       ("r130_none_L0", 823, 130, 30, 30, 1, 0),
                       ("r300_30", 824, 300, 36, 30, 1, 0),
                       ("r300_none", 821, 300, 34, None, 0.12, 2))


# full-size cases the reference finishes as well (minutes)
RECORDED_FULL = tuple(c for c in LONG_CASES if c[0] in ("n520_8", "n130_none_L0", "n300_none", "n1024_80"))


def long_trace(case):
    _, seed, n, steps, _, _, _ = case
    return stair_noise(seed, n, steps, min_len=3 if steps > 8 else n // 8)


# ---- the fixture -----------------------------------------------------------------------------------------------------------
def recorded_cases():
    """(name, trace, num_steps, multiplier, min_step_length) of every case tools/gen_chisq_golden.py --limits records."""
    out = [(n, v, ns, 1, 2) for n, v, ns in extreme_cases()]
    out += [(c[0], long_trace(c), c[4], c[5], c[6]) for c in LONG_CASES_RECORDED + RECORDED_FULL]
    return out


def golden():
    g = np.load(os.path.join(GOLD, "chisq_limits.npz"))
    out = []
    for i in range(len(g["case_len"])):
        fm, rm = g["fit_case"] == i, g["rec_case"] == i
        out.append(dict(name=str(g["case_name"][i]), lum=g["lum"][g["lum_off"][i]:g["lum_off"][i + 1]],
                        num_steps=int(g["case_num_steps"][i]) or None, mult=float(g["case_mult"][i]), L=int(g["case_L"][i]),
                        fit=list(zip(g["fit_start"][fm].tolist(), g["fit_stop"][fm].tolist(), g["fit_h"][fm].tolist())),
                        best=g["rec_best"][rm], counter=g["rec_counter"][rm], counter_n=g["rec_counter_n"][rm], S=g["rec_S"][rm]))
    return out


def check_no_unpinned_nan(recs):
    """the fit chosen among NaN S values is not pinned, so no case may have one among two or more records."""
    assert len(recs) == 1 or not any(math.isnan(r[3]) for r in recs)


# ---- B: block-stride on real traces ----------------------------------------------------------------------------------------
STRIDE_N = 2 * MAX_BLOCKS + 777
# (num_steps, multiplier, min_step_length, min_step_magnitude, ignore_counterfits): the reference's defaults, and a rejecting one
STRIDE_PARAMS = ((None, 1, 2, 0.0, False), (None, 1, 0, 5000.0, True))
STRIDE_BAD = (0, -3, "over", 1)         # lengths of the invalid rows ("over": max_frames + 1; 1: the derived num_steps is -1)


@functools.lru_cache(maxsize=None)
def stride_pool():
    """At most 512 distinct ragged traces: 3 - 40 frames from random_batch (flat ones and exact staircases among them), and
    group C's traces, so that those are followed by ordinary ones in the same block."""
    from _chisq_cases import random_batch
    pool = [v for v in random_batch(4242, 1200) if len(v) <= 40][:480]
    pool += [v for _, v, ns in extreme_cases() if ns is None]
    assert len(pool) <= 512
    return pool


@functools.lru_cache(maxsize=None)
def stride_rows():
    """-> (pool index, length handed to the device) per row.  Rows b, b + 8192, b + 16384 run in the same block: their pool
    traces are taken half and a quarter of the length-sorted pool apart."""
    pool = stride_pool()
    P = len(pool)
    order = np.argsort([len(v) for v in pool], kind="stable")
    r = np.arange(STRIDE_N)
    b, k = r % MAX_BLOCKS, r // MAX_BLOCKS
    idx = order[(b * 197 + np.array([0, P // 2, P // 4])[k]) % P]
    mf = max(len(v) for v in pool)
    lens = np.array([len(pool[i]) for i in idx], dtype=np.int32)
    bad = np.flatnonzero(r % 53 == 7)
    lens[bad] = [mf + 1 if STRIDE_BAD[j % 4] == "over" else STRIDE_BAD[j % 4] for j in range(len(bad))]
    return idx, lens


@functools.lru_cache(maxsize=None)
def stride_expected(k):
    """The restatement's (fit, records) of every pool trace under STRIDE_PARAMS[k]."""
    import _chisq_reference as R
    ns, mult, L, mag, ign = STRIDE_PARAMS[k]
    with np.errstate(all="ignore"):
        return [R.chi_squared(v.tolist(), mult, ns, L, mag, ign) for v in stride_pool()]


# ---- E: merge filter and R^2 at 8192 frames ------------------------------------------------------------------------------------
FILTER_CONFIGS = ((0, None, None), (1, 1e9, None), (1, None, 0.5), (1, 3000.0, 0.25))     # (mode, min_magnitude, min_noise_ratio)
FILTER_FRAMES = 8192


@functools.lru_cache(maxsize=None)
def filter_limit_cases():
    """[{"lum", "pin"}]: single-frame plateaus (cnt == n) at 8192 and 8191 frames, four long plateaus on zero-mean noise whose
    merges refit 3 100 - 8 192 frames (the sums nearly cancel: their last bits show the order of the additions; every other
    stated height is not the mean), a flat 8192-frame row (R^2 = 1 - 0 / 0) and short rows; 71 rows, no multiple of 64."""
    from _chisq_cases import random_batch
    rng = np.random.default_rng(606)
    cases = []
    for n in (8192, 8191):
        v = stair_noise(900 + n, n, 12, min_len=300)
        cases.append(dict(lum=v, pin=[(i, i, float(v[i])) for i in range(n)]))
    for k in range(12):
        n = 8192 if k % 3 == 0 else int(rng.integers(7689, 8192))
        v = rng.normal(0.0, 1e4, n)
        v -= np.mean(v)
        bounds = [0, 1030 + 7 * k, 3100 + 11 * k, 5200 - 9 * k, n]
        pin = [(a, b - 1, float(np.mean(v[a:b])) + (0.0 if j % 2 == 0 else float(rng.normal(0.0, 50.0))))
               for j, (a, b) in enumerate(zip(bounds[:-1], bounds[1:]))]
        cases.append(dict(lum=v, pin=pin))
    cases.append(dict(lum=np.full(8192, 7.25), pin=[(0, 8191, 7.25)]))
    for v in [t for t in random_batch(515, 400) if len(t) <= 60][:56]:
        n = len(v)
        cuts = np.sort(rng.choice(np.arange(1, n), int(rng.integers(0, min(n - 1, 6) + 1)), replace=False)).tolist()
        bounds = [0] + cuts + [n]
        cases.append(dict(lum=v, pin=[(a, b - 1, float(np.mean(v[a:b]))) for a, b in zip(bounds[:-1], bounds[1:])]))
    assert len(cases) % 64
    return cases


def filter_expected(cases, mode, mag, ratio):
    import _chisq_reference as R
    return [R.filter_upsteps(c["lum"].tolist(), c["pin"]) if mode == 0 else R.filter_small_steps(c["lum"].tolist(), c["pin"], mag, ratio)
            for c in cases]


# ---- F: contract -------------------------------------------------------------------------------------------------------------
UNSUPPORTED_CASES = (([1.0, 5.0, 2.0], 2), ([1.0, 5.0, 2.0, 7.0, 3.0, 9.0, 4.0, 8.0, 6.0], 8))      # (trace, num_steps), min_step_length 0


def records_until_raise(lum, num_steps):
    """The restatement's records of the fits tried before it raises the reference's ValueError (:306)."""
    import _chisq_reference as R
    recs = []
    try:
        R.chi_squared(lum, 1, num_steps, 0, records=recs)
    except ValueError as e:
        assert "is greater than len" in str(e)
        return recs
    raise AssertionError("the restatement did not raise")
