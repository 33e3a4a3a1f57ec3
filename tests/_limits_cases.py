"""Inputs of the limit tests (test_limits_host.py, test_gpu_stepfit_limits.py, test_gpu_sequence_limits.py): generated here
once so that the host twin checks exactly what the GPU tests run.  Nothing here needs a GPU."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
P_TINY = 1e-300                 # a true p below it is compared as 0 <= p <= 1e-299, not relatively
MAX_TINY_SHARE = 0.05           # of the sweep
MAX_SKIPPED_SHARE = 0.10        # of a test's traces, for `near` / `unsupported`


def stepfit_generator():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_stepfit_golden
    return gen_stepfit_golden


# ---- A1: the fixture of traces at the length limit -----------------------------------------------------------------------
def length_limit_cases():
    """tests/golden/stepfit_limits.npz (recorded from the reference) with the traces rebuilt from their seeds."""
    G = stepfit_generator()
    g = np.load(os.path.join(GOLD, "stepfit_limits.npz"))
    out = []
    for i in range(len(g["case_len"])):
        phot = G.limits_trace(int(g["case_seed"][i]), int(g["case_len"][i]))
        assert float(np.sum(phot)) == float(g["case_phot_sum"][i]), "the seeded trace generator drifted from the fixture"

        def part(k):
            return g[k][g[k + "_off"][i]:g[k + "_off"][i + 1]]

        def tab(pre):
            m = g[pre + "_trace"] == i
            return list(zip(g[pre + "_start"][m].tolist(), g[pre + "_stop"][m].tolist(), g[pre + "_h"][m].tolist()))
        out.append(dict(phot=phot, ck_out=part("ck_out"), p_pairs=part("p_pairs"), pl=tab("pl"), tf=tab("tf"),
                        mirror=int(g["case_mirror"][i]), ck=int(g["case_ck"][i]), drop_sort=bool(g["case_drop_sort"][i]),
                        thr=float(g["case_thr"][i]), first_pass_pairs=int(g["case_first_pass_pairs"][i])))
    return out


def pairwise_sum(a, depth=None):
    """numpy's pairwise sum (PW_BLOCKSIZE 128, 8 accumulators) in Python; depth limits the number of splits (None: as numpy)."""
    n = len(a)
    if n <= 128 or depth == 0:
        if n < 8:
            res = 0.0
            for x in a:
                res += float(x)
            return res
        r = np.array(a[:8], dtype=np.float64)
        i = 8
        while i < n - (n % 8):
            r = r + a[i:i + 8]
            i += 8
        res = float(((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7])))
        for x in a[i:]:
            res += float(x)
        return res
    n2 = n // 2
    n2 -= n2 % 8
    d = None if depth is None else depth - 1
    return pairwise_sum(a[:n2], d) + pairwise_sum(a[n2:], d)


def long_merge_cases(n_cases=48, seed=88):
    """Two plateaus of zero-mean noise that the t-filter merges into one of 7689 .. 8192 frames (lengths at which a pairwise
    sum that stops one level early adds up a block of more than 128 frames).  The sum nearly cancels, so its last bits show
    every change in the order of the additions.  -> [(luminosities, plateaus)]"""
    from scipy import stats
    G = stepfit_generator()
    rng = np.random.default_rng(seed)
    lengths = [n for n in range(7689, 8193) if G.pairwise_max_leaf(n, 6) > 128]
    out = []
    while len(out) < n_cases:
        n = 8191 if len(out) == 0 else int(rng.choice(lengths))
        lum = rng.normal(0.0, 1e4, n)
        lum -= np.mean(lum)                                        # (the sum is left with rounding residue only)
        cut = int(rng.integers(2, n - 2)) if len(out) % 3 else int(rng.integers(2, 200))
        if stats.ttest_ind(lum[:cut], lum[cut:], equal_var=False).pvalue < 0.05:
            continue
        out.append((lum, [(0, cut - 1, float(np.mean(lum[:cut]))), (cut, n - 1, float(np.mean(lum[cut:])))]))
    return out


# ---- A2: Welch p over the (t, df) plane -----------------------------------------------------------------------------------
def _welch(a, b):
    n1, n2 = len(a), len(b)
    v1, v2 = np.var(a, ddof=1) / n1, np.var(b, ddof=1) / n2
    df = (v1 + v2) ** 2 / (v1 ** 2 / (n1 - 1) + v2 ** 2 / (n2 - 1))
    return np.mean(a), np.mean(b), math.sqrt(v1 + v2), df


def p_sweep(n_points=6000, seed=424242):
    """Two-plateau traces: Welch df log-uniform over 1 .. 8190 (a sixth of them between 38 and 42, around the switch of the
    ln B series at df = 40), |t| log-uniform over 1e-9 .. 1e4, a tenth of the points within 0.1 % of the branch swap of the
    incomplete beta function (t^2 = 3 df / (df + 2)).  Where the true p would underflow (large df and large t), most points
    redraw t, so that at most MAX_TINY_SHARE of the sweep is left to the absolute comparison.
    Returns a list of (a, b) float64 arrays."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n_points):
        if k % 6 == 0:
            df_t = rng.uniform(38.0, 42.0)
        else:
            df_t = math.exp(rng.uniform(0.0, math.log(8190.0)))
        # n1 = n2 = n with equal variances gives df near 2 n - 2; unequal variances pull df down towards n - 1; df < 2 needs
        # a small first sample against a long quiet second one
        if df_t < 4.0:                                              # df near (1 + u)^2 with u the ratio of the two variances of the mean
            n1, n2 = 2, int(rng.integers(20, 200))
            s2 = math.sqrt(max(math.sqrt(df_t) - 1.0, 1e-6) * n2 / 2.0)
        else:
            n = int(math.ceil(df_t / 2.0 + 1.0)) + int(rng.integers(0, 2))
            n1 = n2 = min(n, 4096)
            s2 = 1.0
            full = 2.0 * n1 - 2.0
            if df_t < full and n1 > 2:                              # variance ratio q with df(q) = df_t: (1 + q)^2 / (1 + q^2) = df_t / (n - 1)
                c = df_t / (n1 - 1.0)
                if 1.0 < c < 2.0:
                    s2 = math.sqrt(((1.0) + math.sqrt(max(1.0 - (c - 1.0) ** 2, 0.0))) / (c - 1.0)) if c > 1.0 else 1.0
        a = rng.normal(0.0, 1000.0, n1)
        b = rng.normal(0.0, 1000.0 * s2, n2)
        m1, m2, se, df = _welch(a, b)
        for attempt in range(40):
            if k % 10 == 1:
                t = math.sqrt(3.0 * df / (df + 2.0)) * (1.0 + rng.uniform(-1e-3, 1e-3))
            else:
                t = 10.0 ** rng.uniform(-9.0, 4.0)
            lp = -0.5 * (df - 1.0) * math.log1p(t * t / df)         # the tail's leading factor
            if lp > -660.0 or (k % 10 == 0 and attempt == 0):       # ln 1e-300 = -690.8
                break
        t = t if rng.random() < 0.5 else -t
        b = b + ((m1 - m2) - t * se)                                # mean(a) - mean(b) = t * se
        out.append((a, b))
    return out


def sweep_scipy(points):
    """scipy.stats.ttest_ind(a, b, equal_var=False) of every point -> (p, t, df) float64 arrays."""
    from scipy import stats
    p, t, df = (np.empty(len(points)) for _ in range(3))
    for i, (a, b) in enumerate(points):
        r = stats.ttest_ind(a, b, equal_var=False)
        p[i], t[i], df[i] = r.pvalue, r.statistic, r.df
    return p, t, df


def mp_p(t, df):
    """Two-sided Student p at 50 digits: I_x(df / 2, 1 / 2), x = df / (df + t^2), as a float (0.0 where it underflows)."""
    import mpmath
    with mpmath.workdps(50):
        t, df = mpmath.mpf(float(t)), mpmath.mpf(float(df))
        v = mpmath.betainc(df / 2, mpmath.mpf(1) / 2, 0, df / (df + t * t), regularized=True)
        return float(v)


def mp_subsample(n, k=2000, seed=9):
    return np.sort(np.random.default_rng(seed).choice(n, min(k, n), replace=False))


# ---- A2 / A3: random traces ---------------------------------------------------------------------------------------------------
def random_traces(rng, lengths):
    out = []
    for n in lengths:
        nf = int(rng.integers(0, 5))
        lvl = np.full(n, float(nf))
        for _k in range(nf):
            lvl[int(rng.integers(0, n)):] -= 1
        v = lvl * rng.uniform(5e3, 3e4) + rng.normal(0, rng.uniform(1e3, 6e3), n)
        out.append(np.round(v * 2) / 2 if rng.random() < 0.5 else np.round(v))
    return out


BOUNDARY_LENGTHS = (3, 4, 64, 65, 127, 128, 129)
CK16 = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16, 21, 27, 34, 45, 55, 64)
# (name, seed, mirror, ck, window_radius, drop_sort, window_lengths, M)
PARAM_LIMIT_SETS = (("radius64", 301, 3, 0, 64, True, (2, 4, 8, 16), 10),
                    ("ck16_M64", 302, 3, 1, 6, True, CK16, 64),
                    ("ck16_M1", 303, 0, 1, 6, False, CK16, 1),
                    ("radius64_ck16_M64", 304, 2, 1, 64, True, CK16, 64))


def param_limit_traces(seed, wr):
    rng = np.random.default_rng(seed)
    extra = rng.integers(5, 200 if wr > 20 else 400, 5 if wr > 20 else 17).tolist()
    return random_traces(rng, list(BOUNDARY_LENGTHS) + extra)


def sliding_p_traces(wr):
    rng = np.random.default_rng(7000 + wr)
    return random_traces(rng, [3, 9, 40, 64, 65, 129, 200, 257] if wr == 64 else [1, 2, 5, 11, 12, 64, 65, 127, 128, 129, 400, 1000])


def sliding_p_scipy(seqs, wr):
    """p of every (radius, frame) of sliding_t_fitter's windows (seq[f - r:f] against seq[f:f + r], Python slices) of every
    sequence by scipy.stats.ttest_ind(equal_var=False): the windows of all sequences are grouped by their two lengths and
    every group is one vectorised call.  -> [float64 [window_radius - 5, len(seq)]], NaN where a window is empty."""
    from scipy import stats
    seqs = [np.asarray(q, dtype=np.float64) for q in seqs]
    out = [np.full((max(wr - 5, 0), len(q)), np.nan) for q in seqs]
    groups = {}
    for j, seq in enumerate(seqs):
        n = len(seq)
        for k, r in enumerate(range(5, wr)):
            for f in range(n):
                a, b = seq[f - r:f] if f - r >= -n else seq[0:f], seq[f:f + r]
                if len(a) and len(b):
                    groups.setdefault((len(a), len(b)), []).append((j, k, f, a, b))
    with np.errstate(all="ignore"):
        for items in groups.values():
            p = stats.ttest_ind(np.stack([i[3] for i in items]), np.stack([i[4] for i in items]), axis=1, equal_var=False).pvalue
            for (j, k, f, _, _), v in zip(items, p):
                out[j][k, f] = v
    return out


# ---- A4: the two sort paths ------------------------------------------------------------------------------------------------------
_A = np.array([10.0, 12.0, 11.0, 13.5])
_B = np.array([11.0, 13.0, 10.5, 12.0])


def periodic_case(n_plateaus, breaks=(), width=4):
    """A staircase of n_plateaus plateaus of `width` frames that alternate between two fixed shapes of equal mean, each one
    `step` above the one before.  All values are multiples of 1 / 2, so every sum is exact and every pair test has the
    bit-identical p (about 0.1: the pair merges), except next to a plateau listed in `breaks`, which is lifted by 1e6.  Two
    merged pairs stand two steps apart with twice the frames (p < 0.001: they stay), so the final plateaus show which pairs
    of a tie run the first pass took, i.e. the order in which the sort left the ties."""
    reps = width // 4
    step = 2.0 / reps
    lum = np.concatenate([np.tile(_A if i % 2 == 0 else _B, reps) + step * i + (1e6 if i in breaks else 0.0)
                          for i in range(n_plateaus)])
    pl = [(width * i, width * i + width - 1, float(np.mean(lum[width * i:width * i + width]))) for i in range(n_plateaus)]
    return lum, pl


def nan_mix_case(n_groups):
    """noisy, noisy, constant, constant, constant, ...: pairs of equal constants have p = NaN, the others a finite p (the two
    noisy ones usually merge); fewer than 64
    pairs, so CPython's insertion sort decides where the NaN keys stay."""
    rng = np.random.default_rng(31)
    parts = []
    for g in range(n_groups):
        parts += [rng.normal(100.0 + 3.0 * (g % 3), 5.0, 5).round(1), rng.normal(100.0 + 3.0 * (g % 3), 5.0, 6).round(1),
                  np.full(3, 50.0 + (g % 2)), np.full(4, 50.0 + (g % 2)), np.full(2, 50.0)]
    lum = np.concatenate(parts)
    b = np.cumsum([0] + [len(p) for p in parts])
    pl = [(int(b[i]), int(b[i + 1] - 1), float(np.mean(lum[b[i]:b[i + 1]]))) for i in range(len(parts))]
    return lum, pl


def sort_cases():
    """name -> (luminosities, plateaus, no_merge_start, tied): pairs in the first pass = plateaus - 1."""
    c = {}
    for npairs in (63, 64, 65):
        c["ties_%d" % npairs] = periodic_case(npairs + 1, breaks=(7,)) + (0, True)
        c["ties_%d_nms" % npairs] = periodic_case(npairs + 1, breaks=(20, 42)) + (9, True)
    c["ties_400"] = periodic_case(401, breaks=(100, 101, 333)) + (0, True)
    c["ties_700_wide"] = periodic_case(701, breaks=(5, 350), width=8) + (3, True)
    c["nan_mix_14"] = nan_mix_case(3) + (0, False)
    c["nan_mix_59"] = nan_mix_case(12) + (2, False)
    return c


SORT_THR = 0.01
