"""Inputs and expected values of the limit tests of the single-precision PSF solver (FSQ_MODE_TEXTBOOK_F32, csrc/fsq_fit_f32.h):
tests/test_f32_limits_host.py proves that they reach the edges named here and measures the restatement's constants,
tests/test_gpu_f32_limits.py feeds them to the device.  Everything is seeded and built once.  No torch, no GPU.

  E  evaluation points: 4 157 parameter vectors inside the bounds (a quarter with bounded parameters on their bounds, theta = 0
     and 360 among them) on ROIs of uniform pixels, all-0 and all-65 535 ROIs at the end; eval_reference gives the float64
     evaluation of the same formulas and the cancellation-free magnitudes the error bound is written in
  S  conditioned spots: 3 200 Poisson spots, of which those are kept that the fp64 oracle (the reference's textbook solver) fits
     within 5 % of the truth in all seven parameters; the kept indices are recorded in tests/golden/f32_limits_spots.npz
  B  bound cases: ROIs whose least-squares optimum lies outside the box, each naming the parameter that must end on its bound
  R  the refill batch: 257 distinct ROIs tiled over more fits than two rounds of the persistent grid take"""
import functools
import os
import zlib

import numpy as np

import _f32_reference as R
from _util import DEGEN_NAMES, GOLD, load_field, rois_of

f32, f64 = np.float32, np.float64
LO = np.array([0, 0, 2, 2, .75, .75, 0], f64)
HI = np.array([60000, 65535, 3, 3, 2, 2, 360], f64)          # (the first two: the range E draws from; the solver has no such bound)
BATCHES = (1, 63, 64, 65)                                     # ... and all at once
U = 2.0 ** -24                                                # the unit of the evaluation bound: half an ulp of 1 in float32
# The evaluation bound |N - N64| <= c U sum m_a m_b, |g - g64| <= c U sum m_a m_r, |chi2 - chi2_64| <= c U chi2_64: what the float32
# restatement reaches on E in these units (measured by test_f32_limits_host.py, which asserts that it stays below and within a
# factor 2 of these figures), and the kernel's allowance: 16 times that (__expf, hardware rcp and sincosf, a few ulp each, and
# another summation order).  Never taken from the kernel's own error.
RESTATEMENT_UNITS = {"N": 1.0, "g": 3.0, "chi2": 6.0}
KERNEL_FACTOR = 16.0


# ---- E: evaluation points -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def eval_points():
    """(x float32 [n, 7], rois uint16 [n, 25]), n = 4 157"""
    rng = np.random.default_rng(20250901)
    n, q = 4096, 1024
    x = LO + (HI - LO) * rng.random((n, 7))
    on = np.zeros((n, 7), bool)
    on[:q // 2] = True                                        # every parameter on one of its two bounds
    on[q // 2:q] = rng.random((q // 2, 7)) < 0.5              # each parameter on a bound with probability one half
    x = np.where(on, np.where(rng.random((n, 7)) < 0.5, LO, HI), x)
    rois = rng.integers(0, 65536, (n, 25))
    flat = np.repeat([0, 65535], [31, 30])                    # all-0 and all-65 535 ROIs, a fresh point each; 4 157 = 64 x 64 + 61
    x = np.concatenate([x, LO + (HI - LO) * rng.random((len(flat), 7))])
    rois = np.concatenate([rois, flat[:, None] * np.ones((1, 25), np.int64)])
    return x.astype(f32), rois.astype(np.uint16)


def eval_reference(x, rois):
    """The float64 evaluation at the float32 points x and the bounds' magnitudes:
    (chi2 [n], N [n, 28], g [n, 7], sum m_a m_b [n, 28], sum m_a m_r [n, 7]) with, per pixel, L = |x3 - row| + |x2 - col|,
    ub = L / sigma_h, vb = L / sigma_w, amp = (1 + ub^2 + vb^2)(1 + |phi|), m = (1, E amp, aE (ub / sigma_h + vb / sigma_w) amp (twice),
    aE ub^2 / sigma_h amp, aE vb^2 / sigma_w amp, aE L (ub / sigma_h + vb / sigma_w) amp pi / 180), m_r = |H| + aE amp + |d|."""
    x = np.asarray(x, f32).astype(f64)
    d = np.asarray(rois).reshape(len(x), 25).astype(f64)
    chi2, N, g = R.evaluate(x, d, f64)
    E, _ = R.jacobian(x, f64)
    L = np.abs(x[:, 3:4] - R.ROWS[None]) + np.abs(x[:, 2:3] - R.COLS[None])
    s4, s5 = x[:, 4:5], x[:, 5:6]
    ub, vb = L / s4, L / s5
    amp = (1 + ub * ub + vb * vb) * (1 + np.abs(x[:, 6:7] * (np.pi / 180)))
    aE = np.abs(x[:, 1:2]) * E
    w = ub / s4 + vb / s5
    m = np.stack([np.ones_like(E), E * amp, aE * w * amp, aE * w * amp, aE * ub * ub / s4 * amp, aE * vb * vb / s5 * amp,
                  aE * L * w * amp * (np.pi / 180)], axis=2)
    mr = np.abs(x[:, 0:1]) + aE * amp + np.abs(d)
    mN = np.einsum("npa,npa->na", m[:, :, R.TRI_I], m[:, :, R.TRI_J])
    mg = np.einsum("npa,np->na", m, mr)
    return chi2, N, g, mN, mg


def eval_units(chi2, N, g, ref):
    """the largest errors of an evaluation (chi2, N, g) in units of U times the magnitudes of `ref` = eval_reference(...):
    per point, ([n] for N, [n] for g, [n] for chi2); 0 / 0 counts as 0"""
    c64, N64, g64, mN, mg = ref
    with np.errstate(divide="ignore", invalid="ignore"):
        eN = np.nan_to_num(np.abs(np.asarray(N, f64) - N64) / (U * mN), nan=0.0).max(1)
        eg = np.nan_to_num(np.abs(np.asarray(g, f64) - g64) / (U * mg), nan=0.0).max(1)
        ec = np.nan_to_num(np.abs(np.asarray(chi2, f64) - c64) / (U * c64), nan=0.0)
    return eN, eg, ec


# ---- S: conditioned spots -----------------------------------------------------------------------------------------------------
N_SPOTS = 3200
SPOTS_FILE = os.path.join(GOLD, "f32_limits_spots.npz")


@functools.lru_cache(maxsize=None)
def all_spots():
    """(truth float64 [N_SPOTS, 7], rois uint16 [N_SPOTS, 25]): offset 100 ... 2 000, amplitude 5 000 ... 40 000, centres 2.15 ... 2.85,
    widths 0.9 ... 1.8 at least 0.25 apart, theta 5 ... 40 degrees, Poisson noise"""
    rng = np.random.default_rng(20250902)
    n = N_SPOTS
    s4 = 0.9 + 0.9 * rng.random(n)
    s5 = 0.9 + 0.9 * rng.random(n)
    for _ in range(200):                                     # redraw the second width until the two differ by 0.25
        close = np.abs(s4 - s5) < 0.25
        if not close.any():
            break
        s5[close] = 0.9 + 0.9 * rng.random(int(close.sum()))
    assert (np.abs(s4 - s5) >= 0.25).all()
    truth = np.stack([100 + 1900 * rng.random(n), 5000 + 35000 * rng.random(n), 2.15 + 0.7 * rng.random(n), 2.15 + 0.7 * rng.random(n),
                      s4, s5, 5 + 35 * rng.random(n)], axis=1)
    E, _ = R.jacobian(truth, f64)
    rois = rng.poisson(truth[:, 0:1] + truth[:, 1:2] * E)
    return truth, np.clip(rois, 0, 65535).astype(np.uint16)


def select_spots(fitted):
    """indices of the spots that `fitted` [N_SPOTS, 7] reproduces within 5 % of the truth in all seven parameters"""
    truth, _ = all_spots()
    return np.flatnonzero((np.abs(fitted - truth) <= 0.05 * np.abs(truth)).all(axis=1))


@functools.lru_cache(maxsize=None)
def spots():
    """(truth [n, 7], rois uint16 [n, 25]) of the recorded selection (test_f32_limits_host.py redoes it with the oracle)"""
    truth, rois = all_spots()
    rec = np.load(SPOTS_FILE)
    assert zlib.crc32(rois.tobytes()) == int(rec["rois_crc"]), "the seeded spots drifted from the recorded selection"
    keep = rec["kept"].astype(np.int64)
    return truth[keep], rois[keep]


def chi2_f64(x, rois):
    """sum of squared residuals of the parameters x [n, 7] on the ROIs, in float64"""
    x = np.asarray(x, f64)
    E, _ = R.jacobian(x, f64)
    r = x[:, 0:1] + x[:, 1:2] * E - np.asarray(rois).reshape(len(x), 25).astype(f64)
    return (r * r).sum(1)


def solver_figures(x, niter, status, oracle_p, rois):
    """what item b asserts of a solver's result on S against the oracle's parameters: the share within 1e-3 relative in all seven
    parameters, the share whose float64 chi2 is at most (1 + 1e-4) times the oracle's, median and 99th percentile of niter, the
    number of exits 5"""
    rel = (np.abs(x - oracle_p) / np.maximum(np.abs(oracle_p), 1e-12)).max(axis=1)
    return {"share_1e-3": float((rel <= 1e-3).mean()),
            "share_chi2": float((chi2_f64(x, rois) <= (1 + 1e-4) * chi2_f64(oracle_p, rois)).mean()),
            "niter_median": float(np.median(niter)), "niter_p99": float(np.percentile(niter, 99)),
            "exit5": int((np.asarray(status) == 5).sum())}


@functools.lru_cache(maxsize=None)
def restatement_on_spots():
    """(x, status, niter, nfev) of the float32 restatement on S"""
    return R.fit(spots()[1])


# ---- B: bound cases -----------------------------------------------------------------------------------------------------------
def _gauss(H, A, c_row, c_col, s):
    r, c = np.mgrid[0:5, 0:5]
    return H + A * np.exp(-0.5 * ((r - c_row) ** 2 + (c - c_col) ** 2) / (s * s))


@functools.lru_cache(maxsize=None)
def bound_cases():
    """[(name, roi uint16 [25], parameter index or None, bound or None)]: the named parameter must end exactly on the bound (for the
    amplitude the bound is float32((max - mean) / 3), given as None here and computed by amplitude_floor)"""
    out = []

    def add(name, roi, k=None, bound=None):
        out.append((name, np.clip(np.rint(roi), 0, 65535).astype(np.uint16).reshape(25), k, bound))
    for floor, peak in ((1000, 30000), (200, 65535), (5000, 9000)):        # one hot pixel on a flat floor: narrower than the box allows
        roi = np.full((5, 5), float(floor))
        roi[2, 2] = peak
        add("hot_pixel_%d_%d" % (floor, peak), roi, 4, 0.75)
        add("hot_pixel_%d_%d_w" % (floor, peak), roi, 5, 0.75)
    for s in (4.0, 6.0, 10.0):                                             # a plateau wider than the window
        add("plateau_%g" % s, _gauss(500, 20000, 2.5, 2.5, s), 4, 2.0)
        add("plateau_%g_w" % s, _gauss(500, 20000, 2.5, 2.5, s), 5, 2.0)
    for (r, c) in ((0, 0), (0, 4), (4, 0), (4, 4)):                        # spots centred on the corner pixels
        roi = _gauss(800, 25000, r, c, 1.1)
        add("corner_%d_%d_row" % (r, c), roi, 3, 2.0 if r == 0 else 3.0)   # (x[3] pairs with the row, x[2] with the column)
        add("corner_%d_%d_col" % (r, c), roi, 2, 2.0 if c == 0 else 3.0)
    rng = np.random.default_rng(20250903)
    for i in range(4):                                                     # a faint bump under one outlier pixel: A sits on its floor
        roi = _gauss(1000, 40, 2.3 + 0.1 * i, 2.6, 1.2) + rng.normal(0, 3, (5, 5))
        roi[0, 4 * (i & 1)] += 900
        add("faint_%d" % i, roi, 1, None)
    for v in (0, 1, 65535):
        add("flat_%d" % v, np.full((5, 5), float(v)))
    for name in DEGEN_NAMES:                                               # the ROIs of the committed degenerate frames
        g, img = load_field(name, prefix="degen_")
        if len(g["candidates"]):
            for j, roi in enumerate(rois_of(img, g["candidates"])[:8]):
                add("%s_%d" % (name, j), roi.astype(f64))
    return tuple(out)


def bound_rois():
    return np.stack([c[1] for c in bound_cases()])


def amplitude_floor(rois):
    """float32((max - mean) / 3) as kinit and the kernel compute it, as float64 values"""
    d = np.asarray(rois).reshape(-1, 25).astype(f64)
    return ((d.max(1) - d.sum(1) / 25.0) / 3.0).astype(f32).astype(f64)


def noise_rois(n=2000, seed=20250904):
    """seeded noise ROIs of several levels and spreads: where the exit-code search of the host test looks beyond the fixtures"""
    rng = np.random.default_rng(seed)
    level = 10.0 ** rng.uniform(0.5, 4.5, (n, 1))
    spread = level * 10.0 ** rng.uniform(-3, -0.3, (n, 1))
    return np.clip(np.rint(level + spread * rng.standard_normal((n, 25))), 0, 65535).astype(np.uint16)


EXIT_CODES = (1, 2, 4, 5)
PER_CODE = 8                        # ROIs kept per exit code: one fit is chaotic at the last bits, so the kernel is asked to reach a
                                    # code on at least one of the ROIs on which the restatement reaches it, not on a given one


@functools.lru_cache(maxsize=None)
def exit_code_rois():
    """{exit code: uint16 [<= PER_CODE, 25]}: for every exit code of the float32 restatement the first ROIs that reach it among
    textbook_f3_hard_256, B and the seeded noise ROIs (codes 1 and 2 come from the first two, 4 and 5 from the noise)"""
    g, img = load_field("f3_hard_256", prefix="textbook_")
    pool = np.concatenate([rois_of(img, g["candidates"]), bound_rois(), noise_rois()])
    _, status, _, _ = R.fit(pool)
    return {code: pool[np.flatnonzero(status == code)[:PER_CODE]] for code in EXIT_CODES}


def spot_conditions(fig, base):
    """the conditions of item b that the figures `fig` of a solver on S miss, given the float32 restatement's `base` (both from
    solver_figures): the share within 1e-3 of the oracle at least the restatement's minus 0.03, the chi2 share at least 0.99, the
    median of niter at most the restatement's + 2 and its 99th percentile at most + 6 (rounding differences between NumPy and the
    device's intrinsics), no exit 5"""
    missed = []
    if not fig["share_1e-3"] >= base["share_1e-3"] - 0.03:
        missed.append("share_1e-3")
    if not fig["share_chi2"] >= 0.99:
        missed.append("share_chi2")
    if not fig["niter_median"] <= base["niter_median"] + 2:
        missed.append("niter_median")
    if not fig["niter_p99"] <= base["niter_p99"] + 6:
        missed.append("niter_p99")
    if fig["exit5"]:
        missed.append("exit5")
    return missed


# ---- R: the refill batch ------------------------------------------------------------------------------------------------------
N_REFILL = 257                                                             # coprime to 64: a given ROI meets every lane


@functools.lru_cache(maxsize=None)
def refill_rois():
    """257 distinct ROIs: the bound cases, then the ROIs of textbook_f3_hard_256 with the most and the fewest iterations of the
    float32 restatement, half each"""
    g, img = load_field("f3_hard_256", prefix="textbook_")
    hard = np.unique(rois_of(img, g["candidates"]), axis=0)
    b = np.unique(bound_rois(), axis=0)[:40]
    hard = hard[~(hard[:, None, :] == b[None]).all(2).any(1)]
    _, _, niter, _ = R.fit(hard)
    order = np.argsort(niter, kind="stable")
    k = N_REFILL - len(b)
    pick = np.concatenate([order[:k // 2], order[len(order) - (k - k // 2):]])
    rois = np.concatenate([b, hard[pick]])
    assert len(np.unique(rois, axis=0)) == N_REFILL == len(rois)
    rng = np.random.default_rng(20250905)
    return rois[rng.permutation(N_REFILL)]                                 # (long and short fits side by side in a wave)


def refill_count(cus):
    """more than two rounds of the persistent grid (12 waves of 64 lanes per CU) and a partial wave"""
    return 2 * 12 * 64 * int(cus) + 65
