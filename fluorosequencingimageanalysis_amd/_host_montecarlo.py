"""NumPy / math twin of the seeded Monte-Carlo PSF fit (include/fsq_montecarlo.h): the reference's
_fit_2d_gaussian_monte_carlo (pflib.py:117-177) and the fit_type='monte_carlo' branch of find_peptides (:441-477) under this
library's explicit draws.

Draw j of an (iteration, pixel, field) triple: Philox block j >> 1 at counter (block, iteration, pixel, field) under key
(seed & 0xffffffff, seed >> 32); even j takes words (0, 1), odd j words (2, 3); the uniform is CPython's 53-bit one.  Every
iteration starts numpy's legacy polar method with an empty cache and runs it three times (H, A; h_0, w_0; sigmah, sigmaw).

What numpy rounds the same way on every machine (+, -, *, /, sqrt on arrays) is vectorised over the iterations; exp, log and
pow(x, 2.0) go through `math`, one libm call each, as the reference's scalar and glibc-backed array operations do."""
import math

import numpy as np

from . import _host_peptide_sim as PS

OK, NEVER_IMPROVED, NO_MAXIMUM = 0, 1, 2
INDEX_ERROR_TEXT = "index 0 is out of bounds for axis 0 with size 0"
UNBOUND_TEXT = "local variable 'h_0_current' referenced before assignment"
MAX_N_ITER = 2 ** 31 - 1
_EDGE = [0, 1, 2, 3, 4, 20, 21, 22, 23, 24, 5, 9, 10, 14, 15, 19]     # illumina_s_n's order (pflib.py:279-280)


def check_args(n_iter, seed):
    if not 1 <= int(n_iter) <= MAX_N_ITER:
        raise ValueError("N_iter must be in 1 .. 2^31 - 1")
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("seed must be in 0 .. 2^64 - 1")


def uniform(seed, iteration, pixel, field, j):
    """Draw j of (iteration, pixel, field)."""
    w = PS.philox((j >> 1, iteration, pixel, field), (seed & PS.MASK32, seed >> 32))
    return PS._uniform(w[0], w[1]) if j % 2 == 0 else PS._uniform(w[2], w[3])


def normals(seed, iteration, pixel, field):
    """The six normals of one iteration, in the order the reference draws them (scalar path: _host_peptide_sim.Normals)."""
    j = [0]

    def u():
        j[0] += 1
        return uniform(seed, iteration, pixel, field, j[0] - 1)
    g = PS.Normals(u)
    return [g() for _ in range(6)]


def _libm(fn, a):
    flat = np.ascontiguousarray(a, dtype=np.float64).reshape(-1).tolist()
    return np.array([fn(x) for x in flat], dtype=np.float64).reshape(np.shape(a))


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def _log(x):
    return math.log(x) if x > 0 else (-math.inf if x == 0 else math.nan)


def _pow2(x):
    try:
        return math.pow(x, 2.0)
    except OverflowError:
        return math.inf


def normals_np(seed, first_iteration, n, pixel, field):
    """normals() of the iterations first_iteration .. + n - 1: float64 [n, 6].  One Philox block is one attempt of the polar
    method; pair p of an iteration is its (p + 1)-th accepted block."""
    its = np.arange(first_iteration, first_iteration + n, dtype=np.uint64)
    nb = 8
    while True:
        c = np.empty((n, nb, 4), dtype=np.uint64)
        c[:, :, 0] = np.arange(nb, dtype=np.uint64)[None, :]
        c[:, :, 1] = its[:, None]
        c[:, :, 2] = pixel
        c[:, :, 3] = field
        w = PS.philox_np(c.reshape(-1, 4), (seed & PS.MASK32, seed >> 32)).astype(np.uint64).reshape(n, nb, 2, 2)
        u = ((w[..., 0] >> np.uint64(5)) * np.uint64(67108864) + (w[..., 1] >> np.uint64(6))).astype(np.float64) / 9007199254740992.0
        x1, x2 = 2.0 * u[..., 0] - 1.0, 2.0 * u[..., 1] - 1.0
        r2 = x1 * x1 + x2 * x2
        ok = (r2 > 0.0) & (r2 < 1.0)
        if (ok.sum(axis=1) >= 3).all():
            break
        nb *= 2
    rank = np.cumsum(ok, axis=1)
    out = np.empty((n, 6))
    rows = np.arange(n)
    for p in range(3):
        at = np.argmax(ok & (rank == p + 1), axis=1)
        a, b, r = x1[rows, at], x2[rows, at], r2[rows, at]
        f = np.sqrt(-2.0 * _libm(_log, r) / r)
        out[:, 2 * p], out[:, 2 * p + 1] = f * b, f * a
    return out


def parameters_np(z, h0mean, w0mean):
    """(H, A, h_0, w_0, sigmah, sigmaw) float64 [n, 6] of the normals z [n, 6] (pflib.py:151-156): loc + scale * z, rounded apart."""
    p = np.empty_like(z)
    p[:, 0] = np.abs(0.0 + 0.1 * z[:, 0])
    p[:, 1] = np.abs(1.0 + 0.2 * z[:, 1])
    p[:, 2] = np.clip(float(h0mean) + 0.3 * z[:, 2], 0.01, 4.99)
    p[:, 3] = np.clip(float(w0mean) + 0.3 * z[:, 3], 0.01, 4.99)
    p[:, 4] = np.abs(1.2 + 0.3 * z[:, 4])
    p[:, 5] = np.abs(1.0 + 0.3 * z[:, 5])
    return p


def _sum25(a):
    """np.sum over the last axis of 25 contiguous doubles: numpy's pairwise leaf (eight accumulators, then the tail)."""
    r = a[..., 0:8] + a[..., 8:16]
    r = r + a[..., 16:24]
    return (((r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])) + ((r[..., 4] + r[..., 5]) + (r[..., 6] + r[..., 7]))) + a[..., 24]


def _sum16(a):
    r = a[0:8] + a[8:16]
    return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))


def trials_np(p, roi):
    """The trials of the parameter rows p [n, 6] on roi [25]: (normalised images [n, 25], RMS [n]) (pflib.py:159-163)."""
    with np.errstate(all="ignore"):
        den = 2.0 * _libm(_pow2, p[:, 4])
        r, c = np.repeat(np.arange(5.0), 5), np.tile(np.arange(5.0), 5)
        dh, dw = r[None, :] - p[:, 2:3], c[None, :] - p[:, 3:4]
        g = p[:, 1:2] * _libm(_exp, -((dh * dh + dw * dw) / den[:, None])) + p[:, 0:1]
        g = g / np.max(g, axis=1)[:, None]
        d = roi[None, :] - g
        return g, np.sqrt(_sum25(d * d))


CHUNK = 4096


def best_of(roi, n_iter, seed, pixel=0, field=0):
    """The loop of pflib.py:150-172 on a float ROI [25] -> dict(status, first, start, rms, niter, params [6] or None, fit [25],
    running) - `running`: the winner's iteration number after every iteration (-1 while there is none), for the prefix
    property."""
    check_args(n_iter, seed)
    roi = np.ascontiguousarray(roi, dtype=np.float64).reshape(25)
    vmax = np.max(roi)
    eq = np.nonzero(roi == vmax)[0]
    if len(eq) == 0:
        return {"status": NO_MAXIMUM, "rms": 0.0, "niter": -1, "params": None, "fit": np.zeros(25), "vmax": vmax,
                "running": np.full(n_iter, -1, np.int64)}
    first = int(eq[0])
    h0mean, w0mean = first // 5, first % 5
    with np.errstate(all="ignore"):
        start = 250000000 * vmax
    best, best_it, best_p, fit = start, -1, None, None
    running = np.empty(n_iter, np.int64)
    for a in range(0, n_iter, CHUNK):
        n = min(CHUNK, n_iter - a)
        p = parameters_np(normals_np(seed, a, n, pixel, field), h0mean, w0mean)
        g, rms = trials_np(p, roi)
        fit = g[-1]
        # the strict `<` against the running best: an iteration wins when it is below everything before it
        with np.errstate(all="ignore"):
            before = np.concatenate([[best], np.fmin.accumulate(np.where(rms < best, rms, best))[:-1]])
            wins = rms < before
        idx = np.nonzero(wins)[0]
        run = np.full(n, best_it, np.int64)
        if len(idx):
            marks = np.zeros(n, np.int64)
            marks[idx] = idx + a + 1
            run = np.maximum.accumulate(marks) - 1
            run[run < 0] = best_it
            best, best_it, best_p = float(rms[idx[-1]]), int(idx[-1]) + a, p[idx[-1]].copy()
        running[a:a + n] = run
    return {"status": OK if best_it >= 0 else NEVER_IMPROVED, "rms": float(best), "niter": best_it, "params": best_p,
            "fit": fit.copy(), "vmax": vmax, "first": first, "start": start, "running": running}


def metrics(roi, fit):
    """(rmse, r_2, s_n) of pflib.py:463-473 on the float ROI [25] and the image [25]: Python's sequential sums, numpy scalar
    powers for rmse, np.mean / np.std of the 16 edge values."""
    roi = np.ascontiguousarray(roi, dtype=np.float64).reshape(25)
    fit = np.ascontiguousarray(fit, dtype=np.float64).reshape(25)
    with np.errstate(all="ignore"):
        mean = (0.0 + _sum25(roi)) / 25.0
        d = roi - fit
        e = roi - mean
        num = den = rm = 0.0
        for x, y in zip((d * d).tolist(), (e * e).tolist()):
            num += x
            den += y
        for x in d.tolist():
            rm += _pow2(x)
        r2 = np.float64(1.0) - np.float64(num) / np.float64(den)
        rmse = math.sqrt(rm / 25.0) if rm == rm else math.nan
        op = roi[_EDGE]
        m16 = (0.0 + _sum16(op)) / 16.0
        dev = op - m16
        sd = np.sqrt((0.0 + _sum16(dev * dev)) / 16.0)
        s_n = (np.max(roi) - m16) / sd
    return float(rmse), float(r2), float(s_n)


def fit_roi(roi, n_iter=1000, seed=0, pixel=0, field=0, h=2, w=2, cand_field=0):
    """What fsq_mc_fit_rois / fsq_mc_fit_candidates write for one candidate: dict(row: the FsqRow's fields, fit [25], rms,
    status)."""
    b = best_of(roi, n_iter, seed, pixel, field)
    st = b["status"]
    p = b["params"] if b["params"] is not None else np.zeros(6)
    if st == NO_MAXIMUM:
        rmse = r2 = s_n = 0.0
    else:
        rmse, r2, s_n = metrics(roi, b["fit"])
    row = {"h0": float(p[2]) + float(h) - 2.5, "w0": float(p[3]) + float(w) - 2.5, "H": float(p[0]), "A": float(p[1]),
           "sigma_h": float(p[4]), "sigma_w": float(p[5]), "theta": 0.0, "rmse": rmse, "r2": r2, "s_n": s_n, "p2": float(p[2]),
           "p3": float(p[3]), "h": int(h), "w": int(w), "field": int(cand_field), "status": st, "niter": b["niter"],
           "nfev": int(n_iter), "key_h": -1, "key_w": -1}
    return {"row": row, "fit": b["fit"], "rms": b["rms"], "status": st, "running": b["running"]}


def normalise(sub):
    """pflib.py:446-447 on an integer ROI: (sub - min) / float(max of that); a constant ROI gives NaN."""
    sub = np.asarray(sub).astype(np.int64)
    sub = sub - np.min(sub)
    with np.errstate(all="ignore"):
        return sub / float(np.max(sub))


def raise_for(status):
    """The reference's exception for a fit status (nothing for OK)."""
    if status == NO_MAXIMUM:
        raise IndexError(INDEX_ERROR_TEXT)
    if status == NEVER_IMPROVED:
        raise UnboundLocalError(UNBOUND_TEXT)


def fit_2d_gaussian_monte_carlo(subimage, n_iter=1000, seed=0, candidate=(0, 0)):
    """The reference's 8-tuple (h_0, w_0, H, A, sigma_h, sigma_w, theta: numpy.float64; the last iteration's image 5x5) or its
    exception.  candidate = (pixel, field)."""
    sub = np.asarray(subimage)
    assert sub.shape[0] == 5 and sub.shape[1] == 5
    if int(n_iter) <= 0:
        check_args(1, seed)
        if len(np.nonzero(np.max(sub) == sub)[0]) == 0:
            raise_for(NO_MAXIMUM)
        raise_for(NEVER_IMPROVED)
    b = best_of(np.asarray(sub, dtype=np.float64), n_iter, seed, candidate[0], candidate[1])
    raise_for(b["status"])
    p = b["params"]
    return (np.float64(p[2]), np.float64(p[3]), np.float64(p[0]), np.float64(p[1]), np.float64(p[4]), np.float64(p[5]),
            np.float64(0.0), b["fit"].reshape(5, 5).copy())
