"""NumPy restatement of csrc/fsq_fit_f32.h (FSQ_MODE_TEXTBOOK_F32), all fits in lockstep, in float32 (the "plain fp32 reference of
the same op" the GPU tests compare the kernel with) or in float64 (the same algorithm without the rounding).  It follows the
kernel step by step: the start of kinit with x[1] = max(x[1], float32(llim1)), the pegging test, the damped normal equations with
pegged rows and columns replaced by the identity, the Cholesky solve, the step shortened at the bounds and then snapped (no clamp),
gain ratio, Nielsen's update, the exits 1 (ftol), 2 (xtol, or lam > 1e10), 4 (scaled gradient <= 1e-7 over the unpegged parameters,
after an accepted step that set no other exit - the first evaluation included) and 5 (niter >= 200 or 400 evaluations), and the
counters of the output row (niter starts at 1 and counts accepted steps; nfev counts the evaluations, the first included, plus
kfinish's one for a positive exit).
What differs from the kernel: the sums run over the pixels in the kernel's order but without fused multiply-adds; reciprocals
and square roots are NumPy's (the kernel: hardware rcp / rsq); exp, sin and cos are evaluated in double and rounded to `dtype`
(the kernel: __expf, sincosf), so that the figures the limit tests take from this file do not depend on NumPy's SIMD build.
Individual fits may therefore differ in the last bits and, the fit being chaotic for a fifth of the ROIs of a real field,
occasionally by more: tests compare distributions, and bits only where the kernel is compared with itself."""
import numpy as np
f32, f64 = np.float32, np.float64
LL = np.array([0, 0, 2, 2, .75, .75, 0], f64)
UL = np.array([np.inf, np.inf, 3, 3, 2, 2, 360], f64)
ROWS = np.repeat(np.arange(5), 5)                       # pixel k = row * 5 + col: x[3] pairs with the row, x[2] with the column
COLS = np.tile(np.arange(5), 5)
TRI_I, TRI_J = np.tril_indices(7)                       # f32_tri order: (i, j), i >= j, at i (i + 1) / 2 + j
MUTATIONS = ("J4_with_i5", "J6_second_term_dropped", "J6_doubled")       # the Jacobian mutations the limit tests must catch
EPS_SNAP = 2.0 ** -23                                   # 1.1920929e-7f


def unpack(Np):
    """packed lower triangle [n, 28] -> symmetric [n, 7, 7]"""
    N = np.empty(Np.shape[:1] + (7, 7), Np.dtype)
    N[:, TRI_I, TRI_J] = Np
    N[:, TRI_J, TRI_I] = Np
    return N


def jacobian(x, dtype=f32, mutation=None):
    """x [n, 7] -> (E [n, 25], J [n, 25, 7]) of the model H + A exp(-(u^2 + v^2) / 2) at the 25 pixels, in `dtype`"""
    T = dtype
    x = np.asarray(x).astype(T)
    ph = (x[:, 6:7] * T(0.017453292519943295)).astype(f64)
    cs, sn = np.cos(ph).astype(T), np.sin(ph).astype(T)
    A = x[:, 3:4] - ROWS.astype(T)[None]
    B = x[:, 2:3] - COLS.astype(T)[None]
    nu = A * cs - B * sn
    nv = A * sn + B * cs
    i4, i5 = T(1) / x[:, 4:5], T(1) / x[:, 5:6]
    u, v = nu * i4, nv * i5
    E = np.exp((T(-0.5) * (u * u + v * v)).astype(f64)).astype(T)
    aE = x[:, 1:2] * E
    J = np.empty(x.shape[:1] + (25, 7), T)
    J[:, :, 0] = 1
    J[:, :, 1] = E
    J[:, :, 2] = aE * (u * sn * i4 - v * cs * i5)
    J[:, :, 3] = -aE * (u * cs * i4 + v * sn * i5)
    J[:, :, 4] = aE * u * u * (i5 if mutation == "J4_with_i5" else i4)
    J[:, :, 5] = aE * v * v * i5
    second = T(0) if mutation == "J6_second_term_dropped" else v * nu * i5
    J[:, :, 6] = aE * (u * nv * i4 - second) * T(0.017453292519943295) * T(2 if mutation == "J6_doubled" else 1)
    assert mutation is None or mutation in MUTATIONS
    return E, J


def evaluate(x, d, dtype=f32, mutation=None):
    """x [n, 7], d [n, 25] -> chi2 [n], N [n, 28] (J^T J, packed lower triangle in f32_tri order), g [n, 7] (J^T r), in `dtype`;
    r = model - data, the sums over the pixels in the kernel's order"""
    T = dtype
    x = np.asarray(x).astype(T)
    d = np.asarray(d).reshape(len(x), 25).astype(T)
    E, J = jacobian(x, T, mutation)
    r = (x[:, 0:1] - d) + x[:, 1:2] * E
    chi2, N, g = np.zeros(len(x), T), np.zeros((len(x), 28), T), np.zeros((len(x), 7), T)
    for k in range(25):
        chi2 += r[:, k] * r[:, k]
        g += J[:, k, :] * r[:, k:k + 1]
        N += J[:, k, TRI_I] * J[:, k, TRI_J]
    return chi2, N, g


def start(rois, dtype=f32):
    """kinit's clipped start and the bounds as the kernel sees them: (d [n, 25], x [n, 7], ll [n, 7], ul [7]) in `dtype`; the lower
    bound of the amplitude is float32((max - mean) / 3) whatever `dtype` is."""
    T = dtype
    d64 = np.asarray(rois).reshape(-1, 25).astype(f64)
    n = len(d64)
    mx, mean, med = d64.max(1), d64.sum(1) / 25.0, np.median(d64, 1)
    ll = np.tile(LL, (n, 1))
    ll[:, 1] = ((mx - mean) / 3.0).astype(f32)
    x = np.stack([med, mx, np.full(n, 2.5), np.full(n, 2.5), np.ones(n), np.ones(n), np.zeros(n)], 1)
    x = np.maximum(np.minimum(x, UL[None]), ll)
    return d64.astype(T), x.astype(T), ll.astype(T), UL.astype(T)


def pegged(x, g, ll, ul):
    return ((x <= ll) & (g > 0)) | ((x >= ul[None]) & (g < 0))


def fit(rois, maxtrips=400, ftol=3e-7, xtol=1e-6, lam0=1e-2, gtol=1e-7, maxiter=200, dtype=f32, mutation=None):
    """-> x [n, 7] float64, status, niter, nfev [n] int32 as the output row carries them"""
    T = dtype
    d, x, ll, ul = start(rois, T)
    n = len(d)
    ftol, xtol, gtol = T(ftol), T(xtol), T(gtol)
    chi2, N, g = np.zeros(n, T), np.zeros((n, 28), T), np.zeros((n, 7), T)
    D = np.zeros((n, 7), T)
    lam, nu_ = np.full(n, lam0, T), np.full(n, 2, T)
    status, niter, nfev = np.zeros(n, np.int32), np.ones(n, np.int32), np.zeros(n, np.int32)
    first = True
    while True:
        ix = np.flatnonzero(status == 0)
        if not len(ix):
            break
        m = len(ix)
        xa, ga, Na, Da, lla, lama = x[ix], g[ix], N[ix], D[ix], ll[ix], lam[ix]
        p, ok = np.zeros((m, 7), T), np.ones(m, bool)
        if not first:
            peg = pegged(xa, ga, lla, ul)
            a = unpack(Na)
            a[:, range(7), range(7)] += (lama[:, None] * Da) * Da
            rhs = -ga
            dead = peg[:, :, None] | peg[:, None, :]
            a = np.where(dead, np.eye(7, dtype=T)[None], a)
            rhs = np.where(peg, T(0), rhs)
            Lm = np.zeros_like(a)
            for j in range(7):
                s = a[:, j, j] - (Lm[:, j, :j] * Lm[:, j, :j]).sum(1, dtype=T)
                ok &= s > 0
                Lm[:, j, j] = np.sqrt(np.where(s > 0, s, T(1)))
                for i in range(j + 1, 7):
                    Lm[:, i, j] = (a[:, i, j] - (Lm[:, i, :j] * Lm[:, j, :j]).sum(1, dtype=T)) / Lm[:, j, j]
            y = np.zeros((m, 7), T)
            for i in range(7):
                y[:, i] = (rhs[:, i] - (Lm[:, i, :i] * y[:, :i]).sum(1, dtype=T)) / Lm[:, i, i]
            for i in range(6, -1, -1):
                p[:, i] = (y[:, i] - (Lm[:, i + 1:, i] * p[:, i + 1:]).sum(1, dtype=T)) / Lm[:, i, i]
        # the whole step shortened at the bounds (mpfit.py:1192-1216), then snapped: t <= lo (1 + 2^-23) -> lo, t >= hi (1 - 2^-23) -> hi
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            tl = np.where((p < 0) & (xa + p < lla), (lla - xa) / p, np.inf)
            tu = np.where((p > 0) & (xa + p > ul[None]), (ul[None] - xa) / p, np.inf)
        alpha = np.minimum(T(1), np.minimum(tl.min(1), tu.min(1))).astype(T)
        ps = alpha[:, None] * p
        xt = xa + ps
        xt = np.where(xt <= lla * (T(1) + T(EPS_SNAP)), lla, xt)
        with np.errstate(invalid='ignore'):
            xt = np.where(xt >= ul[None] * (T(1) - T(EPS_SNAP)), ul[None], xt).astype(T)
        chi2t, Nt, gt = evaluate(xt, d[ix], T, mutation)
        nfev[ix] += 1
        gp = (ga * ps).sum(1, dtype=T)
        pNp = ((unpack(Na) * ps[:, None, :]).sum(2, dtype=T) * ps).sum(1, dtype=T)
        pred = -(T(2) * gp + pNp)
        c2 = chi2[ix]
        with np.errstate(divide='ignore', invalid='ignore'):
            rho = np.where(pred > 0, (c2 - chi2t) / pred, T(-1)).astype(T)
            finite_t = np.isfinite(chi2t) & (chi2t < 3.0e38)
            acc = finite_t if first else (ok & finite_t & (rho > T(1e-4)))
            st = np.zeros(m, np.int32)
            if not first:
                actred = np.where(c2 > 0, (c2 - chi2t) / c2, T(0))
                prered = np.where(c2 > 0, pred / c2, T(0))
                dxn, xn = ((Da * ps) ** 2).sum(1, dtype=T), ((Da * xt) ** 2).sum(1, dtype=T)
                by_f = acc & (np.abs(actred) <= ftol) & (prered <= ftol)
                st[by_f] = 1
                st[acc & ~by_f & (dxn <= xtol * xtol * xn)] = 2
                f = T(2) * rho - T(1)
                lama = np.where(acc, lama * np.maximum(T(1) / T(3), T(1) - f * f * f), lama * nu_[ix]).astype(T)
                nu_[ix] = np.where(acc, T(2), nu_[ix] * T(2))
                niter[ix] += acc
                st[~acc & (lama > T(1e10))] = 2
        xa, c2, Na, ga = np.where(acc[:, None], xt, xa), np.where(acc, chi2t, c2), np.where(acc[:, None], Nt, Na), np.where(acc[:, None], gt, ga)
        Dn = np.maximum(Da, np.sqrt(Na[:, TRI_I == TRI_J]))
        Dn[Dn == 0] = 1
        Da = np.where(acc[:, None], Dn, Da)
        st[acc & (c2 == 0)] = 1
        with np.errstate(divide='ignore', invalid='ignore'):
            gn = np.where(pegged(xa, ga, lla, ul), T(0), np.abs(ga) / (Da * np.sqrt(c2)[:, None])).max(1)
        st[acc & (st == 0) & (gn <= gtol)] = 4
        st[(st == 0) & ((niter[ix] >= maxiter) | (nfev[ix] >= maxtrips))] = 5
        if first:
            st[~acc] = -16
        x[ix], chi2[ix], N[ix], g[ix], D[ix], lam[ix], status[ix] = xa, c2, Na, ga, Da, lama, st
        first = False
    return x.astype(f64), status, niter, nfev + (status > 0)
