"""NumPy restatement of chi_squared_step_fitter, filter_upsteps, filter_small_steps and stepfit_r_squared, written from the
specification in DESIGN.md section 4.12 for tests on machines without the reference.

Every number follows the reference's arithmetic, so results are compared bit for bit: heights are np.mean of a slice
(numpy's pairwise sum / n), a residual sum is the left-to-right sum (np.add.accumulate) of glibc's pow(lum - height, 2.0),
plateau sums are added in frame order.  A candidate split's value depends on (start, stop, split) only; the values of a
plateau are computed together and cached per trace."""
import math

import numpy as np

_rng = np.random.default_rng(12345)
_probe = np.concatenate([_rng.normal(0.0, 3000.0, 20000), _rng.normal(0.0, 1e-3, 2000), [0.0, -0.0, 1e-200, -1e200, 0.5, -2.5]])


def _scalar_pow2(v):
    try:
        return math.pow(v, 2.0)
    except OverflowError:                                          # (math.pow raises where libm's pow returns inf)
        return math.inf


_exact = np.array([_scalar_pow2(float(v)) for v in _probe])
_py_pow2 = np.frompyfunc(_scalar_pow2, 1, 1)
# np.power(x, 2.0) multiplies; np.float_power with a scalar exponent goes through libm's pow where that was checked.  The
# check decides: without it every element goes through math.pow (slow, exact).
with np.errstate(all="ignore"):
    VECTOR_POW = bool(np.array_equal(np.float_power(_probe, 2.0).view(np.uint64), _exact.view(np.uint64)))


def pow2(x):
    """Elementwise glibc pow(x, 2.0) of a float64 array."""
    x = np.asarray(x, dtype=np.float64)
    if VECTOR_POW:
        return np.float_power(x, 2.0)
    return _py_pow2(x).astype(np.float64).reshape(x.shape)


def residual(arr, a, b, h):
    """_plateau_squared_residuals: sum from the int 0, left to right, of (lum - h) ** 2 over frames a .. b."""
    return float(np.add.accumulate(pow2(arr[a:b + 1] - h))[-1])


class _Trace(object):
    def __init__(self, lum, min_mag):
        self.arr = np.array([float(v) for v in lum], dtype=np.float64)
        if np.isnan(self.arr).any():
            raise ValueError("NaN luminosity")
        self.n = len(self.arr)
        self.min_mag = min_mag
        r2 = _scalar_pow2(float(np.amax(self.arr) - np.amin(self.arr)))
        self.B, self.B2 = self.n * r2, (2 * self.n) * r2           # the bounds of _best_split (:241) and _split_plateau (:159)
        self.cache = {}

    def mean(self, a, b):
        return np.mean(self.arr[a:b + 1])

    def values(self, a, b):
        """Value of every split u = a .. b - 1 of plateau [a, b]; -1 where the step is below min_step_magnitude."""
        key = (a, b)
        v = self.cache.get(key)
        if v is None:
            seg = self.arr[a:b + 1]
            m = len(seg)
            hl = np.array([np.mean(seg[:k + 1]) for k in range(m - 1)])
            hr = np.array([np.mean(seg[k + 1:]) for k in range(m - 1)])
            left = np.add.accumulate(np.tril(pow2(seg[None, :] - hl[:, None])), axis=1)[np.arange(m - 1), np.arange(m - 1)]
            right = np.add.accumulate(np.triu(pow2(seg[None, :] - hr[:, None]), 1), axis=1)[:, -1]
            v = left + right
            v[np.abs(hl - hr) < self.min_mag] = -1.0
            self.cache[key] = v
        return v

    def scan(self, a, b, allowed):
        """_split_plateau: the allowed split of the smallest value not above 2 B; the later one on a tie."""
        if b <= a:
            return None
        v = self.values(a, b)
        ok = allowed & (v >= 0.0) & (v <= self.B2)
        if not ok.any():
            return None
        best = v[ok].min()
        u = int(np.flatnonzero(ok & (v == best))[-1])
        return a + u, float(best)


def _best_split(T, plateaus, L, bestfit):
    """_best_split: the first plateau whose best split has the smallest value below B is split in two."""
    counter = bestfit is not None
    if counter:
        owner = np.zeros(T.n, dtype=np.int64)                  # index of the best-fit plateau that holds each frame
        for i, (a, b, _, _) in enumerate(bestfit):
            owner[a:b + 1] = i
        taken = np.zeros(len(bestfit), dtype=bool)             # it already holds a counter-fit start
        for a, _, _, _ in plateaus:
            taken[owner[a]] = True
    pick, pick_v, pick_u = None, T.B, None
    for i, (a, b, _, _) in enumerate(plateaus):
        u = np.arange(a, b)
        if counter:
            allowed = (owner[u] == owner[u + 1]) & ~taken[owner[u]] if b > a else np.zeros(0, bool)
        else:
            allowed = (u - a >= L) & (b - u >= L)
        r = T.scan(a, b, allowed)
        if r is not None and r[1] < pick_v:
            pick, pick_u, pick_v = i, r[0], r[1]
    if pick is None:
        return None
    a, b = plateaus[pick][0], plateaus[pick][1]
    hl, hr = T.mean(a, pick_u), T.mean(pick_u + 1, b)
    return (plateaus[:pick] + [(a, pick_u, hl, residual(T.arr, a, pick_u, hl)), (pick_u + 1, b, hr, residual(T.arr, pick_u + 1, b, hr))] +
            plateaus[pick + 1:])


def _res_sum(plateaus):
    r = 0.0
    for p in plateaus:
        r = r + p[3]
    return r


def chi_squared(lum, num_steps_multiplier=1, num_steps=None, min_step_length=2, min_step_magnitude=0.0,
                ignore_counterfits=False, records=None):
    """chi_squared_step_fitter.  Returns (fit, records): the list of (start, stop, height) and, for every plateau count
    tried, (best-fit residual sum, counter-fit residual sum, counter-fit plateau count, S).  A caller's `records` list is
    appended to, so that it holds the fits tried when the reference's ValueError is raised."""
    n = len(lum)
    if not 0 < num_steps_multiplier <= 1:
        raise ValueError("num_steps_multiplier has an invalid value of " + str(num_steps_multiplier))
    if num_steps is not None and not 0 < num_steps < n:
        raise ValueError("num_steps has an invalid value of " + str(num_steps) + " vs len(luminosity_sequence) = " + str(n))
    if num_steps is None:
        num_steps = min(int(np.ceil(num_steps_multiplier * n)), n - 2)
    if num_steps < 0:
        raise IndexError("list index out of range")                # (sorted([])[0] in the reference)
    T = _Trace(lum, min_step_magnitude)
    L = max(int(min_step_length), 0)
    h = T.mean(0, n - 1)
    first = [(0, n - 1, h, residual(T.arr, 0, n - 1, h))]
    fits, records = [], ([] if records is None else records)
    best = None
    for p in range(1, num_steps + 2):
        if best is None:
            best = first
        else:
            grown = _best_split(T, best, L, None)
            if grown is None:
                break
            best = grown
        if p + 1 > n:
            raise ValueError("num_plateaus = " + str(p + 1) + " is greater than len(luminosities) = " + str(n))
        best_res = _res_sum(best)
        counter = first
        while len(counter) < p + 1:
            grown = _best_split(T, counter, 0, best)
            if grown is None:
                break
            counter = grown
        counter_res = _res_sum(counter)
        S = counter_res / best_res if best_res != 0 else 1e10
        fits.append(best)
        records.append((best_res, counter_res, len(counter), S))
    if ignore_counterfits:
        k = len(fits) - 1
    else:
        k = 0
        for i, r in enumerate(records):
            if r[3] > records[k][3]:
                k = i
    return [(a, b, hh) for a, b, hh, _ in fits[k]], records


def _check_plateaus(lum, plateaus):
    ok = len(plateaus) >= 1 and plateaus[0][0] >= 0 and plateaus[-1][1] < len(lum)
    ok = ok and all(a <= b for a, b, _ in plateaus)
    ok = ok and all(plateaus[i][1] + 1 == plateaus[i + 1][0] for i in range(len(plateaus) - 1))
    if not ok:
        raise ValueError("Merged plateaus must be consecutive.")


def _merge_pass(arr, plateaus, test):
    out, r, merged = [], 0, False
    while r < len(plateaus):
        if r + 1 < len(plateaus) and test(plateaus[r], plateaus[r + 1]):
            a, b = plateaus[r][0], plateaus[r + 1][1]
            out.append((a, b, np.mean(arr[a:b + 1])))
            merged = True
            r += 2
        else:
            out.append(plateaus[r])
            r += 1
    return out, merged


def _merge_filter(lum, plateaus, test):
    arr = np.array([float(v) for v in lum], dtype=np.float64)
    plateaus = [(int(a), int(b), h) for a, b, h in plateaus]
    if len(plateaus) < 2:
        return plateaus
    _check_plateaus(arr, plateaus)
    for _ in range(len(plateaus) - 1):
        plateaus, merged = _merge_pass(arr, plateaus, lambda x, y: test(arr, x, y))
        if not merged:
            break
    return plateaus


def filter_upsteps(lum, plateaus):
    return _merge_filter(lum, plateaus, lambda arr, x, y: y[2] > x[2])


def filter_small_steps(lum, plateaus, min_magnitude=None, min_noise_ratio=None):
    if min_magnitude is not None and min_magnitude < 0:
        raise ValueError("min_step_magnitude < 0 makes no sense.")
    if min_noise_ratio is not None and min_noise_ratio < 0:
        raise ValueError("min_step_noise_ratio < 0 makes no sense.")

    def test(arr, x, y):
        step = abs(x[2] - y[2])
        merge = False
        if min_noise_ratio is not None:
            na, nb = math.sqrt(residual(arr, x[0], x[1], x[2])), math.sqrt(residual(arr, y[0], y[1], y[2]))
            merge = step < (nb if nb > na else na) * min_noise_ratio
        if min_magnitude is not None and step < min_magnitude:
            merge = True
        return merge
    return _merge_filter(lum, plateaus, test)


def r_squared(lum, plateaus):
    arr = np.array([float(v) for v in lum], dtype=np.float64)
    _check_plateaus(arr, plateaus)
    a, b = plateaus[0][0], plateaus[-1][1]
    ss_res = 0.0
    for s, o, h in plateaus:
        ss_res = ss_res + residual(arr, s, o, h)
    with np.errstate(all="ignore"):
        return float(np.float64(1.0) - np.float64(ss_res) / np.float64(residual(arr, a, b, np.mean(arr[a:b + 1]))))
