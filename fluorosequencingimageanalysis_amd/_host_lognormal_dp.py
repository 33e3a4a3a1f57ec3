"""Plain Python twin of the lognormal fit by exact dynamic programme (include/fsq_lognormal_dp.h): the winner of
MCsimlib._intensities_to_signal_lognormal_v8 (:5413-5466) in O(T * max_possible^2), with allow_upsteps, and without
enumerating a sequence.  The `solver='dp'` fit of `chain_records(host=True)` and the checker of fsq_lognormal_fit_dp, pinned
to a brute-force restatement of the reference's loop and to its recorded outputs by test_lognormal_dp_host.

The total is a left-to-right product of non-negative doubles, and multiplying by a non-negative double is monotone in the
other factor after rounding.  So the greatest prefix product per (frame, count) gives the greatest total (forward); whether a
prefix can still reach that total is a threshold on its product (backward, `min_prefix`); and the first sequence in the
reference's order with that total takes, at each frame, the largest allowed count whose product passes the threshold.  It
needs neither a GPU nor the library."""
import math
import struct

from . import _host_lognormal

SAT = 1 << 59                       # FSQ_LOGNORMAL_MAX_BUDGET: the count saturates here, as on the device
_MAX_BITS = 0x7fefffffffffffff      # the greatest finite double
INF = float("inf")


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _double(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def may_overflow(beta_sigma, max_frames):
    """The refusal of include/fsq_lognormal_dp.h: the greatest density exceeds 1 and its product over max_frames frames could
    reach inf (max_frames * log(peak) >= 700)."""
    c = _host_lognormal.NORM_PDF_C * beta_sigma
    peak = 1.0 / c if c > 0 else INF
    return peak > 1.0 and max_frames * math.log(peak) >= 700.0


def check_overflow(beta_sigma, max_frames):
    if may_overflow(float(beta_sigma), int(max_frames)):
        raise ValueError("beta_sigma=%r: a product of %d densities could overflow (solver='dp' needs max_frames * "
                         "log(1 / (sqrt(2 pi) * beta_sigma)) < 700)" % (beta_sigma, max_frames))


def min_prefix(s, n):
    """The least double p >= 0 with fl(p * s) >= n, for a finite s >= 0: 0.0 where n <= 0, +inf where no finite p does it.
    Non-negative doubles are ordered like their bit patterns, so n / s and its two neighbours are tried and a search over the
    bit pattern (at most 63 products) is the fallback."""
    if n <= 0.0:
        return 0.0
    if not _double(_MAX_BITS) * s >= n:
        return INF
    q = _bits(n / s) if n < INF else _MAX_BITS + 1                # (s > 0 here)
    if 1 <= q <= _MAX_BITS:
        at, below = _double(q) * s >= n, _double(q - 1) * s >= n
        if at and not below:
            return _double(q)
        if not at and q < _MAX_BITS and _double(q + 1) * s >= n:
            return _double(q + 1)
        if below and q >= 2 and not _double(q - 2) * s >= n:
            return _double(q - 1)
    lo, hi = 0, _MAX_BITS                                         # fails at lo, passes at hi
    while hi - lo > 1:
        mid = lo + ((hi - lo) >> 1)
        if _double(mid) * s >= n:
            hi = mid
        else:
            lo = mid
    return _double(hi)


def successors(u, max_possible, allow_multidrop, allow_upsteps):
    """The counts that may follow count u, ascending."""
    return range(0 if allow_multidrop else max(u - 1, 0), (max_possible if allow_upsteps else u) + 1)


def fit(intensities, categories, log_fluor_means, beta_sigma, max_possible=5, allow_multidrop=True, max_deviation=3,
        allow_upsteps=False):
    """(best_seq or None, best_score, best_intensity_scores or None, number of surviving sequences): _host_lognormal.fit's
    tuple, the count under the mode's transition rule and saturating at 2^59."""
    T = len(intensities)
    if not allow_multidrop and T == 1:
        raise ValueError("max() arg is an empty sequence")           # (:5442, for the first sequence that passes the category rule)
    check_overflow(beta_sigma, T)
    ok, S = _host_lognormal.tables(intensities, categories, log_fluor_means, beta_sigma, max_possible, max_deviation)
    return fit_tables(ok, S, max_possible, allow_multidrop, allow_upsteps)


def fit_tables(ok, S, max_possible, allow_multidrop=True, allow_upsteps=False):
    """fit's tuple of _host_lognormal.tables' (ok, score): finite scores >= 0 whose products stay finite."""
    T, V = len(ok), max_possible + 1
    succ = [successors(u, max_possible, allow_multidrop, allow_upsteps) for u in range(V)]
    # W[f][v]: the admissible completions of frames f .. T-1 that hold v at f
    W = [None] * T
    W[T - 1] = [int(ok[T - 1][v]) for v in range(V)]
    for f in range(T - 2, -1, -1):
        W[f] = [min(sum(W[f + 1][v] for v in succ[u]), SAT) if ok[f][u] else 0 for u in range(V)]
    total = min(sum(W[0]), SAT)
    if total == 0:
        return None, -1, None, 0
    # forward: the greatest prefix product per count, -1.0 where no completable prefix ends there
    P = [1.0 * S[0][v] if W[0][v] else -1.0 for v in range(V)]
    for f in range(1, T):
        best_before = [max([P[u] for u in range(V) if v in succ[u]] + [-1.0]) for v in range(V)]
        P = [best_before[v] * S[f][v] if W[f][v] and best_before[v] >= 0.0 else -1.0 for v in range(V)]
    best = max(P)
    # backward: N[f][v], the least product of a prefix ending in (f, v) that still reaches `best`
    N = [None] * T
    Q = None
    for f in range(T - 1, -1, -1):
        N[f] = [(best if f == T - 1 else min(Q[v] for v in succ[u])) if W[f][u] else INF for u in range(V)]
        Q = [min_prefix(S[f][v], N[f][v]) if W[f][v] else INF for v in range(V)]
    # the winner: at each frame the largest allowed count that can still reach `best`
    seq, p, allowed = [], 1.0, range(V)
    for f in range(T):
        v = max(v for v in allowed if p * S[f][v] >= N[f][v])
        seq.append(v)
        p = p * S[f][v]
        allowed = succ[v]
    assert p == best
    return tuple(seq), best, [S[f][v] for f, v in enumerate(seq)], total
