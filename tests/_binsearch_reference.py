"""The arithmetic contract of include/fsq_binsearch.h restated in Python: what MCsimlib.optimal_bin_size's numpy calls
(np.linspace, np.histogram with explicit edges, np.mean, np.var) compute for one bin count, one IEEE operation at a time.
Python floats are the float64 of the contract; the only numpy calls are element-wise on float64 arrays and np.searchsorted.

The switches restate the contract wrongly on purpose, for the non-vacuity counts of the fixture: fused=True computes an
edge as one fma (exactly, through fractions), inner_le=True counts x <= edge at the inner edges, chunk=None sums the squared
deviations as one pairwise sum instead of np.add.reduce's chunks of 8192, product=True divides by step * step instead of
libm's pow(step, 2.0) (what `bin_size**2` on a numpy float64 scalar calls; glibc's pow is within an ulp of the rounded product,
not always equal to it)."""
import math
from fractions import Fraction

import numpy as np

CHUNK = 8192
MAX_BINS = 10000


def edges(lo, hi, nb, fused=False):
    """(step, the nb + 1 edges as a float64 array)"""
    lo, hi = float(lo), float(hi)
    step = (hi - lo) / float(nb)
    if fused:
        e = np.array([float(Fraction(j) * Fraction(step) + Fraction(lo)) for j in range(nb)])
    else:
        e = np.arange(nb, dtype=np.float64) * step + lo             # two roundings per edge
    return step, np.append(e, hi)


def counts(sorted_values, lo, hi, nb, fused=False, inner_le=False):
    """hist of nb bins over ascending float64 values (lo their first, hi their last), as an int64 array."""
    a = np.asarray(sorted_values, dtype=np.float64)
    _, e = edges(lo, hi, nb, fused)
    rank = np.append(np.searchsorted(a, e[:-1], 'right' if inner_le else 'left'), len(a)).astype(np.int64)
    if inner_le:
        rank[0] = 0
    return rank[1:] - rank[:-1]


def _leaves(off, n, out):
    if n <= 128:
        out.append((off, n))
    else:
        n2 = n // 2
        n2 -= n2 % 8
        _leaves(off, n2, out)
        _leaves(off + n2, n - n2, out)


_COL = np.arange(128)


def _leaf_sums(x, leaves):
    """numpy's leaf for every (off, n <= 128) of `leaves` at once: eight accumulators over the groups of eight, their
    balanced sum, then the n % 8 elements left over one by one.  A shorter leaf is padded with +0.0, which changes nothing
    (no element here is -0.0: they are squares)."""
    offs, lens = np.array([o for o, _ in leaves]), np.array([n for _, n in leaves])
    full = lens - lens % 8
    idx = offs[:, None] + _COL[None, :]
    A = np.where(_COL[None, :] < full[:, None], x[np.minimum(idx, len(x) - 1)], 0.0)
    r = A[:, :8]
    for i in range(8, int(full.max()), 8):
        r = r + A[:, i:i + 8]
    s = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
    tpos = full[:, None] + _COL[None, :7]
    T = np.where(tpos < lens[:, None], x[np.minimum(offs[:, None] + tpos, len(x) - 1)], 0.0)
    for t in range(7):
        s = s + T[:, t]
    return dict(zip(offs.tolist(), s.tolist()))


def _combine(off, n, leaf):
    if n <= 128:
        return leaf[off]
    n2 = n // 2
    n2 -= n2 % 8
    return _combine(off, n2, leaf) + _combine(off + n2, n - n2, leaf)


def pairwise_sum(x):
    """numpy's pairwise sum of a float64 array (128-element leaves, n2 -= n2 % 8)."""
    leaves = []
    _leaves(0, len(x), leaves)
    return _combine(0, len(x), _leaf_sums(x, leaves))


def add_reduce(x, chunk=CHUNK):
    """np.add.reduce of a float64 array: from the identity, chunk by chunk."""
    total = 0.0
    step = len(x) if chunk is None else chunk
    for c in range(0, len(x), step):
        total = total + pairwise_sum(x[c:c + step])
    return total


def cost_of(hist, n, lo, hi, nb, chunk=CHUNK, product=False):
    step = (float(hi) - float(lo)) / float(nb)
    mean = float(n) / float(nb)
    d = np.asarray(hist, dtype=np.float64) - mean
    var = add_reduce(d * d, chunk) / float(nb)
    return (2.0 * mean - var) / (step * step if product else math.pow(step, 2.0))


def cost(sorted_values, lo, hi, nb, fused=False, inner_le=False, chunk=CHUNK, product=False):
    return cost_of(counts(sorted_values, lo, hi, nb, fused, inner_le), len(sorted_values), lo, hi, nb, chunk, product)


def slot_tree_sum(x):
    """The same chunk sum the way the kernel lays it out (csrc/lognormal/fsq_binsearch.hip): 128 slots of a depth-7 tree, each
    walking numpy's splits along its own bits, then seven levels of sibling additions.  For len(x) <= 8192."""
    D = 7
    val, internal = [0.0] * (1 << D), [0] * (1 << D)
    leaves = []
    where = {}
    for slot in range(1 << D):
        off, n, d = 0, len(x), 0
        while d < D and n > 128:
            internal[slot] |= 1 << d
            n2 = n // 2
            n2 -= n2 % 8
            if (slot >> (D - 1 - d)) & 1:
                off, n = off + n2, n - n2
            else:
                n = n2
            d += 1
        if n > 0 and slot & ((1 << (D - d)) - 1) == 0:
            leaves.append((off, n))
            where[slot] = off
    sums = _leaf_sums(x, leaves)
    for slot, off in where.items():
        val[slot] = sums[off]
    for lvl in range(D - 1, -1, -1):
        for slot in range(1 << D):
            if (internal[slot] >> lvl) & 1 and slot & ((1 << (D - lvl)) - 1) == 0:
                val[slot] = val[slot] + val[slot + (1 << (D - 1 - lvl))]
    return val[0]
