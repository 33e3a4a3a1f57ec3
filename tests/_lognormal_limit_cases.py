"""Inputs and expected values of the lognormal family's limit tests (tests/test_lognormal_limits_host.py proves that they
reach the paths named there, tests/test_gpu_lognormal_limits.py feeds them to the device).  Everything is seeded and built
once.  Expected values come from the plain Python twins (_host_lognormal, _host_lognormal_dp, _host_lognormal_chain) and from
the numpy restatement of the remainder correction (tests/_remainder_reference.py): none of them shares code with a kernel."""
import functools
import math

import numpy as np

import _remainder_reference as RR
from fluorosequencingimageanalysis_amd import _host_lognormal as R
from fluorosequencingimageanalysis_amd import _host_lognormal_dp as D
from _lognormal_cases import golden, means_for, random_batch, restated_records
from _lognormal_dp_cases import rising_batch, twin_records

FOUND, NONE, OVER_BUDGET, INVALID = 0, 1, 2, 3
MAX_BLOCKS = 16384                  # kln_fit's and kln_fit_dp's grid
PERIOD = 257                        # no divisor of MAX_BLOCKS: a block meets another base track on every trip
N_STRIDE = 2 * MAX_BLOCKS + 77
LOG_BLOCKS, LOG_THREADS = 4096, 256                                # kln_log's grid
MEANS, SIGMA, M, F_STRIDE = means_for(10000.0, 5), 0.2, 5, 13
LAUNCHES = (("enumerate", False), ("dp", False), ("dp", True))      # (solver, allow_upsteps)
SMALL_BUDGET = 12
FIT_KEYS = ("status", "best_seq", "best_score", "frame_score", "n_surviving")


def words_of(C):
    return np.array([sum(1 << f for f, c in enumerate(cat) if c) for cat in C], dtype=np.uint64)


def rows_of(I, F=None):
    F = F or max(len(v) for v in I)
    rows = np.zeros((len(I), F))
    for i, v in enumerate(I):
        rows[i, :len(v)] = v
    return rows


def twin_fit(I, C, means, sigma, m, multi, dev, solver, upsteps, budget=1 << 22, F=None):
    """lognormal_device's dict by the twin of `solver`, rows padded to F frames."""
    with np.errstate(all="ignore"):
        if solver == "enumerate":
            e = restated_records(R, I, C, means, sigma, m, multi, dev, budget)
        else:
            e = twin_records(D, I, C, means, sigma, m, multi, dev, upsteps)
    have = e["best_seq"].shape[1]
    F = F or have
    for k in ("best_seq", "frame_score"):
        e[k] = np.concatenate([e[k], np.zeros((len(I), F - have), e[k].dtype)], axis=1)
    e["best_score"] = e["best_score"].astype(np.float64)
    return {k: e[k] for k in FIT_KEYS}


# ---- A: the block stride ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stride_base():
    """(rows [257, 13], words, declared lengths, I, C, valid): 236 ragged tracks of 1 .. 13 frames and 21 rows whose declared
    length is 0, -1 or 14, every twelfth row."""
    I0, C0 = random_batch(2571, 120)
    I1, C1 = rising_batch(2572, 116)
    I, C = I0 + I1, C0 + C1
    order = np.random.default_rng(2573).permutation(len(I))
    I, C = [I[i] for i in order], [C[i] for i in order]
    valid = np.ones(PERIOD, bool)
    valid[5::12] = False
    assert int(valid.sum()) == len(I) and max(len(v) for v in I) == F_STRIDE
    rows, words, lens = np.zeros((PERIOD, F_STRIDE)), np.zeros(PERIOD, np.uint64), np.zeros(PERIOD, np.int32)
    where = np.flatnonzero(valid)
    rows[where], words[where], lens[where] = rows_of(I, F_STRIDE), words_of(C), [len(v) for v in I]
    for j, t in enumerate(np.flatnonzero(~valid)):                 # a real track's row under a length that cannot be
        rows[t], words[t], lens[t] = rows[where[3 * j]], words[where[3 * j]], (0, -1, F_STRIDE + 1)[j % 3]
    return rows, words, lens, I, C, valid


@functools.lru_cache(maxsize=None)
def stride_expected(solver, upsteps, budget=1 << 22):
    """The twin's arrays for the 257 base rows: status 3, score -1 and zeros for the rows of an invalid length."""
    rows, words, lens, I, C, valid = stride_base()
    e = twin_fit(I, C, MEANS, SIGMA, M, True, 3, solver, upsteps, budget, F_STRIDE)
    out = {"status": np.full(PERIOD, INVALID, np.int32), "best_seq": np.zeros((PERIOD, F_STRIDE), np.uint8),
           "best_score": np.full(PERIOD, -1.0), "frame_score": np.zeros((PERIOD, F_STRIDE)), "n_surviving": np.zeros(PERIOD, np.int64)}
    for k in FIT_KEYS:
        out[k][valid] = e[k]
    return out


def stride_index(n=N_STRIDE):
    return np.arange(n) % PERIOD


def log_stride():
    """(x, log x) of the recorded values tiled past kln_log's grid: 4096 * 256 + 3 values."""
    g = golden()
    idx = np.arange(LOG_BLOCKS * LOG_THREADS + 3) % len(g["c_x"])
    return g["c_x"][idx], g["c_log"][idx]


# ---- B: the budget and the lanes' shares ------------------------------------------------------------------------------------
BUDGET_TRACK = ([20000.0] * 8, (True,) * 8, 1e9, 495)               # all ON at a wide deviation: C(12, 4) sequences
SURVIVOR_TARGETS = (1, 2, 63, 64, 65, 127, 128, 129)


@functools.lru_cache(maxsize=None)
def survivor_tracks():
    """{survivors: (intensities, category, max_deviation)} for every target the seeded search finds: ON-prefix and all-ON
    tracks of 2 .. 12 frames at a narrow deviation, counted by the twin's count_surviving (with multi-drop)."""
    rng = np.random.default_rng(6465)
    found = {}
    for _ in range(60000):
        T = int(rng.integers(2, 13))
        k = T if rng.random() < 0.6 else int(rng.integers(1, T + 1))
        dev = float(rng.choice([0.75, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0]))
        noise = float(rng.choice([0.1, 0.2, 0.3]))
        seq = sorted(rng.integers(1, M + 1, k).tolist(), reverse=True)
        I = [float(int(math.exp(rng.normal(MEANS[s - 1], noise)))) for s in seq] + [float(int(rng.normal(40.0, 300.0))) for _ in range(T - k)]
        C = (True,) * k + (False,) * (T - k)
        ok, _ = R.tables(I, C, MEANS, SIGMA, M, dev)
        n = R.count_surviving(ok, M, True)
        if n in SURVIVOR_TARGETS and n not in found:
            found[n] = (I, C, dev)
            if len(found) == len(SURVIVOR_TARGETS):
                break
    return found


# ---- C: values the record routes refuse -------------------------------------------------------------------------------------
VALUES = (0.0, -0.0, -5.0, float("nan"), float("inf"), float("-inf"), 5e-324, 1.7e308)
DEVIATIONS = (3, 1e9, float("inf"))


@functools.lru_cache(maxsize=None)
def value_tracks():
    """(I, C, meta): tracks of 3 .. 6 frames with an ON prefix, each of VALUES once at an ON frame and once at an OFF frame of
    every length; meta holds (value index, True at an ON frame, frame)."""
    rng = np.random.default_rng(308)
    I, C, meta = [], [], []
    for vi, val in enumerate(VALUES):
        for T in (3, 4, 5, 6):
            k = 1 + (vi + T) % (T - 1)                              # ON frames: 1 .. T - 1
            seq = sorted(rng.integers(1, M + 1, k).tolist(), reverse=True)
            base = [float(int(math.exp(rng.normal(MEANS[s - 1], 0.1)))) for s in seq] + [float(int(rng.normal(40.0, 300.0))) for _ in range(T - k)]
            for on in (True, False):
                f = int(rng.integers(0, k)) if on else int(rng.integers(k, T))
                v = list(base)
                v[f] = val
                I.append(v), C.append((True,) * k + (False,) * (T - k)), meta.append((vi, on, f))
    return I, C, meta


@functools.lru_cache(maxsize=None)
def value_expected(dev, solver, upsteps):
    I, C, _ = value_tracks()
    return twin_fit(I, C, MEANS, SIGMA, M, True, dev, solver, upsteps, F=6)


# ---- D: the remainder correction --------------------------------------------------------------------------------------------
def all_on(F):
    return (1 << F) - 1


def _remainder_table(rng, sizes, remainders, F):
    """Tracks of segments of `sizes` tracks with `remainders` remainders each at random places: positive integer intensities."""
    rows, cats = [], []
    for n, k in zip(sizes, remainders):
        for remainder in rng.permutation([True] * k + [False] * (n - k)):
            rows.append(np.round(float(rng.integers(2000, 20000)) * np.exp(rng.normal(0.0, 0.2, F))))
            cats.append(all_on(F) if remainder else int(rng.integers(0, 1 << min(F, 62))) & ~(1 << int(rng.integers(0, F))))
    seg_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return np.array(rows, dtype=np.float64).reshape(len(rows), F), np.array(cats, dtype=np.uint64), seg_off


def nan_specials(F):
    """(name, {frame: value}) of the remainder tracks that hold what the record routes refuse."""
    nan, inf = float("nan"), float("inf")
    out = [("nan first", {0: nan}), ("nan middle", {F // 2: nan}), ("nan last", {F - 1: nan})]
    if F == 5:
        out.append(("two nans", {1: nan, 3: nan}))
    return out + [("inf", {F // 2: inf}), ("-inf, inf", {0: -inf, F - 1: inf})]


NAN_FRAMES = (3, 4, 5, 64)
SMALL_R, LARGE_R = 9, 600           # remainders per segment: ranked in LDS (<= 512), radix select


@functools.lru_cache(maxsize=None)
def nan_table(F):
    """(rows, cats, seg_off, meta): per special track one segment of 9 and one of 600 remainders that holds it (at a random
    place among the remainders), and a clean segment of each size before, between and after them.  meta: (segment, name,
    {frame: value}), a clean segment with name None."""
    rng = np.random.default_rng(900 + F)
    specials = nan_specials(F)
    plan = [None] + [p for sp in specials for p in (sp, None)]
    sizes, remainders, meta = [], [], []
    for p in plan:
        for R_ in (SMALL_R, LARGE_R):
            sizes.append(R_ + (3 if R_ == SMALL_R else 40)), remainders.append(R_), meta.append((len(meta), None if p is None else p[0], {} if p is None else p[1]))
    rows, cats, seg_off = _remainder_table(rng, sizes, remainders, F)
    for s, name, frames in meta:
        if name is None:
            continue
        a, b = int(seg_off[s]), int(seg_off[s + 1])
        rem = a + np.flatnonzero(cats[a:b] == np.uint64(all_on(F)))
        t = int(rem[int(rng.integers(0, len(rem)))])
        for f, v in frames.items():
            rows[t, f] = v
    return rows, cats, seg_off, tuple(meta)


@functools.lru_cache(maxsize=None)
def nan_expected(F, mode):
    rows, cats, seg_off, _ = nan_table(F)
    return RR.adjust_arrays(rows, cats, seg_off, mode, 5)


MALFORMED_OFFSETS = ([0, 30, 80, 100], [100, 80, 30, 0], [0, 30, 500, 100], [0, -5, 80, 100], [0, 80, 30, 100], [1 << 40, 3, 3, 3],
                     [0, 30, 80, 1 << 33], [0, 0, 0, 0])           # (the lists of the chain's malformed-offsets test)


@functools.lru_cache(maxsize=None)
def malformed_table():
    """100 tracks of 5 frames whose well-formed offsets are [0, 30, 80, 100]: 10, 30 and 7 remainders."""
    return _remainder_table(np.random.default_rng(41), [30, 50, 20], [10, 30, 7], 5)


def well_formed(seg_off, s, n):
    a, b = int(seg_off[s]), int(seg_off[s + 1])
    return 0 <= a <= b <= n


MANY_SEGMENTS = 66000


@functools.lru_cache(maxsize=None)
def many_segments(F):
    """(rows, cats, seg_off, status): 66 000 segments of 0 .. 3 tracks of F frames, a third of them empty; about half of the
    tracks are remainders at F = 2 and a tenth above, the others hold any category word; status 0 or 1 per track (the chain's first fit)."""
    rng = np.random.default_rng(66000 + F)
    sizes = rng.choice([0, 1, 2, 3], MANY_SEGMENTS, p=[1.0 / 3, 2.0 / 9, 2.0 / 9, 2.0 / 9])
    n = int(sizes.sum())
    rows = np.round(rng.integers(2000, 20000, n)[:, None] * np.exp(rng.normal(0.0, 0.2, (n, F))))
    cats = np.where(rng.random(n) < (0.5 if F == 2 else 0.1), all_on(F), rng.integers(0, 1 << F, n)).astype(np.uint64)
    seg_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return rows, cats, seg_off, (rng.random(n) < 0.3).astype(np.int32)


def _small_medians(pad, count):
    """np.median over the first count[s] of pad[s, :, f] for count 0 .. 3: one sort per count (NaN for none)."""
    S, _, F = pad.shape
    out = np.full((S, F), np.nan)
    for c in (1, 2, 3):
        sel = count == c
        a = np.sort(pad[sel, :c], axis=1)
        out[sel] = a[:, c // 2] + 0.0 if c % 2 else (a[:, 0] + (0.0 + a[:, 1])) / 2.0
    return out


def many_remainder_expected(mode, minimum, segments=None):
    """fsq_remainder_adjust's dict for many_segments(2) (its first `segments` segments), without a Python loop over segments."""
    rows, cats, seg_off, _ = many_segments(2)
    S = MANY_SEGMENTS if segments is None else segments
    seg_off = seg_off[:S + 1]
    n = int(seg_off[-1])
    rows, cats = rows[:n], cats[:n]
    seg = np.repeat(np.arange(S), np.diff(seg_off))
    m = (rows[:, 0] + (0.0 + rows[:, 1])) / 2.0                     # the median of two
    values = (rows - m[:, None]) / m[:, None] if mode == RR.RATIO else rows
    idx = np.flatnonzero(cats == np.uint64(3))
    count = np.bincount(seg[idx], minlength=S).astype(np.int32)
    pad = np.full((S, 3, 2), np.nan)
    pad[seg[idx], np.arange(len(idx)) - np.searchsorted(seg[idx], seg[idx], side="left")] = values[idx]
    adjustment = _small_medians(pad, count)
    if mode == RR.ADDITIVE:
        adjustment = adjustment - adjustment[:, :1]
    kept = ((count >= minimum) & ((mode == RR.RATIO) | (count >= 1))).astype(np.uint8)
    with np.errstate(all="ignore"):
        moved = rows * (1.0 - adjustment[seg]) if mode == RR.RATIO else rows - adjustment[seg]
    adjusted = np.where(kept[seg].astype(bool)[:, None], moved, 0.0)
    return {"adjusted": adjusted, "adjustment": adjustment, "n_remainders": count, "kept": kept}


# ---- E: the chain's steps ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def value_table():
    """(rows [n, 4], cats): every one of VALUES at an ON frame before an OFF frame (a last drop), at an ON frame before an ON
    frame and at an OFF frame, among ordinary tracks."""
    rng = np.random.default_rng(55)
    rows, cats = [], []
    for val in VALUES + (9000.0,):
        for word, f in ((0b0011, 1), (0b0111, 1), (0b0001, 2), (0b0101, 2), (0b0101, 0)):
            v = np.round(rng.uniform(500.0, 30000.0, 4))
            v[f] = val
            rows.append(v), cats.append(word)
    return np.array(rows), np.array(cats, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def nan_key_table():
    """(rows [n, 4], cats, seg_off, status, (segment, frame)): three fields of 40 tracks, every track with a sequence and an
    ON -> OFF step at frames 0 and 2; one entry of one key is NaN."""
    rng = np.random.default_rng(56)
    n = 120
    rows = np.round(rng.uniform(500.0, 30000.0, (n, 4)))
    cats = np.full(n, 0b0101, np.uint64)
    rows[57, 2] = np.nan
    return rows, cats, np.array([0, 40, 80, 120], np.int64), np.zeros(n, np.int32), (1, 2)
