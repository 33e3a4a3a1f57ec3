"""Inputs and expected values of the limit tests of the joint-signal sweep and of the multi-letter simulation
(tests/test_joint_limits_host.py proves that they reach the edges named here, tests/test_gpu_joint_limits.py feeds them to the
device).  Everything is seeded and built once.  Joint signals have no reference output: the oracle is the plain-Python
H.classify_joint_rows and the `simulate_labels` twin of _host_peptide_sim.  No torch, no GPU.

  C  the joint key's extreme values (every channel at 15 dyes, D(K) drops of channel K - 1 at cycle 63: bit 63 and all the
     bits below it), a joint tally of more rows than one pass of kss_tally_joint's grid, and one whose channels lie more than
     2^32 bytes apart
  D  fsq_peptide_simulate_labels_points with extreme parameters in neighbouring lanes at 1 and at 64 frames, and over more
     than two passes of its grid
  E  fsq_signal_pair_best over a thousand points, and a sweep whose keys carry bit 63"""
import functools

import numpy as np

import _simulate_limit_cases as SL
from _joint_sweep_cases import GRID4, LETTERS, random_molecules
from fluorosequencingimageanalysis_amd import _host_peptide_sim as PSIM
from fluorosequencingimageanalysis_amd import _host_signal_sweep as H

ALL_ONES = (1 << 64) - 1
TOP_BIT = 1 << 63

# ---- C: the joint key's extreme values ----------------------------------------------------------------------------------------
EXTREME_KEYS = {1: ALL_ONES, 2: ALL_ONES, 3: 0xff0bfbfbfbfbfbff, 4: ALL_ONES}
EXTREME_COPIES = (7, 5, 11)                                     # of the extreme row, the all-zero molecule, the mid-range one


def extreme_rows(K, more=0):
    """[K][64]: every channel at 15 dyes throughout, channel K - 1 losing D(K) + more dyes at frame 63."""
    rows = [[15] * 64 for _ in range(K)]
    rows[K - 1][63] = 15 - H.JOINT_MAX_DROPS[K] - more
    return rows


def mid_rows(K):
    """[K][64]: channel k starts at 3 + k dyes and loses one at frame 10 + k; the last channel another at frame 40."""
    rows = [[3 + k] * (10 + k) + [2 + k] * (54 - k) for k in range(K)]
    rows[K - 1][40:] = [r - 1 for r in rows[K - 1][40:]]
    return rows


def extreme_molecules(K):
    """(rows uint8 [K][23][64], [(key, copies)] of the three molecules in their order)."""
    each = [extreme_rows(K), [[0] * 64 for _ in range(K)], mid_rows(K)]
    rows = np.array([m for m, n in zip(each, EXTREME_COPIES) for _ in range(n)], np.uint8).transpose(1, 0, 2)
    return np.ascontiguousarray(rows), [(H.classify_joint_rows(m)[1], n) for m, n in zip(each, EXTREME_COPIES)]


# ---- C: more rows than one pass of kss_tally_joint ----------------------------------------------------------------------------
T_N, T_K, T_FRAMES, T_POINTS, T_BASE, T_SLOTS, T_CUT = SL.TALLY_BLOCKS * SL.TALLY_BLOCK + 300, 2, 3, 3, 997, 512, 1234567
T_PER = -(-T_N // T_POINTS)


@functools.lru_cache(maxsize=None)
def tally_base():
    """uint8 [2][997][3]: seeded molecules of two channels, a few with an upstep."""
    return random_molecules(np.random.default_rng(997), T_K, T_BASE, T_FRAMES, max_start=2)


@functools.lru_cache(maxsize=None)
def tally_valid():
    """uint8 [T_N]: nine rows in ten."""
    return (np.random.default_rng(998).random(T_N) < 0.9).astype(np.uint8)


def tally_rows_of(lo, hi):
    """(rows [2][hi - lo][3], points) lo .. hi - 1 of the large case: row i is base molecule i mod 997 at point i // T_PER."""
    i = np.arange(lo, hi)
    return np.ascontiguousarray(tally_base()[:, i % T_BASE]), (i // T_PER).astype(np.int32)


def tally_expected(lo, hi, valid=None):
    """H.tally_joint_rows' triple for rows lo .. hi - 1: the 997 base molecules are classified once, then one np.add.at over
    (point, base index)."""
    base = tally_base()
    i = np.arange(lo, hi)
    if valid is not None:
        i = i[valid[lo:hi] != 0]
    n = np.zeros((T_POINTS, T_BASE), np.int64)
    np.add.at(n, (i // T_PER, i % T_BASE), 1)
    return tables_of_counts(base, n)


# ---- C: a channel stride beyond 32 bits ----------------------------------------------------------------------------------------
# kss_tally_joint finds channel k of molecule g at (k * n_rows + g) * frames.  With 64 frames and 2^26 + 300 molecules the
# channel stride is 2^32 + 19 200 bytes: one kept in 32 bits would take channel 1 from molecule g + 300's channel 0 (inside
# the table, and another molecule: 300 is no multiple of 101).  No smaller table has a stride that 32 bits do not hold.
W_N, W_K, W_FRAMES, W_POINTS, W_BASE, W_SLOTS, W_SHIFT = (1 << 26) + 300, 2, 64, 3, 101, 512, 300
W_PER = -(-W_N // W_POINTS)


@functools.lru_cache(maxsize=None)
def wide_base():
    """uint8 [2][101][64]: seeded molecules of two channels and 64 frames, at most two dyes a channel."""
    return random_molecules(np.random.default_rng(101), W_K, W_BASE, W_FRAMES, max_start=2)


def wide_counts(lo, hi):
    """int64 [3][101]: how many rows i of lo .. hi - 1 lie at point i // W_PER with i mod 101 == j, in closed form."""
    j = np.arange(W_BASE, dtype=np.int64)
    upto = lambda x: (x - j + W_BASE - 1) // W_BASE                                  # noqa: E731  rows below x that are j mod 101
    return np.stack([upto(max(min(hi, (k + 1) * W_PER), lo)) - upto(min(max(lo, k * W_PER), hi)) for k in range(W_POINTS)])


def tables_of_counts(base, n):
    """H.tally_joint_rows' triple of n[point][base index] molecules of base [K][m][frames]: m molecules are classified."""
    kinds = [H.classify_joint_rows(base[:, j].tolist()) for j in range(base.shape[1])]
    tables, none, unkeyed = [{} for _ in n], [0] * len(n), [0] * len(n)
    for k, row in enumerate(np.asarray(n).tolist()):
        for (what, key), c in zip(kinds, row):
            if what == H.ROW_SIGNAL and c:
                tables[k][key] = tables[k].get(key, 0) + c
            elif what == H.ROW_NONE:
                none[k] += c
            elif what == H.ROW_UNKEYED:
                unkeyed[k] += c
    return tables, none, unkeyed


def wide_rows_of(lo, hi, shift=0):
    """(rows [2][hi - lo][64], points) lo .. hi - 1 of the wide case: row i is base molecule i mod 101 at point i // W_PER.
    With `shift`, channel 1 is channel 0 of the molecule `shift` rows on: what a stride of 32 bits would read."""
    i = np.arange(lo, hi)
    rows = np.ascontiguousarray(wide_base()[:, i % W_BASE])
    if shift:
        rows[1] = wide_base()[0, (i + shift) % W_BASE]
    return rows, (i // W_PER).astype(np.int32)


def wide_expected(lo=0, hi=W_N):
    return tables_of_counts(wide_base(), wide_counts(lo, hi))


# ---- D: the multi-letter points kernel ----------------------------------------------------------------------------------------
def point_dicts(values):
    """float64 [P][5] of (p, per_cycle_b, u, s, s2) as the point dicts a sweep takes."""
    return [dict(zip(SL.POINT_KEYS, (float(x) for x in row))) for row in np.asarray(values).tolist()]


D_SEED, D_FIRST_MOLECULE = 4243, 7
D_SHAPES = {
    "3_letters_1_frame": (("GKACDAKC", "KCD", 0, 0),
                          dict(sc=3, beta={"K": 7e4, "C": 3e4, "D": 5e4}, beta_sigma={"K": 0.2, "C": 0.25, "D": 0.15},
                               ddif=[0.0] + [0.3] * 14, superdye_rate={"K": 0.3, "C": 0.0, "D": 1.0}, superdye_factor=2.0)),
    "4_letters_64_frames": (("GA" * 20 + "KCDE" * 6, "KCDE", 23, 40),
                            dict(sc=3, beta={"K": 7e4, "C": 3e4, "D": 5e4, "E": 9e4}, beta_sigma=0.2, ddif=[0.0] + [0.3] * 14,
                                 superdye_rate={"K": 0.3, "C": 0.0, "D": 1.0, "E": 0.0}, superdye_factor=2.0)),
}


def labels_params(shape, fixed, values, seed, first_molecule):
    """(the base FsqPeptideLabelsParams, float64 [P][5], the sorted letters) as a joint sweep builds them from point dicts."""
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    base, point_values, _, letters = SW._joint_point_params(*shape, seed, first_molecule, point_dicts(values), fixed)
    assert np.array_equal(point_values, np.asarray(values, np.float64))
    return base, point_values, letters


def labels_twin(prm, point, first_molecule, n):
    """_host_peptide_sim.simulate_labels of n molecules under the channel values of `prm` and one point's five values."""
    K = prm.n_channels
    p, per_cycle_b, u, s, s2 = (float(x) for x in point)
    return PSIM.simulate_labels(prm.length, list(prm.channel_mask)[:K], prm.num_mocks, prm.num_edmans, p, per_cycle_b, u, s, prm.sc, s2,
                                list(prm.log_beta)[:K], list(prm.beta_sigma)[:K], [list(prm.ddif[k])[:prm.n_ddif[k]] for k in range(K)],
                                list(prm.superdye_rate)[:K], list(prm.superdye_factor)[:K], prm.seed, first_molecule, n)


def twin_rows(prm, values, n_per_point, stride, first_molecule, lo, hi, keys=("counts", "intensity", "category")):
    """Rows lo .. hi - 1 of the flattened [points][n_per_point] space by the twin, a point's part at a time: the channel-major
    tables along their molecule axis, the per-molecule ones (loss_cause, edman_fail) along their first."""
    parts = []
    while lo < hi:
        k = lo // n_per_point
        n = min(hi, (k + 1) * n_per_point) - lo
        parts.append(labels_twin(prm, values[k], first_molecule + k * stride + lo - k * n_per_point, n))
        lo += n
    return tuple(np.concatenate([p[key] for p in parts], axis=1 if key in ("counts", "intensity", "category") else 0) for key in keys)


@functools.lru_cache(maxsize=None)
def extreme_points_expected(shape_name, stride, keys=("counts", "intensity", "category")):
    """The 70 points of _simulate_limit_cases.limit_points, 3 molecules each, point by point."""
    shape, fixed = D_SHAPES[shape_name]
    values = SL.limit_points()
    prm, _, _ = labels_params(shape, fixed, values, D_SEED, D_FIRST_MOLECULE)
    return twin_rows(prm, values, SL.B_PER, stride, D_FIRST_MOLECULE, 0, SL.B_POINTS * SL.B_PER, keys)


# more than two passes: 16 384 blocks of 64 rows are launched at most
P_SHAPE, P_FIXED = ("KGCK", "KC", 0, 1), dict(sc=1, beta={"K": 7e4, "C": 3e4}, beta_sigma={"K": 0.2, "C": 0.25},
                                              ddif=[0.0, 0.3, 0.3], superdye_rate={"K": 0.0, "C": 0.4}, superdye_factor=2.0)
P_POINTS = SL.A1_POINTS
P_PASS = SL.SIM_BLOCKS * SL.SIM_WAVE
P_PER, P_STRIDE, P_FIRST_ROW, P_ROWS, P_SEED, P_FIRST_MOLECULE = 419500, 1000003, 100, 2 * P_PASS + 130, 20262, 17


def p_windows():
    """[lo, hi) in local rows: the head, the tail, +-100 round the two pass seams and +-70 round every point boundary."""
    w = [(0, 100), (P_ROWS - 100, P_ROWS), (P_PASS - 100, P_PASS + 100), (2 * P_PASS - 100, 2 * P_PASS + 100)]
    return w + [(k * P_PER - P_FIRST_ROW - 70, k * P_PER - P_FIRST_ROW + 70) for k in range(1, len(P_POINTS))]


def p_point_ranges():
    """(point, local row lo, local row hi, first molecule) of every point's part of the launch."""
    out = []
    g, end = P_FIRST_ROW, P_FIRST_ROW + P_ROWS
    while g < end:
        k = g // P_PER
        n = min(end, (k + 1) * P_PER) - g
        out.append((k, g - P_FIRST_ROW, g - P_FIRST_ROW + n, P_FIRST_MOLECULE + k * P_STRIDE + g - k * P_PER))
        g += n
    return out


@functools.lru_cache(maxsize=None)
def p_expected():
    """{(lo, hi): (counts, intensity, category)} of p_windows by the twin."""
    prm, _, _ = labels_params(P_SHAPE, P_FIXED, P_POINTS, P_SEED, P_FIRST_MOLECULE)
    return {(lo, hi): twin_rows(prm, P_POINTS, P_PER, P_STRIDE, P_FIRST_MOLECULE, P_FIRST_ROW + lo, P_FIRST_ROW + hi)
            for lo, hi in p_windows()}


# ---- E: the pair kernel over a sweep-sized grid -------------------------------------------------------------------------------
E_S, E_P = 60, 1000
# candidates of score_case(60, 1000): heat-map keys, keys that observe 0, 1 and 2, one in no dict (-1), the key that observes
# 2^30, one never fitted, the zero-variance key, the DOMAIN key, the 2^31 - 1 key and one that is not admitted
E_ROWS = [0, 3, 12, 13, -1, 25, SL.KEY_HALF, 55, SL.KEY_ZERO_VARIANCE, SL.KEY_DOMAIN, SL.KEY_BIG, 6]
E_METRICS = ("my_euclidean", "my_std_normalized_euclidean", "my_normalized_chebyshev")
E_RUNS = [(norm, reverse) for norm in (H.NORMALIZE_COUNTS, H.HEATMAP_NORMALIZE_COUNTS) for reverse in (False, True)]


@functools.lru_cache(maxsize=None)
def pair_expected(metric):
    """{(normalization, reverse_order): (H.pair_best's dict, H.pair_extremes' pair)} on score_case(60, 1000)."""
    table, fit, total = SL.score_case(E_S, E_P)
    out = {}
    for norm, reverse in E_RUNS:
        best = H.pair_best(table, E_ROWS, fit, total, metric, norm, None, reverse)
        out[(norm, reverse)] = (best, H.pair_extremes(best["dist"], len(E_ROWS), reverse))
    return out


# ---- E: a sweep whose keys carry bit 63 ---------------------------------------------------------------------------------------
TOP_QUENCH = [0, 0.1] + [0.1] * 8
TOP_SHAPE, TOP_N = ("GGCKKKKKKKK", "KC", 1, 3), 200
TOP_KW = dict(seed=5, max_possible=8, quench_factors=TOP_QUENCH, s=0.0, sc=3, s2=0.0, beta={"K": 70000.0, "C": 30000.0},
              beta_sigma={"K": 0.1, "C": 0.15}, ddif=TOP_QUENCH)
TOP_LETTERS = LETTERS[2]
_cache = {}


def top_bit_sweep():
    """joint_sweep_records(host=True) of the eight-lysine peptide, computed once: channel K starts with 8 dyes."""
    if "sweep" not in _cache:
        from fluorosequencingimageanalysis_amd import signal_sweep as SW
        _cache["sweep"] = SW.joint_sweep_records(*TOP_SHAPE, GRID4, TOP_N, host=True, **TOP_KW)
    return _cache["sweep"]


def has_top_bit(signal):
    return bool(H.joint_key_of_signal(TOP_LETTERS, signal) & TOP_BIT)


def top_bit_observed():
    """An observed dict for scoring: the second point's fitted signals, every count doubled and one more."""
    sweep = top_bit_sweep()
    return {s: 2 * n + 1 for s, n in sweep["all_simulations"][sweep["points"][1]][0].items()}


def top_bit_candidates():
    """Twelve heat-map signals and the eight most frequent observed signals with bit 63 set: the candidates of the pair loop."""
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    obs = top_bit_observed()
    top = sorted((s for s in obs if has_top_bit(s)), key=lambda s: (-obs[s], H.joint_key_of_signal(TOP_LETTERS, s)))[:8]
    return list(SW.joint_split_heatmap(TOP_LETTERS, 4, 0)[1][:12]) + top
