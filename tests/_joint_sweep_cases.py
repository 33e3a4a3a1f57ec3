"""Shared by the joint-signal sweep tests (several label letters): hand-made molecules of K = 1 .. 4 colour channels with the
joint signal each must give, seeded random molecules, and the small sweeps the host and the GPU tests run.

There is no reference output for joint signals - the reference stops at one letter.  The oracle is the plain-Python
peptide_simulator.joint_signal and the NumPy twin (_host_signal_sweep), and K = 1 is tied to the one-letter key, which the
reference's recorded runs pin."""
import numpy as np

from fluorosequencingimageanalysis_amd import _host_signal_sweep as H

LETTERS = {1: ("K",), 2: ("C", "K"), 3: ("C", "D", "K"), 4: ("C", "D", "E", "K")}

# (rows [K][frames], kind, (decrements, zeros, starts) or None)
HAND = [
    # K = 2: drops of both channels at one cycle stand in channel order; channel 1 keeps a dye
    ([[2, 2, 1, 0, 0], [1, 1, 0, 0, 0]], H.ROW_SIGNAL, ((("C", 2), ("K", 2), ("C", 3)), (True, True), (2, 1))),
    ([[0, 0, 0, 0, 0], [3, 1, 1, 1, 1]], H.ROW_SIGNAL, ((("K", 1), ("K", 1)), (True, False), (0, 3))),
    ([[1, 1, 1], [1, 1, 1]], H.ROW_SIGNAL, ((), (False, False), (1, 1))),
    ([[0, 0, 0], [0, 0, 0]], H.ROW_SIGNAL, ((), (True, True), (0, 0))),
    ([[1, 1, 0], [1, 2, 0]], H.ROW_NONE, None),                                       # an upstep in channel 1 only
    ([[1, 2, 0], [1, 1, 0]], H.ROW_NONE, None),                                       # in channel 0 only
    ([[16, 0], [0, 0]], H.ROW_UNKEYED, None),
    ([[0, 0], [16, 16]], H.ROW_UNKEYED, None),
    ([[15, 15], [15, 15]], H.ROW_SIGNAL, ((), (False, False), (15, 15))),
    ([[4, 0, 0], [4, 4, 0]], H.ROW_SIGNAL, ((("C", 1),) * 4 + (("K", 2),) * 4, (True, True), (4, 4))),      # D(2) = 8 drops
    ([[5, 0, 0], [4, 4, 0]], H.ROW_UNKEYED, None),                                    # 9
    # K = 3
    ([[1, 0, 0, 0], [1, 1, 0, 0], [1, 1, 1, 0]], H.ROW_SIGNAL, ((("C", 1), ("D", 2), ("K", 3)), (True, True, True), (1, 1, 1))),
    ([[2, 2, 0, 0], [2, 2, 0, 0], [2, 2, 0, 1]], H.ROW_NONE, None),
    ([[2, 2, 0, 0], [2, 2, 0, 0], [2, 2, 2, 0]], H.ROW_SIGNAL,
     ((("C", 2), ("C", 2), ("D", 2), ("D", 2), ("K", 3), ("K", 3)), (True, True, True), (2, 2, 2))),        # D(3) = 6
    ([[2, 2, 0, 0], [2, 2, 0, 0], [3, 2, 2, 0]], H.ROW_UNKEYED, None),                # 7
    ([[0, 0], [0, 0], [15, 14]], H.ROW_SIGNAL, ((("K", 1),), (True, True, False), (0, 0, 15))),
    # K = 4
    ([[1, 0], [1, 0], [1, 0], [1, 0]], H.ROW_SIGNAL, ((("C", 1), ("D", 1), ("E", 1), ("K", 1)), (True,) * 4, (1, 1, 1, 1))),
    ([[3, 3, 0], [0, 0, 0], [0, 0, 0], [9, 6, 6]], H.ROW_SIGNAL,
     ((("K", 1), ("K", 1), ("K", 1), ("C", 2), ("C", 2), ("C", 2)), (True, True, True, False), (3, 0, 0, 9))),     # D(4) = 6
    ([[3, 3, 0], [1, 1, 0], [0, 0, 0], [9, 6, 6]], H.ROW_UNKEYED, None),
    ([[3, 3, 0], [0, 0, 0], [0, 1, 0], [9, 6, 6]], H.ROW_NONE, None),
    ([[0], [7], [0], [15]], H.ROW_SIGNAL, ((), (True, False, True, False), (0, 7, 0, 15))),     # one frame
]


def hand_rows(K):
    """The hand-made molecules of K channels: (rows, kind, signal)."""
    return [(rows, kind, sig) for rows, kind, sig in HAND if len(rows) == K]


def pad(rows, frames):
    """A molecule's rows continued at their last count to `frames` frames: the same drops, the same signal."""
    return [row + [row[-1]] * (frames - len(row)) for row in rows]


def random_molecules(rng, K, n, frames, max_start=3, upstep_rate=0.05):
    """uint8 [K][n][frames] of non-increasing rows, a few with an upstep."""
    rows = np.sort(rng.integers(0, max_start + 1, (K, n, frames)), axis=2)[:, :, ::-1].astype(np.uint8)
    for i in np.flatnonzero(rng.random(n) < upstep_rate).tolist():
        if frames > 1:
            rows[rng.integers(0, K), i, frames - 1] += 1
    return np.ascontiguousarray(rows)


# ---- the small sweeps ----

DDIF = [0, 0.3] + [0.3] * 5
QUENCH = dict(quench_factors=DDIF)                              # the fit's: max_possible + 2 entries
FIXED2 = dict(s=0.1, sc=3, s2=0.05, beta={"K": 70000.0, "C": 30000.0}, beta_sigma={"K": 0.2, "C": 0.25}, ddif=DDIF)
SHAPE2 = ("GAKCAK", "KC", 1, 4)                                 # two letters, 1 mock + 4 Edmans: 6 frames
FIXED3 = dict(s=0.1, sc=3, s2=0.05, beta={"K": 70000.0, "C": 30000.0, "D": 50000.0}, beta_sigma=0.2, ddif=DDIF)
SHAPE3 = ("GDKCAKD", "KCD", 2, 4)
POINTS3 = [(0.9, 0.05, 0.1), (0.7, 0.2, 0.4), (0.95, 0.1, 0.25)]
GRID4 = [(p, b, 0.2) for p in (0.8, 0.95) for b in (0.05, 0.15)]
GRID8 = [(p, b, u) for p in (0.8, 0.95) for b in (0.05, 0.15) for u in (0.1, 0.4)]

_cache = {}


def host_sweep(name, shape, points, n, fixed, **kw):
    """joint_sweep_records(host=True), computed once per name and shared: the reference of the GPU tests."""
    if name not in _cache:
        from fluorosequencingimageanalysis_amd import signal_sweep as SW
        _cache[name] = SW.joint_sweep_records(*shape, points, n, seed=5, host=True, **QUENCH, **dict(fixed, **kw))
    return _cache[name]


def observed_of(sweep, point_index=1):
    """An observed dict for scoring: one point's fitted signals, every count doubled and one signal more."""
    key = sweep["points"][point_index]
    obs = {s: 2 * n + 1 for s, n in sweep["all_simulations"][key][0].items()}
    obs[((("C", 1), ("K", 2)), (True, True), (1, 1))] = obs.get(((("C", 1), ("K", 2)), (True, True), (1, 1)), 0) + 3
    return obs
