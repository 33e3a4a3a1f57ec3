"""Inputs of the background correction's limit tests (tests/test_background_limits_host.py proves that they reach the paths
named there, tests/test_gpu_background_limits.py feeds them to the device).  Every problem is the argument tuple of
iterative_peak_finding_v3; expected values come from the restatement (tests/_background_reference.py)."""
import functools

from _background_cases import key, problem, tiny_problem

NAN, INF = float("nan"), float("inf")

# ---- F: keys of six drops ---------------------------------------------------------------------------------------------------
SIX_DROP_SEED, SIX_DROP_KEYS, SIX_DROP_CAP = 69, 461, 40           # (the cap on the passes of every run of these problems)
# the keys without controls, by hand: 728 and 242 neighbours in range, and two at the edge; without multi-drop no key repeats
# a position, and key(2, 3, 4) keeps 12 of its 26 neighbours
LACKING = {True: (key(2, 2, 3, 3, 4, 4), key(2, 3, 3, 4, 4), key(1, 1), key(5)), False: (key(2, 3, 4), key(1, 2), key(5))}


@functools.lru_cache(maxsize=None)
def six_drop_problem(include_multidrop):
    """The full key set of up to 6 drops over 5 cycles (461 keys; 31 without multi-drop), the keys of LACKING without
    controls.  With multi-drop it stops at the threshold after 25 passes; without, at a threshold of 1, it runs into the cap."""
    boc, pct, avg, std, C, _, md = problem(SIX_DROP_KEYS, SIX_DROP_SEED, C=5, D=6, undefined=0, include_multidrop=include_multidrop)
    for k in LACKING[bool(include_multidrop)]:
        del avg[k], std[k]
    return boc, pct, avg, std, C, 2.0 if include_multidrop else 1.0, md


def no_neighbour_problem():
    """One cycle: key(3) lies outside the filter and has no neighbour in range, so its trial value is the mean of nothing.  Its
    percent counts as 0, the trial lowers its z-score from 5 to 0 and is accepted: its count ends as NaN."""
    return {key(1): 100, key(3): 5}, {key(1): 1.0, key(3): 0.05}, {key(1): 1.0, key(3): 0.0}, {key(1): 0.01, key(3): 0.01}, 1, 2.0, True


# ---- G: zero totals ---------------------------------------------------------------------------------------------------------
def zero_total_problems():
    """name -> problem whose total is 0 somewhere: in the only trial (the only count replaced by the mean of an absent
    neighbour, 0), in the head, in the head only after the undefined key(1) is interpolated to its neighbour's 3, and in a
    trial of the second pass (the first accepts key(1): counts 10, 10, -10, 20, and key(4)'s trial then adds up 10 + 10 - 10 - 10)."""
    one = {key(1): 0.1}, {key(1): 0.01}
    two = {key(1): 0.1, key(2): 0.1}, {key(1): 0.01, key(2): 0.01}
    late = {key(2): 0.1, key(3): 0.1}, {key(2): 0.01, key(3): 0.01}
    boc = {key(1): 100, key(2): 10, key(3): -10, key(4): 20}
    pct = {k: v / 120.0 for k, v in boc.items()}
    avg = dict(pct)
    avg[key(1)] = 0.3
    return {"zero trial": ({key(1): 100}, {key(1): 1.0}) + one + (3, 2.0, True),
            "zero head": ({key(1): 5, key(2): -5}, {key(1): 0.5, key(2): -0.5}) + two + (3, 2.0, True),
            "zero after interpolation": ({key(1): 4, key(2): 3, key(3): -6}, {key(1): 4.0, key(2): 3.0, key(3): -6.0}) + late + (3, 2.0, True),
            "zero trial in the second pass": (boc, pct, avg, {k: 0.01 for k in boc}, 4, 2.0, True)}


ZERO_TOTAL_OUTCOMES = {"zero trial": (1, 0), "zero head": (1, 0), "zero after interpolation": (1, 0),
                       "zero trial in the second pass": (2, 1)}   # (passes, acceptances)


# ---- H: NaN and infinite scores ---------------------------------------------------------------------------------------------
def five_keys(nan_place=None, std_of=None):
    """The five-key problem of equal scores (keys 2 and 4 far above their controls, in that order), with a NaN control
    average at entry `nan_place` of the defined list, or other control stds."""
    boc = {key(1): 10, key(2): 100, key(3): 10, key(4): 100, key(5): 10}
    total = float(sum(boc.values()))
    pct = {k: v / total for k, v in boc.items()}
    order = [key(2), key(4), key(1), key(3), key(5)]
    avg = {k: (0.1 if k in (key(2), key(4)) else pct[k]) for k in order}
    std = {k: 0.01 for k in order}
    if nan_place is not None:
        avg[order[nan_place]] = NAN
    std.update(std_of or {})
    return boc, pct, avg, std, 5, 2.0, True


NAN_ENTRIES = (255, 256, 300)       # the last lane of the reduction's first round, the first of its second, and a later one


@functools.lru_cache(maxsize=None)
def nan_lane_problem(entry=None):
    """problem(400, 77) with a NaN control average at `entry` of the defined list (None: as it is)."""
    boc, pct, avg, std, C, sigma, md = problem(400, 77)
    if entry is not None:
        avg[[k for k in avg if std[k] != 0][entry]] = NAN
    return boc, pct, avg, std, C, sigma, md


def score_problems():
    """name -> problem with a NaN or an infinite z-score.  The infinite ones come from a control std of 1e-160, whose square is
    subnormal; at 1e-200 the square is 0 and the reference's own division raises ZeroDivisionError."""
    out = {"nan first": five_keys(0), "nan third": five_keys(2), "nan last": five_keys(4),
           "infinite z": five_keys(std_of={key(2): 1e-160}), "tied infinite z": five_keys(std_of={key(2): 1e-160, key(4): 1e-160})}
    out.update({"nan at %d" % e: nan_lane_problem(e) for e in NAN_ENTRIES})
    return out


# ---- I: many problems in one call -------------------------------------------------------------------------------------------
MANY, MANY_CAP = 300, 64            # problems, and the cap on the passes of each


@functools.lru_cache(maxsize=None)
def many_problems():
    """300 problems: tiny_problem(1), tiny_problem(2), 293 of problem(n, ...) with n cycling through 3 .. 40, the two six-drop
    problems (25 passes, and more than the cap) and three zero totals, spread over the list."""
    out = [tiny_problem(1), tiny_problem(2)] + [problem(3 + i % 38, 1000 + i) for i in range(MANY - 7)]
    zero = zero_total_problems()
    for at, args in ((40, zero["zero trial"]), (90, six_drop_problem(True)), (150, zero["zero head"]),
                     (210, six_drop_problem(False)), (260, zero["zero trial in the second pass"])):
        out.insert(at, args)
    assert len(out) == MANY
    return out


def ordinary_problems():
    return [problem(40, 22), tiny_problem(2)]
