"""Joint-signal problems for the background correction of two-colour experiments: the one-letter fixture rewritten as joint
keys, and synthetic problems of two label letters after the recipe of _background_cases.problem."""
import itertools

import numpy as np

LETTERS = ('C', 'K')


def jkey(pairs, letters=LETTERS):
    """The joint signal of (letter, cycle) drops that all end at zero: drops ascending by (cycle, letter), one True and the
    number of its drops per letter."""
    pairs = sorted(((aa, int(c)) for aa, c in pairs), key=lambda d: (d[1], letters.index(d[0])))
    return (tuple(pairs), (True,) * len(letters), tuple(sum(1 for aa, _ in pairs if aa == L) for L in letters))


def as_joint(key, letters=None):
    """The reference's (s, True, len(s)) as a joint key of its one letter, or of `letters` with every other channel empty."""
    s, z, si = key
    assert z and si == len(s)
    if letters is None:
        return (s, (True,), (si,))
    return (s, (True,) * len(letters), tuple(si if L == s[0][0] else 0 for L in letters))


def joint_dict(d, letters=None):
    return {as_joint(k, letters): v for k, v in d.items()}


def all_jkeys(C, D, letters=LETTERS, d_min=1):
    """Every joint key of d_min .. D drops over C cycles, in ascending order of its drops."""
    drops = [(L, c) for c in range(1, C + 1) for L in letters]
    return [jkey(combo, letters) for d in range(d_min, D + 1) for combo in itertools.combinations_with_replacement(drops, d)]


def joint_problem(n_keys, seed, C=12, D=3, d_min=1, letters=LETTERS, peaks=3, n_ac=3, sigma=2.0, include_multidrop=True, undefined=2,
                  skip=0):
    """(boc_raw, boc_percent, ac_average, ac_std, num_cycles, sigma, include_multidrop) with n_keys joint boc keys (fewer with
    multidrop excluded): smooth counts with planted peaks, ac- percents scattered around the smooth shape, `undefined` keys
    (from 8 keys on) that no ac- experiment has."""
    from fluorosequencingimageanalysis_amd import background as BG
    rng = np.random.default_rng(seed)
    keys = all_jkeys(C, D, letters, d_min)[skip:]
    assert len(keys) >= n_keys, (len(keys), n_keys)
    keys = keys[:n_keys]
    smooth = {k: 4000.0 * np.exp(-0.1 * sum(c for _, c in k[0])) for k in keys}
    boc = {k: int(round(v * rng.uniform(0.99, 1.01))) for k, v in smooth.items()}
    for i in rng.choice(n_keys, min(peaks, n_keys), replace=False):
        boc[keys[i]] += int(200 + 100 * rng.random())
    lacking = set(keys[i] for i in rng.choice(n_keys, undefined, replace=False)) if n_keys >= 8 else set()
    acs = [{k: int(round(v * rng.uniform(0.9, 1.1))) for k, v in smooth.items() if rng.random() > 0.03 and k not in lacking}
           for _ in range(n_ac)]
    avg = BG.average_signals(acs, include_multidrop=include_multidrop)
    std = BG.signals_std(acs, include_multidrop=include_multidrop)
    if not include_multidrop:
        boc = {k: v for k, v in boc.items() if not BG.is_multidrop(k[0])}
    pct = BG.counts_to_percent(boc, include_multidrop=include_multidrop)
    return boc, pct, avg, std, C, sigma, include_multidrop


def tiny_joint_problem(n):
    """One or two keys, the ac- dicts written by hand."""
    a, b = jkey([('C', 1), ('K', 2)]), jkey([('C', 1), ('K', 3)])
    if n == 1:
        return {a: 7}, {a: 1.0}, {a: 0.9}, {a: 0.1}, 3, 2.0, True                 # z = 1: the threshold stops it
    boc = {a: 100, b: 50}
    return boc, {a: 100 / 150.0, b: 50 / 150.0}, {a: 0.5, b: 0.5}, {a: 0.05, b: 0.05}, 3, 2.0, True
