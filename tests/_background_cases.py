"""The fixture of the background correction (tests/golden/background_signals.npz, written by tools/gen_background_golden.py)
decoded into the reference's dicts, and synthetic problems for the shapes the fixture lacks."""
import os

import numpy as np

from _util import GOLD

_G = None


def golden():
    global _G
    if _G is None:
        with np.load(os.path.join(GOLD, "background_signals.npz")) as g:
            _G = {k: g[k] for k in g.files}
    return _G


def key(*positions, si=None, letter='A'):
    return (tuple((letter, int(p)) for p in positions), True, len(positions) if si is None else si)


def dec_keys(g, prefix):
    pos, aa, z, si = (g["%s__%s" % (prefix, part)] for part in ("pos", "aa", "z", "si"))
    return [(tuple((chr(a), int(p)) for a, p in zip(aa[i], pos[i]) if p >= 0), bool(z[i]), int(si[i])) for i in range(len(z))]


def dec_values(g, prefix):
    values = g[prefix + "__bits"].view(np.float64)
    return [int(v) if i else float(v) for v, i in zip(values, g[prefix + "__int"])]


def dec(g, prefix):
    """A recorded dict, in its order."""
    return dict(zip(dec_keys(g, prefix), dec_values(g, prefix)))


def case_names():
    return [str(n) for n in golden()["cases"]]


def case(name):
    """The inputs, arguments and recorded outputs of one script case."""
    g = golden()
    c = {"name": name, "boc": dec(g, name + "__in_boc"), "acs": [dec(g, "%s__in_ac%d" % (name, i)) for i in range(int(g[name + "__n_ac"]))]}
    for k in ("head_boc", "head_ac", "boc_total", "ac_total", "omit_multidrop"):
        c[k] = int(g["%s__arg_%s" % (name, k)])
    c["boc_total"], c["ac_total"] = (None if c[k] < 0 else c[k] for k in ("boc_total", "ac_total"))
    c["num_cycles"], c["sigma"] = int(g[name + "__arg_num_cycles"]), float(g[name + "__arg_sigma"])
    for k in ("boc_experiment", "averaged_ac", "ac_stds", "boc_percent", "updated_boc_raw", "updated_boc_percent"):
        c[k] = dec(g, "%s__%s" % (name, k))
    c["corrected"] = None if int(g[name + "__corrected_keyerror"]) else dec(g, name + "__corrected")
    cols = [g["%s__undefined__%s" % (name, col)].view(np.float64) for col in ("bp", "ap", "sp")]
    c["undefined_peaks"] = [(k[0], k[1], k[2], float(bp), float(ap), float(sp))
                            for k, bp, ap, sp in zip(dec_keys(g, name + "__undefined"), *cols)]
    c["accepted"] = dec_keys(g, name + "__accepted")
    c["stop"], c["passes"] = int(g[name + "__stop"]), int(g[name + "__passes"])
    return c


def bits(values):
    return np.array([float(v) for v in values], dtype=np.float64).view(np.uint64).tolist()


def same_dict(got, exp, what=None):
    """Equal keys in equal order, values with equal bits."""
    assert list(got.keys()) == list(exp.keys()), what
    assert bits(got.values()) == bits(exp.values()), what


def same_peaks(got, exp, what=None):
    assert [u[:3] for u in got] == [u[:3] for u in exp], what
    for j in (3, 4, 5):
        assert bits(u[j] for u in got) == bits(u[j] for u in exp), (what, j)


# ---- synthetic problems (the recipe of the fixture's generator) ----

def signals(seed, n, C, D, planted=(), drop=0.0):
    rng = np.random.default_rng(seed)
    d = {}

    def add(positions, count):
        k = key(*positions)
        d[k] = d.get(k, 0) + int(count)
    for _ in range(n):
        drops = int(rng.integers(1, D + 1))
        add(sorted(min(int(rng.geometric(0.35)), C) for _ in range(drops)), 1)
    for positions, count in planted:
        add(positions, count)
    if drop > 0:
        d = {k: v for k, v in d.items() if rng.random() >= drop}
    return d


def all_keys(C, D):
    """Every sorted key of up to D drops over C cycles."""
    import itertools
    return [key(*p) for d in range(1, D + 1) for p in itertools.combinations_with_replacement(range(1, C + 1), d)]


def problem(n_keys, seed, C=12, D=4, peaks=3, n_ac=3, sigma=2.0, include_multidrop=True, undefined=2):
    """(boc_raw, boc_percent, ac_average, ac_std, num_cycles, sigma, include_multidrop) with exactly n_keys boc keys: smooth
    counts with `peaks` planted ones, ac- percents scattered around the smooth shape, `undefined` keys (from 8 keys on) that
    no ac- experiment has."""
    from fluorosequencingimageanalysis_amd import background as BG
    rng = np.random.default_rng(seed)
    keys = all_keys(C, D)
    assert len(keys) >= n_keys, (len(keys), n_keys)
    keys = keys[:n_keys]                                            # (neighbours in the list's order are mostly present)
    smooth = {k: 4000.0 * np.exp(-0.1 * sum(p for _, p in k[0])) for k in keys}
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


def tiny_problem(n):
    """One or two keys, the ac- dicts written by hand (an average over experiments of one key is 1 with a std of 0)."""
    if n == 1:
        return {key(1): 7}, {key(1): 1.0}, {key(1): 0.9}, {key(1): 0.1}, 3, 2.0, True                    # z = 1: the threshold stops it
    boc = {key(1): 100, key(2): 50}
    return boc, {key(1): 100 / 150.0, key(2): 50 / 150.0}, {key(1): 0.5, key(2): 0.5}, {key(1): 0.05, key(2): 0.05}, 3, 2.0, True
