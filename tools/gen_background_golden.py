"""Writes tests/golden/background_signals.npz: synthetic signals dicts through the reference's iterative_background_v2 chain
(head_truncate, discard_late_signals, average_signals, signals_std, counts_to_percent, iterative_peak_finding_v3), the helper
functions on small inputs, and what the reference does with the inputs background.py refuses.

Loads MCsimlib.py at run time through oracle/refload.py, as tools/gen_lognormal_golden.py does, with the key-order contract of
DESIGN.md 4.19 patched in: every `combined_keys = tuple(set(` becomes `combined_keys = _ordered(set(` with
`_ordered = lambda s: tuple(sorted(s))`, and dicts are Python 3's (insertion order).  `sum` is injected as Python 2's plain
left-to-right sum and `round` as Python 2's.  Five more patches only record: they append the pass starts, the accepted key and
the stop reason of iterative_peak_finding_v3 to a list.  The rest of iterative_background_v2.py is at module level and parses
its arguments on import; `script()` below is the composition of the MCsimlib calls it makes (:176-299), in its order.

Signals are own code (the recipe of the issue): per molecule d = rng.integers(1, D + 1) drops at positions
sorted(min(rng.geometric(0.35), C)), counts accumulated per key ((('A', p), ...), True, d); boc peaks planted on top at (2,),
(1, 3), (2, 2) and, for D >= 3, (2, 3, 5); optionally each key dropped with a probability, so that key sets differ.

The generator asserts that the fixture is not vacuous: a case with >= 10 accepted replacements, one with undefined keys and
accepted replacements, one without a defined z-score, one stopped by the threshold.  It prints which of the other two stop
reasons occurred.  In the fixture as committed both occur: "no improvement" (z_diff <= 0) in late_keys, five_drops and
truncated, "converged" (largest change < 0.001) in two_ac after 1 100 accepted replacements.  one_ac inserts keys that boc
lacks, on which the reference's script ends with a KeyError at :295-299; the fixture records that instead of `corrected`.

  python tools/gen_background_golden.py [--reference DIR]
"""
import argparse
import ctypes
import os
import subprocess
import sys
import time
import types

NPY_ENV = "AVX512F AVX512CD AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR"
if __name__ == "__main__" and os.environ.get("NPY_DISABLE_CPU_FEATURES") != NPY_ENV:
    os.environ["NPY_DISABLE_CPU_FEATURES"] = NPY_ENV
    sys.exit(subprocess.call([sys.executable] + sys.argv))         # a fresh child: numpy reads the variable at import

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_DROPS = 6
STOPS = {1: "no defined z-score", 2: "threshold", 3: "no improvement", 4: "converged"}
TRACE = []


def _py2_sum(values, start=0):
    for v in values:
        start = start + v
    return start


def load_mcsimlib(refload):
    import multiprocessing.pool  # noqa: F401  (before the reference's `import multiprocessing` is used)
    import string
    if not hasattr(string, "letters"):
        string.letters = string.ascii_letters
    sk = types.ModuleType("sklearn")
    sk.mixture, sk.cluster = types.ModuleType("sklearn.mixture"), types.ModuleType("sklearn.cluster")
    sk.mixture.GMM = sk.mixture.DPGMM = sk.cluster.KMeans = None
    for name, mod in (("sklearn", sk), ("sklearn.mixture", sk.mixture), ("sklearn.cluster", sk.cluster)):
        sys.modules.setdefault(name, mod)
    libm = ctypes.CDLL("libm.so.6")
    libm.round.restype, libm.round.argtypes = ctypes.c_double, [ctypes.c_double]
    patches = [
        # the key-order contract
        ("combined_keys = tuple(set(", "combined_keys = _ordered(set("),
        # recording only
        ("        z_scores, undefined_z_scores = outlier_z_scores(", "        _trace.append(('pass',)); z_scores, undefined_z_scores = outlier_z_scores("),
        ("        if len(z_scores) == 0:\n            break", "        if len(z_scores) == 0:\n            _trace.append(('stop', 1))\n            break"),
        ("        if z_scores[outlier] <= sigma_threshold:\n            break",
         "        if z_scores[outlier] <= sigma_threshold:\n            _trace.append(('stop', 2))\n            break"),
        ("        if z_diffs[best_improvement] <= 0:\n            break",
         "        if z_diffs[best_improvement] <= 0:\n            _trace.append(('stop', 3))\n            break"),
        ("            if max(abs_diffs) < 0.001:\n                break",
         "            if max(abs_diffs) < 0.001:\n                _trace.append(('stop', 4))\n                break"),
        ("        outlier = best_improvement\n", "        outlier = best_improvement\n        _trace.append(('accept', outlier))\n"),
    ]
    return refload.load("MCsimlib", "MCsimlib.py", patches=patches,
                        inject={"round": lambda x: libm.round(float(x)), "sum": _py2_sum, "_ordered": lambda s: tuple(sorted(s)),
                                "_trace": TRACE})


# ---- synthetic signals (own code) ----

def signals(seed, n, C, D, planted=True, drop=0.0):
    rng = np.random.default_rng(seed)
    d = {}

    def add(positions, count):
        key = (tuple(('A', int(p)) for p in positions), True, len(positions))
        d[key] = d.get(key, 0) + int(count)
    for _ in range(n):
        drops = int(rng.integers(1, D + 1))
        add(sorted(min(int(rng.geometric(0.35)), C) for _ in range(drops)), 1)
    if planted:
        add((2,), n // 10)
        add((1, 3), n // 15)
        add((2, 2), n // 20)
        if D >= 3 and C >= 5:
            add((2, 3, 5), n // 20)
    if drop > 0:
        d = {k: v for k, v in d.items() if rng.random() >= drop}
    return d


# ---- the script's composition (iterative_background_v2.py:176-299) ----

def script(M, boc, acs, num_cycles, head_boc=0, head_ac=0, boc_total=None, ac_total=None, omit_multidrop=False, sigma=2):
    include_multidrop = not omit_multidrop
    include_remainders = False
    ac_experiments = {}
    for ac_index, ac_signals in enumerate(acs):
        ac_experiments.setdefault(ac_index, {k: count for k, count in ac_signals.items() if k[1]})
    if head_ac > 0:
        for ac_index in list(ac_experiments.keys()):
            ac_experiments[ac_index] = M.head_truncate(signals=ac_experiments[ac_index], num_cycles=head_ac)
    if ac_total is not None:
        for ac_index in list(ac_experiments.keys()):
            ac_experiments[ac_index] = M.discard_late_signals(signals=ac_experiments[ac_index], max_cycle=ac_total)
    boc_experiment = {k: count for k, count in boc.items() if k[1]}
    if head_boc > 0:
        boc_experiment = M.head_truncate(signals=boc_experiment, num_cycles=head_boc)
    if boc_total is not None:
        boc_experiment = M.discard_late_signals(signals=boc_experiment, max_cycle=boc_total)
    if omit_multidrop:
        boc_experiment = {(s, z, si): count for (s, z, si), count in boc_experiment.items() if len(s) == len(set(s))}
    averaged_ac = M.average_signals(experiments=list(ac_experiments.values()), include_remainders=include_remainders,
                                    include_multidrop=include_multidrop, max_cycle=None)
    ac_stds = M.signals_std(experiments=list(ac_experiments.values()), include_remainders=include_remainders,
                            include_multidrop=include_multidrop, max_cycle=None)
    boc_percent = M.counts_to_percent(signals=boc_experiment, include_remainders=include_remainders,
                                      include_multidrop=include_multidrop, max_cycle=None)
    del TRACE[:]
    peak_list, undefined_peaks, updated_boc_raw, updated_boc_percent = M.iterative_peak_finding_v3(
        boc_raw=boc_experiment, boc_percent=boc_percent, ac_average=averaged_ac, ac_std=ac_stds, num_cycles=num_cycles,
        sigma_threshold=sigma, include_multidrop=include_multidrop)
    assert peak_list == []
    try:
        corrected = {k: max(boc_experiment[k] - background_count, 0) for k, background_count in updated_boc_raw.items()}
    except KeyError:                  # (a key inserted by the iteration: the reference's script ends here, :295-299)
        corrected = None
    return dict(boc_experiment=boc_experiment, averaged_ac=averaged_ac, ac_stds=ac_stds, boc_percent=boc_percent,
                undefined_peaks=undefined_peaks, updated_boc_raw=updated_boc_raw, updated_boc_percent=updated_boc_percent,
                corrected=corrected, trace=list(TRACE))


# ---- encoding: keys as integer arrays, floats as bits ----

def enc_keys(keys):
    keys = list(keys)
    pos = np.full((len(keys), MAX_DROPS), -1, np.int16)
    aa = np.zeros((len(keys), MAX_DROPS), np.uint8)
    for i, (s, z, si) in enumerate(keys):
        for j, (a, p) in enumerate(s):
            pos[i, j], aa[i, j] = p, ord(a)
    return {"pos": pos, "aa": aa, "z": np.array([bool(k[1]) for k in keys], dtype=np.uint8),
            "si": np.array([int(k[2]) for k in keys], dtype=np.int64)}


def enc_values(values):
    values = list(values)
    return {"bits": np.array([float(v) for v in values], dtype=np.float64).view(np.uint64),
            "int": np.array([isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in values], dtype=np.uint8)}


def put(out, prefix, d):
    """A dict in its order."""
    for part, a in list(enc_keys(d.keys()).items()) + list(enc_values(d.values()).items()):
        out["%s__%s" % (prefix, part)] = a


def put_trace(out, prefix, trace):
    accepts = [t[1] for t in trace if t[0] == 'accept']
    stops = [t[1] for t in trace if t[0] == 'stop']
    assert len(stops) == 1, trace
    for part, a in enc_keys(accepts).items():
        out["%s__accepted__%s" % (prefix, part)] = a
    out[prefix + "__stop"] = np.int64(stops[0])
    out[prefix + "__passes"] = np.int64(sum(1 for t in trace if t[0] == 'pass'))
    return len(accepts), stops[0]


def put_script(out, name, M, boc, acs, **kw):
    t0 = time.time()
    r = script(M, boc, acs, **kw)
    put(out, name + "__in_boc", boc)
    out[name + "__n_ac"] = np.int64(len(acs))
    for i, ac in enumerate(acs):
        put(out, "%s__in_ac%d" % (name, i), ac)
    args = dict(head_boc=0, head_ac=0, boc_total=-1, ac_total=-1, omit_multidrop=0, sigma=2.0)
    args.update({k: (-1 if v is None else v) for k, v in kw.items()})
    for k, v in args.items():
        out["%s__arg_%s" % (name, k)] = np.float64(v) if k == "sigma" else np.int64(v)
    for k in ("boc_experiment", "averaged_ac", "ac_stds", "boc_percent", "updated_boc_raw", "updated_boc_percent", "corrected"):
        if r[k] is not None:
            put(out, "%s__%s" % (name, k), r[k])
    out[name + "__corrected_keyerror"] = np.int64(r["corrected"] is None)
    up = r["undefined_peaks"]
    for part, a in enc_keys([(s, z, si) for s, z, si, bp, ap, sp in up]).items():
        out["%s__undefined__%s" % (name, part)] = a
    for j, col in enumerate(("bp", "ap", "sp")):
        out["%s__undefined__%s" % (name, col)] = np.array([float(u[3 + j]) for u in up], dtype=np.float64).view(np.uint64)
    n_acc, stop = put_trace(out, name, r["trace"])
    n_und = len(set((u[0], u[1], u[2]) for u in up))
    info = dict(name=name, accepted=n_acc, stop=stop, undefined_records=len(up), undefined_keys=n_und,
                boc_keys=len(r["boc_experiment"]), keys_after=len(r["updated_boc_raw"]), defined=sum(1 for v in r["ac_stds"].values() if v != 0))
    print("%-22s %s  %.1f s" % (name, {k: v for k, v in info.items() if k != "name"}, time.time() - t0), flush=True)
    return info


def outcome(fn):
    """What the reference does: '' or the exception's class name and message."""
    try:
        fn()
    except BaseException as e:      # noqa: BLE001 - recorded
        return "%s: %s" % (type(e).__name__, e)
    return ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None)
    args = ap.parse_args()
    if args.reference:
        os.environ["FSQ_REFERENCE"] = args.reference
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import refload
    M = load_mcsimlib(refload)
    out, names, infos = {}, [], []

    def case(name, boc, acs, **kw):
        names.append(name)
        infos.append(put_script(out, name, M, boc, acs, **kw))

    boc = signals(3, 4000, 6, 3)
    acs3 = [signals(11 + i, 4000, 6, 3, planted=False, drop=0.1 + 0.025 * i) for i in range(3)]
    case("three_ac_multidrop", boc, acs3, num_cycles=6)
    case("three_ac_no_multidrop", boc, acs3, num_cycles=6, omit_multidrop=True)
    boc_lacking = signals(3, 4000, 6, 3, drop=0.1)                   # (ac- keys that boc lacks are inserted where their std is 0)
    case("two_ac", boc_lacking, acs3[:2], num_cycles=6)
    case("one_ac", boc_lacking, acs3[:1], num_cycles=6)
    case("late_keys", boc, acs3, num_cycles=5)
    case("five_drops", signals(5, 3000, 3, 5), [signals(21 + i, 3000, 3, 5, planted=False, drop=0.12) for i in range(3)], num_cycles=3)
    case("truncated", signals(7, 3000, 7, 2), [signals(31 + i, 3000, 8, 2, planted=False, drop=0.1) for i in range(3)],
         num_cycles=5, head_boc=1, head_ac=2, boc_total=5, ac_total=5, sigma=1.5)
    case("eight_cycles", signals(3, 6000, 8, 3, drop=0.05), [signals(41 + i, 6000, 8, 3, planted=False, drop=0.1 + 0.02 * i) for i in range(3)],
         num_cycles=8)
    case("high_sigma", boc, acs3, num_cycles=6, sigma=1000.0)
    out["cases"] = np.array(names)

    # ---- helpers on small inputs ----
    small = signals(9, 300, 4, 2)
    put(out, "helpers__in", small)
    for c in (0, 1, 2):
        put(out, "helpers__head_truncate_%d" % c, M.head_truncate(signals=small, num_cycles=c))
        put(out, "helpers__discard_late_%d" % c, M.discard_late_signals(signals=small, max_cycle=c))
    put(out, "helpers__percent", M.counts_to_percent(small))
    put(out, "helpers__percent_no_multidrop_3", M.counts_to_percent(small, include_multidrop=False, max_cycle=3))
    second, third = signals(10, 300, 4, 2, drop=0.3), signals(12, 300, 4, 2, drop=0.3)
    put(out, "helpers__in2", second)
    put(out, "helpers__in3", third)
    put(out, "helpers__sum", M.sum_signals([small, second]))
    out["helpers__is_multidrop"] = np.array([M.is_multidrop(k[0]) for k in small], dtype=np.uint8)
    target = ((('A', 2), ('A', 3)), True, 2)
    for md in (0, 1):
        out["helpers__adjacent_%d" % md] = np.array(M.generate_adjacent_positions(target, include_multidrop=bool(md)), dtype=np.int64)
        out["helpers__interpolated_%d" % md] = np.array([float(M.interpolate_signal(small, k, 4, include_multidrop=bool(md)))
                                                         for k in small], dtype=np.float64).view(np.uint64)
    pct = M.counts_to_percent(small)
    avg = M.average_signals([second, third])
    std = M.signals_std([second, third])
    for k in list(std)[:2]:
        std[k] = 0.0                                                 # (two undefined keys for outlier_z_scores below)
    put(out, "helpers__average", avg)
    put(out, "helpers__std_two_zeroed", std)
    zs, und = M.outlier_z_scores(pct, avg, std)
    put(out, "helpers__z", zs)
    put(out, "helpers__undefined", {k: v[0] for k, v in und.items()})

    # ---- what the reference does with the refused inputs ----
    one = {((('A', 1),), True, 1): 5, ((('A', 2),), True, 1): 7, ((('A', 1), ('A', 2)), True, 2): 3}
    ac_a = {((('A', 1),), True, 1): 4, ((('A', 2),), True, 1): 9}
    ac_b = {((('A', 1),), True, 1): 6, ((('A', 2),), True, 1): 5, ((('A', 1), ('A', 2)), True, 2): 2}
    # two keys that boc lacks next to a negative count: their interpolated counts are negative, so that with a negative
    # threshold each is the best trial of a pass, and the second one inserted trips the assert at :6006
    key = lambda *p: (tuple(('A', q) for q in p), True, len(p))       # noqa: E731
    neg = {key(1): 50, key(2): 70, key(1, 2): -30}
    neg_a = {key(1): 40, key(2): 90, key(1, 2): 5, key(2, 3): 4, key(1, 1): 3}
    neg_b = {key(1): 60, key(2): 50, key(1, 2): 9, key(2, 3): 8, key(1, 1): 9}

    ac_far = dict(ac_a)
    ac_far[((('A', 6), ('A', 7)), True, 2)] = 3                      # std 0, every position >= num_cycles + 2

    def v3(boc_raw, acs, num_cycles, sigma=2, boc_percent=None):
        avg, std = M.average_signals(acs), M.signals_std(acs)
        pct = M.counts_to_percent(boc_raw) if boc_percent is None else boc_percent
        return M.iterative_peak_finding_v3(boc_raw, pct, avg, std, num_cycles, sigma_threshold=sigma, include_multidrop=True)
    two = dict(one)
    two[((('B', 2), ('B', 3)), True, 2)] = 4
    refusals = {
        "two_letters": lambda: v3(two, [ac_a, ac_b], 3),
        "key_mismatch": lambda: v3(one, [ac_a, ac_b], 3, boc_percent={((('A', 1),), True, 1): 1.0}),
        "negative_sigma": lambda: v3(neg, [neg_a, neg_b], 4, sigma=-1000.0),
        "zero_total": lambda: v3({k: 0 for k in one}, [ac_a, ac_b], 3, boc_percent={k: 0.0 for k in one}),
        "no_neighbour_one_cycle": lambda: v3({((('A', 1),), True, 1): 5}, [{((('A', 1),), True, 1): 4}], 1),
        "no_neighbour_far_key": lambda: v3(one, [ac_far], 4),
    }
    for name, fn in refusals.items():
        out["refusal__" + name] = np.array(outcome(fn))
        print("refusal %-24s %r" % (name, str(out["refusal__" + name])), flush=True)
        assert str(out["refusal__" + name]), name

    # ---- the fixture is not vacuous ----
    assert any(i["accepted"] >= 10 for i in infos), infos
    assert any(i["undefined_keys"] > 0 and i["accepted"] > 0 and i["defined"] > 0 for i in infos), infos
    assert any(i["stop"] == 1 for i in infos), infos
    assert any(i["stop"] == 2 for i in infos), infos
    for stop in (3, 4):
        print("stop reason %r occurs in: %s" % (STOPS[stop], [i["name"] for i in infos if i["stop"] == stop] or "no case"))
    path = os.path.join(ROOT, "tests", "golden", "background_signals.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
