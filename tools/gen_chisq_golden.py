"""Writes tests/golden/chisq_traces.npz: seeded traces through the reference's chi_squared_step_fitter, filter_upsteps,
filter_small_steps and stepfit_r_squared.

Loads the reference at run time through oracle/refload.py, with numpy's AVX-512 paths disabled as oracle/gen_golden.py does.
Per fit case the fixture holds the trace, the parameters, the returned fit and - recorded by wrapping _fit_steps - the best-fit
residual sum, the counter-fit residual sum, the counter-fit plateau count and S of every plateau count tried.  Merge-filter
and R^2 cases run on recorded fits and on hand-made plateau lists.

The generator asserts three properties of its own fixture, so that the tests cannot pass vacuously: at least 20 recorded
residual sums change when `** 2` is replaced by a plain multiply, at least 5 cases tie under each of the two tie rules
(`<=` inside a plateau, `<` across plateaus), and at least 5 cases have a counter-fit count different from p + 1.

  python tools/gen_chisq_golden.py [--reference DIR]

--limits writes tests/golden/chisq_limits.npz instead: the cases of tests/_chisq_limit_cases.recorded_cases() through the
reference, recorded the same way (fit and per-p records), in about three minutes.  Reference-recorded are every extreme-scale
case (1e-165 .. 1e154, the 2^52 and 1e15 offsets, the -0.0 / +0.0 mixes, each with num_steps 5 and None), the reduced long
cases (LONG_CASES_RECORDED: 300 frames with 31 and 37 fits, 130 frames with 31 plateaus, the pairwise split lengths 129 / 136 /
257 with num_steps 8) and the full-size long cases of RECORDED_FULL (300 frames with 105 fits, 130 frames with 129 plateaus,
520 frames, 1 024 frames with num_steps 80).  The reference is pure Python without caching; the other full-size cases of
LONG_CASES (1 024 frames with 104 fits and counter-fits of 104 plateaus, 700 and 1 023 frames) are carried by the restatement,
which tests/test_chisq_limits_host.py pins to these records.

  python tools/gen_chisq_golden.py --limits [--reference DIR]
"""
import argparse
import os
import subprocess
import sys

NPY_ENV = "AVX512F AVX512CD AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR"
if __name__ == "__main__" and os.environ.get("NPY_DISABLE_CPU_FEATURES") != NPY_ENV:
    os.environ["NPY_DISABLE_CPU_FEATURES"] = NPY_ENV
    sys.exit(subprocess.call([sys.executable] + sys.argv))         # a fresh child: numpy reads the variable at import

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_stepfit_golden import synth_trace


def unrounded_trace(seed, n):
    """Full-mantissa values on four levels: the sum of such doubles depends on the order of the additions."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.integers(n // 8, n - n // 8, 3))
    i = np.arange(n)
    level = 3.0 - (i >= cuts[0]) - (i >= cuts[1]) - (i >= cuts[2])
    return level * 20000.0 + 5000.0 + rng.normal(0.0, 2500.0, n)


def staircase(seed, n):
    """Exact half-integer plateaus without noise: residual 0, S = 1e10 ties and equal split values all occur."""
    rng = np.random.default_rng(seed)
    v = np.zeros(n)
    k = int(rng.integers(2, 5))
    cuts = np.sort(rng.choice(np.arange(2, n - 1), k, replace=False))
    level = float(rng.integers(4, 9))
    prev = 0
    for c in list(cuts) + [n]:
        v[prev:c] = level
        level -= float(rng.integers(1, 4)) * 0.5
        prev = c
    return v


def fit_cases():
    """(name, trace, num_steps, multiplier, min_step_length, min_step_magnitude, ignore_counterfits, probe_ties)"""
    rng = np.random.default_rng(2024)
    cases = []
    for n in range(3, 9):
        v = synth_trace(np.random.default_rng(100 + n), n, "half")
        cases.append(("short", v, 1, 1, 0, 0.0, False, True))
        cases.append(("short", v, None, 1, 2, 0.0, False, True))
        cases.append(("short", v, None, 0.5, 0, 0.0, True, True))
    v50 = [synth_trace(np.random.default_rng(200 + k), 50, "int" if k % 2 else "half") for k in range(4)]
    for k, ns in enumerate((1, 3, 10, None)):
        for L in (0, 2, 5):
            cases.append(("n50", v50[k], ns, 1, L, 0.0, False, False))
    cases.append(("n50", v50[0], None, 0.3, 2, 0.0, True, False))
    cases.append(("n50", v50[1], 10, 1, 2, 8000.0, False, False))
    cases.append(("n50", v50[2], 10, 1, 2, 8000.0, True, False))
    cases.append(("n64", synth_trace(np.random.default_rng(264), 64, "int"), None, 1, 2, 0.0, False, False))
    v200 = [synth_trace(np.random.default_rng(300 + k), 200, "int" if k % 2 else "half") for k in range(3)]
    cases.append(("n200", v200[0], 3, 1, 2, 0.0, False, False))
    cases.append(("n200", v200[1], 10, 1, 2, 0.0, False, False))
    cases.append(("n200", v200[2], 10, 1, 5, 6000.0, False, False))
    cases.append(("n200", v200[0], 10, 1, 0, 0.0, True, False))
    cases.append(("n200u", unrounded_trace(31, 200), 10, 1, 2, 0.0, False, False))
    cases.append(("n512", synth_trace(np.random.default_rng(512), 512, "int"), 3, 1, 2, 0.0, False, False))
    cases.append(("n1023u", unrounded_trace(1023, 1023), 3, 1, 2, 0.0, False, False))
    cases.append(("n1024u", unrounded_trace(1024, 1024), 3, 1, 2, 0.0, False, False))
    cases.append(("flat", np.full(12, 5.0), None, 1, 2, 0.0, False, True))
    cases.append(("flat", np.full(12, 5.0), 3, 1, 0, 0.0, False, True))
    cases.append(("flat", np.full(9, 0.1), None, 1, 0, 0.0, False, True))
    cases.append(("flat", np.full(30, -7.3), 5, 1, 2, 0.0, True, True))
    for k, n in enumerate((12, 16, 24, 24, 40, 40, 20, 28, 32, 36)):
        v = staircase(400 + k, n)
        cases.append(("stair", v, None if k % 2 else min(8, n - 3), 1, 2 if k % 3 == 1 else 0, 0.0, bool(k % 2 and k > 2), True))
    del rng
    return cases


def record_limits(sf, out_path):
    """tests/golden/chisq_limits.npz: fit and per-p records of tests/_chisq_limit_cases.recorded_cases()."""
    import time
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _chisq_limit_cases as CL
    log = []
    real_fit_steps = sf._fit_steps

    def fit_steps_rec(*args, **kw):
        r = real_fit_steps(*args, **kw)
        log.append((kw.get("bestfit_plateaus") is not None, list(r)))
        return r
    sf._fit_steps = fit_steps_rec
    meta = {k: [] for k in ("len", "num_steps", "mult", "L")}
    names, lum_flat, lum_off, fit_rows, rec_rows = [], [], [0], [], []
    t_all = time.time()
    for ci, (name, v, ns, mult, L) in enumerate(CL.recorded_cases()):
        lum = [float(x) for x in v]
        del log[:]
        t0 = time.time()
        with np.errstate(all="ignore"):
            fit = sf.chi_squared_step_fitter(lum, num_steps_multiplier=mult, num_steps=ns, min_step_length=L)
            k = p = 0
            while k + 1 < len(log):
                assert not log[k][0] and log[k + 1][0]
                best, counter = log[k][1], log[k + 1][1]
                p += 1
                assert len(best) == p
                br = np.float64(sf._plateaus_squared_residuals(lum, best))
                cr = np.float64(sf._plateaus_squared_residuals(lum, counter))
                rec_rows.append((ci, float(br), float(cr), len(counter), float(cr / br) if br != 0 else 1e10))
                k += 2
        names.append(name)
        meta["len"].append(len(lum)); meta["num_steps"].append(0 if ns is None else ns); meta["mult"].append(mult); meta["L"].append(L)
        lum_flat.extend(lum); lum_off.append(len(lum_flat))
        fit_rows += [(ci, s, o, float(h)) for s, o, h in fit]
        print("case %d %s: n=%d num_steps=%s mult=%g L=%d -> %d plateaus, %d fits tried, %.1f s" %
              (ci, name, len(lum), ns, mult, L, len(fit), p, time.time() - t0), flush=True)
    sf._fit_steps = real_fit_steps
    out = {"case_name": np.array(names), "lum": np.array(lum_flat), "lum_off": np.array(lum_off, dtype=np.int64)}
    for k, v in meta.items():
        out["case_" + k] = np.array(v, dtype=np.float64 if k == "mult" else np.int64)
    for pre, rows, cols in (("fit", fit_rows, (("case", True), ("start", True), ("stop", True), ("h", False))),
                            ("rec", rec_rows, (("case", True), ("best", False), ("counter", False), ("counter_n", True), ("S", False)))):
        for j, (c, integer) in enumerate(cols):
            col = np.array([r[j] for r in rows], dtype=np.float64)
            out[pre + "_" + c] = col.astype(np.int64) if integer else col
    np.savez_compressed(out_path, **out)
    print("wrote", out_path, os.path.getsize(out_path), "bytes, %.0f s" % (time.time() - t_all))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("FSQ_REFERENCE", "/root/reference"))
    ap.add_argument("--limits", action="store_true", help="write tests/golden/chisq_limits.npz instead")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "tests", "golden", "chisq_limits.npz" if a.limits else "chisq_traces.npz")
    os.environ["FSQ_REFERENCE"] = a.reference
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import refload
    refload.REF = a.reference
    refload.load_reference()
    sf = refload.load("stepfitting_library", "stepfitting_library.py")
    if a.limits:
        return record_limits(sf, a.out)

    log = []                 # (is_counter, fit) of every _fit_steps call
    ties = {"within": False, "across": False}
    state = {"probe": False, "totals": None}
    real_fit_steps, real_split, real_best = sf._fit_steps, sf._split_plateau, sf._best_split

    def fit_steps_rec(*args, **kw):
        r = real_fit_steps(*args, **kw)
        log.append((kw.get("bestfit_plateaus") is not None, list(r)))
        return r

    def split_rec(luminosities, plateau, forbidden_splits=None, min_step_magnitude=5000):
        r = real_split(luminosities=luminosities, plateau=plateau, forbidden_splits=forbidden_splits,
                       min_step_magnitude=min_step_magnitude)
        if state["probe"] and r[0] is not None:
            state["totals"].append(r[4])
            forb = set(forbidden_splits or ())
            start, stop, _ = plateau
            same = 0
            for s in range(start, stop):
                if (s, s + 1) in forb:
                    continue
                lp, rp = sf._fit_plateau(luminosities, start, s), sf._fit_plateau(luminosities, s + 1, stop)
                if abs(lp[2] - rp[2]) < min_step_magnitude:
                    continue
                tot = sf._plateau_squared_residuals(luminosities, lp) + sf._plateau_squared_residuals(luminosities, rp)
                same += tot == r[4]
            if same > 1:
                ties["within"] = True
        return r

    def best_rec(*args, **kw):
        state["totals"] = []
        r = real_best(*args, **kw)
        t = state["totals"]
        if state["probe"] and r is not None and len(t) > 1 and sum(1 for x in t if x == min(t)) > 1:
            ties["across"] = True
        return r
    sf._fit_steps, sf._split_plateau, sf._best_split = fit_steps_rec, split_rec, best_rec

    def mul_residuals(lum, plateaus):
        tot = 0
        for s, o, h in plateaus:
            tot = tot + sum([(x - h) * (x - h) for x in lum[s:o + 1]])
        return tot

    cases = fit_cases()
    # short full-mantissa traces whose recorded residual sums change when `** 2` becomes a multiply: glibc's pow(x, 2.0)
    # differs from x * x for about one value in a thousand, and a sum of a few terms of one size keeps that last bit
    sens_total, seed = 0, 0
    while sens_total < 24:
        assert seed < 100000, "no pow-sensitive short traces found"
        rng = np.random.default_rng(50000 + seed)
        n = 5 + seed % 4
        v = (rng.integers(0, 3, n) * 4000.0 + rng.normal(0.0, 3000.0, n)).tolist()
        del log[:]
        sf.chi_squared_step_fitter(v, num_steps=None, min_step_length=0)
        k = sum(int(float(sf._plateaus_squared_residuals(v, f)) != float(mul_residuals(v, f))) for _, f in log[:len(log) // 2 * 2])
        if k:
            cases.append(("powsens", np.array(v), None, 1, 0, 0.0, False, False))
            sens_total += k
        seed += 1
    print("%d pow-sensitive short traces from %d seeds" % (sum(1 for c in cases if c[0] == "powsens"), seed))
    meta = {k: [] for k in ("len", "num_steps", "mult", "L", "mag", "ignore", "tie_within", "tie_across")}
    names = []
    lum_flat, lum_off = [], [0]
    fit_rows, rec_rows = [], []
    fits_by_case = []
    n_pow_sensitive = n_counter_short = 0
    for ci, (name, v, ns, mult, L, mag, ign, probe) in enumerate(cases):
        lum = [float(x) for x in v]
        del log[:]
        ties["within"] = ties["across"] = False
        state["probe"] = probe
        fit = sf.chi_squared_step_fitter(lum, num_steps_multiplier=mult, num_steps=ns, min_step_length=L,
                                         min_step_magnitude=mag, ignore_counterfits=ign)
        state["probe"] = False
        k, p, short = 0, 0, False
        while k + 1 < len(log):
            assert not log[k][0] and log[k + 1][0]
            best, counter = log[k][1], log[k + 1][1]
            p += 1
            assert len(best) == p
            br = sf._plateaus_squared_residuals(lum, best)
            cr = sf._plateaus_squared_residuals(lum, counter)
            S = float(cr) / float(br) if float(br) != 0 else 10 ** 10
            rec_rows.append((ci, float(br), float(cr), len(counter), float(S)))
            n_pow_sensitive += int(float(br) != float(mul_residuals(lum, best))) + int(float(cr) != float(mul_residuals(lum, counter)))
            short |= len(counter) != p + 1
            k += 2
        n_counter_short += int(short)
        names.append(name)
        meta["len"].append(len(lum)); meta["num_steps"].append(0 if ns is None else ns); meta["mult"].append(mult)
        meta["L"].append(L); meta["mag"].append(mag); meta["ignore"].append(int(ign))
        meta["tie_within"].append(int(ties["within"])); meta["tie_across"].append(int(ties["across"]))
        lum_flat.extend(lum); lum_off.append(len(lum_flat))
        fit_rows += [(ci, s, o, float(h)) for s, o, h in fit]
        fits_by_case.append([(int(s), int(o), float(h)) for s, o, h in fit])
        print("case %d %s: n=%d num_steps=%s L=%d mag=%g ignore=%d -> %d plateaus, %d fits tried, ties %d/%d" %
              (ci, name, len(lum), ns, L, mag, ign, len(fit), p, ties["within"], ties["across"]), flush=True)
    sf._fit_steps, sf._split_plateau, sf._best_split = real_fit_steps, real_split, real_best
    assert n_pow_sensitive >= 20, n_pow_sensitive
    assert sum(meta["tie_within"]) >= 5 and sum(meta["tie_across"]) >= 5, (sum(meta["tie_within"]), sum(meta["tie_across"]))
    assert n_counter_short >= 5, n_counter_short
    print("pow-sensitive residual sums: %d; tie cases within / across: %d / %d; cases with a short counter-fit: %d" %
          (n_pow_sensitive, sum(meta["tie_within"]), sum(meta["tie_across"]), n_counter_short))

    # ---- merge filters and R^2: (fit case of the luminosities, plateaus in, mode, min_magnitude, min_noise_ratio) ----------
    filt = []
    by_name = {}
    for ci, nme in enumerate(names):
        by_name.setdefault(nme, []).append(ci)
    for ci in by_name["n50"][:8] + by_name["n200"] + by_name["n200u"] + by_name["n512"] + by_name["stair"][:2]:
        pl = fits_by_case[ci]
        filt.append((ci, pl, 0, None, None))
        filt.append((ci, pl, 1, None, None))
        filt.append((ci, pl, 1, 9000.0, None))
        filt.append((ci, pl, 1, None, 0.6))
        filt.append((ci, pl, 1, 4000.0, 0.3))
    # hand-made lists on a 50-frame and a 200-frame trace: equal-width plateaus refitted by the reference (many small steps,
    # cascades that merge down to one plateau), and stated heights that are not the means
    for ci, width in ((by_name["n50"][0], 5), (by_name["n50"][3], 2), (by_name["n200"][1], 8), (by_name["n200u"][0], 1)):
        lum = lum_flat[lum_off[ci]:lum_off[ci + 1]]
        n = len(lum)
        pl = sf.refit_plateaus(lum, [(s, min(s + width, n) - 1, 0.0) for s in range(0, n, width)])
        pl = [(s, o, float(h)) for s, o, h in pl]
        filt.append((ci, pl, 0, None, None))
        filt.append((ci, pl, 1, 1e9, None))                       # everything merges: down to one plateau
        filt.append((ci, pl, 1, None, 1e6))
        filt.append((ci, pl, 1, 7000.0, 0.5))
        filt.append((ci, pl, 1, 0.0, 0.0))
        rising = [(s, o, float(k)) for k, (s, o, _) in enumerate(pl)]   # stated heights rise: upsteps cascade
        filt.append((ci, rising, 0, None, None))
        filt.append((ci, rising[1:-1], 1, 2.5, None))             # plateaus that do not cover the whole trace
    f_meta = {k: [] for k in ("case", "mode", "has_mag", "mag", "has_ratio", "ratio", "r2")}
    f_in, f_out = [], []
    n_to_one = 0
    for fi, (ci, pl, mode, mmag, ratio) in enumerate(filt):
        lum = lum_flat[lum_off[ci]:lum_off[ci + 1]]
        if mode == 0:
            out = sf.filter_upsteps(lum, list(pl))
        else:
            out = sf.filter_small_steps(lum, list(pl), min_magnitude=mmag, min_noise_ratio=ratio)
        with np.errstate(all="ignore"):
            r2 = float(sf.stepfit_r_squared(lum, list(pl)))
        n_to_one += int(len(pl) > 2 and len(out) == 1)
        f_meta["case"].append(ci); f_meta["mode"].append(mode); f_meta["has_mag"].append(int(mmag is not None))
        f_meta["mag"].append(0.0 if mmag is None else mmag); f_meta["has_ratio"].append(int(ratio is not None))
        f_meta["ratio"].append(0.0 if ratio is None else ratio); f_meta["r2"].append(r2)
        f_in += [(fi, s, o, float(h)) for s, o, h in pl]
        f_out += [(fi, s, o, float(h)) for s, o, h in out]
    assert n_to_one >= 3, n_to_one
    print("%d filter cases, %d cascade down to one plateau" % (len(filt), n_to_one))

    out = {"case_name": np.array(names)}
    for k, v in meta.items():
        out["case_" + k] = np.array(v, dtype=np.float64 if k in ("mult", "mag") else np.int64)
    out["lum"] = np.array(lum_flat, dtype=np.float64)
    out["lum_off"] = np.array(lum_off, dtype=np.int64)

    def table(pre, rows, cols):
        arr = np.array(rows, dtype=np.float64).reshape(-1, len(cols))
        for j, (c, integer) in enumerate(cols):
            out[pre + "_" + c] = arr[:, j].astype(np.int64) if integer else arr[:, j]
    table("fit", fit_rows, (("case", True), ("start", True), ("stop", True), ("h", False)))
    table("rec", rec_rows, (("case", True), ("best", False), ("counter", False), ("counter_n", True), ("S", False)))
    table("fin", f_in, (("case", True), ("start", True), ("stop", True), ("h", False)))
    table("fout", f_out, (("case", True), ("start", True), ("stop", True), ("h", False)))
    for k, v in f_meta.items():
        out["filt_" + k] = np.array(v, dtype=np.float64 if k in ("mag", "ratio", "r2") else np.int64)
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
