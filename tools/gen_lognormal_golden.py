"""Writes tests/golden/lognormal_tracks.npz: seeded tracks through the reference's _intensities_to_signal_lognormal_v8, one
synthetic track_photometries CSV through the whole lognormal_fitter_v2 chain, and (x, log x) pairs of this container's libm.

Loads the reference at run time through oracle/refload.py, with numpy's AVX-512 paths disabled as oracle/gen_golden.py does
(scipy's norm.pdf then equals the closed form with glibc's exp).  MCsimlib.py is loaded with sklearn.mixture, sklearn.cluster
and string.letters stood in for (nothing of theirs is called) and Python 2's round(); grab_ON_OFFS, ON_OFF_adjust_photometries and
unwind_photometries are taken out of jupyter_development.py by name, since the module itself needs a notebook.

  (a) single tracks: T = 1 .. 13, max_possible 1 / 3 / 5 / 8 (T <= 8) / 15 (T = 4), multi-drop on and off, max_deviation
      3 / 0.5 / 1e9, integer and alpha-adjusted float intensities, non-positive intensities on ON frames, categories all ON,
      ON-prefix, all OFF, OFF-first and ON-after-OFF, all-underflow ties, equal intensities on every frame, densities that are subnormal doubles, and the error of one frame without
      multi-drop.
  (b) a three-field CSV of about 450 tracks of 8 cycles: alpha, both betas, on_offs, the adjusted intensities, both signals
      tables and all_fit_info.
  (c) about 4 000 (x, log x) pairs.

The generator asserts that (a) is not vacuous: 20 .. 80 % of the cases end without a sequence, at least 5 are ties decided by
order, at least 10 have a winner that differs from the per-frame greedy choice.

  python tools/gen_lognormal_golden.py [--reference DIR]
"""
import argparse
import ast
import ctypes
import math
import os
import subprocess
import sys
import tempfile
import time
import types

NPY_ENV = "AVX512F AVX512CD AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR"
if __name__ == "__main__" and os.environ.get("NPY_DISABLE_CPU_FEATURES") != NPY_ENV:
    os.environ["NPY_DISABLE_CPU_FEATURES"] = NPY_ENV
    sys.exit(subprocess.call([sys.executable] + sys.argv))         # a fresh child: numpy reads the variable at import

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_MEANS = 17


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
    # Python-2 round() (half away from zero) for the CSV reader's int(round(float(...))) (:2550, 2566), as refload gives pflib
    return refload.load("MCsimlib", "MCsimlib.py", inject={"round": lambda x: libm.round(float(x))})


def load_functions(refload, rel, names, namespace):
    """The named top-level functions of a reference file, converted as refload.load converts a module, in `namespace`."""
    if refload._RT is None:
        refload._RT = refload._refactor_tool()
    src = open(os.path.join(refload.REF, rel)).read().expandtabs(8)
    out = str(refload._RT.refactor_string(src if src.endswith("\n") else src + "\n", rel))
    tree = ast.parse(out)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {n.name for n in keep} == set(names), names
    exec(compile(ast.Module(body=keep, type_ignores=[]), os.path.join(refload.REF, rel), "exec"), namespace)
    return namespace


def means_for(beta, max_possible, ddif=0.30):
    q = [0.0] + [ddif] * (max_possible + 1)
    return [math.log(beta) + math.log(i + 1.0) - q[i] for i in range(max_possible + 2)]


def single_cases():
    """(name, intensities, categories, means, beta_sigma, max_possible, allow_multidrop, max_deviation)"""
    rng = np.random.default_rng(20240611)
    cases = []
    shapes = [(T, m) for m in (1, 3, 5) for T in range(1, 14)] + [(T, 8) for T in range(1, 9)] + [(4, 15)]
    for T, m in shapes:
        for multi in (True, False):
            if not multi and T == 1:
                continue                            # (the reference's max() of an empty list: a_t1_error records it)
            for dev in (3, 0.5, 1e9):
                if dev == 1e9 and m == 5 and T > 11 and not multi:
                    continue
                for rep in range(2 if m in (3, 5) else 1):
                    beta = float(rng.choice([9000.0, 12000.0, 20000.5]))
                    sigma = float(rng.choice([0.2, 0.15, 0.3]))
                    means = means_for(beta, m)
                    start = int(rng.integers(1, m + 1))
                    seq, v = [], start
                    for f in range(T):
                        seq.append(v)
                        if v > 0 and rng.random() < 0.35:
                            v -= 1 if (not multi or rng.random() < 0.7) else min(v, 2)
                    noise = sigma * float(rng.choice([0.5, 1.0, 1.6]))
                    inten = []
                    for s in seq:
                        if s > 0:
                            inten.append(math.exp(rng.normal(means[s - 1], noise)))
                        else:
                            inten.append(rng.normal(40.0, 300.0))
                    cat = [s > 0 for s in seq]
                    kind = int(rng.integers(0, 12))
                    name = "prefix"
                    if kind == 0:
                        cat, name = [True] * T, "all_on"
                    elif kind == 1:
                        cat, name = [False] * T, "all_off"
                    elif kind == 2 and T > 1:
                        cat, name = [False] + cat[1:], "off_first"
                    elif kind == 3 and T > 2:
                        cat = list(cat)
                        cat[-1], cat[-2], name = True, False, "on_after_off"
                    elif kind == 4:
                        k = int(rng.integers(0, T))
                        inten[k], name = -abs(inten[k]) if rng.random() < 0.5 else 0.0, "nonpositive"
                    elif kind == 5:
                        inten, name = [inten[0]] * T, "equal"
                    if rep == 0:
                        inten = [int(round(x)) for x in inten]
                    else:
                        alpha = 37.25 + float(rng.random())
                        inten = [int(round(x)) - alpha for x in inten]
                    cases.append((name, inten, cat, means, sigma, m, multi, dev))
    # all-underflow ties: every density is 0, the first surviving sequence wins by order
    for T, m, multi in ((2, 3, True), (3, 5, True), (4, 5, False), (5, 3, True), (6, 5, True), (3, 8, False), (2, 15, True), (7, 1, True)):
        cases.append(("underflow", [1] * T, [True] * T, means_for(10000.0, m), 0.2, m, multi, 1e9))
    # densities that are subnormal doubles: exp() of -745 .. -708, the special-case tail of glibc's exp
    for vals in ([5], [5.2], [4.8], [4.5], [5, 5], [4.5, 10000]):
        for m in (1, 3):
            cases.append(("subnormal", vals, [True] * len(vals), means_for(10000.0, m), 0.2, m, True, 1e9))
    # equal intensities on every frame, all ON, at a mean and between two means
    for T in (2, 5, 9):
        for x in (10000, 14000):
            for multi in (True, False):
                cases.append(("equal", [x] * T, [True] * T, means_for(10000.0, 5), 0.2, 5, multi, 3))
    return cases


def log_inputs():
    rng = np.random.default_rng(77)
    x = [float(i) for i in range(1, 801)] + [float(i) for i in rng.integers(1, 2 ** 31, 600)] + [2.0 ** 31, 2.0 ** 31 - 1]
    x += (1.0 + rng.uniform(-2.0 ** -4, 2.0 ** -4, 700)).tolist()
    x += [1.0 - 2.0 ** -4, np.nextafter(1.0 - 2.0 ** -4, 0.0), 1.0 + 2.0 ** -4, 1.0 + float.fromhex("0x1.09p-4"),
          np.nextafter(1.0 + float.fromhex("0x1.09p-4"), 0.0), np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), 1.0]
    x += [1.0 + s * 2.0 ** -k for k in range(5, 53) for s in (1, -1)]
    x += [2.0 ** k for k in range(-1074, 1024, 4)]
    x += np.frombuffer(rng.integers(1, 2 ** 52, 200).astype(np.uint64).tobytes(), dtype=np.float64).tolist()     # subnormals
    x += [np.finfo(np.float64).max, np.nextafter(np.finfo(np.float64).max, 0.0)] + (np.finfo(np.float64).max * rng.uniform(0.5, 1.0, 48)).tolist()
    bits = rng.integers(0, 2 ** 63, 1000).astype(np.uint64)                                              # positive, full mantissa
    full = np.frombuffer(bits.tobytes(), dtype=np.float64)
    x += full[np.isfinite(full) & (full > 0)].tolist()
    x = np.array(x, dtype=np.float64)
    return x, np.array([math.log(v) for v in x.tolist()], dtype=np.float64)


def chain_csv():
    """The text of a synthetic track_photometries CSV: three fields, about 450 tracks of 8 cycles, one other-channel row, one
    row with an upstep category (dropped by downstep_filtered), values that end in .5 (Python-2 rounding)."""
    rng = np.random.default_rng(4242)
    F = 8
    lines = ["CHANNEL,FIELD,H,W,CATEGORY," + ",".join("FRAME %d" % i for i in range(F))]
    gains = (1.0, 1.12, 0.9)
    n = 0
    for field in range(3):
        for k in range(150):
            start = int(rng.choice([1, 1, 1, 2, 2, 3]))
            seq, v = [], start
            for f in range(F):
                seq.append(v)
                if v > 0 and rng.random() < 0.3:
                    v -= 1
            cyc_gain = [gains[field] * (1.0 + 0.05 * math.sin(f + field)) for f in range(F)]
            vals = []
            for f, s in enumerate(seq):
                if s > 0:
                    mu = math.log(10000.0) + math.log(s) - (0.3 if s > 1 else 0.0)
                    vals.append(120.0 + cyc_gain[f] * math.exp(rng.normal(mu, 0.18)))
                else:
                    vals.append(rng.normal(120.0, 260.0))
            vals = [float(int(x)) + (0.5 if rng.random() < 0.1 else float(rng.integers(0, 4)) / 4) for x in vals]
            cat = tuple(s > 0 for s in seq)
            if k == 17:
                cat = (False,) + cat[1:]
            if k == 23:
                cat = cat[:-2] + (False, True)
            h, w = int(rng.integers(5, 500)), int(rng.integers(5, 500))
            lines.append('ch1,%d,%d,%d,"%s",%s' % (field, h, w, str(cat), ",".join(repr(x) for x in vals)))
            n += 1
            if k == 40:
                lines.append('ch2,%d,%d,%d,"%s",%s' % (field, h, w, str(cat), ",".join(repr(x) for x in vals)))
            if k == 41:
                lines.append('ch1,%d,None,None,"%s",%s' % (field, str(cat), ",".join(repr(x) for x in vals)))
    return "\n".join(lines) + "\n"


def encode_fit_info(all_fit_info, F):
    n = len(all_fit_info)
    o = {"field": np.zeros(n, np.int64), "h": np.zeros(n, np.int64), "w": np.zeros(n, np.int64), "row": np.zeros(n, np.int64),
         "category": np.zeros((n, F), np.bool_), "intensity": np.zeros((n, F)), "has_seq": np.zeros(n, np.bool_),
         "best_seq": np.zeros((n, F), np.uint8), "best_score": np.zeros(n), "frame_score": np.zeros((n, F)),
         "is_zero": np.full(n, -1, np.int64), "start": np.full(n, -1, np.int64), "signal": []}
    for i, (ch, field, h, w, row, cat, inten, signal, is_zero, seq, lmii, score, fscores, start) in enumerate(all_fit_info):
        assert len(inten) == F and ch == "ch1"
        o["field"][i], o["h"][i], o["w"][i], o["row"][i] = field, h, w, row
        o["category"][i], o["intensity"][i] = cat, inten
        o["best_score"][i] = score
        o["signal"].append(str(signal))
        if seq is not None:
            o["has_seq"][i], o["best_seq"][i], o["frame_score"][i] = True, seq, fscores
            o["is_zero"][i], o["start"][i] = int(is_zero), start
    o["signal"] = np.array(o["signal"])
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("FSQ_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lognormal_tracks.npz"))
    a = ap.parse_args()
    os.environ["FSQ_REFERENCE"] = a.reference
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, ROOT)
    import refload
    refload.REF = a.reference
    refload.load_reference()
    mc = load_mcsimlib(refload)
    import itertools
    jd = load_functions(refload, "jupyter_development.py", ("_pairwise", "grab_ON_OFFS", "ON_OFF_adjust_photometries"),
                        {"np": np, "tee": itertools.tee, "izip": zip})
    jd["unwind_photometries"] = mc.unwind_photometries
    from fluorosequencingimageanalysis_amd import _host_lognormal as R
    out = {}

    # ---- (a) single tracks ------------------------------------------------------------------------------------------
    cases = single_cases()
    keys = ("T", "max_possible", "multidrop", "has_seq", "is_zero", "start", "lmii", "tie", "greedy_differs", "n_surviving")
    meta = {k: [] for k in keys}
    names, sig, dev, sigma, score, means, cat_bits, inten, seqs, fscores, off = [], [], [], [], [], [], [], [], [], [], [0]
    t0 = time.time()
    for name, I, cat, mn, sg, m, multi, dv in cases:
        T = len(I)
        r = mc._intensities_to_signal_lognormal_v8(list(I), 1.0, sg, max_possible=m, allow_multidrop=multi, allow_upsteps=False,
                                                   max_deviation=dv, quench_factor=0, categories=tuple(cat), log_fluor_means=list(mn))
        signal, is_zero, best_seq, lmii, best_score, best_scores, start = r
        # the survivors' totals, for the tie and greedy flags (restatement's tables; the recorded outputs are the reference's)
        ok, sc = R.tables(I, cat, mn, sg, m, dv)
        _, _, _, n_surv = R.fit(I, cat, mn, sg, m, multi, dv)
        tie = greedy = False
        if best_seq is not None:
            totals = []

            def walk(f, p, prod):
                if f == T:
                    totals.append(prod)
                    return
                for v in range(p, -1, -1):
                    if ok[f][v] and (multi or f == 0 or p - v <= 1):
                        walk(f + 1, v, prod * sc[f][v])
            walk(0, m, 1.0)
            assert len(totals) == n_surv and max(totals) == best_score
            tie = sum(1 for x in totals if x == best_score) > 1
            g = tuple(max((v for v in range(m + 1) if ok[f][v]), key=lambda v: sc[f][v]) for f in range(T))
            greedy = g != tuple(best_seq)
        names.append(name)
        for k, val in zip(keys, (T, m, int(multi), int(best_seq is not None), -1 if is_zero is None else int(is_zero),
                                 -1 if start is None else start, lmii, int(tie), int(greedy), n_surv)):
            meta[k].append(val)
        sig.append(str(signal)); dev.append(float(dv)); sigma.append(sg); score.append(float(best_score))
        means.append(list(mn) + [0.0] * (MAX_MEANS - len(mn)))
        cat_bits.append(sum(1 << f for f, c in enumerate(cat) if c))
        inten.extend(float(x) for x in I)
        seqs.extend(best_seq if best_seq is not None else [0] * T)
        fscores.extend(best_scores if best_seq is not None else [0.0] * T)
        off.append(len(inten))
    n_cases = len(cases)
    none = n_cases - sum(meta["has_seq"])
    print("(a) %d cases in %.1f s (%.2f ms per track): %d without a sequence, %d ties, %d differ from greedy" %
          (n_cases, time.time() - t0, 1e3 * (time.time() - t0) / n_cases, none, sum(meta["tie"]), sum(meta["greedy_differs"])))
    assert 0.2 * n_cases <= none <= 0.8 * n_cases, (none, n_cases)
    assert sum(meta["tie"]) >= 5 and sum(meta["greedy_differs"]) >= 10
    n_subnormal = sum(1 for x in fscores if 0.0 < x < 2.2250738585072014e-308)
    assert n_subnormal >= 5, n_subnormal
    # one frame without multi-drop: the reference ends in max() of an empty list whatever the category is
    t1_error = []
    for I, cat, m in (([10000], (True,), 1), ([30], (False,), 3), ([9000.5], (True,), 5)):
        try:
            mc._intensities_to_signal_lognormal_v8(list(I), 1.0, 0.2, max_possible=m, allow_multidrop=False, allow_upsteps=False,
                                                   max_deviation=3, quench_factor=0, categories=cat, log_fluor_means=means_for(10000.0, m))
            t1_error.append("")
        except Exception as e:
            t1_error.append(type(e).__name__ + ": " + str(e))
    assert all(x.startswith("ValueError") for x in t1_error), t1_error
    out["a_t1_error"] = np.array(t1_error)
    out.update({"a_" + k: np.array(v, dtype=np.int64) for k, v in meta.items()})
    out.update(a_name=np.array(names), a_signal=np.array(sig), a_max_deviation=np.array(dev), a_beta_sigma=np.array(sigma),
               a_best_score=np.array(score), a_means=np.array(means), a_category=np.array(cat_bits, dtype=np.uint64),
               a_intensity=np.array(inten), a_best_seq=np.array(seqs, dtype=np.uint8), a_frame_score=np.array(fscores),
               a_off=np.array(off, dtype=np.int64))

    # ---- (b) the chain of lognormal_fitter_v2 -----------------------------------------------------------------------
    text = chain_csv()
    with tempfile.NamedTemporaryFile("w", suffix=".csv", delete=False) as f:
        f.write(text)
    try:
        photometries, row_photometries = mc.read_track_photometries_csv(f.name, head_truncate=0, tail_truncate=0,
                                                                        downstep_filtered=True, channels=["ch1"])
    finally:
        os.unlink(f.name)
    unwind = jd["unwind_photometries"]
    raw = tuple([i for ch, field, h, w, cat, intens, row in unwind(photometries) for i in intens])
    t0 = time.time()
    m0 = mc._get_m0Dm1(raw_photometries=raw, optimal_bin_number=None)
    alpha = m0[7]
    t_alpha = time.time() - t0
    adjusted, truncated = {}, {}
    for ch, field, h, w, cat, intens, row in unwind(photometries):
        adjusted.setdefault(ch, {}).setdefault(field, {}).setdefault((h, w), (cat, tuple([i - alpha for i in intens]), row))
        truncated.setdefault(ch, {}).setdefault(field, {}).setdefault((h, w), (cat[0:], intens[0:], row))
    t0 = time.time()
    beta0, beta0_sigma = mc.last_drop_method_v2(photometries=truncated)
    t_beta = time.time() - t0
    ddif = tuple([0.0] + [0.30] * 6)
    kw = dict(beta_sigma=0.20, max_possible=5, allow_upsteps=False, allow_multidrop=True, max_deviation=3, quench_factor=0,
              quench_factors=ddif)
    t0 = time.time()
    fit0 = mc._photometries_lognormal_fit_MP_v8(photometries=adjusted, beta=beta0, **kw)
    t_fit = time.time() - t0
    on_offs = jd["grab_ON_OFFS"](fit0[3], alpha_adjust=0)
    adj = jd["ON_OFF_adjust_photometries"](photometries=photometries, ON_OFFS=on_offs, alpha=alpha)
    beta1, beta1_sigma = mc.last_drop_method_v2(photometries=adj)
    fit1 = mc._photometries_lognormal_fit_MP_v8(photometries=adj, beta=beta1, **kw)
    n_tracks = fit1[1]
    print("(b) %d tracks: alpha %.1f s, beta %.1f s, one batch fit %.1f s (%.2f ms per track on this container's CPUs)" %
          (n_tracks, t_alpha, t_beta, t_fit, 1e3 * t_fit / n_tracks))
    out["b_csv"] = np.frombuffer(text.encode(), dtype=np.uint8)
    out["b_scalars"] = np.array([alpha, beta0, beta0_sigma, beta1, beta1_sigma, float(m0[0])])
    oo = [(c, fld, ion, d) for (c, fld), drops in on_offs.items() for ion, d in drops]
    out["b_on_offs"] = np.array(oo, dtype=np.float64).reshape(-1, 4)
    for pre, fit in (("b_fit0_", fit0), ("b_fit1_", fit1)):
        signals, total, none_count, info = fit
        out[pre + "signal_keys"] = np.array([str(k) for k in signals])
        out[pre + "signal_counts"] = np.array(list(signals.values()), dtype=np.int64)
        out[pre + "counts"] = np.array([total, none_count], dtype=np.int64)
        for k, v in encode_fit_info(info, 8).items():
            out[pre + k] = v

    # ---- (c) log ----------------------------------------------------------------------------------------------------
    out["c_x"], out["c_log"] = log_inputs()
    print("(c) %d log pairs" % len(out["c_x"]))
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
