"""Writes tests/golden/lognormal_upsteps.npz: seeded tracks through the reference's _intensities_to_signal_lognormal_v8 with
allow_upsteps=True (itertools.product: every sequence of counts, (max_possible + 1)^T of them).

Loads the reference at run time as tools/gen_lognormal_golden.py does: through oracle/refload.py, with numpy's AVX-512 paths
disabled (scipy's norm.pdf then equals the closed form with glibc's exp).

181 tracks: T = 1 .. 6, max_possible 1 / 3 / 5 (5 only up to T = 5, which keeps a track under about a second of the
reference), multi-drop on and off, max_deviation 3 / 0.5 / 1e9, intensities whose counts rise so that the winner steps up,
ON-prefix tracks, broken categories (ON after OFF), non-positive intensities, all-underflow ties and densities that are
subnormal doubles.

The generator asserts that the set is not vacuous: at least 30 winners with an upstep (signal None with a best_seq), at least 20
tracks without any sequence, at least 5 ties decided by order, and no more than 60 % of the tracks in any one of these groups.

  python tools/gen_lognormal_dp_golden.py [--reference DIR]
"""
import argparse
import itertools
import math
import os
import subprocess
import sys
import time

NPY_ENV = "AVX512F AVX512CD AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR"
if __name__ == "__main__" and os.environ.get("NPY_DISABLE_CPU_FEATURES") != NPY_ENV:
    os.environ["NPY_DISABLE_CPU_FEATURES"] = NPY_ENV
    sys.exit(subprocess.call([sys.executable] + sys.argv))         # a fresh child: numpy reads the variable at import

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
MAX_MEANS = 17


def cases():
    """(name, intensities, categories, means, beta_sigma, max_possible, allow_multidrop, max_deviation)"""
    from gen_lognormal_golden import means_for
    rng = np.random.default_rng(20250118)
    out = []
    shapes = [(T, m) for m in (1, 3) for T in range(1, 7)] + [(T, 5) for T in range(1, 6)]
    for T, m in shapes:
        for multi in (True, False):
            if not multi and T == 1:
                continue                            # (the reference's max() of an empty list)
            for dev in (3, 0.5, 1e9):
                for rep in range(2 if T >= 3 else 1):
                    beta = float(rng.choice([9000.0, 12000.0, 20000.5]))
                    sigma = float(rng.choice([0.2, 0.15, 0.3]))
                    means = means_for(beta, m)
                    rising = rng.random() < 0.7
                    v, seq = int(rng.integers(0 if rising else 1, m + 1)), []
                    for f in range(T):
                        seq.append(v)
                        if rising:
                            v = int(np.clip(v + rng.choice([-1, 0, 1, 1, 2]), 0, m))
                        elif v > 0 and rng.random() < 0.35:
                            v -= 1
                    noise = sigma * float(rng.choice([0.5, 1.0, 1.6]))
                    inten = [math.exp(rng.normal(means[s - 1], noise)) if s > 0 else rng.normal(40.0, 300.0) for s in seq]
                    cat = [s > 0 for s in seq]
                    name = "rising" if rising else "prefix"
                    kind = int(rng.integers(0, 10))
                    if kind == 0 and T > 2:
                        cat = list(cat)
                        cat[-1], cat[-2], name = True, False, "on_after_off"
                    elif kind == 1:
                        k = int(rng.integers(0, T))
                        inten[k], name = -abs(inten[k]) if rng.random() < 0.5 else 0.0, "nonpositive"
                    elif kind == 2:
                        cat, name = [True] * T, "all_on"
                    if rep == 0:
                        inten = [int(round(x)) for x in inten]
                    else:
                        alpha = 37.25 + float(rng.random())
                        inten = [int(round(x)) - alpha for x in inten]
                    out.append((name, inten, cat, means, sigma, m, multi, dev))
    # all-underflow ties: every density is 0, the first surviving sequence wins by order
    for T, m, multi in ((2, 3, True), (3, 5, True), (4, 3, False), (5, 3, True), (6, 1, True), (3, 3, False), (4, 5, True), (2, 1, True)):
        out.append(("underflow", [1] * T, [True] * T, means_for(10000.0, m), 0.2, m, multi, 1e9))
    # densities that are subnormal doubles: exp() of -745 .. -708
    for vals in ([5], [5.2], [4.8], [4.5], [5, 5], [4.5, 10000], [10000, 4.5, 20000]):
        for m in (1, 3):
            out.append(("subnormal", vals, [True] * len(vals), means_for(10000.0, m), 0.2, m, True, 1e9))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("FSQ_REFERENCE"), help="the reference's directory (default: oracle/refload.py's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lognormal_upsteps.npz"))
    a = ap.parse_args()
    if a.reference:
        os.environ["FSQ_REFERENCE"] = a.reference
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, ROOT)
    import refload
    from gen_lognormal_golden import load_mcsimlib
    if a.reference:
        refload.REF = a.reference
    refload.load_reference()
    mc = load_mcsimlib(refload)
    from fluorosequencingimageanalysis_amd import _host_lognormal as R

    keys = ("T", "max_possible", "multidrop", "has_seq", "is_zero", "start", "tie", "upstep", "n_surviving")
    meta = {k: [] for k in keys}
    names, sig, dev, sigma, score, means, cat_bits, inten, seqs, fscores, off = [], [], [], [], [], [], [], [], [], [], [0]
    t0 = time.time()
    worst = 0.0
    all_cases = cases()
    for name, I, cat, mn, sg, m, multi, dv in all_cases:
        T = len(I)
        t1 = time.time()
        r = mc._intensities_to_signal_lognormal_v8(list(I), 1.0, sg, max_possible=m, allow_multidrop=multi, allow_upsteps=True,
                                                   max_deviation=dv, quench_factor=0, categories=tuple(cat), log_fluor_means=list(mn))
        worst = max(worst, time.time() - t1)
        signal, is_zero, best_seq, lmii, best_score, best_scores, start = r
        assert lmii == m
        # the survivors' totals, for the count and the tie flag (the restatement's tables; the recorded outputs are the reference's)
        ok, sc = R.tables(I, cat, mn, sg, m, dv)
        totals = []
        for seq in itertools.product(range(m, -1, -1), repeat=T):
            if all(ok[f][v] for f, v in enumerate(seq)) and (multi or all(p - q <= 1 for p, q in zip(seq, seq[1:]))):
                prod = 1.0
                for f, v in enumerate(seq):
                    prod = prod * sc[f][v]
                totals.append(prod)
        assert (len(totals) == 0) == (best_seq is None)
        tie = upstep = False
        if best_seq is not None:
            assert max(totals) == best_score
            tie = sum(1 for x in totals if x == best_score) > 1
            upstep = any(q > p for p, q in zip(best_seq, best_seq[1:]))
            assert upstep == (signal is None)
        names.append(name)
        for k, val in zip(keys, (T, m, int(multi), int(best_seq is not None), -1 if is_zero is None else int(is_zero),
                                 -1 if start is None else start, int(tie), int(upstep), len(totals))):
            meta[k].append(val)
        sig.append(str(signal)); dev.append(float(dv)); sigma.append(sg); score.append(float(best_score))
        means.append(list(mn) + [0.0] * (MAX_MEANS - len(mn)))
        cat_bits.append(sum(1 << f for f, c in enumerate(cat) if c))
        inten.extend(float(x) for x in I)
        seqs.extend(best_seq if best_seq is not None else [0] * T)
        fscores.extend(best_scores if best_seq is not None else [0.0] * T)
        off.append(len(inten))
    n = len(all_cases)
    none, ties, ups = n - sum(meta["has_seq"]), sum(meta["tie"]), sum(meta["upstep"])
    print("%d cases in %.1f s (the slowest %.2f s): %d winners with an upstep, %d without a sequence, %d ties" %
          (n, time.time() - t0, worst, ups, none, ties))
    assert ups >= 30 and none >= 20 and ties >= 5, (ups, none, ties)
    assert max(ups, none, ties) <= 0.6 * n, (ups, none, ties, n)
    n_subnormal = sum(1 for x in fscores if 0.0 < x < 2.2250738585072014e-308)
    assert n_subnormal >= 5, n_subnormal
    assert any(s == 0.0 and t for s, t in zip(score, meta["tie"]))                       # the all-underflow tie
    out = {k: np.array(v, dtype=np.int64) for k, v in meta.items()}
    out.update(name=np.array(names), signal=np.array(sig), max_deviation=np.array(dev), beta_sigma=np.array(sigma),
               best_score=np.array(score), means=np.array(means), category=np.array(cat_bits, dtype=np.uint64),
               intensity=np.array(inten), best_seq=np.array(seqs, dtype=np.uint8), frame_score=np.array(fscores),
               off=np.array(off, dtype=np.int64))
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
