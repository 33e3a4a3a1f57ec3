"""Writes tests/golden/binsearch.npz: the reference's histogram bin search (MCsimlib.optimal_bin_size, :3888-3909) on seeded
value sets, its cost of every bin count and the counts of np.histogram(a, bins=np.linspace(lo, hi, nb + 1)).

Loads the reference at run time through oracle/refload.py exactly as tools/gen_lognormal_golden.py does: numpy's AVX-512
paths disabled, the same stand-ins.

  (a) seeded sets of N = 2, 7, 300 and 5 000 values of two kinds: integer photometries (a normal background plus a lognormal
      population, some negative) and their logs.  Bin counts 1 .. 20, 127 / 128 / 129 / 136, 255 / 256 / 257, 1 023, 4 097,
      8 191 / 8 192 / 8 193, 9 999 and 10 000 for every set, and up to three more per set at which pow(step, 2.0), the
      reference's `bin_size**2`, is not the rounded product step * step.
  (b) on-edge sets: "all integers lo .. hi" with the bin counts at which an edge computed with one fma gives other counts
      than np.linspace's two roundings, and heavy-duplicate sets with many values exactly on inner edges.
  (c) the 10 .. 10 000 search over the raw photometries of the chain CSV that tests/golden/lognormal_tracks.npz holds (its
      argmin is the bin count recorded there), and the 10 .. 1 000 search over that chain's first last_drop_list.

The generator asserts that the fixture is not vacuous, with the contract restated in tests/_binsearch_reference.py: the
restatement equals every recorded number, at least 20 cases change with a fused edge, at least 20 with <= at the inner edges,
at least 5 costs change without np.add.reduce's chunks of 8 192 and at least 5 with step * step in place of pow(step, 2.0).

  python tools/gen_binsearch_golden.py [--reference DIR]
"""
import argparse
import math
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_lognormal_golden import NPY_ENV, load_mcsimlib  # noqa: E402

if __name__ == "__main__" and os.environ.get("NPY_DISABLE_CPU_FEATURES") != NPY_ENV:
    os.environ["NPY_DISABLE_CPU_FEATURES"] = NPY_ENV
    sys.exit(subprocess.call([sys.executable] + sys.argv))         # a fresh child: numpy reads the variable at import

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def seeded_sets(sizes):
    rng = np.random.default_rng(20250310)
    out = []
    for N in sizes:
        bg = rng.normal(100.0, 300.0, N - N // 2)
        pop = np.exp(rng.normal(math.log(10000.0), 0.3, N // 2))
        ints = tuple(int(round(float(x))) for x in np.concatenate([bg, pop]))
        assert min(ints) < max(ints) and (N < 7 or min(ints) < 0)
        out.append(("int_%d" % N, ints))
        logs = tuple(math.log(float(x)) for x in np.exp(rng.normal(math.log(10000.0), 0.35, N)).round())
        assert min(logs) < max(logs)
        out.append(("log_%d" % N, logs))
    return out


def pow_sensitive(raw, but):
    """Up to three bin counts at which libm's pow(step, 2.0), the reference's `bin_size**2`, is not the rounded step * step."""
    span = float(max(raw)) - float(min(raw))
    return [nb for nb in range(21, 10001) if nb not in but and math.pow(span / nb, 2.0) != (span / nb) * (span / nb)][:3]


def on_edge_sets(B):
    """(name, values, bin counts): integer ranges with their fma-sensitive bin counts, and heavy-duplicate sets."""
    out = []
    for lo in range(-5, 6):
        for span in range(3, 60):
            a = np.arange(lo, lo + span + 1, dtype=np.float64)
            nbs = [nb for nb in range(2, 41)
                   if not np.array_equal(B.counts(a, a[0], a[-1], nb, fused=True), B.counts(a, a[0], a[-1], nb))]
            if nbs:
                out.append(("range_%d_%d" % (lo, lo + span), tuple(range(lo, lo + span + 1)), nbs[:3]))
    out = out[::max(1, len(out) // 48)]
    assert len(out) >= 40, len(out)
    if not any(n == "range_-5_-1" for n, _, _ in out):
        out.append(("range_-5_-1", tuple(range(-5, 0)), [20]))
    rng = np.random.default_rng(99)
    out.append(("dup_quarters", tuple(float(x) * 0.25 for x in rng.integers(0, 33, 4000)), [3, 5, 7, 8, 16, 32, 64, 128]))
    out.append(("dup_ints", tuple(int(x) for x in rng.integers(-20, 21, 3000)), [4, 5, 8, 10, 16, 20, 40, 80]))
    out.append(("dup_two", (3,) * 500 + (7,) * 300 + (5,) * 11, [1, 2, 4, 8, 9]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="the reference's directory (default: oracle/refload.py's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "binsearch.npz"))
    a = ap.parse_args()
    if a.reference:
        os.environ["FSQ_REFERENCE"] = a.reference
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import refload
    if a.reference:
        refload.REF = a.reference
    refload.load_reference()
    mc = load_mcsimlib(refload)
    import _binsearch_reference as B
    import _binsearch_cases as C

    sets = [(name, raw, C.FIXED_BIN_COUNTS + pow_sensitive(raw, C.FIXED_BIN_COUNTS)) for name, raw in seeded_sets(C.SEEDED_SIZES)]
    sets += on_edge_sets(B)
    names, is_int, values, set_off = [], [], [], [0]
    case_set, case_nb, case_cost, case_hist, case_off = [], [], [], [], [0]
    for si, (name, raw, nbs) in enumerate(sets):
        names.append(name)
        is_int.append(all(isinstance(x, int) for x in raw))
        values.extend(float(x) for x in raw)
        set_off.append(len(values))
        lo, hi = min(raw), max(raw)
        _, _, cost = mc.optimal_bin_size(raw, np.array(nbs))
        for nb, c in zip(nbs, cost[:, 0].tolist()):
            hist, _ = np.histogram(a=raw, bins=np.linspace(lo, hi, nb + 1))
            assert hist.sum() == len(raw)
            case_set.append(si); case_nb.append(nb); case_cost.append(c)
            case_hist.extend(hist.tolist())
            case_off.append(len(case_hist))
    out = dict(set_name=np.array(names), set_is_int=np.array(is_int), set_values=np.array(values), set_off=np.array(set_off, np.int64),
               case_set=np.array(case_set, np.int32), case_nb=np.array(case_nb, np.int32), case_cost=np.array(case_cost),
               case_hist=np.array(case_hist, np.int32), case_off=np.array(case_off, np.int64))

    # ---- (c) the chain's two searches ----
    g = np.load(os.path.join(ROOT, "tests", "golden", "lognormal_tracks.npz"))
    with tempfile.NamedTemporaryFile("w", suffix=".csv", delete=False) as f:
        f.write(g["b_csv"].tobytes().decode())
    try:
        photometries, _ = mc.read_track_photometries_csv(f.name, head_truncate=0, tail_truncate=0, downstep_filtered=True,
                                                         channels=["ch1"])
    finally:
        os.unlink(f.name)
    tracks = list(mc.unwind_photometries(photometries))
    raw = tuple([i for t in tracks for i in t[5]])
    _, where, cost = mc.optimal_bin_size(raw, np.array(range(10, 10001)))
    assert int(where[0][0]) + 10 == int(g["b_scalars"][5]), (where, g["b_scalars"][5])
    out["full_values"], out["full_cost"] = np.array(raw, dtype=np.float64), cost[:, 0].copy()
    last_drop = [math.log(intens[i]) for t in tracks for cat, intens in [(t[4], t[5])] for i in range(len(intens) - 1)
                 if cat[i] and not cat[i + 1] and intens[i] > 0]
    _, where, cost = mc.optimal_bin_size(last_drop, np.array(range(10, 1001)))
    out["ld_values"], out["ld_cost"], out["ld_n_bins"] = np.array(last_drop), cost[:, 0].copy(), np.int64(int(where[0][0]) + 10)
    print("%d sets, %d cases, %d raw photometries (argmin %d), %d last drops (argmin %d)" %
          (len(sets), len(case_nb), len(raw), int(g["b_scalars"][5]), len(last_drop), int(out["ld_n_bins"])))

    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    assert os.path.getsize(a.out) <= 512 * 1024

    # ---- not vacuous, and the restatement equals every recorded number ----
    C.golden.cache_clear(); C.value_sets.cache_clear(); C.cases.cache_clear()
    vs, cs = C.value_sets(), C.cases()
    for c in cs:
        s = vs[c["set"]]
        assert np.array_equal(B.counts(s["sorted"], s["lo"], s["hi"], c["nb"]), c["hist"]), (s["name"], c["nb"])
        assert B.cost(s["sorted"], s["lo"], s["hi"], c["nb"]) == c["cost"], (s["name"], c["nb"])
    fused, le, chunk, product = C.non_vacuity_counts(cs, vs, C.searches())
    print("change with a fused edge: %d cases, with <= at the inner edges: %d cases, without the 8192 chunking: %d costs, "
          "with step * step for pow(step, 2.0): %d costs" % (fused, le, chunk, product))
    assert fused >= 20 and le >= 20 and chunk >= 5 and product >= 5


if __name__ == "__main__":
    main()
