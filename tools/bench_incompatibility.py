"""Times match_diagnostic's incompatibility loop over signal pairs against the only way to do it before, on
`GAKAGAKC` / `K` at simulate_peptide's defaults (3 mocks imaged + 8 Edmans, 12 frames) and a 10 x 10 x 10 grid of (Edman
efficiency, dye destruction per cycle, dud rate) x 10^5 molecules.  The sweep is made once and not timed.

  kernels   fsq_signal_pair_best + fsq_signal_pair_extremes for the 78 heat-map signals of 12 cycles (3 003 pairs), and for
            the 465 signals of 30 cycles (107 880 pairs; the sweep has 11 cycles, so most of those stand in no dict - what is
            measured is the kernels' cost at that many pairs): device events around the two launches, the inputs on the
            device, median of --reps runs after a warm-up.
  records   incompatibility_records(pairs=False) end to end from sweep_device's tables: the unique keys, the count matrix,
            the key table's upload, the two kernels, the scores to Python.  Wall clock between two synchronisations.
  loop      the parent commit's route: score_records(select_signals={a, b}, contributions=True) + best_point once per pair,
            over --sample pairs spread evenly over the 3 003, wall clock, scaled to 3 003.
Writes profiles/incompatibility_summary.md.

  python tools/bench_incompatibility.py [--grid 10 --molecules 100000 --reps 5 --sample 50 --out FILE]"""
import argparse
import itertools
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequence", default="GAKAGAKC")
    ap.add_argument("--label", default="K")
    ap.add_argument("--grid", type=int, default=10)
    ap.add_argument("--molecules", type=int, default=10 ** 5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=50)
    ap.add_argument("--seed", type=int, default=20241019)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "incompatibility_summary.md"))
    a = ap.parse_args()
    import torch
    from fluorosequencingimageanalysis_amd import _host_signal_sweep as H, signal_sweep as SW
    ddif = [0, 0.3] + [0.3] * 5
    fixed = dict(s=0.3, sc=3, s2=0.1, beta=70000.0, beta_sigma=0.2, ddif=ddif, superdye_rate=0.0, superdye_factor=1.0)
    fit = dict(max_possible=5, allow_multidrop=True, max_deviation=3, quench_factors=ddif)
    mocks, edmans, G, n = 3, 8, a.grid, a.molecules
    points = [(p, -math.log(1.0 - d), u) for p in np.linspace(0.80, 0.98, G).tolist() for d in np.linspace(0.02, 0.20, G).tolist()
              for u in np.linspace(0.05, 0.50, G).tolist()]
    sweep = SW.sweep_device(a.sequence, a.label, mocks, edmans, points, n, seed=a.seed, **fit, **fixed)
    observed = SW.records_of_sweep(sweep)["all_simulations"][points[len(points) // 2]][0]
    kw = dict(metric='my_euclidean', heatmap_normalize_counts=True)
    med = lambda v: float(np.median(v))                                                  # noqa: E731
    rng = lambda v: "%.3g (%.3g-%.3g)" % (med(v), min(v), max(v))                        # noqa: E731

    # the two kernels, inputs on the device
    signals, d_fit, d_total = SW._counts_on_device(observed, sweep, False, None)
    table = H.key_table(observed, signals)
    kernels = {}
    for cycles in (12, 30):
        L = list(SW.split_heatmap(cycles, 0)[1])
        rows = SW._candidate_rows(signals, L)
        spans = []
        real = SW._engine.launch

        def timed(fn, what, dev, *args):
            if not what.startswith("fsq_signal_pair"):
                return real(fn, what, dev, *args)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            real(fn, what, dev, *args)
            t1.record()
            spans.append((what, t0, t1))
        SW._engine.launch = timed
        try:
            for _ in range(a.reps + 1):
                out = SW.pair_best_device(table, rows, d_fit, d_total, 'my_euclidean', H.HEATMAP_NORMALIZE_COUNTS, None, False)
                SW.pair_extremes_device(out["dist"], len(L), False)
            torch.cuda.synchronize()
        finally:
            SW._engine.launch = real
        per = {}
        for what, t0, t1 in spans[2:]:                                                   # (the first run of each is the warm-up)
            per.setdefault(what, []).append(t0.elapsed_time(t1))
        kernels[cycles] = (len(L), len(L) * (len(L) - 1) // 2, int((rows >= 0).sum()), per)

    # end to end
    SW.incompatibility_records(observed, sweep, num_cycles=12, pairs=False, **kw)
    records = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        rec = SW.incompatibility_records(observed, sweep, num_cycles=12, pairs=False, **kw)
        torch.cuda.synchronize()
        records.append((time.perf_counter() - t) * 1e3)

    # the parent's route over a sample of the pairs
    L = list(SW.split_heatmap(12, 0)[1])
    pairs = list(itertools.combinations(L, 2))
    sample = [pairs[i] for i in np.linspace(0, len(pairs) - 1, a.sample).astype(int).tolist()]

    def loop_once(some):
        out = {}
        for ss1, ss2 in some:
            scores = SW.score_records(observed, sweep, select_signals={ss1, ss2}, on_error='none', **kw)
            try:
                point, _, factor, contrib = SW.best_point(scores)
                out[(ss1, ss2)] = (point, (contrib.get(ss1), contrib.get(ss2)), factor)
            except ValueError:
                out[(ss1, ss2)] = (None, (None, None), None)
        return out
    loop_once(sample[:3])
    torch.cuda.synchronize()
    t = time.perf_counter()
    looped = loop_once(sample)
    torch.cuda.synchronize()
    loop_ms = (time.perf_counter() - t) * 1e3
    full = SW.incompatibility_records(observed, sweep, num_cycles=12, **kw)
    assert all(full["pairs"][p] == v for p, v in looped.items()) and full["scores"] == rec["scores"]
    scaled = loop_ms * len(pairs) / len(sample)

    S, P = (int(x) for x in d_fit.shape)
    lines = ["# Incompatibility scores of signal pairs (`tools/bench_incompatibility.py`)", "",
             "`%s`, label `%s`, %d mocks + %d Edmans (%d frames), a %d x %d x %d grid x %d molecules (the sweep of" %
             (a.sequence, a.label, mocks, edmans, mocks + edmans + 1, G, G, G, n),
             "`profiles/signal_sweep_summary.md`, made once and not timed): a count matrix of %d keys x %d points.  `my_euclidean`," % (S, P),
             "`heatmap_normalize_counts`.  One session on one %s; median (min-max) of %d runs after a warm-up." %
             (torch.cuda.get_device_name(0), a.reps), "",
             "| what | signals | pairs | ms |", "|---|---|---|---|"]
    for cycles, (n_sel, K, present, per) in kernels.items():
        for what, v in per.items():
            lines.append("| `%s`, %d cycles (%d of the signals stand in a dict; device events) | %d | %d | %s |" %
                         (what, cycles, present, n_sel, K, rng(v)))
    n_sel, K = kernels[12][:2]
    lines += ["| `incompatibility_records(pairs=False)` end to end, from `sweep_device`'s tables (wall clock) | %d | %d | %s |" %
              (n_sel, K, rng(records)),
              "| the parent's route: `score_records(select_signals={a, b})` + `best_point` per pair, %d pairs timed (wall clock) | %d | %d | %.0f |" %
              (len(sample), n_sel, len(sample), loop_ms),
              "| the same scaled to all pairs (x %d / %d) | %d | %d | %.0f |" % (len(pairs), len(sample), n_sel, K, scaled), "",
              "The per-pair loop, scaled, takes %.0f times as long as `incompatibility_records`; its %d sampled pairs give the same"
              % (scaled / med(records), len(sample)),
              "(point, distances, factor) as the kernels.", ""]
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
