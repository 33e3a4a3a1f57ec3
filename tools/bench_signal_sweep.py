"""Times a simulation parameter sweep against the only way to do it before: a 10 x 10 x 10 grid of (Edman
efficiency, dye destruction per cycle, dud rate) x 10^5 molecules of `GAKAGAKC` / `K` at simulate_peptide's defaults (3 mocks
imaged + 8 Edmans, 12 frames).

  sweep   signal_sweep.sweep_device over the whole grid, then score_device (my_euclidean against the middle point's own
          signals) and the best point: wall clock between two synchronisations, median of --reps runs after one warm-up run.
          Per kernel: device events around every fsq_peptide_simulate_points, lognormal fit and fsq_signal_tally call of one
          further run, summed; the rest of that run's device time is torch's compaction and bincounts.
  loop    a Python loop of peptide_simulator.simulate_and_fit_records over the same points (simulate, fit, torch.unique, the
          unique rows turned into dicts), wall clock, --loop-reps runs after a warm-up of 20 points.
Writes profiles/signal_sweep_summary.md.

  python tools/bench_signal_sweep.py [--grid 10 --molecules 100000 --reps 3 --loop-reps 1 --out FILE]"""
import argparse
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-reps", type=int, default=1)
    ap.add_argument("--seed", type=int, default=20241019)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "signal_sweep_summary.md"))
    a = ap.parse_args()
    import torch
    from fluorosequencingimageanalysis_amd import lognormal as LN, peptide_simulator as PS, signal_sweep as SW
    ddif = [0, 0.3] + [0.3] * 5
    fixed = dict(s=0.3, sc=3, s2=0.1, beta=70000.0, beta_sigma=0.2, ddif=ddif, superdye_rate=0.0, superdye_factor=1.0)
    fit = dict(max_possible=5, allow_multidrop=True, max_deviation=3, quench_factors=ddif)
    mocks, edmans, G, n = 3, 8, a.grid, a.molecules
    points = [(p, -math.log(1.0 - d), u) for p in np.linspace(0.80, 0.98, G).tolist() for d in np.linspace(0.02, 0.20, G).tolist()
              for u in np.linspace(0.05, 0.50, G).tolist()]
    middle = points[len(points) // 2]

    def sweep_once():
        sweep = SW.sweep_device(a.sequence, a.label, mocks, edmans, points, n, seed=a.seed, **fit, **fixed)
        return sweep

    def score_once(sweep, observed):
        return SW.best_point(SW.score_records(observed, sweep, metric='my_euclidean', heatmap_only=False, zero_only=False,
                                              allow_multidrop=True, contributions=False))

    sweep = sweep_once()                                                                 # warm-up: allocator, code objects
    observed = SW.records_of_sweep(sweep)["all_simulations"][middle][0]
    signals_per_point = float((sweep["signals"]["keys"] != 0x400).sum()) / len(points)
    del sweep
    whole, scoring = [], []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        sweep = sweep_once()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        best = score_once(sweep, observed)
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - t) * 1e3)
        scoring.append((time.perf_counter() - t1) * 1e3)
        del sweep
    assert best[0] == middle and best[1] == 0.0, best

    # one more run with device events around the three entries
    spans = {"fsq_peptide_simulate_points": [], "lognormal fit": [], "fsq_signal_tally": []}

    def timed(name, fn):
        def wrapper(*args, **kw):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = fn(*args, **kw)
            t1.record()
            spans[name].append((t0, t1))
            return out
        return wrapper
    real = SW.simulate_points_device, LN.lognormal_device, SW.tally_device
    SW.simulate_points_device = timed("fsq_peptide_simulate_points", real[0])
    LN.lognormal_device = timed("lognormal fit", real[1])
    SW.tally_device = timed("fsq_signal_tally", real[2])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    try:
        torch.cuda.synchronize()
        e0.record()
        sweep = sweep_once()
        e1.record()
        torch.cuda.synchronize()
    finally:
        SW.simulate_points_device, LN.lognormal_device, SW.tally_device = real
    device_ms = e0.elapsed_time(e1)
    kernel_ms = {k: sum(t0.elapsed_time(t1) for t0, t1 in v) for k, v in spans.items()}
    calls = {k: len(v) for k, v in spans.items()}
    del sweep

    def loop_once(pts):
        out = {}
        for p, b, u in pts:
            r = PS.simulate_and_fit_records(a.sequence, a.label, mocks, edmans, n, seed=a.seed, p=p, b=b, u=u, **fit, **fixed)
            out[(p, b, u)] = (r["signals"], r["molecular_error_signals"])
        return out
    loop_once(points[:20])
    loop = []
    for _ in range(a.loop_reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        sims = loop_once(points)
        torch.cuda.synchronize()
        loop.append((time.perf_counter() - t) * 1e3)
    assert sims[middle][0] == observed

    med = lambda v: float(np.median(v))                                                  # noqa: E731
    rng = lambda v: "%.0f (%.0f-%.0f)" % (med(v), min(v), max(v))                        # noqa: E731
    rest = device_ms - sum(kernel_ms.values())
    lines = ["# Simulation parameter sweep (`tools/bench_signal_sweep.py`)", "",
             "`%s`, label `%s`, %d mocks + %d Edmans (%d frames), a %d x %d x %d grid of (Edman efficiency 0.80-0.98, dye destruction" %
             (a.sequence, a.label, mocks, edmans, mocks + edmans + 1, G, G, G),
             "per cycle 0.02-0.20, dud rate 0.05-0.50) x %d molecules, common random numbers, seed %d; one session on one %s." %
             (n, a.seed, torch.cuda.get_device_name(0)),
             "Wall clock between two synchronisations, median (min-max).  %.0f distinct fitted signals per point on average." % signals_per_point, "",
             "| route | runs | ms | points/s | molecules/s |", "|---|---|---|---|---|",
             "| sweep: `sweep_device` + `score_records` + `best_point` | %d | %s | %.3g | %.3g |" %
             (a.reps, rng(whole), len(points) / med(whole) * 1e3, len(points) * n / med(whole) * 1e3),
             "| of which scoring (`score_records`: unique keys, lookup, scores, 1 000 results to Python) | %d | %s | | |" % (a.reps, rng(scoring)),
             "| loop: `simulate_and_fit_records` per point (the parent's route; no scoring) | %d | %s | %.3g | %.3g |" %
             (a.loop_reps, rng(loop), len(points) / med(loop) * 1e3, len(points) * n / med(loop) * 1e3), "",
             "The loop takes %.2f times as long as the sweep." % (med(loop) / med(whole)), "",
             "One further run of `sweep_device` with device events around its entries (%.0f ms of device time from the first launch to the last):" % device_ms, "",
             "| stage | calls | ms | share |", "|---|---|---|---|"]
    for k, v in kernel_ms.items():
        lines.append("| %s | %d | %.1f | %.1f %% |" % (k, calls[k], v, 100.0 * v / device_ms))
    lines += ["| the rest: torch's compaction of kept rows, point indices, bincounts, allocation | | %.1f | %.1f %% |" % (rest, 100.0 * rest / device_ms), "",
              "The tally's share of the sweep is %.1f %% (both tables: the molecules' count rows and the fits' winning rows)." %
              (100.0 * kernel_ms["fsq_signal_tally"] / device_ms), ""]
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
