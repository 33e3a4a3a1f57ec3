"""Times the parameter sweep over several label letters on the shape of tools/bench_signal_sweep.py: a two-letter
peptide, 3 mocks + 8 Edmans (12 frames), a 10 x 10 x 10 grid of (Edman efficiency, dye destruction per cycle, dud rate) x
100 000 molecules, common random numbers.  Wall clock between two synchronisations, median (min-max) of --reps calls after a
warm-up call:

  * `signal_sweep.joint_sweep_device`, fitted and unfitted;
  * the loop of `peptide_simulator.multilabel_and_fit_records` over the same points, the only way without the sweep: --loop-points
    points are timed and the figure is scaled to the grid - an extrapolation, and the table says so;
  * `fsq_peptide_simulate_labels_points` at K = 1 against `fsq_peptide_simulate_points` on the same parameters and rows, each a
    bare launch into buffers allocated beforehand, alternating in one loop (device events);
  * `multilabel_and_fit_records` at K = 4, 10^7 molecules: its joint ground truth is now the joint key tally.

No other method is timed over the whole grid.  Writes profiles/joint_sweep_summary.md.

  python tools/bench_joint_sweep.py [--grid G --num-sims N --reps R --loop-points L --k4-molecules M --table-slots S --out FILE]"""
import argparse
import ctypes
import itertools
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEQUENCE, LABELS = "GAKCGAKC", "KC"
ONE = ("GAKAGAKC", "K")
FOUR = ("GAKCDEAKCDEG", "KCDE")
MOCKS, EDMANS = 3, 8


def med(xs):
    return "%.1f (%.1f-%.1f)" % (float(np.median(xs)), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=10, help="values per axis")
    ap.add_argument("--num-sims", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-points", type=int, default=20)
    ap.add_argument("--k4-molecules", type=int, default=10 ** 7)
    ap.add_argument("--table-slots", type=int, default=1 << 14, help="two letters have more distinct joint signals than one has signals")
    ap.add_argument("--seed", type=int, default=20241019)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_sweep_summary.md"))
    a = ap.parse_args()
    import torch
    from fluorosequencingimageanalysis_amd import _native_signal_sweep as NS
    from fluorosequencingimageanalysis_amd import engine
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    ddif = [0, 0.3] + [0.3] * 5
    fixed = dict(s=0.3, sc=3, s2=0.1, beta={"K": 70000.0, "C": 40000.0}, beta_sigma=0.2, ddif=ddif, superdye_rate=0.0, superdye_factor=1.0)
    G, n = a.grid, a.num_sims
    grid = list(itertools.product(np.linspace(0.80, 0.98, G).tolist(), np.linspace(0.02, 0.20, G).tolist(), np.linspace(0.05, 0.50, G).tolist()))
    points = [(p, -math.log(1.0 - d), u) for p, d, u in grid]
    P = len(points)

    def wall(call, reps):
        out = []
        for _ in range(reps + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = call()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t) * 1e3)
        return out[1:], res                                                        # (the first call warms the allocator up)

    fitted, sweep = wall(lambda: SW.joint_sweep_device(SEQUENCE, LABELS, MOCKS, EDMANS, points, n, seed=a.seed, quench_factors=ddif,
                                                       table_slots=a.table_slots, **fixed),
                         a.reps)
    distinct = float((sweep["signals"]["keys"] != NS.EMPTY).sum()) / P
    distinct_mol = float((sweep["molecular"]["keys"] != NS.EMPTY).sum()) / P
    del sweep
    unfitted, _ = wall(lambda: SW.joint_sweep_device(SEQUENCE, LABELS, MOCKS, EDMANS, points, n, seed=a.seed, fit=False,
                                                    table_slots=a.table_slots, **fixed), a.reps)
    some = points[::max(1, P // a.loop_points)][:a.loop_points]

    def loop():
        for p, b, u in some:
            PS.multilabel_and_fit_records(SEQUENCE, LABELS, MOCKS, EDMANS, n, seed=a.seed, max_possible=5, allow_multidrop=True,
                                          max_deviation=3, quench_factors=ddif, p=p, b=b, u=u, **fixed)
    looped, _ = wall(loop, 1)
    scaled = [t * P / len(some) for t in looped]

    # ---- K = 1: the labels-points kernel against the one-letter points kernel, alternating ----
    one_fixed = dict(fixed, beta=70000.0)
    base1, values1, _ = SW._point_params(*ONE, MOCKS, EDMANS, a.seed, 0, points, one_fixed)
    baseL, valuesL, _, _ = SW._joint_point_params(*ONE, MOCKS, EDMANS, a.seed, 0, points, one_fixed)
    assert np.array_equal(values1, valuesL)
    d_points = torch.from_numpy(values1).cuda()
    rows = min(P * n, 1 << 22)
    old = SW.simulate_points_device(base1, d_points, P, n, 0, 0, rows)
    new = SW.simulate_labels_points_device(baseL, d_points, P, n, 0, 0, rows)
    torch.cuda.synchronize()
    assert all(bool((new[k][0] == old[k]).all()) for k in ("counts", "intensity", "category"))

    def entry(fn, what, prm, tables):
        return lambda: engine.launch(fn, what, d_points.device, ctypes.byref(prm), d_points.data_ptr(), P, n, 0, 0, rows,
                                     *[tables[k].data_ptr() for k in ("counts", "intensity", "category")])
    calls = [("fsq_peptide_simulate_labels_points, K = 1", entry(NS.lib().fsq_peptide_simulate_labels_points,
                                                                 "fsq_peptide_simulate_labels_points", baseL, new)),
             ("fsq_peptide_simulate_points", entry(NS.lib().fsq_peptide_simulate_points, "fsq_peptide_simulate_points", base1, old))]
    times = {name: [] for name, _ in calls}
    for r in range(3 * a.reps + 1):
        for name, call in calls:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            call()
            t1.record()
            torch.cuda.synchronize()
            if r:
                times[name].append(t0.elapsed_time(t1))
    del old, new

    # ---- K = 4: the joint ground truth of multilabel_and_fit_records ----
    four_fixed = dict(fixed, beta=70000.0, p=0.9, b=-math.log(1.0 - 0.1), u=0.5)
    k4, res = wall(lambda: PS.multilabel_and_fit_records(*FOUR, MOCKS, EDMANS, a.k4_molecules, seed=a.seed, max_possible=5,
                                                         allow_multidrop=True, max_deviation=3, quench_factors=ddif, **four_fixed), 3)
    n_mes = len(res["molecular_error_signals"])
    sim = res["simulation"]
    del res
    truth, _ = wall(lambda: PS.joint_signals_from_device(sim), 3)
    del sim

    m_fit, m_unfit, m_loop = float(np.median(fitted)), float(np.median(unfitted)), float(np.median(scaled))
    a_new, a_old = (float(np.median(times[name])) for name, _ in calls)
    lines = ["# Parameter sweep over several label letters (`tools/bench_joint_sweep.py`)", "",
             "`%s`, labels `%s`, %d mocks + %d Edmans (%d frames), a %d x %d x %d grid of (Edman efficiency 0.80-0.98, dye destruction" %
             (SEQUENCE, LABELS, MOCKS, EDMANS, MOCKS + EDMANS + 1, G, G, G),
             "per cycle 0.02-0.20, dud rate 0.05-0.50) x %d molecules, common random numbers, seed %d; one run on one %s." %
             (n, a.seed, torch.cuda.get_device_name(0)),
             "Wall clock between two synchronisations after a warm-up call, median (min-max).  %.0f distinct fitted and %.0f distinct" %
             (distinct, distinct_mol),
             "molecular joint signals per point on average; table_slots=%d." % a.table_slots, "",
             "| route | runs | ms | points/s | molecules/s |", "|---|---|---|---|---|",
             "| `joint_sweep_device`, fitted | %d | %s | %.3g | %.3g |" % (len(fitted), med(fitted), P / m_fit * 1e3, P * n / m_fit * 1e3),
             "| `joint_sweep_device`, fit=False | %d | %s | %.3g | %.3g |" % (len(unfitted), med(unfitted), P / m_unfit * 1e3, P * n / m_unfit * 1e3),
             "| loop: `multilabel_and_fit_records` per point, EXTRAPOLATED from %d timed points (x %d / %d) | %d | %s | %.3g | %.3g |" %
             (len(some), P, len(some), len(looped), med(scaled), P / m_loop * 1e3, P * n / m_loop * 1e3), "",
             "The loop was not run over the grid: %d of its %d points took %s ms, and the row above scales that by %d / %d.  By that" %
             (len(some), P, med(looped), P, len(some)),
             "figure the loop would take %.1f times as long as the fitted sweep.  The loop fits each channel's signals apart and tallies" % (m_loop / m_fit),
             "only the molecular signals jointly; the sweep tallies both jointly.", "",
             "## K = 1 against `fsq_peptide_simulate_points`", "",
             "`%s` with `%s`, the same points, the first %d rows of the grid, bit-equal tables, each a bare launch into buffers allocated" % (ONE[0], ONE[1], rows),
             "beforehand, alternating in one loop of %d rounds after a warm-up round (device events, ms):" % (3 * a.reps), "",
             "| " + " | ".join(name for name, _ in calls) + " | ratio of medians |", "|---|---|---|",
             "| " + " | ".join("%.3f (%.3f-%.3f)" % (float(np.median(times[name])), min(times[name]), max(times[name])) for name, _ in calls) +
             " | %.3f |" % (a_new / a_old), "",
             "## `multilabel_and_fit_records` at K = 4", "",
             "`%s` with `%s`, %d molecules, %d distinct joint molecular signals: %s ms, median (min-max) of %d calls; of which" %
             (FOUR[0], FOUR[1], a.k4_molecules, n_mes, med(k4), len(k4)),
             "`joint_signals_from_device` (the joint key tally and the decoding of its occupied slots) %s ms." % med(truth), ""]
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
