"""Times the proteome Monte-Carlo over a (p, b, u) grid on bench_proteome_mc.py's synthetic proteome: --proteins
proteins of --length residues, cleaved after E, attached by C, labels K and D with windows 1 .. 30 each, --samples samples per
attached peptide and point, a --grid P x B x U grid (p 0.80 .. 0.95, b 0.02 .. 0.10, u 0.05 .. 0.20).

  signals     device events around fsq_proteome_signals_points over all points and rows in one launch (keys only).
  tally       device events around fsq_proteome_tally_points of those keys into fresh tables.
  sorts       wall clock of the compaction of all points' tables and the three sorts (torch) on a grid_device result.
  uniques     device events around fsq_proteome_uniques over the concatenated segments of all points.
  batched     wall clock of grid_curve_records between two synchronisations.
  loop        wall clock of what it replaces, point by point: monte_carlo_device + uniques_records + identifiable_proteins.
All in one session, each the median (min-max) of --reps runs after one warm-up run; the loop and the batched call are checked to
name the same number of identifiable proteins at every point.  Writes profiles/proteome_sweep_summary.md.

  python tools/bench_proteome_sweep.py [--proteins 2000 --length 300 --samples 100 --grid 4 4 4 --reps 5 --out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_proteome_mc import proteome                                                  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proteins", type=int, default=2000)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--grid", type=int, nargs=3, default=[4, 4, 4])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--stride", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proteome_sweep_summary.md"))
    a = ap.parse_args()
    import torch
    from fluorosequencingimageanalysis_amd import MCsimlib as MC
    windows = {'K': tuple(range(1, 31)), 'D': tuple(range(1, 31))}
    peptides = MC.attach(MC.cleave(proteome(a.proteins, a.length, a.seed), 'E'), 'C')
    table = MC.proteome_table(peptides, windows)
    n_pep, S = len(table["protein"]), a.samples
    rows = n_pep * S
    points = MC.grid_points(np.linspace(0.80, 0.95, a.grid[0]), np.linspace(0.02, 0.10, a.grid[1]), np.linspace(0.05, 0.20, a.grid[2]))
    K = len(points)
    scan = dict(worst_ratio=10.0, absolute_min=5)

    def events(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), out

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    gtable = MC.grid_device_table(table, points)
    slots = min(max(1 << (2 * rows - 1).bit_length(), 1024), 1 << 26)
    k_ms, t_ms = [], []
    for rep in range(a.reps + 1):
        ms, (key, protein, _) = events(lambda: MC.signals_points_device(gtable, S, a.seed, 0, a.stride))
        tables = MC.new_tables(slots, slots, "cuda", n_masks=K)
        torch.cuda.synchronize()
        ms_t, _ = events(lambda: MC.tally_points_device(tables, key, protein))
        if rep:                                                                          # (the first round warms up)
            k_ms.append(ms), t_ms.append(ms_t)
        del key, protein, tables
    del gtable
    modes = MC.H.scan_modes(10.0, 5, None)
    s_ms, u_ms = [], []
    for rep in range(a.reps + 1):
        grid = MC.grid_device(table, points, S, a.seed, sample_stride=a.stride)
        ms_s, (_, _, d_protein, d_count, d_segment) = wall(lambda: MC._sorted_projection(grid))
        ms_u, _ = events(lambda: MC.uniques_device(d_protein, d_count, d_segment, modes))
        if rep:
            s_ms.append(ms_s), u_ms.append(ms_u)
        n_signals, n_pairs = int(d_segment.shape[0]) - 1, int(d_protein.shape[0])
        del grid, d_protein, d_count, d_segment

    def batched():
        return MC.grid_curve_records(table, points, sample_size=S, seed=a.seed, sample_stride=a.stride, **scan)

    def loop():
        found = []
        for k, (p, b, u) in enumerate(points):
            run = MC.monte_carlo_device(table, p, b, u, S, a.seed, first_sample=k * a.stride)
            found.append(len(MC.identifiable_proteins(MC.uniques_records(run, **scan))))
        return found
    b_ms, l_ms = [], []
    for rep in range(a.reps + 1):
        ms_b, curve = wall(batched)
        ms_l, found = wall(loop)
        assert curve["n_identifiable_proteins"].tolist() == found, "the batched call and the loop disagree"
        if rep:
            b_ms.append(ms_b), l_ms.append(ms_l)

    med = lambda v: float(np.median(v))                                                  # noqa: E731
    rng = lambda v: "%.4g (%.4g-%.4g)" % (med(v), min(v), max(v))                        # noqa: E731
    below = med(b_ms) < min(l_ms)
    lines = ["# Proteome Monte-Carlo over a (p, b, u) grid (`tools/bench_proteome_sweep.py`)", "",
             "%d synthetic proteins of %d residues (`bench_proteome_mc.py`'s, seed %d), cleaved after `E`, attached by `C`: %d attached" %
             (a.proteins, a.length, a.seed, n_pep),
             "peptides of %d proteins; labels `K` and `D`, windows 1 .. 30 each.  A %d x %d x %d grid (p %.2f .. %.2f, b %.2f .. %.2f," %
             (len(peptides), a.grid[0], a.grid[1], a.grid[2], points[0][0], points[-1][0], points[0][1], points[-1][1]),
             "u %.2f .. %.2f): %d points, %d samples per peptide and point, %d samples a point, %d in all; sample_stride %d; tables of" %
             (points[0][2], points[-1][2], K, S, rows, K * rows, a.stride),
             "%d / %d slots a point.  One session on one %s; median (min-max) of %d runs after one warm-up run, the batched call" %
             (slots, slots, torch.cuda.get_device_name(0), a.reps),
             "and the loop alternating.  Kernel rows: device events around the one launch; the others: wall clock between two",
             "synchronisations.", "",
             "| stage | ms | ms a point |", "|---|---|---|",
             "| `fsq_proteome_signals_points` (keys of all points, one launch) | %s | %.4g |" % (rng(k_ms), med(k_ms) / K),
             "| `fsq_proteome_tally_points` (all points, one launch) | %s | %.4g |" % (rng(t_ms), med(t_ms) / K),
             "| compaction of the %d tables and three sorts (torch; wall clock) | %s | %.4g |" % (K, rng(s_ms), med(s_ms) / K),
             "| `fsq_proteome_uniques` (%d signals, %d pairs of all points, one launch) | %s | %.4g |" %
             (n_signals, n_pairs, rng(u_ms), med(u_ms) / K),
             "| batched: `grid_curve_records` | %s | %.4g |" % (rng(b_ms), med(b_ms) / K),
             "| loop: `monte_carlo_device` + `uniques_records` + `identifiable_proteins` per point | %s | %.4g |" % (rng(l_ms), med(l_ms) / K),
             "",
             "The batched median %s the loop's minimum (%.4g ms against %.4g ms; median against median: %.3g times)." %
             ("lies below" if below else "does NOT lie below", med(b_ms), min(l_ms), med(l_ms) / med(b_ms)),
             "Of the batched call's %.4g ms, %.4g ms are the two new kernels, %.4g ms the compaction and the sorts and %.4g ms the scan;" %
             (med(b_ms), med(k_ms) + med(t_ms), med(s_ms), med(u_ms)),
             "the rest is host-built tables and their upload, table allocation and fill, the per-point sums and the trip back.",
             "Identifiable proteins over the grid: %d .. %d of %d; both paths name the same number at every point." %
             (int(curve["n_identifiable_proteins"].min()), int(curve["n_identifiable_proteins"].max()), len(peptides)), ""]
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
