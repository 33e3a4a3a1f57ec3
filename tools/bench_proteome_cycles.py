"""Times the cycle curve of the proteome Monte-Carlo on the synthetic proteome of tools/bench_proteome_mc.py:
one run at windows 1 .. 30 for two labels, then identifiable proteins for cycles 1 .. 30 from that one tally.

  projection  device events around fsq_proteome_project over all 30 masks in one launch into fresh tables, median of --reps
              after one warm-up: pair-major and mask-major item order, alternating, and 30 launches of one mask.
  compaction  device events around the compaction of all 30 tables and the three sorts (torch), median of --reps.
  uniques     device events around the one fsq_proteome_uniques launch over the concatenated segments, median of --reps.
  end to end  wall clock of cycle_curve_records on the device run between two synchronisations, median of --reps after one
              warm-up.
  host=True   wall clock of cycle_curve_records on the records of a run scaled down to --host-proteins proteins, on the device
              and with host=True (NumPy twin, one core) on the same triples.
  drop-in     wall clock of SignalTrie.truncating_projection(c) for the 30 cycle counts, each on a fresh trie of the records of
              a run scaled down to --trie-proteins proteins (building the tries is not counted).
Writes profiles/proteome_cycles_summary.md.

  python tools/bench_proteome_cycles.py [--proteins 2000 --length 300 --samples 1000 --reps 5 --host-proteins 200 --trie-proteins 10 --out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_proteome_mc import proteome                                           # noqa: E402

P, B, U = 0.9, 0.05, 0.1
WINDOWS = {'K': tuple(range(1, 31)), 'D': tuple(range(1, 31))}
CYCLES = list(range(1, 31))
UNIQUES = (10.0, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proteins", type=int, default=2000)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--trie-proteins", type=int, default=10)
    ap.add_argument("--host-proteins", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proteome_cycles_summary.md"))
    a = ap.parse_args()
    import torch
    from fluorosequencingimageanalysis_amd import MCsimlib as MC
    H = MC.H
    peptides = MC.attach(MC.cleave(proteome(a.proteins, a.length, a.seed), 'E'), 'C')
    table = MC.proteome_table(peptides, WINDOWS)
    run = MC.monte_carlo_device(table, P, B, U, a.samples, a.seed)
    key, protein, count, n_signals = MC._source_pairs(run)
    n_pairs = int(key.shape[0])
    sa, sb = MC._pow2_at_least(2 * n_signals), MC._pow2_at_least(2 * n_pairs)
    d_mask = torch.from_numpy(H.cycle_masks(table["layout"], CYCLES).view(np.int64)).cuda()
    NP = MC._native()

    def events(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), out

    def fresh():
        tables = MC.new_tables(sa, sb, "cuda", n_masks=len(CYCLES))
        torch.cuda.synchronize()
        return tables

    def one_by_one(tables):
        for i in range(len(CYCLES)):
            MC.project_into({k: v[i:i + 1] for k, v in tables.items()}, key, protein, count, d_mask[i:i + 1])

    ms = {"pair": [], "mask": [], "single": [], "compact": [], "uniques": []}
    modes = H.scan_modes(*UNIQUES, None)
    for rep in range(a.reps + 1):
        t_pair = fresh()
        pair = events(lambda: MC.project_into(t_pair, key, protein, count, d_mask, NP.PROJECT))[0]
        t_mask = fresh()
        mask = events(lambda: MC.project_into(t_mask, key, protein, count, d_mask, NP.PROJECT | NP.MASK_MAJOR))[0]
        t_single = fresh()
        single = events(lambda: one_by_one(t_single))[0]
        assert not int(t_pair["overflow"].sum()) and all(torch.equal(t_pair["counts"].sum(dim=1), t["counts"].sum(dim=1))
                                                        for t in (t_mask, t_single))
        proj = {"tables": t_pair}
        compact, (cyc, _, d_protein, d_count, d_segment) = events(lambda: MC._sorted_projection(proj))
        uniq = events(lambda: MC.uniques_device(d_protein, d_count, d_segment, modes))[0]
        if rep:                                                                      # (the first round warms up)
            for name, v in zip(("pair", "mask", "single", "compact", "uniques"), (pair, mask, single, compact, uniq)):
                ms[name].append(v)
        del t_pair, t_mask, t_single, proj
    total_pairs, total_signals = int(cyc.shape[0]), int(d_segment.shape[0]) - 1
    del cyc, d_protein, d_count, d_segment

    def wall(fn, reps):
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            got = fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t) * 1e3)
        return out, got
    MC.cycle_curve_records(run, *UNIQUES, cycles=CYCLES)
    e_ms, curve = wall(lambda: MC.cycle_curve_records(run, *UNIQUES, cycles=CYCLES), a.reps)
    del run
    scaled = MC.attach(MC.cleave(proteome(a.host_proteins, a.length, a.seed), 'E'), 'C')
    scaled_records = MC.monte_carlo_records(scaled, P, B, U, WINDOWS, sample_size=a.samples, seed=a.seed)
    MC.cycle_curve_records(scaled_records, *UNIQUES, cycles=CYCLES)
    d_ms, on_device = wall(lambda: MC.cycle_curve_records(scaled_records, *UNIQUES, cycles=CYCLES), a.reps)
    h_ms, host = wall(lambda: MC.cycle_curve_records(scaled_records, *UNIQUES, cycles=CYCLES, host=True), 1)
    assert all(np.array_equal(host[k], on_device[k]) for k in H.CURVE_FIELDS + ("identifiable",))

    small = MC.attach(MC.cleave(proteome(a.trie_proteins, a.length, a.seed), 'E'), 'C')
    small_records = MC.monte_carlo_records(small, P, B, U, WINDOWS, sample_size=a.samples, seed=a.seed)
    tries = [MC.trie_of_records(small_records) for _ in CYCLES]
    t = time.perf_counter()
    for trie, c in zip(tries, CYCLES):
        trie.truncating_projection(c)
    trie_ms = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    MC.cycle_curve_records(small_records, *UNIQUES, cycles=CYCLES)
    torch.cuda.synchronize()
    small_ms = (time.perf_counter() - t) * 1e3

    med = lambda v: float(np.median(v))                                                  # noqa: E731
    rng = lambda v: "%.3g (%.3g-%.3g)" % (med(v), min(v), max(v))                        # noqa: E731
    items = n_pairs * len(CYCLES)
    lines = ["# Cycle curve of the proteome Monte-Carlo (`tools/bench_proteome_cycles.py`)", "",
             "%d synthetic proteins of %d residues (seed %d), cleaved after `E`, attached by `C`, labels `K` and `D` with windows" %
             (a.proteins, a.length, a.seed),
             "1 .. 30, p = %g, b = %g, u = %g, %d samples per attached peptide: %d distinct signals, %d (signal, protein) pairs." %
             (P, B, U, a.samples, n_signals, n_pairs),
             "Cycle counts 1 .. 30 from that one tally: %d (pair, mask) items, tables of %d / %d slots per cycle count; the 30" %
             (items, sa, sb),
             "projections hold %d signals and %d pairs together.  One session on one %s; median (min-max) of %d runs after" %
             (total_signals, total_pairs, torch.cuda.get_device_name(0), a.reps),
             "one warm-up.  Kernel rows: device events; end to end: wall clock between two synchronisations.", "",
             "| stage | ms | items/s |", "|---|---|---|",
             "| `fsq_proteome_project`, 30 masks in one launch, pair-major (the default) | %s | %.3g |" % (rng(ms["pair"]), items / med(ms["pair"]) * 1e3),
             "| the same, mask-major (`FSQ_PMC_MASK_MAJOR`) | %s | %.3g |" % (rng(ms["mask"]), items / med(ms["mask"]) * 1e3),
             "| the same, 30 launches of one mask | %s | %.3g |" % (rng(ms["single"]), items / med(ms["single"]) * 1e3),
             "| compaction of the 30 tables and three sorts (torch) | %s | |" % rng(ms["compact"]),
             "| `fsq_proteome_uniques`, one launch over %d signals | %s | |" % (total_signals, rng(ms["uniques"])),
             "| end to end: `cycle_curve_records` on the device run | %s | |" % rng(e_ms)]
    lines += ["", "Scaled comparison with the NumPy twin: on %d proteins of the same kind (%d pairs), `cycle_curve_records` on the records," %
              (a.host_proteins, len(scaled_records["key"])),
              "upload included, takes %s ms on the device and %.3g ms with `host=True` (one core, one run) on the same triples, with" %
              (rng(d_ms), h_ms[0]),
              "equal results.  The twin scans every signal of every cycle count in a Python loop; it is scaled down to stay in seconds."]
    lines += ["", "The curve: %s identifiable proteins at cycles %s." %
              (", ".join(str(int(curve["n_identifiable_proteins"][i])) for i in (0, 4, 9, 19, 29)), "1, 5, 10, 20, 30"), "",
              "Scaled comparison with the drop-in: on %d proteins of the same kind (%d pairs), `SignalTrie.truncating_projection` for" %
              (a.trie_proteins, len(small_records["key"])),
              "the 30 cycle counts, each on a trie built beforehand, takes %.3g ms of Python; `cycle_curve_records` on those records," % trie_ms,
              "upload and scan included, takes %.3g ms.  The problem is scaled down %d times in proteins because a trie of the full" %
              (small_ms, a.proteins // max(a.trie_proteins, 1)),
              "run is one Python object per node, 30 times over.", ""]
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
