"""Times the proteome Monte-Carlo on a synthetic proteome: --proteins proteins of --length residues drawn from
this tool's own amino-acid frequency table, cleaved after E, attached by C, labels K and D with windows 1 .. 30 each (60
observable pairs), --samples samples per attached peptide.

  kernel      device events around fsq_proteome_signals over the whole space in one launch (keys only), median of --reps.
  tally       device events around fsq_proteome_tally of those keys into fresh tables, median of --reps.
  uniques     device events around fsq_proteome_uniques over the sorted pairs, median of --reps.
  end to end  wall clock of monte_carlo_device + uniques_records + identifiable_proteins between two synchronisations
              (tables built on the host, chunks, torch's compaction and sorts, the scan, the answer as a dict), median of --reps
              after one warm-up run.
Writes profiles/proteome_mc_summary.md.  The comparison is the reference's pure-Python random_signal as
tools/gen_proteome_mc_golden.py prints its rate: pass it with --reference-rate.

  python tools/bench_proteome_mc.py [--proteins 2000 --length 300 --samples 1000 --reps 5 --reference-rate 1.5e4 --out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# a fixed table of this tool's own (roughly a vertebrate proteome's composition), in per cent
FREQUENCY = {'A': 7.0, 'C': 2.3, 'D': 4.7, 'E': 7.1, 'F': 3.7, 'G': 6.6, 'H': 2.6, 'I': 4.4, 'K': 5.7, 'L': 10.0, 'M': 2.1, 'N': 3.6,
             'P': 6.3, 'Q': 4.8, 'R': 5.6, 'S': 8.3, 'T': 5.3, 'V': 6.0, 'W': 1.2, 'Y': 2.7}


def proteome(n, length, seed):
    rng = np.random.default_rng(seed)
    acids, p = list(FREQUENCY), np.array(list(FREQUENCY.values())) / sum(FREQUENCY.values())
    return {"protein%05d" % i: "".join(rng.choice(acids, length, p=p)) for i in range(n)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proteins", type=int, default=2000)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--reference-rate", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proteome_mc_summary.md"))
    a = ap.parse_args()
    import torch
    from fluorosequencingimageanalysis_amd import MCsimlib as MC
    p, b, u = 0.9, 0.05, 0.1
    windows = {'K': tuple(range(1, 31)), 'D': tuple(range(1, 31))}
    peptides = MC.attach(MC.cleave(proteome(a.proteins, a.length, a.seed), 'E'), 'C')
    table = MC.proteome_table(peptides, windows)
    n_pep, S = len(table["protein"]), a.samples
    rows = n_pep * S
    dtable = MC.device_table(table, p, b)

    def events(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), out

    slots = min(max(1 << (2 * rows - 1).bit_length(), 1024), 1 << 26)
    k_ms, t_ms, u_ms = [], [], []
    for rep in range(a.reps + 1):
        ms, (key, protein, _) = events(lambda: MC.signals_device(dtable, u, S, a.seed))
        tables = MC.new_tables(slots, slots, "cuda")
        torch.cuda.synchronize()
        ms_t, _ = events(lambda: MC.tally_device(tables, key, protein))
        MC.check_tables(tables)
        _, d_protein, d_count, d_segment = MC.pairs_device(tables)
        torch.cuda.synchronize()
        ms_u, _ = events(lambda: MC.uniques_device(d_protein, d_count, d_segment, MC.H.scan_modes(10.0, 5, None)))
        if rep:                                                                          # (the first round warms up)
            k_ms.append(ms), t_ms.append(ms_t), u_ms.append(ms_u)
    n_signals, n_pairs = int(d_segment.shape[0]) - 1, int(d_protein.shape[0])
    empty = int((key == 0).sum())
    del key, protein, tables

    def whole():
        run = MC.monte_carlo_device(table, p, b, u, S, a.seed)
        return MC.identifiable_proteins(MC.uniques_records(run, 10.0, 5))
    whole()
    e_ms = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        found = whole()
        torch.cuda.synchronize()
        e_ms.append((time.perf_counter() - t) * 1e3)

    med = lambda v: float(np.median(v))                                                  # noqa: E731
    rng = lambda v: "%.3g (%.3g-%.3g)" % (med(v), min(v), max(v))                        # noqa: E731
    lines = ["# Proteome Monte-Carlo (`tools/bench_proteome_mc.py`)", "",
             "%d synthetic proteins of %d residues (the tool's own frequency table, seed %d), cleaved after `E`, attached by `C`:" %
             (a.proteins, a.length, a.seed),
             "%d attached peptides of %d proteins, %d labelled residues; labels `K` and `D`, windows 1 .. 30 each (60 observable pairs)," %
             (n_pep, len(peptides), int(table["label_start"][-1])),
             "p = %g, b = %g, u = %g, %d samples per peptide: %d samples.  One session on one %s; median (min-max) of %d runs" %
             (p, b, u, S, rows, torch.cuda.get_device_name(0), a.reps),
             "after one warm-up run.  Kernel rows: device events around the one launch; end to end: wall clock between two synchronisations.", "",
             "| stage | ms | samples/s |", "|---|---|---|",
             "| `fsq_proteome_signals` (keys, proteins) | %s | %.3g |" % (rng(k_ms), rows / med(k_ms) * 1e3),
             "| `fsq_proteome_tally` (tables of %d / %d slots) | %s | %.3g |" % (slots, slots, rng(t_ms), rows / med(t_ms) * 1e3),
             "| `fsq_proteome_uniques` (%d signals, %d pairs) | %s | |" % (n_signals, n_pairs, rng(u_ms)),
             "| end to end: `monte_carlo_device` + `uniques_records` + `identifiable_proteins` | %s | %.3g |" %
             (rng(e_ms), rows / med(e_ms) * 1e3), "",
             "%d of the samples are empty signals (counted nowhere); %d distinct signals, %d (signal, protein) pairs; %d of %d proteins" %
             (empty, n_signals, n_pairs, len(found), len(peptides)),
             "are best for at least one signal at worst_ratio 10, absolute_min 5.", ""]
    if a.reference_rate:
        lines += ["The reference's pure-Python `random_signal` (one core of Python on the build container's CPU, a 13-residue head and a",
                  "4-residue tail, two labels, windows 1 .. 16, as `tools/gen_proteome_mc_golden.py` prints it): %.3g signals/s.  The kernel's" % a.reference_rate,
                  "rate is %.3g times that, the end-to-end rate %.3g times, on a larger problem per signal (windows 1 .. 30)." %
                  (rows / med(k_ms) * 1e3 / a.reference_rate, rows / med(e_ms) * 1e3 / a.reference_rate), ""]
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
