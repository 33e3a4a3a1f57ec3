"""Times the peptide Monte-Carlo simulation for several label letters on the shape of tools/bench_peptide_sim.py:
4 mocks with 1 omitted and 8 Edmans (12 frames), the command line's default rates, at K = 1, 2 and 4 colour channels.  Two
figures per (K, N): the kernel alone (device events around `peptide_simulator.multilabel_device_prm`, outputs allocated
beforehand by a warm-up call and recycled by the caching allocator; median of --reps) and simulate plus fit
(`multilabel_and_fit_records`: simulation, per channel the drop of dark molecules and the lognormal fit, torch.unique and the
unique rows turned into dictionaries; wall clock between two synchronisations, median of --chain-reps).

The one comparison: K = 1 of fsq_peptide_simulate_labels against fsq_peptide_simulate on the same parameters, each a bare
launch into buffers allocated beforehand, the calls alternating in one loop; with --parent-lib also against
fsq_peptide_simulate of a libfsq_hip.so built from the parent commit, in the same loop.  The tables of all of them are
compared before the loop.  Writes profiles/peptide_labels_summary.md.

  python tools/bench_peptide_labels.py [--sizes N ... --reps R --chain-reps R --parent-lib FILE --out FILE]"""
import argparse
import ctypes
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEPTIDES = {1: ("GAKAGAKC", "K"), 2: ("GAKCGAKC", "KC"), 4: ("GAKCDEAKCDEG", "KCDE")}
MOCKS, EDMANS = 3, 8


def med(xs):
    return "%.3f (%.3f-%.3f)" % (float(np.median(xs)), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10 ** 6, 10 ** 7])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--chain-reps", type=int, default=5, help="calls of simulate plus fit (seconds each at K = 4)")
    ap.add_argument("--seed", type=int, default=20240903)
    ap.add_argument("--parent-lib", default=None, help="libfsq_hip.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "peptide_labels_summary.md"))
    a = ap.parse_args()
    import torch
    from fluorosequencingimageanalysis_amd import _native_peptide_labels as NL
    from fluorosequencingimageanalysis_amd import _native_peptide_sim as NP
    from fluorosequencingimageanalysis_amd import engine
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS
    ddif = [0, 0.3] + [0.3] * 5
    ep = dict(p=0.9, b=-math.log(1.0 - 0.1), u=0.5, s=0.3, sc=3, s2=0.1, beta=70000.0, beta_sigma=0.2, ddif=ddif, superdye_rate=0.0,
              superdye_factor=1.0)
    F = MOCKS + EDMANS + 1

    def timed(call):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = call()
        t1.record()
        torch.cuda.synchronize()
        del out
        return t0.elapsed_time(t1)

    rows = []
    for K, (sequence, labels) in sorted(PEPTIDES.items()):
        for n in a.sizes:
            prm, meta = PS._labels_params(sequence, labels, MOCKS, EDMANS, a.seed, 0, ep)
            out = PS.multilabel_device_prm(prm, n)
            torch.cuda.synchronize()
            draws = int(out["n_draws"].sum())
            del out
            ms = [timed(lambda: PS.multilabel_device_prm(prm, n)) for _ in range(a.reps)]
            chain = []
            for _ in range(a.chain_reps + 1):
                torch.cuda.synchronize()
                t = time.perf_counter()
                res = PS.multilabel_and_fit_records(sequence, labels, MOCKS, EDMANS, n, seed=a.seed, max_possible=5, allow_multidrop=True,
                                                    max_deviation=3, quench_factors=ddif, **ep)
                torch.cuda.synchronize()
                chain.append((time.perf_counter() - t) * 1e3)
                kept, n_mes = [res[L]["total_count"] for L in meta["labels"]], len(res["molecular_error_signals"])
                del res
            bytes_per = K * F * 17 + 2 * len(meta["positions"]) + 8 + 8 * K + 4 * (1 + 2 * K)
            rows.append((K, n, ms, chain[1:], draws, bytes_per, kept, n_mes))       # (the first call warms the allocator up)

    # ---- K = 1 against fsq_peptide_simulate, alternating ----
    sequence, label = PEPTIDES[1]
    parent = None
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        parent.fsq_peptide_simulate.restype = ctypes.c_int
        parent.fsq_peptide_simulate.argtypes = [ctypes.POINTER(NP.FsqPeptideSimParams), ctypes.c_int64] + [ctypes.c_void_p] * 9
    versus = []
    for n in a.sizes:
        new_prm, _ = PS._labels_params(sequence, label, MOCKS, EDMANS, a.seed, 0, ep)
        old_prm, _ = PS._params(sequence, label, MOCKS, EDMANS, a.seed, 0, ep)
        bufs, new_bufs = PS.simulate_device_prm(old_prm, n), PS.multilabel_device_prm(new_prm, n)
        dev = bufs["counts"].device

        # (all three launch into buffers allocated beforehand: nothing but the launch stands between the two events)
        def entry(fn, what, prm, tables):
            return lambda: engine.launch(fn, what, dev, ctypes.byref(prm), n, *[tables[k].data_ptr() for k in PS.TABLES])
        calls = [("fsq_peptide_simulate_labels, K = 1", entry(NL.lib().fsq_peptide_simulate_labels, "fsq_peptide_simulate_labels", new_prm, new_bufs)),
                 ("fsq_peptide_simulate", entry(NP.lib().fsq_peptide_simulate, "fsq_peptide_simulate", old_prm, bufs))]
        if parent is not None:
            calls.append(("fsq_peptide_simulate, parent commit's library",
                          entry(parent.fsq_peptide_simulate, "fsq_peptide_simulate (parent)", old_prm, bufs)))
        for _, call in calls:
            call()
        torch.cuda.synchronize()
        # the three compute the same tables
        assert all(bool((new_bufs[k].reshape(bufs[k].shape) == bufs[k]).all()) for k in PS.TABLES)
        if parent is not None:
            mine = {k: v.clone() for k, v in bufs.items()}
            for v in bufs.values():
                v.zero_()
            calls[2][1]()
            torch.cuda.synchronize()
            assert all(bool((mine[k] == bufs[k]).all()) for k in PS.TABLES)
            del mine
        times = {name: [] for name, _ in calls}
        for _ in range(a.reps):
            for name, call in calls:
                times[name].append(timed(call))
        versus.append((n, times))
        del bufs, new_bufs

    lines = ["# Peptide Monte-Carlo simulation for several label letters (`tools/bench_peptide_labels.py`)", "",
             "%d mocks + %d Edmans (%d frames), the command line's default rates, seed %d; one run on one %s, median (min-max) of %d" %
             (MOCKS, EDMANS, F, a.seed, torch.cuda.get_device_name(0), a.reps),
             "calls.  Kernel: device events around `multilabel_device_prm` (the launch and the allocation of its outputs).  Simulate + fit:",
             "wall clock of `multilabel_and_fit_records` between two synchronisations, median of %d calls." % a.chain_reps,
             "Peptides: %s." %
             ", ".join("K = %d `%s` with `%s`" % (K, s, L) for K, (s, L) in sorted(PEPTIDES.items())), "",
             "| K | molecules | kernel ms | kernel molecules/s | Philox draws/s | output GB/s | simulate + fit ms | simulate + fit molecules/s | kept per channel | joint molecular error signals |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for K, n, ms, chain, draws, bytes_per, kept, n_mes in rows:
        m, c = float(np.median(ms)), float(np.median(chain))
        lines.append("| %d | %d | %s | %.3g | %.3g | %.0f | %s | %.3g | %s | %d |" %
                     (K, n, med(ms), n / m * 1e3, draws / m * 1e3, n * bytes_per / m / 1e6, med(chain), n / c * 1e3,
                      " ".join(str(k) for k in kept), n_mes))
    lines += ["", "## K = 1 against `fsq_peptide_simulate`", "",
              "`%s` with `%s`, the same parameters and bit-equal tables, each a bare launch into buffers allocated beforehand, alternating in one loop of %d rounds (device events, ms):" % (sequence, label, a.reps), "",
              "| molecules | " + " | ".join(name for name, _ in calls) + " |", "|---|" + "---|" * len(calls)]
    for n, times in versus:
        lines.append("| %d | " % n + " | ".join(med(times[name]) for name, _ in calls) + " |")
    lines.append("")
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
