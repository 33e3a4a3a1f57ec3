"""Times the iterative background correction of one problem at three key counts, the device against the host twin
in the same run, and at the smallest also the reference-shaped Python loop of the restatement (one dict copy, one
renormalisation and one z-score table per trial: tests/_background_reference.py `iterate_dicts`).

  smallest   the fixture's largest case (`eight_cycles` of tests/golden/background_signals.npz)
  middle     every sorted key of up to 5 drops over 9 cycles (2 001 keys), synthetic counts with planted peaks
  largest    the same over 12 cycles (6 187 keys)

  device     `background.background_records([problem], device="cuda")`: upload, fsq_background_iterate (which synchronises after
             every batch of passes), download.  Wall time between two device synchronisations, after one warm-up call: median
             (min-max) of --reps calls.
  host       `background.background_records([problem], device=None)`, numpy on this machine's CPU, one process, once; its
             outputs are compared with the device's bit for bit.
Writes profiles/background_summary.md.

  python tools/bench_background.py [--reps R] [--no-loop] [--out FILE]
"""
import argparse
import os
import re
import shlex
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CSRC = os.path.join(ROOT, "fluorosequencingimageanalysis_amd", "csrc")
KERNELS = ("kbg_neighbours", "kbg_first", "kbg_head", "kbg_trials", "kbg_tail")


def resources():
    """{kernel: {VGPRs, ScratchSize, LDS, Occupancy, SGPRs Spill, VGPRs Spill}} as the compiler reports them for the command with
    which csrc/Makefile builds the kernels (a dry run of make gives it)."""
    obj = "background/fsq_background.o"
    dry = subprocess.run(["make", "-n", "-B", obj], cwd=CSRC, capture_output=True, text=True, check=True).stdout
    compiles = [line for line in dry.splitlines() if "fsq_background.hip" in line]
    assert compiles, "csrc/Makefile's dry run of %s names no compile of fsq_background.hip:\n%s" % (obj, dry)
    cmd = shlex.split(compiles[-1])
    cmd[cmd.index("-o") + 1] = os.devnull
    err = subprocess.run(cmd + ["-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]|"
                      r"SGPRs Spill|VGPRs Spill): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = next((k for k in KERNELS if k in m.group(2)), m.group(2))
            out[name] = {}
        elif name:
            out[name][m.group(1).split(" [")[0]] = int(m.group(2))
    return out


def same(a, b):
    ok = all(a[k] == b[k] for k in ("stop_reason", "n_passes", "n_accepted"))
    for k in ("count", "percent"):
        ok = ok and np.array_equal(np.asarray(a[k]).view(np.uint64), np.asarray(b[k]).view(np.uint64))
    return ok and np.array_equal(a["rounded"], b["rounded"]) and np.array_equal(a["accepted_key"], b["accepted_key"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-loop", action="store_true", help="leave the reference-shaped loop out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "background_summary.md"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this measures the GPU: there is nothing to time without one"
    import _background_cases as C
    import _background_reference as R
    from fluorosequencingimageanalysis_amd import background as BG
    c = C.case("eight_cycles")
    fixture = (c["boc_experiment"], c["boc_percent"], c["averaged_ac"], c["ac_stds"], c["num_cycles"], c["sigma"], not c["omit_multidrop"])
    sizes = [("fixture `eight_cycles`", fixture),
             ("<= 5 drops over 9 cycles", C.problem(len(C.all_keys(9, 5)), 41, C=9, D=5, peaks=12)),
             ("<= 5 drops over 12 cycles", C.problem(len(C.all_keys(12, 5)), 42, C=12, D=5, peaks=12))]
    name = "%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName.split(":")[0])
    lines = ["# Iterative background correction of signal counts (`tools/bench_background.py`)", "",
             "One run on one %s, `python tools/bench_background.py --reps %d`.  One problem per call (P = 1).  Device: upload," % (name, a.reps),
             "`fsq_background_iterate`, download, wall time between two device synchronisations after a warm-up call, median (min-max)",
             "of %d calls.  Host: the numpy twin (`device=None`, numpy %s, one process of this machine's CPU), once." % (a.reps, np.__version__), "",
             "| problem | keys | defined | passes | accepted | device ms | host twin ms | same bits |", "|---|---|---|---|---|---|---|---|"]
    all_same = True
    kw = dict(accepted_cap=8192, undefined_cap=0)
    for label, args in sizes:
        prob = BG.pack_problem(*args)
        BG.background_records([prob], device="cuda", **kw)
        ms = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            (dev,) = BG.background_records([prob], device="cuda", **kw)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        (host,) = BG.background_records([prob], device=None, **kw)
        host_ms = (time.perf_counter() - t0) * 1e3
        ok = same(dev, host)
        all_same = all_same and ok
        lines.append("| %s | %d | %d | %d | %d | %.1f (%.1f-%.1f) | %.0f | %s |" %
                     (label, len(prob["code"]), len(prob["def_key"]), dev["n_passes"], dev["n_accepted"], float(np.median(ms)), min(ms),
                      max(ms), host_ms, "yes" if ok else "NO"))
    if not a.no_loop:
        t0 = time.perf_counter()
        r = R.iterate_dicts(*fixture)
        loop_s = time.perf_counter() - t0
        lines += ["", "The reference-shaped Python loop of the restatement (`iterate_dicts`: per trial one dict copy, one renormalisation of all",
                  "keys and one z-score table) on the fixture case, once: %.2f s for %d passes." % (loop_s, r["passes"])]
    lines += ["", "Resources (hipcc `-Rpass-analysis=kernel-resource-usage`, gfx950):", ""]
    for k, r in resources().items():
        lines.append("- `%s`: %s VGPRs, %s bytes of scratch per lane, %s bytes of LDS per block, %s waves per SIMD, %s SGPRs and %s VGPRs spilled"
                     % (k, r.get("VGPRs"), r.get("ScratchSize"), r.get("LDS Size"), r.get("Occupancy"), r.get("SGPRs Spill"), r.get("VGPRs Spill")))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)
    assert all_same, "the device's results differ from the host's"


if __name__ == "__main__":
    main()
