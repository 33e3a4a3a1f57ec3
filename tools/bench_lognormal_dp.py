"""Times fsq_lognormal_fit_dp next to fsq_lognormal_fit at the size of tools/bench_lognormal.py: 262 144 tracks
x 12 cycles, max_possible=5, max_deviation=3, the same seeded table (alpha-adjusted intensities, the first fit's beta).  Each
is timed with device events after a warm-up call (median, least and greatest of --reps calls):

  enumerate            the default solver
  dp                   the dynamic programme, the same outputs (checked here, bit for bit)
  dp, upsteps          allow_upsteps=True
  dp, 64 x 15          --long-tracks tracks of 64 ON frames at max_possible=15, max_deviation=1e9: every track is over the
                       enumerating kernel's budget (checked here)

Writes profiles/lognormal_dp_summary.md.

  python tools/bench_lognormal_dp.py [--tracks N --cycles T --reps R --long-tracks N --out FILE --other-lib LIBFSQ_HIP.SO]

--other-lib: another build of libfsq_hip.so (the parent commit's, say).  `enumerate` is timed on it too, in a child process
of its own, and the summary sets the two side by side: the yardstick for "the enumerating kernel is no slower than it was"."""
import argparse
import json
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def time_fit(LN, torch, reps, *args, **kw):
    """(median ms, least, greatest, device outputs) of lognormal_device after one warm-up call."""
    out = LN.lognormal_device(*args, **kw)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = LN.lognormal_device(*args, **kw)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms), out


def default_table(torch, n, T):
    from bench_lognormal import make_tracks
    vals, words, _ = make_tracks(n, T)
    ddif = [0.0] + [0.3] * 6
    means = [math.log(10000.0) + math.log(i + 1.0) - ddif[i] for i in range(7)]
    return (torch.from_numpy(vals - 120.0).cuda(), torch.from_numpy(words.view(np.int64)).cuda(),
            torch.full((n,), T, dtype=torch.int32, device="cuda"), means)


def long_table(torch, n, seed=6415):
    rng = np.random.default_rng(seed)
    ddif = [0.0] + [0.3] * 16
    means = [math.log(10000.0) + math.log(i + 1.0) - ddif[i] for i in range(17)]
    seq = -np.sort(-rng.integers(1, 16, (n, 64)), axis=1)
    vals = np.floor(np.exp(rng.normal(np.array(means)[seq - 1], 0.2)))
    return (torch.from_numpy(vals).cuda(), torch.full((n,), -1, dtype=torch.int64, device="cuda"),
            torch.full((n,), 64, dtype=torch.int32, device="cuda"), means)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=262144)
    ap.add_argument("--cycles", type=int, default=12)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--long-tracks", type=int, default=16384)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--only-enumerate", action="store_true", help="(the child of --other-lib) time enumerate and print one JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lognormal_dp_summary.md"))
    a = ap.parse_args()
    import torch
    from fluorosequencingimageanalysis_amd import lognormal as LN
    n, T = a.tracks, a.cycles
    d_int, d_cat, d_len, means = default_table(torch, n, T)
    enum = time_fit(LN, torch, a.reps, d_int, d_cat, d_len, means, 0.2, 5, True, 3)
    if a.only_enumerate:
        print(json.dumps({"ms": enum[:3]}))
        return
    rows = [("enumerate", n, enum)]
    dp = time_fit(LN, torch, a.reps, d_int, d_cat, d_len, means, 0.2, 5, True, 3, solver='dp')
    for k in enum[3]:
        assert torch.equal(enum[3][k], dp[3][k]), k                 # (bit for bit: the scores are compared as doubles, none is NaN)
    assert not bool(torch.isnan(dp[3]["best_score"]).any())
    rows.append(("dp", n, dp))
    ups = time_fit(LN, torch, a.reps, d_int, d_cat, d_len, means, 0.2, 5, True, 3, solver='dp', allow_upsteps=True)
    rows.append(("dp, upsteps", n, ups))
    l_int, l_cat, l_len, l_means = long_table(torch, a.long_tracks)
    over = LN.lognormal_device(l_int, l_cat, l_len, l_means, 0.2, 15, True, 1e9)
    assert bool((over["status"] == LN.STATUS_OVER_BUDGET).all())
    long_dp = time_fit(LN, torch, a.reps, l_int, l_cat, l_len, l_means, 0.2, 15, True, 1e9, solver='dp')
    assert bool((long_dp[3]["status"] == LN.STATUS_FOUND).all())
    rows.append(("dp, 64 frames x max_possible 15, max_deviation 1e9", a.long_tracks, long_dp))
    lines = ["# Lognormal fit by dynamic programme (`tools/bench_lognormal_dp.py`)", "",
             "%d tracks x %d cycles, max_possible=5, max_deviation=3, beta_sigma=0.2, multi-drop allowed (the first fit of" % (n, T),
             "`tools/bench_lognormal.py`); the last row %d tracks of 64 ON frames.  Device events around `lognormal.lognormal_device`"
             % a.long_tracks, "after a warm-up call, median (min-max) of %d calls on one %s." % (a.reps, torch.cuda.get_device_name(0)), "",
             "| solver | tracks | ms | tracks/s | with a sequence | winners that step up |", "|---|---|---|---|---|---|"]
    for name, count, (ms, lo, hi, out) in rows:
        seq = out["best_seq"].to(torch.int16)
        up = ((seq[:, 1:] > seq[:, :-1]).any(dim=1) & (out["status"] == 0)).float().mean().item()
        lines.append("| %s | %d | %.3f (%.3f-%.3f) | %.3g | %.1f %% | %.1f %% |" %
                     (name, count, ms, lo, hi, count / ms * 1e3, 100.0 * (out["status"] == 0).float().mean().item(), 100.0 * up))
    lines += ["", "`dp` and `enumerate` gave the same five outputs, bit for bit.  `enumerate` reports every track of the last row over its",
              "budget (C(78, 14) surviving sequences each)."]
    if a.other_lib:
        env = dict(os.environ, FSQ_HIP_LIB=os.path.abspath(a.other_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--only-enumerate", "--tracks", str(n), "--cycles", str(T), "--reps", str(a.reps)]
        other = json.loads(subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=300).stdout.strip().split("\n")[-1])["ms"]
        lines += ["", "`enumerate` on the other build of the library given with `--other-lib` (the parent commit's), same machine, same",
                  "process layout: %.3f (%.3f-%.3f) ms; on this build %.3f (%.3f-%.3f) ms." % (tuple(other) + enum[:3])]
    text = "\n".join(lines + [""])
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
