"""Times fsq_lognormal_fit at a user's size: 262 144 tracks x 12 cycles, max_possible=5, max_deviation=3, tracks
seeded like fixture (b) of tools/gen_lognormal_golden.py (three fields with their own gain, lognormal ON frames, normal OFF
frames).  The first fit runs on alpha-adjusted intensities with the first beta, the second on ON/OFF-adjusted intensities
with the second beta, as lognormal_fitter_v2 runs them; each is timed with device events after a warm-up (median of --reps).
Writes profiles/lognormal_summary.md: tracks/s, surviving sequences per track and sequences/s of both fits.

  python tools/bench_lognormal.py --reference-ms MS [--tracks N --cycles T --reps R --out FILE]

--reference-ms (required): the reference's time per track, as tools/gen_lognormal_golden.py prints it for the batch fit of
fixture (b) on the machine it runs on; the summary quotes it next to the device's figures."""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_tracks(n, T, seed=4242):
    """(intensities float64 [n, T] raw, category words uint64 [n], fields int [n]): ON-prefix tracks as chain_csv() draws them."""
    rng = np.random.default_rng(seed)
    field = rng.integers(0, 3, n)
    gains = np.array([1.0, 1.12, 0.9])[field]
    start = rng.choice([1, 1, 1, 2, 2, 3], n)
    drops = rng.random((n, T)) < 0.3
    seq = np.zeros((n, T), np.int64)
    v = start.copy()
    for f in range(T):
        seq[:, f] = v
        v = np.where((v > 0) & drops[:, f], v - 1, v)
    cyc = 1.0 + 0.05 * np.sin(np.arange(T)[None, :] + field[:, None])
    mu = math.log(10000.0) + np.log(np.maximum(seq, 1)) - np.where(seq > 1, 0.3, 0.0)
    on = 120.0 + gains[:, None] * cyc * np.exp(rng.normal(mu, 0.18))
    off = rng.normal(120.0, 260.0, (n, T))
    vals = np.floor(np.where(seq > 0, on, off))
    words = ((seq > 0) * (1 << np.arange(T, dtype=np.uint64))[None, :]).sum(axis=1).astype(np.uint64)
    return vals, words, field


def time_fit(LN, torch, d_int, d_cat, d_len, means, reps):
    """(median ms, host outputs) of lognormal_device after one warm-up call."""
    out = LN.lognormal_device(d_int, d_cat, d_len, means, 0.2, 5, True, 3)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = LN.lognormal_device(d_int, d_cat, d_len, means, 0.2, 5, True, 3)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms), {k: v.cpu().numpy() for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=262144)
    ap.add_argument("--cycles", type=int, default=12)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--reference-ms", type=float, required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lognormal_summary.md"))
    a = ap.parse_args()
    import torch
    from fluorosequencingimageanalysis_amd import lognormal as LN
    n, T = a.tracks, a.cycles
    vals, words, field = make_tracks(n, T)
    alpha, ddif = 120.0, [0.0] + [0.3] * 6
    d_cat = torch.from_numpy(words.view(np.int64)).cuda()
    d_len = torch.full((n,), T, dtype=torch.int32, device="cuda")
    rows = []
    # first fit: alpha-adjusted intensities, beta from the last ON frames (here: the generator's 10 000)
    beta0 = 10000.0
    means0 = [math.log(beta0) + math.log(i + 1.0) - ddif[i] for i in range(7)]
    r0 = time_fit(LN, torch, torch.from_numpy(vals - alpha).cuda(), d_cat, d_len, means0, a.reps)
    rows.append(("first fit (alpha-adjusted)",) + r0)
    # second fit: every frame but the last scaled by its (cycle, field)'s median last-ON intensity, as ON_OFF_adjust_photometries
    h = r0[3]
    on = (words[:, None] >> np.arange(T, dtype=np.uint64)[None, :]) & np.uint64(1)
    last_on = (on[:, :-1] == 1) & (on[:, 1:] == 0) & (h["status"] == 0)[:, None]
    med = np.full((T, 3), np.nan)
    for c in range(T - 1):
        for fld in range(3):
            sel = last_on[:, c] & (field == fld)
            if sel.any():
                med[c, fld] = np.median(vals[sel, c])
    overall = float(np.nanmedian(med))
    scale = overall / med[np.arange(T)[None, :], field[:, None]]
    adj = np.where(np.isfinite(scale) & (np.arange(T)[None, :] < T - 1), (vals - alpha) * scale, vals)
    lastdrop = np.log(adj[:, :-1][last_on & (adj[:, :-1] > 0)])
    hist, bins = np.histogram(lastdrop, bins=200)
    beta1 = math.exp(0.5 * (bins[np.argmax(hist)] + bins[np.argmax(hist) + 1]))
    means1 = [math.log(beta1) + math.log(i + 1.0) - ddif[i] for i in range(7)]
    r1 = time_fit(LN, torch, torch.from_numpy(np.ascontiguousarray(adj)).cuda(), d_cat, d_len, means1, a.reps)
    rows.append(("second fit (ON/OFF-adjusted)",) + r1)
    lines = ["# Lognormal fluor-count fit (`tools/bench_lognormal.py`)", "",
             "%d tracks x %d cycles, max_possible=5, max_deviation=3, beta_sigma=0.2, multi-drop allowed; device events around"
             % (n, T), "`lognormal.lognormal_device` after a warm-up call, median (min-max) of %d calls on one %s." %
             (a.reps, torch.cuda.get_device_name(0)), "",
             "| fit | ms | tracks/s | with a sequence | surviving sequences per track (mean / max) | sequences/s |", "|---|---|---|---|---|---|"]
    for name, ms, lo, hi, host in rows:
        surv = host["n_surviving"]
        lines.append("| %s | %.3f (%.3f-%.3f) | %.3g | %.1f %% | %.1f / %d | %.3g |" %
                     (name, ms, lo, hi, n / ms * 1e3, 100.0 * (host["status"] == 0).mean(), surv.mean(), surv.max(), surv.sum() / ms * 1e3))
    ms0 = rows[0][1]
    lines += ["", "The reference (`_photometries_lognormal_fit_MP_v8` through its `multiprocessing.Pool`, as `tools/gen_lognormal_golden.py`",
              "prints it for fixture (b): 444 tracks of 8 cycles, every core of the build container's CPU): %.2f ms per track, %.3g tracks/s; the first fit above is"
              % (a.reference_ms, 1e3 / a.reference_ms), "%.3g times that, at 12 cycles instead of 8." % (n / ms0 * 1e3 / (1e3 / a.reference_ms)), ""]
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
