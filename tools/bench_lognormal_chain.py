"""Times the lognormal chain on a track table at a user's size: 262 144 tracks x 12 cycles in three fields, drawn
as tools/bench_lognormal.py draws them, beta_sigma=0.2, max_possible=5, ddif=0.3.

  lognormal.chain_device     device events around the whole call (table on the device, results on the device) after a warm-up,
                             median (min-max) of --reps calls; and its three new entries alone, the same way
  lognormal.chain_records    wall clock, end to end: host arrays in, host arrays and the tally out
  the dict chain             what lognormal_fitter_v2 runs without --device_chain between reading the CSV and writing the files
                             (nested dicts of tuples, the fit and the bin searches on the device), wall clock, once, on the same
                             table (--dict-tracks M: on its first M tracks only, with chain_records on those tracks next to it)

Writes profiles/lognormal_chain_summary.md.

  python tools/bench_lognormal_chain.py [--tracks N --cycles T --reps R --dict-tracks M --out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KW = dict(max_possible=5, ddif=0.30, allow_multidrop=True, truncate=0)


def events(torch, fn, reps):
    """(median, min, max) ms of fn() by device events after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms)


def dict_chain(LN, photometries, device):
    """lognormal_fitter_v2.main's default computation between the reader and the files."""
    tracks = list(LN.unwind_photometries(photometries))
    raw = tuple([i for t in tracks for i in t[5]])
    alpha = LN._get_m0Dm1(raw_photometries=raw, optimal_bin_number=None, device=device)[7]
    alpha_adjusted, truncated = {}, {}
    for ch, field, h, w, category, intensities, row in tracks:
        alpha_adjusted.setdefault(ch, {}).setdefault(field, {}).setdefault((h, w), (category, tuple([i - alpha for i in intensities]), row))
        truncated.setdefault(ch, {}).setdefault(field, {}).setdefault((h, w), (category[0:], intensities[0:], row))
    beta0, _ = LN.last_drop_method_v2(photometries=truncated, device=device)
    ddif = tuple([0.0] + [KW["ddif"]] * (KW["max_possible"] + 1))
    fit_kw = dict(beta_sigma=0.2, max_possible=KW["max_possible"], allow_upsteps=False, allow_multidrop=True, max_deviation=3,
                  quench_factor=0, quench_factors=ddif, device=device)
    first = LN.photometries_lognormal_fit(photometries=alpha_adjusted, beta=beta0, **fit_kw)
    on_offs = LN.grab_ON_OFFS(first[3], alpha_adjust=0)
    adjusted = LN.ON_OFF_adjust_photometries(photometries=photometries, ON_OFFS=on_offs, alpha=alpha)
    beta1, _ = LN.last_drop_method_v2(photometries=adjusted, device=device)
    return alpha, beta0, beta1, LN.photometries_lognormal_fit(photometries=adjusted, beta=beta1, **fit_kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=262144)
    ap.add_argument("--cycles", type=int, default=12)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dict-tracks", type=int, default=0, help="0: all tracks")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lognormal_chain_summary.md"))
    a = ap.parse_args()
    import torch
    from bench_lognormal import make_tracks
    from fluorosequencingimageanalysis_amd import lognormal as LN
    n, T = a.tracks, a.cycles
    vals, words, field = make_tracks(n, T)
    order = np.argsort(field, kind='stable')
    seg_off = np.concatenate([[0], np.cumsum(np.bincount(field, minlength=3))]).astype(np.int64)
    d_int = torch.from_numpy(np.ascontiguousarray(vals[order])).cuda()
    d_cat = torch.from_numpy(np.ascontiguousarray(words[order]).view(np.int64)).cuda()
    d_off = torch.from_numpy(seg_off).cuda()

    out = {}
    say = lambda *what: print(*what, file=sys.stderr, flush=True)          # noqa: E731  (progress; the summary goes to stdout)
    say("table drawn: %d tracks x %d cycles" % (n, T))

    def whole():
        out["chain"] = LN.chain_device(d_int, d_cat, d_off, None, 0.2, **KW)
    chain_ms = events(torch, whole, a.reps)
    res = out["chain"]
    say("chain_device: %.2f ms" % chain_ms[0])
    alpha = float(res["alpha"])
    stages = [("`fsq_chain_last_drops` (two passes, `torch.cumsum` and the count's read-back between them)",
               events(torch, lambda: LN.last_drops_device(d_int, d_cat, 0), a.reps)),
              ("`fsq_chain_on_off_medians`", events(torch, lambda: out.__setitem__("med", LN.on_off_medians_device(
                  d_int, d_cat, d_off, res["fit0"]["status"], alpha)), a.reps))]
    stages.append(("`fsq_chain_on_off_adjust`", events(torch, lambda: LN.on_off_adjust_device(d_int, d_off, alpha, out["med"]), a.reps)))

    t0 = time.perf_counter()
    rec = LN.chain_records(vals, words, field, 0.2, device="cuda", **KW)
    records_s = time.perf_counter() - t0
    say("chain_records: %.3f s" % records_s)

    m = min(a.dict_tracks, n) if a.dict_tracks > 0 else n
    rec_m, records_m_s = rec, records_s
    if m < n:
        t0 = time.perf_counter()
        rec_m = LN.chain_records(vals[:m], words[:m], field[:m], 0.2, device="cuda", **KW)
        records_m_s = time.perf_counter() - t0
    photometries = {}
    for t in range(m):
        photometries.setdefault("ch1", {}).setdefault(int(field[t]), {})[(t, t)] = (
            tuple(bool((int(words[t]) >> f) & 1) for f in range(T)), tuple(int(x) for x in vals[t]), t + 1)
    t0 = time.perf_counter()
    d_alpha, d_beta0, d_beta1, (d_signals, d_total, d_none, _) = dict_chain(LN, photometries, "cuda")
    dict_s = time.perf_counter() - t0
    say("the dict chain on %d tracks: %.3f s" % (m, dict_s))
    same = (np.float64(d_alpha).tobytes() == np.float64(rec_m["alpha"]).tobytes()
            and np.float64(d_beta1).tobytes() == np.float64(rec_m["adj_beta"]).tobytes()
            and d_signals == rec_m["signals"] and (d_total, d_none) == (rec_m["total_count"], rec_m["none_count"]))

    lines = ["# Lognormal chain on a track table (`tools/bench_lognormal_chain.py`)", "",
             "%d tracks x %d cycles in 3 fields, drawn as `tools/bench_lognormal.py` draws them; beta_sigma=0.2, max_possible=5," % (n, T),
             "ddif=0.3, multi-drop allowed; one %s." % torch.cuda.get_device_name(0), "",
             "| what | how it is timed | time |", "|---|---|---|",
             "| `lognormal.chain_device`: table on the device to both fits on the device | device events, median (min-max) of %d "
             "calls after a warm-up | %.2f ms (%.2f-%.2f) |" % ((a.reps,) + chain_ms)]
    for name, ms in stages:
        lines.append("| %s alone | the same | %.3f ms (%.3f-%.3f) |" % ((name,) + ms))
    lines += ["| `lognormal.chain_records`: host arrays to host arrays and the tally | wall clock, once | %.3f s |" % records_s,
              ] + (["| `lognormal.chain_records` on the first %d tracks | wall clock, once | %.3f s |" % (m, records_m_s)] if m < n else []) + [
              "| the dict chain of `lognormal_fitter_v2` (the route before `--device_chain`; fits and bin searches on the device) on the "
              "%s | wall clock, once | %.3f s |" % ("same table" if m == n else "same %d tracks" % m, dict_s), "",
              "`chain_device`'s time holds its host round trips (the scalars and the histograms that cross between the steps), not",
              "only its kernels.  The result: alpha %.17g in %d bins, beta %.17g then %.17g; %d of %d tracks with a signal, %d keys in the tally."
              % (alpha, int(res["n_bins"]), float(res["original_beta"]), float(res["adj_beta"]),
                 rec["total_count"] - rec["none_count"], rec["total_count"], len(rec["signals"])),
              "On the %d tracks the dict chain and `chain_records` give %s alpha, second beta and tally." % (m, "the same" if same else "DIFFERENT"), ""]
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
