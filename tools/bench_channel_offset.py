"""Times the estimate of the integer offset between two colour channels, on bench_colocalize.py's tables:
--fields fields x --tracks tracks per channel in fields of 1 024 x 1 024, about 90 % of the second channel's tracks a true
partner within one pixel, the second channel moved by --shift:

  * `fsq_channel_offset_votes` alone at W = 18 (max_shift 16, radius 2) and at W = 64: bare launches into buffers allocated
    beforehand (device events; the two memsets included);
  * `fsq_colocalize_match` on the same tables in the same session: it walks the same pairs, so the difference is the price of
    voting, of clearing the LDS histogram and of the flush;
  * `fsq_channel_offset_peak` alone at (W, R, tol_sq) = (18, 16, 4) and (64, 60, 16);
  * `colocalize.estimate_offsets_records` end to end, from NumPy tables to the offsets (wall clock);
  * the NumPy twin `_host_channel_offset.votes` on --twin-fields fields of the same size.

Device events, median (min-max) of --launches launches after a warm-up launch, unless the row says wall clock.  Writes
profiles/channel_offset_summary.md.

  python tools/bench_channel_offset.py [--fields N --tracks N --twin-fields N --launches L --reps R --seed S --out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_colocalize import SIDE, med, two_channels              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", type=int, default=256)
    ap.add_argument("--tracks", type=int, default=2048)
    ap.add_argument("--twin-fields", type=int, default=8)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shift", type=int, nargs=2, default=(5, -7))
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "channel_offset_summary.md"))
    a = ap.parse_args()
    import torch
    from fluorosequencingimageanalysis_amd import _host_channel_offset as HO
    from fluorosequencingimageanalysis_amd import _host_colocalize as H
    from fluorosequencingimageanalysis_amd import colocalize as CL
    rng = np.random.default_rng(a.seed)
    dev = torch.device("cuda")
    shift = np.array(a.shift)
    ta, tb, partners = two_channels(rng, a.fields, a.tracks)
    tb = (tb[0] - shift, tb[1])                                    # (so `shift` is what has to be added to the second channel)
    ids = np.arange(a.fields, dtype=np.int64)
    a_order, a_seg, a_off = H.grouped(ta[1], ids)
    b_order, _, b_off = H.grouped(tb[1], ids)
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).to(dev)              # noqa: E731
    args = (up(ta[0][a_order], np.int32), up(a_seg, np.int32), up(a_off, np.int64), up(tb[0][b_order], np.int32), up(b_off, np.int64))
    n = a.fields * a.tracks

    def events(call):
        out = []
        for r in range(a.launches + 1):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            res = call()
            t1.record()
            torch.cuda.synchronize()
            if r:
                out.append(t0.elapsed_time(t1))
        return out, res

    votes = {}
    for W in (18, 64):
        votes[W], (d_V, d_bad) = events(lambda: CL._launch_votes(*args, W))
        assert int(d_bad) == 0
        votes[W] = (votes[W], d_V)
    match, out = events(lambda: CL._launch_match(*args, 4))
    assert int(out[3]) == 0
    peaks = {}
    for W, R, tol_sq in ((18, 16, 4), (64, 60, 16)):
        peaks[W], d_rec = events(lambda: CL.offset_peak_device(votes[W][1], R, tol_sq))
        rec = d_rec.cpu().numpy()
        # (under tol_sq 16 every offset within two pixels of the shift covers the whole cluster of +-1: noise picks among them)
        assert max(abs(int(rec[0]) - a.shift[0]), abs(int(rec[1]) - a.shift[1])) <= (0 if tol_sq == 4 else 2), rec
        peaks[W] = (peaks[W], rec, R, tol_sq)
    rec = peaks[18][1]
    in_window = {W: int(votes[W][1].sum()) for W in votes}
    nonzero = {W: int((votes[W][1] != 0).sum()) for W in votes}

    e2e = []
    for _ in range(a.reps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        offsets, _ = CL.estimate_offsets_records([ta, tb], 2)
        torch.cuda.synchronize()
        e2e.append((time.perf_counter() - t) * 1e3)
    e2e = e2e[1:]
    assert offsets == [(0, 0), tuple(a.shift)]

    nt = a.twin_fields * a.tracks
    sel_a, sel_b = ta[1] < a.twin_fields, tb[1] < a.twin_fields
    ids_t = np.arange(a.twin_fields, dtype=np.int64)
    oa, sa, offa = H.grouped(ta[1][sel_a], ids_t)
    ob, _, offb = H.grouped(tb[1][sel_b], ids_t)
    twin = []
    for _ in range(3):
        t = time.perf_counter()
        HO.votes(ta[0][sel_a][oa], sa, offa, tb[0][sel_b][ob], offb, 18)
        twin.append((time.perf_counter() - t) * 1e3)

    pairs = float(n) * a.tracks
    m_med = float(np.median(match))
    row = "| %s | %s | %d | %s | %s |"
    lines = ["# The offset between two colour channels (`tools/bench_channel_offset.py`)", "",
             "One session on one %s; nobody had measured these kernels before, and nothing here is a target.  Fields of %d x %d pixels," %
             (torch.cuda.get_device_name(0), SIDE, SIDE),
             "%d fields of %d tracks per channel (%d + %d tracks, %.3g pairs of one field), %.1f %% of the second channel's tracks a partner" %
             (a.fields, a.tracks, n, n, pairs, 100 * partners),
             "within one pixel, the second channel moved so that (%d, %d) brings it back; seed %d.  Device events around bare launches" %
             (a.shift[0], a.shift[1], a.seed),
             "unless the row says wall clock; median (min-max) after a warm-up call.", "",
             "| what | size | runs | ms, median (min-max) | pairs/s |", "|---|---|---|---|---|"]
    for W in (18, 64):
        lines.append(row % ("`fsq_channel_offset_votes`, W = %d (%d B of LDS per block; the two memsets included)" % (W, 4 * (2 * W + 1) ** 2),
                            "%d blocks; %d votes in %d of %d bins" % ((n + 255) // 256, in_window[W], nonzero[W], (2 * W + 1) ** 2),
                            len(votes[W][0]), med(votes[W][0]), "%.3g" % (pairs / float(np.median(votes[W][0])) * 1e3)))
    lines.append(row % ("`fsq_colocalize_match`, radius_sq 4, the same tables (its two memsets included)", "%d blocks" % ((n + 255) // 256),
                        len(match), med(match), "%.3g" % (pairs / m_med * 1e3)))
    for W in (18, 64):
        t, _, R, tol_sq = peaks[W]
        lines.append(row % ("`fsq_channel_offset_peak`, W = %d, R = %d, tol_sq = %d" % (W, R, tol_sq),
                            "one block; %d offsets x %d taps, twice" % ((2 * R + 1) ** 2, len(HO.taps(tol_sq))), len(t), med(t), "-"))
    lines.append(row % ("`estimate_offsets_records`, K = 2, radius 2, max_shift 16 (wall clock: checks, grouping by field, upload, two launches)",
                        "the same tables", len(e2e), med(e2e), "%.3g" % (pairs / float(np.median(e2e)) * 1e3)))
    lines.append(row % ("`_host_channel_offset.votes`, the NumPy twin, W = 18 (wall clock)", "%d fields, %d + %d tracks" % (a.twin_fields, nt, nt),
                        len(twin), med(twin), "%.3g" % (float(nt) * a.tracks / float(np.median(twin)) * 1e3)))
    lines += ["",
              "Voting against the walk alone: W = 18 takes %.2f times the match's time, W = 64 %.2f times (medians)." %
              (float(np.median(votes[18][0])) / m_med, float(np.median(votes[64][0])) / m_med),
              "The peak at W = 18: offset (%d, %d), score %d, runner-up %d, %d votes in the window, at_edge %d, n_ties %d." %
              tuple(int(x) for x in rec[:7]),
              "The peak at W = 64, tol_sq 16: offset (%d, %d), score %d, runner-up %d, %d votes, at_edge %d, n_ties %d (every offset within" %
              tuple(int(x) for x in peaks[64][1][:7]),
              "two pixels of the shift covers the whole +-1 cluster under that tolerance, so the background picks among them).", ""]
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
