#!/usr/bin/env python3
"""Throughput of fsq_sequence_photometry (include/fsq_sequence.h) at the bench's scale: 1 024 sequences of 512 x 512, 500 traces
each, 16 frames, ~30 % of the (trace, frame) entries undetected, hat (radius 9, brim 6), interpolate on.

Device time: HIP events around the launch after a warm-up, median of 5 (min and max are reported as the spread).  Yardstick, in
the same process on the same frames: fsq_mexican_hat of include/fsq.h on exactly the windows the fused kernel measured.
Wall clock of the two Python routes on a subset of the sequences (--route-seqs): the records surface
(sequencing.sequence_photometry_records, host arrays in and out) and the objects surface
(MultifieldMultichannelSequenceExperiment.discard_invalid_traces on Image / Spot objects).  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fluorosequencingimageanalysis_amd import _native as N  # noqa: E402
from fluorosequencingimageanalysis_amd import flexlibrary as fl  # noqa: E402
from fluorosequencingimageanalysis_amd import sequencing as S  # noqa: E402


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def make_traces(rng, n_seq, per, F, H, W, holes):
    n = n_seq * per
    base = np.stack([rng.integers(2, H - 2, n), rng.integers(2, W - 2, n)], axis=1)
    off = np.round(rng.uniform(-1.5, 1.5, (n_seq, F, 2)) * 20) / 20
    off[:, 0] = 0
    seq = np.repeat(np.arange(n_seq, dtype=np.int32), per)
    cum = np.cumsum(off, axis=1)
    hw = np.rint(base[:, None, :] - cum[seq]).astype(np.int32)
    hw[..., 0] = np.clip(hw[..., 0], 2, H - 3)
    hw[..., 1] = np.clip(hw[..., 1], 2, W - 3)
    miss = rng.random((n, F)) < holes
    miss[np.arange(n), rng.integers(0, F, n)] = False           # every trace keeps a Spot
    hw[miss] = -1
    return hw, seq, off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=1024)
    ap.add_argument("--traces", type=int, default=500)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--holes", type=float, default=0.3)
    ap.add_argument("--route-seqs", type=int, default=16)
    a = ap.parse_args()
    n_seq, per, F, H, W = a.seqs, a.traces, a.frames, a.size, a.size
    rng = np.random.default_rng(0)
    dev = torch.device("cuda")
    d_frames = torch.randint(0, 4000, (n_seq, F, H, W), dtype=torch.int16, device=dev)
    hw, seq, off = make_traces(rng, n_seq, per, F, H, W, a.holes)
    d_hw, d_seq, d_off = torch.from_numpy(hw).to(dev), torch.from_numpy(seq).to(dev), torch.from_numpy(off).to(dev)

    keep = {}

    def fused():
        keep["o"] = S.run_device(d_frames, d_hw, d_seq, d_off, radius=9, brim_size=6, spot_size=5, interpolate=True)
    ms, lo, hi = timed(fused)
    o = keep["o"]
    have = (o["flags"] & 3) != 0
    n_windows = int(have.sum().item())

    # the yardstick on the same windows
    idx = have.nonzero()
    frame_index = (d_seq[idx[:, 0]].to(torch.int64) * F + idx[:, 1]).to(torch.int32)
    d_fhw = torch.cat([frame_index[:, None], o["hw"][idx[:, 0], idx[:, 1]]], dim=1).contiguous()
    d_out = torch.empty(n_windows, dtype=torch.float64, device=dev)
    L, s = N.lib(), torch.cuda.current_stream().cuda_stream

    def yardstick():
        N.check(L.fsq_mexican_hat(d_frames.data_ptr(), n_seq * F, H, W, d_fhw.data_ptr(), n_windows, 6, 9, d_out.data_ptr(), s), "mh")
    y_ms, y_lo, y_hi = timed(yardstick)
    same = bool(torch.equal(d_out.view(torch.int64), o["photometry"][idx[:, 0], idx[:, 1]].view(torch.int64)))

    def counts():
        keep["c"] = S.category_counts_device(o["category"], d_seq)
    c_ms, _, _ = timed(counts)
    n_groups = int(keep["c"][4].item())

    # the Python routes on a subset
    k = min(a.route_seqs, n_seq)
    sub = slice(0, k * per)
    frames_host = d_frames[:k].cpu().numpy().view(np.uint16)
    S.sequence_photometry_records(frames_host[:1], hw[:per], seq[:per], off[:1])
    t0 = time.perf_counter()
    S.sequence_photometry_records(frames_host, hw[sub], seq[sub], off[:k])
    records_s = time.perf_counter() - t0
    fields = []
    for q in range(k):
        images = [fl.Image(image=frames_host[q, f]) for f in range(F)]
        ex = fl.SequenceExperiment(peptide_frames=images)
        ex.offsets = [(0, 0)] + [(float(x), float(y)) for x, y in off[q, 1:]]
        ex.spot_traces = [[fl.Spot(images[f], int(h), int(w), 5) if h >= 0 else None for f, (h, w) in enumerate(row)]
                          for row in hw[q * per:(q + 1) * per]]
        fields.append(fl.MultichannelSequenceExperiment({"ch1": ex}))
    m = fl.MultifieldMultichannelSequenceExperiment(fields)
    t0 = time.perf_counter()
    m.discard_invalid_traces()
    objects_s = time.perf_counter() - t0
    entries = k * per * F
    print(json.dumps({
        "metric": "sequence_windows_per_sec", "value": n_windows / (ms * 1e-3), "device_ms": ms, "device_ms_min": lo,
        "device_ms_max": hi, "sequences": n_seq, "traces": n_seq * per, "frames": F, "entries": n_seq * per * F, "windows": n_windows,
        "ns_per_window": ms * 1e6 / n_windows,
        "yardstick": {"kernel": "fsq_mexican_hat", "ms": y_ms, "ms_min": y_lo, "ms_max": y_hi, "ns_per_window": y_ms * 1e6 / n_windows,
                      "spots_per_sec": n_windows / (y_ms * 1e-3), "photometries_identical": same},
        "ratio_to_yardstick": ms / y_ms,
        "category_counts": {"device_ms": c_ms, "groups": n_groups},
        "routes": {"sequences": k, "entries": entries, "records_s": records_s, "records_us_per_entry": records_s * 1e6 / entries,
                   "objects_s": objects_s, "objects_us_per_entry": objects_s * 1e6 / entries},
        "roofline": {"bound": "hbm", "achieved": n_windows * (361 * 2 + 8) / (ms * 1e-3) / 1e9, "peak": 8000.0, "unit": "GB/s"}}))


if __name__ == "__main__":
    main()
