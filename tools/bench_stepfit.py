"""Step-fit throughput (traces/s) at 65 536 traces x 256 frames, mirror_start=3, chung_kennedy 0 and 1.

Three ways, one JSON line per configuration:
  device   fsq_stepfit_traces on device-resident inputs and outputs (device events, after a warm-up)
  records  stepfit_records from host arrays (copies in and out included; wall clock)
  objects  stepfit_photometries (the reference's 4-tuples of Trace objects; wall clock)

  python tools/bench_stepfit.py [--traces N] [--frames F] [--reps R]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def traces(n, frames, seed=0):
    rng = np.random.default_rng(seed)
    lvl = np.zeros((n, frames))
    nf = rng.integers(0, 5, n)
    for k in range(4):
        at = rng.integers(0, frames, n)
        lvl += (np.arange(frames)[None, :] < at[:, None]) * (k < nf)[:, None]
    v = lvl * rng.uniform(5e3, 3e4, (n, 1)) + rng.normal(0, 1, (n, frames)) * rng.uniform(1e3, 6e3, (n, 1))
    return np.round(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traces", type=int, default=65536)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from fluorosequencingimageanalysis_amd import stepfitting as S
    rows = traces(a.traces, a.frames)
    lens = np.full(a.traces, a.frames, np.int32)
    d_rows, d_lens = torch.from_numpy(rows).cuda(), torch.from_numpy(lens).cuda()
    for ck in (0, 1):
        prm = S._params(3, ck, 0.01, None)
        S.run_device(d_rows, d_lens, a.frames, prm)                     # warm-up
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = S.run_device(d_rows, d_lens, a.frames, prm)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 1e3)
            del out
        dev_s = float(np.median(ts))
        S.stepfit_records(rows, mirror_start=3, chung_kennedy=ck)
        t0 = time.perf_counter()
        S.stepfit_records(rows, mirror_start=3, chung_kennedy=ck)
        rec_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        S.stepfit_photometries(rows, mirror_start=3, chung_kennedy=ck)
        obj_s = time.perf_counter() - t0
        print(json.dumps({"workload": "stepfit", "traces": a.traces, "frames": a.frames, "mirror_start": 3, "chung_kennedy": ck,
                          "device_ms": round(dev_s * 1e3, 3), "device_traces_per_s": round(a.traces / dev_s),
                          "records_traces_per_s": round(a.traces / rec_s), "objects_traces_per_s": round(a.traces / obj_s)}))


if __name__ == "__main__":
    main()
