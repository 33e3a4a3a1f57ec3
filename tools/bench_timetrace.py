"""Measures the timetrace experiment table on one GPU (results: profiles/timetrace_summary.md).

Three measurements, each in a child process of its own under its own time limit; the first that fails ends the run:

  table     fsq_timetrace_table alone, 65 536 traces x 256 frames with four plateaus each: device events around `--repeats`
            launches after two warm-up launches
  records   timetrace.timetrace_records end to end (upload, tracking, photometry, step fit, table, download), 4 096 spots x
            1 000 frames of 256 x 256: a host clock around the call, which ends in the download, after a warm-up call on 32 frames
  objects   the object path (TimetraceExperiment.lc_create_traces + stepfit_tracks) and timetrace_records on the same 256 spots x
            100 frames of 256 x 256, alternating, best of three each

  python tools/bench_timetrace.py [--out FILE] [--parts table,records,objects] [--small]

Every part prints one JSON line; --out appends them to a file.  --small shrinks every shape (a rehearsal of the tool)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"table": 240, "records": 420, "objects": 300}               # seconds per child


def synthetic_stack(n_frames, n_side, size=256, seed=1):
    """uint16 frames of n_side^2 spots on a grid, in four groups that each lose one of two fluors at its own frame."""
    import numpy as np
    rng = np.random.default_rng(seed)
    pos = np.unique(np.rint(np.linspace(10, size - 11, n_side)).astype(np.int32))
    assert len(pos) == n_side
    hw = np.array([(h, w) for h in pos for w in pos], np.int32)
    yy, xx = np.mgrid[-3:4, -3:4]
    stamp = 400.0 * np.exp(-(yy ** 2 + xx ** 2) / (2 * 1.2 ** 2))
    groups = np.zeros((4, size, size))
    for i, (h, w) in enumerate(hw):
        groups[i % 4, h - 3:h + 4, w - 3:w + 4] += stamp
    bleach = [n_frames // 5, 2 * n_frames // 5, 3 * n_frames // 5, 4 * n_frames // 5]
    frames = np.empty((n_frames, size, size), np.uint16)
    for f in range(n_frames):
        img = rng.normal(120.0, 12.0, (size, size))
        for g in range(4):
            img += groups[g] * (2.0 if f < bleach[g] else 1.0)
        frames[f] = np.clip(np.rint(img), 0, 65535)
    return frames, hw


def part_table(small, repeats):
    import numpy as np
    import torch
    from fluorosequencingimageanalysis_amd import timetrace as TT
    n, F = (4096, 256) if small else (65536, 256)
    rng = np.random.default_rng(2)
    cuts = np.stack([32 + rng.integers(0, 32, n), 96 + rng.integers(0, 32, n), 160 + rng.integers(0, 64, n)], axis=1)
    start = np.zeros((n, F), np.int32)
    stop = np.zeros((n, F), np.int32)
    start[:, 1:4] = cuts
    stop[:, :3] = cuts - 1
    stop[:, 3] = F - 1
    level = np.zeros((n, F))
    frame = np.arange(F)[None]
    for k in range(3):
        level += (frame >= cuts[:, k:k + 1]) * -9000.0
    phot = 40000.0 + level + rng.normal(0.0, 3000.0, (n, F))
    h = np.zeros((n, F))
    edges = np.concatenate([np.zeros((n, 1), np.int64), cuts, np.full((n, 1), F)], axis=1)
    for k in range(4):
        m = (frame >= edges[:, k:k + 1]) & (frame < edges[:, k + 1:k + 2])
        h[:, k] = (phot * m).sum(axis=1) / m.sum(axis=1)
    dev = torch.device("cuda")
    args = [torch.from_numpy(a).to(dev) for a in (phot, np.full(n, F, np.int32), start, stop, h, np.full(n, 4, np.int32))]
    out = TT.table_out(n, F, dev)
    for _ in range(2):
        TT.table_device(*args, out=out)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(repeats):
        TT.table_device(*args, out=out)
    ev[1].record()
    torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1]) / repeats
    assert int(out["status"].count_nonzero()) == 0
    bytes_per_frame = 8 + 8 + 8 + 4 + 4 + 4                            # photometry read; two double and three int32 columns written
    return {"part": "table", "traces": n, "frames": F, "plateaus": 4, "repeats": repeats, "ms_per_launch": ms,
            "traces_per_s": n / ms * 1e3, "frames_per_s": n * F / ms * 1e3, "column_GB_per_s": n * F * bytes_per_frame / ms / 1e6}


def part_records(small, repeats):
    from fluorosequencingimageanalysis_amd import timetrace as TT
    n_frames, n_side = (64, 16) if small else (1000, 64)
    frames, hw = synthetic_stack(n_frames, n_side)
    TT.timetrace_records(frames[:32], hw)                               # (code objects, allocator)
    t0 = time.perf_counter()
    rec = TT.timetrace_records(frames, hw)
    dt = time.perf_counter() - t0
    assert (rec["status"] == 0).all()
    return {"part": "records", "spots": len(hw), "frames": n_frames, "image": list(frames.shape[1:]), "seconds": dt,
            "spot_frames_per_s": len(hw) * n_frames / dt, "present_fraction": float(rec["present"].mean()),
            "plateaus_per_trace": float(rec["tf_n"].mean())}


def part_objects(small, repeats):
    import numpy as np
    from fluorosequencingimageanalysis_amd import flexlibrary as fl
    from fluorosequencingimageanalysis_amd import timetrace as TT
    n_frames, n_side = (16, 8) if small else (100, 16)
    frames, hw = synthetic_stack(n_frames, n_side)

    def objects():
        imgs = [fl.Image(image=f) for f in frames]
        ex = fl.TimetraceExperiment(imgs)
        ex.lc_create_traces(initial_spots=[fl.Spot(imgs[0], int(h), int(w), 5) for h, w in hw], search_radius=3)
        ex.stepfit_tracks()
        return ex

    objects()
    TT.timetrace_records(frames, hw)
    t_obj, t_rec = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        ex = objects()
        t_obj.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        rec = TT.timetrace_records(frames, hw)
        t_rec.append(time.perf_counter() - t0)
    for t, tr in enumerate(ex.spot_traces):                            # the two paths fit the same plateaus
        k = int(rec["tf_n"][t])
        assert [(a, o) for a, o, _ in ex.step_fits[(tr.h, tr.w)].trace] == list(zip(rec["tf_start"][t, :k].tolist(), rec["tf_stop"][t, :k].tolist()))
    return {"part": "objects", "spots": len(hw), "frames": n_frames, "object_path_seconds": min(t_obj), "records_seconds": min(t_rec),
            "object_path_spot_frames_per_s": len(hw) * n_frames / min(t_obj), "records_spot_frames_per_s": len(hw) * n_frames / min(t_rec),
            "all_object_path_seconds": t_obj, "all_records_seconds": t_rec}


PARTS = {"table": part_table, "records": part_records, "objects": part_objects}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parts", default="table,records,objects")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        import torch
        assert torch.cuda.is_available(), "bench_timetrace needs a GPU"
        print(json.dumps(PARTS[a.child](a.small, a.repeats)), flush=True)
        return 0
    for part in a.parts.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", part, "--repeats", str(a.repeats)] + (["--small"] if a.small else [])
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True, timeout=LIMITS[part])
        except subprocess.TimeoutExpired:
            print("part %s ran into its limit of %d s; stopping" % (part, LIMITS[part]), file=sys.stderr)
            return 124
        if r.returncode != 0:
            print("part %s failed with status %d; stopping" % (part, r.returncode), file=sys.stderr)
            return r.returncode or 1
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
