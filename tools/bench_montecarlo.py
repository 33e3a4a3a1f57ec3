"""Times the seeded Monte-Carlo PSF fit at N_iter = 1000 on the benchmark's field shape (512x512 uint16 fields of
~500 spots, bench.py's workload).  Two figures: the fit kernel alone (fsq_mc_fit_candidates on the candidates fsq_detect
finds, device events, median of --reps) and the whole path (pflib.find_peptides_records(fit_type='monte_carlo'): upload,
detect, fit, consolidate, records back; wall clock between two synchronisations, median of --reps).  Writes
profiles/montecarlo_summary.md.

  python tools/bench_montecarlo.py [--fields F --n-iter N --reps R --reference-ms MS --out FILE]

--reference-ms: the reference's time per candidate at N_iter = 1000 as tools/gen_montecarlo_golden.py measures it (one CPU
core, numpy's own generator); by default the figure that generator stored in tests/golden/montecarlo.npz."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spots", type=int, default=500)
    ap.add_argument("--n-iter", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--reference-ms", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "montecarlo_summary.md"))
    a = ap.parse_args()
    import torch
    from fluorosequencingimageanalysis_amd import _native_montecarlo as NM
    from fluorosequencingimageanalysis_amd import engine, pflib, synth
    ref_ms = a.reference_ms
    if ref_ms is None:
        ref_ms = float(np.load(os.path.join(ROOT, "tests", "golden", "montecarlo.npz"))["reference_ms_per_candidate"])
    imgs = np.stack([synth.make_field(s, (a.size, a.size), a.spots) for s in range(a.fields)])
    dev = torch.device("cuda:%d" % torch.cuda.current_device())
    d_img = engine.to_device_u16(imgs, dev)
    eng = engine.Engine(a.fields, a.size, a.size, fit_workspace=False)
    prm = engine.detect_params(5, engine.DEFAULT_CORRELATION_MATRIX, 2)
    total = eng.detect(d_img, prm)
    cand = torch.from_numpy(np.ascontiguousarray(eng.candidates(total)[0], dtype=np.int32)).to(dev)
    n = int(cand.shape[0])
    rows = torch.empty((n, 128), dtype=torch.uint8, device=dev)
    fit = torch.empty((n, 25), dtype=torch.float64, device=dev)
    rms = torch.empty(n, dtype=torch.float64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)

    def kernel():
        engine.launch(NM.lib().fsq_mc_fit_candidates, "fsq_mc_fit_candidates", dev, d_img.data_ptr(), a.fields, a.size, a.size,
                      cand.data_ptr(), n, a.n_iter, a.seed, 0, rows.data_ptr(), fit.data_ptr(), rms.data_ptr(), status.data_ptr())
    kernel()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        kernel()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    k_ms = statistics.median(ms)
    failing = int((status != 0).sum().item())
    path = []
    for _ in range(a.reps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        rec, counts, _ = pflib.find_peptides_records(imgs, fit_type='monte_carlo', N_iter=a.n_iter, seed=a.seed)
        torch.cuda.synchronize()
        path.append((time.perf_counter() - t) * 1e3)
    p_ms = statistics.median(path[1:])
    name = torch.cuda.get_device_name(dev)
    lines = [
        "# Seeded Monte-Carlo PSF fit: one run",
        "",
        "`python tools/bench_montecarlo.py --fields %d --n-iter %d --reps %d` on %s." % (a.fields, a.n_iter, a.reps, name),
        "%d fields of %dx%d with %d spots each (bench.py's field shape): %d candidates, %d of them with a failing fit status;"
        % (a.fields, a.size, a.size, a.spots, n, failing),
        "%d peaks kept at the default r_2_threshold (the image measured is the last iteration's, DESIGN §4.22)." % int(np.maximum(counts, 0).sum()),
        "",
        "| what | time | candidates/s | trials/s |",
        "|---|---|---|---|",
        "| fit kernel alone (`fsq_mc_fit_candidates`, device events, median of %d; all runs: %s ms) | %.2f ms | %.3g | %.3g |"
        % (a.reps, ", ".join("%.2f" % x for x in ms), k_ms, n / k_ms * 1e3, n * a.n_iter / k_ms * 1e3),
        "| whole path (`find_peptides_records(fit_type='monte_carlo')`: upload, detect, fit, consolidate, records back; wall, "
        "median of %d after a warm-up; all runs: %s ms) | %.2f ms | %.3g | %.3g |"
        % (a.reps, ", ".join("%.1f" % x for x in path[1:]), p_ms, n / p_ms * 1e3, n * a.n_iter / p_ms * 1e3),
        "| the reference, one CPU core, numpy's generator (tools/gen_montecarlo_golden.py) | %.1f ms per candidate | %.3g | %.3g |"
        % (ref_ms, 1e3 / ref_ms, a.n_iter * 1e3 / ref_ms),
        "",
        "Kernel against the reference's single core: %.0f times the candidates per second." % ((n / k_ms * 1e3) / (1e3 / ref_ms)),
        "One trial is 3+ Philox blocks, 3 logs, 1 pow, 25 exps, 50 fp64 divisions and a square root.",
        "",
    ]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
