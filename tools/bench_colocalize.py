"""Times the colocalisation of tracks between colour channels:

  * `fsq_colocalize_match` alone: bare launches into buffers allocated beforehand (device events), --fields fields x --tracks
    tracks per channel, K = 2, radius 2, about 90 % of the second channel's tracks a true partner within one pixel;
  * `colocalize.molecules_device` on the same tables (the launch plus the torch sorts, searches and the append);
  * `colocalize.joint_observed_records` end to end on a simulated two-letter experiment of 12 frames (--e2e-fields fields):
    the merge, both channels' lognormal chains and the joint tally, from NumPy tables to the dict;
  * the NumPy twin `_host_colocalize.match` on --twin-fields fields of the same size.

Wall clock between two synchronisations, median (min-max) of --reps calls after a warm-up call, unless the row says device
events.  Writes profiles/colocalize_summary.md.

  python tools/bench_colocalize.py [--fields N --tracks N --e2e-fields N --twin-fields N --reps R --seed S --out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEQUENCE, LABELS, MOCKS, EDMANS = "GAKCGAKC", "KC", 3, 8
SIDE = 1024                                                       # the fields' edge in pixels


def med(xs):
    return "%.3g (%.3g-%.3g)" % (float(np.median(xs)), min(xs), max(xs))


def two_channels(rng, fields, tracks):
    """(hw, field) of two channels: the first one's tracks anywhere in the field, the second one's 90 % partners within one pixel
    and 10 % others, in another order."""
    field = np.repeat(np.arange(fields, dtype=np.int64), tracks)
    a = rng.integers(2, SIDE - 2, (fields * tracks, 2))
    partner = rng.random(len(a)) < 0.9
    b = np.where(partner[:, None], a + rng.integers(-1, 2, a.shape), rng.integers(2, SIDE - 2, a.shape))
    order = np.lexsort((rng.random(len(a)), field))                 # (shuffled within every field)
    return (a.astype(np.int64), field), (b[order].astype(np.int64), field[order]), float(partner.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", type=int, default=256)
    ap.add_argument("--tracks", type=int, default=2048)
    ap.add_argument("--e2e-fields", type=int, default=64)
    ap.add_argument("--twin-fields", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colocalize_summary.md"))
    a = ap.parse_args()
    import torch
    from fluorosequencingimageanalysis_amd import _host_colocalize as H
    from fluorosequencingimageanalysis_amd import colocalize as CL
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS
    rng = np.random.default_rng(a.seed)
    dev = torch.device("cuda")

    def wall(call, reps):
        out = []
        for _ in range(reps + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = call()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t) * 1e3)
        return out[1:], res                                        # (the first call warms the allocator up)

    # ---- the kernel alone ----
    ta, tb, partners = two_channels(rng, a.fields, a.tracks)
    ids = np.arange(a.fields, dtype=np.int64)
    a_order, a_seg, a_off = H.grouped(ta[1], ids)
    b_order, _, b_off = H.grouped(tb[1], ids)
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).to(dev)              # noqa: E731
    args = (up(ta[0][a_order], np.int32), up(a_seg, np.int32), up(a_off, np.int64), up(tb[0][b_order], np.int32), up(b_off, np.int64))
    kernel = []
    for r in range(a.launches + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        out = CL._launch_match(*args, 4)
        t1.record()
        torch.cuda.synchronize()
        if r:
            kernel.append(t0.elapsed_time(t1))
    assert int(out[3]) == 0
    paired = float((out[0] >= 0).float().mean())
    n = a.fields * a.tracks
    d_tables = [(up(ta[0], np.int64), up(ta[1], np.int64)), (up(tb[0], np.int64), up(tb[1], np.int64))]
    merge, mols = wall(lambda: CL.molecules_device(d_tables, 2), a.reps)
    M = int(mols["member"].shape[1])
    del mols, d_tables, args, out

    # ---- the twin ----
    nt = a.twin_fields * a.tracks
    sel_a, sel_b = ta[1] < a.twin_fields, tb[1] < a.twin_fields
    ids_t = np.arange(a.twin_fields, dtype=np.int64)
    oa, sa, offa = H.grouped(ta[1][sel_a], ids_t)
    ob, _, offb = H.grouped(tb[1][sel_b], ids_t)
    twin = []
    for _ in range(3):
        t = time.perf_counter()
        H.match(ta[0][sel_a][oa], sa, offa, tb[0][sel_b][ob], offb, 4)
        twin.append((time.perf_counter() - t) * 1e3)

    # ---- joint_observed_records end to end ----
    m = a.e2e_fields * a.tracks
    ddif = [0, 0.3] + [0.3] * 5
    rec = PS.multilabel_records(SEQUENCE, LABELS, MOCKS, EDMANS, m, seed=a.seed, p=0.9, b=0.1, u=0.2, s=0.1, sc=3, s2=0.05,
                                beta={"K": 70000.0, "C": 40000.0}, beta_sigma=0.2, ddif=ddif)
    F = int(rec["counts"].shape[2])
    field = np.repeat(np.arange(a.e2e_fields, dtype=np.int64), a.tracks)
    pos = rng.integers(2, SIDE - 2, (m, 2))
    tables = {}
    for k, L in enumerate(rec["labels"]):
        at = np.flatnonzero(rec["counts"][k][:, 0] != 0)
        hw = pos[at] + (rng.integers(-1, 2, (len(at), 2)) if k else 0)
        tables[L] = (np.rint(rec["intensity"][k][at]), rec["category"][k][at], field[at], hw.astype(np.int64), np.arange(1, len(at) + 1))
    e2e, res = wall(lambda: CL.joint_observed_records(tables, 0.2, radius=2, solver='dp', table_slots=1 << 14), min(a.reps, 3))
    sizes = ", ".join("%s %d" % (L, len(tables[L][0])) for L in tables)

    k_med = float(np.median(kernel))
    lines = ["# Colocalisation of tracks between colour channels (`tools/bench_colocalize.py`)", "",
             "One run on one %s; nobody had measured this kernel before, and nothing here is a target.  Fields of %d x %d pixels," %
             (torch.cuda.get_device_name(0), SIDE, SIDE),
             "%d tracks per field and channel, K = 2, radius 2 (radius_sq = 4); %.1f %% of the second channel's tracks have a partner" %
             (a.tracks, 100 * partners),
             "within one pixel in the first, the others stand anywhere; seed %d.  %.1f %% of the first channel's tracks came out paired." %
             (a.seed, 100 * paired), "",
             "| what | size | runs | ms, median (min-max) | tracks/s |", "|---|---|---|---|---|",
             "| `fsq_colocalize_match`, bare launch (device events; the two memsets included) | %d fields, %d + %d tracks | %d | %s | %.3g |" %
             (a.fields, n, n, len(kernel), med(kernel), n / k_med * 1e3),
             "| `molecules_device` (one launch, the torch sorts, searches and the append; %d molecules) | the same | %d | %s | %.3g |" %
             (M, len(merge), med(merge), n / float(np.median(merge)) * 1e3),
             "| `_host_colocalize.match`, the NumPy twin | %d fields, %d + %d tracks | %d | %s | %.3g |" %
             (a.twin_fields, nt, nt, len(twin), med(twin), nt / float(np.median(twin)) * 1e3),
             "| `joint_observed_records`, end to end, %d frames | %d fields, %d molecules simulated, tracks: %s | %d | %s | %.3g |" %
             (F, a.e2e_fields, m, sizes, len(e2e), med(e2e), sum(len(t[0]) for t in tables.values()) / float(np.median(e2e)) * 1e3), "",
             "The kernel is the brute force of DESIGN §4.30: every lane reads its field's %d positions of the other channel and, where it" % a.tracks,
             "found a partner, up to %d of its own.  Per launch that is %.3g distance evaluations at the least, %.3g per second." %
             (a.tracks, float(n) * a.tracks, float(n) * a.tracks / k_med * 1e3),
             "End to end, `%s` labelled at `%s`, %d mocks + %d Edmans: %d molecules, %d rejected, %d distinct joint signals, none_count %d." %
             (SEQUENCE, LABELS, MOCKS, EDMANS, res["n_molecules"], res["n_rejected"], len(res["signals"]), res["none_count"]),
             "End to end is the merge, the two lognormal chains (lognormal.chain_records with solver='dp': the tables go up, the fits come",
             "back as NumPy arrays) and the joint tally.", ""]
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
