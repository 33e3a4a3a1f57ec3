"""Writes tests/golden/stepfit_traces.npz (seeded synthetic bleaching traces through the reference's step fit) and
tests/golden/stepfit_timetrace.npz (a synthetic frame stack through TimetraceExperiment.lc_create_traces + stepfit_tracks).

Loads the reference at run time through oracle/refload.py (as oracle/gen_golden.py does) and runs
Trace.stepfit_photometries (flexlibrary.py:1380-1462) - or, for the window_radius / drop_sort variants the live path does
not reach, the same sequence of stepfitting_library calls with those arguments.  Every ttest_ind p is recorded; a seed is
rejected when a p lies within 1e-8 (relative) of the threshold or two distinct sorted p lie within 1e-8 of each other.

  python tools/gen_stepfit_golden.py [--reference DIR]
"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-8


def synth_trace(rng, n, kind):
    n_fluors = int(rng.integers(0, 5))
    step = rng.uniform(5e3, 3e4)
    noise = rng.uniform(1e3, 6e3)
    level = np.full(n, float(n_fluors))
    for k in range(n_fluors):
        level[int(rng.integers(0, max(n, 1))):] -= 1.0
    v = level * step + rng.normal(0.0, noise, n)
    if kind == "half":
        v = np.round(v * 2.0) / 2.0
    else:
        v = np.round(v)
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("FSQ_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "stepfit_traces.npz"))
    ap.add_argument("--limits", action="store_true",
                    help="write only tests/golden/stepfit_limits.npz (traces at the 8192-frame limit); the other fixtures stay")
    a = ap.parse_args()
    os.environ["FSQ_REFERENCE"] = a.reference
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import refload
    refload.REF = a.reference
    ref = refload.load_reference()
    sf = refload.load("stepfitting_library", "stepfitting_library.py")
    fl = refload.load_flexlibrary(ref).fl
    real_ttest = sf.ttest_ind
    rec = []

    def ttest_rec(x, y, equal_var=True):
        r = real_ttest(x, y, equal_var=equal_var)
        rec.append(float(r[1]))
        return r
    sf.ttest_ind = ttest_rec

    class Stub:
        def __init__(self, v):
            self.v = v

        def photometry(self, method=None, **kw):
            return self.v

    if a.limits:
        return gen_limits(sf, fl, rec, Stub, os.path.join(os.path.dirname(a.out), "stepfit_limits.npz"))

    # (length, kind, mirror, ck, window_radius, drop_sort, thr, special)
    cases = []
    for n in range(1, 9):
        cases.append((n, "int", 0, 0, 6, True, 0.01, ""))
        cases.append((n, "half", 3, 0, 20, True, 0.01, ""))
    for n in (3, 5, 8):
        cases.append((n, "int", 0, 1, 6, True, 0.01, ""))
    for mirror in (0, 3, 7):
        for ck in (0, 1, 2):
            cases.append((50, "int", mirror, ck, 6, True, 0.01, ""))
            cases.append((200, "half", mirror, ck, 6, True, 0.001, ""))
    for wr in (6, 20):
        for ds in (True, False):
            for thr in (0.01, 0.001):
                cases.append((200, "int", 3, 1, wr, ds, thr, ""))
    cases += [(200, "int", 3, 0, 6, True, 0.01, "dropout"), (200, "int", 3, 1, 6, True, 0.01, "dropout"),
              (200, "int", 3, 0, 6, True, 0.01, "clamp"), (50, "int", 0, 1, 6, True, 0.01, "clamp"),
              (50, "int", 3, 0, 6, True, 0.01, "constant"), (50, "int", 3, 1, 6, True, 0.01, "constant"),
              (200, "half", 3, 0, 6, True, 0.01, "nan"), (200, "half", 3, 1, 6, False, 0.01, "nan"),
              (1000, "int", 3, 0, 6, True, 0.01, ""), (1000, "half", 3, 1, 6, True, 0.01, "")]

    recs = {k: [] for k in ("len", "mirror", "ck", "wr", "drop_sort", "thr", "has_min", "pmin", "seed")}
    flat = {k: [] for k in ("phot", "phot_out", "ck_out", "p_slide", "p_pairs")}
    offs = {k: [0] for k in flat}
    tabs = {k: [] for k in ("pl_trace", "pl_start", "pl_stop", "pl_h", "tf_trace", "tf_start", "tf_stop", "tf_h")}
    for ci, (n, kind, mirror, ck, wr, ds, thr, special) in enumerate(cases):
        seed = 1000 * ci
        while True:
            rng = np.random.default_rng(seed)
            v = synth_trace(rng, n, kind)
            pmin = None
            phot = [float(x) for x in v]
            if special == "dropout":
                for i in rng.choice(n, n // 10, replace=False):
                    phot[i] = None
            elif special == "clamp":
                pmin = 0.0
            elif special == "constant":
                phot = [12345.0] * n
            elif special == "nan":
                pmin = -1000.0
                for i in rng.choice(n, 5, replace=False):
                    phot[i] = math.nan
            tr = fl.Trace.__new__(fl.Trace)
            tr.trace = [None if x is None else Stub(x) for x in phot]
            del rec[:]
            if wr == 6 and ds:
                res = fl.Trace.stepfit_photometries(tr, 0, 0, mirror_start=mirror, chung_kennedy=ck, p_threshold=thr,
                                                    photometry_min=pmin)
                ph_o, ck_o, pl_o, tf_o = res[0].trace, res[1].trace, res[2].trace, res[3].trace
            else:
                photometries = tr.photometries(photometry_min=pmin)
                mir = sf.mirror_photometries(photometries, mirror_size=mirror)
                ckf = mir
                for c in range(ck):
                    ckf = sf.chung_kennedy_filter(luminosities=mir, window_lengths=(2, 4, 8, 16))
                pl = sf.sliding_t_fitter(luminosity_sequence=ckf, window_radius=wr, p_threshold=thr)
                pl = sf.refit_plateaus(mir, pl)
                tf = sf.t_test_filter(luminosities=mir, plateaus=pl, p_threshold=thr, drop_sort=ds, no_merge_start=mirror)
                ph_o, ck_o = photometries, sf.unmirror_photometries(ckf, mirror)
                pl_o, tf_o = sf.unmirror_plateaus(pl, mirror), sf.unmirror_plateaus(tf, mirror)
            Lm = n + min(mirror, n)
            n_slide = max(wr - 5, 0) * Lm
            ps = np.array(rec, dtype=np.float64)
            fin = ps[np.isfinite(ps)]
            bad = bool(np.any(np.abs(fin - thr) <= REL * np.maximum(np.abs(fin), thr)))
            pairs = np.sort(fin[n_slide:] if len(ps) > n_slide else np.zeros(0))
            if len(pairs) > 1:
                d = np.diff(pairs)
                bad |= bool(np.any((d > 0) & (d <= REL * np.abs(pairs[1:]))))
            if not bad:
                break
            seed += 1
        recs["len"].append(n); recs["mirror"].append(mirror); recs["ck"].append(ck); recs["wr"].append(wr)
        recs["drop_sort"].append(int(ds)); recs["thr"].append(thr); recs["has_min"].append(int(pmin is not None))
        recs["pmin"].append(0.0 if pmin is None else pmin); recs["seed"].append(seed)
        for key, arr in (("phot", [0.0 if x is None else x for x in phot]), ("phot_out", [float(x) for x in ph_o]),
                         ("ck_out", [float(x) for x in ck_o]), ("p_slide", ps[:n_slide]),
                         ("p_pairs", ps[n_slide:])):
            flat[key].extend(list(arr))
            offs[key].append(len(flat[key]))
        for pre, pls in (("pl", pl_o), ("tf", tf_o)):
            for s, o, h in pls:
                tabs[pre + "_trace"].append(ci); tabs[pre + "_start"].append(s); tabs[pre + "_stop"].append(o)
                tabs[pre + "_h"].append(float(h))
        print("case %d: n=%d m=%d ck=%d wr=%d ds=%d thr=%g %s seed=%d -> %d / %d plateaus" %
              (ci, n, mirror, ck, wr, ds, thr, special, seed, len(pl_o), len(tf_o)))
    out = {}
    for k, v in recs.items():
        out["case_" + k] = np.array(v, dtype=np.float64 if k in ("thr", "pmin") else np.int64)
    for k, v in flat.items():
        out[k] = np.array(v, dtype=np.float64)
        out[k + "_off"] = np.array(offs[k], dtype=np.int64)
    for k, v in tabs.items():
        out[k] = np.array(v, dtype=np.float64 if k.endswith("_h") else np.int64)
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    gen_timetrace(fl, os.path.join(os.path.dirname(a.out), "stepfit_timetrace.npz"))


# ---- tests/golden/stepfit_limits.npz: traces whose mirrored length is 8191 / 8192 -------------------------------------
# (frames, mirror_start, chung_kennedy, drop_sort, p_threshold); window_radius 6.  At 1e-6 chance finds no step in 8192 frames
# of noise, so the first plateau stays whole; the last case (0.01) starts its t-filter with more than 64 plateau pairs.
LIMIT_CASES = ((8188, 3, 0, True, 1e-6), (8189, 3, 0, True, 1e-6), (8189, 3, 1, True, 1e-6), (8192, 0, 0, True, 1e-6),
               (8192, 0, 1, True, 1e-6), (8189, 3, 0, False, 1e-6), (8189, 3, 0, True, 0.01))


def limits_trace(seed, n):
    """One long first plateau (more than 7700 frames) and three of 150 - 170 frames, UNROUNDED: the sum of full-mantissa
    doubles depends on the order of the additions, so a mean over a plateau pins numpy's pairwise order."""
    rng = np.random.default_rng(seed)
    c1 = 7700 + int(rng.integers(0, 8))
    c2 = c1 + 150 + int(rng.integers(0, 20))
    c3 = c2 + 150 + int(rng.integers(0, 20))
    i = np.arange(n)
    level = 3.0 - (i >= c1) - (i >= c2) - (i >= c3)
    return level * 40000.0 + 5000.0 + rng.normal(0.0, 1500.0, n)


def pairwise_max_leaf(n, depth):
    """Largest block that numpy's pairwise sum of n elements adds up sequentially when the recursion stops after `depth`
    splits (numpy itself recurses until a block has at most 128 elements)."""
    if n <= 128 or depth == 0:
        return n
    n2 = n // 2
    n2 -= n2 % 8
    return max(pairwise_max_leaf(n2, depth - 1), pairwise_max_leaf(n - n2, depth - 1))


def gen_limits(sf, fl, rec, Stub, out_path):
    recs = {k: [] for k in ("len", "mirror", "ck", "drop_sort", "seed", "first_pass_pairs")}
    thrs = []
    flat = {k: [] for k in ("ck_out", "p_pairs")}
    offs = {k: [0] for k in flat}
    tabs = {k: [] for k in ("pl_trace", "pl_start", "pl_stop", "pl_h", "tf_trace", "tf_start", "tf_stop", "tf_h")}
    sums = []
    for ci, (n, mirror, ck, ds, thr) in enumerate(LIMIT_CASES):
        seed = 77000 + 100 * ci
        while True:
            v = limits_trace(seed, n)
            phot = [float(x) for x in v]
            tr = fl.Trace.__new__(fl.Trace)
            tr.trace = [Stub(x) for x in phot]
            del rec[:]
            if ds:
                res = fl.Trace.stepfit_photometries(tr, 0, 0, mirror_start=mirror, chung_kennedy=ck, p_threshold=thr,
                                                    photometry_min=None)
                ck_o, pl_o, tf_o = res[1].trace, res[2].trace, res[3].trace
            else:
                mir = sf.mirror_photometries(phot, mirror_size=mirror)
                ckf = mir
                for c in range(ck):
                    ckf = sf.chung_kennedy_filter(luminosities=mir, window_lengths=(2, 4, 8, 16))
                pl = sf.sliding_t_fitter(luminosity_sequence=ckf, window_radius=6, p_threshold=thr)
                pl = sf.refit_plateaus(mir, pl)
                tf = sf.t_test_filter(luminosities=mir, plateaus=pl, p_threshold=thr, drop_sort=ds, no_merge_start=mirror)
                ck_o = sf.unmirror_photometries(ckf, mirror)
                pl_o, tf_o = sf.unmirror_plateaus(pl, mirror), sf.unmirror_plateaus(tf, mirror)
            Lm = n + min(mirror, n)
            ps = np.array(rec, dtype=np.float64)
            fin = ps[np.isfinite(ps)]
            bad = bool(np.any(np.abs(fin - thr) <= REL * np.maximum(np.abs(fin), thr)))
            pairs = np.sort(fin[Lm:])
            d = np.diff(pairs)
            bad |= bool(np.any((d > 0) & (d <= REL * np.abs(pairs[1:]))))
            bad |= bool(np.isnan(ps[Lm:]).any())                   # (>= 64 pairs with a NaN p: not built on the device)
            # the conditions on the case: a final plateau of more than 7689 frames whose length a 6-level recursion would
            # sum differently, at least three of 130 - 7689 frames, and a first t-filter pass of at least 64 pairs
            lens = [o - s + 1 for s, o, _ in tf_o]
            if thr < 0.01:
                bad |= not (max(lens) > 7689 and pairwise_max_leaf(max(lens) + min(mirror, n), 6) > 128)
                bad |= sum(1 for x in lens if 129 < x <= 7689) < 3
            else:
                bad |= len(pl_o) - 1 < 64
            assert seed % 100 < 20, "no seed meets the conditions of limits case %d" % ci
            if not bad:
                break
            seed += 1
        recs["len"].append(n); recs["mirror"].append(mirror); recs["ck"].append(ck); recs["drop_sort"].append(int(ds))
        recs["seed"].append(seed); recs["first_pass_pairs"].append(len(pl_o) - 1); thrs.append(thr)
        sums.append(float(np.sum(v)))
        for key, arr in (("ck_out", [float(x) for x in ck_o] if ck else []), ("p_pairs", ps[Lm:])):
            flat[key].extend(list(arr))
            offs[key].append(len(flat[key]))
        for pre, pls in (("pl", pl_o), ("tf", tf_o)):
            for s, o, h in pls:
                tabs[pre + "_trace"].append(ci); tabs[pre + "_start"].append(s); tabs[pre + "_stop"].append(o)
                tabs[pre + "_h"].append(float(h))
        print("limits case %d: n=%d m=%d ck=%d ds=%d seed=%d -> %d / %d plateaus, %d pair tests" %
              (ci, n, mirror, ck, ds, seed, len(pl_o), len(tf_o), len(ps) - Lm), flush=True)
    out = {"case_" + k: np.array(v, dtype=np.int64) for k, v in recs.items()}
    out["case_phot_sum"] = np.array(sums, dtype=np.float64)        # (guards the seeded generator against drift)
    out["case_thr"] = np.array(thrs, dtype=np.float64)
    for k, v in flat.items():
        out[k] = np.array(v, dtype=np.float64)
        out[k + "_off"] = np.array(offs[k], dtype=np.int64)
    for k, v in tabs.items():
        out[k] = np.array(v, dtype=np.float64 if k.endswith("_h") else np.int64)
    np.savez_compressed(out_path, **out)
    print("wrote", out_path, os.path.getsize(out_path), "bytes")


def timetrace_stack(seed=17, n_frames=40, shape=(96, 96)):
    """uint16 frames of one field: Gaussian spots of 1 - 3 fluors (each bleaching at a random frame) on a noisy
    background.  Returns (frames, spot centres)."""
    rng = np.random.default_rng(seed)
    centres = [(h, w) for h in range(14, shape[0] - 10, 17) for w in range(14, shape[1] - 10, 17)]
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    frames = rng.normal(120.0, 12.0, (n_frames,) + shape)
    for h, w in centres:
        n_fl = int(rng.integers(1, 4))
        bleach = np.sort(rng.integers(3, n_frames + 8, n_fl))
        amp = rng.uniform(350.0, 600.0)
        g = np.exp(-((yy - h) ** 2 + (xx - w) ** 2) / (2 * 1.4 ** 2))
        for f in range(n_frames):
            frames[f] += amp * int(np.sum(bleach > f)) * g
    return np.clip(np.round(frames), 0, 65535).astype(np.uint16), np.array(centres, np.int32)


def gen_timetrace(fl, out_path):
    """TimetraceExperiment(frames).lc_create_traces(initial_spots) + stepfit_tracks() with basic_timetrace_script's
    defaults (photometry_min None, mexican_hat, mirror_start 0, chung_kennedy 0, p_threshold 0.01)."""
    frames, centres = timetrace_stack()
    # Spot.mexican_hat_photometry_metric (flexlibrary.py:206) adds the crown's uint16 pixels with Python's sum, which wraps
    # at 2^16 under numpy's scalar rules; fsq_mexican_hat sums exactly.  Keep every 7 x 7 crown below 2^16.
    wide = frames.astype(np.int64)
    for h, w in centres:
        for dh in range(-3, 4):
            for dw in range(-3, 4):
                assert wide[:, h - 6 + dh:h + 7 + dh, w - 6 + dw:w + 7 + dw][:, 3:10, 3:10].sum(axis=(1, 2)).max() < 65536
    imgs = [fl.Image(image=f) for f in frames]
    spots = [fl.Spot(imgs[0], int(h), int(w), 5) for h, w in centres]
    ex = fl.TimetraceExperiment(imgs)
    # (search_radius as the int 3: the default 3.0 slices frames with floats, which Python 2's numpy accepted and
    # Python 3's refuses)
    ex.lc_create_traces(initial_spots=spots, search_radius=3)
    step_fits, inter = ex.stepfit_tracks()
    out = {"frames": frames, "init_hw": centres, "keys": np.array(list(step_fits.keys()), np.int64).reshape(-1, 2)}
    ph, ck, rows = [], [], {"pl": [], "tf": []}
    for k, key in enumerate(step_fits.keys()):
        d = inter[key]
        ph.append([float(x) for x in d["photometries"].trace])
        ck.append([float(x) for x in d["ck_filtered_photometries"].trace])
        for pre, name in (("pl", "plateaus"), ("tf", "t_filtered_plateaus")):
            rows[pre] += [(k, s, o, float(h)) for s, o, h in d[name].trace]
        assert d["t_filtered_plateaus"] is step_fits[key]
    out["photometries"] = np.array(ph, np.float64)
    out["ck_filtered"] = np.array(ck, np.float64)
    for pre in ("pl", "tf"):
        r = np.array(rows[pre], np.float64).reshape(-1, 4)
        out[pre + "_trace"], out[pre + "_start"], out[pre + "_stop"] = (r[:, 0].astype(np.int64), r[:, 1].astype(np.int64),
                                                                        r[:, 2].astype(np.int64))
        out[pre + "_h"] = r[:, 3]
    np.savez_compressed(out_path, **out)
    print("wrote", out_path, os.path.getsize(out_path), "bytes;", len(step_fits), "tracks,", len(rows["tf"]), "final plateaus")


if __name__ == "__main__":
    main()
