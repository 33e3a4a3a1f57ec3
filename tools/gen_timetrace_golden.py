"""Writes tests/golden/timetrace_experiment.npz: TimetraceExperiment.save_experiment_as_csv of the reference, recorded.

Loads the reference at run time through oracle/refload.py (as tools/gen_stepfit_golden.py does, with numpy's AVX-512 paths
disabled) and records three experiments:

  s0, s1   tools/gen_stepfit_golden.py:timetrace_stack() through lc_create_traces + stepfit_tracks + save_experiment_as_csv with
           (mirror_start 0, chung_kennedy 0, photometry_min None) and (3, 1, 2000.0)
  cr       a crafted experiment built from SimpleTrace / PlateauTrace objects: traces with None spots (one of them in frame 0),
           a first plateau of one frame in a multi-plateau fit, a trace whose every frame is its own plateau, lengths 2, 7, 8,
           9, 127, 128, 129, stated heights that are not the means

Per experiment the fixture holds the photometry rows and the present mask, the step-fit plateaus (flat, one entry per plateau),
the intermediates, every CSV column parsed back into float64 / int arrays with a mask for None, rss / tss / r_2 per trace from
the reference's own methods, and the CSV text as bytes.  A one-frame trace cannot be written (its total sum of squares is 0, the
reference raises ZeroDivisionError): it is recorded among the error cases, with the exception types of a gap, a length mismatch,
missing and unequal intermediates.  kat_json holds known answers of last_step_info, frame_plateau, plateau_value and
plateaus_to_steps on plateau lists and on true step lists.

  python tools/gen_timetrace_golden.py [--reference DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

NPY_ENV = "AVX512F AVX512CD AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR"
if __name__ == "__main__" and os.environ.get("NPY_DISABLE_CPU_FEATURES") != NPY_ENV:
    os.environ["NPY_DISABLE_CPU_FEATURES"] = NPY_ENV
    sys.exit(subprocess.call([sys.executable] + sys.argv))         # a fresh child: numpy reads the variable at import

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_stepfit_golden import timetrace_stack

SETS = ((0, 0, None), (3, 1, 2000.0))                              # (mirror_start, chung_kennedy, photometry_min)
INTERMEDIATES = ("ck_filtered_photometries", "photometries", "plateaus", "t_filtered_plateaus")


class StubSpot(object):
    """A Spot as far as SimpleTrace and save_experiment_as_csv use one: (h, w) and a photometry."""

    def __init__(self, h, w, v):
        self.h, self.w, self.v = h, w, v

    def photometry(self, method=None, **kwargs):
        return self.v


def parse_csv(text, with_step_fits=True):
    """The CSV text -> columns.  str() of a float64 round-trips, so float() of a cell is the number the reference held."""
    lines = text.split("\r\n")
    assert lines[-1] == ""
    header, rows = lines[0].split(","), [ln.split(",") for ln in lines[1:-1]]
    want = ["Trace #", "Hcoord", "Wcoord", "Frame #", "Photometry", "Step #", "Plateau Height", "Step Size", "Plateau Length",
            "Overall Fit R^2"] + list(INTERMEDIATES)
    assert header == want, header
    col = lambda j: [r[j] for r in rows]
    out = {"trace": np.array(col(0), np.int64), "h": np.array(col(1), np.int64), "w": np.array(col(2), np.int64),
           "frame": np.array(col(3), np.int64), "photometry": np.array([float(c) for c in col(4)]),
           "photometry_is_int": np.array(["." not in c and "e" not in c for c in col(4)]),
           "step_none": np.array([c == "None" for c in col(5)])}
    assert all((a == "None") == (b == "None") for a, b in zip(col(5), col(7)))
    out["step_num"] = np.array([-1 if c == "None" else int(c) for c in col(5)], np.int64)
    out["plateau_height"] = np.array([float(c) for c in col(6)])
    out["step_size"] = np.array([0.0 if c == "None" else float(c) for c in col(7)])
    out["plateau_length"] = np.array(col(8), np.int64)
    out["r2"] = np.array([float(c) for c in col(9)])
    for j, name in enumerate(INTERMEDIATES):
        out["inter_" + name] = np.array([float(c) for c in col(10 + j)])
    return out


def record(fl, ex, prefix, out):
    """One experiment through the reference's save_experiment_as_csv -> out[prefix + ...]."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "t.csv")
        n_rows = ex.save_experiment_as_csv(path, include_step_fits=True, include_intermediates=True)
        with open(path, newline="") as f:
            text = f.read()
    cols = parse_csv(text)
    assert n_rows == 1 + len(cols["trace"])
    traces = ex.spot_traces
    lens = np.array([t.num_frames for t in traces], np.int64)
    F = int(lens.max())
    phot, present = np.zeros((len(traces), F)), np.zeros((len(traces), F), bool)
    hw = np.zeros((len(traces), F, 2), np.int64)
    ck = np.zeros((len(traces), F))
    clamped = np.zeros((len(traces), F))
    rss, tss, r2, tabs = [], [], [], {"pl": [], "tf": []}
    for t, tr in enumerate(traces):
        key = (tr.h, tr.w)
        for f, spot in enumerate(tr.trace):
            phot[t, f] = float(tr.photometry(f))
            if spot is not None:
                present[t, f] = True
                hw[t, f] = spot.h, spot.w
        sf = ex.step_fits[key]
        inter = ex.step_fit_intermediates[key]
        assert sorted(inter) == list(INTERMEDIATES)
        ck[t, :lens[t]] = [float(v) for v in inter["ck_filtered_photometries"].trace]
        clamped[t, :lens[t]] = [float(v) for v in inter["photometries"].trace]
        rss.append(float(fl.Trace.trace_comparison_rss(tr, sf)))
        tss.append(float(tr.total_sum_squares()))
        r2.append(float(fl.Trace.coefficient_of_determination(tr, sf)))
        for pre, pls in (("pl", inter["plateaus"].trace), ("tf", sf.trace)):
            tabs[pre] += [(t, s, o, float(h)) for s, o, h in pls]
    out.update({prefix + "len": lens, prefix + "photometry": phot, prefix + "present": present, prefix + "hw": hw,
                prefix + "keys": np.array([(tr.h, tr.w) for tr in traces], np.int64), prefix + "ck_filtered": ck,
                prefix + "photometries": clamped, prefix + "rss": np.array(rss), prefix + "tss": np.array(tss),
                prefix + "r_2": np.array(r2), prefix + "csv": np.frombuffer(text.encode("ascii"), np.uint8)})
    for pre in ("pl", "tf"):
        r = np.array(tabs[pre], np.float64).reshape(-1, 4)
        for j, k in enumerate(("trace", "start", "stop")):
            out[prefix + pre + "_" + k] = r[:, j].astype(np.int64)
        out[prefix + pre + "_h"] = r[:, 3]
    for k, v in cols.items():
        out[prefix + "col_" + k] = v
    print("%s %d traces, %d rows, %d bytes of CSV, plateaus per trace %d .. %d, %d None spots, %d rows without a step" %
          (prefix, len(traces), n_rows, len(text), np.bincount(out[prefix + "tf_trace"]).min(),
           np.bincount(out[prefix + "tf_trace"]).max(), int((~present & (np.arange(F)[None] < lens[:, None])).sum()),
           int(cols["step_none"].sum())), flush=True)


def crafted(fl, sf, bad=None):
    """The crafted experiment; `bad` swaps in one of the error cases."""
    rng = np.random.default_rng(4711)
    specs = []                                                     # (length, plateau stops, None frames, stated heights?)
    specs.append((7, (2, 6), (0, 4), False))
    specs.append((8, (0, 4, 7), (), False))                        # a first plateau of one frame
    specs.append((9, tuple(range(9)), (), False))                  # every frame its own plateau
    specs.append((2, (1,), (), False))
    specs.append((127, (30, 31, 100, 126), (5, 6, 64, 126), False))
    specs.append((128, (127,), (), False))                         # one plateau: R^2 == 0.0
    specs.append((129, (63, 128), (), True))
    specs.append((40, (0, 1, 39), (20,), True))
    traces, step_fits, inters = [], {}, {}
    for i, (n, stops, nones, stated) in enumerate(specs):
        h, w = 10 + 3 * i, 20 + 5 * i
        level = np.zeros(n)
        a = 0
        for k, o in enumerate(stops):
            level[a:o + 1] = 40000.0 - 9000.0 * k
            a = o + 1
        vals = level + rng.normal(0.0, 3000.0, n)
        spots = [None if f in nones else StubSpot(h + (f % 3) - 1, w + (f % 2), np.float64(vals[f])) for f in range(n)]
        tr = fl.SimpleTrace(spots)
        phot = tr.photometries(photometry_min=None)
        pls, a = [], 0
        for o in stops:
            pls.append((a, o, 0.0))
            a = o + 1
        pls = sf.refit_plateaus(list(phot), pls)
        if stated:
            pls = [(s, o, np.float64(h_ + 1234.5678 * (k + 1))) for k, (s, o, h_) in enumerate(pls)]
        fine = sf.refit_plateaus(list(phot), [(f, min(f + 2, n - 1), 0.0) for f in range(0, n, 3)])
        key = (tr.h, tr.w)
        traces.append(tr)
        step_fits[key] = fl.PlateauTrace(pls, *key)
        inters[key] = {"photometries": fl.PhotometryTrace(phot, *key),
                       "ck_filtered_photometries": fl.PhotometryTrace([float(v) * 0.5 + 100.0 for v in phot], *key),
                       "plateaus": fl.PlateauTrace(fine, *key), "t_filtered_plateaus": step_fits[key]}
    if bad is not None:
        tr = traces[1]
        key = (tr.h, tr.w)
        if bad == "gap":
            step_fits[key] = fl.PlateauTrace([(0, 2, 1.0), (4, 7, 2.0)], *key)
        elif bad == "length":
            step_fits[key] = fl.PlateauTrace([(0, 2, 1.0), (3, 6, 2.0)], *key)
        elif bad == "zero_tss":
            traces[1] = fl.SimpleTrace([StubSpot(key[0], key[1], np.float64(777.25))])
            step_fits[key] = fl.PlateauTrace([(0, 0, np.float64(777.25))], *key)
        elif bad == "constant":
            traces[1] = fl.SimpleTrace([StubSpot(key[0], key[1], np.float64(5.5)) for _ in range(8)])
        elif bad == "missing_intermediates":
            del inters[key]
        elif bad == "unequal_intermediates":
            del inters[key]["plateaus"]
        else:
            raise ValueError(bad)
    return fl.TimetraceExperiment(None, spot_traces=traces, step_fits=step_fits, step_fit_intermediates=inters)


def kats(sf):
    """Known answers of the plateau / step list helpers, on plateau lists and on the step lists made from them."""
    lists = [[(0, 9, 3.5)], [(0, 0, 9.0), (1, 4, 7.25), (5, 9, 2.0)], [(0, 3, 9.0), (4, 4, 7.0), (5, 5, 6.5), (6, 11, 1.0)],
             [(0, 5, 2.0), (6, 7, 8.0)], [(f, f, float(10 - f)) for f in range(6)], [(2, 4, 1.0), (6, 8, 2.0)], []]
    out = []
    for pls in lists:
        steps = sf.plateaus_to_steps(pls)
        last = pls[-1][1] if pls else 2
        entry = {"plateaus": [list(p) for p in pls], "steps": [list(s) for s in steps], "frames": list(range(0, last + 3)),
                 "last_step_info_of_plateaus": [list(sf.last_step_info(pls, f)) for f in range(0, last + 3)],
                 "last_step_info_of_steps": [list(sf.last_step_info(steps, f)) for f in range(0, last + 3)],
                 "frame_plateau": [[list(sf.frame_plateau(pls, f)[0]), sf.frame_plateau(pls, f)[1]] for f in range(0, last + 3)],
                 "plateau_value": []}
        for f in range(0, last + 3):
            try:
                entry["plateau_value"].append(sf.plateau_value(pls, f))
            except ValueError:
                entry["plateau_value"].append("ValueError")
        out.append(entry)
    try:
        sf.last_step_info([(0, 1, 2.0)], -1)
        neg = "none"
    except Exception as e:      # noqa: BLE001
        neg = type(e).__name__
    return {"lists": out, "negative_frame": neg}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("FSQ_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "timetrace_experiment.npz"))
    a = ap.parse_args()
    os.environ["FSQ_REFERENCE"] = a.reference
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import refload
    refload.REF = a.reference
    ref = refload.load_reference()
    sf = refload.load("stepfitting_library", "stepfitting_library.py")
    fl = refload.load_flexlibrary(ref).fl
    out = {}
    frames, centres = timetrace_stack()
    out["set_params"] = np.array([(m, c, 0.0 if p is None else p, p is not None) for m, c, p in SETS], np.float64)
    for k, (mirror, ck, pmin) in enumerate(SETS):
        imgs = [fl.Image(image=f) for f in frames]
        spots = [fl.Spot(imgs[0], int(h), int(w), 5) for h, w in centres]
        ex = fl.TimetraceExperiment(imgs)
        ex.lc_create_traces(initial_spots=spots, search_radius=3)  # (the int 3: see tools/gen_stepfit_golden.py)
        ex.stepfit_tracks(photometry_min=pmin, mirror_start=mirror, chung_kennedy=ck)
        record(fl, ex, "s%d_" % k, out)
    record(fl, crafted(fl, sf), "cr_", out)
    assert (out["cr_tf_stop"][out["cr_tf_start"] == 0] == 0).sum() >= 2 and out["cr_col_step_none"].any()
    errors = {}
    for bad in ("gap", "length", "zero_tss", "constant", "missing_intermediates", "unequal_intermediates"):
        with tempfile.TemporaryDirectory() as d:
            try:
                crafted(fl, sf, bad).save_experiment_as_csv(os.path.join(d, "t.csv"), include_step_fits=True,
                                                            include_intermediates=True)
                errors[bad] = "none"
            except Exception as e:      # noqa: BLE001
                errors[bad] = type(e).__name__
        print("error case %s: %s" % (bad, errors[bad]), flush=True)
    out["errors_json"] = np.array(json.dumps(errors, sort_keys=True))
    out["kat_json"] = np.array(json.dumps(kats(sf)))
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
