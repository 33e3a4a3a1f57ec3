"""Writes tests/golden/remainder_tracks.npz: nested track-photometry dicts through the reference's _remainder_adjust_2 and
_remainder_adjust (MCsimlib.py:3434-3472, :3398-3431), inputs and outputs.

Loads the reference at run time through oracle/refload.py, MCsimlib as tools/gen_lognormal_golden.py loads it.

  (a) two seeded synthetic track_photometries CSV texts, F = 8 and F = 5, read by the reference's own reader: 2 channels x 6
      fields with 0, 1, 2, 4, 5, 6 remainders in the first channel and 0, 1, 2, 3, 4, 0 in the second, each corrected with
      minimum_r_per_field 1 and 5 (so min - 1, min and min + 1 remainders, a field with none, and with 5 a channel without a
      kept field), duplicate (h, w) rows, None coordinates, values ending in .5.
  (b) direct dicts, F = 1, 2, 3, 7, 64: even and odd R, minimum_r_per_field 0, 1, 3, 5, remainders with median 0 (inf and NaN
      ratios, NaN and infinite medians), negative medians, many equal ratios at the middle, a field without a remainder kept by minimum 0.
No (segment, frame) holds both -0.0 and +0.0: the remainders of one field have medians of one sign.

Floats are recorded as float64 bits; text is not (Python 3 prints floats differently, _py2_str carries that convention).
The generator asserts that the fixture is not vacuous: at least 25 % of the segments kept and 25 % dropped, at least 10 even-R
medians of two different middle values, at least 5 NaN medians.

  python tools/gen_remainder_golden.py [--reference DIR]
"""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSV_REMAINDERS = {"ch1": (0, 1, 2, 4, 5, 6), "ch2": (0, 1, 2, 3, 4, 0)}


def csv_text(F, seed):
    rng = np.random.default_rng(seed)
    lines = ["CHANNEL,FIELD,H,W,CATEGORY," + ",".join("FRAME %d" % i for i in range(F))]
    for channel, remainders in CSV_REMAINDERS.items():
        for field, R in enumerate(remainders):
            n = R + int(rng.integers(6, 12))
            gain = [1.0 + 0.08 * np.sin(f + field) for f in range(F)]
            kinds = rng.permutation([True] * R + [False] * (n - R))
            for k, remainder in enumerate(kinds):
                if remainder:
                    cat = (True,) * F
                else:
                    drop = int(rng.integers(0, F))                 # OFF from `drop` on; 0: never ON
                    cat = tuple(f < drop for f in range(F))
                    if k % 5 == 0 and drop > 1:
                        cat = (False,) + cat[1:]
                level = float(rng.choice([1, 1, 2, 3])) * 9000.0
                vals = [(120.0 + gain[f] * level * np.exp(rng.normal(0.0, 0.15))) if cat[f] else rng.normal(120.0, 200.0) for f in range(F)]
                vals = [float(int(x)) + (0.5 if rng.random() < 0.15 else float(rng.integers(0, 4)) / 4) for x in vals]
                h, w = int(rng.integers(5, 500)), int(rng.integers(5, 500))
                text = ",".join(repr(x) for x in vals)
                lines.append('%s,%d,%d,%d,"%s",%s' % (channel, field, h, w, str(cat), text))
                if k == 2:                                          # the same place again: the reader keeps the first row
                    lines.append('%s,%d,%d,%d,"%s",%s' % (channel, field, h, w, str((True,) * F), ",".join(repr(x + 77.0) for x in vals)))
                if k == 3:
                    lines.append('%s,%d,None,None,"%s",%s' % (channel, field, str((True,) * F), text))
    return "\n".join(lines) + "\n"


def direct_cases():
    """(name, F, minimum, photometries)"""
    rng = np.random.default_rng(977)
    out = []
    for F in (1, 2, 3, 7, 64):
        for minimum in (0, 1, 3, 5):
            d, row = {}, 0
            for field, (R, sign) in enumerate([(0, 1), (1, 1), (2, -1), (3, 1), (4, 1), (5, -1), (6, 1), (7, 1), (8, -1), (12, 1)]):
                fdict = d.setdefault("ch1", {}).setdefault(field, {})
                n = R + int(rng.integers(1, 5))
                for k in range(n):
                    row += 1
                    remainder = k < R
                    cat = (True,) * F if remainder else tuple(bool(x) for x in rng.integers(0, 2, F - 1)) + (False,)
                    base = int(rng.integers(2000, 20000))
                    vals = tuple(sign * int(base + rng.integers(-base // 4, base // 4)) for _ in range(F))
                    fdict[(row, 3 * row + 1)] = (cat, vals, row)
            # a field of equal remainders: every ratio at the middle is the same
            fdict = d["ch1"].setdefault(20, {})
            vals = tuple(int(1000 + 37 * f) for f in range(F))
            for k in range(6 + (minimum % 2)):
                row += 1
                fdict[(row, 7)] = ((True,) * F, vals if k < 5 else tuple(v + 11 * (f % 3) for f, v in enumerate(vals)), row)
            # medians 0: +-inf and NaN among the ratios
            fdict = d.setdefault("ch2", {}).setdefault(3, {})
            for k in range(5):
                row += 1
                if k == 0:
                    vals = (0,) * F
                elif k == 1 and F >= 3:
                    vals = tuple([-5 - f for f in range(F // 2)] + [0] * (F - 2 * (F // 2)) + [7 + f for f in range(F // 2)])
                else:
                    vals = tuple(int(rng.integers(500, 900)) for _ in range(F))
                fdict[(row, 9)] = ((True,) * F, vals, row)
            # a zero-median track whose ratios are infinite, not NaN, among enough finite ones: medians stay finite or infinite
            if F >= 2 and F % 2 == 0:
                fdict = d["ch2"].setdefault(4, {})
                for k in range(6):
                    row += 1
                    vals = tuple([-3 - f for f in range(F // 2)] + [3 + f for f in range(F // 2)]) if k < 2 else \
                        tuple(int(rng.integers(500, 900)) for _ in range(F))
                    fdict[(row, 11)] = ((True,) * F, vals, row)
                # -inf and +inf are the two middle ratios: their mean is NaN by plain arithmetic
                fdict = d["ch2"].setdefault(5, {})
                half = tuple(3 + f for f in range(F // 2))
                for vals in (tuple(-v for v in half) + half, half + tuple(-v for v in half)):
                    row += 1
                    fdict[(row, 13)] = ((True,) * F, vals, row)
                # one zero-median remainder alone: infinite medians
                row += 1
                d["ch2"].setdefault(6, {})[(row, 15)] = ((True,) * F, tuple(-v for v in half) + half, row)
            out.append(("direct_F%d_min%d" % (F, minimum), F, minimum, d))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("FSQ_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "remainder_tracks.npz"))
    a = ap.parse_args()
    os.environ["FSQ_REFERENCE"] = a.reference
    for sub in ("", "oracle", "tests", "tools"):
        sys.path.insert(0, os.path.join(ROOT, sub))
    import refload
    from gen_lognormal_golden import load_mcsimlib
    refload.REF = a.reference
    refload.load_reference()
    mc = load_mcsimlib(refload)
    import _remainder_cases as C

    todo, texts = [], [csv_text(8, 8101), csv_text(5, 5101)]
    for k, text in enumerate(texts):
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "track_photometries_%d.csv" % k)
            with open(path, "w") as f:
                f.write(text)
            photometries, rows = mc.read_track_photometries_csv(path, head_truncate=0, tail_truncate=0, downstep_filtered=False)
        F = len(next(iter(rows.values()))[4])
        assert F == (8, 5)[k] and set(photometries) == {"ch1", "ch2"} and all(len(c) == 6 for c in photometries.values())
        for minimum in (1, 5):
            todo.append(("csv%d_min%d" % (k, minimum), F, minimum, photometries, k))
    todo += [c + (-1,) for c in direct_cases()]

    results = {"r2": ([], []), "r1": ([], [])}
    for name, F, minimum, photometries, k in todo:
        for key, fn in (("r2", mc._remainder_adjust_2), ("r1", mc._remainder_adjust)):
            adjusted, medians = fn(photometries, F, minimum_r_per_field=minimum)
            results[key][0].append(adjusted)
            results[key][1].append(medians)
    out = {"name": np.array([t[0] for t in todo]), "F": np.array([t[1] for t in todo], dtype=np.int64),
           "min": np.array([t[2] for t in todo], dtype=np.int64), "csv": np.array([t[4] for t in todo], dtype=np.int64),
           "csv_0": np.frombuffer(texts[0].encode(), dtype=np.uint8), "csv_1": np.frombuffer(texts[1].encode(), dtype=np.uint8)}
    out.update({"in_" + k: v for k, v in C.pack_tracks([t[3] for t in todo]).items()})
    for key, (adjusted, medians) in results.items():
        out.update({key + "_adj_" + k: v for k, v in C.pack_tracks(adjusted).items()})
        out.update({key + "_med_" + k: v for k, v in C.pack_medians(medians).items()})
    np.savez_compressed(a.out, **out)

    C.golden.cache_clear(), C.cases.cache_clear()
    C.GOLD = os.path.dirname(a.out)
    recorded = C.cases()
    for (name, F, minimum, photometries, k), c in zip(todo, recorded):                      # the file holds what went in
        assert c["photometries"] == photometries and list(c["photometries"]) == list(photometries), name
    kept, dropped, split, nans = C.counts(recorded)
    print("%d cases, %d segments kept, %d dropped, %d even-R medians of two values, %d NaN medians, %d bytes"
          % (len(todo), kept, dropped, split, nans, os.path.getsize(a.out)))
    assert kept >= 0.25 * (kept + dropped) and dropped >= 0.25 * (kept + dropped) and split >= 10 and nans >= 5
    # the csv cases with 5: the second channel has no kept field and is in neither output
    for c in recorded:
        if c["csv"] is not None and c["min"] == 5:
            assert list(c["r2"][0]) == ["ch1"] == list(c["r2"][1]) and list(c["r1"][0]) == ["ch1"]


if __name__ == "__main__":
    main()
