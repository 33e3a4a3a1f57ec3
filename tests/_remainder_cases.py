"""The remainder fixture (tests/golden/remainder_tracks.npz, written by tools/gen_remainder_golden.py) as nested dicts, and
the comparisons the remainder tests share.  Floats are recorded and compared as float64 bits, NaN equal to NaN."""
import functools
import os

import numpy as np

from _util import GOLD, bits_equal

MAX_F = 64
MODES = (("r2", "ratio"), ("r1", "additive"))      # _remainder_adjust_2, _remainder_adjust


def pack_tracks(dicts):
    """Nested {channel: {field: {(h, w): (category, values, row)}}} dicts, one per case, as flat arrays (values as bits, padded
    to 64 frames); the order of every dict is kept."""
    case, ch, field, h, w, row, cat, val = [], [], [], [], [], [], [], []
    for c, d in enumerate(dicts):
        for channel, cdict in d.items():
            for fld, fdict in cdict.items():
                assert len(fdict), "a field without a track cannot be recorded"
                for (hh, ww), (category, values, r) in fdict.items():
                    case.append(c), ch.append(str(channel)), field.append(fld), h.append(hh), w.append(ww), row.append(r)
                    cat.append(sum(1 << f for f, x in enumerate(category) if x))
                    v = np.zeros(MAX_F)
                    v[:len(values)] = [float(x) for x in values]
                    val.append(v.view(np.uint64))
    i64 = lambda x: np.array(x, dtype=np.int64)
    return {"case": i64(case), "ch": np.array(ch, dtype="U8"), "field": i64(field), "h": i64(h), "w": i64(w), "row": i64(row),
            "cat": np.array(cat, dtype=np.uint64), "val": np.array(val, dtype=np.uint64).reshape(len(val), MAX_F)}


def unpack_tracks(g, pre, n_cases, frames, as_int):
    """pack_tracks undone: one dict per case.  as_int: values as Python ints in tuples (the reader's), else float64 in lists."""
    out = [{} for _ in range(n_cases)]
    a = {k: g[pre + k] for k in ("case", "ch", "field", "h", "w", "row", "cat", "val")}       # (an .npz reads an array at every access)
    for i, c in enumerate(a["case"].tolist()):
        F = frames[c]
        category = tuple(bool((int(a["cat"][i]) >> f) & 1) for f in range(F))
        v = a["val"][i, :F].view(np.float64)
        values = tuple(int(x) for x in v) if as_int else list(v)
        key = (int(a["h"][i]), int(a["w"][i]))
        out[c].setdefault(str(a["ch"][i]), {}).setdefault(int(a["field"][i]), {})[key] = (category, values, int(a["row"][i]))
    return out


def pack_medians(dicts):
    case, ch, field, val = [], [], [], []
    for c, d in enumerate(dicts):
        for channel, cdict in d.items():
            for fld, medians in cdict.items():
                case.append(c), ch.append(str(channel)), field.append(fld)
                v = np.zeros(MAX_F)
                v[:len(medians)] = [float(x) for x in medians]
                val.append(v.view(np.uint64))
    return {"case": np.array(case, dtype=np.int64), "ch": np.array(ch, dtype="U8"), "field": np.array(field, dtype=np.int64),
            "val": np.array(val, dtype=np.uint64).reshape(len(val), MAX_F)}


def unpack_medians(g, pre, n_cases, frames):
    out = [{} for _ in range(n_cases)]
    a = {k: g[pre + k] for k in ("case", "ch", "field", "val")}
    for i, c in enumerate(a["case"].tolist()):
        out[c].setdefault(str(a["ch"][i]), {})[int(a["field"][i])] = list(a["val"][i, :frames[c]].view(np.float64))
    return out


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLD, "remainder_tracks.npz"))


@functools.lru_cache(maxsize=None)
def cases():
    """Every recorded case: name, F, minimum, csv (the text the photometries were read from, or None), photometries, and per
    mode key ("r2" / "r1") the reference's (adjusted_photometries, medians)."""
    g = golden()
    frames = g["F"].tolist()
    n = len(frames)
    inputs = unpack_tracks(g, "in_", n, frames, True)
    texts = [t.tobytes().decode() for t in (g["csv_0"], g["csv_1"])]
    out = []
    names, minimum, which = g["name"].tolist(), g["min"].tolist(), g["csv"].tolist()
    for c in range(n):
        k = which[c]
        out.append({"name": names[c], "F": frames[c], "min": minimum[c], "csv": texts[k] if k >= 0 else None,
                    "photometries": inputs[c]})
    for key, _ in MODES:
        adjusted, medians = unpack_tracks(g, key + "_adj_", n, frames, False), unpack_medians(g, key + "_med_", n, frames)
        for c in range(n):
            out[c][key] = (adjusted[c], medians[c])
    return out


def same_adjusted(got, exp, what=None):
    """Nested adjusted dicts with the same keys in the same order, equal categories and rows, values equal bit for bit."""
    assert list(got) == list(exp), what
    for channel in exp:
        assert list(got[channel]) == list(exp[channel]), (what, channel)
        for field in exp[channel]:
            g, e = got[channel][field], exp[channel][field]
            assert list(g) == list(e), (what, channel, field)
            for hw in e:
                assert tuple(g[hw][0]) == tuple(e[hw][0]) and g[hw][2] == e[hw][2], (what, channel, field, hw)
                assert len(g[hw][1]) == len(e[hw][1]) and bits_equal(g[hw][1], e[hw][1]).all(), (what, channel, field, hw)


def same_medians(got, exp, what=None):
    assert list(got) == list(exp), what
    for channel in exp:
        assert list(got[channel]) == list(exp[channel]), (what, channel)
        for field in exp[channel]:
            assert len(got[channel][field]) == len(exp[channel][field]), (what, channel, field)
            assert bits_equal(got[channel][field], exp[channel][field]).all(), (what, channel, field)


def same_arrays(got, exp, what=None):
    """The dicts of fsq_remainder_adjust's outputs, bit for bit."""
    for k in ("n_remainders", "kept"):
        assert np.array_equal(got[k], exp[k]), (what, k)
    for k in ("adjustment", "adjusted"):
        assert got[k].shape == exp[k].shape and bits_equal(got[k], exp[k]).all(), (what, k)


def arrays_of(photometries, F):
    """(rows, category words, one segment index per track, segment keys) of a nested dict, in its order."""
    rows, cats, seg, keys = [], [], [], []
    for channel, cdict in photometries.items():
        for field, fdict in cdict.items():
            keys.append((channel, field))
            for hw, (category, values, row) in fdict.items():
                rows.append([float(v) for v in values])
                cats.append(sum(1 << f for f, x in enumerate(category) if x))
                seg.append(len(keys) - 1)
    return np.array(rows, dtype=np.float64).reshape(len(rows), F), np.array(cats, dtype=np.uint64), np.array(seg, dtype=np.int64), keys


def counts(all_cases):
    """What makes the fixture not vacuous: (segments kept, segments dropped, even-R medians of two different middle values,
    NaN medians), over both modes."""
    import _remainder_reference as RR
    kept = dropped = split = nans = 0
    for c in all_cases:
        rows, cats, seg, keys = arrays_of(c["photometries"], c["F"])
        for key, mode in MODES:
            medians = c[key][1]
            for s, (channel, field) in enumerate(keys):
                if field in medians.get(channel, {}):
                    kept += 1
                    nans += int(np.isnan(medians[channel][field]).sum())
                else:
                    dropped += 1
                    continue
                rem = [t for t in np.flatnonzero(seg == s) if RR.is_remainder(cats[t], c["F"])]
                if len(rem) % 2 or not rem:
                    continue
                for f in range(c["F"]):
                    with np.errstate(all="ignore"):
                        v = np.sort([(rows[t, f] - RR.median(rows[t])) / RR.median(rows[t]) if mode == "ratio" else rows[t, f] for t in rem])
                    mid = v[len(v) // 2 - 1:len(v) // 2 + 1]
                    split += bool(np.isfinite(mid).all() and mid[0] != mid[1])
    return kept, dropped, split, nans
