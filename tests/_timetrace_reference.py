"""NumPy restatement of the timetrace experiment table (include/fsq_timetrace.h), written from DESIGN.md section 4.13 for
tests on machines without the reference, and the loader of tests/golden/timetrace_experiment.npz.

Per frame f of a trace, in the plateau k that holds it: index k, height h_k, length stop_k - start_k + 1 and the reference's
`last_step_info` of the plateaus: (k - 1, h_{k-1}) for k >= 1; for k == 0 (0, h_0) when there is one plateau or stop_0 == 0,
else None (step_num -1, step_size 0.0).  Per trace: rss, the left-to-right sum (np.add.accumulate) over all frames of glibc's
pow(p_f - h_k(f), 2.0); tss, the same sum of pow(p_f - mean, 2.0) with mean = float(np.mean(p)); r2 = 1.0 - rss / tss."""
import json
import os

import numpy as np

import _chisq_reference as R
from _util import GOLD

OK, INVALID, ZERO_TSS = 0, 2, 3
INTERMEDIATES = ("ck_filtered_photometries", "photometries", "plateaus", "t_filtered_plateaus")


def valid(n, plateaus, whole=True):
    """Consecutive plateaus from frame 0 (to frame n - 1 when `whole`)."""
    k = len(plateaus)
    if not (n >= 1 and 1 <= k <= n and plateaus[0][0] == 0):
        return False
    for i, (a, o, _) in enumerate(plateaus):
        if not (a <= o < n) or (i + 1 < k and o + 1 != plateaus[i + 1][0]):
            return False
    return not whole or plateaus[-1][1] == n - 1


def expand(plateaus):
    """Per frame 0 .. stop_last: (index, height) of consecutive plateaus."""
    idx = np.concatenate([np.full(o - a + 1, i, np.int32) for i, (a, o, _) in enumerate(plateaus)])
    return idx, np.array([float(p[2]) for p in plateaus])[idx]


def table(phot, plateaus, pow2=None):
    """One trace -> dict (status, and for a valid trace the per-frame columns, rss, tss and r2 - None when tss == 0)."""
    pow2 = pow2 or R.pow2
    p = np.array([0.0 if v is None else float(v) for v in phot], dtype=np.float64)
    n = len(p)
    if not valid(n, plateaus):
        return {"status": INVALID}
    idx, height = expand(plateaus)
    h = np.array([float(q[2]) for q in plateaus])
    start = np.array([q[0] for q in plateaus])
    stop = np.array([q[1] for q in plateaus])
    first_is_step = len(plateaus) == 1 or stop[0] == 0
    step_num = np.where(idx >= 1, idx - 1, 0 if first_is_step else -1).astype(np.int32)
    step_size = np.where(step_num >= 0, h[np.maximum(step_num, 0)], 0.0)
    mean = float(np.mean(p))
    rss = float(np.add.accumulate(pow2(p - height))[-1])
    tss = float(np.add.accumulate(pow2(p - mean))[-1])
    with np.errstate(all="ignore"):
        r2 = None if tss == 0.0 else float(np.float64(1.0) - np.float64(rss) / np.float64(tss))
    return {"status": ZERO_TSS if tss == 0.0 else OK, "plateau_index": idx, "plateau_height": height,
            "plateau_length": (stop - start + 1)[idx].astype(np.int32), "step_num": step_num, "step_size": step_size, "rss": rss,
            "tss": tss, "r2": r2}


def mul2(x):
    """x * x in the place of pow(x, 2.0): what the table must NOT compute."""
    x = np.asarray(x, dtype=np.float64)
    return x * x


# ---- the golden fixture ------------------------------------------------------------------------------------------------
_G = []


def golden():
    if not _G:
        _G.append(np.load(os.path.join(GOLD, "timetrace_experiment.npz")))
    return _G[0]


def experiment(prefix):
    """One recorded experiment ("s0_", "s1_", "cr_") -> dict: len, photometry, present, hw, keys, ck_filtered, photometries,
    rss, tss, r_2, csv (text), pl / tf (plateau lists per trace) and cols (per trace a dict of the CSV's columns)."""
    g = golden()
    e = {k: g[prefix + k] for k in ("len", "photometry", "present", "hw", "keys", "ck_filtered", "photometries", "rss", "tss", "r_2")}
    e["csv"] = g[prefix + "csv"].tobytes().decode("ascii")
    n = len(e["len"])
    for pre in ("pl", "tf"):
        tr, a, o, h = (g[prefix + pre + "_" + k] for k in ("trace", "start", "stop", "h"))
        e[pre] = [[(int(a[i]), int(o[i]), float(h[i])) for i in np.flatnonzero(tr == t)] for t in range(n)]
    names = [k[len(prefix) + 4:] for k in g.files if k.startswith(prefix + "col_")]
    tr = g[prefix + "col_trace"]
    e["cols"] = [{k: g[prefix + "col_" + k][tr == t] for k in names} for t in range(n)]
    return e


def set_params(k):
    m, ck, pmin, has = golden()["set_params"][k]
    return int(m), int(ck), float(pmin) if has else None


def errors():
    return json.loads(str(golden()["errors_json"]))


def kats():
    return json.loads(str(golden()["kat_json"]))


def records_of(e, params):
    """The recorded numbers of an experiment laid out as timetrace.timetrace_records lays them out (for write_csv)."""
    n, F = e["photometry"].shape
    rec = {"hw": e["hw"].copy(), "present": e["present"], "lengths": e["len"].astype(np.int32), "photometry": e["photometry"],
           "ck_filtered": e["ck_filtered"], "photometries": e["photometries"], "r2": e["r_2"], "params": params}
    rec["hw"][:, 0] = e["keys"]                                    # (the trace's (h, w): its first Spot)
    for k, src in (("step_num", "step_num"), ("plateau_height", "plateau_height"), ("step_size", "step_size"),
                   ("plateau_length", "plateau_length"), ("plateaus_height", "inter_plateaus")):
        a = np.zeros((n, F), e["cols"][0][src].dtype)
        for t in range(n):
            a[t, :e["len"][t]] = e["cols"][t][src]
        rec[k] = a
    return rec


def check_csv_text(got, ref):
    """The project's CSV text against the reference's: the header and every integer / None cell equal, every float cell is
    Python 2's str() of the reference's number, the Photometry cell repr(float) of it (or '0')."""
    from fluorosequencingimageanalysis_amd.pflib import _py2_str
    gl, rl = got.split("\r\n"), ref.split("\r\n")
    assert len(gl) == len(rl) and gl[0] == rl[0] and gl[-1] == rl[-1] == ""
    for i, (a, b) in enumerate(zip(gl[1:-1], rl[1:-1])):
        ca, cb = a.split(","), b.split(",")
        assert len(ca) == len(cb), i
        for j, (x, y) in enumerate(zip(ca, cb)):
            if y == "None" or not any(c in y for c in ".en"):      # (an integer or None; 'e', 'n': exponents, inf, nan)
                assert x == y, (i, j, x, y)
            elif j == 4:
                assert x == repr(float(y)), (i, j, x, y)
            else:
                assert x == _py2_str(float(y)), (i, j, x, y)
