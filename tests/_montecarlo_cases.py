"""Shared by the Monte-Carlo fit tests: the golden (tests/golden/montecarlo.npz, the reference under this library's draws), the
twin's answers in the layout of the C ABI, and bit comparisons."""
import functools
import os

import numpy as np

from fluorosequencingimageanalysis_amd import _host_montecarlo as T
from fluorosequencingimageanalysis_amd import _native as N
from _util import GOLD

STATUS_OF = {"": T.OK, "UnboundLocalError": T.NEVER_IMPROVED, "IndexError": T.NO_MAXIMUM}
FLOAT_FIELDS = ("h0", "w0", "H", "A", "sigma_h", "sigma_w", "theta", "rmse", "r2", "s_n", "p2", "p3")
INT_FIELDS = ("h", "w", "field", "status", "niter", "nfev", "key_h", "key_w")
FIELD_TAGS = ("f5_default", "f5_low", "f5_low_field7", "tiny")


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLD, "montecarlo.npz"))


def bits(a):
    """uint64 view of doubles, every NaN mapped to one pattern (x86 and the GPU give 0 / 0 different signs)."""
    a = np.ascontiguousarray(a, dtype=np.float64).copy()
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def twin_table(key):
    """The twin on a tuple of (roi bytes, n_iter, seed, pixel, field, h, w, cand_field) -> dict(rows, fit, rms, status) as the
    C ABI lays them out; computed once per distinct request."""
    rows = np.zeros(len(key), N.ROW_DTYPE)
    fit, rms, status = np.zeros((len(key), 25)), np.zeros(len(key)), np.zeros(len(key), np.int32)
    for i, (roi, n_iter, seed, pixel, field, h, w, cf) in enumerate(key):
        r = T.fit_roi(np.frombuffer(roi, np.float64), n_iter, seed, pixel, field, h, w, cf)
        for k, v in r["row"].items():
            rows[k][i] = v
        fit[i], rms[i], status[i] = r["fit"], r["rms"], r["status"]
    return {"rows": rows, "fit": fit, "rms": rms, "status": status}


def twin_rois(rois, ids, n_iter, seed):
    rois = np.ascontiguousarray(rois, dtype=np.float64).reshape(-1, 25)
    return twin_table(tuple((rois[i].tobytes(), int(n_iter), int(seed), int(ids[i][0]), int(ids[i][1]), 2, 2, 0) for i in range(len(rois))))


def same_tables(got, exp, what=""):
    assert np.array_equal(got["status"], exp["status"]), what
    for k in INT_FIELDS:
        assert np.array_equal(got["rows"][k], exp["rows"][k]), (what, k)
    for k in FLOAT_FIELDS:
        assert same(got["rows"][k], exp["rows"][k]), (what, k)
    assert same(got["fit"], exp["fit"]) and same(got["rms"], exp["rms"]), what


def golden_roi_case(n_iter):
    """The recorded answers of the reference for every golden ROI at one N_iter."""
    g = golden()
    pre = "n%d_" % n_iter
    return {"status": np.array([STATUS_OF[str(t)] for t in g[pre + "exc_type"]], np.int32), "params": g[pre + "params"],
            "fit": g[pre + "fit"].reshape(-1, 25), "rms": g[pre + "rms"], "niter": g[pre + "niter"],
            "exc_type": [str(t) for t in g[pre + "exc_type"]], "exc_text": [str(t) for t in g[pre + "exc_text"]],
            "types": [str(t) for t in g[pre + "types"]]}


def rows_match_golden(rows, fit, rms, status, exp):
    """FsqRow tables (h = w = 2) against golden_roi_case: the seven parameters, the image, the kept RMS and the winner."""
    assert np.array_equal(status, exp["status"])
    ok = exp["status"] == T.OK
    got7 = np.stack([rows[k] for k in ("p2", "p3", "H", "A", "sigma_h", "sigma_w", "theta")], axis=1)
    assert same(got7[ok], exp["params"][ok])
    assert same(rows["h0"][ok], exp["params"][ok, 0] + 2.0 - 2.5) and same(rows["w0"][ok], exp["params"][ok, 1] + 2.0 - 2.5)
    assert same(fit[ok], exp["fit"][ok]) and same(rms[ok], exp["rms"][ok])
    assert np.array_equal(rows["niter"][ok], exp["niter"][ok]) and (rows["niter"][~ok] == -1).all()


def field_image(tag):
    g = golden()
    if tag.startswith("f5"):
        return np.load(os.path.join(GOLD, "field_f5_small_96.npz"))["image"]
    return g[tag + "_image"]


def field_kwargs(tag):
    g = golden()
    kw = dict(fit_type='monte_carlo', N_iter=int(g["field_n_iter"]), seed=int(g["field_seed"][0]))
    if tag != "f5_default":
        kw["r_2_threshold"] = float(g["low_threshold"])
    if tag == "f5_low_field7":
        kw["first_field"] = 7
    return kw


def dict_matches_golden(d, tag):
    """A find_peptides dict against the reference's recorded one: keys in order, values bit for bit, value types by name."""
    g = golden()
    keys = [tuple(int(x) for x in k) for k in g[tag + "_keys"]]
    assert list(d.keys()) == keys
    vals = list(d.values())
    if not vals:
        return
    assert same(np.array([[float(x) for x in v[:7]] for v in vals]), g[tag + "_t7"])
    assert same(np.array([v[7] for v in vals]), g[tag + "_sub"]) and same(np.array([v[8] for v in vals]), g[tag + "_fit"])
    assert same(np.array([[float(v[9]), float(v[10]), float(v[11])] for v in vals]), g[tag + "_metrics"])
    assert ",".join(type(x).__name__ for x in vals[0]) == str(g[tag + "_types"][0])
    assert ",".join(type(x).__name__ for x in list(d.keys())[0]) == str(g[tag + "_key_types"][0])
    assert all(v[7].shape == (5, 5) and v[8].shape == (5, 5) and v[7].dtype == np.float64 for v in vals)


@functools.lru_cache(maxsize=None)
def upper_clip_case():
    """(roi [1, 25] with its maximum at (4, 4), ids, n_iter, seed) such that the LAST iteration draws h_0 = N(4, .3) above
    4.99: the clipped centre is in the image the fit returns."""
    seed, ids = 4242, np.array([[123456, 9]], np.uint32)
    z = T.normals_np(seed, 0, 30000, 123456, 9)
    hit = np.nonzero(4.0 + 0.3 * z[:, 2] > 4.99)[0]
    assert len(hit), "no draw above the upper clip among 30 000 iterations"
    rng = np.random.default_rng(5)
    roi = rng.uniform(0.0, 0.6, (1, 25))
    roi[0, 24] = 1.0
    return roi, ids, int(hit[0]) + 1, seed
