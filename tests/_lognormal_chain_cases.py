"""Seeded track tables for the lognormal chain's host and GPU tests, the recorded chain (fixture (b) of
tests/golden/lognormal_tracks.npz) as a table, and the bit-for-bit comparison of two chain results."""
import functools

import numpy as np

from _lognormal_cases import chain_csv_text, golden, random_batch
from _util import bits_equal

SCALARS = ("alpha", "original_beta", "original_beta_sigma", "adj_beta", "adj_beta_sigma", "last_beta_median")
ARRAYS = ("alpha_adjusted", "adjusted", "on_off_median", "on_off_count")
FIT = ("status", "best_seq", "best_score", "frame_score", "n_surviving")


def word_of(category):
    return sum(1 << f for f, c in enumerate(category) if c)


def table(seed, n, F, sizes, beta=10000.0, every=7):
    """n tracks of F frames in fields of `sizes` tracks (contiguous): (rows float64 [n, F], cats uint64 [n], fields int64 [n]).
    random_batch's tracks (mostly ON-prefix categories with lognormal ON frames, normal OFF frames around 40 that are often
    negative, some broken categories, some zeros); the category of every `every`-th track alternates, several ON -> OFF steps."""
    assert sum(sizes) == n
    I, C = random_batch(seed, n, beta=beta, t_lo=F, t_hi=F)
    if every:
        for t in range(3, n, every):
            C[t] = tuple((f + t) % 2 == 0 for f in range(F))
    fields = np.repeat(np.arange(len(sizes)) * 3 + 2, sizes).astype(np.int64)          # (field numbers 2, 5, 8, ...)
    return np.array(I, dtype=np.float64).reshape(n, F), np.array([word_of(c) for c in C], dtype=np.uint64), fields


def photometries_of(rows, cats, fields, channel="ch1"):
    """The table as the nested dict of read_track_photometries_csv: track t at (t, t + 1), row t + 1."""
    F = rows.shape[1]
    d = {}
    for t, (I, c, f) in enumerate(zip(rows.tolist(), cats.tolist(), fields.tolist())):
        d.setdefault(channel, {}).setdefault(f, {})[(t, t + 1)] = (tuple(bool((c >> k) & 1) for k in range(F)), tuple(I), t + 1)
    return d


@functools.lru_cache(maxsize=None)
def recorded_table():
    """(rows, cats, fields, tracks) of the recorded chain's CSV, read as lognormal_fitter_v2 reads it."""
    import os
    import tempfile
    from fluorosequencingimageanalysis_amd import lognormal as LN
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "track_photometries_abc123.csv")
        with open(path, "w") as f:
            f.write(chain_csv_text())
        phot, _ = LN.read_track_photometries_csv(path, head_truncate=0, tail_truncate=0, downstep_filtered=True, channels=["ch1"])
    rows, cats, fields, hw, row = LN.track_table_from_photometries(phot)
    return rows, cats, fields, list(LN.unwind_photometries(phot))


def same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        assert bits_equal(a, b).all(), what
    else:
        assert np.array_equal(a, b), what


def same_chain(got, exp, what=None):
    """Two chain_records / chain_device results (as host values): bit for bit, NaN equal to NaN, the tally with its key order."""
    for k in SCALARS:
        same_bits([got[k]], [exp[k]], (what, k))
    assert int(got["n_bins"]) == int(exp["n_bins"]), what
    for k in ARRAYS:
        same_bits(got[k], exp[k], (what, k))
    for fit in ("fit0", "fit1"):
        for k in FIT:
            same_bits(got[fit][k], exp[fit][k], (what, fit, k))
    for k in ("signals", "total_count", "none_count"):
        if k in got and k in exp:
            assert got[k] == exp[k], (what, k)
    if "signals" in got and "signals" in exp:
        assert list(got["signals"].items()) == list(exp["signals"].items()), what


def check_against_record(res, tracks):
    """A chain_records result on recorded_table() against the recorded chain."""
    from fluorosequencingimageanalysis_amd import _host_lognormal_chain as HC, lognormal_fitter_v2 as CL
    from _lognormal_cases import check_fit_against_record
    g = golden()
    same_bits([res[k] for k in SCALARS[:5]], g["b_scalars"][:5], "scalars")
    assert int(res["n_bins"]) == int(g["b_scalars"][5])
    same_bits(res["alpha_adjusted"], g["b_fit0_intensity"], "alpha_adjusted")
    same_bits(res["adjusted"], g["b_fit1_intensity"], "adjusted")
    for fit, pre, values in (("fit0", "b_fit0_", res["alpha_adjusted"]), ("fit1", "b_fit1_", res["adjusted"])):
        signals, total, none = HC.tally(res[fit]["status"], res[fit]["best_seq"])
        info = CL._chain_fit_info(tracks, res, fit, [tuple(v) for v in values.tolist()], 5)
        check_fit_against_record((signals, total, none, info), pre)
    assert (res["signals"], res["total_count"], res["none_count"]) == HC.tally(res["fit1"]["status"], res["fit1"]["best_seq"])
    # the recorded ON/OFF entries (cycle, field, iON, drop) as per-key medians and counts
    rec = g["b_on_offs"]
    keys = {}
    for c, f, ion, _ in rec.tolist():
        keys.setdefault((int(c), int(f)), []).append(ion)
    segment_of_field = {int(f): s for s, f in enumerate(res["field_ids"].tolist())}
    exp_m, exp_n = np.full(res["on_off_median"].shape, np.nan), np.zeros(res["on_off_count"].shape, np.int32)
    for (c, f), ions in keys.items():
        exp_m[segment_of_field[f], c], exp_n[segment_of_field[f], c] = np.median(ions), len(ions)
    assert len(keys) > 3 and max(map(len, keys.values())) > 3
    same_bits(res["on_off_median"], exp_m, "on_off_median")
    same_bits(res["on_off_count"], exp_n, "on_off_count")
    same_bits([res["last_beta_median"]], [np.median([np.median(v) for v in keys.values()])], "last_beta_median")
