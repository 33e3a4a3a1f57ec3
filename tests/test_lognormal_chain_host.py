"""The lognormal chain on a track table, host side (no GPU needed): the NumPy twin of the records route
(_host_lognormal_chain, lognormal.chain_records(host=True)) against the recorded chain of tests/golden/lognormal_tracks.npz
and against the dict functions lognormal_fitter_v2 runs by default, the table builders, the command line's --device_chain and
--no_intermediates, and the C ABI declarations.  Nothing is compared with a tolerance; NaN equals NaN."""
import ctypes
import os
import re

import numpy as np
import pytest

from fluorosequencingimageanalysis_amd import _host_lognormal as R, _tracks
from _lognormal_cases import chain_csv_text, restated_records
from _lognormal_chain_cases import check_against_record, photometries_of, recorded_table, same_bits, same_chain, table
from _util import ROOT

USED_VALUES = []                # every list of values a bin search of these tests ran on, with the bin count it settled on


@pytest.fixture()
def restated(monkeypatch):
    """The dict route's fit computed by the restatement, as test_lognormal_host does."""
    from fluorosequencingimageanalysis_amd import lognormal as LN

    def records(intensities, categories, means, beta_sigma, max_possible=5, allow_multidrop=True, max_deviation=3, budget=1 << 22,
                lengths=None, device=None):
        return restated_records(R, intensities, categories, means, beta_sigma, max_possible, allow_multidrop, max_deviation, budget)
    monkeypatch.setattr(LN, "lognormal_records", records)


def test_twin_equals_the_recorded_chain():
    from fluorosequencingimageanalysis_amd import lognormal as LN
    rows, cats, fields, tracks = recorded_table()
    assert rows.shape[0] == 444 and len(set(fields.tolist())) == 3
    res = LN.chain_records(rows, cats, fields, 0.2, host=True)
    check_against_record(res, tracks)
    USED_VALUES.append((rows.reshape(-1), int(res["n_bins"])))


def _dict_route(phot, beta_sigma=0.2, max_possible=5, ddif=0.30, allow_multidrop=True, truncate=0, beta=None, no_adjustment=False):
    """lognormal_fitter_v2.main's default computation on a nested dict, with the functions it calls."""
    from fluorosequencingimageanalysis_amd import lognormal as LN
    tracks = list(LN.unwind_photometries(phot))
    raw = tuple(i for t in tracks for i in t[5])
    m0 = LN._get_m0Dm1(raw_photometries=raw)
    alpha = m0[7]
    alpha_adjusted, truncated = {}, {}
    for ch, field, h, w, category, intensities, row in tracks:
        alpha_adjusted.setdefault(ch, {}).setdefault(field, {})[(h, w)] = (category, tuple(i - alpha for i in intensities), row)
        truncated.setdefault(ch, {}).setdefault(field, {})[(h, w)] = (category[truncate:], intensities[truncate:], row)
    beta0, sigma0 = LN.last_drop_method_v2(photometries=truncated)
    if beta is not None:
        beta0 = beta
    quench = tuple([0.0] + [ddif] * (max_possible + 1))
    kw = dict(beta_sigma=beta_sigma, max_possible=max_possible, allow_multidrop=allow_multidrop, max_deviation=3, quench_factors=quench)
    plf0 = LN.photometries_lognormal_fit(photometries=alpha_adjusted, beta=beta0, **kw)
    on_offs = LN.grab_ON_OFFS(plf0[3], alpha_adjust=0)
    with np.errstate(all='ignore'):
        adj = alpha_adjusted if no_adjustment else LN.ON_OFF_adjust_photometries(photometries=phot, ON_OFFS=on_offs, alpha=alpha)
    beta1, sigma1 = LN.last_drop_method_v2(photometries=adj)
    if beta is not None:
        beta1 = beta
    plf1 = LN.photometries_lognormal_fit(photometries=adj, beta=beta1, **kw)
    drops = lambda d, skip: [np.log(i) for t in LN.unwind_photometries(d) for k, i in enumerate(t[5][:-1])      # noqa: E731
                             if k >= skip and t[4][k] and not t[4][k + 1] and i > 0]
    USED_VALUES.extend([(np.array(raw, dtype=np.float64), m0[0]), (np.array(drops(phot, truncate)), None), (np.array(drops(adj, 0)), None)])
    return dict(alpha=alpha, n_bins=m0[0], beta0=beta0, sigma0=sigma0, beta1=beta1, sigma1=sigma1, alpha_adjusted=alpha_adjusted,
                on_offs=on_offs, adj=adj, plf0=plf0, plf1=plf1)


def _same_fit(fit, info, what):
    """A fit's arrays against all_fit_info tuples."""
    for t, f in enumerate(info):
        seq, score, scores = f[9], f[11], f[12]
        if seq is None:
            assert fit["status"][t] == 1 and fit["best_score"][t] == -1 and not fit["best_seq"][t].any(), (what, t)
        else:
            assert fit["status"][t] == 0 and tuple(fit["best_seq"][t].tolist()) == seq, (what, t)
            same_bits([fit["best_score"][t]], [score], (what, t))
            same_bits(fit["frame_score"][t], scores, (what, t))


def _against_dict_route(rows, cats, fields, what, **kw):
    from fluorosequencingimageanalysis_amd import lognormal as LN
    exp = _dict_route(photometries_of(rows, cats, fields), **kw)
    res = LN.chain_records(rows, cats, fields, 0.2, host=True, **kw)
    same_bits([res["alpha"], res["original_beta"], res["original_beta_sigma"], res["adj_beta"], res["adj_beta_sigma"]],
              [exp["alpha"], exp["beta0"], exp["sigma0"], exp["beta1"], exp["sigma1"]], what)
    assert res["n_bins"] == exp["n_bins"], what
    # the dict walks the tracks field by field: `order` is the caller's index of every track it walks (photometries_of's h)
    values = lambda d: np.array([t[5] for t in LN.unwind_photometries(d)], dtype=np.float64)          # noqa: E731
    order = [t[2] for t in LN.unwind_photometries(exp["adj"])]
    same_bits(res["alpha_adjusted"][order], values(exp["alpha_adjusted"]), what)
    same_bits(res["adjusted"][order], values(exp["adj"]), what)
    _same_fit({k: v[order] for k, v in res["fit0"].items()}, exp["plf0"][3], (what, "fit0"))
    _same_fit({k: v[order] for k, v in res["fit1"].items()}, exp["plf1"][3], (what, "fit1"))
    segment_of_field = {f: s for s, f in enumerate(res["field_ids"].tolist())}
    exp_m, exp_n = np.full(res["on_off_median"].shape, np.nan), np.zeros(res["on_off_count"].shape, np.int32)
    for (c, f), drops in exp["on_offs"].items():
        exp_m[segment_of_field[f], c], exp_n[segment_of_field[f], c] = np.median([ion for ion, _ in drops]), len(drops)
    same_bits(res["on_off_median"], exp_m, what)
    same_bits(res["on_off_count"], exp_n, what)
    if exp["on_offs"]:
        same_bits([res["last_beta_median"]], [float(np.median([np.median([ion for ion, _ in d]) for d in exp["on_offs"].values()]))], what)
    _, total, none, info = exp["plf1"]
    signals, _ = _tracks.tally_signals((f[7], f[8], f[13]) for f in sorted(info, key=lambda f: f[2]))     # (in the caller's order)
    assert order != sorted(order) or list(signals.items()) == list(exp["plf1"][0].items())
    assert list(res["signals"].items()) == list(signals.items()) and (res["total_count"], res["none_count"]) == (total, none), what
    return res, exp


CASES = [  # (F, the fields' sizes, keywords)
    (2, [90], {}), (2, [50, 40], dict(beta=9000)), (2, [30, 10, 25, 20, 5], dict(no_adjustment=True)),
    (3, [70], dict(allow_multidrop=False)), (3, [40, 45], {}), (3, [20, 20, 20, 10, 15], dict(beta=9000)),
    (8, [80], dict(truncate=2)), (8, [35, 45], dict(no_adjustment=True, beta=9000)), (8, [20, 1, 30, 25, 14], {}),
    (13, [75], dict(beta=9000)), (13, [40, 35], dict(truncate=2, allow_multidrop=False)), (13, [25, 15, 10, 20, 30], {}),
]


@pytest.mark.parametrize("F,sizes,kw", CASES, ids=["F%d_S%d" % (c[0], len(c[1])) for c in CASES])
def test_twin_equals_the_dict_functions(restated, F, sizes, kw):
    rows, cats, fields = table(1000 + 16 * F + len(sizes), sum(sizes), F, sizes)
    steps = [bin(int(c) & ~(int(c) >> 1) & ((1 << (F - 1)) - 1)).count("1") for c in cats]
    assert (rows <= 0).any() and (F < 4 or sum(s >= 2 for s in steps) >= 5)      # non-positive intensities, several ON -> OFF steps per track
    res, exp = _against_dict_route(rows, cats, fields, (F, sizes), **kw)
    assert (res["on_off_count"] > 0).any() and (res["fit1"]["status"] == 0).any()
    if "beta" in kw:
        assert res["original_beta"] == res["adj_beta"] == 9000
    if kw.get("no_adjustment"):
        same_bits(res["adjusted"], res["alpha_adjusted"], "no_adjustment")


def test_np_histogram_takes_the_linspace_edges():
    """What the device's histogram relies on: with a bin count, np.histogram counts as with np.linspace(lo, hi, n + 1).  On
    every list of values the tests above searched (collected as they ran, with the bin count alpha settled on), and on the raw
    values and the first last-drop list of every table, drawn here again so that the test stands alone."""
    from fluorosequencingimageanalysis_amd import _host_lognormal_chain as HC
    lists = list(USED_VALUES)
    tables = [table(1000 + 16 * F + len(sizes), sum(sizes), F, sizes)[:2] + (kw.get("truncate", 0),) for F, sizes, kw in CASES]
    for rows, cats, truncate in tables + [recorded_table()[:2] + (0,)]:
        lists += [(rows.reshape(-1), None), (HC.last_drops(rows, HC.category_bits(cats, rows.shape[1]), truncate), None)]
    assert len(lists) >= 2 * len(CASES) + 2
    for values, chosen in lists:
        assert len(values) > 1 and values.min() < values.max()
        for n in sorted({chosen or 10, 10, 37, 1000, 10000}):
            assert np.array_equal(np.histogram(values, bins=n)[0],
                                  np.histogram(values, bins=np.linspace(values.min(), values.max(), n + 1))[0]), (len(values), n)


def test_errors_and_degenerate_tables(restated, monkeypatch):
    from fluorosequencingimageanalysis_amd import _host_lognormal_chain as HC, lognormal as LN
    rows, cats, fields = table(77, 60, 5, [25, 35])
    # an empty last-drop list: no ON frame before an OFF one
    with pytest.raises(ValueError):
        LN.chain_records(rows, np.full(60, 31, np.uint64), fields, 0.2, host=True)
    with pytest.raises(ValueError):                                 # ... from frame `truncate` on
        LN.chain_records(rows, np.full(60, 1, np.uint64), fields, 0.2, truncate=1, host=True)
    # a key whose median is 0.  (An entry is the ON intensity of a track with a sequence, which is positive, so no table gives
    # one: the medians are replaced.)
    real = HC.on_off_medians

    def zero_median(*a):
        m, counts, M = real(*a)
        s, f = np.argwhere(counts > 0)[0]
        m[s, f] = 0.0
        return m, counts, M
    monkeypatch.setattr(HC, "on_off_medians", zero_median)
    with pytest.raises(ValueError, match="not finite"):
        LN.chain_records(rows, cats, fields, 0.2, host=True)
    monkeypatch.setattr(HC, "on_off_medians", real)
    # ... and a table that does reach a non-finite adjusted intensity: (I - alpha) * M overflows
    with pytest.raises(ValueError, match="not finite"):
        LN.chain_records(rows * 1e160, cats, fields, 0.2, host=True)
    with pytest.raises((ValueError, IndexError)):                   # (the dict route ends in its second bin search)
        _dict_route(photometries_of(rows * 1e160, cats, fields))
    # 65 frames, ragged rows, one frame, one frame without multi-drop, non-finite intensities, a field missing
    with pytest.raises(NotImplementedError, match="64 frames"):
        LN.chain_records(np.ones((3, 65)), np.ones(3, np.uint64), [0, 0, 0], 0.2, host=True)
    with pytest.raises(ValueError, match="exactly 3"):
        LN.chain_records([[1.0, 2.0, 3.0], [1.0, 2.0]], [(True, False, False), (True, False)], [0, 0], 0.2, host=True)
    with pytest.raises(ValueError):
        LN.chain_records(np.array([[900.0], [950.0], [40.0]]), np.array([1, 1, 0], np.uint64), [0, 0, 0], 0.2, host=True)
    with pytest.raises(ValueError, match="empty"):
        LN.chain_records(np.array([[900.0], [950.0]]), np.array([1, 1], np.uint64), [0, 0], 0.2, allow_multidrop=False, host=True)
    bad = rows.copy()
    bad[3, 2] = np.inf
    with pytest.raises(ValueError, match="finite"):
        LN.chain_records(bad, cats, fields, 0.2, host=True)
    with pytest.raises(ValueError, match="one field per track"):
        LN.chain_records(rows, cats, fields[:-1], 0.2, host=True)
    with pytest.raises(ValueError):
        LN.chain_records(np.zeros((0, 4)), np.zeros(0, np.uint64), [], 0.2, host=True)
    # no key at all (with a beta no intensity is near, no track has a sequence): M is NaN and the adjusted values are the raw ones
    res, _ = _against_dict_route(rows, cats, fields, "no key", beta=1e9)
    assert not (res["on_off_count"] > 0).any() and np.isnan(res["on_off_median"]).all() and np.isnan(res["last_beta_median"])
    same_bits(res["adjusted"], rows, "no key")
    assert res["signals"] == {} and res["none_count"] == res["total_count"] == 60
    # a track over the budget
    with pytest.raises(NotImplementedError, match="budget"):
        LN.chain_records(rows, cats, fields, 0.2, budget=1, host=True)


def test_tracks_in_any_order(restated):
    """Shuffled tracks give the same per-track results in the caller's order, and the tally of that order; the fields stand in
    the order of their first track."""
    from fluorosequencingimageanalysis_amd import lognormal as LN
    rows, cats, fields = table(91, 70, 6, [20, 30, 20])
    base = LN.chain_records(rows, cats, fields, 0.2, host=True)
    perm = np.random.default_rng(3).permutation(70)
    perm = np.concatenate([[65], perm[perm != 65]])                 # (a track of the last field comes first)
    res, _ = _against_dict_route(rows[perm], cats[perm], fields[perm], "shuffled")
    seen = list(dict.fromkeys(fields[perm].tolist()))
    assert res["field_ids"].tolist() == seen and res["field_ids"].tolist() != base["field_ids"].tolist()
    assert np.array_equal(res["field_ids"][res["segment"]], fields[perm])
    back = [base["field_ids"].tolist().index(f) for f in seen]
    exp = dict(base, alpha_adjusted=base["alpha_adjusted"][perm], adjusted=base["adjusted"][perm],
               on_off_median=base["on_off_median"][back], on_off_count=base["on_off_count"][back],
               fit0={k: v[perm] for k, v in base["fit0"].items()}, fit1={k: v[perm] for k, v in base["fit1"].items()})
    del exp["signals"]                                             # (its key order is the other order's)
    same_chain(res, exp, "shuffled")
    assert res["signals"] == base["signals"]


def test_table_builders(tmp_path):
    from fluorosequencingimageanalysis_amd import experiment as EX, lognormal as LN
    from test_lognormal_host import _records
    rec = _records()
    rec["hw"][6] = rec["hw"][0]                                    # (not staying: must not shadow trace 0)
    for method in ("mexican_hat", "simple"):
        rec["photometry_method"] = np.str_(method)
        for channel in ("ch1", "ch2", "ch3"):
            for filt in (True, False):
                got = LN.track_table_from_records(rec, channel, downstep_filtered=filt)
                exp = LN.track_table_from_photometries(LN.photometries_from_records(rec, channel, downstep_filtered=filt))
                assert len(got) == len(exp) == 5
                if len(exp[0]) == 0:
                    assert len(got[0]) == 0
                    continue
                for a, b in zip(got, exp):
                    assert a.dtype == b.dtype
                    same_bits(a, b, (method, channel, filt))
    assert len(LN.track_table_from_records(rec, "ch1")[0]) == 3 and len(LN.track_table_from_records(rec, "ch1", False)[0]) == 4
    # two staying traces at one (field, h, w): the first one stays, as in the dict
    rec["hw"][1] = rec["hw"][0]
    got = LN.track_table_from_records(rec, "ch1", False)
    exp = LN.track_table_from_photometries(LN.photometries_from_records(rec, "ch1", False))
    assert len(got[0]) == 3 and all(np.array_equal(a, b) for a, b in zip(got, exp))
    # renamed channels; and the table of a dict against the dict itself
    got = LN.track_table_from_records(rec, "B", False, channels=["A", "B"])
    assert np.array_equal(got[4], LN.track_table_from_records(rec, "ch2", False)[4]) and len(got[4]) == 2
    rows, cats, fields = table(5, 12, 4, [5, 7])
    phot = photometries_of(rows, cats, fields)
    I, C, Fd, hw, row = LN.track_table_from_photometries(phot)
    same_bits(I, rows, "rows")
    assert np.array_equal(C, cats) and np.array_equal(Fd, fields) and hw.tolist() == [[t, t + 1] for t in range(12)]
    assert row.tolist() == list(range(1, 13))
    with pytest.raises(NotImplementedError, match="multiple channels"):
        LN.track_table_from_photometries(dict(phot, ch2=phot["ch1"]))
    phot["ch1"][2][(0, 1)] = ((True, False), (1.0, 2.0), 1)
    with pytest.raises(ValueError, match="exactly 2"):
        LN.track_table_from_photometries(phot)


def test_command_line_device_chain_writes_the_same_files(restated, tmp_path, capsys):
    """--device_chain (here with the twin, host=True) against the default route with the restated fit: INTERMEDIATES_v2.pkl,
    CLUSTERED.csv, SIGNALS.pkl, RAW_PHOTOMETRIES.pkl and the printed text byte for byte.  COMMANDLINE.pkl holds the command
    line itself, the flag included, and is the same once the flag is taken out of both."""
    import pickle
    from fluorosequencingimageanalysis_amd import lognormal_fitter_v2 as CL
    from fluorosequencingimageanalysis_amd.pflib import _py2_pickle_bytes
    names = ["CLUSTERED.csv", "COMMANDLINE.pkl", "INTERMEDIATES_v2.pkl", "RAW_PHOTOMETRIES.pkl", "SIGNALS.pkl"]

    path = str(tmp_path / "track_photometries_abc123.csv")
    with open(path, "w") as f:
        f.write(chain_csv_text())

    def run(extra, **kw):
        """One run on the one CSV: (result, text, {name: bytes}); the files are taken away for the next run."""
        capsys.readouterr()
        res = CL.main(["lognormal_fitter_v2.py", path] + extra, timestamp_epoch=1500000000, **kw)
        text = capsys.readouterr().out
        base = res["output_filepath_base"]
        files = {}
        for f in sorted(os.listdir(os.path.dirname(base))):
            if f.startswith(os.path.basename(base)):
                full = os.path.join(os.path.dirname(base), f)
                files[f[len(os.path.basename(base)):]] = open(full, "rb").read()
                os.remove(full)
        return res, text, files

    for extra in ([], ["--no_adjustment", "--beta", "9000", "--truncate", "1"]):
        res0, text0, files0 = run(extra)
        res1, text1, files1 = run(extra + ["--device_chain"], host=True)
        assert sorted(files0) == sorted(files1) == names
        assert text0 == text1 and "Signals:" in text0
        for name in names:
            if name == "COMMANDLINE.pkl":
                argv = pickle.loads(files1[name])
                assert argv == ["lognormal_fitter_v2.py", path] + extra + ["--device_chain"]
                argv.remove("--device_chain")
                assert _py2_pickle_bytes(argv) == files0[name]
            else:
                assert files0[name] == files1[name], name
        assert len(files0["INTERMEDIATES_v2.pkl"]) > 100000
        same_bits([res1[k] for k in ("alpha", "original_beta", "original_beta_sigma", "adj_beta", "adj_beta_sigma")],
                  [res0[k] for k in ("alpha", "original_beta", "original_beta_sigma", "adj_beta", "adj_beta_sigma")], extra)
    # --no_intermediates: four files, on either route, the same ones
    _, text2, files2 = run(["--device_chain", "--no_intermediates"], host=True)
    _, text3, files3 = run(["--no_intermediates"])
    assert sorted(files2) == sorted(files3) == [n for n in names if n != "INTERMEDIATES_v2.pkl"]
    assert text2 == text3
    for name in ("CLUSTERED.csv", "RAW_PHOTOMETRIES.pkl", "SIGNALS.pkl"):
        assert files2[name] == files3[name], name
    a = CL.make_parser().parse_args(["t.csv"])
    assert (a.device_chain, a.no_intermediates) == (False, False)


def test_header_matches_binding_and_library():
    from fluorosequencingimageanalysis_amd import _native, _native_lognormal_chain as NC, _native_remainder as NR
    hdr = open(os.path.join(ROOT, "include", "fsq_lognormal_chain.h")).read()
    declared = set(re.findall(r"\b(fsq_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(NC.EXPORTED) == {"fsq_chain_last_drops_workspace_bytes", "fsq_chain_on_off_medians_workspace_bytes",
                                            "fsq_chain_on_off_adjust_workspace_bytes", "fsq_chain_last_drops",
                                            "fsq_chain_on_off_medians", "fsq_chain_on_off_adjust"}
    for name in declared:                                          # the number of parameters of every declaration
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr).group(1)
        assert len(params.split(",")) == len(NC._SIGS[name][1]), name
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    L = ctypes.CDLL(_native.LIB_PATH)
    for name in declared:
        getattr(L, name)
    assert int(re.search(r"#define FSQ_CHAIN_MAX_FRAMES (\d+)", hdr).group(1)) == NC.MAX_FRAMES == NR.MAX_FRAMES == 64
    assert "fsq_lognormal_chain.h" in open(os.path.join(ROOT, "fluorosequencingimageanalysis_amd", "csrc", "Makefile")).read()
    Lb = NC.lib()
    for fn in (Lb.fsq_chain_last_drops_workspace_bytes, Lb.fsq_chain_on_off_medians_workspace_bytes,
               Lb.fsq_chain_on_off_adjust_workspace_bytes):
        assert fn(1000, 64, 3) >= 0 and fn(0, 1, 0) >= 0
        assert fn(1000, 65, 3) < 0 and fn(-1, 8, 3) < 0 and fn(10, 0, 3) < 0 and fn(1 << 31, 8, 3) < 0
    assert Lb.fsq_chain_on_off_medians_workspace_bytes(1000, 12, 3) == 8 + (1000 + 3) * 11 * 8
    assert Lb.fsq_chain_on_off_medians_workspace_bytes(1000, 1, 3) == 8
    assert Lb.fsq_chain_on_off_medians_workspace_bytes(10, 12, -1) < 0 and Lb.fsq_chain_on_off_medians_workspace_bytes(10, 12, 1 << 30) < 0
    assert Lb.fsq_chain_last_drops_workspace_bytes(10, 12, -5) == 0        # (n_segments is not used there)
