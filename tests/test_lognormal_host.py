"""Lognormal fluor-count fit, host side: the Python restatement against the reference's recorded outputs, the C ABI
declarations, the argument checks of the Python surface, the host pieces of the lognormal_fitter_v2 chain against the recorded
chain, and the command line with the fit computed by the restatement (no GPU needed)."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

from fluorosequencingimageanalysis_amd import _host_lognormal as R
from _lognormal_cases import (chain_csv_text, check_fit_against_record, golden, recorded_fit_info, restated_records,
                              single_cases)
from _util import ROOT, _bits


def test_fixture_is_not_vacuous():
    cases = single_cases()
    none = sum(1 for c in cases if c["best_seq"] is None)
    assert 0.2 * len(cases) <= none <= 0.8 * len(cases)
    assert sum(c["tie"] for c in cases) >= 5 and sum(c["greedy_differs"] for c in cases) >= 10
    assert {c["T"] for c in cases} >= set(range(1, 14)) and {c["max_possible"] for c in cases} == {1, 3, 5, 8, 15}
    assert {c["name"] for c in cases} >= {"prefix", "all_on", "all_off", "off_first", "on_after_off", "nonpositive", "equal", "underflow", "subnormal"}
    assert {c["max_deviation"] for c in cases} == {3, 0.5, 1e9} and {c["multidrop"] for c in cases} == {True, False}
    assert any(c["best_score"] == 0.0 and c["tie"] for c in cases)                    # the all-underflow tie
    # densities that are subnormal doubles: the special-case tail of exp()
    assert sum(1 for c in cases if c["best_seq"] is not None for x in c["frame_score"] if 0.0 < x < 2.2250738585072014e-308) >= 5
    assert any(any(x <= 0 for x, on in zip(c["intensity"], c["category"]) if on) for c in cases)
    assert any(any(x != int(x) for x in c["intensity"]) for c in cases)


def test_restatement_equals_golden():
    for i, c in enumerate(single_cases()):
        got = R.intensities_to_signal(c["intensity"], c["beta_sigma"], c["max_possible"], c["multidrop"], c["max_deviation"],
                                      c["category"], c["means"])
        signal, is_zero, best_seq, lmii, best_score, scores, start = got
        assert (str(signal), is_zero, best_seq, lmii, start) == (c["signal"], c["is_zero"], c["best_seq"], c["lmii"], c["start"]), i
        assert _bits([best_score])[0] == _bits([c["best_score"]])[0], i
        if best_seq is None:
            assert scores is None and best_score == -1
        else:
            assert np.array_equal(_bits(scores), _bits(c["frame_score"])), i
        ok, _ = R.tables(c["intensity"], c["category"], c["means"], c["beta_sigma"], c["max_possible"], c["max_deviation"])
        assert R.count_surviving(ok, c["max_possible"], c["multidrop"]) == c["n_surviving"], i
        assert (c["n_surviving"] == 0) == (c["best_seq"] is None), i


def test_one_frame_without_multidrop_raises_as_recorded():
    """The reference's max() of an empty list (recorded by the generator), from the restatement and from the package."""
    from fluorosequencingimageanalysis_amd import lognormal as LN
    recorded = golden()["a_t1_error"].tolist()
    assert len(recorded) == 3 and all(r.startswith("ValueError: max()") and "empty" in r for r in recorded)
    for I, cat, m in (([10000], (True,), 1), ([30], (False,), 3), ([9000.5], (True,), 5)):
        means = [9.2, 9.6, 10.0, 10.3, 10.5, 10.7, 10.9][:m + 2]
        with pytest.raises(ValueError, match="empty"):
            R.fit(I, cat, means, 0.2, m, False, 3)
        with pytest.raises(ValueError, match="empty"):
            LN.intensities_to_signal_lognormal(I, 1.0, 0.2, m, False, categories=cat, log_fluor_means=means)
        with pytest.raises(ValueError, match="empty"):
            LN.photometries_lognormal_fit({"ch1": {0: {(1, 2): (cat, tuple(I), 1)}}}, 10000.0, 0.2, m, allow_multidrop=False,
                                          quench_factors=(0.0,) + (0.3,) * (m + 1))


def test_header_matches_binding_and_library():
    from fluorosequencingimageanalysis_amd import _native, _native_lognormal as NL
    hdr = open(os.path.join(ROOT, "include", "fsq_lognormal.h")).read()
    declared = set(re.findall(r"\b(fsq_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(NL.EXPORTED) == {"fsq_lognormal_workspace_bytes", "fsq_lognormal_fit", "fsq_lognormal_log"}
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    L = ctypes.CDLL(_native.LIB_PATH)
    for name in declared:
        getattr(L, name)
    P = NL.FsqLognormalParams
    assert (P.beta_sigma.offset, P.max_deviation.offset, P.budget.offset, P.max_possible.offset, P.allow_multidrop.offset,
            ctypes.sizeof(P)) == (136, 144, 152, 160, 164, 168)
    for name, val in (("MAX_FRAMES", NL.MAX_FRAMES), ("MAX_POSSIBLE", NL.MAX_POSSIBLE)):
        assert int(re.search(r"#define FSQ_LOGNORMAL_%s (\d+)" % name, hdr).group(1)) == val
    assert (NL.MAX_BUDGET, NL.DEFAULT_BUDGET) == (1 << 59, 1 << 22)
    assert "(1ll << 59)" in hdr and "(1ll << 22)" in hdr
    for k, name in enumerate(("FOUND", "NONE", "OVER_BUDGET", "INVALID")):
        assert int(re.search(r"#define FSQ_LOGNORMAL_%s (\d+)" % name, hdr).group(1)) == k
    Lb = NL.lib()
    assert Lb.fsq_lognormal_workspace_bytes(1000, 64) == 0 and Lb.fsq_lognormal_workspace_bytes(1000, 65) < 0
    assert Lb.fsq_lognormal_workspace_bytes(-1, 8) < 0 and Lb.fsq_lognormal_workspace_bytes(10, 0) < 0


def test_argument_checks_before_any_launch():
    from fluorosequencingimageanalysis_amd import lognormal as LN
    means = [9.2, 9.6, 10.0, 10.3, 10.5, 10.7, 10.9]
    I, c = [10000, 9000, 50], (True, True, False)
    with pytest.raises(ValueError, match="categories required in v7\\+"):
        LN.intensities_to_signal_lognormal(I, 1.0, 0.2, log_fluor_means=means)
    with pytest.raises(ValueError, match="v8\\+ requires log_fluor_means"):
        LN.intensities_to_signal_lognormal(I, 1.0, 0.2, categories=c)
    with pytest.raises(ValueError, match="empty sequence"):
        LN.intensities_to_signal_lognormal([10000], 1.0, 0.2, allow_multidrop=False, categories=(True,), log_fluor_means=means)
    with pytest.raises(NotImplementedError, match="allow_upsteps"):
        LN.intensities_to_signal_lognormal(I, 1.0, 0.2, allow_upsteps=True, categories=c, log_fluor_means=means)
    for kw, exc in ((dict(max_possible=16), NotImplementedError), (dict(max_possible=0), ValueError),
                    (dict(beta_sigma=0.0), ValueError), (dict(beta_sigma=float("inf")), ValueError),
                    (dict(beta_sigma=float("nan")), ValueError), (dict(max_deviation=float("nan")), ValueError),
                    (dict(budget=0), ValueError), (dict(budget=(1 << 59) + 1), ValueError)):
        args = dict(beta_sigma=0.2, max_possible=5, max_deviation=3)
        args.update(kw)
        with pytest.raises(exc):
            LN.lognormal_records([I], [c], means, **args)
    with pytest.raises(ValueError, match="finite"):
        LN.lognormal_records([[1.0, float("nan")]], [(True, True)], means, 0.2)
    with pytest.raises(ValueError, match="finite"):
        LN.lognormal_records([[1.0, float("inf")]], [(True, True)], means, 0.2)
    with pytest.raises(ValueError, match="finite"):
        LN.lognormal_records([I], [c], [9.2, float("inf")] + means[2:], 0.2)
    with pytest.raises(NotImplementedError, match="64 frames"):
        LN.lognormal_records([[1.0] * 65], [(True,) * 65], means, 0.2)
    with pytest.raises(ValueError, match="width of the rows"):
        LN.lognormal_records(np.ones((2, 3)), np.array([7, 7], np.uint64), means, 0.2, lengths=[3, 4])
    with pytest.raises(ValueError, match="empty sequence"):
        LN.lognormal_records([[]], [()], means, 0.2)
    with pytest.raises(IndexError):
        LN.lognormal_records([I], [c], means[:5], 0.2)
    with pytest.raises(IndexError):
        LN.lognormal_records([I], [c[:2]], means, 0.2)
    phot = {"ch1": {0: {(1, 2): (c, tuple(I), 1)}}}
    with pytest.raises(NotImplementedError, match="multiple channels"):
        LN.photometries_lognormal_fit(dict(phot, ch2=phot["ch1"]), 10000.0, 0.2, quench_factors=(0.0,) + (0.3,) * 6)
    for q in (None, (0.0,) + (0.3,) * 5):
        with pytest.raises(ValueError, match="quench_factors required for v8\\+"):
            LN.photometries_lognormal_fit(phot, 10000.0, 0.2, quench_factors=q)
    with pytest.raises(NotImplementedError, match="multiple channels"):
        LN.last_drop_method_v2(dict(phot, ch2=phot["ch1"]))
    assert LN.lognormal_records([], [], means, 0.2)["status"].shape == (0,)


def test_csv_reader(tmp_path):
    from fluorosequencingimageanalysis_amd import lognormal as LN
    p = tmp_path / "t.csv"
    p.write_text('CHANNEL,FIELD,H,W,CATEGORY,FRAME 0,FRAME 1,FRAME 2\n'
                 'ch1,0,10.5,11.5,"(True, True, False)",0.5,1.5,2.5\n'
                 'ch1,0,12,13,"(True, False, True)",5,6,7\n'
                 'ch2,0,12,13,"(True, False, False)",5,6,7\n'
                 'ch1,1.0,None,3,"(True, False, False)",5,6,7\n'
                 'ch1,1.0,2,3,"(False, False, False)",-0.5,-1.5,-2.4\n'
                 'ch1,0,10.5,11.5,"(True, False, False)",9,9,9\n')
    d, d2 = LN.read_track_photometries_csv(str(p))
    # Python-2 rounding: halves go away from zero (Python 3's round() would give 0, 2, 2 and 10, 12)
    assert d["ch1"][0][(11, 12)] == ((True, True, False), (1, 2, 3), 1)           # (the later row with the same key is dropped)
    assert d["ch1"][1][(2, 3)] == ((False, False, False), (-1, -2, -2), 5)
    assert d["ch2"][0][(12, 13)][2] == 3 and sorted(d2) == [1, 2, 3, 5, 6]
    assert d2[6] == ("ch1", 0, 11, 12, (True, False, False), (9, 9, 9))
    f, _ = LN.read_track_photometries_csv(str(p), downstep_filtered=True, channels=["ch1"])
    assert list(f) == ["ch1"] and list(f["ch1"]) == [0] and list(f["ch1"][0]) == [(11, 12)]
    t, _ = LN.read_track_photometries_csv(str(p), head_truncate=1, tail_truncate=1, channels=["ch2"])
    assert t["ch2"][0][(12, 13)] == ((False,), (6,), 3)
    h, _ = LN.read_track_photometries_csv(str(p), omit_header=False, channels=["ch2"])
    assert h["ch2"][0][(12, 13)][2] == 3
    p.write_text('CHANNEL,FIELD,H,W,CATEGORY,FRAME 0,FRAME 1\nch1,0,1,2,"(True, False)",5,None\n')
    with pytest.raises(ValueError):
        LN.read_track_photometries_csv(str(p))


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """The recorded chain's CSV read back, and the host pieces run on it once."""
    from fluorosequencingimageanalysis_amd import lognormal as LN
    path = tmp_path_factory.mktemp("lognormal") / "track_photometries_abc123.csv"
    path.write_text(chain_csv_text())
    phot, _ = LN.read_track_photometries_csv(str(path), head_truncate=0, tail_truncate=0, downstep_filtered=True, channels=["ch1"])
    tracks = list(LN.unwind_photometries(phot))
    raw = tuple(i for t in tracks for i in t[5])
    return dict(path=str(path), phot=phot, tracks=tracks, raw=raw, m0=LN._get_m0Dm1(raw_photometries=raw))


def test_chain_reader_and_alpha(chain):
    g = golden()
    text = chain_csv_text()
    assert ".5," in text and "ch2," in text and "None,None" in text
    assert len(chain["tracks"]) == int(g["b_fit0_counts"][0]) < text.count("\n") - 3
    assert [(t[1], t[2], t[3], t[6]) for t in chain["tracks"]] == list(zip(g["b_fit0_field"].tolist(), g["b_fit0_h"].tolist(),
                                                                          g["b_fit0_w"].tolist(), g["b_fit0_row"].tolist()))
    assert chain["m0"][0] == int(g["b_scalars"][5])
    alpha = chain["m0"][7]
    assert _bits([alpha])[0] == _bits(g["b_scalars"][:1])[0]
    adjusted = np.array([[i - alpha for i in t[5]] for t in chain["tracks"]])
    assert np.array_equal(_bits(adjusted), _bits(g["b_fit0_intensity"]))


def test_chain_bin_search_beta_and_adjustment(chain):
    from fluorosequencingimageanalysis_amd import lognormal as LN
    g = golden()
    alpha = chain["m0"][7]
    min_cost, where, costs = LN.optimal_bin_size(chain["raw"])
    assert costs.shape == (91, 1) and min_cost == costs.min() and LN.optimal_bin_count(chain["raw"], 10, 100) == 10 + int(where[0][0])
    beta0, sigma0 = LN.last_drop_method_v2(chain["phot"])
    assert np.array_equal(_bits([beta0, sigma0]), _bits(g["b_scalars"][1:3]))
    on_offs = LN.grab_ON_OFFS(recorded_fit_info("b_fit0_"), alpha_adjust=0)
    flat = [(c, f, ion, d) for (c, f), drops in on_offs.items() for ion, d in drops]
    assert np.array_equal(_bits(np.array(flat, dtype=np.float64)), _bits(g["b_on_offs"]))
    with pytest.raises(TypeError):                                # (the swapped branches: without alpha_adjust, iON - None)
        LN.grab_ON_OFFS(recorded_fit_info("b_fit0_"))
    bad = LN.grab_ON_OFFS(recorded_fit_info("b_fit0_"), allow_bad_fits=True, alpha_adjust=2.0)
    assert all(d is None for drops in bad.values() for _, d in drops) and sum(map(len, bad.values())) >= len(flat)
    adj = LN.ON_OFF_adjust_photometries(chain["phot"], on_offs, alpha)
    got = np.array([t[5] for t in LN.unwind_photometries(adj)], dtype=np.float64)
    assert np.array_equal(_bits(got), _bits(g["b_fit1_intensity"]))
    beta1, sigma1 = LN.last_drop_method_v2(adj)
    assert np.array_equal(_bits([beta1, sigma1]), _bits(g["b_scalars"][3:5]))
    assert beta1 != beta0


def _records(F=4):
    """A hand-made sequence_experiment_records dict: 2 fields x 2 channels, 7 traces."""
    from fluorosequencingimageanalysis_amd import _native_sequence as NQ
    D, I = NQ.DETECTED, NQ.INTERPOLATED
    seq = np.array([0, 0, 1, 2, 2, 3, 0], np.int32)                # sequence = field * C + channel
    cat = np.array([0b0011, 0b0001, 0b0111, 0b0101, 0b1111, 0b0001, 0b0011], np.uint64)
    flags = np.array([[D, D, I, I], [D, 0, 0, 0], [D, D, D, I], [D, I, D, I], [D, D, D, D], [0, D, I, I], [D, D, I, I]], np.int32)
    rng = np.random.default_rng(5)
    phot = np.floor(rng.uniform(-200, 20000, (7, F))) + np.array([0.5, 0.25, 0.0, 0.5])[None, :]
    hw = rng.integers(3, 200, (7, F, 2)).astype(np.int32)
    return {"shape": np.array([2, 2, F, 256, 256], np.int64), "trace_seq": seq, "category": cat, "flags": flags, "hw": hw,
            "photometry": phot, "trace_valid": np.array([1, 1, 1, 1, 1, 1, 0], bool), "keep_invalid": np.bool_(False),
            "photometry_method": np.str_("mexican_hat")}


def test_photometries_from_records_equals_the_csv_round_trip(tmp_path):
    from fluorosequencingimageanalysis_amd import experiment as EX, lognormal as LN
    rec = _records()
    path = str(tmp_path / "track_photometries.csv")
    assert EX.write_track_photometries_csv(path, rec, save_averages=False) == 6
    for channel in ("ch1", "ch2"):
        for filt in (True, False):
            exp, _ = LN.read_track_photometries_csv(path, downstep_filtered=filt, channels=[channel])
            got = LN.photometries_from_records(rec, channel, downstep_filtered=filt)
            assert got == exp and [list(v) for v in got.values()] == [list(v) for v in exp.values()]
            assert all(list(got[c][e]) == list(exp[c][e]) for c in got for e in got[c])
    assert sum(len(fd) for fd in LN.photometries_from_records(rec, "ch1")["ch1"].values()) == 3     # (0b0101 is not a downstep)
    rec["photometry_method"] = np.str_("simple")
    EX.write_track_photometries_csv(path, rec, save_averages=False)
    assert LN.photometries_from_records(rec, "ch2", False) == LN.read_track_photometries_csv(path, channels=["ch2"])[0]


def test_command_line_parsing():
    from fluorosequencingimageanalysis_amd import lognormal_fitter_v2 as CL
    a = CL.make_parser().parse_args(["t.csv"])
    assert (a.tracks, a.channel, a.wavelength, a.num_mocks, a.num_mocks_omitted, a.num_edmans, a.sequence, a.num_processors) == \
        (["t.csv"], 1, 0, 4, 1, 8, None, None)
    assert (a.max_possible, a.max_deviation, a.ddif, a.beta_sigma, a.beta, a.no_adjustment, a.no_multidrop, a.truncate) == \
        (5, 3, 0.30, 0.20, None, False, False, 0)
    a = CL.make_parser().parse_args("t.csv -c 2 -w 647 -m 3 -o 0 -e 9 -s AK -n 4 --max_possible 3 --max_deviation 2 --ddif 0.1 "
                                    "--beta_sigma 0.3 --beta 9000 --no_adjustment --no_multidrop --truncate 2".split())
    assert (a.channel, a.wavelength, a.num_mocks, a.num_mocks_omitted, a.num_edmans, a.sequence, a.num_processors, a.max_possible,
            a.max_deviation, a.ddif, a.beta_sigma, a.beta, a.no_adjustment, a.no_multidrop, a.truncate) == \
        (2, 647, 3, 0, 9, "AK", 4, 3, 2, 0.1, 0.3, 9000.0, True, True, 2)
    with pytest.raises(SystemExit):
        CL.make_parser().parse_args([])


def test_command_line_files_and_text_with_the_restated_fit(chain, monkeypatch, capsys):
    from fluorosequencingimageanalysis_amd import lognormal as LN, lognormal_fitter_v2 as CL
    g = golden()
    seen = []

    def records(intensities, categories, means, beta_sigma, max_possible=5, allow_multidrop=True, max_deviation=3, budget=1 << 22,
                lengths=None, device=None):
        seen.append(max_deviation)
        return restated_records(R, intensities, categories, means, beta_sigma, max_possible, allow_multidrop, max_deviation, budget)
    monkeypatch.setattr(LN, "lognormal_records", records)
    argv = ["lognormal_fitter_v2.py", chain["path"], "--max_deviation", "7", "-n", "3"]
    res = CL.main(argv, timestamp_epoch=1500000000)
    assert seen == [3, 3]                                          # (--max_deviation is parsed; the fit gets 3)
    check_fit_against_record(res["original_plf_results"], "b_fit0_")
    check_fit_against_record(res["plf_results"], "b_fit1_")
    assert np.array_equal(_bits([res["alpha"], res["original_beta"], res["original_beta_sigma"], res["adj_beta"], res["adj_beta_sigma"]]),
                          _bits(g["b_scalars"][:5]))
    base = res["output_filepath_base"]
    assert base == chain["path"] + "_ot27eo_ch1_"
    assert sorted(f[len(os.path.basename(base)):] for f in os.listdir(os.path.dirname(base)) if f.startswith(os.path.basename(base))) == \
        ["CLUSTERED.csv", "COMMANDLINE.pkl", "INTERMEDIATES_v2.pkl", "RAW_PHOTOMETRIES.pkl", "SIGNALS.pkl"]
    assert os.path.getsize(base + "CLUSTERED.csv") == 0
    for name in ("COMMANDLINE.pkl", "INTERMEDIATES_v2.pkl", "SIGNALS.pkl", "RAW_PHOTOMETRIES.pkl"):
        raw = open(base + name, "rb").read()
        assert raw[:1] in (b"(", b"c") and raw.endswith(b".") and b"\x80" not in raw[:2]     # protocol 0: text opcodes, no PROTO
    signals = res["plf_results"][0]
    assert pickle.load(open(base + "COMMANDLINE.pkl", "rb")) == argv
    assert pickle.load(open(base + "SIGNALS.pkl", "rb")) == signals
    assert pickle.load(open(base + "RAW_PHOTOMETRIES.pkl", "rb")) == chain["raw"]
    (alpha, adj_beta, beta_sigma, ddif), plf, args = pickle.load(open(base + "INTERMEDIATES_v2.pkl", "rb"))
    assert (alpha, adj_beta, beta_sigma, ddif) == (res["alpha"], res["adj_beta"], 0.2, (0.0,) + (0.3,) * 6)
    assert plf[0] == signals and plf[1:3] == res["plf_results"][1:3] and args.max_deviation == 7 and args.num_processors == 3
    lines = capsys.readouterr().out.split("\n")
    assert lines[0] == "Using timestamp_hash ot27eo" and lines[1:3] == ["", "Signals:"]
    body = lines[3:3 + len(signals)]
    assert body == [str(k) + "    " + str(n) for k, n in sorted(signals.items(), key=lambda x: x[0])]
    rest = lines[3 + len(signals):]
    assert rest[0] == "Total number of signals: %d" % sum(signals.values())
    assert rest[1] == "Total number of signals that fall to 0: %d" % sum(n for (s, z, si), n in signals.items() if z)
    assert rest[2] == "" and [x.split(" using ")[0] for x in rest[3:6]] == \
        ["Error saving histogram", "Error saving single drops heatmap", "Error saving double drops heatmap"]
    assert all("not built" in x for x in rest[3:6])
    # --no_adjustment fits the alpha-adjusted dict twice; --beta overrides both betas
    res2 = CL.main(["x", chain["path"], "--no_adjustment", "--beta", "9000"], timestamp_epoch=1500000001)
    assert res2["original_beta"] == res2["adj_beta"] == 9000.0 and res2["plf_results"] == res2["original_plf_results"]
