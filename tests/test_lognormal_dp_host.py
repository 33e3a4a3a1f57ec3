"""The lognormal fit by exact dynamic programme, host side (no GPU needed): the plain Python twin (_host_lognormal_dp) against
a brute-force restatement of the reference's loop on seeded tables, against the reference's recorded outputs with and without
upsteps, `min_prefix` at its edges, the overflow refusal, the C ABI declarations, and solver='dp' through chain_records and the
command line with the twin.  Nothing is compared with a tolerance."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

from fluorosequencingimageanalysis_amd import _host_lognormal as R, _host_lognormal_dp as D
from _lognormal_cases import chain_csv_text, single_cases
from _lognormal_chain_cases import same_chain, table
from _lognormal_dp_cases import brute_force, seeded_tables, twin_records, upstep_cases
from _util import ROOT, _bits

MEANS = [9.2, 9.6, 10.0, 10.3, 10.5, 10.7, 10.9]


def _same_fit(got, exp, what):
    seq, score, scores, n = got
    assert seq == exp[0], what
    assert _bits([score])[0] == _bits([exp[1]])[0], what
    if exp[0] is None:
        assert scores is None and score == -1, what
    else:
        assert np.array_equal(_bits(scores), _bits(exp[2])), what
    assert n == exp[3] and type(n) is int, what


def test_twin_equals_brute_force_on_seeded_tables():
    tabs = seeded_tables()
    assert len(tabs) >= 3000
    several = none = 0
    seen = set()
    for i, (kind, ok, score, m, multi, ups) in enumerate(tabs):
        exp = brute_force(ok, score, m, multi, ups)
        _same_fit(D.fit_tables(ok, score, m, multi, ups), exp, (i, kind, m, multi, ups))
        several += exp[0] is not None and exp[4] > 1
        none += exp[0] is None
        seen.add((kind, len(ok), m, multi, ups))
    assert several >= 500 and none >= 300, (several, none)
    assert {s[1] for s in seen} == set(range(1, 7)) and {s[2] for s in seen} == {1, 2, 3, 4}
    assert {(s[0], s[3], s[4]) for s in seen} == {(k, a, b) for k in ("realistic", "adversarial") for a in (True, False) for b in (True, False)}


def test_upstep_fixture_is_not_vacuous():
    cases = upstep_cases()
    n = len(cases)
    ups = sum(c["upstep"] for c in cases)
    none = sum(c["best_seq"] is None for c in cases)
    ties = sum(c["tie"] for c in cases)
    assert ups >= 30 and none >= 20 and ties >= 5 and max(ups, none, ties) <= 0.6 * n
    assert all((c["signal"] == "None") == (c["best_seq"] is None or c["upstep"]) for c in cases)
    assert {c["T"] for c in cases} == set(range(1, 7)) and {c["max_possible"] for c in cases} == {1, 3, 5}
    assert {c["max_deviation"] for c in cases} == {3, 0.5, 1e9} and {c["multidrop"] for c in cases} == {True, False}
    assert {c["name"] for c in cases} >= {"rising", "prefix", "on_after_off", "nonpositive", "underflow", "subnormal"}
    assert any(c["best_score"] == 0.0 and c["tie"] for c in cases)
    assert sum(1 for c in cases if c["best_seq"] is not None for x in c["frame_score"] if 0.0 < x < 2.2250738585072014e-308) >= 5
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "lognormal_upsteps.npz")) <= \
        os.path.getsize(os.path.join(ROOT, "tests", "golden", "lognormal_tracks.npz"))


def test_twin_equals_the_recorded_upstep_fits():
    from fluorosequencingimageanalysis_amd import lognormal as LN
    for i, c in enumerate(upstep_cases()):
        got = D.fit(c["intensity"], c["category"], c["means"], c["beta_sigma"], c["max_possible"], c["multidrop"], c["max_deviation"],
                    allow_upsteps=True)
        _same_fit(got, (c["best_seq"], c["best_score"] if c["best_seq"] is not None else -1, c["frame_score"], c["n_surviving"]), i)
        if c["best_seq"] is not None:
            signal, is_zero, start = LN.signal_of(c["best_seq"])
            assert (str(signal), is_zero, start) == (c["signal"], c["is_zero"], c["start"]), i


def test_twin_without_upsteps_equals_the_recorded_fits():
    """The reference's own outputs of tests/golden/lognormal_tracks.npz, every single-track record."""
    cases = single_cases()
    assert len(cases) > 300
    for i, c in enumerate(cases):
        got = D.fit(c["intensity"], c["category"], c["means"], c["beta_sigma"], c["max_possible"], c["multidrop"], c["max_deviation"])
        _same_fit(got, (c["best_seq"], c["best_score"] if c["best_seq"] is not None else -1, c["frame_score"], c["n_surviving"]), i)
    with pytest.raises(ValueError, match="empty"):
        D.fit([10000], (True,), MEANS, 0.2, 5, False, 3)


def _least_by_definition(s, n):
    """min_prefix's answer checked from its definition: it passes, and the double below it does not."""
    p = D.min_prefix(s, n)
    assert p * s >= n
    assert p == 0.0 or not np.nextafter(p, 0.0) * s >= n
    return p


def test_min_prefix_edges():
    inf, tiny = float("inf"), 5e-324
    assert D.min_prefix(0.0, 0.0) == 0.0 and D.min_prefix(0.0, -1.0) == 0.0 and D.min_prefix(0.0, tiny) == inf     # s = 0
    assert D.min_prefix(0.5, 0.0) == 0.0 and D.min_prefix(1e-300, 0.0) == 0.0                                     # n = 0
    # n = 5e-324 with s = 2^-60: products up to 2^-1075 round to 0 (ties to even), so the least p is the double above 2^-1015
    p = _least_by_definition(2.0 ** -60, tiny)
    assert p == np.nextafter(2.0 ** -1015, 1.0) and 2.0 ** -1015 * 2.0 ** -60 == 0.0
    # s and n subnormal: n / s is an ordinary double and the answer is near it
    for s, n in ((1e-310, 3e-320), (tiny, tiny), (tiny, 1e-310), (2e-308, tiny), (3e-310, 2.2250738585072014e-308)):
        p = _least_by_definition(s, n)
        assert 0.0 < p < inf
    assert D.min_prefix(tiny, tiny) == 0.5 + 2.0 ** -53                                 # (0.5 * 5e-324 ties to 0; the next double rounds up)
    # no finite answer: the greatest double times s stays below n
    assert D.min_prefix(1e-300, 1e10) == inf and D.min_prefix(tiny, 1e-10) == inf and D.min_prefix(0.5, inf) == inf
    assert D.min_prefix(1e-300, 1.7e8) < inf
    # ordinary values, and values whose quotient is off by an ulp either way
    rng = np.random.default_rng(5)
    for _ in range(2000):
        s = float(rng.choice([rng.uniform(1e-3, 3.0), 10.0 ** rng.uniform(-320, -290), 10.0 ** rng.uniform(-20, 2)]))
        n = float(rng.choice([rng.uniform(1e-6, 1.0), 10.0 ** rng.uniform(-323, -300), 10.0 ** rng.uniform(-200, 0)]))
        if s > 0.0 and n > 0.0:
            _least_by_definition(s, n) if D.min_prefix(s, n) < inf else None


def test_overflow_refusal():
    """peak = 1 / (sqrt(2 pi) * beta_sigma) > 1 and max_frames * log(peak) >= 700: refused by the twin and by the package,
    before anything is launched."""
    from fluorosequencingimageanalysis_amd import lognormal as LN
    assert not D.may_overflow(0.2, 64) and not D.may_overflow(0.39, 64) and not D.may_overflow(1e-4, 64)       # 64 * log(3989) = 531
    assert not D.may_overflow(1e-5, 64)                                                                        # 64 * log(39894) = 678
    assert D.may_overflow(5e-6, 64) and D.may_overflow(5e-6, 63) and not D.may_overflow(5e-6, 62)              # log(79788) = 11.287: 722, 711, 699.8
    assert D.may_overflow(1e-300, 2) and not D.may_overflow(1e-300, 1) and D.may_overflow(5e-324, 1)
    I, c = [10000.0] * 64, (True,) * 64
    with pytest.raises(ValueError, match="overflow"):
        D.fit(I, c, MEANS, 5e-6, 5, True, 1e9)
    with pytest.raises(ValueError, match="overflow"):
        LN.lognormal_records([I], [c], MEANS, 5e-6, solver='dp')
    with pytest.raises(ValueError, match="overflow"):
        LN.intensities_to_signal_lognormal(I, 1.0, 5e-6, categories=c, log_fluor_means=MEANS, solver='dp')
    with pytest.raises(ValueError, match="overflow"):
        LN.chain_records(np.full((3, 64), 1e4), np.full(3, 2 ** 64 - 1, np.uint64), [0, 0, 0], 5e-6, beta=1e4, host=True, solver='dp')
    assert D.fit(I[:62], c[:62], MEANS, 5e-6, 5, True, 1e9)[:2] == ((5,) * 62, 0.0)     # (62 frames: served; every density underflows)


def test_header_matches_binding_and_library():
    from fluorosequencingimageanalysis_amd import _native, _native_lognormal as NL, _native_lognormal_dp as ND
    hdr = open(os.path.join(ROOT, "include", "fsq_lognormal_dp.h")).read()
    declared = set(re.findall(r"\b(fsq_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(ND.EXPORTED) == {"fsq_lognormal_dp_workspace_bytes", "fsq_lognormal_fit_dp"}
    assert '#include "fsq_lognormal.h"' in hdr and "700" in hdr and ND.FsqLognormalParams is NL.FsqLognormalParams
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    L = ctypes.CDLL(_native.LIB_PATH)
    for name in declared:
        getattr(L, name)
    Lb = ND.lib()
    assert Lb.fsq_lognormal_dp_workspace_bytes(1000, 64) == 0 and Lb.fsq_lognormal_dp_workspace_bytes(1000, 65) < 0
    assert Lb.fsq_lognormal_dp_workspace_bytes(-1, 8) < 0 and Lb.fsq_lognormal_dp_workspace_bytes(10, 0) < 0
    # refused by the C entry before any launch (no GPU is touched): bad parameters and the overflow condition
    prm = NL.FsqLognormalParams()
    for i, x in enumerate(MEANS):
        prm.log_fluor_means[i] = x
    prm.beta_sigma, prm.max_deviation, prm.budget, prm.max_possible, prm.allow_multidrop = 5e-6, 3.0, 0, 5, 1
    EINVAL = Lb.fsq_lognormal_fit_dp(None, None, None, 1, 65, ctypes.byref(prm), None, None, None, None, None, 0, None, 0, None)
    assert EINVAL != 0
    assert Lb.fsq_lognormal_fit_dp(None, None, None, 1, 64, ctypes.byref(prm), None, None, None, None, None, 0, None, 0, None) == EINVAL
    assert Lb.fsq_lognormal_fit_dp(None, None, None, 0, 64, ctypes.byref(prm), None, None, None, None, None, 0, None, 0, None) == EINVAL
    assert Lb.fsq_lognormal_fit_dp(None, None, None, 0, 62, ctypes.byref(prm), None, None, None, None, None, 0, None, 0, None) == 0    # (budget 0 is ignored)


def test_solver_and_upsteps_errors():
    from fluorosequencingimageanalysis_amd import lognormal as LN
    I, c = [10000, 9000, 50], (True, True, False)
    phot = {"ch1": {0: {(1, 2): (c, tuple(I), 1)}}}
    q = (0.0,) + (0.3,) * 6
    for call in (lambda **kw: LN.intensities_to_signal_lognormal(I, 1.0, 0.2, categories=c, log_fluor_means=MEANS, **kw),
                 lambda **kw: LN.photometries_lognormal_fit(phot, 10000.0, 0.2, quench_factors=q, **kw),
                 lambda **kw: LN.lognormal_records([I], [c], MEANS, 0.2, **kw)):
        with pytest.raises(NotImplementedError, match=r"allow_upsteps.*solver='dp'"):
            call(allow_upsteps=True)
        with pytest.raises(NotImplementedError, match=r"allow_upsteps.*solver='dp'"):
            call(allow_upsteps=True, solver='enumerate')
        for bad in ('DP', 'exact', None, 1):
            with pytest.raises(ValueError, match="solver must be 'enumerate' or 'dp'"):
                call(solver=bad)
    rows, cats, fields = table(91, 12, 4, [5, 7])
    with pytest.raises(ValueError, match="solver must be 'enumerate' or 'dp'"):
        LN.chain_records(rows, cats, fields, 0.2, host=True, solver='fast')
    with pytest.raises(TypeError):
        LN.chain_records(rows, cats, fields, 0.2, host=True, solver='dp', allow_upsteps=True)      # (not through the chain)
    from fluorosequencingimageanalysis_amd import lognormal_fitter_v2 as CL
    assert CL.make_parser().parse_args(["t.csv"]).solver == 'enumerate'
    assert CL.make_parser().parse_args(["t.csv", "--solver", "dp"]).solver == 'dp'
    with pytest.raises(SystemExit):
        CL.make_parser().parse_args(["t.csv", "--solver", "fast"])


def test_dict_interfaces_with_the_twin(monkeypatch):
    """allow_upsteps through the two dict interfaces with the launch stood in for by the twin: a winner that steps up has no
    signal, keeps its sequence and counts towards none_count."""
    from fluorosequencingimageanalysis_amd import lognormal as LN
    seen = []

    def records(intensities, categories, means, beta_sigma, max_possible=5, allow_multidrop=True, max_deviation=3, budget=1 << 22,
                lengths=None, device=None, solver='enumerate', allow_upsteps=False):
        seen.append((solver, allow_upsteps, budget))
        return twin_records(D, intensities, categories, means, beta_sigma, max_possible, allow_multidrop, max_deviation, allow_upsteps)
    monkeypatch.setattr(LN, "lognormal_records", records)
    cases = upstep_cases()
    for c in cases:
        got = LN.intensities_to_signal_lognormal(c["intensity"], 1.0, c["beta_sigma"], c["max_possible"], c["multidrop"], True,
                                                 c["max_deviation"], categories=c["category"], log_fluor_means=c["means"],
                                                 solver='dp', budget=1)
        assert (str(got[0]), got[1], got[2], got[3], got[6]) == (c["signal"], c["is_zero"], c["best_seq"], c["max_possible"], c["start"])
        assert _bits([got[4]])[0] == _bits([c["best_score"]])[0]
        if c["upstep"]:
            assert got[0] is None and got[1] is None and got[2] is not None and got[6] == got[2][0]
            assert np.array_equal(_bits(got[5]), _bits(c["frame_score"]))
    assert seen and all(s == ('dp', True, 1) for s in seen)
    # one batch: beta 10 000 gives the means of means_for(10000, 3)
    I, C = [[9000.0, 21000.0, 9500.0], [9000.0, 8000.0, 50.0], [50.0, 40.0, 9000.0]], [(True,) * 3, (True, True, False), (True, True, True)]
    phot = {"ch1": {0: {(k, k): (c, tuple(i), k + 1) for k, (i, c) in enumerate(zip(I, C))}}}
    signals, total, none_count, info = LN.photometries_lognormal_fit(phot, 10000.0, 0.2, 3, allow_upsteps=True,
                                                                    quench_factors=(0.0,) + (0.3,) * 4, solver='dp')
    assert total == 3 and none_count == 2 and list(signals.values()) == [1]
    assert info[0][7] is None and info[0][9] == (1, 3, 1) and info[0][13] == 1          # the winner steps up: no signal, its sequence kept
    assert info[1][7] == (('A', 2),) and info[2][9] is None


def test_chain_records_with_the_twin_needs_no_budget():
    """solver='dp' with budget=1 gives what solver='enumerate' gives with the default budget, where enumerate with budget=1
    raises."""
    from fluorosequencingimageanalysis_amd import lognormal as LN
    rows, cats, fields = table(91, 70, 6, [20, 30, 20])
    exp = LN.chain_records(rows, cats, fields, 0.2, host=True, budget=1 << 22)
    with pytest.raises(NotImplementedError, match="budget"):
        LN.chain_records(rows, cats, fields, 0.2, host=True, budget=1)
    got = LN.chain_records(rows, cats, fields, 0.2, host=True, solver='dp', budget=1)
    same_chain(got, exp, "dp")
    assert got["signals"] == exp["signals"] and list(got["signals"]) == list(exp["signals"])
    assert (got["total_count"], got["none_count"]) == (exp["total_count"], exp["none_count"])
    assert (exp["fit1"]["n_surviving"] > 1).any() and (exp["fit1"]["status"] == 0).any() and (exp["fit1"]["status"] == 1).any()
    got = LN.chain_records(rows, cats, fields, 0.2, host=True, solver='dp', allow_multidrop=False, no_adjustment=True)
    same_chain(got, LN.chain_records(rows, cats, fields, 0.2, host=True, allow_multidrop=False, no_adjustment=True), "dp, no multi-drop")


def test_command_line_solver_dp_writes_the_same_files(tmp_path, capsys, monkeypatch):
    """`--solver dp` on the host route (--device_chain with the twin) and on the default route (its launch stood in for by the
    twin) against the host route's default solver: every file but COMMANDLINE.pkl and the printed text byte for byte."""
    from fluorosequencingimageanalysis_amd import lognormal as LN, lognormal_fitter_v2 as CL
    names = ["CLUSTERED.csv", "COMMANDLINE.pkl", "INTERMEDIATES_v2.pkl", "RAW_PHOTOMETRIES.pkl", "SIGNALS.pkl"]
    path = str(tmp_path / "track_photometries_abc123.csv")
    with open(path, "w") as f:
        f.write(chain_csv_text())
    seen = []

    def records(intensities, categories, means, beta_sigma, max_possible=5, allow_multidrop=True, max_deviation=3, budget=1 << 22,
                lengths=None, device=None, solver='enumerate', allow_upsteps=False):
        seen.append((solver, allow_upsteps))
        return twin_records(D, intensities, categories, means, beta_sigma, max_possible, allow_multidrop, max_deviation, allow_upsteps)
    monkeypatch.setattr(LN, "lognormal_records", records)

    def run(extra, **kw):
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

    _, text0, files0 = run(["--device_chain"], host=True)
    assert seen == [] and sorted(files0) == names and len(files0["INTERMEDIATES_v2.pkl"]) > 100000
    for extra, kw in ((["--device_chain", "--solver", "dp"], dict(host=True)), (["--solver", "dp"], {})):
        _, text1, files1 = run(extra, **kw)
        assert text1 == text0 and sorted(files1) == names
        for name in names:
            if name == "COMMANDLINE.pkl":
                assert pickle.loads(files1[name]) == ["lognormal_fitter_v2.py", path] + extra
            else:
                assert files1[name] == files0[name], (extra, name)
    assert seen == [('dp', False), ('dp', False)]                 # (the default route's two fits went to the dynamic programme)
    args = pickle.loads(files0["INTERMEDIATES_v2.pkl"])[2]
    assert not hasattr(args, "solver") and not hasattr(args, "device_chain")
