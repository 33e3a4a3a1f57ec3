"""match_diagnostic's incompatibility loop on the host (no GPU): the NumPy twin of fsq_signal_pair_best and
fsq_signal_pair_extremes bit for bit against the reference's recorded loop and against scores() called once per pair, the
heat-map tables, Python 2's rounding, match_diagnostic end to end and the command line."""
import itertools
import os
import pickle
import re

import numpy as np
import pytest

from fluorosequencingimageanalysis_amd import _host_signal_sweep as H
from fluorosequencingimageanalysis_amd import _native_signal_sweep as NS
from fluorosequencingimageanalysis_amd import signal_sweep as SW, simulate_peptide, sweep_peptide
from _incompatibility_cases import assert_same_outputs, case, case_names, golden, host_inputs, runs, same_bits, synthetic

DDIF = [0, 0.3] + [0.3] * 5
FIXED = dict(s=0.1, sc=3, s2=0.05, beta=70000.0, beta_sigma=0.2, ddif=DDIF)
GRID = [(p, b, u) for p in (0.8, 0.95) for b in (0.05, 0.15) for u in (0.1, 0.4)]


def sig(start, *cycles):
    return H.signal_of_key(H.key_of(start, cycles))


def test_binding_and_header_name_the_new_entries():
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "fsq_signal_sweep.h")).read()
    assert {"fsq_signal_pair_best", "fsq_signal_pair_extremes"} <= set(NS.EXPORTED) & set(re.findall(r"^int (fsq_\w+)\(", text, re.M))
    assert int(re.search(r"#define FSQ_SIGNAL_PAIR_MAX_SEL (\d+)", text).group(1)) == NS.MAX_SEL == H.MAX_SEL >= 2016


# ---- the twin against the reference's loop ----

@pytest.mark.parametrize("name", case_names())
def test_twin_is_the_reference_loop_bit_for_bit(name):
    observed, sweep, candidates, cutoff = case(name)
    n = 0
    for metric, nc, hn, reverse, best, factor, dist, is_none in runs(name):
        table, rows, fit, fit_total = host_inputs(observed, sweep, candidates)
        got = H.pair_best(table, rows, fit, fit_total, metric, H.normalization_of(nc, hn), cutoff, reverse)
        what = (name, metric, nc, hn, reverse)
        assert np.array_equal(got["best_point"], best), what
        assert np.array_equal(np.isnan(got["dist"]), is_none), what
        assert same_bits(got["dist"], dist) and same_bits(got["factor"], factor), what
        assert (got["error_point"] == -1).all() and (got["error_status"] == 0).all(), what
        n += 1
    assert n == 40


def test_golden_holds_every_situation():
    g = golden()
    a, cut = g["cycles4_best_point"], g["cycles4_cutoff_best_point"]
    candidates = case("cycles4")[2]
    nothing = H.pair_index(candidates.index(sig(2, 1, 2)), candidates.index(sig(2, 1, 3)), len(candidates))
    assert (a[..., nothing] == -1).all() and (np.delete(a, nothing, axis=-1) >= 0).all()         # the pair in which nothing pairs
    assert not (a == 6).any() and (a == 0).any()                                                 # point 6 is point 0 again
    assert (cut == -1).sum() > (a == -1).sum()                                                   # the cutoff takes members out
    for name in ("cycles5_fit_only", "cycles5_observed_zero"):
        assert g[name + "_dist_is_none"].any() and not g[name + "_dist_is_none"].all()
    assert case("cycles5_observed_zero")[0][sig(1, 5)] == 0
    assert sig(1, 5) not in case("cycles5_fit_only")[0]
    observed, sweep, candidates, _ = case("cycles4")
    assert sig(1, 1) in observed and all(sig(1, 1) not in sweep["all_simulations"][k][0] for k in sweep["points"])


def test_records_give_the_reference_shapes_on_the_golden():
    observed, sweep, candidates, cutoff = case("cycles4")
    for metric, nc, hn, reverse, best, factor, dist, is_none in itertools.islice(runs("cycles4"), 0, 40, 7):
        rec = SW.incompatibility_records(observed, sweep, num_cycles=4, metric=metric, normalize_counts=nc, heatmap_normalize_counts=hn,
                                         reverse_order=reverse, host=True)
        assert list(rec["pairs"]) == list(itertools.combinations(candidates, 2))
        for t, value in enumerate(rec["pairs"].values()):
            if best[t] < 0:
                assert value == (None, (None, None), None)
                continue
            point, d, nf = value
            assert point == best[t] and same_bits(nf, factor[t])
            assert [x is None for x in d] == is_none[t].tolist()
            assert all(x is None or same_bits(x, dist[t][i]) for i, x in enumerate(d))
        lists = {}
        for (ss1, ss2), (_, (d1, d2), _) in rec["pairs"].items():                                 # :875-889, None skipped
            lists.setdefault(ss1, []).append(d1)
            lists.setdefault(ss2, []).append(d2)
        want = {s: (min if reverse else max)(x for x in v if x is not None) for s, v in lists.items() if any(x is not None for x in v)}
        assert rec["scores"] == want and len(want) < len(candidates)
        assert SW.incompatibility_records(observed, sweep, num_cycles=4, metric=metric, normalize_counts=nc, heatmap_normalize_counts=hn,
                                          reverse_order=reverse, host=True, pairs=False) == {"pairs": None, "scores": want}


# ---- the twin against its definition ----

def _by_definition(table, rows, fit, fit_total, metric, norm, cutoff, reverse):
    """scores() once per pair with the admitted mask ANDed with the pair, then best_point's rule."""
    n_sel, P = len(rows), len(fit_total)
    K = n_sel * (n_sel - 1) // 2
    out = {"best_point": np.full(K, -1, np.int32), "result": np.full(K, np.nan), "factor": np.full(K, np.nan),
           "dist": np.full((K, 2), np.nan), "error_point": np.full(K, -1, np.int32), "error_status": np.zeros(K, np.int32)}
    for t, (i, j) in enumerate(itertools.combinations(range(n_sel), 2)):
        mask = np.zeros_like(table["admitted"])
        for r in (rows[i], rows[j]):
            if r >= 0:
                mask[r] = table["admitted"][r]
        score, factor, status, contrib = H.scores(dict(table, admitted=mask), fit, fit_total, metric, norm, cutoff)
        bad = np.flatnonzero(status >= H.SCORE_DIVZERO)
        if len(bad):
            out["error_point"][t], out["error_status"][t] = bad[0], status[bad[0]]
        ok = np.flatnonzero(status == H.SCORE_OK)
        if len(ok):
            k = ok[np.argmax(score[ok]) if reverse else np.argmin(score[ok])]                    # (the first among equal ones)
            out["best_point"][t], out["result"][t], out["factor"][t] = k, score[k], factor[k]
            out["dist"][t] = [contrib[r, k] if r >= 0 else np.nan for r in (rows[i], rows[j])]
    return out


@pytest.mark.parametrize("norm, cutoff", [(1, None), (2, None), (0, None), (3, 3.0), (2, 3.0)])
def test_twin_is_scores_once_per_pair(norm, cutoff):
    observed, sweep, candidates, _ = case("cycles4")
    table, rows, fit, fit_total = host_inputs(observed, sweep, candidates)
    for metric in H.METRICS:
        for reverse in (False, True):
            got = H.pair_best(table, rows, fit, fit_total, metric, norm, cutoff, reverse)
            assert_same_outputs(got, _by_definition(table, rows, fit, fit_total, metric, norm, cutoff, reverse), (metric, norm, reverse))


def test_twin_is_scores_once_per_pair_with_errors_and_rows_of_minus_one():
    table, fit, fit_total = synthetic(12, 9, 5)
    fit[:, 4] = 0                                                                                 # a heat-map total of zero
    table["n_observed"] = int(table["observed"].max())                                            # a zero variance
    rows = np.array([0, 3, -1, 7, 2, 11, -1, 5], np.int32)
    seen = set()
    for metric in H.METRICS:
        for norm in (0, 1, 2):
            got = H.pair_best(table, rows, fit, fit_total, metric, norm, None, False)
            assert_same_outputs(got, _by_definition(table, rows, fit, fit_total, metric, norm, None, False), (metric, norm))
            seen |= set(got["error_status"].tolist())
    assert seen == {0, H.SCORE_DIVZERO, H.SCORE_DOMAIN}


def test_the_tie_rule_and_points_without_a_result():
    table, fit, fit_total = synthetic(6, 5, 1)
    table["admitted"][:], table["in_observed"][:] = 1, 1
    table["observed"][:2] = (10, 20)
    fit[0], fit[1] = (0, 7, 9, 7, 0), (0, 17, 2, 17, 0)                                          # points 1 and 3 are equal
    fit[5] = 0
    table["in_observed"][5] = 0                                                                   # key 5: in neither dict
    got = H.pair_best(table, [0, 1, 5], fit, fit_total, 'my_euclidean', 0, 1.0, False)            # cutoff 1: points 0 and 4 are EMPTY
    assert got["best_point"].tolist() == [1, 2, 1] and got["result"][0] == np.sqrt(9.0 + 9.0)    # (1, not 3)
    assert np.isnan(got["dist"][1, 1]) and got["dist"][1, 0] == 1.0 and got["dist"][2].tolist()[:1] == [9.0]
    assert H.pair_best(table, [0, 1, 5], fit, fit_total, 'my_euclidean', 0, 1.0, True)["best_point"].tolist() == [2, 1, 2]
    none = H.pair_best(table, [5, -1], fit, fit_total, 'my_euclidean', 0, None, False)
    assert none["best_point"].tolist() == [-1] and np.isnan(none["result"]).all() and np.isnan(none["factor"]).all()
    for bad in ([0], [0, 6], [0, -2]):
        with pytest.raises(ValueError):
            H.pair_best(table, bad, fit, fit_total, 'my_euclidean')


def test_extremes_against_a_restatement():
    rng = np.random.default_rng(8)
    for n_sel in (2, 3, 10, 66):
        dist = rng.random((n_sel * (n_sel - 1) // 2, 2))
        dist[rng.random(dist.shape) < 0.3] = np.nan
        for t, (i, j) in enumerate(itertools.combinations(range(n_sel), 2)):
            if 1 in (i, j):
                dist[t, (i, j).index(1)] = np.nan                                                 # candidate 1 has no distance
        for reverse in (False, True):
            lists = [[] for _ in range(n_sel)]
            for t, (i, j) in enumerate(itertools.combinations(range(n_sel), 2)):
                lists[i].append(dist[t, 0])
                lists[j].append(dist[t, 1])
            kept = [[x for x in v if x == x] for v in lists]
            want = [(min if reverse else max)(v) if v else np.nan for v in kept]
            score, n = H.pair_extremes(dist, n_sel, reverse)
            assert same_bits(score, want) and n.tolist() == [len(v) for v in kept] and np.isnan(score[1]) and n.dtype == np.int32
    with pytest.raises(ValueError):
        H.pair_extremes(np.zeros((4, 2)), 3)


# ---- split_heatmap, the tables, Python 2's rounding ----

def test_split_heatmap():
    before, after = SW.split_heatmap(3, 0)
    assert before == () and after == (sig(1, 1), sig(1, 2), sig(1, 3), sig(2, 1, 2), sig(2, 1, 3), sig(2, 2, 3))
    before, after = SW.split_heatmap(3, 3)
    assert before == (sig(1, 1), sig(1, 2), sig(2, 1, 2)) and after == (sig(1, 3), sig(2, 1, 3), sig(2, 2, 3))
    for n in (4, 5):
        assert [H.key_of_signal(s) for s in SW.split_heatmap(n, 0)[1]] == golden()["cycles%d%s_candidates" % (n, "" if n == 4 else "_fit_only")].tolist()
    assert len(SW.split_heatmap(12, 0)[1]) == 78 and len(SW.split_heatmap(63, 0)[1]) == 2016


def test_python_2_rounding():
    assert int(SW.py2_round(2.5)) == 3 and int(SW.py2_round(-2.5)) == -3 and int(SW.py2_round(3.5)) == 4 and round(2.5) == 2
    assert SW.py2_round(0.49999999999999994) == 0.0 and SW.py2_round(2.4999) == 2.0 and SW.py2_round(-0.2) == 0.0
    assert SW.py2_round2(0.125) == 0.13 and round(0.125, 2) == 0.12 and SW.py2_round2(-0.125) == -0.13
    assert SW.py2_round2(2.675) == 2.67 and SW.py2_round2(0.375) == 0.38 and SW.py2_round2(7) == 7.0       # (2.675 is below the half)


def test_single_drops_table():
    signals = {sig(1, 2): 5, sig(1, 3): 0.125, sig(1): 9, sig(0): 4, sig(2, 1, 2): 8, sig(2, 1): 3, sig(1, 4): 2,
               ((('A', 1),), False, 1): 6}
    table, header = SW.single_drops_table(signals, 3, 2, 1)                                       # 2 imaged mocks + 2 Edmans
    assert header == ["M2", "M3", "E1", "E2", "R"] and table.dtype == np.int64
    assert table.tolist() == [[0, 5, 0, 2, 9]]                                                    # (0.125 truncates in the integer table)
    table, header = SW.single_drops_table(signals, 3, 2, 1, float_data=True)
    assert table.dtype == np.float64 and table.tolist() == [[0.0, 5.0, 0.13, 2.0, 9.0]]
    assert SW.single_drops_table(signals, 3, 2, 1, plot_remainders=False)[0].tolist() == [[0, 5, 0, 2]]
    with pytest.raises(AssertionError):                                                           # the remainder cell written twice
        SW.single_drops_table({sig(1): 9, ((('A', 0),), False, 0): 1}, 3, 2, 1)
    with pytest.raises(IndexError):
        SW.single_drops_table({sig(1, 6): 1}, 3, 2, 1)


def test_double_drops_table():
    signals = {sig(2, 1, 3): 5, sig(2, 2, 2): 7, sig(2, 2): 4, sig(1, 2): 6, sig(2): 9, sig(3, 1, 2, 3): 8, sig(2, 3, 4): 0.375,
               sig(3, 1): 2}
    table, columns, rows = SW.double_drops_table(signals, 3, 2, 1)
    assert rows == ["M2", "M3", "E1", "E2"] and columns == rows + ["R"] and table.shape == (4, 5) and table.dtype == np.int64
    want = np.zeros((4, 5), np.int64)
    want[0, 2], want[1, 4] = 5, 4
    assert np.array_equal(table, want)
    multi = SW.double_drops_table(signals, 3, 2, 1, plot_multidrops=True, float_data=True)[0]
    assert multi[1, 1] == 7.0 and multi[2, 3] == 0.38 and multi[0, 2] == 5.0 and multi.dtype == np.float64
    flat, columns, _ = SW.double_drops_table(signals, 3, 2, 1, plot_remainders=False)
    assert flat.shape == (4, 4) and columns == rows and flat.sum() == 5
    with pytest.raises(AssertionError):                                                           # (starts of 1 and 2 share a remainder cell)
        SW.double_drops_table({sig(2, 2): 4, ((('A', 2),), False, 1): 3}, 3, 2, 1)


# ---- match_diagnostic ----

_sweep = {}


def host_sweep():
    if not _sweep:
        _sweep.update(SW.sweep_records('GAKAGAKC', 'K', 2, 4, GRID, 500, seed=21, first_molecule=3, host=True, quench_factors=DDIF, **FIXED))
    return _sweep


ARGS = dict(metric='my_euclidean', reverse_order=False, normalize_counts=False, heatmap_normalize_counts=True, heatmap_only=True,
            zero_only=True, allow_multidrop=False, small_count_cutoff=None, matching_p=0.10, split_cycle=3,
            incompatibility_threshold=25.0, compute_incompatibility_scores=True, num_mocks=3, num_mocks_omitted=1, num_edmans=4)


def test_match_diagnostic_on_the_host_end_to_end():
    sweep = host_sweep()
    observed = dict(sweep["all_simulations"][GRID[5]][0])
    observed[sig(1, 2)] = observed.get(sig(1, 2), 0) + 40                                          # one signal the fits cannot explain
    d = SW.match_diagnostic(sweep, observed, host=True, **ARGS)
    scores = SW.score_records(observed, sweep, metric='my_euclidean', heatmap_normalize_counts=True, host=True)
    point, result, factor, contrib = SW.best_point(scores)
    assert (d["optimal_pbu"], d["result"], d["normalization_factor"], d["optimal_contributions"]) == (point, result, factor, contrib)
    assert d["num_cycles"] == 6 and set(d["incompatibility_scores"]) <= set(SW.split_heatmap(6, 0)[1])
    rec = SW.incompatibility_records(observed, sweep, num_cycles=6, metric='my_euclidean', heatmap_normalize_counts=True, host=True)
    assert d["incompatibility_scores"] == rec["scores"] and len(rec["pairs"]) == 21 * 20 // 2
    above = {s for s, v in rec["scores"].items() if v > 25.0}
    assert sig(1, 2) in above and len(above) < len(rec["scores"])
    assert d["exclude_signals"] == above | set(SW.split_heatmap(6, 3)[0])
    fits, molecular = sweep["all_simulations"][point]
    assert d["normalized_plot_signals"] == {s: int(SW.py2_round(n * factor)) for s, n in fits.items()}
    assert d["normalized_plot_molecular_signals"] == {s: int(SW.py2_round(n * factor)) for s, n in molecular.items()}
    assert d["diff_plot_signals"] == {s: float(n - d["normalized_plot_signals"][s]) / n for s, n in observed.items()
                                      if s in fits and n > 0}
    assert set(d["tables"]) == set(SW.TABLE_NAMES) and len(SW.TABLE_NAMES) == 12
    assert d["tables"]["single_observed"].shape == (1, 7) and d["tables"]["double_fit"].shape == (6, 7)
    assert d["tables"]["single_observed"][0, 1] == observed[sig(1, 2)]
    assert d["tables"]["single_incompatibility"][0, 1] == SW.py2_round2(rec["scores"][sig(1, 2)])
    assert d["tables"]["double_contributions"][0, 4] == SW.py2_round2(contrib[sig(2, 1, 5)])
    assert d["z_ranges"]["single_drop"][0] == 0 and d["z_ranges"]["incompatibility"][1] == max(list(rec["scores"].values()) + list(contrib.values()))
    assert d["headers"]["single"] == ["M2", "M3", "E1", "E2", "E3", "E4", "R"]
    assert SW.reference_tuple(d) == (d["normalized_plot_signals"], contrib, rec["scores"])
    # the reference's {point: (signals, molecular_signals)} is taken as well; the exclusion changes the fit only when asked to
    plain = SW.match_diagnostic(sweep["all_simulations"], observed, host=True, **ARGS)
    assert plain["optimal_pbu"] == point and plain["incompatibility_scores"] == rec["scores"]
    applied = SW.match_diagnostic(sweep, observed, host=True, apply_exclusion=True, **ARGS)
    assert not set(applied["optimal_contributions"]) & applied["exclude_signals"] and applied["result"] < d["result"]
    off = SW.match_diagnostic(sweep, observed, host=True, **dict(ARGS, compute_incompatibility_scores=False, incompatibility_threshold=None))
    assert off["incompatibility_scores"] == {} and off["exclude_signals"] == set(SW.split_heatmap(6, 3)[0])
    assert SW.match_diagnostic(sweep, observed, host=True, num_cycles=4, **ARGS)["incompatibility_scores"].keys() <= set(SW.split_heatmap(4, 0)[1])


def test_match_diagnostic_raises_the_three_value_errors():
    sweep, observed = host_sweep(), host_sweep()["all_simulations"][GRID[0]][0]
    for bad, text in ((dict(normalize_counts=True), "normalize_counts == heatmap_normalize_counts"),
                      (dict(heatmap_normalize_counts=False), "normalize_counts == heatmap_normalize_counts"),
                      (dict(heatmap_normalize_counts=False, normalize_counts=True), "If heatmap_only"),
                      (dict(allow_multidrop=True), "If heatmap_only"),
                      (dict(compute_incompatibility_scores=False), "If incompatibility_threshold is not None")):
        with pytest.raises(ValueError, match=text):
            SW.match_diagnostic(sweep, observed, host=True, **dict(ARGS, **bad))


def test_errors_name_the_pair_and_the_point_or_count_as_no_result():
    sweep = host_sweep()
    observed = sweep["all_simulations"][GRID[0]][0]
    broken = {"points": sweep["points"], "all_simulations": dict(sweep["all_simulations"])}
    broken["all_simulations"][GRID[2]] = ({sig(3, 1, 2, 3): 5}, {})                               # a heat-map total of zero
    kw = dict(num_cycles=3, metric='my_euclidean', heatmap_normalize_counts=True, host=True)
    with pytest.raises(ZeroDivisionError, match=re.escape(repr(GRID[2]))) as e:
        SW.incompatibility_records(observed, broken, **kw)
    assert repr(sig(1, 1)) in str(e.value)
    with pytest.raises(ZeroDivisionError):
        SW.score_records(observed, broken, metric='my_euclidean', heatmap_normalize_counts=True, host=True)
    rec = SW.incompatibility_records(observed, broken, on_error='none', **kw)
    assert all(point != GRID[2] for point, _, _ in rec["pairs"].values()) and len(rec["scores"]) > 0
    for metric in H.OTHER_METRICS:
        with pytest.raises(NotImplementedError, match=metric):
            SW.incompatibility_records(observed, sweep, num_cycles=3, metric=metric, host=True)
    with pytest.raises(ValueError):
        SW.incompatibility_records(observed, sweep, select_signals=[sig(1, 1), sig(1, 1)], host=True)
    with pytest.raises(ValueError):
        SW.incompatibility_records(observed, sweep, on_error='skip', num_cycles=3, host=True)


def test_command_line_on_the_host_with_incompatibility(tmp_path, capsys):
    common = ["GAKAGAKC", "K", "-N", "80", "-m", "3", "-e", "4", "--seed", "5", "--host", "--output_directory", str(tmp_path)]
    single = simulate_peptide.main(common + ["--edman_efficiency", "0.8", "--dud_dyes", "0.3", "--no_csv"])
    path = sweep_peptide.main(common + ["--observed", single, "--edman_efficiency", "0.8:0.95:2", "--dud_dyes", "0.1:0.3:2",
                                        "--heatmap_normalize_counts", "--incompatibility", "--incompatibility_threshold", "1.5",
                                        "--split_cycle", "2"])
    with open(path, "rb") as f:
        out = pickle.load(f)
    d = out["diagnostic"]
    assert d["optimal_pbu"] == out["best_point"][0] and d["result"] == out["best_point"][1] and d["num_cycles"] == 6
    observed = sweep_peptide.load_observed(single)
    rec = SW.incompatibility_records(observed, {"points": out["points"], "all_simulations": out["all_simulations"]}, num_cycles=6,
                                     metric='my_euclidean', heatmap_normalize_counts=True, host=True, on_error='none', pairs=False)
    assert d["incompatibility_scores"] == rec["scores"] and len(rec["scores"]) > 5
    assert d["exclude_signals"] == {s for s, v in rec["scores"].items() if v > 1.5} | set(SW.split_heatmap(6, 2)[0])
    printed = capsys.readouterr().out
    assert "Excluded signals: %d" % len(d["exclude_signals"]) in printed
    top = sorted(rec["scores"].values(), reverse=True)[:5]
    assert [float(x) for x in re.findall(r"^  \(.*\): (\S+)$", printed, re.M)] == top
    for bad in ([], ["--normalize_counts"], ["--heatmap_normalize_counts", "--score_multidrop"]):    # refused before the sweep is run
        with pytest.raises(SystemExit):
            sweep_peptide.main(common + ["--observed", single, "--incompatibility"] + bad)
    capsys.readouterr()
    # reverse_order: the largest result is the best, the smallest distance the score
    path = sweep_peptide.main(common + ["--observed", single, "--edman_efficiency", "0.8:0.95:2", "--dud_dyes", "0.3", "--metric", "naive",
                                        "--all_signals", "--normalize_counts", "--reverse_order", "--incompatibility"])
    with open(path, "rb") as f:
        out = pickle.load(f)
    assert out["diagnostic"]["exclude_signals"] == set() and out["diagnostic"]["optimal_pbu"] == out["best_point"][0]
