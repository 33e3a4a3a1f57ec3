"""The simulation parameter sweep without a GPU: the NumPy twin of fsq_signal_scores against the reference's recorded
signal_correlation (tests/golden/signal_sweep.npz), the 64-bit signal key, the host sweep against the single-point host route,
and the command line."""
import itertools
import os
import pickle
import re

import numpy as np
import pytest

from fluorosequencingimageanalysis_amd import _host_signal_sweep as H
from fluorosequencingimageanalysis_amd import _native_signal_sweep as NS
from fluorosequencingimageanalysis_amd import _tracks, lognormal, peptide_simulator, signal_sweep as SW, simulate_peptide, sweep_peptide
from _signal_sweep_cases import case, case_names, check_against_golden, outcome, runs

DDIF = [0, 0.3] + [0.3] * 5
FIXED = dict(s=0.1, sc=3, s2=0.05, beta=70000.0, beta_sigma=0.2, ddif=DDIF)
POINTS = [(0.9, 0.05, 0.1), (0.7, 0.2, 0.4), (0.95, 0.1, 0.25)]


def test_binding_declares_the_header():
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "fsq_signal_sweep.h")).read()
    assert set(re.findall(r"^int (fsq_\w+)\(", text, re.M)) == set(NS.EXPORTED)
    for name in ("MAX_DROPS", "MAX_FRAMES", "EMPTY", "NEVER", "MAX_SLOTS"):
        value = re.search(r"#define FSQ_SIGNAL_%s (\(1 << 24\)|\w+)" % name, text).group(1)
        assert getattr(NS, name) == (1 << 24 if value.startswith("(") else int(value.rstrip("ul"), 0)), name
    for i, metric in enumerate(NS.METRICS):
        assert re.search(r"#define FSQ_SCORE_%s %d\n" % (metric.upper(), i), text), metric
    assert NS.METRICS == H.METRICS and (NS.EMPTY, NS.NEVER, NS.MAX_DROPS) == (H.EMPTY, H.NEVER, H.MAX_DROPS)


@pytest.mark.parametrize("name", case_names())
def test_twin_against_the_reference(name):
    observed, fit, opts = case(name)
    n = 0
    for metric, nc, hn, status, result, factor, contrib in runs(name):
        got = outcome(lambda: SW.signal_correlation(observed, fit, metric=metric, normalize_counts=nc, heatmap_normalize_counts=hn,
                                                    host=True, **opts))
        check_against_golden((name, metric, nc, hn), metric, got, (status, result, factor, contrib))
        n += 1
    assert n == 30


def test_golden_holds_every_outcome():
    from _signal_sweep_cases import golden
    assert set(np.unique(golden()["status"]).tolist()) == {H.SCORE_OK, H.SCORE_EMPTY, H.SCORE_DIVZERO, H.SCORE_DOMAIN}


def test_twin_does_not_depend_on_dict_order():
    observed, fit, opts = case("hand_wide")
    a = SW.signal_correlation(observed, fit, metric='my_euclidean', normalize_counts=True, host=True, **opts)
    b = SW.signal_correlation(dict(reversed(list(observed.items()))), dict(reversed(list(fit.items()))), metric='my_euclidean',
                              normalize_counts=True, host=True, **opts)
    assert a == b


def _reference_signal(row):
    return _tracks.decrements_of_row(row), row[-1] == 0, row[0]


def test_key_round_trips_every_row_shape():
    """Every non-increasing row of 4 frames that starts at up to 10 dyes (0 .. 10 drops, single and multiple), and the
    extremes: 64 frames, cycle 63, 15 dyes, 10 drops."""
    rows = [r for r in itertools.product(range(11), repeat=4) if all(a >= b for a, b in zip(r, r[1:]))]
    rows += [(15,) * 63 + (5,), (15,) + (5,) * 63, tuple(range(15, 5, -1)) + (5,) * 54, (10,) * 32 + (0,) * 32, (0,) * 64, (7,), (0,)]
    assert {r[0] - r[-1] for r in rows} == set(range(11))
    seen = {}
    for row in rows:
        what, key = H.classify_row(row)
        assert what == H.ROW_SIGNAL and 0 <= key < 1 << 64 and key not in (H.EMPTY, H.NEVER)
        signal = H.signal_of_key(key)
        assert signal == _reference_signal(list(row)) == lognormal.signal_of(tuple(row)), row
        assert H.key_of_signal(signal) == key
        assert seen.setdefault(key, signal) == signal               # (rows of different lengths share a key only with the signal)
    for marker in (H.EMPTY, H.NEVER):
        with pytest.raises(ValueError):
            H.signal_of_key(marker)


def test_rows_without_a_key_or_a_signal():
    assert H.classify_row([11] + [0] * 3) == (H.ROW_UNKEYED, None)                      # 11 drops
    assert H.classify_row(list(range(11, -1, -1))) == (H.ROW_UNKEYED, None)
    assert H.classify_row([16, 16]) == (H.ROW_UNKEYED, None)                            # a start beyond 4 bits
    assert H.classify_row([2, 1, 2, 0]) == (H.ROW_NONE, None)                           # an upstep
    assert H.classify_row([12, 0, 1]) == (H.ROW_NONE, None)                             # an upstep wins over too many drops
    assert lognormal.signal_of((2, 1, 2, 0))[0] is None
    tables, none, unkeyed = H.tally_rows([[2, 1, 0], [2, 1, 0], [11, 0, 0], [1, 2, 2], [3, 3, 3], [2, 1, 0]], [0, 1, 1, 1, 5, 0],
                                         [1, 1, 1, 1, 1, 0], 2)
    assert tables == [{H.key_of(2, [1, 2]): 1}, {H.key_of(2, [1, 2]): 1}] and none == [0, 1] and unkeyed == [0, 1]
    for signal in [((('B', 1),), True, 1), ((('A', 2), ('A', 1)), True, 2), ((('A', 1),), False, 1), ((('A', 1),), True, 2),
                   ((('A', 64),), True, 1), (H.NO_DROPS, True, 16), ((('A', 1),) * 11, False, 12)]:
        assert H.key_of_signal(signal) is None, signal


@pytest.mark.parametrize("stride", [0, 1000])
def test_host_sweep_is_the_single_point_host_route(stride):
    n, seed, first = 150, 11, 40
    sweep = SW.sweep_records('GAKAGAKC', 'K', 2, 4, POINTS, n, seed=seed, first_molecule=first, molecule_stride=stride, host=True,
                             quench_factors=DDIF, **FIXED)
    assert sweep["points"] == POINTS and list(sweep["all_simulations"]) == POINTS
    for k, (p, b, u) in enumerate(POINTS):
        records = peptide_simulator.simulation_records('GAKAGAKC', 'K', 2, 4, n, seed, first + k * stride, host=True, p=p, b=b, u=u, **FIXED)
        photometries, kept = simulate_peptide.photometries_of_records(records)
        mes = simulate_peptide.molecular_error_signals_of_records(records, kept)
        signals, total, none_count = simulate_peptide.host_fit(photometries, FIXED["beta"], FIXED["beta_sigma"], 5, True, 3, DDIF)
        assert sweep["all_simulations"][(p, b, u)] == (signals, mes)
        assert (sweep["total_count"][(p, b, u)], sweep["none_count"][(p, b, u)]) == (total, none_count)
        assert total > 100 and len(signals) > 5


def test_unsupported_metrics_raise_with_their_name():
    observed, fit, opts = case("hand_wide")
    for metric in H.OTHER_METRICS:
        with pytest.raises(NotImplementedError, match=metric):
            SW.signal_correlation(observed, fit, metric=metric, host=True, **opts)
    with pytest.raises(ValueError, match="Invalid metric"):
        SW.signal_correlation(observed, fit, metric='nonsense', host=True)
    assert set(H.METRICS).isdisjoint(H.OTHER_METRICS) and len(H.METRICS) == 10


def test_best_point_and_its_tie_rule():
    scores = {"a": (None, (1.0, {})), "b": (2.0, (1.0, {})), "c": (1.0, (0.5, {"x": 1.0})), "d": (1.0, (1.0, {})), "e": (2.0, (1.0, {}))}
    assert SW.best_point(scores) == ("c", 1.0, 0.5, {"x": 1.0})
    assert SW.best_point(scores, reverse_order=True)[0] == "b"
    with pytest.raises(ValueError):
        SW.best_point({"a": (None, (1.0, {}))})


def test_host_scores_pick_the_point_the_observed_signals_came_from():
    sweep = SW.sweep_records('GAKAGAKC', 'K', 2, 4, POINTS, 120, seed=3, host=True, quench_factors=DDIF, **FIXED)
    observed = sweep["all_simulations"][POINTS[1]][0]
    scores = SW.score_records(observed, sweep, metric='my_euclidean', heatmap_only=False, zero_only=False, allow_multidrop=True, host=True)
    assert list(scores) == POINTS
    point, result, factor, contrib = SW.best_point(scores)
    assert point == POINTS[1] and result == 0.0 and factor == 1.0 and set(contrib) == set(observed)


def test_command_line_arguments():
    assert sweep_peptide.value_range("0.5") == [0.5]
    assert sweep_peptide.value_range("0.8:0.9:3") == np.linspace(0.8, 0.9, 3).tolist() and sweep_peptide.value_range("0:1:5") == [0.0, 0.25, 0.5, 0.75, 1.0]
    assert sweep_peptide.value_range("0.1:0.1:1") == [0.1]
    parser = sweep_peptide.build_parser()
    for bad in ("0.1:0.2", "0.1:0.2:0", "0.1:0.2:1", "a:b:3"):
        with pytest.raises(SystemExit):
            parser.parse_args(["GAKC", "K", "--observed", "x.pkl", "--dud_dyes", bad])
    with pytest.raises(SystemExit):
        parser.parse_args(["GAKC", "K"])                                                 # --observed is required
    with pytest.raises(SystemExit):
        parser.parse_args(["GAKC", "K", "--observed", "x.pkl", "--normalize_counts", "--heatmap_normalize_counts"])
    with pytest.raises(SystemExit):
        parser.parse_args(["GAKC", "K", "--observed", "x.pkl", "--metric", "my_pearson"])
    args = parser.parse_args(["GAKC", "K", "--observed", "x.pkl"])
    theirs = simulate_peptide.build_parser().parse_args(["GAKC", "K"])
    for name in ("num_sims", "num_mocks", "num_mocks_omitted", "num_edmans", "surface_degradation_1", "surface_degradation_1_num_cycles",
                 "surface_degradation_2", "fluor_intensity", "ddif_2", "ddif_3", "beta_sigma", "no_multidrop", "superdye_rate",
                 "superdye_factor"):
        assert getattr(args, name) == getattr(theirs, name), name
    assert (args.edman_efficiency, args.dye_destruction, args.dud_dyes) == ([theirs.edman_efficiency], [theirs.dye_destruction], [theirs.dud_dyes])
    assert args.metric == 'my_euclidean' and not args.host and args.table_slots == 1024 and args.molecule_stride == 0


def test_command_line_on_the_host(tmp_path, capsys):
    """A 2 x 1 x 2 grid against the signals simulate_peptide's own run writes for one of its points."""
    common = ["GAKAGAKC", "K", "-N", "80", "-m", "3", "-e", "4", "--seed", "5", "--host", "--output_directory", str(tmp_path)]
    single = simulate_peptide.main(common + ["--edman_efficiency", "0.8", "--dud_dyes", "0.3", "--no_csv"])
    path = sweep_peptide.main(common + ["--observed", single, "--edman_efficiency", "0.8:0.95:2", "--dud_dyes", "0.1:0.3:2",
                                        "--all_signals", "--nonzero_signals", "--score_multidrop"])
    assert os.path.basename(path).startswith("Sweep_") and path.endswith(".pkl")
    with open(path, "rb") as f:
        out = pickle.load(f)
    with open(single, "rb") as f:
        _, signals, mes = pickle.load(f)
    assert out["points"] == [(0.8, 0.1, 0.1), (0.8, 0.1, 0.3), (0.95, 0.1, 0.1), (0.95, 0.1, 0.3)] == list(out["scores"])
    assert out["all_simulations"][(0.8, 0.1, 0.3)] == (signals, mes)
    assert out["best_point"][:3] == ((0.8, 0.1, 0.3), 0.0, 1.0)
    assert "Best point (edman_efficiency, dye_destruction, dud_dyes): (0.8, 0.1, 0.3)" in capsys.readouterr().out
