"""The sequence-experiment records route without a GPU: the NumPy restatement of the two glue kernels
(tests/_experiment_reference.py) against what the reference recorded (tests/golden/experiment_end_to_end.npz), the writers'
bytes against the reference's texts, the command line's argparse surface and its refusals."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _experiment_cases as C  # noqa: E402
import _experiment_reference as R  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(C.GOLDEN)


def test_golden_inputs_meet_their_conditions(golden):
    g = golden
    assert g["frames"].shape == C.SHAPE and g["frames"].dtype == np.uint16
    assert np.array_equal(g["frames"], C.experiment_frames(int(g["seed"])))         # the package's own generator, reproducible
    H, W = C.SHAPE[3:]
    hw = g["two_spot_hw"]
    assert ((hw[:, 0] == H - 2) | (hw[:, 1] == W - 2)).any()
    assert g["two_n_dropouts"].sum() > 0
    det = g["two_traces_hw"][:, :, 0] >= 0
    assert (~det[:, 0]).any() and (~det[:, -1]).any() and (det[:, :-2] & ~det[:, 1:-1] & det[:, 2:]).any()
    for c in range(2):
        assert (g["two_invalid_seq"] % 2 == c).any() and (det.all(axis=1) & (g["two_traces_seq"] % 2 == c)).any()


@pytest.mark.parametrize("record_bytes", [378, 428])
def test_spot_table_restatement_equals_reference(golden, record_bytes):
    """Records made of the reference's own keys and fitted centres -> its Spot tables and discard counts, per frame, in the order
    of its dicts; the crafted dict takes Spot.__init__ through every outcome."""
    g = golden
    H, W = C.SHAPE[3:]
    rec = C.records_from(g["psf_key"], g["psf_centre"], record_bytes)
    got = R.spot_table(rec, g["psf_counts"].reshape(-1), H, W)
    assert np.array_equal(got["hw"], g["two_spot_hw"])
    assert np.array_equal(got["counts"].reshape(g["two_spot_counts"].shape), g["two_spot_counts"])
    assert np.array_equal(got["discarded"].reshape(g["two_spots_discarded"].shape), g["two_spots_discarded"])
    assert not got["status"].any()
    # the first channel alone: every other sequence
    F = C.SHAPE[2]
    one = np.concatenate([np.arange(s * F, (s + 1) * F) for s in range(0, g["psf_counts"].shape[0], 2)])
    starts = np.concatenate([[0], np.cumsum(got["counts"])])
    assert np.array_equal(np.concatenate([got["hw"][starts[k]:starts[k + 1]] for k in one]), g["one_spot_hw"])
    crafted = R.spot_table(C.records_from(g["crafted_key"], g["crafted_centre"], record_bytes), [len(g["crafted_key"])], H, W)
    assert np.array_equal(crafted["hw"], g["crafted_spot_hw"])
    assert int(crafted["discarded"][0]) == int(g["crafted_discarded"]) > 0


@pytest.mark.parametrize("run", ["two", "one", "alt"])
def test_trace_rows_restatement_equals_reference(golden, run):
    """The reference's traces as spot numbers (what the tracker leaves) -> its rows of (h, w), sequence after sequence."""
    g = golden
    traces, n_traces, field_start = C.tracker_output_from(g, run)
    F = C.SHAPE[2]
    got = R.trace_rows(traces, n_traces, field_start, g[run + "_spot_hw"], F)
    assert np.array_equal(got["trace_hw"], g[run + "_traces_hw"])
    assert np.array_equal(got["trace_seq"], g[run + "_traces_seq"])
    hw = g[run + "_spot_hw"]
    have = got["trace_spot"] >= 0
    assert np.array_equal(hw[got["trace_spot"][have]], got["trace_hw"][have])


def test_restatement_on_synthetic_tables():
    """Failed frames, both record sizes and guarded tables, on the host alone."""
    rng = np.random.default_rng(3)
    peaks = [7, -1, 9, -1, -1, 64, 0, -1, 5]
    rec = C.record_table(rng, peaks, 37, 53, 428)
    got = R.spot_table(rec, peaks, 37, 53)
    assert got["status"].tolist() == [0, 1, 0, 1, 1, 0, 0, 1, 0]
    assert (got["counts"] + got["discarded"]).tolist() == [max(p, 0) for p in peaks]
    assert got["spot_record"].tolist() == sorted(got["spot_record"].tolist()) and len(set(got["spot_record"].tolist())) == len(got["hw"])
    h_0, w_0, key_h, key_w = R.record_fields(rec)
    assert np.array_equal(got["hw"], np.stack([key_h, key_w], axis=1)[got["spot_record"]])
    assert R.spot_accepted(1, 30, 2.2, 30.1, 96, 96) and not R.spot_accepted(0, 50, 0.4, 50.2, 96, 96)
    assert R.spot_accepted(40, 95, 40.3, 200.0, 96, 96)             # the precedence: off the right edge passes


@pytest.mark.parametrize("run", ["two", "one", "alt"])
def test_writers_equal_reference_texts(golden, run, tmp_path):
    """write_category_counts_csv / write_track_photometries_csv / summary_text on records assembled from the golden (the
    reference's traces, the filled-in positions and photometries of the restatement of fsq_sequence_photometry) == the
    reference's bytes."""
    from fluorosequencingimageanalysis_amd import experiment as E
    rec, save_averages, collate = C.records_from_golden(golden, run)
    texts = C.records_texts(E, rec, str(tmp_path), save_averages, collate)
    g = golden
    assert texts["counts_csv"] == bytes(g[run + "_csv_counts"])
    assert texts["photometries_csv"] == bytes(g[run + "_csv_photometries"]), texts["photometries_csv"].decode()[:800]
    assert texts["summary"].encode() == bytes(g[run + "_summary"]), texts["summary"]
    for key, filtered in (("category_stats", False), ("filtered_stats", True)):
        assert C.stats_rows(E.category_stats(rec, filtered=filtered)) == C.golden_stats_rows(g, run + "_" + key), key


# ---- the command line ----

def _parser():
    import datetime
    from fluorosequencingimageanalysis_amd import basic_experiment_script as S
    return S, S.build_parser(datetime.datetime(2016, 6, 3))


def test_command_line_surface():
    """The reference's options (basic_experiment_script.py:70-219): names, short forms, defaults, nargs."""
    S, p = _parser()
    a = p.parse_args(["--peptide_files", "a/x.png", "b/x.png"])
    assert a.peptide_files == ["a/x.png", "b/x.png"] and a.alignment_files is None and a.second_channel is None
    assert a.output_directory is None and a.photometry_parameters == [None] and a.save_photometries is True
    assert a.extraction_number == 10 and a.extraction_size == 9 and isinstance(a.num_processes, list) and a.num_processes[0] >= 1
    for flag in ("debug", "recompute", "keep_invalid", "pkl_invalid", "no_self_align", "no_sanity_check_images", "save_tracks",
                 "sextractor", "not_all_photometries", "collate_fields", "all_categories"):
        assert getattr(a, flag) is False, flag
    assert a.log_path == ["/home/basic_experiment_script_2016-06-03 00:00:00.log"]
    b = p.parse_args(["-D", "-n", "3", "-L", "x.log", "--output_directory", "out", "-r", "-ns", "-en", "4", "-es", "7",
                      "--photometry_parameters", "{'radius': 5}", "--alignment_files", "p", "q", "--peptide_files", "r",
                      "--second_channel", "s", "t"])
    assert (b.debug, b.num_processes, b.log_path, b.output_directory, b.recompute, b.no_self_align) == (True, [3], ["x.log"], ["out"], True, True)
    assert (b.extraction_number, b.extraction_size, b.photometry_parameters) == (4, 7, ["{'radius': 5}"])
    assert (b.alignment_files, b.peptide_files, b.second_channel) == (["p", "q"], ["r"], ["s", "t"])
    with pytest.raises(SystemExit):
        p.parse_args([])                                            # --peptide_files is required
    names = set(o for action in p._actions for o in action.option_strings)
    assert names == {"-h", "--help", "-D", "--debug", "-n", "--num_processes", "-L", "--log_path", "--output_directory", "-r",
                     "--recompute", "--keep_invalid", "--pkl_invalid", "-ns", "--no_self_align", "--no_sanity_check_images", "-en",
                     "--extraction_number", "-es", "--extraction_size", "--save_tracks", "--sextractor", "--photometry_parameters",
                     "--save_photometries", "--not_all_photometries", "--collate_fields", "--all_categories", "--alignment_files",
                     "--peptide_files", "--second_channel"}


@pytest.mark.parametrize("extra", [["--recompute"], ["--all_categories"], ["--save_tracks"], ["--pkl_invalid"], ["--sextractor"], []])
def test_command_line_refusals(extra, tmp_path, monkeypatch):
    """NotImplementedError before any work is done: nothing is read, fitted, logged or written (a run without
    --no_sanity_check_images among them)."""
    S, _ = _parser()
    monkeypatch.setattr(S.pflib, "parallel_image_batch", lambda **kw: pytest.fail("work was started"))
    monkeypatch.setattr(S.logging, "basicConfig", lambda **kw: pytest.fail("the log was opened"))
    argv = ["--peptide_files", str(tmp_path / "missing.png"), "--output_directory", str(tmp_path / "out"), "-L", str(tmp_path / "log")]
    if extra:
        argv += ["--no_sanity_check_images"] + extra
    with pytest.raises(NotImplementedError):
        S.main(argv)
    assert not os.path.exists(str(tmp_path / "out")) and not os.path.exists(str(tmp_path / "log"))
