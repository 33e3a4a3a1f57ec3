"""Sweeps over several label letters on the GPU (include/fsq_signal_sweep.h): fsq_signal_tally_joint against the NumPy twin as
sets of (key, count), fsq_peptide_simulate_labels_points bit for bit against the single-point kernel, and the joint sweep, its
scores and its diagnostics against their host twins.  There is no reference output for joint signals (the reference stops at
one letter): the oracle is the twin and the plain-Python joint_signal, and K = 1 is tied to the one-letter kernels."""
import contextlib
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from fluorosequencingimageanalysis_amd import _host_signal_sweep as H
from _joint_sweep_cases import (DDIF, FIXED2, FIXED3, GRID8, LETTERS, POINTS3, QUENCH, SHAPE2, SHAPE3, hand_rows, host_sweep,
                                observed_of, pad, random_molecules)
from _peptide_labels_cases import golden_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


@contextlib.contextmanager
def _prefilled():
    """Every output tensor a binding allocates starts as a byte pattern, not as zeros: what a kernel leaves unwritten shows."""
    import torch
    real = torch.empty

    def filled(*a, **k):
        t = real(*a, **k)
        if t.is_cuda:
            t.view(torch.uint8).fill_(0xA5)
        return t
    torch.empty = filled
    try:
        yield
    finally:
        torch.empty = real


# ---- the tally ----

def _tally_joint(rows, points, valid, n_points, slots, joint=True):
    """fsq_signal_tally_joint of host arrays [K][n][frames] - with joint=False fsq_signal_tally of [n][frames] -: ([{key: count}]
    of the occupied slots, none, unkeyed, overflow)."""
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    tables = SW.new_tables(n_points, slots, torch.device("cuda"))
    (SW.tally_joint_device if joint else SW.tally_device)(tables, torch.from_numpy(np.ascontiguousarray(rows, np.uint8)).cuda(),
                          torch.from_numpy(np.ascontiguousarray(points, np.int32)).cuda(),
                          None if valid is None else torch.from_numpy(np.ascontiguousarray(valid, np.uint8)).cuda())
    keys, counts = tables["keys"].cpu().numpy().view(np.uint64), tables["counts"].cpu().numpy()
    assert ((keys == H.EMPTY) == (counts == 0)).all()
    got = []
    for k in range(n_points):
        at = np.flatnonzero(keys[k] != H.EMPTY)
        assert len(set(keys[k][at].tolist())) == len(at)                                 # a key sits in one slot
        got.append(dict(zip(keys[k][at].tolist(), counts[k][at].tolist())))
    return got, tables["none"].cpu().tolist(), tables["unkeyed"].cpu().tolist(), tables["overflow"].cpu().tolist()


def _same_as_twin(rows, points, valid, n_points, slots=1024):
    exp, e_none, e_unkeyed = H.tally_joint_rows(rows, points, valid, n_points)
    got, none, unkeyed, overflow = _tally_joint(rows, points, valid, n_points, slots)
    assert got == exp and (none, unkeyed, overflow) == (e_none, e_unkeyed, [0] * n_points)
    return exp, e_none, e_unkeyed


def test_one_channel_is_fsq_signal_tally():
    rng = np.random.default_rng(11)
    rows = random_molecules(rng, 1, 3000, 9, max_start=6)
    rows[0, :40, 0] = 16                                                                 # unkeyed: a start above 15
    rows[0, 40:60] = [12] + [0] * 8                                                      # unkeyed: 12 drops
    points = np.sort(rng.integers(0, 3, 3000)).astype(np.int32)
    valid = (rng.random(3000) < 0.9).astype(np.uint8)
    one = _tally_joint(rows[0], points, valid, 3, 1024, joint=False)
    assert _tally_joint(rows, points, valid, 3, 1024) == one
    assert sum(one[1]) > 0 and sum(one[2]) > 0 and all(len(t) > 100 for t in one[0])
    _same_as_twin(rows, points, valid, 3)


@pytest.mark.parametrize("K", [2, 3, 4])
def test_hand_rows(K):
    cases = hand_rows(K)
    frames = max(len(rows[0]) for rows, _, _ in cases)
    rows = np.array([pad(r, frames) for r, _, _ in cases], np.uint8).transpose(1, 0, 2)      # [K][n][frames]
    n = rows.shape[1]
    exp, none, unkeyed = _same_as_twin(rows, np.zeros(n, np.int32), None, 1)
    kinds = [kind for _, kind, _ in cases]
    assert (none, unkeyed) == ([kinds.count(H.ROW_NONE)], [kinds.count(H.ROW_UNKEYED)])
    want = {}
    for _, kind, sig in cases:
        if kind == H.ROW_SIGNAL:
            want[sig] = want.get(sig, 0) + 1
    assert {H.joint_signal_of_key(LETTERS[K], k): c for k, c in exp[0].items()} == want


@pytest.mark.parametrize("n", [0, 1, 256, 257])
def test_row_counts_around_one_block(n):
    rng = np.random.default_rng(n)
    rows = random_molecules(rng, 2, n, 6, max_start=2)
    points = np.sort(rng.integers(0, 2, n)).astype(np.int32)
    exp, _, _ = _same_as_twin(rows, points, None, 2)
    assert sum(sum(t.values()) for t in exp) <= n and (n < 256 or len(exp[0]) > 10)


@pytest.mark.parametrize("frames", [1, 64])
def test_one_frame_and_sixty_four(frames):
    rng = np.random.default_rng(frames)
    rows = random_molecules(rng, 3, 600, frames, max_start=2, upstep_rate=0.1 if frames > 1 else 0.0)
    if frames == 64:                                                                     # drops at the last cycle, 63
        rows[:, :50, :63] = rows[:, :50, :1]
        rows[:, :50, 63] = 0
        rows[0, 50:60] = 16                                                              # and molecules without a key
    exp, none, unkeyed = _same_as_twin(rows, np.zeros(600, np.int32), None, 1, 4096)
    if frames == 64:
        assert any(((k >> 4) & 63) == 63 for k in exp[0]) and none[0] > 0 and unkeyed[0] > 0
    else:
        assert len(exp[0]) == 27 and (none, unkeyed) == ([0], [0])


def test_six_points_inside_one_block():
    rng = np.random.default_rng(6)
    rows = random_molecules(rng, 2, 256, 5, max_start=2)
    points = (np.arange(256) // 43).astype(np.int32)                                     # 0 .. 5: more than the block's 4 sub-tables
    exp, _, _ = _same_as_twin(rows, points, None, 6)
    assert all(len(t) > 5 for t in exp)
    _same_as_twin(rows, points[::-1].copy(), None, 6)                                    # and in descending order


def test_two_hundred_keys_of_one_point_in_one_block():
    """More distinct keys than a 128-slot LDS sub-table holds: the rest goes to the global table itself."""
    rows = np.zeros((2, 256, 8), np.uint8)
    f = np.arange(8)
    shapes = [(a, b, c) for a in range(1, 8) for c in range(a, 8) for b in range(1, 9)][:200]
    for n, (a, b, c) in enumerate(shapes):
        rows[0, n] = 2 - (f >= a) - (f >= c)                                             # channel 0: two dyes, drops at a <= c
        rows[1, n] = 1 - (f >= b)                                                        # channel 1: one dye, a drop at b or (b = 8) none
    n = len(shapes)
    rows[:, 200:] = rows[:, :56]
    exp, _, _ = _same_as_twin(rows, np.zeros(256, np.int32), None, 1, 256)
    assert n == 200 and len(exp[0]) == 200 and sorted(exp[0].values()) == [1] * 144 + [2] * 56


def test_overflow_sets_the_flag_and_returns():
    rows = np.array([[[1, 0, 0]] * 3, [[1, 1, 0], [1, 0, 0], [1, 1, 1]]], np.uint8)      # three distinct joint signals
    rows = np.tile(rows, (1, 100, 1))
    got, none, unkeyed, overflow = _tally_joint(rows, np.zeros(300, np.int32), None, 1, 2)
    exp, _, _ = H.tally_joint_rows(rows, np.zeros(300, np.int32), None, 1)
    assert overflow == [1] and len(exp[0]) == 3 and len(got[0]) == 2 and all(exp[0][k] == c for k, c in got[0].items())
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    with pytest.raises(ValueError, match="table_slots=2"):
        SW.joint_sweep_device(*SHAPE2, POINTS3, 200, seed=4, table_slots=2, **QUENCH, **FIXED2)


def test_an_empty_mask_and_points_outside_their_range():
    rng = np.random.default_rng(8)
    rows = random_molecules(rng, 2, 500, 5, max_start=2)
    got = _tally_joint(rows, np.zeros(500, np.int32), np.zeros(500, np.uint8), 1, 64)
    assert got == ([{}], [0], [0], [0])
    points = rng.integers(-2, 5, 500).astype(np.int32)                                   # -2, -1, 3, 4 are outside 0 .. 2
    exp, none, unkeyed = _same_as_twin(rows, points, None, 3)
    assert sum(sum(t.values()) for t in exp) + sum(none) + sum(unkeyed) == int(((points >= 0) & (points < 3)).sum())


def test_invalid_tally_shapes_are_refused():
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    tables = SW.new_tables(1, 16, torch.device("cuda"))
    pts = torch.zeros(4, dtype=torch.int32, device="cuda")
    for shape in ((5, 4, 3), (2, 4, 65), (4, 3)):
        with pytest.raises(ValueError):
            SW.tally_joint_device(tables, torch.zeros(shape, dtype=torch.uint8, device="cuda"), pts)
    from fluorosequencingimageanalysis_amd import _native_signal_sweep as NS
    rows = torch.zeros((2, 4, 3), dtype=torch.uint8, device="cuda")
    args = lambda K, F, slots: (rows.data_ptr(), K, F, pts.data_ptr(), None, 4, 1, slots, tables["keys"].data_ptr(),        # noqa: E731
                                tables["counts"].data_ptr(), tables["none"].data_ptr(), tables["unkeyed"].data_ptr(),
                                tables["overflow"].data_ptr(), None)
    assert NS.lib().fsq_signal_tally_joint(*args(2, 3, 16)) == 0
    for bad in ((0, 3, 16), (5, 3, 16), (2, 0, 16), (2, 65, 16), (2, 3, 12)):
        assert NS.lib().fsq_signal_tally_joint(*args(*bad)) != 0, bad
    torch.cuda.synchronize()
    assert int(tables["counts"].sum()) == 4


# ---- the batched simulation ----

def _labels_points_run(shape, fixed, points, n, stride, first_molecule=17, seed=9, first_row=0, n_rows=None):
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    base, values, _, letters = SW._joint_point_params(*shape, seed, first_molecule, points, fixed)
    with _prefilled():
        out = SW.simulate_labels_points_device(base, torch.from_numpy(values).cuda(), len(points), n, stride, first_row, n_rows)
        return {k: v.cpu().numpy() for k, v in out.items()}


def _single_labels(shape, fixed, point, n, first_molecule, seed=9):
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS
    p, b, u = point
    out = PS.multilabel_device(*shape, n, seed, first_molecule, p=p, b=b, u=u, **fixed)
    return {k: out[k].cpu().numpy() for k in ("counts", "intensity", "category")}


_singles = {}


def _expected(stride):
    """The three points' single-point tables, concatenated along the molecule axis: computed once per stride."""
    if stride not in _singles:
        each = [_single_labels(SHAPE2, FIXED2, point, 100, 17 + k * stride) for k, point in enumerate(POINTS3)]
        _singles[stride] = {k: np.concatenate([e[k] for e in each], axis=1) for k in ("counts", "intensity", "category")}
    return _singles[stride]


@pytest.mark.parametrize("stride", [0, 1000])
@pytest.mark.parametrize("first_row, n_rows", [(0, None), (37, 150)], ids=["whole", "rows_37_to_186"])
def test_points_are_the_single_point_kernel_bit_for_bit(stride, first_row, n_rows):
    got = _labels_points_run(SHAPE2, FIXED2, POINTS3, 100, stride, first_row=first_row, n_rows=n_rows)
    exp = _expected(stride)
    rows = slice(first_row, 300 if n_rows is None else first_row + n_rows)              # a chunk starts and ends inside a wavefront and a point
    assert got["counts"].shape == (2, rows.stop - rows.start, 6) and got["counts"].dtype == np.uint8
    assert np.array_equal(got["counts"], exp["counts"][:, rows])
    assert np.array_equal(got["intensity"].view(np.uint64), exp["intensity"][:, rows].view(np.uint64))
    assert np.array_equal(got["category"], exp["category"][:, rows])
    assert exp["counts"][0].max() > 0 and exp["counts"][1].max() > 0
    assert len({exp["counts"][:, k * 100:(k + 1) * 100].tobytes() for k in range(3)}) == 3


def test_one_channel_is_fsq_peptide_simulate_points():
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    shape, fixed = ("GAKAGAKC", "K", 2, 4), dict(s=0.1, sc=3, s2=0.05, beta=70000.0, beta_sigma=0.2, ddif=DDIF, superdye_rate=0.3)
    got = _labels_points_run(shape, fixed, POINTS3, 130, 1000)
    base, values, _ = SW._point_params(*shape, 9, 17, POINTS3, fixed)
    one = SW.simulate_points_device(base, torch.from_numpy(values).cuda(), 3, 130, 1000)
    for k in ("counts", "intensity", "category"):
        a, b = got[k][0], one[k].cpu().numpy()
        assert a.shape == b.shape and np.array_equal(a.view(np.uint64) if k == "intensity" else a, b.view(np.uint64) if k == "intensity" else b), k
    assert got["counts"].shape == (1, 390, 7) and got["counts"].max() == 2


def test_the_limit_shape_four_channels_sixty_four_frames():
    shape = ("GA" * 20 + "KCDE" * 6, "KCDE", 23, 40)                                     # 4 letters, 64 frames, 6 dyes a channel
    fixed = dict(s=0.02, sc=30, s2=0.01, beta={"K": 7e4, "C": 3e4, "D": 5e4, "E": 9e4}, beta_sigma=0.2, ddif=[0.0] + [0.3] * 14,
                 superdye_rate={"K": 0.3, "C": 0.0, "D": 1.0, "E": 0.0}, superdye_factor=2.0)
    points = [(0.9, 0.02, 0.1), (0.95, 0.01, 0.3)]
    got = _labels_points_run(shape, fixed, points, 70, 5)
    assert got["counts"].shape == (4, 140, 64)
    for k, point in enumerate(points):
        exp = _single_labels(shape, fixed, point, 70, 17 + 5 * k)
        rows = slice(70 * k, 70 * (k + 1))
        assert np.array_equal(got["counts"][:, rows], exp["counts"])
        assert np.array_equal(got["intensity"][:, rows].view(np.uint64), exp["intensity"].view(np.uint64))
        assert np.array_equal(got["category"][:, rows], exp["category"])
    assert got["counts"][:, :, 0].max() >= 5 and got["counts"][:, :, 63].max() > 0


def test_invalid_shapes_are_refused():
    """No shape within the limits of fsq_peptide_labels.h (4 channels, 64 frames) needs more LDS than a launch gets, so the entry's
    LDS check cannot be reached from here; a shape beyond them is refused by the parameter checks before it."""
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    base, values, _, _ = SW._joint_point_params(*SHAPE2, 9, 0, POINTS3, FIXED2)
    d_points = torch.from_numpy(values).cuda()
    for bad in (dict(first_row=280, n_rows=21), dict(first_row=-1, n_rows=5), dict(molecule_stride=-1)):
        with pytest.raises(ValueError):
            SW.simulate_labels_points_device(base, d_points, 3, 100, **bad)
    base.num_edmans = 64                                                                 # 66 frames
    with pytest.raises(ValueError):
        SW.simulate_labels_points_device(base, d_points, 3, 100)
    base.num_edmans, base.first_molecule = 4, 2 ** 63 - 50
    with pytest.raises(ValueError):
        SW.simulate_labels_points_device(base, d_points, 3, 100)
    base.first_molecule = 0
    assert SW.simulate_labels_points_device(base, d_points, 3, 100, first_row=300, n_rows=0)["counts"].shape == (2, 0, 6)


# ---- end to end ----

def _grid8():
    return host_sweep("grid8", SHAPE2, GRID8, 256, FIXED2)


@pytest.mark.parametrize("chunk_rows", [1 << 22, 97])
def test_the_sweep_is_its_host_twin(chunk_rows):
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    host = _grid8()
    with _prefilled():
        got = SW.joint_sweep_records(*SHAPE2, GRID8, 256, seed=5, chunk_rows=chunk_rows, **QUENCH, **FIXED2)
    assert got == host
    for key in GRID8:
        sig, mol = got["all_simulations"][key]
        assert len(mol) > 10 and len(sig) > 5 and 0 < got["none_count"][key] < got["total_count"][key] <= 256


def test_three_letters_unfitted():
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    host = host_sweep("three", SHAPE3, POINTS3, 200, FIXED3, fit=False)
    got = SW.joint_sweep_records(*SHAPE3, POINTS3, 200, seed=5, fit=False, chunk_rows=333, **FIXED3)
    assert got == host and got["labels"] == ("C", "D", "K") and all(len(got["all_simulations"][k][1]) > 20 for k in POINTS3)


def _bits(x):
    return None if x is None else np.float64(x).view(np.uint64)


@pytest.mark.parametrize("metric, norm", [("my_euclidean", dict(heatmap_normalize_counts=True)), ("my_canberra", dict(normalize_counts=True)),
                                          ("my_std_normalized_chebyshev", {})])
def test_scores_and_incompatibility_are_their_host_twins_bit_for_bit(metric, norm):
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    host = _grid8()
    observed = observed_of(host)
    dev = SW.joint_sweep_device(*SHAPE2, GRID8, 256, seed=5, **QUENCH, **FIXED2)
    opts = dict(metric=metric, on_error="none", heatmap_only=False, **norm)
    for sweep in (dev, host):                                                            # the tables where they are, and uploaded dicts
        got, exp = SW.score_records(observed, sweep, **opts), SW.score_records(observed, host, host=True, **opts)
        assert list(got) == GRID8 == list(exp)
        for key in GRID8:
            (r, (f, c)), (er, (ef, ec)) = got[key], exp[key]
            assert _bits(r) == _bits(er) and _bits(f) == _bits(ef) and set(c) == set(ec), key
            assert all(_bits(c[s]) == _bits(ec[s]) for s in c), key
    assert sum(r is not None for r, _ in exp.values()) >= 6
    cand = SW.joint_split_heatmap(("C", "K"), 5, 0)[1][:20]
    got = SW.incompatibility_records(observed, dev, cand, **opts)
    exp = SW.incompatibility_records(observed, host, cand, host=True, **opts)
    assert set(got["scores"]) == set(exp["scores"]) and len(exp["scores"]) > 3
    assert all(_bits(got["scores"][s]) == _bits(exp["scores"][s]) for s in exp["scores"])
    assert list(got["pairs"]) == list(exp["pairs"]) and len(exp["pairs"]) == 190
    for pair, (point, dist, factor) in exp["pairs"].items():
        g = got["pairs"][pair]
        assert g[0] == point and [_bits(x) for x in g[1]] == [_bits(x) for x in dist] and _bits(g[2]) == _bits(factor), pair


def test_match_diagnostic_of_a_joint_sweep():
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    host = _grid8()
    observed = observed_of(host)
    dev = SW.joint_sweep_device(*SHAPE2, GRID8, 256, seed=5, **QUENCH, **FIXED2)
    args = (observed, "my_euclidean", False, False, True, True, True, False, None, 0.1, 2, 1e9, True, 1, 0, 4)
    got, exp = SW.match_diagnostic(dev, *args, on_error="none"), SW.match_diagnostic(host, *args, host=True, on_error="none")
    for k in ("optimal_pbu", "normalized_plot_signals", "normalized_plot_molecular_signals", "exclude_signals", "tables", "labels"):
        assert got[k] == exp[k], k
    assert _bits(got["result"]) == _bits(exp["result"]) and got["tables"] is None and len(exp["incompatibility_scores"]) > 3
    assert {s: _bits(v) for s, v in got["incompatibility_scores"].items()} == {s: _bits(v) for s, v in exp["incompatibility_scores"].items()}
    assert {s: _bits(v) for s, v in got["diff_plot_signals"].items()} == {s: _bits(v) for s, v in exp["diff_plot_signals"].items()}


def test_joint_signals_of_fits_is_its_host_twin():
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    rng = np.random.default_rng(12)
    best = random_molecules(rng, 2, 700, 6, max_start=2)
    category = (rng.random((2, 700)) < 0.8).astype(np.int64) * 5
    found = (rng.random((2, 700)) < 0.9).astype(np.uint8)
    exp = SW.joint_signals_of_fits(("C", "K"), best, found, category, host=True)
    assert SW.joint_signals_of_fits(("C", "K"), best, found, category) == exp and len(exp) > 30


@pytest.mark.parametrize("ci", range(7))
def test_joint_signals_from_device_on_the_multilabel_cases(ci):
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS
    c = golden_cases()[ci]
    sim = PS.multilabel_device(c["sequence"], c["labels"], c["num_mocks"], c["num_edmans"], c["n"], seed=c["seed"],
                               first_molecule=c["first"], **c["api"])
    rec = {"labels": sim["labels"], "counts": sim["counts"].cpu().numpy()}
    assert PS.joint_signals_from_device(sim) == PS.joint_signals_of_records(rec), c["name"]


def test_joint_signals_from_device_keeps_its_other_route_for_unkeyed_molecules():
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS
    kw = dict(p=0.9, b=0.4, u=0.0, s=0.0, sc=0, s2=0.0, beta=7e4, beta_sigma=0.2, ddif=[0.0] * 15)
    sim = PS.multilabel_device("KKKKKKCCCCCC", "KC", 0, 8, 400, seed=2, **kw)           # up to 12 drops: beyond D(2) = 8
    rec = {"labels": sim["labels"], "counts": sim["counts"].cpu().numpy()}
    exp = PS.joint_signals_of_records(rec)
    assert PS.joint_signals_from_device(sim) == exp and max(len(s[0]) for s in exp) > 8


def test_command_line_in_a_child_process(tmp_path):
    from fluorosequencingimageanalysis_amd import sweep_peptide
    observed = observed_of(_grid8())
    with open(tmp_path / "joint.pkl", "wb") as f:
        pickle.dump(observed, f, protocol=2)
    common = ["GAKCAK", "KC", "--observed", str(tmp_path / "joint.pkl"), "--edman_efficiency", "0.8:0.95:2", "--dye_destruction",
              "0.05:0.15:2", "--dud_dyes", "0.2", "-N", "256", "-m", "2", "-o", "1", "-e", "4", "--seed", "5", "--fluor_intensity",
              "K=70000,C=30000", "--beta_sigma", "K=0.2,C=0.25", "--all_signals", "--score_multidrop"]
    run = subprocess.run([sys.executable, "-m", "fluorosequencingimageanalysis_amd.sweep_peptide"] + common +
                         ["--output_directory", str(tmp_path / "dev")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    path = [line for line in run.stdout.splitlines() if line.startswith("Saved results to ")][0][len("Saved results to "):]
    dev = pickle.load(open(path, "rb"))
    host = pickle.load(open(sweep_peptide.main(common + ["--host", "--output_directory", str(tmp_path / "host")]), "rb"))
    assert dev["labels"] == host["labels"] == ("C", "K") and len(dev["points"]) == 4
    assert dev["all_simulations"] == host["all_simulations"] and dev["total_count"] == host["total_count"]
    assert dev["best_point"][0] == host["best_point"][0] and _bits(dev["best_point"][1]) == _bits(host["best_point"][1])
    assert dev["best_point"][3] and set(dev["best_point"][3]) == set(host["best_point"][3])
