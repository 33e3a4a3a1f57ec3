"""The colocalisation of tracks between colour channels without a GPU: the NumPy twin against the plain-Python restatement of
the definition, the merge over K channels, joint_observed_records(host=True) against fits aligned by hand, the command line
and the errors."""
import csv
import os
import re

import numpy as np
import pytest

from _colocalize_cases import (BIG, SIGMA, channel_tables, experiment, match_cases, photometries_of, plain_match, plain_molecules,
                               segments)
from _lognormal_chain_cases import same_chain

from fluorosequencingimageanalysis_amd import _host_colocalize as H
from fluorosequencingimageanalysis_amd import colocalize as CL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = match_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_twin_equals_the_plain_loop(name):
    a_hw, a_field, b_hw, b_field, r2 = CASES[name]
    sa_hw, a_seg, a_off, sb_hw, b_seg, b_off = segments(a_hw, a_field, b_hw, b_field)
    exp = plain_match(sa_hw.tolist(), a_seg.tolist(), sb_hw.tolist(), b_seg.tolist(), r2)
    got = H.match(sa_hw, a_seg, a_off, sb_hw, b_off, r2)
    assert [g.dtype for g in got] == [np.int32, np.int32, np.int64]
    assert [g.tolist() for g in got] == [list(e) for e in exp], name
    assert CL.match_records(sa_hw, a_seg, a_off, sb_hw, b_off, r2, host=True)[0].tolist() == list(exp[0])


def test_the_cases_say_what_they_are_meant_to():
    def of(name):
        a_hw, a_field, b_hw, b_field, r2 = CASES[name]
        sa_hw, a_seg, a_off, sb_hw, b_seg, b_off = segments(a_hw, a_field, b_hw, b_field)
        return [x.tolist() for x in H.match(sa_hw, a_seg, a_off, sb_hw, b_off, r2)]
    assert of("two b at one distance") == [[0], [0, -1, -1], [1]]
    assert of("two a at one distance") == [[0, -1, -1], [0], [1, -1, -1]]
    assert of("duplicate positions") == [[0, -1, 2], [0, -1, 2, -1], [0, -1, 0]]
    assert of("no second choice") == [[-1, 0], [1, -1], [-1, 0]]
    assert of("at the radius") == [[0, -1], [0, -1], [4, -1]]                   # d2 = 4 pairs, d2 = 5 does not
    assert of("radius 0") == [[-1, 1, 2], [-1, 1, 2, -1], [-1, 0, 0]]
    assert of("radius 2.5") == [[0, -1, -1], [0, -1, -1], [5, -1, -1]]          # 5 <= 6 < 8 < 9
    assert of("one each, other fields") == [[-1], [-1], [-1]]
    assert of("the corners") == [[-1, 1], [-1, 1], [-1, 1]]
    assert of("across the plane") == [[0], [0], [(1 << 63) - (1 << 34) + 8]]    # int64 does not wrap
    assert of("across the plane, one short") == [[-1], [-1], [-1]]
    assert of("unsorted fields") == [[1, 0, 3, 2], [1, 0, 3, 2], [0, 0, 0, 0]]  # grouped by field: all four pair
    sizes = of("field sizes")
    assert len(sizes[0]) == 323 and 200 < sum(m >= 0 for m in sizes[0]) < 323


def test_radius_squared_is_exact():
    assert [H.radius_sq_of(r) for r in (0, 0.0, 1, 2, 2.5, 2.4494897427831779, 2.45, 3, np.float32(1.5), np.int64(7))] == \
        [0, 0, 1, 4, 6, 5, 6, 9, 2, 49]
    assert H.radius_sq_of(3037000499) == 3037000499 ** 2 and H.radius_sq_of(2.0 ** 31) == 1 << 62
    for bad in (-1, -0.5, float("nan"), float("inf"), 2.0 ** 32):
        with pytest.raises(ValueError):
            H.radius_sq_of(bad)


def test_twin_refuses_what_the_kernel_flags():
    a_hw, b_hw = np.zeros((4, 2), np.int64), np.zeros((3, 2), np.int64)
    good = (np.array([0, 0, 1, 1], np.int32), np.array([0, 2, 4]), np.array([0, 1, 3]))
    bad, flag = H.bad_lanes(*good, 4, 3)
    assert not flag and not bad.any()
    for a_seg, a_off, b_off, lanes in (
            ([0, -1, 1, 2], [0, 2, 4], [0, 1, 3], [0, 1, 0, 1]),        # a_seg out of range
            ([0, 0, 1, 1], [0, 2, 5], [0, 1, 3], [0, 0, 1, 1]),         # an offset beyond n_a
            ([0, 0, 1, 1], [0, 2, 4], [0, 4, 3], [1, 1, 1, 1]),         # b's offsets descend
            ([0, 0, 1, 1], [0, 2, 4], [-1, 1, 3], [1, 1, 0, 0]),        # a negative offset
            ([0, 1, 1, 1], [0, 2, 4], [0, 1, 3], [0, 1, 0, 0]),         # a lane outside its segment's range
            ([0, 0, 1, 1], [0, 2, 4], [0, 1, 2], [0, 0, 0, 0]),         # b's offsets end before n_b: the flag alone
            ([0, 0, 1, 1], [1, 2, 4], [0, 1, 3], [1, 0, 0, 0])):        # a's start after 0
        bad, flag = H.bad_lanes(a_seg, a_off, b_off, 4, 3)
        assert flag and bad.tolist() == [bool(x) for x in lanes], (a_seg, a_off, b_off)
        with pytest.raises(ValueError, match="not well formed"):
            H.match(a_hw, a_seg, a_off, b_hw, b_off, 4)


@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("seed", [1, 2])
def test_molecules_equal_the_sequential_definition(K, seed):
    tables, offsets = channel_tables(seed, K)
    for radius, r2 in ((2, 4), (1.5, 2), (0, 0)):
        member, field, hw = plain_molecules([(hw.tolist(), f.tolist()) for hw, f in tables], r2, offsets)
        got = H.molecules(tables, radius, offsets)
        assert got["member"].dtype == np.int32 and got["member"].shape == (K, len(field))
        assert got["member"].tolist() == member and got["field"].tolist() == field and got["hw"].tolist() == hw, (K, seed, radius)
        again = CL.molecules_records(tables, radius, offsets, host=True)
        assert all(np.array_equal(again[k], got[k]) for k in got)
    # every track stands in exactly one molecule, fields ascend, and with K >= 2 some molecules have several members
    got = H.molecules(tables, 2, offsets)
    for k, (hw, _) in enumerate(tables):
        assert sorted(t for t in got["member"][k].tolist() if t >= 0) == list(range(len(hw)))
    assert (np.diff(got["field"]) >= 0).all() and (K == 1 or ((got["member"] >= 0).sum(axis=0) > 1).sum() > 20)


def test_molecules_without_an_offset_do_not_match_shifted_tables():
    tables, offsets = channel_tables(1, 2)
    with_offset, without = H.molecules(tables, 1, offsets), H.molecules(tables, 1)
    assert with_offset["member"].shape[1] < without["member"].shape[1]


# ---- joint_observed_records ----

def _aligned(tables, out, on_filtered):
    """(best [K][M'][F], found, lit) of the molecules that count, aligned by hand from `member` and the channels' chains."""
    from fluorosequencingimageanalysis_amd import lognormal as LN
    letters, member = out["labels"], out["molecules"]["member"]
    F = tables[letters[0]][0].shape[1]
    rows = []
    n_rejected = 0
    for m in range(member.shape[1]):
        best, found, lit, failed = [], [], [], False
        for k, L in enumerate(letters):
            t = int(member[k][m])
            kept = out["kept"][L].tolist()
            if t >= 0 and t not in kept:
                failed = True
            if t < 0 or t not in kept:
                best.append([0] * F), found.append(0), lit.append(0)
                continue
            fit1 = out["channels"][L]["fit1"]
            i = kept.index(t)
            best.append(fit1["best_seq"][i][:F].tolist()), found.append(int(fit1["status"][i] == LN.STATUS_FOUND)), lit.append(1)
        if (failed and on_filtered == "reject") or not any(lit):
            n_rejected += 1
        else:
            rows.append((best, found, lit))
    K = len(letters)
    return (np.array([[r[0][k] for r in rows] for k in range(K)], np.uint8).reshape(K, len(rows), F),
            np.array([[r[1][k] for r in rows] for k in range(K)], np.uint8).reshape(K, len(rows)),
            np.array([[r[2][k] for r in rows] for k in range(K)], np.uint8).reshape(K, len(rows)), n_rejected)


@pytest.fixture(scope="module")
def host_runs():
    tables, _ = experiment()
    return {mode: CL.joint_observed_records(tables, SIGMA, radius=2, on_filtered=mode, host=True) for mode in CL.ON_FILTERED}


@pytest.mark.parametrize("mode", CL.ON_FILTERED)
def test_joint_observed_records_against_fits_aligned_by_hand(host_runs, mode):
    from fluorosequencingimageanalysis_amd import lognormal as LN
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    tables, molecule_of = experiment()
    out = host_runs[mode]
    assert out["labels"] == ("C", "K")
    for L in out["labels"]:
        intensity, words, field, _, _ = tables[L]
        at = np.flatnonzero(CL.downstep_filtered(words, 8))
        assert np.array_equal(out["kept"][L], at) and 0 < len(at) < len(words)
        same_chain(out["channels"][L], LN.chain_records(intensity[at], words[at], field[at], SIGMA[L], host=True), L)
    best, found, lit, n_rejected = _aligned(tables, out, mode)
    assert out["signals"] == SW.joint_signals_of_fits(out["labels"], best, found, lit, host=True)
    M = out["molecules"]["member"].shape[1]
    assert out["n_molecules"] == M and out["n_rejected"] == n_rejected == int(out["rejected"].sum())
    assert out["total_count"] == M - n_rejected == sum(out["signals"].values()) + out["none_count"]
    assert out["none_count"] == int(((lit == 1) & (found == 0)).any(axis=0).sum())
    assert len(out["signals"]) > 10 and n_rejected > 0
    # the molecules are the simulated ones: two tracks share a molecule exactly when they came from one
    member = out["molecules"]["member"]
    both = (member >= 0).all(axis=0)
    assert both.sum() > 100
    assert np.array_equal(molecule_of["C"][member[0][both]], molecule_of["K"][member[1][both]])
    alone = set(molecule_of["C"][member[0][member[1] < 0]].tolist()) & set(molecule_of["K"][member[1][member[0] < 0]].tolist())
    assert not alone


def test_on_filtered_dark_keeps_what_reject_drops(host_runs):
    reject, dark = host_runs["reject"], host_runs["dark"]
    assert np.array_equal(reject["molecules"]["member"], dark["molecules"]["member"])
    assert dark["n_rejected"] < reject["n_rejected"] and not (dark["rejected"] & ~reject["rejected"]).any()
    assert sum(dark["signals"].values()) > sum(reject["signals"].values())
    # in dark mode a filtered member's channel reads as no member at all
    k, m = np.argwhere((reject["fit_index"] < 0) & (reject["molecules"]["member"] >= 0) & ~dark["rejected"][None, :])[0]
    assert dark["fit_index"][k][m] == -1 and reject["rejected"][m]


def test_per_letter_values_and_one_letter(host_runs):
    tables, _ = experiment()
    one = CL.joint_observed_records({"K": tables["K"]}, 0.2, host=True)
    assert one["labels"] == ("K",) and one["molecules"]["member"].shape[0] == 1
    assert one["total_count"] == one["channels"]["K"]["total_count"]                 # the filtered tracks, each a molecule
    assert one["none_count"] == one["channels"]["K"]["none_count"]
    # K = 1: the joint signals are the channel's own, under the joint signal's form
    assert sum(one["signals"].values()) == sum(one["channels"]["K"]["signals"].values())
    with pytest.raises(ValueError, match="no value for the label letters"):
        CL.joint_observed_records(tables, {"K": 0.2}, host=True)
    moved = dict(tables, K=tables["K"][:3] + (tables["K"][3] + np.array([40, -7]),) + tables["K"][4:])
    a = CL.joint_observed_records(moved, SIGMA, offsets={"K": (-40, 7)}, host=True)
    b = host_runs["reject"]
    assert a["signals"] == b["signals"] and np.array_equal(a["molecules"]["member"], b["molecules"]["member"])
    assert np.array_equal(a["molecules"]["hw"], b["molecules"]["hw"])
    assert H.molecules([(moved[L][3], moved[L][2]) for L in "CK"], 2)["member"].shape[1] > b["n_molecules"]


def test_the_errors():
    tables, _ = experiment()
    K, C = tables["K"], tables["C"]
    with pytest.raises(ValueError, match="same number of frames"):
        CL.joint_observed_records({"K": K, "C": (C[0][:, :7],) + C[1:]}, SIGMA, host=True)
    with pytest.raises(ValueError, match="1 .. 4 label letters"):
        CL.joint_observed_records({L: K for L in "ABCDE"}, 0.2, host=True)
    with pytest.raises(ValueError, match="1 .. 4 channels"):
        H.molecules([(K[3], K[2])] * 5, 2)
    for value in (1 << 30, -(1 << 30)):
        hw = K[3].copy()
        hw[3, 1] = value
        with pytest.raises(ValueError, match=r"\|coordinate\| < 2\^30"):
            CL.joint_observed_records({"K": K[:3] + (hw,) + K[4:], "C": C}, SIGMA, host=True)
        with pytest.raises(ValueError, match=r"\|coordinate\| < 2\^30"):
            H.match(hw, np.zeros(len(hw), np.int32), [0, len(hw)], hw, [0, len(hw)], 4)
    hw = K[3].copy()
    hw[3, 1] = BIG                                                  # the largest one passes; an offset that lifts it does not
    CL.molecules_records([(hw, K[2]), (C[3], C[2])], 2, host=True)
    with pytest.raises(ValueError, match=r"\|coordinate\| < 2\^30"):
        CL.molecules_records([(hw, K[2]), (C[3], C[2])], 2, offsets=[(0, 1), (0, 0)], host=True)
    with pytest.raises(ValueError, match="negative"):
        CL.joint_observed_records(tables, SIGMA, radius=-1, host=True)
    with pytest.raises(ValueError, match="negative"):
        H.match(K[3], np.zeros(len(K[3]), np.int32), [0, len(K[3])], K[3], [0, len(K[3])], -1)
    with pytest.raises(ValueError, match="on_filtered"):
        CL.joint_observed_records(tables, SIGMA, on_filtered="keep", host=True)
    with pytest.raises(ValueError, match="table_slots=1000"):
        CL.joint_observed_records(tables, SIGMA, table_slots=1000, host=True)
    with pytest.raises(ValueError, match="have no table"):
        CL.joint_observed_records(tables, SIGMA, offsets={"D": (0, 0)}, host=True)
    with pytest.raises(ValueError, match="integers"):
        H.molecules([(K[3].astype(np.float64), K[2])], 2)
    with pytest.raises(NotImplementedError, match="64 frames"):
        CL.joint_observed_records({"K": (np.zeros((2, 65)), np.ones(2, np.uint64), np.zeros(2, np.int64), np.zeros((2, 2), np.int64),
                                         np.arange(2))}, 0.2, host=True)


def test_the_joint_key_limits_stand(host_runs):
    """More drops over both channels than the two-letter key holds: NotImplementedError naming the limit."""
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    best = np.zeros((2, 1, 8), np.uint8)
    best[0, 0], best[1, 0] = [5, 4, 3, 2, 1, 0, 0, 0], [4, 3, 2, 1, 0, 0, 0, 0]          # 9 drops, D(2) = 8
    with pytest.raises(NotImplementedError, match="more than 8 drops"):
        SW.joint_signals_of_fits(("C", "K"), best, np.ones((2, 1), np.uint8), np.ones((2, 1), np.uint8), host=True)


# ---- the command line ----

def test_command_line_on_the_host(tmp_path, capsys, host_runs):
    from fluorosequencingimageanalysis_amd import joint_signals, lognormal as LN, sweep_peptide
    tables, _ = experiment()
    channel_of = {"K": "ch1", "C": "ch2"}
    path = str(tmp_path / "track_photometries_abc123.csv")
    n_rows = LN.write_photometries_dict_to_csv(photometries_of(tables, channel_of), path)
    assert n_rows == sum(len(t[0]) for t in tables.values())
    signals_path, molecules_path = joint_signals.main([path, "--labels", "K=ch1", "C=ch2", "--beta_sigma", "K=0.2,C=0.25", "--host",
                                                       "--output_directory", str(tmp_path / "out")])
    assert re.fullmatch(r"JointSignals_\w+\.pkl", os.path.basename(signals_path))
    assert re.fullmatch(r"JointMolecules_\w+\.csv", os.path.basename(molecules_path))
    observed = sweep_peptide.load_observed(signals_path)
    read = joint_signals.read_tables(path, channel_of)
    # the file's tables are the experiment's but for the rows, which are the file's own: so is the result
    for L in "CK":
        assert all(np.array_equal(x, y) for x, y in zip(read[L][:4], tables[L][:4]))
    assert read["C"][4].tolist() == list(range(1, len(read["C"][4]) + 1))
    exp = host_runs["reject"]
    assert observed == exp["signals"] and type(observed) is dict and len(observed) > 10
    with open(molecules_path, newline="") as f:
        lines = list(csv.reader(f))
    assert lines[0] == ["FIELD", "H", "W", "REJECTED", "ROW C", "STATUS C", "SIGNAL C", "ROW K", "STATUS K", "SIGNAL K"]
    assert len(lines) == 1 + exp["n_molecules"]
    assert sum(line[3] == "True" for line in lines[1:]) == exp["n_rejected"]
    assert {line[5] for line in lines[1:]} <= {"", "FOUND", "NONE", "FILTERED"} and any(line[5] == "FILTERED" for line in lines[1:])
    rows_c = [int(line[4]) for line in lines[1:] if line[4]]
    assert sorted(rows_c) == sorted(read["C"][4].tolist())           # every track of the channel stands in one molecule
    text = capsys.readouterr().out
    assert "Molecules: %d, rejected: %d, counted: %d" % (exp["n_molecules"], exp["n_rejected"], exp["total_count"]) in text
    assert "Letter C (ch2)" in text and "alpha " + repr(float(exp["channels"]["C"]["alpha"])) in text
    # the other options: dark mode, and a shift of one channel that its --offset takes back
    shifted = dict(tables, K=tables["K"][:3] + (tables["K"][3] + np.array([3, -4]),) + tables["K"][4:])
    LN.write_photometries_dict_to_csv(photometries_of(shifted, channel_of), path)
    dark, _ = joint_signals.main([path, "--labels", "K=ch1", "C=ch2", "--beta_sigma", "K=0.2,C=0.25", "--host", "--on_filtered", "dark",
                                  "--offset", "K=-3,4", "--radius", "2.0", "--output_directory", str(tmp_path / "dark")])
    assert sweep_peptide.load_observed(dark) == host_runs["dark"]["signals"] != observed
    for argv in ([path, "--labels", "K=ch1", "K=ch2"], [path, "--labels", "K=ch1", "C=ch1"], [path, "--labels", "K=ch1", "--offset", "C=1,2"],
                 [path, "--labels", "Kch1"], [path, "--labels", "K=ch1", "--offset", "K=1"]):
        with pytest.raises(SystemExit):
            joint_signals.main(argv)
    with pytest.raises(ValueError, match="no track of channel ch3"):
        joint_signals.main([path, "--labels", "K=ch1", "C=ch3", "--host"])


def test_the_header_declares_what_the_binding_binds():
    from fluorosequencingimageanalysis_amd import _native_colocalize as NCL
    with open(os.path.join(ROOT, "include", "fsq_colocalize.h")) as f:
        text = f.read()
    assert set(re.findall(r"^int (fsq_\w+)\(", text, re.M)) == set(NCL.EXPORTED) == {"fsq_colocalize_match"}
    with open(os.path.join(ROOT, "fluorosequencingimageanalysis_amd", "csrc", "Makefile")) as f:
        assert "../../include/fsq_colocalize.h" in f.read()
