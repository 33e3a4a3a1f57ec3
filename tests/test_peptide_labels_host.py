"""Peptide Monte-Carlo simulation for several label letters, host side (no GPU needed): the NumPy twin against the reference's
recorded runs under the same draws (tests/golden/peptide_labels.npz), the drop-ins' tuples and event buffers, the one-letter
case against the existing simulation, the binding against the header, the refusals, and the command line on the twin.
Every comparison is exact: integers equal, floats by bit pattern."""
import math
import os
import pickle
import re

import numpy as np
import pytest

from fluorosequencingimageanalysis_amd import _host_lognormal as R
from fluorosequencingimageanalysis_amd import _host_peptide_sim as T
from _peptide_labels_cases import golden_cases, log_of, same_records
from _peptide_sim_cases import golden_cases as one_letter_cases
from _util import ROOT, _bits

N_CASES = 7
CLI_DDIF = [0, 0.3] + [0.3] * 5


def _case(name):
    return next(c for c in golden_cases() if c["name"] == name)


def test_fixture_is_not_vacuous():
    cases = golden_cases()
    assert len(cases) == N_CASES and [c["name"] for c in cases][0] == "two_letters"
    seen, two_in_one_cycle, dark_and_lit = set(), 0, 0
    for c in cases:
        pos = [ch for ch in c["sequence"] if ch in c["letters"]]
        cause, cyc = c["tables"]["loss_cause"], c["tables"]["loss_cycle"]
        for k, letter in enumerate(pos):
            seen |= {(c["letters"].index(letter) if len(c["letters"]) > 1 else -1, x) for x in set(cause[:, k].tolist())}
        for i in range(c["n"]):
            lost = {(int(cyc[i, k]), pos[k]) for k in range(len(pos)) if cause[i, k]}
            two_in_one_cycle += any(len({L for cy, L in lost if cy == f}) > 1 for f in range(c["tables"]["counts"].shape[2]))
        cat = c["tables"]["category"]
        dark_and_lit += int(((cat == 0).any(axis=0) & (cat != 0).any(axis=0)).sum())
    # every cause, and a surviving dye, in each of the first three channels of a case with several letters
    assert {(k, x) for k in range(3) for x in range(5)} <= seen
    assert two_in_one_cycle > 20 and dark_and_lit > 20
    assert len(_case("three_interleaved")["letters"]) == 3 and _case("three_interleaved")["labels"] != "CDK"
    rates = _case("three_interleaved")["twin"]["superdye_rate"]
    assert sorted(rates) == [0.0, 0.0, 0.4] and len(set(_case("three_interleaved")["twin"]["log_beta"])) == 3
    c = _case("three_interleaved")
    assert c["first"] < 2 ** 32 <= c["first"] + c["n"]                            # the carry into counter word 2
    absent = _case("absent_letter")
    k = absent["letters"].index("Y")
    assert "Y" not in absent["sequence"] and not absent["tables"]["counts"][k].any() and not absent["tables"]["category"][k].any()
    assert not absent["intensity"][k].any() and absent["tables"]["counts"][1 - k].any()
    assert len(_case("shorter_than_edmans")["sequence"]) < _case("shorter_than_edmans")["num_edmans"]
    assert _case("mocks_only")["num_edmans"] == 0 and _case("mocks_only")["num_mocks"] > 0
    assert _case("one_frame")["tables"]["counts"].shape[2] == 1
    assert any((c["tables"]["edman_fail"] != 0).any() for c in cases)


@pytest.mark.parametrize("ci", range(N_CASES))
def test_twin_equals_the_reference_under_the_same_draws(ci):
    c = golden_cases()[ci]
    got = T.simulate_labels(seed=c["seed"], first_molecule=c["first"], n_molecules=c["n"], **c["twin"])
    same_records(got, dict(c["tables"], intensity=c["intensity"], log_intensity=log_of(c["intensity"])), c["name"])
    # a chunk has the streams of the whole
    part = T.simulate_labels(seed=c["seed"], first_molecule=c["first"] + 40, n_molecules=30, **c["twin"])
    same_records(part, {k: (v[:, 40:70] if k in ("counts", "intensity", "log_intensity", "category") else v[40:70])
                        for k, v in got.items()}, c["name"])


def test_one_letter_is_the_existing_case():
    """Case (g) was recorded with the parameters of tests/golden/peptide_sim.npz's first case: the same tables."""
    c, old = _case("one_letter"), one_letter_cases()[0]
    assert (c["sequence"], c["labels"], c["seed"], c["first"]) == (old["sequence"], old["label"], old["seed"], old["first"])
    n = c["n"]
    for k in ("counts", "category"):
        assert np.array_equal(c["tables"][k][0], old["tables"][k][:n]), k
    for k in ("loss_cycle", "loss_cause", "edman_fail", "n_draws"):
        assert np.array_equal(c["tables"][k], old["tables"][k][:n]), k
    assert np.array_equal(_bits(c["intensity"][0]), _bits(old["intensity"][:n]))


@pytest.mark.parametrize("ci", range(N_CASES))
def test_drop_ins_rebuild_the_reference_tuples(ci):
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS
    c = golden_cases()[ci]
    n = len(c["tuples"])
    args = (c["sequence"], c["labels"], c["num_mocks"], c["num_edmans"], n)
    kw = dict(random_seed=c["seed"], reserved_character=c["reserved"], first_molecule=c["first"], host=True, **c["api"])
    res = PS.simulate_dye_counts(*args, **kw)
    assert len(res) == n
    records = PS.multilabel_records(*args, seed=c["seed"], first_molecule=c["first"], host=True, **c["api"])
    for i, (dec, dye_counts, events, tracker) in enumerate(res):
        categories = {}
        for k, letter in enumerate(c["letters"]):
            a = c["api"]
            category, (intensities,) = PS.simulate_photometries(dye_counts[letter], a["beta"][letter], a["beta_sigma"][letter], 1,
                                                                ddif=a["ddif"][letter], superdye_rate=a["superdye_rate"][letter],
                                                                superdye_factor=a["superdye_factor"][letter])
            categories[letter] = category
            assert np.array_equal(_bits(intensities), _bits(c["intensity"][k][i])), (c["name"], i, letter)
        assert list(dye_counts) == c["letters"]
        assert repr((dec, dict(dye_counts), events, tracker, categories)) == c["tuples"][i], (c["name"], i)
        assert all(isinstance(e, PS.FluorEvent) for e in events)
        assert PS.events_from_records(records, i, c["reserved"]) == events
    merged = PS.peptide_simulation(*args, num_processes=3, **kw)
    assert [m[:3] for m in merged] == [r[:3] for r in res]
    for k, letter in enumerate(c["letters"]):
        assert [m[3][letter][1][0] for m in merged] == [tuple(x) for x in c["intensity"][k][:n].tolist()]
    if len(c["letters"]) > 1:
        with pytest.raises(Exception, match="Oldstyle only works with one label."):
            PS.convert_to_oldstyle(merged)


def test_issue_example_decrements_keep_the_reference_order():
    """Within a cycle the decrements stand in event order - Edman, strip, destruction, each in position order - not in
    letter order: some recorded molecule loses a K before a C in one cycle and another a C before a K."""
    orders = set()
    for text in _case("two_letters")["tuples"] + _case("three_interleaved")["tuples"]:
        dec = eval(text, {"FluorEvent": lambda **k: None})[0]
        orders |= {(a[0], b[0]) for a, b in zip(dec[:-1], dec[1:]) if a[1] == b[1] and a[0] != b[0]}
    assert ("K", "C") in orders and ("C", "K") in orders


@pytest.mark.parametrize("ci", [0, 1, 6])
def test_one_letter_through_multilabel_records_equals_simulation_records(ci):
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS
    c = one_letter_cases()[ci if ci < 6 else 3]
    args = (c["sequence"], c["label"], c["num_mocks"], c["num_edmans"], 60)
    one = PS.simulation_records(*args, seed=c["seed"], first_molecule=c["first"], host=True, **c["api"])
    many = PS.multilabel_records(*args, seed=c["seed"], first_molecule=c["first"], host=True, **c["api"])
    assert many["labels"] == (c["label"],) and [p for p, k in many["positions"]] == [i for i, ch in enumerate(c["sequence"]) if ch == c["label"]]
    for k in ("counts", "intensity", "log_intensity", "category"):
        assert many[k].shape == (1,) + one[k].shape and many[k].dtype == one[k].dtype, k
        assert np.array_equal(many[k][0].view(np.uint64) if many[k].dtype == np.float64 else many[k][0],
                              one[k].view(np.uint64) if one[k].dtype == np.float64 else one[k]), k
    for k in ("loss_cycle", "loss_cause", "edman_fail", "n_draws"):
        assert many[k].shape == one[k].shape and many[k].dtype == one[k].dtype and np.array_equal(many[k], one[k]), k


@pytest.mark.parametrize("ci", range(N_CASES))
def test_counts_follow_from_the_loss_tables(ci):
    """A dye of channel k is there at frame f iff its cause is none or its loss cycle is greater than f."""
    c = golden_cases()[ci]
    got = T.simulate_labels(seed=c["seed"] ^ 1, first_molecule=c["first"], n_molecules=80, **c["twin"])
    pos, channel_of, F = T.check_channels(c["twin"]["length"], c["twin"]["channel_masks"], c["num_mocks"], c["num_edmans"], c["twin"]["ddif"])
    assert [c["sequence"][i] for i in pos] == [c["letters"][k] for k in channel_of]
    K = len(c["letters"])
    for i in range(80):
        exp = T.counts_from_losses(channel_of, got["loss_cycle"][i].tolist(), got["loss_cause"][i].tolist(), K, F)
        assert got["counts"][:, i].tolist() == exp, (c["name"], i)
    assert (np.diff(got["counts"].astype(int), axis=2) <= 0).all()


def test_the_order_of_the_letters_changes_nothing():
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS
    c = _case("three_interleaved")
    args = (c["num_mocks"], c["num_edmans"], 50)
    ref = PS.multilabel_records(c["sequence"], "CDK", *args, seed=9, host=True, **c["api"])
    for labels in ("KDC", "DKC", ["K", "C", "D", "K"], {"D", "C", "K"}):
        got = PS.multilabel_records(c["sequence"], labels, *args, seed=9, host=True, **c["api"])
        assert got["labels"] == ("C", "D", "K") and got["positions"] == ref["positions"]
        same_records(got, ref, labels)


def test_scalar_and_dict_parameters_agree():
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS
    kw = dict(p=0.9, b=0.1, u=0.3, s=0.2, sc=2, s2=0.05)
    scalar = dict(beta=52000.0, beta_sigma=0.25, ddif=[0.0, 0.2, 0.3], superdye_rate=0.4, superdye_factor=2.5)
    a = PS.multilabel_records("KCAKC", "KC", 1, 3, 60, seed=11, host=True, **kw, **scalar)
    b = PS.multilabel_records("KCAKC", "KC", 1, 3, 60, seed=11, host=True, **kw, **{k: {"K": v, "C": v} for k, v in scalar.items()})
    same_records(a, b)
    assert a["intensity"].any() and not np.array_equal(a["intensity"][0], a["intensity"][1])
    # a dict changes its own letter's channel alone
    c = PS.multilabel_records("KCAKC", "KC", 1, 3, 60, seed=11, host=True, **kw, **dict(scalar, beta={"K": 52000.0, "C": 9000.0}))
    assert np.array_equal(_bits(c["intensity"][1]), _bits(a["intensity"][1])) and np.array_equal(c["counts"], a["counts"])
    lit = a["intensity"][0] > 0
    assert lit.any() and (c["intensity"][0][lit] < a["intensity"][0][lit]).all()
    with pytest.raises(ValueError, match="beta has no value"):
        PS.multilabel_records("KCAKC", "KC", 1, 3, 2, seed=11, host=True, **kw, **dict(scalar, beta={"K": 52000.0}))


def test_binding_declares_the_header():
    from fluorosequencingimageanalysis_amd import _native_peptide_labels as NL
    text = open(os.path.join(ROOT, "include", "fsq_peptide_labels.h")).read()
    assert set(re.findall(r"^int (fsq_\w+)\(", text, re.M)) == set(NL.EXPORTED) == {"fsq_peptide_simulate_labels"}
    fields = re.search(r"typedef struct \{(.*?)\} FsqPeptideLabelsParams;", text, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    decls = [decl.strip().split(None, 1) for decl in fields.split(";") if decl.strip()]
    names = [n.strip().split("[")[0] for _, rest in decls for n in rest.split(",")]
    assert names == [f[0] for f in NL.FsqPeptideLabelsParams._fields_]
    # array extents and element types, field by field
    import ctypes
    ctype = {"uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "int32_t": ctypes.c_int32}
    extent = {"FSQ_PEPTIDE_MAX_CHANNELS": NL.MAX_CHANNELS, "FSQ_PEPTIDE_MAX_LABELLED": NL.MAX_LABELLED}
    declared = dict(NL.FsqPeptideLabelsParams._fields_)
    for base, rest in decls:
        for n in rest.split(","):
            t = ctype[base]
            for dim in reversed(re.findall(r"\[(\w+)\]", n)):
                t = t * extent[dim]
            assert declared[n.strip().split("[")[0]] is t, n
    assert int(re.search(r"#define FSQ_PEPTIDE_MAX_CHANNELS (\d+)", text).group(1)) == NL.MAX_CHANNELS == T.MAX_CHANNELS == 4
    mk = open(os.path.join(ROOT, "fluorosequencingimageanalysis_amd", "csrc", "Makefile")).read()
    assert "$(wildcard simulate/*.hip)" in mk and "fsq_peptide_labels.h" in mk
    assert os.path.exists(os.path.join(ROOT, "fluorosequencingimageanalysis_amd", "csrc", "simulate", "fsq_peptide_labels.hip"))
    # the draw contract: the streams of the channels, none of them the proteome Monte-Carlo's stream 3
    streams = [(T.superdye_stream(k), T.normal_stream(k)) for k in range(4)]
    assert streams == [(1, 2), (4, 5), (6, 7), (8, 9)]


def test_refusals():
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    kw = one_letter_cases()[0]["api"]
    with pytest.raises(NotImplementedError, match="one label"):
        PS.simulation_records("GAKC", "KC", 1, 1, 2, host=True, **kw)
    with pytest.raises(NotImplementedError, match="one label"):
        PS.simulate_device("GAKC", "KC", 1, 1, 2, **kw)
    with pytest.raises(NotImplementedError, match="distance_ddif"):
        PS.multilabel_records("GAKC", "KC", 1, 1, 2, host=True, distance_ddif={1: 0.1}, **kw)
    with pytest.raises(NotImplementedError, match="at most 4 label letters"):
        PS.multilabel_records("GAKCDE", "GAKCD", 1, 1, 2, host=True, **kw)
    with pytest.raises(ValueError, match="at most 15 labelled residues of one letter"):
        PS.multilabel_records("K" * 16 + "C", "KC", 1, 1, 2, host=True, **dict(kw, ddif=[0.0] * 15))
    with pytest.raises(NotImplementedError, match="one label"):
        SW.sweep_records("GAKC", "KC", 1, 1, [dict(p=0.9)], 4, host=True, **{k: v for k, v in kw.items() if k != "p"})
    # 15 of each of two letters is served: the cap is per colour
    ok = PS.multilabel_records("KC" * 15, "KC", 0, 1, 2, host=True, **dict(kw, ddif=[0.0] * 15, u=0.0))
    assert ok["counts"].shape == (2, 2, 2) and ok["loss_cause"].shape == (2, 30)
    for bad in (dict(sequence=""), dict(sequence="A" * 65), dict(num_mocks=40, num_edmans=24), dict(sequence="KKKC", ddif=[0.0, 0.1]),
                dict(seed=1 << 64), dict(superdye_rate={"K": 0.5, "C": 1.5}), dict(labels=""), dict(beta=float("inf"))):
        a = dict(sequence="GAKC", labels="KC", num_mocks=1, num_edmans=1, num_simulations=1, host=True)
        a.update(kw)
        a.update(bad)
        with pytest.raises(ValueError):
            PS.multilabel_records(**a)
    with pytest.raises(NotImplementedError):
        PS.simulate_photometries((1, 0), 1.0, 0.2, 1)
    with pytest.raises(ValueError):
        T.simulate_labels(4, [0b0011, 0b0110], 1, 1, 0.9, 0.9, 0.1, 0.1, 1, 0.1, [1.0] * 2, [0.2] * 2, [[0.0] * 3] * 2, [0.0] * 2, [1.0] * 2)
    with pytest.raises(ValueError):
        T.simulate_labels(4, [1, 2, 4, 8, 0], 1, 1, 0.9, 0.9, 0.1, 0.1, 1, 0.1, [1.0] * 5, [0.2] * 5, [[0.0]] * 5, [0.0] * 5, [1.0] * 5)


def test_joint_signal_definition():
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS
    key = PS.joint_signal(("C", "K"), [[1, 1, 0, 0], [3, 1, 1, 1]])
    assert key == ((("K", 1), ("K", 1), ("C", 2)), (True, False), (1, 3))
    assert PS.joint_signal(("C", "K"), [[0, 0], [2, 2]]) == ((), (True, False), (0, 2))
    assert PS.joint_signal(("C", "K"), [[1, 0], [1, 0]])[0] == (("C", 1), ("K", 1))
    records = {"labels": ("C", "K"), "counts": np.array([[[1, 0], [0, 0], [1, 0]], [[1, 0], [0, 0], [1, 0]]], np.uint8)}
    assert PS.joint_signals_of_records(records) == {((("C", 1), ("K", 1)), (True, True), (1, 1)): 2}


def _expected_cli(sequence, labels, n, seed, mocks=3, edmans=8):
    """What simulate_peptide pickles and writes at its defaults for several letters, from the twin's records and the
    restated fit."""
    letters = sorted(set(labels))
    b = -math.log(1.0 - 0.1)
    K = len(letters)
    masks = [sum(1 << i for i, ch in enumerate(sequence) if ch == letter) for letter in letters]
    rec = T.simulate_labels(len(sequence), masks, mocks, edmans, 0.9, math.e ** -b, 0.5, 0.3, 3, 0.1, [math.log(70000.0)] * K, [0.2] * K,
                            [CLI_DDIF] * K, [0.0] * K, [1.0] * K, seed, 0, n)
    means = [math.log(70000.0) + math.log(i + 1.0) - CLI_DDIF[i] for i in range(7)]
    signals, mes, rows = {letter: {} for letter in letters}, {}, []
    for i in range(n):
        joint = rec["counts"][:, i].tolist()
        if any(row[0] for row in joint):
            dec = tuple((L, c) for c in range(1, mocks + edmans + 1) for L, row in zip(letters, joint) for _ in range(row[c - 1] - row[c]))
            key = (dec, tuple(row[-1] == 0 for row in joint), tuple(row[0] for row in joint))
            mes[key] = mes.get(key, 0) + 1
    for k, letter in enumerate(letters):
        t = 0
        for counts, inten in zip(rec["counts"][k].tolist(), rec["intensity"][k].tolist()):
            if not any(counts):
                continue
            cat = tuple(x > 0 for x in counts)
            rows.append(("ch%d" % (k + 1), t, cat, inten))
            t += 1
            signal, is_zero, _, _, _, _, start = R.intensities_to_signal(inten, 0.2, 5, True, 3, cat, means)
            if signal is not None:
                signals[letter][(signal, is_zero, start)] = signals[letter].get((signal, is_zero, start), 0) + 1
    return signals, mes, rows


def test_command_line_on_the_twin(tmp_path, capsys):
    from fluorosequencingimageanalysis_amd import simulate_peptide as SP
    from fluorosequencingimageanalysis_amd.pflib import _py2_str
    path = SP.main(["GAKCGAKC", "KC", "-N", "120", "--seed", "20240918", "--host", "--output_directory", str(tmp_path / "out")])
    printed = capsys.readouterr().out
    assert "Seed: 20240918" in printed and ". Saving results to " + os.path.basename(path) in printed
    raw = open(path, "rb").read()
    assert not raw.startswith(b"\x80")                                           # protocol 0
    args, signals, mes = pickle.loads(raw)
    exp_signals, exp_mes, rows = _expected_cli("GAKCGAKC", "KC", 120, 20240918)
    assert list(signals) == ["C", "K"] and signals == exp_signals and mes == exp_mes
    assert len(mes) > 10 and all(len(s) > 3 for s in signals.values()) and signals["C"] != signals["K"]
    assert args.seed == 20240918 and args.num_sims == 120 and args.labels == ["KC"]
    assert "Wrote %d rows to " % len(rows) in printed
    lines = open(path[:-4] + ".csv", newline='').read().split("\r\n")
    assert lines[0] == "CHANNEL,FIELD,H,W,CATEGORY," + ",".join("FRAME %d" % i for i in range(12)) and len(lines) == len(rows) + 2
    assert {r[0] for r in rows} == {"ch1", "ch2"}
    for j, (channel, t, cat, inten) in enumerate(rows):
        assert lines[j + 1] == '%s,0,%d,%d,"%s",%s' % (channel, t, t, str(cat), ",".join(_py2_str(x) for x in inten)), j
    # --no_csv writes the pickle alone
    path2 = SP.main(["GAKCGAKC", "CK", "-N", "30", "--seed", "20240918", "--host", "--no_csv", "--output_directory", str(tmp_path / "out2")])
    assert os.listdir(str(tmp_path / "out2")) == [os.path.basename(path2)]
    assert pickle.load(open(path2, "rb"))[1:] == _expected_cli("GAKCGAKC", "KC", 30, 20240918)[:2]
