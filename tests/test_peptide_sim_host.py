"""Peptide Monte-Carlo simulation, host side (no GPU needed): the Philox known answers, the NumPy twin against the reference's
recorded runs under the same draws (tests/golden/peptide_sim.npz), the drop-ins' tuples and event buffers, convert_to_oldstyle
and the photometries CSV against the recorded text, the command line on the twin, and one distribution check."""
import math
import os
import pickle
import re

import numpy as np
import pytest

from fluorosequencingimageanalysis_amd import _host_lognormal as R
from fluorosequencingimageanalysis_amd import _host_peptide_sim as T
from _peptide_sim_cases import golden, golden_cases, same_records
from _util import ROOT, _bits


def test_philox_known_answers():
    for counter, key, words in T.KNOWN_ANSWERS:
        assert T.philox(counter, key) == words
    got = T.philox_np([c for c, _, _ in T.KNOWN_ANSWERS], [k for _, k, _ in T.KNOWN_ANSWERS])
    assert got.tolist() == [list(w) for _, _, w in T.KNOWN_ANSWERS]
    # the vectorised draws are the scalar ones, across the carry into counter word 2
    u = T.uniforms_np(77, [2 ** 32 - 1, 2 ** 32, 5], 1, 5)
    assert u[1, 3] == T.uniform(77, 2 ** 32, 1, 3) and u[0, 4] == T.uniform(77, 2 ** 32 - 1, 1, 4) and u[2, 0] == T.uniform(77, 5, 1, 0)
    assert 0.0 <= u.min() and u.max() < 1.0


def test_fixture_is_not_vacuous():
    cases = golden_cases()
    assert len(cases) >= 6
    causes = np.concatenate([c["tables"]["loss_cause"].reshape(-1) for c in cases])
    assert set(causes.tolist()) == {0, 1, 2, 3, 4}
    assert any((c["tables"]["edman_fail"] != 0).any() for c in cases)
    assert any(c["twin"]["superdye_rate"] not in (0.0, 1.0) for c in cases) and any(c["twin"]["superdye_rate"] == 1.0 for c in cases)
    assert any(c["first"] < 2 ** 32 <= c["first"] + c["n"] for c in cases)           # the carry into counter word 2
    assert any(c["tables"]["counts"].shape[1] == 1 for c in cases) and any(c["tables"]["counts"].max() >= 10 for c in cases)
    assert any(c["twin"]["length"] < c["num_edmans"] for c in cases)
    assert max(len({tuple(r) for r in c["tables"]["counts"].tolist()}) for c in cases) >= 35


@pytest.mark.parametrize("ci", range(6))
def test_twin_equals_the_reference_under_the_same_draws(ci):
    c = golden_cases()[ci]
    got = T.simulate(seed=c["seed"], first_molecule=c["first"], n_molecules=c["n"], **c["twin"])
    same_records(got, dict(c["tables"], intensity=c["intensity"]), c["name"])
    exp_log = np.array([[math.log(x) if x > 0 else -10000.0 for x in row] for row in c["intensity"].tolist()])
    assert np.array_equal(_bits(got["log_intensity"]), _bits(exp_log))
    # a chunk has the streams of the whole
    part = T.simulate(seed=c["seed"], first_molecule=c["first"] + 40, n_molecules=30, **c["twin"])
    same_records(part, {k: v[40:70] for k, v in got.items()}, c["name"])


@pytest.mark.parametrize("ci", range(6))
def test_drop_ins_rebuild_the_reference_tuples(ci):
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS
    c = golden_cases()[ci]
    n = len(c["tuples"])
    res = PS.simulate_dye_counts(c["sequence"], c["label"], c["num_mocks"], c["num_edmans"], n, random_seed=c["seed"],
                                 reserved_character=c["reserved"], first_molecule=c["first"], host=True, **c["api"])
    assert len(res) == n
    for i, (dec, dye_counts, events, tracker) in enumerate(res):
        category, (intensities,) = PS.simulate_photometries(dye_counts[c["label"]], c["api"]["beta"], c["api"]["beta_sigma"], 1,
                                                            ddif=c["api"]["ddif"], superdye_rate=c["api"]["superdye_rate"],
                                                            superdye_factor=c["api"]["superdye_factor"])
        assert repr((dec, dict(dye_counts), events, tracker, category)) == c["tuples"][i], (c["name"], i)
        assert all(isinstance(e, PS.FluorEvent) for e in events)
        assert np.array_equal(_bits(intensities), _bits(c["intensity"][i])), (c["name"], i)
        assert PS.events_from_records(dye_counts[c["label"]].records, i) == events
    merged = PS.peptide_simulation(c["sequence"], c["label"], c["num_mocks"], c["num_edmans"], n, random_seed=c["seed"],
                                   num_processes=3, reserved_character=c["reserved"], first_molecule=c["first"], host=True, **c["api"])
    assert [m[:3] for m in merged] == [r[:3] for r in res]
    assert [m[3][c["label"]][1][0] for m in merged] == [tuple(x) for x in c["intensity"][:n].tolist()]


def test_out_of_scope_arguments():
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS
    kw = golden_cases()[0]["api"]
    with pytest.raises(NotImplementedError):
        PS.simulation_records("GAKC", "KC", 1, 1, 2, host=True, **kw)
    with pytest.raises(NotImplementedError):
        PS.simulation_records("GAKC", "K", 1, 1, 2, host=True, distance_ddif={1: 0.1}, **kw)
    with pytest.raises(NotImplementedError):
        PS.simulate_photometries((1, 0), 1.0, 0.2, 1)
    for bad in (dict(sequence=""), dict(sequence="A" * 65), dict(sequence="K" * 16), dict(num_mocks=40, num_edmans=24),
                dict(sequence="KKK", ddif=[0.0, 0.1]), dict(seed=1 << 64), dict(superdye_rate=1.5)):
        a = dict(sequence="GAKC", labels="K", num_mocks=1, num_edmans=1, num_simulations=1, host=True)
        a.update(kw)
        a.update(bad)
        with pytest.raises(ValueError):
            PS.simulation_records(**a)


def test_binding_declares_the_header():
    from fluorosequencingimageanalysis_amd import _native_peptide_sim as NP
    text = open(os.path.join(ROOT, "include", "fsq_peptide_sim.h")).read()
    assert set(re.findall(r"^int (fsq_\w+)\(", text, re.M)) == set(NP.EXPORTED)
    fields = re.search(r"typedef struct \{(.*?)\} FsqPeptideSimParams;", text, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip().split("[")[0] for decl in fields.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in NP.FsqPeptideSimParams._fields_]
    mk = open(os.path.join(ROOT, "fluorosequencingimageanalysis_amd", "csrc", "Makefile")).read()
    assert "$(wildcard simulate/*.hip)" in mk and "fsq_peptide_sim.h" in mk and "simulate/*.o" in mk


def test_convert_to_oldstyle_and_csv_reproduce_the_recorded_text(tmp_path):
    from fluorosequencingimageanalysis_amd import lognormal as LN
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS
    g, c = golden(), golden_cases()[0]
    merged = PS.peptide_simulation(c["sequence"], c["label"], c["num_mocks"], c["num_edmans"], c["n"], random_seed=c["seed"],
                                   reserved_character=c["reserved"], first_molecule=c["first"], host=True, **c["api"])
    index_of = {id(m[2]): i for i, m in enumerate(merged)}
    old = PS.convert_to_oldstyle(merged)
    assert [index_of[id(o[2])] for o in old] == g["old_kept"].tolist()
    assert repr([o[0] for o in old]) == str(g["old_decrements"])
    photometries, mes, t = {'ch1': {0: {}}}, {}, 0
    for dec, dye_counts, events, idict in old:                                     # (simulate_peptide.py:243-252)
        for label, (category, (intensities,)) in idict.items():
            assert label == 'A'
            photometries['ch1'][0].setdefault((t, t), (category, intensities, t))
            t += 1
        (label, seq), = dye_counts.items()
        key = (dec, True if seq[-1] == 0 else False, seq[0])
        mes[key] = mes.get(key, 0) + 1
    assert repr(sorted(mes.items())) == str(g["old_molecular_error_signals"])
    path = str(tmp_path / "x.csv")
    assert LN.write_photometries_dict_to_csv(photometries=photometries, filepath=path) == len(old)
    assert open(path, newline='').read() == g["old_csv"].tobytes().decode()


def _expected_pickle(sequence, label, n, seed, mocks=3, edmans=8, multidrop=True):
    """What simulate_peptide pickles at its defaults, from the twin's records and the restated fit."""
    ddif = [0, 0.3] + [0.3] * 5
    mask = sum(1 << i for i, ch in enumerate(sequence) if ch == label)
    b = -math.log(1.0 - 0.1)
    rec = T.simulate(len(sequence), mask, mocks, edmans, 0.9, math.e ** -b, 0.5, 0.3, 3, 0.1, math.log(70000.0), 0.2, ddif, 0.0, 1.0, seed, 0, n)
    means = [math.log(70000.0) + math.log(i + 1.0) - ddif[i] for i in range(7)]
    signals, mes, rows = {}, {}, []
    for counts, inten in zip(rec["counts"].tolist(), rec["intensity"].tolist()):
        if not any(counts):
            continue
        dec = tuple(('A', f) for f in range(1, len(counts)) for _ in range(counts[f - 1] - counts[f])) or (('A', 0),)
        key = (dec, counts[-1] == 0, counts[0])
        mes[key] = mes.get(key, 0) + 1
        cat = tuple(x > 0 for x in counts)
        rows.append((cat, inten))
        signal, is_zero, _, _, _, _, start = R.intensities_to_signal(inten, 0.2, 5, multidrop, 3, cat, means)
        if signal is not None:
            signals[(signal, is_zero, start)] = signals.get((signal, is_zero, start), 0) + 1
    return signals, mes, rows


def test_command_line_on_the_twin(tmp_path, capsys):
    from fluorosequencingimageanalysis_amd import simulate_peptide as SP
    from fluorosequencingimageanalysis_amd.pflib import _py2_str
    path = SP.main(["GAKAGAKC", "K", "-N", "150", "--seed", "20240902", "--host", "--output_directory", str(tmp_path / "out"),
                    "--distance_ddifs", "0.1", "0.2", "-n", "2"])
    printed = capsys.readouterr().out
    assert "Seed: 20240902" in printed and "Parameters loaded. Starting simulation at " in printed
    assert "Simulation complete. Fitting simulated tracks at " in printed and ". Saving results to " + os.path.basename(path) in printed
    assert re.fullmatch(r"Simulated_[0-9a-z]+\.pkl", os.path.basename(path))
    raw = open(path, "rb").read()
    assert not raw.startswith(b"\x80")                                           # protocol 0
    args, signals, mes = pickle.loads(raw)
    exp_signals, exp_mes, rows = _expected_pickle("GAKAGAKC", "K", 150, 20240902)
    assert signals == exp_signals and mes == exp_mes and len(mes) > 5 and len(signals) > 5
    assert args.seed == 20240902 and args.num_sims == 150 and args.num_mocks == 4 and args.num_mocks_omitted == 1 and args.num_edmans == 8
    assert "Wrote %d rows to " % len(rows) in printed
    lines = open(path[:-4] + ".csv", newline='').read().split("\r\n")
    assert lines[0] == "CHANNEL,FIELD,H,W,CATEGORY," + ",".join("FRAME %d" % i for i in range(12)) and len(lines) == len(rows) + 2
    for t, (cat, inten) in enumerate(rows):
        assert lines[t + 1] == 'ch1,0,%d,%d,"%s",%s' % (t, t, str(cat), ",".join(_py2_str(x) for x in inten)), t
    # --no_csv, --no_multidrop, and a fresh seed when none is given
    path2 = SP.main(["GAKAGAKC", "K", "-N", "40", "--host", "--no_csv", "--no_multidrop", "--output_directory", str(tmp_path / "out2")])
    args2, signals2, mes2 = pickle.load(open(path2, "rb"))
    assert os.listdir(str(tmp_path / "out2")) == [os.path.basename(path2)]
    exp2 = _expected_pickle("GAKAGAKC", "K", 40, args2.seed, multidrop=False)
    assert 0 <= args2.seed < 2 ** 64 and (signals2, mes2) == exp2[:2]


def test_draws_are_distributed_as_the_model_says():
    """65 536 molecules with 3 labelled residues and one mock cycle under a fixed seed: Pearson's statistic of the frame-0
    counts against Binomial(3, (1 - u) per_cycle_b), and of (count at frame 0, dyes dropped at the mock) against strip with
    probability s, else Binomial(count, 1 - per_cycle_b), each below the chi-squared quantile of 1e-9.  (A fixed seed: a
    deterministic condition, checked to hold before the seed was committed; statistics 6.86 and 20.46 against bounds of 44.8 and 60.7.)"""
    from scipy.stats import chi2
    n, u, pcb, s = 65536, 0.5, 0.9, 0.3
    rec = T.simulate(5, 0b10101, 1, 0, 0.9, pcb, u, s, 3, 0.1, math.log(70000.0), 0.2, [0.0, 0.3, 0.3], 0.0, 1.0, 0xC0FFEE, 0, n)
    counts = rec["counts"].astype(int)
    q = (1 - u) * pcb
    p0 = [math.comb(3, k) * q ** k * (1 - q) ** (3 - k) for k in range(4)]
    obs0 = np.bincount(counts[:, 0], minlength=4)
    stat0 = sum((o - n * e) ** 2 / (n * e) for o, e in zip(obs0.tolist(), p0))
    print("frame 0:", obs0.tolist(), stat0)
    assert stat0 < chi2.isf(1e-9, 3)
    stat1, cells = 0.0, 0
    for c in range(4):
        for d in range(c + 1):
            e = n * p0[c] * ((s if d == c else 0.0) + (1 - s) * math.comb(c, d) * (1 - pcb) ** d * pcb ** (c - d))
            o = int(((counts[:, 0] == c) & (counts[:, 0] - counts[:, 1] == d)).sum())
            assert e > 50
            stat1 += (o - e) ** 2 / e
            cells += 1
    print("first mock:", stat1)
    assert cells == 10 and stat1 < chi2.isf(1e-9, cells - 1)
