"""Background correction of joint signals (two-colour experiments) on the host: the twin (_host_background with
joint_neighbour_lists) against a plain-Python restatement written from the rules (tests/_joint_background_reference.py),
against the one-letter route and its recorded fixture, the helper functions on joint keys, the limits and the command line.
Nothing is compared with a tolerance; NaN equals NaN."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

import _joint_background_reference as JR
from _background_cases import bits, case, case_names, key, problem, same_dict, same_peaks
from _joint_background_cases import LETTERS, all_jkeys, as_joint, jkey, joint_dict, joint_problem, tiny_joint_problem
from _util import ROOT


def _v3(args, **kw):
    from fluorosequencingimageanalysis_amd import background as BG
    info = {}
    peak_list, undefined_peaks, raw, pct = BG.iterative_peak_finding_v3(*args, device=None, info=info, **kw)
    assert peak_list == []
    return undefined_peaks, raw, pct, info


def _joint_args(args, letters=None):
    boc, pct, avg, std = (joint_dict(d, letters) for d in args[:4])
    return (boc, pct, avg, std) + tuple(args[4:])


def _joint_peaks(peaks, letters=None):
    return [as_joint(u[:3], letters) + tuple(u[3:]) for u in peaks]


@pytest.mark.parametrize("n,multidrop", [(1, True), (2, True), (65, True), (65, False), (300, True), (300, False)])
def test_twin_equals_the_restatement_on_two_letters(n, multidrop):
    args = tiny_joint_problem(n) if n < 3 else joint_problem(n, 40 + n, include_multidrop=multidrop)
    assert len(args[0]) == n or not multidrop
    assert n < 3 or len(set(aa for k in args[0] for aa, _ in k[0])) == 2
    r = JR.iterate(*args)
    undefined_peaks, raw, pct, info = _v3(args, labels=LETTERS)
    same_dict(raw, r["updated_boc_raw"], n)
    same_dict(pct, r["updated_boc_percent"], n)
    same_peaks(undefined_peaks, r["undefined_peaks"], n)
    assert (info["stop_reason"], info["n_passes"], info["accepted_keys"]) == (r["stop"], r["passes"], r["accepted"])
    assert n < 100 or (r["accepted"] and r["undefined_peaks"])


@pytest.mark.parametrize("name", case_names())
def test_fixture_cases_as_one_letter_joint_keys_equal_golden(name):
    c = case(name)
    assert len(case_names()) == 9
    args = (c["boc_experiment"], c["boc_percent"], c["averaged_ac"], c["ac_stds"], c["num_cycles"], c["sigma"], not c["omit_multidrop"])
    undefined_peaks, raw, pct, info = _v3(_joint_args(args))
    same_dict(raw, joint_dict(c["updated_boc_raw"]), name)
    assert all(type(v) is int for v in raw.values())
    same_dict(pct, joint_dict(c["updated_boc_percent"]), name)
    same_peaks(undefined_peaks, _joint_peaks(c["undefined_peaks"]), name)
    assert (info["stop_reason"], info["n_passes"], info["accepted_keys"]) == (c["stop"], c["passes"], [as_joint(k) for k in c["accepted"]])


@pytest.mark.parametrize("multidrop", [True, False])
def test_two_letters_with_all_drops_in_one_channel_equal_one_letter(multidrop):
    args = problem(150, 9, include_multidrop=multidrop)
    up1, raw1, pct1, info1 = _v3(args)
    for letters in (('A', 'B'), ('0', 'A')):                           # the dropping letter is the first channel, and the second
        up2, raw2, pct2, info2 = _v3(_joint_args(args, letters), labels=letters)
        same_dict(raw2, joint_dict(raw1, letters), letters)
        same_dict(pct2, joint_dict(pct1, letters), letters)
        same_peaks(up2, _joint_peaks(up1, letters), letters)
        assert info2["accepted_keys"] == [as_joint(k, letters) for k in info1["accepted_keys"]] and info1["accepted_keys"]
        assert (info2["stop_reason"], info2["n_passes"]) == (info1["stop_reason"], info1["n_passes"])
    with pytest.raises(ValueError, match="labels"):                    # one letter never drops: it must be named
        _v3(_joint_args(args, ('A', 'B')))


def test_helpers_on_joint_keys():
    from fluorosequencingimageanalysis_amd import background as BG
    a, b, m = jkey([('C', 2), ('K', 3)]), jkey([('K', 4)]), jkey([('C', 2), ('K', 2)])
    remainder = ((('C', 2),), (True, False), (1, 1))
    signals = {a: 30, remainder: 50, b: 10, m: 60}
    assert BG.is_multidrop(m[0]) and not BG.is_multidrop(a[0])          # a cycle repeats, whatever the letters
    same_dict(BG.counts_to_percent(signals), {a: 0.3, b: 0.1, m: 0.6})
    same_dict(BG.counts_to_percent(signals, include_multidrop=False), {a: 0.75, b: 0.25})
    same_dict(BG.counts_to_percent(signals, include_remainders=True), {a: 0.2, remainder: 50 / 150.0, b: 10 / 150.0, m: 0.4})
    same_dict(BG.counts_to_percent(signals, max_cycle=3), {a: 30 / 90.0, m: 60 / 90.0})
    other = {a: 10, b: 30, remainder: 7}
    avg = BG.average_signals([signals, other])
    assert list(avg) == sorted([a, b, m]) and remainder not in avg
    assert avg[a] == (0.3 + 0.25) / 2 and avg[m] == 0.6 / 2
    std = BG.signals_std([signals, other])
    assert list(std) == list(avg) and bits([std[b]]) == bits([np.std([0.1, 0.75])])
    assert BG.generate_adjacent_positions(a) == [(1, 2), (1, 3), (1, 4), (2, 4), (3, 2), (3, 4)]                 # (2, 3) +- 1, no repeat
    assert BG.generate_adjacent_positions(a, include_multidrop=True) == [(1, 2), (1, 3), (1, 4), (2, 2), (2, 4), (3, 2), (3, 3), (3, 4)]
    with pytest.raises(ValueError, match="remainders"):
        BG.generate_adjacent_positions(remainder)
    with pytest.raises(ValueError, match="empty"):
        BG.generate_adjacent_positions(((), (True, True), (0, 0)))
    with pytest.raises(ValueError, match="remainders"):
        BG.joint_pack_problem({remainder: 5}, {remainder: 1.0}, {}, {}, 5, labels=LETTERS)
    with pytest.raises(ValueError, match="empty"):
        BG.joint_pack_problem({((), (True, True), (0, 0)): 5}, {((), (True, True), (0, 0)): 1.0}, {}, {}, 5, labels=LETTERS)
    # interpolate_signal: the mean over the kept neighbours of `a` within 3 cycles, as they stand
    table = {jkey([('C', 1), ('K', 2)]): 8.0, jkey([('C', 1), ('K', 3)]): 4.0, jkey([('C', 3), ('K', 3)]): 100.0, m: 6.0}
    got = BG.interpolate_signal(table, a, 3, include_multidrop=True)
    # kept: (1,2) (1,3) (2,2) (3,2) (3,3); ((C,3),(K,3)) is present and ascends (C before K at one cycle)
    assert bits([got]) == bits([np.mean([8.0, 4.0, 6.0, 0, 100.0])])
    assert bits([BG.interpolate_signal(table, a, 3)]) == bits([np.mean([8.0, 4.0, 0])])     # (1,2), (1,3) and (3,2) are kept
    assert np.isnan(BG.interpolate_signal(table, jkey([('C', 1)]), 1))


def test_a_crossing_perturbation_counts_zero():
    """The lookup does not canonicalise: ((K,2),(C,3)) perturbed by (+1, -1) is ((K,3),(C,2)), no experiment's key, and not the
    count of ((C,2),(K,3))."""
    from fluorosequencingimageanalysis_amd import _host_background as HB, _host_signal_sweep as HS, background as BG
    target, crossed = jkey([('K', 2), ('C', 3)]), jkey([('C', 2), ('K', 3)])
    assert target[0] == (('K', 2), ('C', 3)) and crossed[0] == (('C', 2), ('K', 3))
    signals = {target: 10, crossed: 800}
    assert BG.interpolate_signal(signals, target, 5, include_multidrop=True) == 0.0
    assert BG.interpolate_signal(signals, crossed, 5, include_multidrop=True) == 0.0
    straight = jkey([('K', 3), ('C', 4)])                              # (+1, +1): ascends, is looked up and found
    signals[straight] = 16
    assert BG.interpolate_signal(signals, target, 5, include_multidrop=True) == 16 / 8.0
    code = np.array([HS.joint_key_of_signal(LETTERS, k) for k in signals], dtype=np.uint64)
    (nb,) = HB.joint_neighbour_lists(code, 2, 5, True, rows=[0])
    assert nb.tolist() == [-1, -1, -1, -1, -1, -1, -1, 2]              # (+1, -1) is the 7th of 8 and absent; (+1, +1) the last
    # the whole iteration: the twin and the restatement agree where a crossing neighbour exists
    args = joint_problem(90, 3, C=6, D=2)
    assert any(k[0][0][0] == 'K' and len(k[0]) == 2 and k[0][1][0] == 'C' and k[0][1][1] == k[0][0][1] + 1 for k in args[0])
    r = JR.iterate(*args)
    _, raw, pct, info = _v3(args)
    same_dict(raw, r["updated_boc_raw"])
    same_dict(pct, r["updated_boc_percent"])


def test_joint_neighbour_lists_are_the_rule():
    from fluorosequencingimageanalysis_amd import _host_background as HB, _host_signal_sweep as HS
    for letters, C, D, md in ((LETTERS, 5, 3, False), (LETTERS, 4, 3, True), (('A',), 6, 4, False), (('C', 'K', 'S', 'Y'), 3, 2, True)):
        keys = all_jkeys(C, D, letters)[::3]
        row = {k: i for i, k in enumerate(keys)}
        code = np.array([HS.joint_key_of_signal(letters, k) for k in keys], dtype=np.uint64)
        lists = HB.joint_neighbour_lists(code, len(letters), C, md)
        for k, nb in zip(keys, lists):
            assert nb.tolist() == [row.get(q, -1) for q in JR.neighbours(k, C, md)], (letters, k)


def test_every_limit_is_refused_under_its_name():
    from fluorosequencingimageanalysis_amd import background as BG
    a = jkey([('C', 2), ('K', 3)])

    def pack(boc, num_cycles=10, **kw):
        return BG.joint_pack_problem(boc, {k: 1.0 / len(boc) for k in boc}, {}, {}, num_cycles, **kw)
    assert pack({a: 5})["n_channels"] == 2
    for cycles in (0, 64, -3):
        with pytest.raises(NotImplementedError, match="num_cycles"):
            pack({a: 5}, cycles)
    assert pack({a: 5}, 63)["num_cycles"] == 63 and pack({jkey([('C', 1), ('K', 2)]): 5}, 2)["num_cycles"] == 2
    for letters, cap in ((('A',), 8), (('C', 'K'), 8), (('C', 'K', 'S'), 6), (('C', 'K', 'S', 'Y'), 6)):
        ok = jkey([(letters[i % len(letters)], 1 + i) for i in range(cap)], letters)
        over = jkey([(letters[i % len(letters)], 1 + i) for i in range(cap + 1)], letters)
        assert len(pack({ok: 5}, labels=letters)["code"]) == 1
        with pytest.raises(NotImplementedError, match="%d drops" % cap):
            pack({over: 5}, labels=letters)
    start16 = ((('C', 2),) * 2, (True, True), (2, 16))
    with pytest.raises(NotImplementedError, match="15"):
        pack({start16: 5}, labels=LETTERS)
    with pytest.raises(ValueError, match="mixed"):
        BG.iterative_peak_finding_v3({a: 5, key(1): 3}, {a: 0.5, key(1): 0.5}, {}, {}, 5)
    with pytest.raises(ValueError, match="mixed"):
        BG.iterative_peak_finding_v3({a: 5}, {a: 1.0}, {key(1): 0.5}, {key(1): 0.1}, 5)
    three = jkey([('C', 2), ('S', 3)], ('C', 'K', 'S'))
    with pytest.raises(ValueError, match="letters"):
        pack({a: 5, three: 5})
    with pytest.raises(ValueError, match="letters"):
        pack({a: 5}, labels=('C', 'S'))
    # sum(3^d - 1) < 2^31: 327 400 keys of 8 drops ask for 6 560 entries each
    n = (1 << 31) // 6560 + 1
    code = np.full(n, BG.joint_pack_problem({jkey([('C', 1 + i) for i in range(8)]): 1}, {jkey([('C', 1 + i) for i in range(8)]): 1.0},
                                            {}, {}, 10, labels=LETTERS)["code"][0], dtype=np.uint64)
    big = {"code": code, "n_channels": 2, "num_cycles": 10}
    for device in (None, "cuda"):
        with pytest.raises(ValueError, match="2\\^31"):
            BG.joint_background_records([big], device=device)
    with pytest.raises(ValueError, match="letters"):
        BG.joint_background_records([pack({a: 5}), pack({three: 5}, labels=('C', 'K', 'S'))], device=None)
    with pytest.raises(ValueError, match="letters"):
        BG.joint_background_records([BG.pack_problem({key(1): 5}, {key(1): 1.0}, {}, {}, 5)], device=None)
    nine = dict(pack({jkey([('A', 1 + i) for i in range(8)], ('A',)): 5}, labels=('A',)))
    nine["code"] = nine["code"] | np.uint64(9 << (4 + 6 * 8))          # a ninth drop field by hand
    with pytest.raises(NotImplementedError, match="8 drops"):
        BG.joint_background_records([nine], device=None)
    with pytest.raises(NotImplementedError, match="host"):            # no device kernel iterates joint keys: said, not hidden
        BG.joint_background_records([pack({a: 5})], device="cuda")
    with pytest.raises(NotImplementedError, match="host"):
        BG.iterative_peak_finding_v3({a: 5}, {a: 1.0}, {}, {}, 5, device="cuda")
    with pytest.raises(ValueError, match="joint_background_records"):
        BG.background_records([pack({a: 5})], device=None)
    with pytest.raises(ValueError, match="6560"):
        BG.neighbour_means_records([np.zeros(6561, np.int64)], np.ones(3), device=None)
    got = BG.neighbour_means_records([[0, 2], [], [5, -1, 1]], [1.0, 2.0, 4.0], device=None)
    assert got[0] == 2.5 and np.isnan(got[1]) and got[2] == 2.0 / 3


def test_header_matches_binding_and_library():
    from fluorosequencingimageanalysis_amd import _native, _native_background as NB
    hdr = open(os.path.join(ROOT, "include", "fsq_background_joint.h")).read()
    declared = set(re.findall(r"\b(fsq_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(NB.JOINT_EXPORTED) and "fsq_background_neighbour_means" in declared
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    L = ctypes.CDLL(_native.LIB_PATH)
    for name in declared:
        getattr(L, name)
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (FSQ_BACKGROUND_JOINT_[A-Z_]+) (\d+)", hdr)}
    assert defines == NB.JOINT_CAPS and NB.JOINT_MAX_NEIGHBOURS == 3 ** NB.JOINT_MAX_DROPS - 1
    Lb = NB.lib()
    assert Lb.fsq_background_neighbour_means(None, None, -1, None, 0, None, None) < 0
    assert Lb.fsq_background_neighbour_means(None, None, 0, None, 0, None, None) == 0


# ---- the command line ----

def _write(tmp, boc, acs):
    from fluorosequencingimageanalysis_amd.pflib import _py2_pickle_bytes
    boc_path = str(tmp / "JointSignals_boc.pkl")
    with open(boc_path, "wb") as f:
        f.write(_py2_pickle_bytes(boc))
    rows = ["Index,Filepath,Mocks,Edmans,Mocks omitted,Description"]
    for i, ac in enumerate(acs):
        p = str(tmp / ("JointSignals_ac%d.pkl" % i))
        with open(p, "wb") as f:
            f.write(_py2_pickle_bytes(ac))
        rows.append('%d,%s,2,8,1,"ac %d"' % (i, p, i))
    csv_path = str(tmp / "ac.csv")
    with open(csv_path, "w") as f:
        f.write("\n".join(rows) + "\n")
    return boc_path, csv_path


def command_line_case(seed=5, n=90):
    """boc- and ac- joint pickles of two letters with remainders among them, and the arguments."""
    rng = np.random.default_rng(seed)
    keys = all_jkeys(6, 2)[:n]
    smooth = {k: 3000.0 * np.exp(-0.15 * sum(c for _, c in k[0])) for k in keys}
    boc = {k: int(round(v * rng.uniform(0.99, 1.01))) for k, v in smooth.items()}
    for i in rng.choice(n, 3, replace=False):
        boc[keys[i]] += 250
    acs = [{k: int(round(v * rng.uniform(0.9, 1.1))) for k, v in smooth.items()} for _ in range(3)]
    remainder = ((('C', 2),), (True, False), (1, 1))
    boc[remainder] = 400
    acs[0][remainder] = 90
    return boc, acs, remainder


@pytest.mark.parametrize("omit_multidrop", [False, True])
def test_command_line_on_two_letters(tmp_path, omit_multidrop):
    from fluorosequencingimageanalysis_amd import background as BG, iterative_background_v2 as CL, sweep_peptide
    boc, acs, remainder = command_line_case()
    boc_path, csv_path = _write(tmp_path, boc, acs)
    out = str(tmp_path / "out")
    argv = ["iterative_background_v2.py", "--boc_file", boc_path, "--ac_file", csv_path, "--num_cycles", "6", "--sigma", "2.0",
            "--output_directory", out, "--host"] + (["--omit_multidrop"] if omit_multidrop else [])
    res = CL.main(argv, timestamp_epoch=1500000000)
    names = sorted(os.listdir(out))
    assert names == ["average_background_ot27eo.pkl", "corrected_experiment_ot27eo.pkl", "experiment_background_ot27eo.pkl",
                     "std_background_ot27eo.pkl"]
    kept = {k: v for k, v in boc.items() if k != remainder and not (omit_multidrop and BG.is_multidrop(k[0]))}
    assert omit_multidrop == (len(kept) < len(boc) - 1)                # the repeated-cycle rule took keys out
    r = JR.iterate(kept, BG.counts_to_percent(kept, include_multidrop=not omit_multidrop),
                   BG.average_signals(acs, include_multidrop=not omit_multidrop),
                   BG.signals_std(acs, include_multidrop=not omit_multidrop), 6, 2.0, not omit_multidrop)
    assert r["accepted"] and res["info"]["accepted_keys"] == r["accepted"]
    files = {n.split("_ot27eo")[0]: pickle.loads(open(os.path.join(out, n), "rb").read()) for n in names}
    same_dict(files["experiment_background"], r["updated_boc_raw"])
    same_dict(files["corrected_experiment"], {k: max(kept[k] - v, 0) for k, v in r["updated_boc_raw"].items()})
    for d in files.values():
        assert d and all(isinstance(k[1], tuple) and all(k[1]) and len(k[2]) == 2 for k in d) and remainder not in d
    with pytest.raises(NotImplementedError, match="--host"):           # joint files run on the host only, and the run says so
        CL.main([a for a in argv if a != "--host"], timestamp_epoch=1500000000, device="cuda")
    observed = sweep_peptide.load_observed(os.path.join(out, "corrected_experiment_ot27eo.pkl"))
    assert observed == files["corrected_experiment"] and list(observed) == list(files["corrected_experiment"])


def test_command_line_refuses_mixed_files(tmp_path):
    from fluorosequencingimageanalysis_amd import iterative_background_v2 as CL
    boc, acs, _ = command_line_case()
    one_letter = {key(1): 5, key(2): 7}
    three = {jkey([('C', 2), ('S', 3)], ('C', 'K', 'S')): 4}
    for k, (b, a, what) in enumerate(((boc, [one_letter], "joint"), (one_letter, acs, "joint"), (boc, [three], "letters"))):
        work = tmp_path / str(k)
        work.mkdir()
        boc_path, csv_path = _write(work, b, a)
        with pytest.raises(ValueError, match=what):
            CL.main(["iterative_background_v2.py", "--boc_file", boc_path, "--ac_file", csv_path, "--num_cycles", "6", "--host",
                     "--output_directory", str(work / "out")], timestamp_epoch=1500000000)
