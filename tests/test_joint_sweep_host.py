"""Sweeps over several label letters without a GPU: the joint 64-bit signal key (include/fsq_signal_sweep.h) and its codec, the
twin's joint tally against the plain-Python peptide_simulator.joint_signal, the key table's rules for joint signals, and the
host sweep against a per-point loop.  There is no reference output for joint signals (the reference stops at one letter): the
oracle is joint_signal, and K = 1 is tied to the one-letter key."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from fluorosequencingimageanalysis_amd import _host_lognormal
from fluorosequencingimageanalysis_amd import _host_signal_sweep as H
from fluorosequencingimageanalysis_amd import _native_signal_sweep as NS
from fluorosequencingimageanalysis_amd import _tracks, peptide_simulator as PS, signal_sweep as SW
from _joint_sweep_cases import DDIF, FIXED2, FIXED3, GRID4, HAND, LETTERS, QUENCH, SHAPE2, SHAPE3, hand_rows, pad, random_molecules
from _signal_sweep_cases import case, case_names

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def _short_rows(K, frames, max_start):
    """Every molecule of K non-increasing rows of `frames` frames that start at max_start or below."""
    one = [r for r in itertools.product(range(max_start + 1), repeat=frames) if all(a >= b for a, b in zip(r, r[1:]))]
    return itertools.product(one, repeat=K)


# ---- the key ----

def test_constants_are_the_headers():
    text = open(os.path.join(ROOT, "include", "fsq_signal_sweep.h")).read()
    bits = re.search(r"#define FSQ_SIGNAL_JOINT_DROP_BITS\(K\) \(\(K\) <= 1 \? (\d+) : \(K\) == 2 \? (\d+) : (\d+)\)", text).groups()
    drops = re.search(r"#define FSQ_SIGNAL_JOINT_MAX_DROPS\(K\) \(\(K\) <= 1 \? (\d+) : \(K\) == 2 \? (\d+) : (\d+)\)", text).groups()
    for K in (1, 2, 3, 4):
        assert H.JOINT_DROP_BITS[K] == NS.JOINT_DROP_BITS[K] == int(bits[min(K, 3) - 1]) == 6 + (K - 1).bit_length()
        assert H.JOINT_MAX_DROPS[K] == NS.JOINT_MAX_DROPS[K] == int(drops[min(K, 3) - 1])
        # the drops end below the top nibbles
        assert 4 + H.JOINT_DROP_BITS[K] * H.JOINT_MAX_DROPS[K] <= 64 - 4 * (K - 1)
    assert [H.JOINT_MAX_DROPS[K] for K in (1, 2, 3, 4)] == [10, 8, 6, 6] and H.JOINT_MAX_DROPS[1] == H.MAX_DROPS


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_key_round_trip(K):
    letters = LETTERS[K]
    rng = np.random.default_rng(K)
    mols = [np.array(rows) for rows, kind, _ in hand_rows(K) if kind == H.ROW_SIGNAL]
    mols += list(random_molecules(rng, K, 300, 7, max_start=4 - K if K < 3 else 1, upstep_rate=0.0).transpose(1, 0, 2))
    seen = {}
    for rows in mols:
        rows = rows.tolist()
        kind, key = H.classify_joint_rows(rows)
        sig = PS.joint_signal(letters, rows)
        if kind == H.ROW_UNKEYED:
            assert len(sig[0]) > H.JOINT_MAX_DROPS[K] and H.joint_key_of_signal(letters, sig) is None
            continue
        assert kind == H.ROW_SIGNAL and 0 <= key < 1 << 64
        assert H.joint_signal_of_key(letters, key) == sig                      # the key holds the whole signal
        assert H.joint_key_of_signal(letters, sig) == key
        assert H.joint_signal_of_key(letters, np.array([key], np.uint64).view(np.int64)[0]) == sig      # (read signed)
        assert seen.setdefault(key, sig) == sig                                 # and nothing else
    assert len(seen) > 20


def test_hand_rows():
    for rows, kind, sig in HAND:
        K = len(rows)
        got_kind, key = H.classify_joint_rows(rows)
        assert got_kind == kind, rows
        if kind == H.ROW_SIGNAL:
            assert PS.joint_signal(LETTERS[K], rows) == sig, rows
            assert H.joint_signal_of_key(LETTERS[K], key) == sig, rows
            assert H.classify_joint_rows(pad(rows, 64)) == (kind, key)         # the last frames add nothing
        else:
            assert key is None


def test_one_channel_is_the_one_letter_key():
    signals = set()
    for name in case_names():
        observed, fit, opts = case(name)
        signals |= set(observed) | set(fit)
    assert len(signals) > 50
    for s, z, start in signals:
        joint = (() if tuple(s) == H.NO_DROPS else tuple(s), (bool(z),), (start,))
        assert H.joint_key_of_signal(("A",), joint) == H.key_of_signal((s, z, start)) is not None
        assert H.joint_signal_of_key(("A",), H.key_of_signal((s, z, start))) == joint
    rng = np.random.default_rng(3)
    rows = random_molecules(rng, 1, 500, 9, max_start=6)
    for row in rows[0].tolist():
        assert H.classify_joint_rows([row]) == H.classify_row(row)
    for row in ([11] + [0] * 5, [12] + [0] * 5, [16, 16], [15, 15]):                    # 11 drops, 12, a start of 16, of 15
        assert H.classify_joint_rows([row]) == H.classify_row(row)
    assert H.tally_joint_rows(rows, np.zeros(500, np.int32), None, 1) == H.tally_rows(rows[0], np.zeros(500, np.int32), None, 1)


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_the_sentinels_are_never_keys(K):
    letters = LETTERS[K]
    # structurally: bit 10 or 11 alone decodes to a drop whose cycle is 0, or to a drop that follows an absent one
    B = H.JOINT_DROP_BITS[K]
    for sentinel in (H.EMPTY, H.NEVER):
        assert sentinel & 15 == 0 and sentinel >> (4 + B * H.JOINT_MAX_DROPS[K]) == 0       # every start is 0, no bit beyond the drops
        fields = [(sentinel >> (4 + B * i)) & ((1 << B) - 1) for i in range(H.JOINT_MAX_DROPS[K])]
        at = [i for i, f in enumerate(fields) if f]
        assert len(at) == 1
        i, field = at[0], fields[at[0]]
        assert field & 63 == 0 or (i > 0 and fields[i - 1] == 0)
        with pytest.raises(ValueError):
            H.joint_signal_of_key(letters, sentinel)
    # exhaustively over short rows: no molecule's key is a sentinel
    frames, max_start = {1: (8, 4), 2: (5, 3), 3: (4, 2), 4: (3, 2)}[K]
    n = 0
    for rows in _short_rows(K, frames, max_start):
        kind, key = H.classify_joint_rows(rows)
        assert kind != H.ROW_SIGNAL or key not in (H.EMPTY, H.NEVER)
        n += 1
    assert n >= 400
    # and at the cycles the sentinels' bits would spell: drops at cycles 1 and 2 of every channel
    for k in range(K):
        for c in (1, 2):
            rows = [[0] * 4 for _ in range(K)]
            rows[k][:c] = [1] * c
            kind, key = H.classify_joint_rows(rows)
            assert kind == H.ROW_SIGNAL and key not in (H.EMPTY, H.NEVER)


def test_drops_at_one_cycle_stand_in_channel_order():
    rows = [[1, 0, 0], [2, 0, 0], [1, 0, 0]]
    kind, key = H.classify_joint_rows(rows)
    B = H.JOINT_DROP_BITS[3]
    fields = [(key >> (4 + B * i)) & 255 for i in range(6)]
    assert fields == [1 | 0 << 6, 1 | 1 << 6, 1 | 1 << 6, 1 | 2 << 6, 0, 0]
    assert (key & 15, (key >> 56) & 15, (key >> 60) & 15) == (1, 2, 1)
    assert H.joint_signal_of_key(LETTERS[3], key)[0] == (("C", 1), ("D", 1), ("D", 1), ("K", 1))
    # a later cycle of a lower channel stands after an earlier cycle of a higher one
    kind, key = H.classify_joint_rows([[1, 1, 0], [1, 0, 0]])
    assert H.joint_signal_of_key(LETTERS[2], key)[0] == (("K", 1), ("C", 2))
    # drops out of order, or of a letter the sweep does not have, have no key
    assert H.joint_key_of_signal(LETTERS[2], ((("C", 2), ("K", 1)), (True, True), (1, 1))) is None
    assert H.joint_key_of_signal(LETTERS[2], ((("K", 1), ("C", 1)), (True, True), (1, 1))) is None
    assert H.joint_key_of_signal(LETTERS[2], ((("D", 1),), (True, True), (1, 0))) is None
    assert H.joint_key_of_signal(LETTERS[2], ((("C", 1),), (False, True), (1, 0))) is None         # zeros must follow
    assert H.joint_key_of_signal(LETTERS[2], ((("C", 1),), (True, True), (1,))) is None
    assert H.joint_key_of_signal(LETTERS[2], ((("C", 64),), (True, True), (1, 0))) is None


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_capacity_boundaries(K):
    D = H.JOINT_MAX_DROPS[K]
    for k in range(K):
        # D(K) drops are keyed, D(K) + 1 are not: all in channel k, and spread over the channels
        for rows in (_drops_in(K, k, D), _spread(K, D)):
            kind, key = H.classify_joint_rows(rows)
            assert kind == H.ROW_SIGNAL and len(H.joint_signal_of_key(LETTERS[K], key)[0]) == D
        for rows in (_drops_in(K, k, D + 1), _spread(K, D + 1)):
            assert H.classify_joint_rows(rows) == (H.ROW_UNKEYED, None)
        # a start of 15 is keyed, of 16 is not
        rows = [[0, 0] for _ in range(K)]
        rows[k] = [15, 15]
        kind, key = H.classify_joint_rows(rows)
        assert kind == H.ROW_SIGNAL and H.joint_signal_of_key(LETTERS[K], key)[2][k] == 15
        rows[k] = [16, 16]
        assert H.classify_joint_rows(rows) == (H.ROW_UNKEYED, None)
    with pytest.raises(ValueError):
        H.classify_joint_rows([[0] * 65] * K)
    with pytest.raises(ValueError):
        H.classify_joint_rows([[0]] * 5)


def _drops_in(K, k, n):
    rows = [[0, 0, 0] for _ in range(K)]
    rows[k] = [n, n // 2, 0]
    return rows


def _spread(K, n):
    rows = [[n // K + (1 if k < n % K else 0)] for k in range(K)]
    return [[r[0], r[0], 0] for r in rows]


@pytest.mark.parametrize("K", [2, 3, 4])
def test_an_upstep_in_any_one_channel_gives_none(K):
    for k in range(K):
        rows = [[2, 1, 1, 0] for _ in range(K)]
        rows[k] = [2, 1, 2, 0]
        assert H.classify_joint_rows(rows) == (H.ROW_NONE, None)
        rows[k] = [17, 18]                                                              # an upstep goes before a missing key
        assert H.classify_joint_rows([r[:2] for r in rows]) == (H.ROW_NONE, None)


# ---- the tally ----

@pytest.mark.parametrize("shape, fixed", [(SHAPE2, FIXED2), (SHAPE3, FIXED3)], ids=["GAKCAK_KC", "three_letters"])
def test_tally_is_joint_signals_of_records(shape, fixed):
    rec = PS.multilabel_records(*shape, 200, seed=4, host=True, p=0.9, b=0.1, u=0.2, **fixed)
    exp = PS.joint_signals_of_records(rec)
    assert len(exp) > 10
    lit = (rec["counts"][:, :, 0] != 0).any(axis=0)
    (table,), none, unkeyed = H.tally_joint_rows(rec["counts"], np.zeros(200, np.int32), lit, 1)
    assert (none, unkeyed) == ([0], [0])
    assert {H.joint_signal_of_key(rec["labels"], k): n for k, n in table.items()} == exp
    # points and the mask
    points = np.arange(200, dtype=np.int32) % 3
    points[::7] = 5                                                                   # outside its range: left out
    tables, none, unkeyed = H.tally_joint_rows(rec["counts"], points, None, 3)
    for k in range(3):
        exp_k = {}
        for i in np.flatnonzero(points == k).tolist():
            s = PS.joint_signal(rec["labels"], rec["counts"][:, i].tolist())
            exp_k[s] = exp_k.get(s, 0) + 1
        assert {H.joint_signal_of_key(rec["labels"], x): n for x, n in tables[k].items()} == exp_k, k


# ---- the key table ----

def test_key_table_on_joint_signals():
    L = LETTERS[2]
    sigs = {
        "none": ((), (True, True), (0, 0)),                                           # drop-free, all dark: z, counts as one drop
        "rest": ((), (False, True), (1, 0)),                                          # drop-free, a dye stays: not z
        "one": ((("C", 2),), (True, True), (1, 0)),
        "two": ((("C", 2), ("K", 2)), (True, True), (1, 1)),                          # one cycle, two letters: single
        "twice": ((("K", 3), ("K", 3)), (True, True), (0, 2)),                        # a (letter, cycle) pair twice: multidrop
        "three": ((("C", 1), ("K", 2), ("K", 4)), (True, True), (1, 2)),
        "half": ((("C", 1), ("K", 2)), (True, False), (1, 2)),                        # K keeps a dye: not z
        "unkeyed": ((("C", 1),) * 9, (True, True), (9, 0)),
    }
    order = H.ordered_signals(sigs.values(), L)
    keyed = [s for s in order if H.joint_key_of_signal(L, s) is not None]
    assert order[-1] == sigs["unkeyed"] and len(keyed) == 7
    assert [H.joint_key_of_signal(L, s) for s in keyed] == sorted(H.joint_key_of_signal(L, s) for s in keyed)
    observed = {sigs["one"]: 5, sigs["twice"]: 7, sigs["half"]: 11, sigs["none"]: 2}
    names = {v: k for k, v in sigs.items()}

    def flags(**kw):
        t = H.key_table(observed, order, **kw)
        return ({names[s] for s, a in zip(order, t["admitted"]) if a}, {names[s] for s, h in zip(order, t["heatmap"]) if h},
                t["n_observed"])
    heat = {"none", "one", "two"}
    assert flags() == (heat, heat, 5 + 2)                                             # heatmap_only, zero_only, no multidrop
    assert flags(allow_multidrop=True) == (heat | {"twice"}, heat, 5 + 7 + 2)
    adm, h, n = flags(heatmap_only=False)
    assert adm == {"none", "one", "two", "three"} and h == heat and n == 7           # "unkeyed" repeats (C, 1): a multidrop
    adm, h, n = flags(heatmap_only=False, zero_only=False, allow_multidrop=True)
    assert adm == set(sigs) and h == heat and n == 25
    adm, h, n = flags(zero_only=False)
    assert adm == {"none", "rest", "one", "two", "half"} and n == 5 + 11 + 2
    adm, h, n = flags(exclude_signals={sigs["one"]}, select_signals={sigs["one"], sigs["two"]})
    assert adm == {"two"}
    t = H.key_table(observed, order)
    assert t["observed"].tolist() == [observed.get(s, 0) for s in order]
    assert t["in_observed"].tolist() == [int(s in observed) for s in order]
    # one-letter signals read as before
    one = [((("A", 2),), True, 1), (H.NO_DROPS, False, 1), ((("A", 2), ("A", 2)), True, 2)]
    t = H.key_table({one[0]: 3}, H.ordered_signals(one))
    assert sorted(zip(t["admitted"].tolist(), t["heatmap"].tolist())) == [(0, 0), (0, 0), (1, 1)]


def test_joint_split_heatmap():
    before, after = SW.joint_split_heatmap(LETTERS[2], 3, 2)
    every = before + after
    assert len(every) == 6 + 15 and len(set(every)) == 21
    assert all(H.joint_key_of_signal(LETTERS[2], s) is not None and H.signal_flags(s) == (True, len(s[0]), True) for s in every)
    assert set(before) == {s for s in every if s[0][-1][1] < 2} and len(before) == 2 + 1
    assert SW.joint_split_heatmap(LETTERS[2], 3, 0)[0] == ()


# ---- the host sweep ----

def _loop(shape, points, n, fixed, seed, stride=0, first=0, fit=True):
    """{point: (signals, molecular, total, none)} by a per-point loop of multilabel_records(host=True) and the restated fit."""
    out = {}
    for k, (p, b, u) in enumerate(points):
        rec = PS.multilabel_records(*shape, n, seed=seed, first_molecule=first + k * stride, host=True, p=p, b=b, u=u, **fixed)
        letters, K = rec["labels"], len(rec["labels"])
        mol, sig, total, none = {}, {}, 0, 0
        for i in range(n):
            rows = rec["counts"][:, i].tolist()
            if not any(rec["category"][c][i] for c in range(K)):
                continue
            total += 1
            s = PS.joint_signal(letters, rows)
            mol[s] = mol.get(s, 0) + 1
            if not fit:
                continue
            best = []
            for c, letter in enumerate(letters):
                if not rec["category"][c][i]:
                    best.append([0] * len(rows[c]))
                    continue
                beta = fixed["beta"][letter] if isinstance(fixed["beta"], dict) else fixed["beta"]
                sigma = fixed["beta_sigma"][letter] if isinstance(fixed["beta_sigma"], dict) else fixed["beta_sigma"]
                f = _host_lognormal.intensities_to_signal(rec["intensity"][c][i].tolist(), sigma, 5, True, 3,
                                                          tuple(x != 0 for x in rows[c]), _tracks.log_fluor_means(beta, DDIF, 5))
                best.append(None if f[2] is None else list(f[2]))
            if any(b is None for b in best):
                none += 1
                continue
            if any(y > x for b in best for x, y in zip(b, b[1:])):
                continue                                                                # (a fit with an upstep has no signal)
            s = PS.joint_signal(letters, best)
            sig[s] = sig.get(s, 0) + 1
        out[(p, b, u)] = (sig if fit else None, mol, total, none if fit else None)
    return out


@pytest.mark.parametrize("stride", [0, 1000])
def test_host_sweep_is_the_per_point_loop(stride):
    got = SW.joint_sweep_records(*SHAPE2, GRID4, 64, seed=5, first_molecule=3, molecule_stride=stride, host=True, **QUENCH, **FIXED2)
    exp = _loop(SHAPE2, GRID4, 64, FIXED2, 5, stride, 3)
    assert got["points"] == GRID4 and got["labels"] == ("C", "K")
    for key in GRID4:
        sig, mol, total, none = exp[key]
        assert got["all_simulations"][key] == (sig, mol), key
        assert (got["total_count"][key], got["none_count"][key]) == (total, none), key
        assert sum(mol.values()) == total and total > 30 and len(mol) > 5 and len(sig) > 3
    unfitted = SW.joint_sweep_records(*SHAPE2, GRID4, 64, seed=5, first_molecule=3, molecule_stride=stride, fit=False, host=True, **QUENCH, **FIXED2)
    for key in GRID4:
        assert unfitted["all_simulations"][key] == (None, exp[key][1]) and unfitted["none_count"][key] is None


def test_scores_of_a_joint_sweep_on_the_host():
    sweep = SW.joint_sweep_records(*SHAPE2, GRID4, 64, seed=5, host=True, **QUENCH, **FIXED2)
    observed = dict(sweep["all_simulations"][GRID4[2]][0])
    scores = SW.score_records(observed, sweep, metric="my_euclidean", heatmap_only=False, zero_only=False, allow_multidrop=True,
                              host=True)
    point, result, factor, contributions = SW.best_point(scores)
    assert point == GRID4[2] and result == 0.0 and set(contributions) == set(observed)
    assert all(r > 0.0 for k, (r, _) in scores.items() if k != GRID4[2])
    inc = SW.incompatibility_records(observed, sweep, SW.joint_split_heatmap(("C", "K"), 5, 0)[1][:12], metric="my_euclidean",
                                     heatmap_normalize_counts=True, host=True, on_error="none")
    assert len(inc["pairs"]) == 66 and inc["scores"]
    diag = SW.match_diagnostic(sweep, observed, "my_euclidean", False, False, True, True, True, False, None, 0.1, 2, None, False, 1, 0,
                               4, host=True, on_error="none")
    assert diag["optimal_pbu"] in GRID4 and diag["tables"] is None and diag["labels"] == ("C", "K")
    assert diag["exclude_signals"] == set(SW.joint_split_heatmap(("C", "K"), 5, 2)[0])
    with pytest.raises(NotImplementedError, match="one label letter"):
        SW.single_drops_table(observed, 1, 4, 0)
    with pytest.raises(NotImplementedError, match="one label letter"):
        SW.double_drops_table(observed, 1, 4, 0)


def test_joint_signals_of_fits_on_the_host():
    best = np.zeros((2, 5, 4), np.uint8)
    best[0] = [[1, 1, 0, 0], [2, 1, 1, 0], [9, 9, 9, 9], [1, 0, 0, 0], [1, 1, 0, 0]]
    best[1] = [[1, 0, 0, 0], [7, 7, 7, 7], [1, 1, 1, 0], [1, 1, 0, 0], [1, 0, 0, 0]]
    category = np.array([[1, 3, 0, 1, 1], [1, 0, 7, 3, 1]], np.uint64)                 # track 1: K dark; track 2: C dark
    found = np.array([[1, 1, 0, 1, 1], [1, 0, 1, 0, 1]], np.uint8)                     # track 3: K lit and not found
    got = SW.joint_signals_of_fits(("C", "K"), best, found, category, host=True)
    assert got == {((("K", 1), ("C", 2)), (True, True), (1, 1)): 2,
                   ((("C", 1), ("C", 3)), (True, True), (2, 0)): 1,                    # the dark channel is a row of zeros
                   ((("K", 3),), (True, True), (0, 1)): 1}
    assert SW.joint_signals_of_fits(("C", "K"), best[:, :0], found[:, :0], category[:, :0], host=True) == {}


def test_one_letter_sweeps_still_refuse_several_letters():
    kw = dict(p=0.9, b=0.1, u=0.1, s=0.1, sc=3, s2=0.05, beta=7e4, beta_sigma=0.2)
    with pytest.raises(NotImplementedError, match="one label"):
        SW.sweep_records("GAKC", "KC", 1, 1, [(0.9, 0.1, 0.1)], 4, host=True, **{k: v for k, v in kw.items() if k not in "pbu"})
    with pytest.raises(NotImplementedError, match="at most 4 label letters"):
        SW.joint_sweep_records("GAKCDE", "GAKCD", 1, 1, [(0.9, 0.1, 0.1)], 4, host=True, s=0.1, sc=3, s2=0.05, beta=7e4, beta_sigma=0.2)


def test_the_library_exports_the_new_entries():
    from fluorosequencingimageanalysis_amd import _native as N
    assert {"fsq_signal_tally_joint", "fsq_peptide_simulate_labels_points"} <= set(NS.EXPORTED)
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in ("fsq_signal_tally_joint", "fsq_peptide_simulate_labels_points"):
        assert getattr(lib, name) is not None


def test_command_line_on_the_host(tmp_path, capsys):
    import pickle
    from fluorosequencingimageanalysis_amd import sweep_peptide
    truth = SW.joint_sweep_records("GAKCAK", "KC", 1, 4, [(0.95, 0.1, 0.2)], 64, seed=5, host=True, s=0.3, sc=3, s2=0.1,
                                   beta={"K": 70000.0, "C": 30000.0}, beta_sigma=0.2, ddif=DDIF, superdye_rate=0.0, superdye_factor=1.0,
                                   **QUENCH)
    observed = truth["all_simulations"][(0.95, 0.1, 0.2)][0]
    with open(tmp_path / "joint.pkl", "wb") as f:
        pickle.dump(observed, f, protocol=2)
    argv = ["GAKCAK", "KC", "--observed", str(tmp_path / "joint.pkl"), "--edman_efficiency", "0.8:0.95:2", "--dye_destruction",
            "0.05:0.15:2", "--dud_dyes", "0.2", "-N", "64", "-m", "2", "-o", "1", "-e", "4", "--seed", "5", "--fluor_intensity",
            "K=70000,C=30000", "--all_signals", "--nonzero_signals", "--score_multidrop", "--host", "--output_directory", str(tmp_path)]
    out = pickle.load(open(sweep_peptide.main(argv), "rb"))
    assert out["labels"] == ("C", "K") and len(out["points"]) == 4 and out["args"].fluor_intensity == {"K": 70000.0, "C": 30000.0}
    assert all(H.is_joint(s) for sims in out["all_simulations"].values() for d in sims for s in d)
    assert out["best_point"][0] in out["points"] and out["best_point"][1] is not None
    assert "Best point" in capsys.readouterr().out
    # per-letter values need several letters; one letter keeps its plain floats
    with pytest.raises(SystemExit):
        sweep_peptide.main(["GAKAK", "K", "--observed", str(tmp_path / "joint.pkl"), "--fluor_intensity", "K=70000", "--host"])
    assert sweep_peptide.build_parser().parse_args(["GAK", "K", "--observed", "x"]).fluor_intensity == 70000
    assert sweep_peptide.per_letter("0.25") == 0.25 and sweep_peptide.per_letter("K=1,C=2.5") == {"K": 1.0, "C": 2.5}


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_keys_decoded_in_bulk_are_the_keys_decoded_one_by_one(K):
    rng = np.random.default_rng(40 + K)
    rows = random_molecules(rng, K, 400, 8, max_start=3 if K < 3 else 1, upstep_rate=0.0)
    (table,), _, _ = H.tally_joint_rows(rows, np.zeros(400, np.int32), None, 1)
    keys = sorted(table) + [H.classify_joint_rows(r)[1] for r, kind, _ in hand_rows(K) if kind == H.ROW_SIGNAL]
    got = H.joint_signals_of_keys(LETTERS[K], np.array(keys, np.uint64))
    assert got == [H.joint_signal_of_key(LETTERS[K], k) for k in keys] and len(keys) > 20
    assert H.joint_signals_of_keys(LETTERS[K], np.array(keys, np.uint64).view(np.int64)) == got
    assert H.joint_signals_of_keys(LETTERS[K], np.zeros(0, np.uint64)) == []
    assert all(type(x) is bool for s in got for x in s[1]) and all(type(x) is int for s in got for x in s[2])
