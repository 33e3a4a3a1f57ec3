"""The lognormal fit by exact dynamic programme on the GPU (include/fsq_lognormal_dp.h): bit for bit against the reference's
recorded outputs with and without upsteps (tests/golden/lognormal_upsteps.npz, lognormal_tracks.npz), against the enumerating
kernel on the device, and against the plain Python twin (_host_lognormal_dp.py).  Every output tensor starts as a byte pattern.
Nothing is compared with a tolerance."""
import contextlib

import numpy as np
import pytest

from fluorosequencingimageanalysis_amd import _host_lognormal_dp as D
from _lognormal_cases import means_for, random_batch, single_cases
from _lognormal_chain_cases import same_bits, table
from _lognormal_dp_cases import rising_batch, twin_records, upstep_cases
from _util import _bits

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _prefilled():
    """Every output tensor the binding allocates starts as a byte pattern, not as zeros: what the kernel leaves unwritten shows."""
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


def _words(C):
    return [sum(1 << f for f, c in enumerate(cat) if c) for cat in C]


def _fit(I, C, means, sigma, m, multi, dev, solver='dp', upsteps=False, budget=1 << 22, max_frames=None, lens=None):
    """lognormal_device on host rows, outputs pre-filled; returns host arrays."""
    import torch
    from fluorosequencingimageanalysis_amd import lognormal as LN
    lens = [len(v) for v in I] if lens is None else lens
    F = max_frames or max(max(len(v) for v in I), 1)
    rows = np.zeros((len(I), F))
    for i, v in enumerate(I):
        rows[i, :len(v)] = v
    with _prefilled():
        out = LN.lognormal_device(torch.from_numpy(rows).cuda(), torch.from_numpy(np.array(_words(C), np.uint64).view(np.int64)).cuda(),
                                  torch.from_numpy(np.array(lens, np.int32)).cuda(), means, sigma, m, multi, dev, budget,
                                  solver=solver, allow_upsteps=upsteps)
        return {k: v.cpu().numpy() for k, v in out.items()}


def _same(h, e, what=None, count=True):
    """Two fits' arrays, every element of every row."""
    assert h["status"].tolist() == e["status"].tolist(), what
    if count:
        assert h["n_surviving"].tolist() == e["n_surviving"].tolist(), what
    assert np.array_equal(h["best_seq"], e["best_seq"]), what
    assert np.array_equal(_bits(h["best_score"]), _bits(e["best_score"])), what
    assert np.array_equal(_bits(h["frame_score"]), _bits(e["frame_score"])), what


def _three_ways(I, C, means, sigma, m, multi, dev, what):
    """dp against enumerate on the device and against the twin; then upsteps against the twin.  Returns the twin's two fits."""
    F = max(len(v) for v in I)
    e = twin_records(D, I, C, means, sigma, m, multi, dev, False, F)
    h = _fit(I, C, means, sigma, m, multi, dev)
    _same(h, e, (what, "twin"))
    k = _fit(I, C, means, sigma, m, multi, dev, solver='enumerate')
    assert (k["status"] < 2).all(), what
    _same(h, k, (what, "enumerate"))
    u = twin_records(D, I, C, means, sigma, m, multi, dev, True, F)
    _same(_fit(I, C, means, sigma, m, multi, dev, upsteps=True), u, (what, "upsteps"))
    return e, u


def test_both_goldens_through_lognormal_records():
    """Every recorded case of both goldens, alone in a launch: the reference's own outputs, bit for bit."""
    from fluorosequencingimageanalysis_amd import lognormal as LN
    for ups, cases in ((False, single_cases()), (True, upstep_cases())):
        for i, c in enumerate(cases):
            T = c["T"]
            with _prefilled():
                h = LN.lognormal_records([c["intensity"]], [c["category"]], c["means"], c["beta_sigma"], c["max_possible"], c["multidrop"],
                                         c["max_deviation"], budget=1, solver='dp', allow_upsteps=ups)
            assert h["n_surviving"][0] == c["n_surviving"] and h["best_seq"].shape == (1, T), (ups, i, c["name"])
            if c["best_seq"] is None:
                assert h["status"][0] == 1 and h["best_score"][0] == -1.0, (ups, i, c["name"])
                assert not h["best_seq"][0].any() and not h["frame_score"][0].any(), (ups, i)
            else:
                assert h["status"][0] == 0, (ups, i, c["name"])
                assert tuple(h["best_seq"][0].tolist()) == c["best_seq"], (ups, i, c["name"])
                assert _bits(h["best_score"][:1])[0] == _bits([c["best_score"]])[0], (ups, i, c["name"])
                assert np.array_equal(_bits(h["frame_score"][0]), _bits(c["frame_score"])), (ups, i, c["name"])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_batches_of_ragged_lengths(n):
    I, C = random_batch(500 + n, n)
    means = means_for(10000.0, 5)
    e, _ = _three_ways(I, C, means, 0.2, 5, True, 3, n)
    assert n < 60 or (0.1 * n < (e["status"] == 0).sum() < 0.95 * n and {len(v) for v in I} == set(range(1, 14)))
    # tracks whose counts rise: the winner of the upstep fit steps up
    multi = n % 2 == 0
    I, C = rising_batch(900 + n, n, t_lo=1 if multi else 2)        # (one frame without multi-drop: the reference's max() of nothing)
    _, u = _three_ways(I, C, means, 0.2, 5, multi, 3, (n, "rising"))
    ups = sum(1 for s, seq, T in zip(u["status"], u["best_seq"], [len(v) for v in I]) if s == 0 and (np.diff(seq[:T].astype(int)) > 0).any())
    assert n < 60 or ups > 0.1 * n


SHAPES = [  # (T, max_possible, max_deviation, noise): the deviation rule narrow where the enumerating kernel could not follow
    (1, 1, 3, 0.2), (2, 1, 1e9, 0.2), (1, 15, 1e9, 0.2), (2, 15, 3, 0.2), (7, 15, 3, 0.2), (63, 1, 1e9, 0.2), (64, 1, 3, 0.2),
    (63, 5, 2.0, 0.04), (64, 5, 2.0, 0.04), (64, 15, 0.5, 0.02),
]


@pytest.mark.parametrize("T,m,dev,noise", SHAPES, ids=["T%d_m%d" % s[:2] for s in SHAPES])
def test_shapes_at_the_limits(T, m, dev, noise):
    rng = np.random.default_rng(64 * T + m)
    means = means_for(10000.0, m)
    I, C = [], []
    for k in range(4):
        seq = sorted(rng.integers(1, m + 1, T).tolist(), reverse=True)
        if k == 3:
            seq = seq[:T // 2] + [0] * (T - T // 2)                # an ON prefix
        I.append([float(int(np.exp(rng.normal(means[s - 1], noise)))) if s > 0 else float(rng.normal(40.0, 300.0)) for s in seq])
        C.append(tuple(s > 0 for s in seq))
    for multi in (True, False):
        if T == 1 and not multi:
            continue
        e, _ = _three_ways(I, C, means, 0.2, m, multi, dev, (T, m, multi))
        assert (e["status"] == 0).any()


def test_over_budget_track_is_found_and_its_neighbours_are_exact():
    """One 64-frame all-ON track at max_possible 15 with every count from 1 admissible: C(78, 14) sequences without upsteps,
    15^64 (a saturated count) with."""
    import math
    rng = np.random.default_rng(6415)
    means = means_for(10000.0, 15)
    seq = sorted(rng.integers(1, 16, 64).tolist(), reverse=True)
    long_track = [float(int(np.exp(rng.normal(means[s - 1], 0.2)))) for s in seq]
    I = [[9000.0, 8000.0], long_track, [15000.0, 9000.0, 9500.0], [7000.0]]
    C = [(True,) * len(v) for v in I]
    k = _fit(I, C, means, 0.2, 15, True, 1e9, solver='enumerate')
    assert k["status"].tolist() == [0, 2, 0, 0] and k["n_surviving"][1] == math.comb(78, 14) and k["best_score"][1] == -1.0
    found = {}
    for ups in (False, True):
        e = twin_records(D, I, C, means, 0.2, 15, True, 1e9, ups, 64)
        assert e["status"].tolist() == [0, 0, 0, 0] and e["n_surviving"][1] == (1 << 59 if ups else math.comb(78, 14)) and e["best_score"][1] > 0
        h = _fit(I, C, means, 0.2, 15, True, 1e9, upsteps=ups, budget=1)
        _same(h, e, ups)
        found[ups] = h
        if not ups:
            for t in (0, 2, 3):
                assert h["n_surviving"][t] == k["n_surviving"][t] and np.array_equal(h["best_seq"][t], k["best_seq"][t])
                assert _bits(h["best_score"][t:t + 1])[0] == _bits(k["best_score"][t:t + 1])[0]
            assert (np.diff(h["best_seq"][1].astype(int)) <= 0).all()
    from fluorosequencingimageanalysis_amd import lognormal as LN
    phot = {"ch1": {3: {(10 + t, 20): (C[t], tuple(I[t]), t + 1) for t in range(4)}}}
    q = (0.0,) + (0.3,) * 16
    with pytest.raises(NotImplementedError, match="more than the budget"):
        LN.photometries_lognormal_fit(phot, 10000.0, 0.2, 15, max_deviation=1e9, quench_factors=q)
    signals, total, none_count, info = LN.photometries_lognormal_fit(phot, 10000.0, 0.2, 15, max_deviation=1e9, quench_factors=q, solver='dp')
    assert total == 4 and none_count == 0 and sum(signals.values()) == 4
    assert [f[9] for f in info] == [tuple(found[False]["best_seq"][t, :len(I[t])].tolist()) for t in range(4)]


def test_tiny_densities_make_the_bit_search_run():
    """Densities at and below 1e-300 (subnormal thresholds, quotients that overflow or underflow) and all-underflow tracks."""
    means = means_for(10000.0, 5)
    rng = np.random.default_rng(300)
    dim = [4.8, 5.0, 5.2, 5.5, 6.0]                                # z = -37 .. -38.2 at count 1: densities 1e-299 .. 1e-317
    I, C = [], []
    for k in range(64):
        T = int(rng.integers(1, 9))
        v = [float(int(np.exp(rng.normal(means[int(rng.integers(0, 3))], 0.3)))) for _ in range(T)]
        if k % 8 == 0:
            v = [1.0] * T                                          # all-underflow
        else:
            for f in rng.choice(T, min(T, 2 if k % 8 < 3 else 1), replace=False):      # two dim frames: their product is 0
                v[int(f)] = float(rng.choice(dim))
        I.append(v)
        C.append((True,) * T)
    for multi in (True, False):
        J, K = ([v for v in I if len(v) > 1], [c for c in C if len(c) > 1]) if not multi else (I, C)
        e, u = _three_ways(J, K, means, 0.2, 5, multi, 1e9, multi)
        tiny = (e["frame_score"] > 0) & (e["frame_score"] < 1e-300)
        assert tiny.sum() >= 20 and (e["best_score"] == 0.0).sum() >= 8 and ((e["best_score"] > 0) & (e["best_score"] < 1e-300)).sum() >= 5


def test_invalid_lengths():
    means = means_for(10000.0, 5)
    I = [[9000.0, 8000.0, 50.0], [9000.0, 8000.0, 50.0], [9000.0, 8000.0, 50.0], [9000.0, 8000.0, 50.0]]
    C = [(True, True, False)] * 4
    for ups in (False, True):
        h = _fit(I, C, means, 0.2, 5, True, 3, upsteps=ups, lens=[3, 0, 4, -1])
        assert h["status"].tolist() == [0, 3, 3, 3] and h["best_seq"][0].tolist() == [1, 1, 0]
        assert h["best_score"][1:].tolist() == [-1.0] * 3 and h["n_surviving"][1:].tolist() == [0] * 3
        assert not h["best_seq"][1:].any() and not h["frame_score"][1:].any()
    from fluorosequencingimageanalysis_amd import lognormal as LN
    with pytest.raises(ValueError, match="invalid length"):
        LN._fit_tuples(dict(h, lengths=np.array([3, 0, 4, -1], np.int32)), 5, lambda i: "track %d" % i)


def test_chain_device_with_either_solver():
    """65 tracks in 3 fields: every output of chain_device(solver='dp') equals solver='enumerate'."""
    import torch
    from fluorosequencingimageanalysis_amd import lognormal as LN
    rows, cats, fields = table(565, 65, 6, [20, 25, 20])
    seg_off = np.array([0, 20, 45, 65], np.int64)
    d = [torch.from_numpy(rows).cuda(), torch.from_numpy(cats.view(np.int64)).cuda(), torch.from_numpy(seg_off).cuda()]
    res = {}
    for solver in ("enumerate", "dp"):
        with _prefilled():
            res[solver] = LN.chain_device(d[0], d[1], d[2], None, 0.2, solver=solver, budget=1 << 22 if solver == "enumerate" else 1)
    a, b = res["enumerate"], res["dp"]
    assert sorted(a) == sorted(b)
    for key in a:
        if isinstance(a[key], dict):
            assert sorted(a[key]) == sorted(b[key])
            for name in a[key]:
                same_bits(a[key][name].cpu().numpy(), b[key][name].cpu().numpy(), (key, name))
        elif torch.is_tensor(a[key]):
            same_bits(a[key].cpu().numpy(), b[key].cpu().numpy(), key)
        else:
            same_bits([a[key]], [b[key]], key)
    assert (a["fit1"]["status"] == 0).any() and (a["fit1"]["n_surviving"] > 1).any()
    assert LN.tally_device(a["fit1"]) == LN.tally_device(b["fit1"])
