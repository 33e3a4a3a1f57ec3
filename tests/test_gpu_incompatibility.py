"""match_diagnostic's incompatibility loop on the GPU (fsq_signal_pair_best, fsq_signal_pair_extremes): the device against the
NumPy twin bit for bit on pre-filled outputs (every NaN one pattern), the tie rule across lanes, the reference's recorded loop
through incompatibility_records, the complete 63-cycle list, both forms of a sweep as the source, and the argument checks."""
import contextlib
import ctypes
import itertools

import numpy as np
import pytest

from fluorosequencingimageanalysis_amd import _host_signal_sweep as H
from _incompatibility_cases import OUTPUTS, assert_same_outputs, case, case_names, runs, same_bits, synthetic

pytestmark = pytest.mark.gpu

ROWS = {2: [0, 3], 3: [0, -1, 3], 10: [0, 3, -1, 7, 2, 11, -1, 5, 1, 9]}


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


def _device(table, rows, fit, fit_total, metric, norm, cutoff, reverse):
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    with _prefilled():
        out = SW.pair_best_device(table, rows, torch.from_numpy(np.ascontiguousarray(fit)).cuda(),
                                  torch.from_numpy(np.ascontiguousarray(fit_total)).cuda(), metric, norm, cutoff, reverse)
        return {k: out[k].cpu().numpy() for k in OUTPUTS}


# ---- the pair kernel against the twin ----

@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("n_sel", [2, 3, 10])
def test_pair_best_is_the_twin_bit_for_bit(n_sel, P):
    """Ten metrics x the two normalisations x both orders x no cutoff and 3, on a count matrix with keys that are observed
    only, fit only, in neither, not admitted, observed as zero, and candidates in no dict (rows of -1)."""
    table, fit, fit_total = synthetic(12, P, 100 * n_sel + P)
    statuses = set()
    for metric in H.METRICS:
        for norm in (H.NORMALIZE_COUNTS, H.HEATMAP_NORMALIZE_COUNTS):
            for reverse, cutoff in itertools.product((False, True), (None, 3.0)):
                want = H.pair_best(table, ROWS[n_sel], fit, fit_total, metric, norm, cutoff, reverse)
                got = _device(table, ROWS[n_sel], fit, fit_total, metric, norm, cutoff, reverse)
                assert_same_outputs(got, want, (metric, norm, reverse, cutoff))
                statuses |= set(want["error_status"].tolist())
                assert n_sel < 10 or P < 63 or (want["best_point"] >= 0).any()
    assert 0 in statuses


def _tie_case(P, tied, reverse, empty_odd=False):
    """Three observed keys and a fourth in no dict; the best result of every pair stands at the points `tied`."""
    table, fit, fit_total = synthetic(4, P, 3)
    table["observed"][:] = (10, 20, 30, 0)
    table["in_observed"][:], table["admitted"][:] = (1, 1, 1, 0), 1
    k = np.arange(P)
    for r in range(3):
        fit[r] = table["observed"][r] + 5 + (k * (r + 3)) % 7
        fit[r, list(tied)] = table["observed"][r] + (50 if reverse else 1)
    fit[3] = 0
    if empty_odd:
        fit[:, 1::2] = 0                                                              # with a cutoff of 1: nothing pairs at odd points
    return table, fit, fit_total


@pytest.mark.parametrize("reverse", [False, True])
def test_ties_go_to_the_lowest_point_across_lanes_and_waves(reverse):
    rows = [0, 1, 2, 3, -1]                                                           # pairs (3, -1): no result at any point
    for tied, first in (((63, 64), 63), ((0, 129), 0), ((64, 128), 64), (range(130), 0)):
        table, fit, fit_total = _tie_case(130, tied, reverse)
        got = _device(table, rows, fit, fit_total, 'my_euclidean', 0, None, reverse)
        assert_same_outputs(got, H.pair_best(table, rows, fit, fit_total, 'my_euclidean', 0, None, reverse), (tied, reverse))
        assert got["best_point"].tolist() == [first] * 9 + [-1], tied
        assert np.isnan(got["result"][9]) and np.isnan(got["factor"][9]) and np.isnan(got["dist"][9]).all()
        assert np.isnan(got["dist"][[2, 3, 5, 6, 7, 8], 1]).all() and not np.isnan(got["dist"][[0, 1, 4]]).any()


@pytest.mark.parametrize("reverse", [False, True])
def test_points_without_a_result_between_points_with_one(reverse):
    """Odd points are EMPTY (neighbouring lanes differ); the best of the even ones is tied at 64 and 66."""
    table, fit, fit_total = _tie_case(130, (64, 66, 65, 1), reverse, empty_odd=True)
    rows = [0, 1, 2]
    want = H.pair_best(table, rows, fit, fit_total, 'my_chebyshev', H.NORMALIZE_COUNTS, 1.0, reverse)
    got = _device(table, rows, fit, fit_total, 'my_chebyshev', H.NORMALIZE_COUNTS, 1.0, reverse)
    assert_same_outputs(got, want, reverse)
    assert (got["best_point"] % 2 == 0).all()
    plain = _device(table, rows, fit, fit_total, 'my_euclidean', 0, 1.0, reverse)
    assert_same_outputs(plain, H.pair_best(table, rows, fit, fit_total, 'my_euclidean', 0, 1.0, reverse), reverse)
    assert plain["best_point"].tolist() == [64, 64, 64]


def test_errors_under_both_normalisations_are_the_twins():
    table, fit, fit_total = synthetic(12, 70, 5)
    fit[:, 66] = 0                                                                    # a heat-map total of zero at point 66
    table["n_observed"] = int(table["observed"].max())                                # a zero variance in the std metrics
    seen = set()
    for metric in H.METRICS:
        for norm in (H.NORMALIZE_COUNTS, H.HEATMAP_NORMALIZE_COUNTS):
            want = H.pair_best(table, ROWS[10], fit, fit_total, metric, norm, None, False)
            assert_same_outputs(_device(table, ROWS[10], fit, fit_total, metric, norm, None, False), want, (metric, norm))
            seen |= set(want["error_status"].tolist())
            if norm == H.HEATMAP_NORMALIZE_COUNTS and metric == 'my_euclidean':
                assert (want["error_point"] == 66).all() and (want["error_status"] == H.SCORE_DIVZERO).all()
    assert seen == {0, H.SCORE_DIVZERO, H.SCORE_DOMAIN}


# ---- the reference's recorded loop, and the records ----

@pytest.mark.parametrize("name", case_names())
def test_records_are_the_reference_loop_bit_for_bit(name):
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    observed, sweep, candidates, cutoff = case(name)
    pairs = list(itertools.combinations(candidates, 2))
    for metric, nc, hn, reverse, best, factor, dist, is_none in runs(name):
        kw = dict(num_cycles=4 if len(candidates) == 10 else 5, metric=metric, normalize_counts=nc,
                  heatmap_normalize_counts=hn, small_count_cutoff=cutoff, reverse_order=reverse)
        with _prefilled():
            rec = SW.incompatibility_records(observed, sweep, **kw)
        assert list(rec["pairs"]) == pairs
        for t, (point, d, nf) in enumerate(rec["pairs"].values()):
            what = (name, metric, nc, hn, reverse, t)
            if best[t] < 0:
                assert (point, d, nf) == (None, (None, None), None), what
                continue
            assert point == best[t] and same_bits(nf, factor[t]), what
            assert [x is None for x in d] == is_none[t].tolist(), what
            assert all(x is None or same_bits(x, dist[t][i]) for i, x in enumerate(d)), what
        assert rec["scores"] == SW.incompatibility_records(observed, sweep, host=True, pairs=False, **kw)["scores"]


def test_a_zero_heat_map_total_raises_or_counts_as_no_result():
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    observed, sweep, candidates, _ = case("cycles4")
    broken = {"points": sweep["points"], "all_simulations": dict(sweep["all_simulations"])}
    broken["all_simulations"][2] = ({H.signal_of_key(H.key_of(3, [1, 2, 3])): 5}, None)
    kw = dict(num_cycles=4, metric='my_euclidean', heatmap_normalize_counts=True)
    with _prefilled():
        out = SW.incompatibility_device(observed, broken, **kw)
    assert (out["error_point"].cpu().numpy() == 2).all() and (out["error_status"].cpu().numpy() == H.SCORE_DIVZERO).all()
    assert out["signals"] == candidates and out["points"] == sweep["points"]
    with pytest.raises(ZeroDivisionError, match=r"point 2\)"):
        SW.incompatibility_records(observed, broken, **kw)
    got = SW.incompatibility_records(observed, broken, on_error='none', **kw)
    assert got == SW.incompatibility_records(observed, broken, on_error='none', host=True, **kw)
    assert all(point != 2 for point, _, _ in got["pairs"].values())


# ---- the per-signal extremes ----

def _extremes(dist, n_sel, reverse):
    import torch
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    with _prefilled():
        score, n = SW.pair_extremes_device(torch.from_numpy(dist).cuda(), n_sel, reverse)
        return score.cpu().numpy(), n.cpu().numpy()


@pytest.mark.parametrize("n_sel", [2, 3, 10, 65, 66, 130])
def test_extremes_are_the_twins(n_sel):
    """65: a signal's 64 pairs fill one wavefront exactly.  Candidate 1 has no distance at all."""
    rng = np.random.default_rng(n_sel)
    dist = rng.random((n_sel * (n_sel - 1) // 2, 2))
    dist[rng.random(dist.shape) < 0.3] = np.nan
    for t, (i, j) in enumerate(itertools.combinations(range(n_sel), 2)):
        if 1 in (i, j):
            dist[t, (i, j).index(1)] = np.nan
    dist[:3] = dist[:3].round(1)                                                      # (equal distances)
    for reverse in (False, True):
        score, n = _extremes(dist, n_sel, reverse)
        want, want_n = H.pair_extremes(dist, n_sel, reverse)
        assert same_bits(score, want) and np.array_equal(n, want_n) and n.dtype == np.int32
        assert np.isnan(score[1]) and n[1] == 0 and (n_sel < 10 or n.max() > 0)


# ---- at size: the complete list of 63 cycles ----

def _vectorised(table, rows, fit, fit_total):
    """fsq_signal_pair_best's outputs for my_euclidean under the heat-map normalisation, in the plain order.  The factor does
    not depend on the pair there, so a key's term at a point is one number, computed by the twin's own per-term function; a
    pair's result is then the root of a two-term sum."""
    n_sel, P = len(rows), len(fit_total)
    heat_f, heat_s = H.heat_factors(table, fit, fit_total)
    assert (heat_s == H.SCORE_EMPTY).all()
    obs, in_obs, adm = (table[k].tolist() for k in ("observed", "in_observed", "admitted"))
    term, paired = np.zeros((n_sel, P)), np.zeros((n_sel, P), bool)
    for a, r in enumerate(np.asarray(rows).tolist()):
        for k in range(P):
            if r >= 0 and H.is_paired(adm[r], in_obs[r], obs[r], int(fit[r, k]), None):
                paired[a, k] = True
                term[a, k] = H.term(1, obs[r], int(fit[r, k]), float(heat_f[k]), table["n_observed"], int(fit_total[k]))[0]
    i, j = np.triu_indices(n_sel, 1)
    ok = paired[i] | paired[j]
    result = np.where(ok, np.sqrt(np.where(paired[i], term[i], 0.0) + np.where(paired[j], term[j], 0.0)), np.inf)
    best = np.where(ok.any(axis=1), result.argmin(axis=1), -1).astype(np.int32)      # (argmin: the first among equal ones)
    at = np.maximum(best, 0)
    pick = lambda m: np.where(best >= 0, m[np.arange(len(best)), at], np.nan)      # noqa: E731
    return {"best_point": best, "result": pick(result), "factor": np.where(best >= 0, heat_f[at], np.nan),
            "dist": np.stack([pick(np.where(paired[i], term[i], np.nan)), pick(np.where(paired[j], term[j], np.nan))], axis=1),
            "error_point": np.full(len(best), -1, np.int32), "error_status": np.zeros(len(best), np.int32)}


@pytest.mark.parametrize("n_sel", [2016, 2048])
def test_the_63_cycle_list_against_a_vectorised_expectation(n_sel):
    """2 016 candidates, 2 031 120 pairs, two points - and the cap of 2 048: the pair-index arithmetic and the grid bound.  The
    expectation is first held against the twin itself at 40 candidates."""
    from fluorosequencingimageanalysis_amd import _native_signal_sweep as NS, signal_sweep as SW
    P = 2
    assert len(SW.split_heatmap(63, 0)[1]) == 2016 and NS.MAX_SEL == 2048
    table, fit, fit_total = synthetic(2100, P, 63)
    rows = np.random.default_rng(63).permutation(2100)[:n_sel].astype(np.int32)
    rows[::97] = -1
    assert_same_outputs(_vectorised(table, rows[:40], fit, fit_total),
                        H.pair_best(table, rows[:40], fit, fit_total, 'my_euclidean', H.HEATMAP_NORMALIZE_COUNTS), "40 candidates")
    want = _vectorised(table, rows, fit, fit_total)
    assert (want["best_point"] == -1).any() and (want["best_point"] == 0).any() and (want["best_point"] == 1).any()
    got = _device(table, rows, fit, fit_total, 'my_euclidean', H.HEATMAP_NORMALIZE_COUNTS, None, False)
    assert_same_outputs(got, want, "63 cycles")
    score, n = _extremes(got["dist"], n_sel, False)
    want_score, want_n = H.pair_extremes(want["dist"], n_sel, False)
    assert same_bits(score, want_score) and np.array_equal(n, want_n) and 1000 < n.max() <= n_sel - 1


# ---- both forms of a sweep ----

def test_both_forms_of_a_sweep_give_the_same_tensors():
    from fluorosequencingimageanalysis_amd import signal_sweep as SW
    ddif = [0, 0.3] + [0.3] * 5
    grid = [(p, b, u) for p in (0.8, 0.95) for b in (0.05, 0.15) for u in (0.1, 0.4)]
    sweep = SW.sweep_device('GAKAGAKC', 'K', 2, 4, grid, 500, seed=21, first_molecule=3, quench_factors=ddif, s=0.1, sc=3, s2=0.05,
                            beta=70000.0, beta_sigma=0.2, ddif=ddif)
    records = SW.records_of_sweep(sweep)
    observed = dict(records["all_simulations"][grid[5]][0])
    for kw in (dict(metric='my_euclidean', heatmap_normalize_counts=True), dict(metric='log_rmsd', normalize_counts=True, molecular=True),
               dict(metric='naive', normalize_counts=True, reverse_order=True, small_count_cutoff=3)):
        with _prefilled():
            a = SW.incompatibility_device(observed, sweep, num_cycles=6, **kw)
            b = SW.incompatibility_device(observed, records, num_cycles=6, **kw)
        assert a["signals"] == b["signals"] == list(SW.split_heatmap(6, 0)[1]) and a["points"] == b["points"] == grid
        assert_same_outputs({k: a[k].cpu().numpy() for k in OUTPUTS}, {k: b[k].cpu().numpy() for k in OUTPUTS}, kw)
        assert same_bits(a["score"].cpu().numpy(), b["score"].cpu().numpy())
        assert np.array_equal(a["n_distances"].cpu().numpy(), b["n_distances"].cpu().numpy())
        host = SW.incompatibility_records(observed, records, num_cycles=6, host=True, **kw)
        assert SW.incompatibility_records(observed, sweep, num_cycles=6, **kw) == host and len(host["scores"]) > 10
    args = ('my_euclidean', False, False, True, True, True, False, None, 0.10, 0, 30.0, True, 3, 1, 4)
    d, h = SW.match_diagnostic(sweep, observed, *args), SW.match_diagnostic(records, observed, *args, host=True)
    assert d["optimal_pbu"] == grid[5] and all(np.array_equal(d["tables"][k], h["tables"][k]) for k in SW.TABLE_NAMES)
    assert all(d[k] == h[k] for k in d if k != "tables")


# ---- the argument checks ----

def test_invalid_arguments_leave_the_buffers_as_they_were():
    import torch
    from fluorosequencingimageanalysis_amd import _native as N, _native_signal_sweep as NS
    table, fit, fit_total = synthetic(12, 5, 9)
    dev = {k: torch.from_numpy(table[k]).cuda() for k in ("observed", "in_observed", "admitted")}
    d_fit, d_total = torch.from_numpy(fit).cuda(), torch.from_numpy(fit_total).cuda()
    prm = NS.FsqScoreParams()
    prm.n_observed, prm.metric, prm.normalization = table["n_observed"], 1, 0
    K = 10
    outs = [torch.full((K,), 0x5A5A5A5A, dtype=torch.int32).cuda(), torch.full((K,), 1.5, dtype=torch.float64).cuda(),
            torch.full((K,), 2.5, dtype=torch.float64).cuda(), torch.full((K, 2), 3.5, dtype=torch.float64).cuda(),
            torch.full((K,), 0x3C3C3C3C, dtype=torch.int32).cuda(), torch.full((K,), 0x1B1B1B1B, dtype=torch.int32).cuda()]
    before = [t.clone() for t in outs]

    kept = []

    def call(rows, n_keys=12, n_points=5, n_sel=None, metric=1):
        d_rows = torch.tensor(rows, dtype=torch.int32).cuda()
        kept.append(d_rows)
        prm.metric = metric
        return NS.lib().fsq_signal_pair_best(dev["observed"].data_ptr(), dev["in_observed"].data_ptr(), dev["admitted"].data_ptr(),
                                             d_fit.data_ptr(), d_total.data_ptr(), n_keys, n_points, ctypes.byref(prm), d_rows.data_ptr(),
                                             len(rows) if n_sel is None else n_sel, 0, None, None, *[t.data_ptr() for t in outs], None)
    for bad in (dict(rows=[0]), dict(rows=[0, 1], n_sel=1), dict(rows=[0, 1, 12, 3]), dict(rows=[0, -2, 2, 3]), dict(rows=[0, 1, 2], n_points=0),
                dict(rows=[0, 1, 2], n_sel=NS.MAX_SEL + 1), dict(rows=[0, 1, 2], metric=10)):
        assert call(**bad) == N.FSQ_EINVAL, bad
    prm.normalization = NS.HEATMAP_NORMALIZE_COUNTS                                   # the heat-map factors are then needed
    assert call([0, 1, 2]) == N.FSQ_EINVAL
    score, n = torch.full((5,), 4.5, dtype=torch.float64).cuda(), torch.full((5,), 0x2D2D2D2D, dtype=torch.int32).cuda()
    for n_sel in (1, NS.MAX_SEL + 1):
        assert NS.lib().fsq_signal_pair_extremes(outs[3].data_ptr(), n_sel, 0, score.data_ptr(), n.data_ptr(), None) == N.FSQ_EINVAL
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, before)) and bool((score == 4.5).all()) and bool((n == 0x2D2D2D2D).all())
    prm.normalization = 0
    assert call([0, 1, 2, 3, 11]) == N.FSQ_OK                                         # the same buffers, a valid call: all ten pairs written
    torch.cuda.synchronize()
    assert not any(bool((a == b).any()) for a, b in zip(outs[:4], before[:4]))
