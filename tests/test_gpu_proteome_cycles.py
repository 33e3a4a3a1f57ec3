"""fsq_proteome_project and the layer above it on the GPU against the NumPy twin, bit for bit: every output is an integer, so
there is no tolerance.  The golden's triples at every cycle count in both modes; a 64-pair layout with the all-ones key; 4 096
pairs that fold onto one slot; weight 1 against fsq_proteome_tally; more items than one pass of the grid, in both item orders;
launches of one mask against one launch of all; a table that is too small for one mask only; refused parameters, which leave
pre-filled tables as they were; merges; and the cycle curve of 40 synthetic proteins against host=True and, at its last point,
against the unprojected run."""
import numpy as np
import pytest

from fluorosequencingimageanalysis_amd import _host_proteome_mc as H
import _proteome_cycles_cases as C
import _proteome_mc_cases as MCC

pytestmark = pytest.mark.gpu

PPJ_ONE_PASS = 256 * 2048                      # kpm_project's grid (csrc/simulate/fsq_proteome_project.hip)


def _mc():
    from fluorosequencingimageanalysis_amd import MCsimlib as MC
    return MC


def _held(tables):
    key, protein, count, _ = _mc().pairs_device(tables)
    return key.cpu().numpy().view(np.uint64), protein.cpu().numpy(), count.cpu().numpy()


def _of_cycle(projection, i):
    return _held(_mc().cycle_tables(projection, i)["tables"])


def _check_every_cycle(records, cycles, **kw):
    MC = _mc()
    for mode in ("project", "within"):
        proj = MC.project_device(records, cycles, mode, **kw)
        masks = H.cycle_masks(records["layout"], cycles)
        assert proj["cycles"] == list(cycles) and np.array_equal(proj["masks"], masks)
        for i, mask in enumerate(masks.tolist()):
            assert C.same(_of_cycle(proj, i), H.project(C.triples(records), mask, mode)), (mode, cycles[i])
    return proj


@pytest.mark.parametrize("case", ["full", "gapped"])
def test_golden_triples_at_every_cycle_count(case):
    g = C.golden()[case]
    records = C.records_of(case)
    cycles = list(range(g["last_position"] + 2)) + [63, 1000]
    proj = _mc().project_device(records, cycles)
    for rec in g["projections"]:                                                    # the reference itself
        assert C.same(_of_cycle(proj, rec["cycles"]), C.leaves_as_triples(case, rec["leaves"])), rec["cycles"]
    _check_every_cycle(records, cycles)
    assert len(_of_cycle(proj, 0)[0]) == 0                                          # c = 0 empties
    for i in (g["last_position"], len(cycles) - 1):                                 # at and beyond the last position
        assert C.same(_of_cycle(proj, i), C.triples(records))
    got = _mc().projection_records(records, 4)
    assert C.same(C.triples(got), C.triples(_mc().projection_records(records, 4, host=True))) and got["names"] == records["names"]


def test_64_pair_layout_with_the_all_ones_key():
    records = C.random_records("wide", 3000, 21)
    assert records["key"][-1] == np.uint64(2**64 - 1) and records["layout"].n_bits == 64
    proj = _check_every_cycle(records, [0, 1, 2, 16, 31, 32, 33])
    assert 2**64 - 1 in _of_cycle(proj, 5)[0].tolist() and 2**64 - 1 not in _of_cycle(proj, 4)[0].tolist()   # (within: only at c >= 32)


def test_full_contention_onto_one_slot():
    records = C.contention_records()
    MC = _mc()
    for mask_major in (False, True):
        proj = MC.project_device(records, [1, 32], mask_major=mask_major)
        k, p, c = _of_cycle(proj, 0)
        assert k.tolist() == [1] and p.tolist() == [3] and c.tolist() == [int(records["count"].sum())] and c[0] > 2**32
        assert C.same(_of_cycle(proj, 1), C.triples(records))


def test_weight_one_under_the_all_ones_mask_is_the_tally():
    import torch
    MC = _mc()
    keys, proteins, sa, sb = MCC.tally_cases()["many"]                               # repeated rows, key 0 rows, the all-ones key
    k, p = torch.from_numpy(keys.view(np.int64)).cuda(), torch.from_numpy(proteins).cuda()
    a, b = MC.new_tables(sa, sb, "cuda"), MC.new_tables(sa, sb, "cuda")
    MC.tally_device(a, k, p)
    MC.project_into(b, k, p, None, torch.full((1,), -1, dtype=torch.int64, device="cuda"))
    MC.check_tables(b)
    want = H.tally(keys, proteins)
    assert C.same(_held(a), want) and C.same(_held(b), want)
    MC.tally_device(b, k, p)                                                        # fsq_proteome_tally goes on adding to it
    MC.check_tables(b)
    assert C.same(_held(b), (want[0], want[1], 2 * want[2]))


def test_more_items_than_one_pass_of_the_grid_and_both_orders():
    MC = _mc()
    records = C.random_records("wide", 40000, 22, n_proteins=300, exact=17500)
    cycles = list(range(30)) + [40]
    assert len(records["key"]) == 17500 and len(records["key"]) * len(cycles) == 542500 > PPJ_ONE_PASS
    want = [H.project(C.triples(records), m) for m in H.cycle_masks(records["layout"], cycles).tolist()]
    one = MC.project_device(records, cycles)
    other = MC.project_device(records, cycles, mask_major=True)
    single = MC.project_device(records, cycles, masks_per_launch=1)
    some = MC.project_device(records, cycles, masks_per_launch=7)
    for i in range(len(cycles)):
        for proj in (one, other, single, some):
            assert C.same(_of_cycle(proj, i), want[i]), cycles[i]
    assert len(want[0][0]) == 0 and records["count"].sum() == want[-1][2].sum()
    assert len(want[1][0]) < len(want[8][0]) < len(want[-1][0]) == 17500             # (shorter runs fold pairs together)


def _crowded():
    """20 keys over positions 1 .. 6 of the first acid that fold onto one key at c = 1 and onto two at c = 2."""
    L = C.layout("wide")
    k = np.array([1 | (i << 1) for i in range(1, 21)], np.uint64)
    return {"key": k, "protein": np.zeros(20, np.int32), "count": np.arange(1, 21, dtype=np.int64), "names": ["P0"], "layout": L}


def test_a_table_too_small_for_one_mask_only():
    import torch
    MC = _mc()
    records = _crowded()
    masks = H.cycle_masks(records["layout"], [1, 6, 2])
    up = lambda a: torch.from_numpy(a).cuda()                                       # noqa: E731
    for sa, sb, flag in ((8, 64, [[0, 0], [1, 0], [0, 0]]), (64, 8, [[0, 0], [0, 1], [0, 0]])):
        tables = MC.new_tables(sa, sb, "cuda", n_masks=3)
        MC.project_into(tables, up(records["key"].view(np.int64)), up(records["protein"]), up(records["count"]), up(masks.view(np.int64)))
        assert tables["overflow"].cpu().tolist() == flag
        proj = {"tables": tables, "names": records["names"], "layout": records["layout"], "cycles": [1, 6, 2]}
        for i in (0, 2):                                                            # the other masks stay exact
            assert C.same(_of_cycle(proj, i), H.project(C.triples(records), masks[i]))
        k, p, c = _of_cycle(proj, 1)                                                # what found a slot is exact
        assert len(k) == 8 and all(int(records["count"][records["key"] == key][0]) == n for key, n in zip(k.tolist(), c.tolist()))
        with pytest.raises(ValueError, match="signal_slots=8 at cycles=6" if sa == 8 else "pair_slots=8 at cycles=6"):
            MC.check_projection(proj)
    with pytest.raises(ValueError, match="signal_slots=8 at cycles=6"):
        MC.project_device(records, [1, 6, 2], signal_slots=8)
    with pytest.raises(ValueError, match="pair_slots=8 at cycles=6"):
        MC.project_device(records, [1, 6, 2], pair_slots=8)
    assert len(_of_cycle(MC.project_device(records, [1, 6, 2]), 1)[0]) == 20        # the default sizes hold every projection


def test_refused_parameters_write_nothing():
    import torch
    from fluorosequencingimageanalysis_amd import _native as N
    from fluorosequencingimageanalysis_amd import _native_proteome_mc as NP
    MC = _mc()
    records = _crowded()
    up = lambda a: torch.from_numpy(a).cuda()                                       # noqa: E731
    key, protein, count = up(records["key"].view(np.int64)), up(records["protein"]), up(records["count"])
    mask = up(H.cycle_masks(records["layout"], [1, 6]).view(np.int64))
    t = {"signals": torch.empty(2 * 64, dtype=torch.int64, device="cuda"), "pairs": torch.empty(2 * 64, dtype=torch.int64, device="cuda"),
         "counts": torch.empty(2 * 64, dtype=torch.int64, device="cuda"), "overflow": torch.empty(4, dtype=torch.int32, device="cuda")}
    for v in t.values():
        v.view(torch.uint8).fill_(0xA5)
    before = {k: v.clone() for k, v in t.items()}
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(key=key, protein=protein, count=count, n=20, mask=mask, n_masks=2, mode=NP.PROJECT, signals=t["signals"], sa=64,
                pairs=t["pairs"], counts=t["counts"], sb=64, overflow=t["overflow"])

    def call(**change):
        a = dict(good, **change)
        ptr = lambda x: None if x is None else x.data_ptr()                         # noqa: E731
        return NP.lib().fsq_proteome_project(ptr(a["key"]), ptr(a["protein"]), ptr(a["count"]), a["n"], ptr(a["mask"]), a["n_masks"],
                                             a["mode"], ptr(a["signals"]), a["sa"], ptr(a["pairs"]), ptr(a["counts"]), a["sb"],
                                             ptr(a["overflow"]), stream)
    refused = [dict(key=None), dict(protein=None), dict(mask=None), dict(signals=None), dict(pairs=None), dict(counts=None),
               dict(overflow=None), dict(n_masks=0), dict(n_masks=-1), dict(sa=48), dict(sb=48), dict(sa=0), dict(sb=0), dict(mode=2),
               dict(mode=-1), dict(mode=0x200), dict(n=-1)]
    for change in refused:
        assert call(**change) == N.FSQ_EINVAL, change
    assert call(n=0, key=None, protein=None, count=None) == N.FSQ_OK
    torch.cuda.synchronize()
    assert all(torch.equal(t[k], before[k]) for k in t)
    with pytest.raises(ValueError, match="fsq_proteome_project"):                   # the Python layer names the entry
        MC.project_into(MC.new_tables(64, 64, "cuda", n_masks=2), key, protein, count, mask, mode=7)
    with pytest.raises(ValueError, match="do not hold 2 masks"):
        MC.project_into(MC.new_tables(64, 64, "cuda"), key, protein, count, mask)
    with pytest.raises(ValueError, match="signal_slots=48"):
        MC.project_device(records, [1], signal_slots=48)
    with pytest.raises(ValueError, match="masks_per_launch"):
        MC.project_device(records, [1], masks_per_launch=0)
    with pytest.raises(ValueError, match="no cycle count"):
        MC.project_device(records, [])
    with pytest.raises(ValueError, match="'project' or 'within'"):
        MC.project_device(records, [1], mode="fold")


@pytest.mark.parametrize("cycles", [None, 0, 4, 8])
def test_merges_are_the_twin(cycles):
    MC = _mc()
    g = C.golden()["full"]
    a, b = C.records_of("full", g["merge"]["a"]), C.records_of("full", g["merge"]["b"])
    mask = None if cycles is None else H.cycle_masks(a["layout"], [cycles])[0]
    want = H.merge(C.triples(a), C.triples(b), mask)
    assert C.same(C.triples(MC.merge_records(a, b, cycles)), want)
    assert C.same(C.triples(MC.merge_records(a, b, cycles)), C.triples(MC.merge_records(a, b, cycles, host=True)))
    for other in (b, MC.cycle_tables(MC.project_device(b, [63]), 0)):               # records and a run on the device
        run = MC.cycle_tables(MC.project_device(a, [63], signal_slots=1024, pair_slots=1024), 0)
        assert MC.merge_device(run, other, cycles) is run and C.same(_held(run["tables"]), want)
    if cycles is None:
        assert len(a["key"]) <= 128 < len(want[0])
        small = MC.cycle_tables(MC.project_device(a, [63], signal_slots=128, pair_slots=128), 0)
        with pytest.raises(ValueError, match="pair_slots=128"):
            MC.merge_device(small, b)
        with pytest.raises(ValueError, match="different names"):
            MC.merge_device(run, dict(b, names=b["names"][::-1]))
        with pytest.raises(ValueError, match="different layouts"):
            MC.merge_records(a, dict(C.records_of("gapped"), names=a["names"]))


CURVE = ("cycles", "n_signals", "n_pairs", "samples_detected", "n_passing_signals", "n_identifiable_proteins", "identifiable")


def test_cycle_curve_of_40_proteins_against_the_host_and_the_unprojected_run():
    MC = _mc()
    peptides = MCC.e2e_peptides()
    kw = dict(MCC.E2E)
    windows, p, b, u = kw.pop("windows"), kw.pop("p"), kw.pop("b"), kw.pop("u")
    run = MC.monte_carlo_device(MC.proteome_table(peptides, windows), p, b, u, kw["sample_size"], kw["seed"])
    records = MC.monte_carlo_records(peptides, p, b, u, windows, **kw)
    want = MC.cycle_curve_records(records, host=True, **MCC.E2E_UNIQUES)
    assert want["cycles"].tolist() == list(range(1, 11)) and want["names"] == list(peptides) and len(peptides) == 39
    for source in (run, records):
        got = MC.cycle_curve_records(source, **MCC.E2E_UNIQUES)
        for name in CURVE:
            assert np.array_equal(got[name], want[name]) and got[name].dtype == want[name].dtype, name
        assert got["names"] == want["names"] and got["identifiable"].shape == (10, 39)
    for extra in (dict(demote=True), dict(absolute=True, maximum_secondary=2), dict(cycles=[7, 0, 3, 12])):
        args = dict(MCC.E2E_UNIQUES, **extra)
        got, host = MC.cycle_curve_records(run, **args), MC.cycle_curve_records(records, host=True, **args)
        for name in CURVE:
            assert np.array_equal(got[name], host[name]), (name, extra)
    uniq = MC.uniques_records(run, **MCC.E2E_UNIQUES)                                # the last point is today's answer
    found = MC.identifiable_proteins(uniq)
    assert [want["names"][i] for i in np.flatnonzero(want["identifiable"][-1])] == list(found) and len(found) > 0
    assert want["n_passing_signals"][-1] == int(uniq["passed"].sum()) and want["n_signals"][-1] == len(uniq["key"])
    assert want["n_pairs"][-1] == len(records["key"]) and want["samples_detected"][-1] == records["count"].sum()
    assert want["n_identifiable_proteins"][0] < want["n_identifiable_proteins"][-1]
