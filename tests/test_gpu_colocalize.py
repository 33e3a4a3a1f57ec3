"""The colocalisation of tracks between colour channels on the GPU (include/fsq_colocalize.h): fsq_colocalize_match against the
NumPy twin, array for array, on the smallest shapes at which it can go wrong; the merge over K channels, joint_observed_records
and the command line against their host=True forms.  There is no reference output (the reference stops at one label letter):
the twin is pinned to a plain-Python restatement of the definition in test_colocalize_host.py."""
import contextlib
import os

import numpy as np
import pytest

from _colocalize_cases import SIGMA, channel_tables, experiment, fuzz_case, match_cases, photometries_of, segments
from _lognormal_chain_cases import same_chain

from fluorosequencingimageanalysis_amd import _host_colocalize as H

pytestmark = pytest.mark.gpu

CASES = match_cases()


@contextlib.contextmanager
def _prefilled():
    """Every output tensor a binding allocates starts as a byte pattern, not as zeros or -1: what a kernel leaves unwritten
    shows."""
    import torch
    real = torch.empty

    def filled(*a, **k):
        t = real(*a, **k)
        if t.is_cuda and t.numel():
            t.view(torch.uint8).fill_(0xA5)
        return t
    torch.empty = filled
    try:
        yield
    finally:
        torch.empty = real


def _device_match(case):
    from fluorosequencingimageanalysis_amd import colocalize as CL
    a_hw, a_field, b_hw, b_field, r2 = case
    sa_hw, a_seg, a_off, sb_hw, _, b_off = segments(a_hw, a_field, b_hw, b_field) if len(a_hw) + len(b_hw) < 1000 else _fast_segments(case)
    exp = H.match(sa_hw, a_seg, a_off, sb_hw, b_off, r2)
    with _prefilled():
        got = CL.match_records(sa_hw, a_seg, a_off, sb_hw, b_off, r2)
    return got, exp


def _fast_segments(case):
    a_hw, a_field, b_hw, b_field, _ = case
    ids = np.unique(np.concatenate([a_field, b_field]))
    a_order, a_seg, a_off = H.grouped(a_field, ids)
    b_order, b_seg, b_off = H.grouped(b_field, ids)
    return np.asarray(a_hw)[a_order], a_seg, a_off, np.asarray(b_hw)[b_order], b_seg, b_off


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_equals_the_twin(name):
    got, exp = _device_match(CASES[name])
    for g, e, what in zip(got, exp, ("match_of_a", "match_of_b", "dist_sq_of_a")):
        assert g.dtype == e.dtype and np.array_equal(g, e), (name, what)


def test_kernel_equals_the_twin_on_a_dense_lattice():
    got, exp = _device_match(fuzz_case())
    for g, e, what in zip(got, exp, ("match_of_a", "match_of_b", "dist_sq_of_a")):
        assert np.array_equal(g, e), what
    d = exp[2][exp[0] >= 0]
    # two thirds of the lattice's cells are taken in either set: positions repeat, several b's stand at most a's best distance,
    # and more than half of the a's lose their best b to another a
    assert len(exp[0]) == 3300 and 1000 < len(d) < 3000 and {0, 1, 2} <= set(d.tolist()) <= {0, 1, 2, 4}
    assert (exp[0] < 0).sum() > 1000


def test_malformed_segments_are_flagged_and_leave_minus_one():
    """a_seg and the offsets live on the device: the kernel refuses them by its flag, lane by lane, and reads nothing out of
    bounds (no offset it has not proven is ever used as an index).  Checked by the flag and the -1s it must leave."""
    import torch
    from fluorosequencingimageanalysis_amd import colocalize as CL
    rng = np.random.default_rng(5)
    n_a, n_b = 300, 290
    a_hw, b_hw = rng.integers(0, 9, (n_a, 2)), rng.integers(0, 9, (n_b, 2))
    seg = np.repeat(np.arange(3), 100).astype(np.int32)
    a_off, b_off = np.array([0, 100, 200, 300]), np.array([0, 100, 200, 290])
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()                # noqa: E731

    def run(a_seg, a_off, b_off):
        with _prefilled():
            out = CL._launch_match(up(a_hw, np.int32), up(a_seg, np.int32), up(a_off, np.int64), up(b_hw, np.int32), up(b_off, np.int64), 4)
        return [t.cpu().numpy() for t in out]
    good = run(seg, a_off, b_off)
    assert int(good[3][0]) == 0 and all(np.array_equal(g, e) for g, e in zip(good, H.match(a_hw, seg, a_off, b_hw, b_off, 4)))
    wrong_seg = seg.copy()
    wrong_seg[[3, 150, 299]] = [-1, 3, 2 ** 31 - 1]
    for a_seg, ao, bo in ((wrong_seg, a_off, b_off),
                          (seg, [0, 100, 301, 300], b_off),            # beyond n_a
                          (seg, a_off, [0, 200, 100, 290]),            # descending
                          (seg, a_off, [0, -5, 200, 290]),             # negative
                          (seg, a_off, [0, 100, 200, 2 ** 40]),        # far beyond n_b
                          (seg, [0, 90, 200, 300], b_off),             # a's 90 .. 99 stand outside their segment's range
                          (seg, a_off, [0, 100, 200, 280]),            # b's offsets end before n_b: no lane is bad, the flag is set
                          (seg, [5, 100, 200, 300], b_off)):
        bad, flag = H.bad_lanes(a_seg, ao, bo, n_a, n_b)
        assert flag
        match_of_a, match_of_b, dist, d_bad = run(a_seg, ao, bo)
        assert int(d_bad[0]) == 1
        assert (match_of_a[bad] == -1).all() and (dist[bad] == -1).all()
        assert ((match_of_a >= -1) & (match_of_a < n_b)).all() and ((match_of_b >= -1) & (match_of_b < n_a)).all()
        assert not np.isin(np.flatnonzero(bad), match_of_b).any()       # no b is paired with a bad lane
        with pytest.raises(ValueError, match="not well formed"):
            CL.match_device(up(a_hw, np.int32), up(a_seg, np.int32), up(ao, np.int64), up(b_hw, np.int32), up(bo, np.int64), 4)


def test_the_entry_refuses_negative_sizes_and_radius():
    """FSQ_EINVAL of the C entry itself: nothing is launched, nothing written."""
    import torch
    from fluorosequencingimageanalysis_amd import _native_colocalize as NCL, engine
    z = torch.zeros(4, dtype=torch.int64, device="cuda")
    for radius_sq, n_a, n_b, n_seg in ((-1, 0, 0, 0), (4, -1, 0, 0), (4, 0, -1, 0), (4, 0, 0, -1), (4, 1 << 31, 0, 0), (4, 0, 1 << 31, 0)):
        with pytest.raises(ValueError, match="invalid argument"):
            engine.launch(NCL.lib().fsq_colocalize_match, "fsq_colocalize_match", z.device, z.data_ptr(), z.data_ptr(), z.data_ptr(),
                          z.data_ptr(), z.data_ptr(), radius_sq, n_a, n_b, n_seg, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr())
    assert z.tolist() == [0, 0, 0, 0]


def test_tensor_checks_of_match_device():
    import torch
    from fluorosequencingimageanalysis_amd import colocalize as CL
    hw, seg, off = (torch.zeros((2, 2), dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"),
                    torch.tensor([0, 2], device="cuda"))
    assert [t.tolist() for t in CL.match_device(hw, seg, off, hw, off, 0)] == [[0, -1], [0, -1], [0, -1]]
    for args in ((hw.to(torch.int64), seg, off, hw, off), (hw, seg.to(torch.int64), off, hw, off), (hw, seg, off.to(torch.int32), hw, off),
                 (hw, seg, off, hw, off[:1]), (hw.t(), seg, off, hw, off), (hw, seg[:1], off, hw, off), (hw.cpu(), seg, off, hw, off)):
        with pytest.raises(ValueError):
            CL.match_device(*args, 4)
    with pytest.raises(ValueError, match="negative"):
        CL.match_device(hw, seg, off, hw, off, -1)
    big = torch.tensor([[1 << 30, 0], [0, 0]], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match=r"\|coordinate\| < 2\^30"):
        CL.match_device(big, seg, off, hw, off, 4)


@pytest.mark.parametrize("K", [2, 3, 4])
def test_molecules_on_the_device_equal_the_twin(K):
    from fluorosequencingimageanalysis_amd import colocalize as CL
    for seed, radius in ((1, 2), (2, 1.5), (3, 0)):
        tables, offsets = channel_tables(seed, K, n=400, fields=4, side=30)
        exp = CL.molecules_records(tables, radius, offsets, host=True)
        with _prefilled():
            got = CL.molecules_records(tables, radius, offsets)
        for k in ("member", "field", "hw"):
            assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), (K, seed, k)
        # (the input is worth the run: many molecules with several members; with radius 0 only the unjittered ninth pairs)
        assert ((exp["member"] >= 0).sum(axis=0) > 1).sum() > (100 if radius else 20)
    empty = (np.zeros((0, 2), np.int64), np.zeros(0, np.int64))
    for tabs in ([empty] + tables[1:], tables[:-1] + [empty], [empty] * K):
        exp, got = CL.molecules_records(tabs, 2, host=True), CL.molecules_records(tabs, 2)
        assert all(np.array_equal(got[k], exp[k]) for k in exp)


@pytest.fixture(scope="module")
def host_runs():
    from fluorosequencingimageanalysis_amd import colocalize as CL
    tables, _ = experiment()
    return {(solver, mode): CL.joint_observed_records(tables, SIGMA, solver=solver, on_filtered=mode, host=True)
            for solver, mode in (("enumerate", "reject"), ("dp", "dark"))}


@pytest.mark.parametrize("solver,mode", [("enumerate", "reject"), ("dp", "dark")])
def test_joint_observed_records_equal_the_host(host_runs, solver, mode):
    from fluorosequencingimageanalysis_amd import colocalize as CL
    tables, _ = experiment()
    exp = host_runs[(solver, mode)]
    got = CL.joint_observed_records(tables, SIGMA, solver=solver, on_filtered=mode)
    for k in ("signals", "n_molecules", "n_rejected", "total_count", "none_count", "labels"):
        assert got[k] == exp[k], k
    assert got["total_count"] == sum(got["signals"].values()) + got["none_count"] and len(got["signals"]) > 10
    for k in ("member", "field", "hw"):
        assert np.array_equal(got["molecules"][k], exp["molecules"][k]), k
    assert np.array_equal(got["rejected"], exp["rejected"]) and np.array_equal(got["fit_index"], exp["fit_index"])
    for L in exp["labels"]:
        assert np.array_equal(got["kept"][L], exp["kept"][L])
        same_chain(got["channels"][L], exp["channels"][L], (solver, L))


def test_joint_key_limits_on_the_device():
    from fluorosequencingimageanalysis_amd import colocalize as CL
    tables, _ = experiment()
    with pytest.raises(ValueError, match="table_slots=4"):
        CL.joint_observed_records(tables, SIGMA, table_slots=4)


def test_command_line_on_the_device_writes_the_host_pickle(tmp_path):
    from fluorosequencingimageanalysis_amd import joint_signals, lognormal as LN, sweep_peptide
    tables, _ = experiment()
    path = str(tmp_path / "track_photometries_abc123.csv")
    LN.write_photometries_dict_to_csv(photometries_of(tables, {"K": "ch1", "C": "ch2"}), path)
    argv = [path, "--labels", "K=ch1", "C=ch2", "--beta_sigma", "K=0.2,C=0.25", "--radius", "2.5"]
    dev = joint_signals.main(argv + ["--output_directory", str(tmp_path / "dev")])
    host = joint_signals.main(argv + ["--host", "--output_directory", str(tmp_path / "host")])
    assert sweep_peptide.load_observed(dev[0]) == sweep_peptide.load_observed(host[0]) and len(sweep_peptide.load_observed(dev[0])) > 10
    with open(dev[1]) as f, open(host[1]) as g:
        assert f.read() == g.read()
    assert os.path.basename(dev[0]).startswith("JointSignals_")
