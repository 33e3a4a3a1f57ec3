"""The estimate of the integer offset between two colour channels on the GPU (include/fsq_channel_offset.h):
fsq_channel_offset_votes and fsq_channel_offset_peak against the NumPy twin, array for array and with every output pre-filled,
on the smallest shapes at which they can go wrong; malformed and oversized segments by the flag; estimate_offsets_records,
joint_observed_records(offsets='estimate') and the command line against their host=True forms and against the run with the
known offsets.  There is no reference output (the reference stops at one label letter): the twin is pinned to a plain-Python
restatement of the definition in test_channel_offset_host.py."""
import contextlib
import os

import numpy as np
import pytest

from _channel_offset_cases import (MOVED_BY, SHIFT_OFFSETS, SHIFT_RADII, SHIFT_SIZES, peak_cases, shifted_channels, shifted_experiment,
                                   votes_cases, votes_fuzz_case)
from _colocalize_cases import SIGMA, channel_tables, photometries_of, segments
from _lognormal_chain_cases import same_chain

from fluorosequencingimageanalysis_amd import _host_channel_offset as HO
from fluorosequencingimageanalysis_amd import _host_colocalize as H

pytestmark = pytest.mark.gpu

VOTES, PEAKS = votes_cases(), peak_cases()


@contextlib.contextmanager
def _prefilled():
    """Every output tensor a binding allocates starts as a byte pattern, not as zeros: what a kernel leaves unwritten shows."""
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


def _up(x, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()


def _device_votes(case):
    """(the kernel's V, the twin's) of a votes case."""
    from fluorosequencingimageanalysis_amd import colocalize as CL
    a_hw, a_field, b_hw, b_field, W = case
    if len(a_hw) + len(b_hw) < 1000:
        sa_hw, a_seg, a_off, sb_hw, _, b_off = segments(a_hw, a_field, b_hw, b_field)
    else:
        ids = np.unique(np.concatenate([a_field, b_field]))
        (a_order, a_seg, a_off), (b_order, _, b_off) = H.grouped(a_field, ids), H.grouped(b_field, ids)
        sa_hw, sb_hw = np.asarray(a_hw)[a_order], np.asarray(b_hw)[b_order]
    exp = HO.votes(sa_hw, a_seg, a_off, sb_hw, b_off, W)
    with _prefilled():
        got = CL.offset_votes_device(_up(sa_hw, np.int32).reshape(-1, 2), _up(a_seg, np.int32), _up(a_off, np.int64),
                                     _up(sb_hw, np.int32).reshape(-1, 2), _up(b_off, np.int64), W)
    return got.cpu().numpy(), exp


# ---- votes ----

@pytest.mark.parametrize("name", sorted(VOTES))
def test_votes_equal_the_twin(name):
    got, exp = _device_votes(VOTES[name])
    assert got.dtype == exp.dtype and got.shape == exp.shape and np.array_equal(got, exp), name


def test_votes_equal_the_twin_on_a_dense_lattice():
    got, exp = _device_votes(votes_fuzz_case())
    assert np.array_equal(got, exp)
    # 3 300 tracks in 3 fields on a 40 x 40 lattice: every bin of the 37 x 37 window is hit many times, from 13 blocks
    assert exp.shape == (37, 37) and exp.min() > 100 and exp.sum() > 1000000


def test_malformed_segments_are_flagged_and_vote_nothing_out_of_bounds():
    """a_seg and the offsets live on the device: the kernel refuses them by its flag, lane by lane.  votes stands inside one
    larger pre-filled buffer whose guard regions must stay as they were."""
    import torch
    from fluorosequencingimageanalysis_amd import _native_channel_offset as NCO, colocalize as CL, engine
    rng = np.random.default_rng(5)
    n_a, n_b, W = 300, 290, 3
    a_hw, b_hw = rng.integers(0, 9, (n_a, 2)), rng.integers(0, 9, (n_b, 2))
    seg = np.repeat(np.arange(3), 100).astype(np.int32)
    a_off, b_off = np.array([0, 100, 200, 300]), np.array([0, 100, 200, 290])
    bins, guard = (2 * W + 1) ** 2, 64
    d_a_hw, d_b_hw = _up(a_hw, np.int32), _up(b_hw, np.int32)

    def run(a_seg, ao, bo):
        buf = torch.full((guard + bins + guard,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")
        d_bad = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        keep = (_up(a_seg, np.int32), _up(ao, np.int64), _up(bo, np.int64))
        engine.launch(NCO.lib().fsq_channel_offset_votes, "fsq_channel_offset_votes", buf.device, d_a_hw.data_ptr(), keep[0].data_ptr(),
                      keep[1].data_ptr(), keep[2].data_ptr(), d_b_hw.data_ptr(), W, n_a, n_b, 3, buf[guard:].data_ptr(), d_bad.data_ptr())
        buf, flag = buf.cpu().numpy(), int(d_bad)
        assert (buf[:guard] == -0x5A5A5A5A5A5A5A5B).all() and (buf[guard + bins:] == -0x5A5A5A5A5A5A5A5B).all()
        return buf[guard:guard + bins].reshape(2 * W + 1, 2 * W + 1), flag

    def of_good_lanes(a_seg, ao, bo):
        """(the votes of the lanes that pass the kernel's test, each against its segment's B range; the pairs they walk)."""
        bad, _ = H.bad_lanes(a_seg, ao, bo, n_a, n_b)
        exp, pairs = np.zeros((2 * W + 1, 2 * W + 1), np.int64), 0
        for i in np.flatnonzero(~bad):
            b0, b1 = int(bo[a_seg[i]]), int(bo[a_seg[i] + 1])
            d = a_hw[i] - b_hw[b0:b1]
            d = d[(np.abs(d) <= W).all(axis=1)] + W
            np.add.at(exp, (d[:, 0], d[:, 1]), 1)
            pairs += b1 - b0
        return exp, pairs
    V, flag = run(seg, a_off, b_off)
    assert flag == 0 and np.array_equal(V, HO.votes(a_hw, seg, a_off, b_hw, b_off, W)) and V.sum() > 0
    assert np.array_equal(V, of_good_lanes(seg, a_off, b_off)[0])
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
        assert H.bad_lanes(a_seg, ao, bo, n_a, n_b)[1]
        V, flag = run(a_seg, ao, bo)
        assert flag == 1
        exp, pairs = of_good_lanes(np.asarray(a_seg), np.asarray(ao), np.asarray(bo))
        assert np.array_equal(V, exp) and V.sum() <= pairs            # the well-formed lanes' votes, and nothing else
        with pytest.raises(ValueError, match="not well formed"):
            CL.offset_votes_device(d_a_hw, _up(a_seg, np.int32), _up(ao, np.int64), d_b_hw, _up(bo, np.int64), W)
        with pytest.raises(ValueError, match="not well formed"):
            CL.estimate_offset_device(d_a_hw, _up(a_seg, np.int32), _up(ao, np.int64), d_b_hw, _up(bo, np.int64), 2, 1)


def test_a_segment_of_two_to_the_24_is_refused():
    """One a against a segment of 2^24 b's (128 MB of zeros): 256 such lanes could wrap a block's 32-bit bin, so the lane sets
    the flag and casts no vote."""
    import torch
    from fluorosequencingimageanalysis_amd import _native_channel_offset as NCO, colocalize as CL
    n_b = NCO.MAX_SEGMENT_B
    d_b_hw = torch.zeros((n_b, 2), dtype=torch.int32, device="cuda")
    d_a_hw, d_seg = torch.zeros((1, 2), dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    d_a_off = torch.tensor([0, 1], device="cuda")
    with _prefilled():
        V, d_bad = CL._launch_votes(d_a_hw, d_seg, d_a_off, d_b_hw, torch.tensor([0, n_b], device="cuda"), 1)
    assert int(d_bad) == 1 and V.cpu().numpy().tolist() == [[0] * 3] * 3
    with pytest.raises(ValueError, match="2\\^24 or more"):
        CL.offset_votes_device(d_a_hw, d_seg, d_a_off, d_b_hw, torch.tensor([0, n_b], device="cuda"), 1)


# ---- the peak ----

@pytest.mark.parametrize("name", sorted(PEAKS))
def test_peak_equals_the_twin(name):
    from fluorosequencingimageanalysis_amd import colocalize as CL
    V, R, tol_sq = PEAKS[name]
    d_V = _up(V, np.int64)
    with _prefilled():
        rec, S = CL.offset_peak_device(d_V, R, tol_sq, scores=True)
        alone = CL.offset_peak_device(d_V, R, tol_sq)
    assert rec.dtype == S.dtype == d_V.dtype and tuple(rec.shape) == (16,)
    assert np.array_equal(rec.cpu().numpy(), HO.peak(V, R, tol_sq)) and np.array_equal(alone.cpu().numpy(), HO.peak(V, R, tol_sq)), name
    assert np.array_equal(S.cpu().numpy(), HO.scores(V, R, tol_sq)), name
    assert np.array_equal(d_V.cpu().numpy(), V)


# ---- the entries' FSQ_EINVALs ----

def test_the_entries_refuse_their_arguments():
    """FSQ_EINVAL of the C entries themselves: nothing is launched, nothing written."""
    import torch
    from fluorosequencingimageanalysis_amd import _native_channel_offset as NCO, engine
    z = torch.zeros(64, dtype=torch.int64, device="cuda")
    p, odd = z.data_ptr(), z.data_ptr() + 4
    votes = lambda *a: engine.launch(NCO.lib().fsq_channel_offset_votes, "fsq_channel_offset_votes", z.device, *a)   # noqa: E731
    peak = lambda *a: engine.launch(NCO.lib().fsq_channel_offset_peak, "fsq_channel_offset_peak", z.device, *a)      # noqa: E731
    for W, n_a, n_b, n_seg in ((-1, 0, 0, 0), (65, 0, 0, 0), (1, -1, 0, 0), (1, 0, -1, 0), (1, 0, 0, -1), (1, 1 << 31, 0, 0),
                               (1, 0, 1 << 31, 0), (1, 0, 0, 1 << 31)):
        with pytest.raises(ValueError, match="invalid argument"):
            votes(p, p, p, p, p, W, n_a, n_b, n_seg, p, p)
    for args in ((p, p, p, p, p, 1, 1, 1, 1, None, p), (p, p, p, p, p, 1, 1, 1, 1, p, None), (p, p, None, p, p, 1, 1, 1, 1, p, p),
                 (p, p, p, None, p, 1, 1, 1, 1, p, p), (None, p, p, p, p, 1, 1, 1, 1, p, p), (p, None, p, p, p, 1, 1, 1, 1, p, p),
                 (p, p, p, p, None, 1, 1, 1, 1, p, p), (odd, p, p, p, p, 1, 1, 1, 1, p, p), (p, p, p, p, odd, 1, 1, 1, 1, p, p),
                 (p, p, odd, p, p, 1, 1, 1, 1, p, p), (p, p, p, odd, p, 1, 1, 1, 1, p, p), (p, p, p, p, p, 1, 1, 1, 1, odd, p)):
        with pytest.raises(ValueError, match="invalid argument"):
            votes(*args)
    for W, R, tol_sq in ((-1, 0, 0), (65, 0, 0), (3, -1, 0), (3, 0, -1), (3, 4, 0), (3, 3, 1), (3, 2, 4), (3, 0, 16), (64, 61, 16),
                         (3, 0, 1 << 62)):
        with pytest.raises(ValueError, match="invalid argument"):
            peak(p, W, R, tol_sq, p, p)
    for args in ((None, 3, 1, 1, p, p), (p, 3, 1, 1, None, p), (odd, 3, 1, 1, p, p), (p, 3, 1, 1, odd, p), (p, 3, 1, 1, p, odd)):
        with pytest.raises(ValueError, match="invalid argument"):
            peak(*args)
    assert not z.any()


def test_tensor_checks_of_the_device_functions():
    import torch
    from fluorosequencingimageanalysis_amd import colocalize as CL
    hw, seg, off = (torch.zeros((2, 2), dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"),
                    torch.tensor([0, 2], device="cuda"))
    assert CL.offset_votes_device(hw, seg, off, hw, off, 0).tolist() == [[4]]
    est = CL.estimate_offset_device(hw, seg, off, hw, off, 1, 0)
    assert est["offset"] == (0, 0) and est["score"] == est["total"] == 4 and est["votes"].is_cuda and est["centroid"] == (0.0, 0.0)
    for args in ((hw.to(torch.int64), seg, off, hw, off), (hw, seg.to(torch.int64), off, hw, off), (hw, seg, off.to(torch.int32), hw, off),
                 (hw, seg, off, hw, off[:1]), (hw.t(), seg, off, hw, off), (hw, seg[:1], off, hw, off), (hw.cpu(), seg, off, hw, off)):
        with pytest.raises(ValueError):
            CL.offset_votes_device(*args, 2)
    for W in (-1, 65):
        with pytest.raises(ValueError, match="W must be"):
            CL.offset_votes_device(hw, seg, off, hw, off, W)
    big = torch.tensor([[1 << 30, 0], [0, 0]], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match=r"\|coordinate\| < 2\^30"):
        CL.offset_votes_device(big, seg, off, hw, off, 2)
    with pytest.raises(ValueError, match="max_shift=63"):
        CL.estimate_offset_device(hw, seg, off, hw, off, 63, 4)
    V = torch.zeros((7, 7), dtype=torch.int64, device="cuda")
    for bad in (V.to(torch.int32), V[:, :5], V[:6, :6], V.cpu(), torch.zeros((7, 14), dtype=torch.int64, device="cuda")[:, ::2], torch.zeros((131, 131), dtype=torch.int64, device="cuda")):
        with pytest.raises(ValueError, match="votes are"):
            CL.offset_peak_device(bad, 0, 0)
    for R, tol_sq in ((3, 1), (-1, 0), (0, -1), (0, 16), (4, 0)):
        with pytest.raises(ValueError, match="R \\+ isqrt"):
            CL.offset_peak_device(V, R, tol_sq)


# ---- estimates on inputs whose shift is known ----

@pytest.mark.parametrize("size", SHIFT_SIZES)
def test_estimates_equal_the_host_and_the_known_shift(size):
    from fluorosequencingimageanalysis_amd import colocalize as CL
    for offset in SHIFT_OFFSETS + ((17, 0),):
        a_hw, a_field, b_hw, b_field = shifted_channels(17, *size, offset)
        for radius in SHIFT_RADII:
            exp = CL.estimate_offset_records(a_hw, a_field, b_hw, b_field, 16, radius, host=True)
            with _prefilled():
                got = CL.estimate_offset_records(a_hw, a_field, b_hw, b_field, 16, radius)
            assert sorted(got) == sorted(exp) and all(got[k] == exp[k] for k in exp if k != "votes"), (size, offset, radius)
            assert got["votes"].dtype == exp["votes"].dtype and np.array_equal(got["votes"], exp["votes"])
            print(size, offset, radius, "score", got["score"], "runner_up", got["runner_up"], "total", got["total"])
            # (the twin's own results on these inputs, test_channel_offset_host.py: the true shift, or the window's edge next to it)
            assert got["offset"] == (offset if offset != (17, 0) else (16, 0)) and got["at_edge"] == (max(map(abs, offset)) >= 16)


@pytest.mark.parametrize("K", [2, 3, 4])
def test_estimate_offsets_records_equal_the_host_and_the_known_offsets(K):
    from fluorosequencingimageanalysis_amd import colocalize as CL
    tables, offsets = channel_tables(4, K, n=300, fields=3, side=40)
    for radius in SHIFT_RADII:
        exp = CL.estimate_offsets_records(tables, radius, host=True)
        with _prefilled():
            got = CL.estimate_offsets_records(tables, radius)
        assert got[0] == exp[0]
        for g, e in zip(got[1], exp[1]):
            assert (g is None) == (e is None)
            assert g is None or (all(g[k] == e[k] for k in e if k != "votes") and np.array_equal(g["votes"], e["votes"]))
        if radius == 2:                                                # (either channel is jittered by +-1: under radius sqrt(2) the twin is a pixel off)
            known, est = CL.molecules_records(tables, radius, offsets), CL.molecules_records(tables, radius, got[0])
            assert got[0] == list(offsets) and all(np.array_equal(known[k], est[k]) for k in known)
    with pytest.raises(ValueError, match="channel 1: .*max_shift=16.*min_score=100000"):
        CL.estimate_offsets_records(tables, 2, min_score=100000)


def test_joint_observed_records_estimate_equal_the_host_and_the_known_offset():
    from fluorosequencingimageanalysis_amd import colocalize as CL
    tables = shifted_experiment()
    exp = CL.joint_observed_records(tables, SIGMA, offsets='estimate', max_shift=8, host=True)
    with _prefilled():
        got = CL.joint_observed_records(tables, SIGMA, offsets='estimate', max_shift=8)
    known = CL.joint_observed_records(tables, SIGMA, offsets={"K": (-MOVED_BY[0], -MOVED_BY[1])})
    assert "offsets" not in known and got["offsets"] == exp["offsets"] == {"C": (0, 0), "K": (-3, 4)}
    assert sorted(got["offset_estimates"]) == ["K"]
    g, e = got["offset_estimates"]["K"], exp["offset_estimates"]["K"]
    assert all(g[k] == e[k] for k in e if k != "votes") and np.array_equal(g["votes"], e["votes"]) and isinstance(g["votes"], np.ndarray)
    for other in (exp, known):
        for k in ("signals", "n_molecules", "n_rejected", "total_count", "none_count", "labels"):
            assert got[k] == other[k], k
        for k in ("member", "field", "hw"):
            assert np.array_equal(got["molecules"][k], other["molecules"][k]), k
        assert np.array_equal(got["rejected"], other["rejected"]) and np.array_equal(got["fit_index"], other["fit_index"])
    for L in exp["labels"]:
        same_chain(got["channels"][L], exp["channels"][L], L)
    assert len(got["signals"]) > 10


def test_command_line_on_the_device_estimates_the_offset(tmp_path):
    from fluorosequencingimageanalysis_amd import joint_signals, lognormal as LN, sweep_peptide
    path = str(tmp_path / "track_photometries_abc123.csv")
    LN.write_photometries_dict_to_csv(photometries_of(shifted_experiment(), {"K": "ch1", "C": "ch2"}), path)
    argv = [path, "--labels", "K=ch1", "C=ch2", "--beta_sigma", "K=0.2,C=0.25"]
    est = joint_signals.main(argv + ["--estimate_offset", "--max_shift", "8", "--output_directory", str(tmp_path / "est")])
    given = joint_signals.main(argv + ["--offset", "K=-3,4", "--output_directory", str(tmp_path / "given")])
    host = joint_signals.main(argv + ["--host", "--estimate_offset", "--max_shift", "8", "--output_directory", str(tmp_path / "host")])
    assert sweep_peptide.load_observed(est[0]) == sweep_peptide.load_observed(given[0]) == sweep_peptide.load_observed(host[0])
    assert len(sweep_peptide.load_observed(est[0])) > 10 and len(given) == 2
    for a, b in ((est[1], given[1]), (est[1], host[1]), (est[2], host[2])):
        with open(a) as f, open(b) as g:
            assert f.read() == g.read()
    with open(est[2]) as f:
        assert f.read().splitlines()[1].startswith("K,-3,4,")
    assert os.path.basename(est[2]).startswith("ChannelOffsets_")
