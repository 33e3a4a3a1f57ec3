"""Peptide Monte-Carlo simulation for several label letters on the GPU (include/fsq_peptide_labels.h): bit for bit against the
reference's recorded runs under the same draws (tests/golden/peptide_labels.npz), against the NumPy twin
(_host_peptide_sim.simulate_labels) and, with one channel, against fsq_peptide_simulate; the chain into the lognormal fit and
the command line.  Nothing is compared with a tolerance."""
import contextlib
import ctypes
import math
import pickle

import numpy as np
import pytest

from fluorosequencingimageanalysis_amd import _host_peptide_sim as T
from _peptide_labels_cases import golden_cases, log_of, random_twin_params, same_records

pytestmark = pytest.mark.gpu

CHANNEL_MAJOR = ("counts", "intensity", "log_intensity", "category")
BASE = dict(length=8, channel_masks=[0b01000100, 0b10001000], num_mocks=2, num_edmans=4, p=0.9, per_cycle_b=0.9, u=0.5, s=0.3, sc=3,
            s2=0.1, log_beta=[math.log(70000.0), math.log(31000.0)], beta_sigma=[0.2, 0.3], ddif=[[0.0] + [0.3] * 14, [0.0] + [0.2] * 14],
            superdye_rate=[0.0, 0.0], superdye_factor=[1.0, 1.0])


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


def _prm(kw, seed, first, n_channels=None):
    from fluorosequencingimageanalysis_amd import _native_peptide_labels as NL
    prm = NL.FsqPeptideLabelsParams()
    for k in ("p", "per_cycle_b", "u", "s", "s2", "length", "num_mocks", "num_edmans", "sc"):
        setattr(prm, k, kw[k])
    K = len(kw["channel_masks"])
    prm.seed, prm.first_molecule, prm.n_channels = seed, first, K if n_channels is None else n_channels
    for k in range(min(K, 4)):
        prm.channel_mask[k], prm.n_ddif[k] = kw["channel_masks"][k], min(len(kw["ddif"][k]), 15)
        prm.log_beta[k], prm.beta_sigma[k] = kw["log_beta"][k], kw["beta_sigma"][k]
        prm.superdye_rate[k], prm.superdye_factor[k] = kw["superdye_rate"][k], kw["superdye_factor"][k]
        for i, x in enumerate(kw["ddif"][k][:15]):
            prm.ddif[k][i] = x
    return prm


def _device(kw, seed, first, n):
    """fsq_peptide_simulate_labels on pre-filled outputs, as host arrays."""
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS
    with _prefilled():
        out = PS.multilabel_device_prm(_prm(kw, seed, first), n)
        host = {k: v.cpu().numpy() for k, v in out.items()}
    host["edman_fail"], host["category"] = host["edman_fail"].view(np.uint64), host["category"].view(np.uint64)
    return host


def _molecules(records, lo, hi):
    return {k: (v[:, lo:hi] if k in CHANNEL_MAJOR else v[lo:hi]) for k, v in records.items()}


def _against_twin(kw, seed, first, n, what=None):
    got = _device(kw, seed, first, n)
    exp = T.simulate_labels(seed=seed, first_molecule=first, n_molecules=n, **kw)
    same_records(got, exp, what)
    return got


@pytest.mark.parametrize("ci", range(7))
def test_golden_through_c_abi_and_python_surface(ci):
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS
    c = golden_cases()[ci]
    exp = dict(c["tables"], intensity=c["intensity"], log_intensity=log_of(c["intensity"]))
    same_records(_device(c["twin"], c["seed"], c["first"], c["n"]), exp, c["name"])
    with _prefilled():
        rec = PS.multilabel_records(c["sequence"], c["labels"], c["num_mocks"], c["num_edmans"], c["n"], seed=c["seed"],
                                    first_molecule=c["first"], **c["api"])
    same_records(rec, exp, c["name"])
    assert rec["labels"] == tuple(c["letters"]) and rec["category"].dtype == np.uint64


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_random_parameter_sets_equal_the_twin(K):
    rng = np.random.default_rng(2000 + K)
    for rep in range(5):
        kw = random_twin_params(rng, K)
        _against_twin(kw, int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 40)), int(rng.integers(100, 300)), (K, rep))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_one_channel_equals_fsq_peptide_simulate(seed):
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS
    from fluorosequencingimageanalysis_amd import _native_peptide_sim as NP
    from _peptide_sim_cases import random_twin_params as one_letter_params

    def one_letter_prm(kw, seed, first):
        prm = NP.FsqPeptideSimParams()
        for k in ("label_mask", "p", "per_cycle_b", "u", "s", "s2", "log_beta", "beta_sigma", "superdye_rate", "superdye_factor", "length",
                  "num_mocks", "num_edmans", "sc"):
            setattr(prm, k, kw[k])
        prm.seed, prm.first_molecule, prm.n_ddif = seed, first, 15
        for i, x in enumerate(kw["ddif"]):
            prm.ddif[i] = x
        return prm
    rng = np.random.default_rng(seed)
    for rep in range(3):
        one = one_letter_params(rng)
        first = 2 ** 32 - 100 if rep == 0 else int(rng.integers(0, 2 ** 40))
        kw = dict(one, channel_masks=[one["label_mask"]], **{k: [one[k]] for k in ("log_beta", "beta_sigma", "ddif", "superdye_rate", "superdye_factor")})
        del kw["label_mask"]
        got = _device(kw, 77 + seed, first, 200)
        with _prefilled():
            exp = {k: v.cpu().numpy() for k, v in PS.simulate_device_prm(one_letter_prm(one, 77 + seed, first), 200).items()}
        for k, v in exp.items():
            g = got[k][0] if k in CHANNEL_MAJOR else got[k]
            assert g.shape == v.shape and np.array_equal(g.view(np.uint8), v.view(np.uint8)), (seed, rep, k)


LOW_LOSS = dict(u=0.05, s=0.01, s2=0.005, per_cycle_b=0.99)
EDGES = {
    "four_channels_of_15_at_64_frames": dict(length=64, channel_masks=[sum(1 << (4 * i + k) for i in range(15)) for k in range(4)],
                                             num_mocks=13, num_edmans=50, log_beta=[11.0, 10.5, 10.0, 9.5], beta_sigma=[0.2, 0.25, 0.3, 0.15],
                                             ddif=[[0.01 * i * (k + 1) for i in range(15)] for k in range(4)],
                                             superdye_rate=[0.0, 0.5, 1.0, 0.0], superdye_factor=[1.0, 2.0, 1.5, 3.0], **LOW_LOSS),
    "length_64_first_and_last": dict(length=64, channel_masks=[1, 1 << 63], num_edmans=20),
    "one_frame": dict(num_mocks=0, num_edmans=0),
    "empty_first_mask": dict(channel_masks=[0, 0b10001000]),
    "empty_last_mask": dict(channel_masks=[0b01000100, 0]),
    "all_masks_empty": dict(channel_masks=[0, 0]),
    "superdye_0": dict(superdye_rate=[0.0, 0.0], superdye_factor=[2.5, 2.5]),
    "superdye_1": dict(superdye_rate=[1.0, 1.0], superdye_factor=[2.5, 1.5], u=0.1),
    "superdye_mixed": dict(superdye_rate=[0.5, 0.0], superdye_factor=[2.5, 2.5], u=0.1),
    "superdye_mixed_other_way": dict(superdye_rate=[0.0, 1.0], superdye_factor=[2.5, 2.5], u=0.1),
    "shorter_than_edmans": dict(length=2, channel_masks=[0b01, 0b10], num_edmans=9, p=0.95, u=0.1),
    "s_1": dict(s=1.0, u=0.0),
}


@pytest.mark.parametrize("name", sorted(EDGES))
def test_shape_and_parameter_edges(name):
    kw = dict(BASE)
    kw.update(EDGES[name])
    n = 130
    got = _against_twin(kw, 4242, 7, n, name)
    K, F = len(kw["channel_masks"]), kw["num_mocks"] + kw["num_edmans"] + 1
    L = sum(bin(m).count("1") for m in kw["channel_masks"])
    assert got["counts"].shape == (K, n, F) and got["loss_cycle"].shape == (n, L) and got["n_draws"].shape == (n, 1 + 2 * K)
    counts = got["counts"].astype(int)
    # the edge does what its name says
    if name == "four_channels_of_15_at_64_frames":
        assert (K, F, L) == (4, 64, 60) and counts[:, :, 0].max() == 15 and (counts[:, :, -1] > 0).any(axis=1).all()
        assert (got["category"] >> np.uint64(63)).any() and set(got["loss_cause"].reshape(-1).tolist()) == {0, 1, 2, 3, 4}
    if name.startswith("empty") or name == "all_masks_empty":
        for k, m in enumerate(kw["channel_masks"]):
            if m == 0:
                assert not counts[k].any() and not got["intensity"][k].any() and (got["log_intensity"][k] == -10000.0).all()
                assert not got["category"][k].any() and not got["n_draws"][:, 1 + 2 * k:3 + 2 * k].any()
            else:
                assert counts[k].any() and got["category"][k].any()
    if name == "s_1":
        assert (counts[:, :, 1:] == 0).all() and (counts[:, :, 0] > 0).any()
    if name == "shorter_than_edmans":
        assert len(set(got["n_draws"][:, 0].tolist())) > 1          # Edman stops drawing once the molecule is empty
    if name.startswith("superdye") and name != "superdye_0":
        for k, rate in enumerate(kw["superdye_rate"]):
            assert (got["n_draws"][:, 1 + 2 * k] == counts[k, :, 0]).all() and counts[k, :, 0].max() == 2
    if name == "one_frame":
        assert F == 1 and set(got["category"].reshape(-1).tolist()) == {0, 1}


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_molecule_counts_around_one_wavefront(n):
    kw = dict(BASE, channel_masks=[0b00000100, 0b10001000, 0b01000000], log_beta=[11.0, 10.0, 9.0], beta_sigma=[0.2] * 3,
              ddif=[[0.0, 0.3]] * 3, superdye_rate=[0.3, 0.0, 1.0], superdye_factor=[2.0] * 3)
    _against_twin(kw, 99, 10 ** 9, n, n)


def test_first_molecule_chunks_and_carry():
    whole = _device(BASE, 99, 2 ** 32 - 150, 300)
    same_records(whole, T.simulate_labels(seed=99, first_molecule=2 ** 32 - 150, n_molecules=300, **BASE), "carry into counter word 2")
    for lo, hi in ((0, 170), (170, 300)):
        same_records(_device(BASE, 99, 2 ** 32 - 150 + lo, hi - lo), _molecules(whole, lo, hi), (lo, hi))


def test_more_molecules_than_one_pass_of_the_grid():
    """16 384 blocks of 64 molecules are launched at most: beyond that a block takes further chunks."""
    kw = dict(BASE, num_mocks=1, num_edmans=0, length=3, channel_masks=[0b010, 0b101])
    n = 16384 * 64 + 1
    got = _device(kw, 5, 0, n)
    same_records(_molecules(got, 0, 130), T.simulate_labels(seed=5, first_molecule=0, n_molecules=130, **kw), "head")
    same_records(_molecules(got, n - 130, n), T.simulate_labels(seed=5, first_molecule=n - 130, n_molecules=130, **kw), "tail")
    for i in np.random.default_rng(8).integers(0, n, 1000).tolist():
        same_records(_molecules(got, i, i + 1), T.simulate_labels(seed=5, first_molecule=i, n_molecules=1, **kw), i)
    assert abs(float((got["counts"][0, :, 0] > 0).mean()) - 0.45) < 0.01


def test_invalid_parameters_return_einval_and_write_nothing():
    import torch
    from fluorosequencingimageanalysis_amd import _native as N
    from fluorosequencingimageanalysis_amd import _native_peptide_labels as NL
    nan = float("nan")
    bad = {"overlapping_masks": dict(channel_masks=[0b0110, 0b0100]), "bit_beyond_length": dict(channel_masks=[0b100, 1 << 8]),
           "sixteen_bits_in_one_mask": dict(length=40, channel_masks=[0xffff, 1 << 20]), "short_ddif": dict(ddif=[[0.0] * 15, [0.0]]),
           "nan_log_beta": dict(log_beta=[11.0, nan]), "inf_sigma": dict(beta_sigma=[float("inf"), 0.2]), "nan_p": dict(p=nan),
           "nan_ddif": dict(ddif=[[0.0, nan, 0.0], [0.0] * 3]), "superdye_rate_1_5": dict(superdye_rate=[0.0, 1.5]),
           "length_0": dict(length=0, channel_masks=[0, 0]), "length_65": dict(length=65), "65_frames": dict(num_mocks=30, num_edmans=34),
           "negative_mocks": dict(num_mocks=-1)}
    n = 10
    bufs = [torch.empty(n * 4 * 64 * 8, dtype=torch.uint8, device="cuda") for _ in range(8)]
    stream = torch.cuda.current_stream().cuda_stream

    def call(prm, n_molecules, pointers):
        for b in bufs:
            b.fill_(0xA5)
        rc = NL.lib().fsq_peptide_simulate_labels(ctypes.byref(prm), n_molecules, *(pointers + [stream]))
        torch.cuda.synchronize()
        assert all(bool((b == 0xA5).all()) for b in bufs)
        return rc

    pointers = [b.data_ptr() for b in bufs]
    for name, change in bad.items():
        kw = dict(BASE)
        kw.update(change)
        assert call(_prm(kw, 1, 0), n, pointers) == N.FSQ_EINVAL, name
    for K in (0, 5, -1):
        assert call(_prm(BASE, 1, 0, n_channels=K), n, pointers) == N.FSQ_EINVAL, K
    for hole in range(8):
        assert call(_prm(BASE, 1, 0), n, [None if j == hole else p for j, p in enumerate(pointers)]) == N.FSQ_EINVAL, hole
    assert call(_prm(BASE, 1, 0), -1, pointers) == N.FSQ_EINVAL
    assert call(_prm(BASE, 1, 2 ** 63 - 5), n, pointers) == N.FSQ_EINVAL
    # the loss tables may be null when no residue is labelled, and nothing is wrong with the valid call
    assert call(_prm(dict(BASE, channel_masks=[0, 0]), 1, 0), 0, pointers) == N.FSQ_OK
    rc = NL.lib().fsq_peptide_simulate_labels(ctypes.byref(_prm(dict(BASE, channel_masks=[0, 0]), 1, 0)), n,
                                              *([pointers[0], None, None] + pointers[3:] + [stream]))
    torch.cuda.synchronize()
    assert rc == N.FSQ_OK and not bool((bufs[0][:2 * n * 7] != 0).any())


CHAIN = dict(p=0.9, b=-math.log(1.0 - 0.1), u=0.5, s=0.3, sc=3, s2=0.1, beta={"K": 70000.0, "C": 31000.0}, beta_sigma={"K": 0.2, "C": 0.25},
             ddif={"K": [0, 0.3] + [0.3] * 5, "C": [0, 0.2] + [0.25] * 5}, superdye_rate=0.0, superdye_factor=1.0)


def test_multilabel_and_fit_records_equals_the_twin_through_the_fit():
    from fluorosequencingimageanalysis_amd import _tracks
    from fluorosequencingimageanalysis_amd import lognormal as LN
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS
    seq, labels, n, seed = "GAKCGAKC", "KC", 3000, 778
    with _prefilled():
        out = PS.multilabel_and_fit_records(seq, labels, 3, 8, n, seed=seed, max_possible=5, allow_multidrop=True, max_deviation=3,
                                            quench_factors=CHAIN["ddif"], **CHAIN)
    rec = PS.multilabel_records(seq, labels, 3, 8, n, seed=seed, host=True, **CHAIN)
    sim = {k: v.cpu().numpy() for k, v in out["simulation"].items() if hasattr(v, "cpu")}
    same_records(sim, rec)
    assert out["simulation"]["labels"] == ("C", "K")
    for k, letter in enumerate(("C", "K")):
        keep = rec["category"][k] != 0
        means = _tracks.log_fluor_means(CHAIN["beta"][letter], CHAIN["ddif"][letter], 5)
        host = LN.lognormal_records(rec["intensity"][k][keep], rec["category"][k][keep], means, CHAIN["beta_sigma"][letter], 5, True, 3)
        found = host["status"] == LN.STATUS_FOUND
        signals, _ = _tracks.tally_signals(LN.signal_of(tuple(row)) for row in host["best_seq"][found].tolist())
        got = out[letter]
        assert got["signals"] == signals and got["total_count"] == int(keep.sum()) and got["none_count"] == int((~found).sum()), letter
        assert np.array_equal(got["kept"].cpu().numpy(), keep) and len(signals) > 10 and 0 < got["none_count"] < got["total_count"]
    assert out["C"]["signals"] != out["K"]["signals"]
    # the joint ground truth against a plain Python tally of the twin's records
    mes = {}
    for i in range(n):
        rows = rec["counts"][:, i].tolist()
        if not any(row[0] for row in rows):
            continue
        dec = tuple((L, c) for c in range(1, 12) for L, row in zip("CK", rows) for _ in range(row[c - 1] - row[c]))
        key = (dec, tuple(row[-1] == 0 for row in rows), tuple(row[0] for row in rows))
        mes[key] = mes.get(key, 0) + 1
    assert out["molecular_error_signals"] == mes and len(mes) > 40 and sum(mes.values()) < n


def test_command_line_on_the_device_equals_the_twin(tmp_path):
    from fluorosequencingimageanalysis_amd import simulate_peptide as SP
    common = ["KAGKCGC", "CK", "-N", "500", "--seed", "123456790", "--superdye_rate", "0.25", "--superdye_factor", "2.0"]
    dev = SP.main(common + ["--output_directory", str(tmp_path / "dev")])
    host = SP.main(common + ["--host", "--output_directory", str(tmp_path / "host")])
    a, b = pickle.load(open(dev, "rb")), pickle.load(open(host, "rb"))
    assert a[1] == b[1] and a[2] == b[2] and sorted(a[1]) == ["C", "K"] and all(len(s) > 5 for s in a[1].values()) and len(a[2]) > 10
    da, db = vars(a[0]), vars(b[0])
    assert {k: v for k, v in da.items() if k not in ("host", "output_directory")} == {k: v for k, v in db.items() if k not in ("host", "output_directory")}
    text = open(dev[:-4] + ".csv", newline='').read()
    assert text == open(host[:-4] + ".csv", newline='').read() and "\r\nch1,0,0,0," in text and "\r\nch2,0,0,0," in text
