"""The proteome Monte-Carlo on the GPU at its limits (include/fsq_proteome_mc.h): the inputs of tests/_proteome_limit_cases.py,
whose edges tests/test_proteome_limits_host.py proves without a GPU, against the NumPy twin.  Every output is an integer: there
is no tolerance.  Every output buffer starts as a byte pattern, so that what a kernel leaves unwritten shows.

  A  fsq_proteome_signals with eight acids, a 64-bit key whose bit 63 is (63, 'Y'), windows up to position 63 and heads of up
     to 255 residues: whole at four parameter corners, as a chunk that starts and ends inside a peptide, and with sample ids
     across the 32-bit word boundary
  B  fsq_proteome_uniques over 525 000 signals (712 more than one pass of the grid) and on a segment of 100 000 proteins next
     to segments of one, under three scan modes, with and without demote

Run time of this file on an MI355X: 3 s for its 18 tests, 1.6 s of them the first test (it starts the device and builds the
Edman delay rows of gaps 1 .. 246); a scan of 525 000 signals 0.02 s, of the long segment 0.06 s."""
import contextlib

import numpy as np
import pytest

import _proteome_limit_cases as LC
from fluorosequencingimageanalysis_amd import _host_proteome_mc as H

pytestmark = pytest.mark.gpu


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


def _mc():
    from fluorosequencingimageanalysis_amd import MCsimlib as MC
    return MC


def _signals(corner, first_sample=0, first_row=0, n_rows=None):
    MC = _mc()
    p, b, u = LC.CORNERS[corner]
    with _prefilled():
        key, protein, draws = MC.signals_device(MC.device_table(LC.table(), p, b), u, LC.SAMPLE_SIZE, LC.SEED, first_sample, first_row,
                                                n_rows, with_draws=True)
        return key.cpu().numpy().view(np.uint64), protein.cpu().numpy(), draws.cpu().numpy()


# ---- A: the signals at the key's limits ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("corner", range(len(LC.CORNERS)))
def test_signals_with_a_full_key_are_the_twin(corner):
    key, protein, draws = _signals(corner)
    want_key, want_draws = LC.expected_signals(corner)
    assert len(key) == 350 and key.dtype == want_key.dtype and draws.dtype == want_draws.dtype
    assert np.array_equal(key, want_key), np.flatnonzero(key != want_key)[:10]
    assert np.array_equal(draws, want_draws)
    assert np.array_equal(protein, H.row_proteins(LC.table(), LC.SAMPLE_SIZE, 0, 350))


def test_a_chunk_inside_two_peptides_is_that_slice_of_the_whole():
    lo, n = LC.CHUNK
    key, protein, draws = _signals(0, 0, lo, n)
    want_key, want_draws = LC.expected_signals(0)
    assert np.array_equal(key, want_key[lo:lo + n]) and np.array_equal(draws, want_draws[lo:lo + n])
    assert np.array_equal(protein, H.row_proteins(LC.table(), LC.SAMPLE_SIZE, lo, n))


def test_sample_ids_cross_the_word_boundary_with_a_full_key():
    key, protein, draws = _signals(0, LC.FIRST_SAMPLE_WORD)
    want_key, want_draws = LC.expected_signals(0, LC.FIRST_SAMPLE_WORD)
    assert np.array_equal(key, want_key) and np.array_equal(draws, want_draws)
    assert np.array_equal(protein, H.row_proteins(LC.table(), LC.SAMPLE_SIZE, 0, 350))


# ---- B: the scan beyond one pass and on a long segment ------------------------------------------------------------------------
def _uniques(protein, count, segment, mode, demote):
    import torch
    MC = _mc()
    with _prefilled():
        got = MC.uniques_device(torch.from_numpy(protein).cuda(), torch.from_numpy(count).cuda(), torch.from_numpy(segment).cuda(),
                                LC.SCAN_MODES[mode], demote)
        return {k: v.cpu().numpy() for k, v in got.items()}


@pytest.mark.parametrize("demote", [False, True])
@pytest.mark.parametrize("mode", range(len(LC.SCAN_MODES)))
def test_uniques_over_more_signals_than_one_pass(mode, demote):
    """2 048 blocks of 256 signals are launched at most: the first 712 signals' lanes go round twice."""
    _, p, c = LC.block_triples()
    got = _uniques(np.tile(p, LC.TILES), np.tile(c, LC.TILES), LC.tiled_segments(LC.TILES), mode, demote)
    want = LC.block_expected(mode, demote)
    for name, dtype in H.UNIQUE_FIELDS:
        assert got[name].dtype == dtype and got[name].shape == (LC.TILES * LC.BLOCK_SIGNALS,), name
        assert np.array_equal(got[name], np.tile(want[name], LC.TILES)), (name, np.flatnonzero(got[name] != np.tile(want[name], LC.TILES))[:5])


@pytest.mark.parametrize("demote", [False, True])
@pytest.mark.parametrize("mode", range(len(LC.SCAN_MODES)))
def test_uniques_of_a_long_segment_between_two_short_ones(mode, demote):
    k, p, c = LC.long_triples()
    got = _uniques(p, c, H.segments(k), mode, demote)
    want = LC.long_expected(mode, demote)
    for name, dtype in H.UNIQUE_FIELDS:
        assert got[name].dtype == dtype and np.array_equal(got[name], want[name]), (name, got[name], want[name])
    assert got["n_ties"][1] == LC.LONG_TIES - 1 and got["tertiary"][1] > 10 ** 6
    if demote:
        rows = list(zip(*(got[name].tolist() for name in ("best_protein", "best_count", "second_protein", "second_count", "n_ties",
                                                          "tertiary"))))
        assert rows == LC.long_top_two()
