"""Track arrays on the host, NumPy only: what stepfitting, timetrace, lognormal, remainder, peptide_simulator and
simulate_peptide share before a launch and after a download.  A category is a tuple of booleans, one per frame, or the uint64
word with bit f set when frame f is ON; tracks travel as float64 [n, max_frames] rows with int32 [n] lengths."""
from math import log

import numpy as np

def category_word(category):
    """A tuple of booleans as the uint64 word: bit f set when frame f is ON."""
    return sum(1 << f for f, c in enumerate(category) if c)


def pattern_to_tuple(pattern, n_frames):
    """uint64 pattern -> the reference's tuple of booleans (Experiment.trace_to_binary)."""
    p = int(pattern)
    return tuple(bool((p >> f) & 1) for f in range(n_frames))


def category_words(categories, n, n_frames=None):
    """uint64 [n] words of tuples of booleans (exactly n_frames entries each, where given; entries beyond 64 are not read),
    or of the words themselves as a 1-D integer array.  n=None: the caller checks the count."""
    if isinstance(categories, np.ndarray) and categories.ndim == 1 and categories.dtype.kind in "iu":
        cats = np.ascontiguousarray(categories).astype(np.uint64)
    else:
        categories = list(categories)
        if n_frames is not None and any(len(c) != n_frames for c in categories):
            raise ValueError("every track needs exactly %d category entries" % n_frames)
        cats = np.array([category_word(c[:64]) for c in categories], dtype=np.uint64)
    if n is not None and len(cats) != n:
        raise ValueError("one category per track")
    return cats


def pack_rows(sequences, lengths=None, none_is_zero=None, min_frames=0, short_error=None, nan_error=None, width=None, width_error=None):
    """Ragged sequences, or a 2-D array (with `lengths`, or every row full) -> (float64 [n, width] rows, 0 beyond a row's
    length, int32 [n] lengths).

    none_is_zero  True / False: every element through float(), a None counting 0.0 / raising; None: np.asarray per sequence
    min_frames    a shorter sequence raises ValueError(short_error)
    nan_error     the ValueError text (% the sequence's index) for a sequence that holds a NaN; None lets NaN pass
    width         the width every sequence must have, else ValueError(width_error); None: the longest one's, at least 1"""
    if isinstance(sequences, np.ndarray) and sequences.ndim == 2:
        rows = np.ascontiguousarray(sequences, dtype=np.float64)
        lens = np.full(len(rows), rows.shape[1], np.int32) if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
        if width is None and rows.shape[1] == 0:
            rows = np.zeros((len(rows), 1))
    else:
        conv = (lambda v: 0.0 if v is None else float(v)) if none_is_zero else float
        seqs = [np.asarray(s, dtype=np.float64).reshape(-1) if none_is_zero is None else np.array([conv(v) for v in s], dtype=np.float64)
                for s in sequences]
        lens = np.array([len(s) for s in seqs], dtype=np.int32)
        W = width if width is not None else (max(int(lens.max()), 1) if len(seqs) else 1)
        rows = np.zeros((len(seqs), W), dtype=np.float64)
        for i, s in enumerate(seqs):
            if width is not None and len(s) != width:
                raise ValueError(width_error)
            rows[i, :len(s)] = s
    if width is not None and rows.shape[1] != width:
        raise ValueError(width_error)
    if len(lens) and lens.min() < min_frames:
        raise ValueError(short_error)
    if nan_error is not None and np.isnan(rows).any():
        raise ValueError(nan_error % np.flatnonzero(np.isnan(rows).any(axis=1))[0])
    return rows, lens


def log_fluor_means(beta, quench_factors, max_possible):
    """MCsimlib._photometries_lognormal_fit_MP_v8's log_fluor_means (:5531): the mean log intensity of 1 .. max_possible + 2 fluors."""
    if quench_factors is None or len(quench_factors) != max_possible + 2:
        raise ValueError("quench_factors required for v8+")
    return [log(beta) + log(i + 1.0) - quench_factors[i] for i in range(max_possible + 2)]


def tally_signals(fits, counts=None):
    """({(signal, is_zero, starting_intensity): n}, the number of fits without a signal) of (signal, is_zero, start) triples;
    counts: how often each one stands (default: once)."""
    signals, none_count = {}, 0
    for k, (signal, is_zero, start) in enumerate(fits):
        n = 1 if counts is None else counts[k]
        if signal is None:
            none_count += n
        else:
            signals[(signal, is_zero, start)] = signals.get((signal, is_zero, start), 0) + n
    return signals, none_count


def decrements_of_row(counts):
    """A molecule's dye counts per frame as old-style decrements: ('A', c) per dye lost before frame c, (('A', 0),) for none."""
    dec = tuple(('A', c) for c in range(1, len(counts)) for _ in range(counts[c - 1] - counts[c]))
    return dec if dec else (('A', 0),)
