"""Plain Python / NumPy restatement of MCsimlib._intensities_to_signal_lognormal_v8 (:5413-5493, allow_upsteps=False): the
fit of `simulate_peptide --host` and the checker of the device fit, pinned to the reference's recorded outputs by
test_lognormal_host.

The reference enumerates every non-increasing count sequence and skips the ones that break a rule; this walks the same
sequences depth-first in the same order (largest count first) and leaves a branch at the first frame that breaks the
category rule, the multi-drop rule or the deviation rule.  Scores multiply left to right from 1.0, and the winner is the
first sequence with a strictly greater total than all before it, starting from -1.  The density is scipy's
norm(loc, scale).pdf(x) in closed form (equal bit for bit with numpy's AVX-512 paths disabled)."""
import math

import numpy as np

NORM_PDF_C = float(np.sqrt(2 * np.pi))


def norm_pdf(x, loc, scale):
    z = (x - loc) / scale
    return math.exp(-(z * z) / 2.0) / NORM_PDF_C / scale


def log_intensities(intensities):
    return [math.log(i) if i > 0 else -10000 for i in intensities]


def tables(intensities, categories, log_fluor_means, beta_sigma, max_possible, max_deviation):
    """Per frame: ok[v] whether count v passes the category and deviation rules there, score[v] its density."""
    L = log_intensities(intensities)
    ok, score = [], []
    for i, li in enumerate(L):
        o, s = [], []
        for v in range(max_possible + 1):
            if v == 0:
                o.append(not categories[i])
                s.append(1.0)
            else:
                dev = abs(li - log_fluor_means[v - 1]) / beta_sigma
                o.append(bool(categories[i]) and not dev > max_deviation)
                s.append(norm_pdf(li, log_fluor_means[v - 1], beta_sigma))
        ok.append(o)
        score.append(s)
    return ok, score


def count_surviving(ok, max_possible, allow_multidrop):
    """The number of sequences that pass every rule, by completion counts per (frame, count)."""
    T = len(ok)
    W = [int(ok[T - 1][v]) for v in range(max_possible + 1)]
    for f in range(T - 2, -1, -1):
        W = [sum(W[(0 if allow_multidrop else max(v - 1, 0)):v + 1]) if ok[f][v] else 0 for v in range(max_possible + 1)]
    return sum(W)


def fit(intensities, categories, log_fluor_means, beta_sigma, max_possible=5, allow_multidrop=True, max_deviation=3):
    """(best_seq or None, best_score, best_intensity_scores or None, number of surviving sequences)."""
    T = len(intensities)
    if not allow_multidrop and T == 1:
        raise ValueError("max() arg is an empty sequence")           # (:5442, for the first sequence that passes the category rule)
    ok, score = tables(intensities, categories, log_fluor_means, beta_sigma, max_possible, max_deviation)
    best_seq, best_score, best_scores, n = None, -1, None, 0
    seq, prod = [0] * T, [1.0] * (T + 1)
    f, v = 0, max_possible                  # next candidate count v at frame f
    while True:
        lo = 0 if (f == 0 or allow_multidrop) else max(seq[f - 1] - 1, 0)
        while v >= lo and not ok[f][v]:
            v -= 1
        if v < lo:                          # frame f is exhausted: back to the frame before, next smaller count
            f -= 1
            if f < 0:
                break
            v = seq[f] - 1
            continue
        seq[f] = v
        prod[f + 1] = prod[f] * score[f][v]
        if f + 1 < T:
            f += 1
            continue                        # (v stays: the next frame starts at the same count)
        n += 1
        if prod[T] > best_score:
            best_seq, best_score, best_scores = tuple(seq), prod[T], [score[i][s] for i, s in enumerate(seq)]
        v -= 1
    return best_seq, best_score, best_scores, n


def signal_of(best_seq):
    """(signal, is_zero, starting_intensity) as :5467-5491 build them."""
    if best_seq is None:
        return None, None, None
    signal = []
    for i, tf in enumerate([best_seq[f] - fc for f, fc in enumerate(best_seq[1:])]):
        if tf > 0:
            signal += [('A', i + 1)] * tf
        elif tf < 0:
            return None, None, best_seq[0]
    signal = tuple(signal) if signal else (('A', 0),)
    return signal, best_seq[-1] == 0, best_seq[0]


def intensities_to_signal(intensities, beta_sigma, max_possible, allow_multidrop, max_deviation, categories, log_fluor_means):
    """The reference's 7-tuple."""
    best_seq, best_score, scores, _ = fit(intensities, categories, log_fluor_means, beta_sigma, max_possible, allow_multidrop,
                                          max_deviation)
    signal, is_zero, start = signal_of(best_seq)
    return signal, is_zero, best_seq, max_possible, best_score, scores, start
