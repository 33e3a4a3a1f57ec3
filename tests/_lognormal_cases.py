"""The recorded lognormal cases of tests/golden/lognormal_tracks.npz (tools/gen_lognormal_golden.py) and seeded batches for
the host and GPU tests."""
import functools
import math
import os

import numpy as np

from _util import GOLD


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLD, "lognormal_tracks.npz"))


@functools.lru_cache(maxsize=None)
def single_cases():
    """The (a) cases as dicts: inputs, and the reference's outputs (best_seq None without a sequence)."""
    g = golden()
    off = g["a_off"]
    out = []
    for i in range(len(off) - 1):
        T, m = int(g["a_T"][i]), int(g["a_max_possible"][i])
        s = slice(int(off[i]), int(off[i + 1]))
        has = bool(g["a_has_seq"][i])
        word = int(g["a_category"][i])
        dev = float(g["a_max_deviation"][i])
        out.append(dict(name=str(g["a_name"][i]), T=T, max_possible=m, multidrop=bool(g["a_multidrop"][i]),
                        max_deviation=int(dev) if dev == 3 else dev, beta_sigma=float(g["a_beta_sigma"][i]),
                        means=g["a_means"][i][:m + 2].tolist(), intensity=g["a_intensity"][s].tolist(),
                        category=tuple(bool((word >> f) & 1) for f in range(T)), word=word,
                        best_seq=tuple(g["a_best_seq"][s].tolist()) if has else None,
                        best_score=float(g["a_best_score"][i]), frame_score=g["a_frame_score"][s] if has else None,
                        signal=str(g["a_signal"][i]), is_zero=[None, False, True][int(g["a_is_zero"][i]) + 1],
                        start=None if g["a_start"][i] < 0 else int(g["a_start"][i]), lmii=int(g["a_lmii"][i]),
                        tie=bool(g["a_tie"][i]), greedy_differs=bool(g["a_greedy_differs"][i]),
                        n_surviving=int(g["a_n_surviving"][i])))
    return out


def means_for(beta, max_possible, ddif=0.30):
    q = [0.0] + [ddif] * (max_possible + 1)
    return [math.log(beta) + math.log(i + 1.0) - q[i] for i in range(max_possible + 2)]


def random_batch(seed, n, max_possible=5, beta=10000.0, sigma=0.2, t_lo=1, t_hi=13):
    """n seeded tracks of mixed lengths t_lo .. t_hi: (intensities, categories).  Mostly ON-prefix categories with lognormal
    ON frames, some broken categories and non-positive intensities."""
    rng = np.random.default_rng(seed)
    means = means_for(beta, max_possible)
    I, C = [], []
    for k in range(n):
        T = int(rng.integers(t_lo, t_hi + 1))
        v, seq = int(rng.integers(1, max_possible + 1)), []
        for f in range(T):
            seq.append(v)
            if v > 0 and rng.random() < 0.3:
                v -= 1 if rng.random() < 0.8 else min(v, 2)
        noise = sigma * float(rng.choice([0.6, 1.0, 1.5]))
        vals = [math.exp(rng.normal(means[s - 1], noise)) if s > 0 else rng.normal(40.0, 300.0) for s in seq]
        cat = [s > 0 for s in seq]
        kind = int(rng.integers(0, 10))
        if kind == 0:
            cat = [True] * T
        elif kind == 1:
            cat[int(rng.integers(0, T))] ^= True
        elif kind == 2:
            vals[int(rng.integers(0, T))] = 0.0
        if k % 2:
            vals = [float(int(round(x))) for x in vals]
        I.append(vals)
        C.append(tuple(cat))
    return I, C


def restated_records(R, intensities, categories, log_fluor_means, beta_sigma, max_possible=5, allow_multidrop=True,
                     max_deviation=3, budget=1 << 22, lengths=None, device=None):
    """lognormal.lognormal_records computed by the restatement R (_host_lognormal.py): the same dict of arrays."""
    n = len(intensities)
    F = max([len(x) for x in intensities] + [1])
    out = {"status": np.zeros(n, np.int32), "best_seq": np.zeros((n, F), np.uint8), "best_score": np.full(n, -1.0),
           "frame_score": np.zeros((n, F)), "n_surviving": np.zeros(n, np.int64),
           "lengths": np.array([len(x) for x in intensities], np.int32)}
    for t, (I, c) in enumerate(zip(intensities, categories)):
        ok, _ = R.tables(I, c, log_fluor_means, beta_sigma, max_possible, max_deviation)
        out["n_surviving"][t] = R.count_surviving(ok, max_possible, allow_multidrop)
        if out["n_surviving"][t] > budget:
            out["status"][t] = 2
            continue
        seq, score, fs, n_surv = R.fit(I, c, log_fluor_means, beta_sigma, max_possible, allow_multidrop, max_deviation)
        assert n_surv == out["n_surviving"][t]
        if seq is None:
            out["status"][t] = 1
        else:
            out["best_seq"][t, :len(seq)], out["best_score"][t], out["frame_score"][t, :len(seq)] = seq, score, fs
    return out


def chain_csv_text():
    return golden()["b_csv"].tobytes().decode()


def recorded_fit_info(pre):
    """all_fit_info of the recorded chain fit `pre` ("b_fit0_" / "b_fit1_") as the reference's tuples."""
    g = golden()
    out = []
    for i in range(len(g[pre + "field"])):
        has = bool(g[pre + "has_seq"][i])
        seq = tuple(g[pre + "best_seq"][i].tolist()) if has else None
        out.append(("ch1", int(g[pre + "field"][i]), int(g[pre + "h"][i]), int(g[pre + "w"][i]), int(g[pre + "row"][i]),
                    tuple(g[pre + "category"][i].tolist()), tuple(g[pre + "intensity"][i].tolist()),
                    str(g[pre + "signal"][i]), [None, False, True][int(g[pre + "is_zero"][i]) + 1], seq, 5,
                    float(g[pre + "best_score"][i]), g[pre + "frame_score"][i].tolist() if has else None,
                    int(g[pre + "start"][i]) if has else None))
    return out


def check_fit_against_record(fit, pre):
    """A (signals, total_count, none_count, all_fit_info) result against the recorded one: same order, bit for bit."""
    g = golden()
    signals, total, none_count, info = fit
    assert [str(k) for k in signals] == g[pre + "signal_keys"].tolist()
    assert list(signals.values()) == g[pre + "signal_counts"].tolist()
    assert [total, none_count] == g[pre + "counts"].tolist()
    exp = recorded_fit_info(pre)
    assert len(info) == len(exp)
    for got, e in zip(info, exp):
        assert got[:6] == e[:6], e[:5]
        assert np.array_equal(np.asarray(got[6], np.float64).view(np.uint64), np.asarray(e[6]).view(np.uint64)), e[:5]
        assert str(got[7]) == e[7] and got[8] == e[8] and got[9] == e[9] and got[10] == e[10] and got[13] == e[13], e[:5]
        assert np.float64(got[11]).view(np.uint64) == np.float64(e[11]).view(np.uint64), e[:5]
        if e[9] is not None:
            assert np.array_equal(np.asarray(got[12], np.float64).view(np.uint64), np.asarray(e[12]).view(np.uint64)), e[:5]
        else:
            assert got[12] is None
