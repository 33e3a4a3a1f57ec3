"""Loader of tests/golden/chisq_traces.npz (tools/gen_chisq_golden.py) and the seeded random batch of the chi-squared tests."""
import os

import numpy as np

from _util import GOLD


def golden():
    return np.load(os.path.join(GOLD, "chisq_traces.npz"))


def fit_cases():
    g = golden()
    out = []
    for i in range(len(g["case_len"])):
        fm, rm = g["fit_case"] == i, g["rec_case"] == i
        out.append(dict(lum=g["lum"][g["lum_off"][i]:g["lum_off"][i + 1]], name=str(g["case_name"][i]),
                        num_steps=int(g["case_num_steps"][i]) or None, mult=float(g["case_mult"][i]), L=int(g["case_L"][i]),
                        mag=float(g["case_mag"][i]), ignore=bool(g["case_ignore"][i]),
                        fit=list(zip(g["fit_start"][fm].tolist(), g["fit_stop"][fm].tolist(), g["fit_h"][fm].tolist())),
                        best=g["rec_best"][rm], counter=g["rec_counter"][rm], counter_n=g["rec_counter_n"][rm], S=g["rec_S"][rm]))
    return out


def filter_cases():
    g = golden()
    out = []
    for i in range(len(g["filt_case"])):
        ci = int(g["filt_case"][i])
        im, om = g["fin_case"] == i, g["fout_case"] == i
        out.append(dict(lum=g["lum"][g["lum_off"][ci]:g["lum_off"][ci + 1]], mode=int(g["filt_mode"][i]),
                        mag=float(g["filt_mag"][i]) if g["filt_has_mag"][i] else None,
                        ratio=float(g["filt_ratio"][i]) if g["filt_has_ratio"][i] else None, r2=float(g["filt_r2"][i]),
                        pin=list(zip(g["fin_start"][im].tolist(), g["fin_stop"][im].tolist(), g["fin_h"][im].tolist())),
                        pout=list(zip(g["fout_start"][om].tolist(), g["fout_stop"][om].tolist(), g["fout_h"][om].tolist()))))
    return out


# parameter sets of the random batch: (num_steps, multiplier, min_step_length, min_step_magnitude, ignore_counterfits)
BATCH_PARAMS = ((3, 1, 2, 0.0, False), (None, 0.05, 2, 0.0, False), (6, 1, 0, 0.0, True), (5, 1, 3, 5000.0, False),
                (None, 0.1, 0, 2000.0, False), (2, 1, 5, 0.0, False))


def random_batch(seed, n_traces):
    """Ragged traces of 3 - 300 frames (four in five below 60): bleaching staircases in noise, rounded to integers, to halves
    or not at all, some flat, some exact staircases."""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(n_traces):
        n = int(rng.integers(3, 60)) if rng.random() < 0.8 else int(rng.integers(60, 301))
        kind = int(rng.integers(0, 10))
        steps = int(rng.integers(0, 5))
        level = np.full(n, float(steps))
        for _ in range(steps):
            level[int(rng.integers(0, n)):] -= 1.0
        if kind == 0:
            v = np.full(n, float(np.round(rng.normal(0.0, 100.0), 1)))
        elif kind == 1:
            v = level * 1.5 + 2.0
        else:
            v = level * rng.uniform(5e3, 3e4) + rng.normal(0.0, rng.uniform(1e3, 6e3), n)
            if kind < 5:
                v = np.round(v)
            elif kind < 7:
                v = np.round(v * 2.0) / 2.0
        out.append(v)
    return out
