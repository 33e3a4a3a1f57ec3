"""Shared by the several-letter peptide-simulation tests: the golden cases of tests/golden/peptide_labels.npz as keyword sets,
and seeded random parameter sets."""
import functools
import math
import os

import numpy as np

from _util import GOLD

TABLES = ("counts", "loss_cycle", "loss_cause", "edman_fail", "category", "n_draws")


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLD, "peptide_labels.npz"))


@functools.lru_cache(maxsize=None)
def golden_cases():
    """One dict per recorded case: the reference's arguments (`api`: what the package's functions take, per-letter values as
    dicts), the twin's arguments (`twin`), the recorded tables and texts."""
    g = golden()
    out = []
    for ci, name in enumerate(g["case_names"].tolist()):
        pre = "c%d_" % ci
        seq, labels = str(g[pre + "sequence"]), str(g[pre + "labels"])
        letters = sorted(set(labels))
        mocks, edmans, sc, n = (int(x) for x in g[pre + "ints"])
        p, b, pcb, u, s, s2 = g[pre + "floats"].tolist()
        betas, sigmas, rates, factors = g[pre + "channel_floats"].tolist()
        ddif = [row[:m] for row, m in zip(g[pre + "ddif"].tolist(), g[pre + "n_ddif"].tolist())]
        masks = [sum(1 << i for i, ch in enumerate(seq) if ch == letter) for letter in letters]
        by = lambda values: dict(zip(letters, values))
        out.append({"name": name, "n": n, "seed": int(g[pre + "seed"][0]), "first": int(g[pre + "first"][0]),
                    "reserved": str(g[pre + "reserved"]), "sequence": seq, "labels": labels, "letters": letters, "num_mocks": mocks,
                    "num_edmans": edmans,
                    "api": dict(p=p, b=b, u=u, s=s, sc=sc, s2=s2, beta=by(betas), beta_sigma=by(sigmas), ddif=by(ddif),
                                superdye_rate=by(rates), superdye_factor=by(factors)),
                    "twin": dict(length=len(seq), channel_masks=masks, num_mocks=mocks, num_edmans=edmans, p=p, per_cycle_b=pcb, u=u,
                                 s=s, sc=sc, s2=s2, log_beta=[math.log(x) for x in betas], beta_sigma=sigmas, ddif=ddif,
                                 superdye_rate=rates, superdye_factor=factors),
                    "tuples": g[pre + "tuples"].tolist(), "intensity": g[pre + "intensity"],
                    "tables": {k: g[pre + k] for k in TABLES}})
    return out


def same_records(got, exp, what=None):
    """Two record dicts, every table exactly, floats by bit pattern."""
    for k in TABLES:
        assert tuple(got[k].shape) == tuple(exp[k].shape), (what, k)
        assert np.array_equal(np.asarray(got[k]).astype(np.uint64), np.asarray(exp[k]).astype(np.uint64)), (what, k)
    for k in ("intensity", "log_intensity"):
        if k in exp:
            assert tuple(got[k].shape) == tuple(exp[k].shape), (what, k)
            assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint64), np.ascontiguousarray(exp[k]).view(np.uint64)), (what, k)


def log_of(intensity):
    """The log-intensity table of an intensity table: math.log, FSQ_PEPTIDE_OFF_LOG where the intensity is 0."""
    flat = [math.log(x) if x > 0 else -10000.0 for x in np.asarray(intensity).reshape(-1).tolist()]
    return np.array(flat).reshape(np.asarray(intensity).shape)


def random_twin_params(rng, K=None):
    """A seeded random parameter set of simulate_labels' keywords (without seed, first_molecule, n_molecules): K disjoint
    channel masks, some of them empty now and then."""
    K = int(rng.integers(1, 5)) if K is None else K
    length = int(rng.integers(1, 41))
    n_lab = int(rng.integers(0, min(length, 12) + 1))
    pos = rng.choice(length, n_lab, replace=False)
    owner = rng.integers(0, K, n_lab)
    masks = [int(sum(1 << int(i) for i, o in zip(pos, owner) if o == k)) for k in range(K)]
    return dict(length=length, channel_masks=masks, num_mocks=int(rng.integers(0, 6)), num_edmans=int(rng.integers(0, 14)),
                p=float(rng.uniform(0.5, 1.0)), per_cycle_b=float(rng.uniform(0.7, 1.0)), u=float(rng.uniform(0.0, 0.6)),
                s=float(rng.uniform(0.0, 0.4)), sc=int(rng.integers(0, 8)), s2=float(rng.uniform(0.0, 0.2)),
                log_beta=[math.log(float(rng.uniform(5e3, 9e4))) for _ in range(K)],
                beta_sigma=[float(rng.uniform(0.05, 0.4)) for _ in range(K)],
                ddif=[[0.0] + rng.uniform(0.0, 0.5, 14).tolist() for _ in range(K)],
                superdye_rate=[float(rng.choice([0.0, 0.0, 0.3, 1.0])) for _ in range(K)],
                superdye_factor=[float(rng.uniform(1.0, 3.0)) for _ in range(K)])
