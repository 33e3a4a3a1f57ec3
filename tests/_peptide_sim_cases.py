"""Shared by the peptide-simulation tests: the golden cases of tests/golden/peptide_sim.npz as keyword sets, and seeded
random parameter sets."""
import functools
import math
import os

import numpy as np

from _util import GOLD

TABLES = ("counts", "loss_cycle", "loss_cause", "edman_fail", "category", "n_draws")


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLD, "peptide_sim.npz"))


@functools.lru_cache(maxsize=None)
def golden_cases():
    """One dict per recorded case: the reference's arguments (`api`: what the package's functions take), the twin's
    arguments (`twin`), the recorded tables and texts."""
    g = golden()
    out = []
    for ci, name in enumerate(g["case_names"].tolist()):
        pre = "c%d_" % ci
        seq, label = str(g[pre + "sequence"]), str(g[pre + "label"])
        mocks, edmans, sc, n = (int(x) for x in g[pre + "ints"])
        p, b, pcb, u, s, s2, beta, sigma, rate, factor = g[pre + "floats"].tolist()
        seed, first, ddif = int(g[pre + "seed"][0]), int(g[pre + "first"][0]), g[pre + "ddif"].tolist()
        mask = sum(1 << i for i, ch in enumerate(seq) if ch == label)
        out.append({"name": name, "n": n, "seed": seed, "first": first, "reserved": str(g[pre + "reserved"]), "sequence": seq,
                    "label": label, "num_mocks": mocks, "num_edmans": edmans,
                    "api": dict(p=p, b=b, u=u, s=s, sc=sc, s2=s2, beta=beta, beta_sigma=sigma, ddif=ddif, superdye_rate=rate,
                                superdye_factor=factor),
                    "twin": dict(length=len(seq), label_mask=mask, num_mocks=mocks, num_edmans=edmans, p=p, per_cycle_b=pcb, u=u, s=s,
                                 sc=sc, s2=s2, log_beta=math.log(beta), beta_sigma=sigma, ddif=ddif, superdye_rate=rate,
                                 superdye_factor=factor),
                    "per_cycle_b": pcb, "tuples": g[pre + "tuples"].tolist(), "intensity": g[pre + "intensity"],
                    "tables": {k: g[pre + k] for k in TABLES}})
    return out


def same_records(got, exp, what=None):
    """Two record dicts, every table exactly, floats by bit pattern."""
    for k in TABLES:
        assert np.array_equal(np.asarray(got[k]).astype(np.uint64), np.asarray(exp[k]).astype(np.uint64)), (what, k)
        assert tuple(got[k].shape) == tuple(exp[k].shape), (what, k)
    for k in ("intensity", "log_intensity"):
        if k in exp:
            assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint64), np.ascontiguousarray(exp[k]).view(np.uint64)), (what, k)


def random_twin_params(rng):
    """A seeded random parameter set of the twin's keywords (without seed, first_molecule, n_molecules)."""
    length = int(rng.integers(1, 41))
    n_lab = int(rng.integers(0, min(length, 15) + 1))
    pos = rng.choice(length, n_lab, replace=False)
    mocks, edmans = int(rng.integers(0, 6)), int(rng.integers(0, 14))
    rate = float(rng.choice([0.0, 0.0, 0.3, 1.0]))
    return dict(length=length, label_mask=int(sum(1 << int(i) for i in pos)), num_mocks=mocks, num_edmans=edmans,
                p=float(rng.uniform(0.5, 1.0)), per_cycle_b=float(rng.uniform(0.7, 1.0)), u=float(rng.uniform(0.0, 0.6)),
                s=float(rng.uniform(0.0, 0.4)), sc=int(rng.integers(0, 8)), s2=float(rng.uniform(0.0, 0.2)),
                log_beta=math.log(float(rng.uniform(5e3, 9e4))), beta_sigma=float(rng.uniform(0.05, 0.4)),
                ddif=[0.0] + rng.uniform(0.0, 0.5, 14).tolist(), superdye_rate=rate, superdye_factor=float(rng.uniform(1.0, 3.0)))
