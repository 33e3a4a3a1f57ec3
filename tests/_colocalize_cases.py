"""Shared by the colocalisation tests: the match cases, a plain-Python double-loop restatement of the definition (written from
DESIGN.md 4.30's text, not from the NumPy twin), random channel tables for the merge over K channels, and a small simulated
two-colour experiment as track tables.

There is no reference output: the reference stops at one label letter.  The oracle is the plain loop below; the NumPy twin
(_host_colocalize) is pinned to it on the host, and the kernel to the twin on the GPU."""
import functools

import numpy as np

BIG = (1 << 30) - 1                                              # the largest coordinate's magnitude


# ---- the definition, restated ----

def d2(p, q):
    return (int(p[0]) - int(q[0])) ** 2 + (int(p[1]) - int(q[1])) ** 2


def plain_match(a_hw, a_field, b_hw, b_field, radius_sq):
    """(match_of_a, match_of_b, dist_sq_of_a) as lists, -1 where unmatched: mutual nearest neighbours within a field, the
    smallest (d2, index) among d2 <= radius_sq, ties to the lowest index, no second choice."""
    def best(p, field, hw, fields):
        found = None
        for j in range(len(hw)):
            if fields[j] == field:
                d = d2(p, hw[j])
                if d <= radius_sq and (found is None or (d, j) < found):
                    found = (d, j)
        return found
    match_of_a, match_of_b, dist = [-1] * len(a_hw), [-1] * len(b_hw), [-1] * len(a_hw)
    for i in range(len(a_hw)):
        to_b = best(a_hw[i], a_field[i], b_hw, b_field)
        if to_b is None:
            continue
        back = best(b_hw[to_b[1]], b_field[to_b[1]], a_hw, a_field)
        if back[1] == i:
            match_of_a[i], match_of_b[to_b[1]], dist[i] = to_b[1], i, to_b[0]
    return match_of_a, match_of_b, dist


def plain_molecules(tables, radius_sq, offsets=None):
    """The sequential definition of the merge: (member [K][M], field [M], hw [M]) as lists.  tables: per channel (hw, field)."""
    K = len(tables)
    offsets = offsets or [(0, 0)] * K
    moved = [([(int(h) + o[0], int(w) + o[1]) for h, w in hw], [int(f) for f in field]) for (hw, field), o in zip(tables, offsets)]
    mols = [{"hw": p, "field": f, "member": [t] + [-1] * (K - 1)} for t, (p, f) in enumerate(zip(*moved[0]))]
    for k in range(1, K):
        hw, field = moved[k]
        _, match_of_b, _ = plain_match([m["hw"] for m in mols], [m["field"] for m in mols], hw, field, radius_sq)
        for t, a in enumerate(match_of_b):
            if a >= 0:
                mols[a]["member"][k] = t
        for t, a in enumerate(match_of_b):
            if a < 0:
                mols.append({"hw": hw[t], "field": field[t], "member": [-1] * k + [t] + [-1] * (K - 1 - k)})
    mols.sort(key=lambda m: m["field"])                            # (stable)
    return [[m["member"][k] for m in mols] for k in range(K)], [m["field"] for m in mols], [list(m["hw"]) for m in mols]


# ---- from two tables to the kernel's arguments ----

def segments(a_hw, a_field, b_hw, b_field):
    """(a_hw int64 [n_a, 2], a_seg int32, a_off int64, b_hw, b_seg, b_off) with the tracks grouped stably by field, the
    segments the sorted union of the fields, plus the sorted fields of a and b."""
    a_hw, b_hw = np.asarray(a_hw, np.int64).reshape(-1, 2), np.asarray(b_hw, np.int64).reshape(-1, 2)
    a_field, b_field = np.asarray(a_field, np.int64).reshape(-1), np.asarray(b_field, np.int64).reshape(-1)
    ids = sorted(set(a_field.tolist()) | set(b_field.tolist()))
    out = []
    for hw, field in ((a_hw, a_field), (b_hw, b_field)):
        order = sorted(range(len(field)), key=lambda t: field[t])  # (stable)
        seg = np.array([ids.index(field[t]) for t in order], np.int32)
        off = np.array([sum(1 for s in seg if s < j) for j in range(len(ids) + 1)], np.int64)
        out += [hw[order].reshape(-1, 2), seg, off]
    return tuple(out)


def lattice(rng, n, side, low=0):
    return rng.integers(low, low + side, (n, 2))


def _sizes_case():
    """Fields of 1, 63, 64, 65 and 130 tracks in one call (323 a's: two blocks of 256, waves that straddle field boundaries)."""
    rng = np.random.default_rng(7)
    sizes = [1, 63, 64, 65, 130]
    field = np.repeat(np.arange(5) * 2 + 1, sizes)
    a = lattice(rng, len(field), 24)
    b = a + rng.integers(-1, 2, a.shape)
    keep = rng.random(len(field)) < 0.9
    return a, field, b[keep][::-1], field[keep][::-1], 4


def _fuzz_case(seed, fields, per_field, side=40, radius_sq=4):
    rng = np.random.default_rng(seed)
    na, nb = fields * per_field, fields * per_field - 17
    return (lattice(rng, na, side), rng.integers(0, fields, na), lattice(rng, nb, side), rng.integers(0, fields, nb), radius_sq)


def match_cases():
    """{name: (a_hw, a_field, b_hw, b_field, radius_sq)}: the smallest shapes at which the match can go wrong."""
    far = 2 * (2 * BIG) ** 2                                     # d2 of two opposite corners: 2^63 - 2^34 + 8
    cases = {
        "no a": ([], [], [(1, 1), (2, 2), (3, 3)], [0, 0, 1], 4),
        "no b": ([(1, 1), (2, 2)], [0, 1], [], [], 4),
        "nothing": ([], [], [], [], 4),
        "one each": ([(5, 5)], [3], [(6, 6)], [3], 4),
        "one each, too far": ([(5, 5)], [3], [(7, 7)], [3], 4),
        "one each, other fields": ([(5, 5)], [3], [(5, 5)], [4], 4),
        "a field in one channel only": ([(0, 0), (9, 9), (0, 0)], [0, 1, 1], [(0, 0), (9, 9), (0, 0)], [1, 2, 2], 4),
        "two b at one distance": ([(0, 0)], [0], [(0, 1), (1, 0), (0, -1)], [0, 0, 0], 1),
        "two a at one distance": ([(0, 1), (1, 0), (0, -1)], [0, 0, 0], [(0, 0)], [0], 1),
        "duplicate positions": ([(5, 5), (5, 5), (8, 8)], [0, 0, 0], [(5, 5), (5, 5), (8, 8), (8, 8)], [0, 0, 0, 0], 4),
        # a0's best b is b0, which prefers a1: a0 stays alone although b1 lies within the radius
        "no second choice": ([(0, 0), (0, 1)], [0, 0], [(0, 1), (0, -2)], [0, 0], 4),
        "no second choice, longer": ([(0, 0), (0, 3), (0, 6)], [0, 0, 0], [(0, 2), (0, 5), (0, 8)], [0, 0, 0], 4),
        "at the radius": ([(0, 0), (10, 10)], [0, 0], [(0, 2), (11, 12)], [0, 0], 4),
        "radius 0": ([(0, 0), (3, 3), (5, 5)], [0, 0, 0], [(0, 1), (3, 3), (5, 5), (5, 5)], [0, 0, 0, 0], 0),
        "radius 2.5": ([(0, 0), (10, 10), (20, 20)], [0, 0, 0], [(1, 2), (12, 12), (20, 23)], [0, 0, 0], 6),
        "negative positions": ([(-5, -5), (-9, 4), (3, -7)], [0, 0, 0], [(-6, -5), (-9, 5), (4, -8), (-100, -100)], [0, 0, 0, 0], 2),
        "the corners": ([(BIG, -BIG), (BIG, BIG)], [0, 0], [(-BIG, BIG), (BIG - 1, BIG)], [0, 0], 4),
        "across the plane": ([(BIG, -BIG)], [0], [(-BIG, BIG)], [0], far),
        "across the plane, one short": ([(BIG, -BIG)], [0], [(-BIG, BIG)], [0], far - 1),
        "any distance": ([(BIG, -BIG), (0, 0)], [0, 0], [(-BIG, BIG), (1, 1)], [0, 0], (1 << 63) - 1),
        "unsorted fields": ([(0, 0), (0, 0), (1, 1), (2, 2)], [7, 2, 7, 2], [(2, 2), (1, 1), (0, 0), (0, 0)], [2, 7, 2, 7], 0),
        "field sizes": _sizes_case(),
        "small fuzz": _fuzz_case(3, 3, 150, side=14),
    }
    return cases


def fuzz_case():
    """A few thousand tracks on a 40 x 40 lattice per field: ties are common.  (Too many for the plain loop: twin and kernel.)"""
    return _fuzz_case(11, 3, 1100)


def channel_tables(seed, K, n=70, fields=3, side=12):
    """K random channel tables (hw int64 [n_k, 2], field [n_k]) that share most positions up to a jitter, with fields that
    stand in any order, and per-channel integer offsets (some negative) that the tables are shifted against."""
    rng = np.random.default_rng(seed)
    base, base_field = lattice(rng, n, side, -3), rng.integers(0, fields, n) * 5 - 5
    offsets = [(0, 0), (3, -2), (-4, 0), (-1, -1)][:K]
    tables = []
    for k in range(K):
        keep = rng.permutation(np.flatnonzero(rng.random(n) < 0.8))
        extra = int(rng.integers(0, 6))
        hw = np.concatenate([base[keep] + rng.integers(-1, 2, (len(keep), 2)), lattice(rng, extra, side, -3)]) - np.array(offsets[k])
        field = np.concatenate([base_field[keep], rng.integers(0, fields + 1, extra) * 5 - 5])
        tables.append((hw.astype(np.int64), field.astype(np.int64)))
    return tables, offsets


# ---- a simulated two-colour experiment as track tables ----

FIXED = dict(s=0.1, sc=3, s2=0.05, beta={"K": 70000.0, "C": 30000.0}, beta_sigma={"K": 0.2, "C": 0.25}, ddif=[0, 0.3] + [0.3] * 5)
SIGMA = {"K": 0.2, "C": 0.25}


@functools.lru_cache(maxsize=None)
def experiment(n=240, seed=9, per_field=60):
    """({letter: track table}, {letter: the molecule of every track}) of n simulated molecules of GAKCAK labelled at K and C
    over 8 frames (multilabel_records(host=True)): a molecule has a track in a channel where the channel is lit at frame 0, but
    for a few that are dropped; the molecules stand 6 pixels apart, a track's position is its molecule's plus a jitter of at
    most one pixel in the second channel (d2 <= 2, below radius 2), intensities are rounded as the CSV reader rounds them, and
    every 11th track of a channel gets a category that fails the downstep filter."""
    from fluorosequencingimageanalysis_amd import peptide_simulator as PS
    rec = PS.multilabel_records("GAKCAK", "KC", 1, 6, n, seed=seed, host=True, p=0.9, b=0.1, u=0.15, **FIXED)
    rng = np.random.default_rng(seed)
    letters = tuple(rec["labels"])
    F = rec["counts"].shape[2]
    mol = np.arange(n)
    field, cell = mol // per_field + 1, mol % per_field
    pos = np.stack([cell // 10 * 6 + 3, cell % 10 * 6 + 3], axis=1)
    tables, molecule_of = {}, {}
    for k, L in enumerate(letters):
        lit = rec["counts"][k][:, 0] != 0
        at = np.flatnonzero(lit & (rng.random(n) < 0.93))
        at = at[rng.permutation(len(at))] if k else at            # (the second channel's tracks in another order, field by field)
        at = at[np.argsort(field[at], kind="stable")]
        words = rec["category"][k][at].astype(np.uint64)
        words[5::11] = np.uint64(0b101)                             # ON, OFF, ON: not a downstep
        hw = pos[at] + (rng.integers(-1, 2, (len(at), 2)) if k else 0)
        tables[L] = (np.rint(rec["intensity"][k][at]).astype(np.float64), words, field[at].astype(np.int64), hw.astype(np.int64),
                     np.arange(1, len(at) + 1, dtype=np.int64) + k * 1000)
        molecule_of[L] = at
    assert F == 8
    return tables, molecule_of


def photometries_of(tables, channel_of):
    """The tables as the nested dict that lognormal.write_photometries_dict_to_csv writes: {channel: {field: {(h, w): ...}}}."""
    d = {}
    for L, (intensity, words, field, hw, row) in tables.items():
        F = intensity.shape[1]
        for I, c, f, (h, w), r in zip(intensity.tolist(), words.tolist(), field.tolist(), hw.tolist(), row.tolist()):
            d.setdefault(channel_of[L], {}).setdefault(f, {})[(h, w)] = (tuple(bool((c >> j) & 1) for j in range(F)),
                                                                         tuple(int(x) for x in I), r)
    return d
