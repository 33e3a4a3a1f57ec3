"""NumPy / math twin of the peptide Monte-Carlo kernel (include/fsq_peptide_sim.h): Philox4x32-10 draws, numpy's legacy polar
normals, and the per-molecule walk of the reference's peptide_simulator.py (simulate_dye_counts :44-169, 251-277 and
simulate_photometries :333-353, 405-434) for one label letter.  math.log / math.exp / math.sqrt are the libm calls the
reference makes, so every float here has the reference's bits under the same draws.

Draw j of a (molecule, stream) pair: Philox block j >> 1 at counter (block, molecule & 0xffffffff, molecule >> 32, stream)
and key (seed & 0xffffffff, seed >> 32); even j takes words (0, 1), odd j words (2, 3); the uniform is CPython's
((a >> 5) * 67108864 + (b >> 6)) / 2**53.  Stream 0: the chemistry (random.random() of simulate_dye_counts); stream 1: the
superdye draws; stream 2: the uniforms behind the normals.

Also the engine of `python -m fluorosequencingimageanalysis_amd.simulate_peptide --host`."""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xffffffff
CAUSE_NONE, CAUSE_DUD, CAUSE_DESTRUCTION, CAUSE_EDMAN, CAUSE_STRIP = 0, 1, 2, 3, 4
CAUSE_NAMES = {CAUSE_DUD: 'dye dud', CAUSE_DESTRUCTION: 'dye destruction', CAUSE_EDMAN: 'edman', CAUSE_STRIP: 'surface strip'}
MAX_FRAMES, MAX_LENGTH, MAX_LABELLED = 64, 64, 15
OFF_LOG = -10000.0

KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK32,) * 4, (MASK32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox(counter, key):
    """Philox4x32-10 of one counter (4 words) under one key (2 words): 4 words, Python ints."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def philox_np(counters, keys):
    """philox for uint32 [n, 4] counters and uint32 [n, 2] (or [2]) keys: uint32 [n, 4]."""
    c = np.asarray(counters, dtype=np.uint64).reshape(-1, 4)
    k = np.broadcast_to(np.asarray(keys, dtype=np.uint64).reshape(-1, 2), (len(c), 2))
    c0, c1, c2, c3 = (c[:, i].copy() for i in range(4))
    k0, k1 = k[:, 0].copy(), k[:, 1].copy()
    m, sh = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & m, (p0 >> sh) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(W0)) & m, (k1 + np.uint64(W1)) & m
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def _uniform(a, b):
    return ((a >> 5) * 67108864 + (b >> 6)) / 9007199254740992.0


def uniform(seed, molecule, stream, j):
    """Draw j of (molecule, stream)."""
    w = philox((j >> 1, molecule & MASK32, molecule >> 32, stream), (seed & MASK32, seed >> 32))
    return _uniform(w[0], w[1]) if j % 2 == 0 else _uniform(w[2], w[3])


def uniforms_np(seed, molecules, stream, n_draws):
    """The first n_draws draws of `stream` for every molecule: float64 [n, n_draws]."""
    mol = np.asarray(molecules, dtype=np.uint64).reshape(-1)
    n, nb = len(mol), (int(n_draws) + 1) // 2
    if n == 0 or nb == 0:
        return np.zeros((n, 0))
    c = np.empty((n, nb, 4), dtype=np.uint64)
    c[:, :, 0] = np.arange(nb, dtype=np.uint64)[None, :]
    c[:, :, 1] = (mol & np.uint64(MASK32))[:, None]
    c[:, :, 2] = (mol >> np.uint64(32))[:, None]
    c[:, :, 3] = stream
    w = philox_np(c.reshape(-1, 4), (seed & MASK32, seed >> 32)).astype(np.uint64).reshape(n, nb, 2, 2)
    u = ((w[..., 0] >> np.uint64(5)) * np.uint64(67108864) + (w[..., 1] >> np.uint64(6))).astype(np.float64) / 9007199254740992.0
    return u.reshape(n, 2 * nb)[:, :int(n_draws)]


class Stream(object):
    """The draws of one (molecule, stream) pair in order; .j is the number consumed.  `row`: draws already computed."""

    def __init__(self, seed, molecule, stream, row=()):
        self.key, self.molecule, self.stream, self.row, self.j = seed, molecule, stream, row, 0

    def __call__(self):
        j = self.j
        self.j = j + 1
        if j < len(self.row):
            return self.row[j]
        return uniform(self.key, self.molecule, self.stream, j)

    random = __call__

    def seed(self, *a):                     # (the reference seeds at the top of simulate_dye_counts; the draws here are explicit)
        pass


class Normals(object):
    """numpy's legacy polar Gaussian (legacy_gauss) on a Stream, starting with an empty cache."""

    def __init__(self, stream):
        self.u, self.cached = stream, None

    def __call__(self):
        if self.cached is not None:
            z, self.cached = self.cached, None
            return z
        while True:
            x1 = 2.0 * self.u() - 1.0
            x2 = 2.0 * self.u() - 1.0
            r2 = x1 * x1 + x2 * x2
            if 0.0 < r2 < 1.0:
                break
        f = math.sqrt(-2.0 * math.log(r2) / r2)
        self.cached = f * x1
        return f * x2


def lognormal(normals, mean, sigma):
    """np.random.lognormal(mean, sigma) from its Gaussian: exp(mean + sigma * z), the multiply and the add rounded apart."""
    return math.exp(mean + sigma * normals())


def check_shape(length, label_mask, num_mocks, num_edmans, ddif):
    """(labelled positions, frames) after the checks fsq_peptide_simulate makes."""
    if not 1 <= length <= MAX_LENGTH:
        raise ValueError("the peptide's length must be in 1 .. 64")
    if label_mask < 0 or label_mask >> length:
        raise ValueError("a labelled position beyond the peptide")
    pos = [i for i in range(length) if (label_mask >> i) & 1]
    if len(pos) > MAX_LABELLED:
        raise ValueError("at most 15 labelled residues")
    if num_mocks < 0 or num_edmans < 0 or num_mocks + num_edmans + 1 > MAX_FRAMES:
        raise ValueError("num_mocks + num_edmans + 1 must be in 1 .. 64 frames")
    if len(ddif) < len(pos):
        raise ValueError("ddif is shorter than the number of labelled residues")
    return pos, num_mocks + num_edmans + 1


def max_chemistry_draws(n_labelled, num_mocks, num_edmans):
    return 2 * n_labelled + num_mocks * (1 + n_labelled) + num_edmans * (2 + n_labelled)


def walk(pos, length, num_mocks, num_edmans, p, per_cycle_b, u, s, sc, s2, rnd):
    """The chemistry of one molecule on the stream-0 draws `rnd`: (counts, loss_cycle, loss_cause, edman_fail)."""
    L = len(pos)
    live = [True] * L
    loss_cycle, loss_cause = [0] * L, [CAUSE_NONE] * L
    for k in range(L):                                              # dud (:105-120)
        if rnd() < u:
            live[k], loss_cycle[k], loss_cause[k] = False, 0, CAUSE_DUD
    for k in range(L):                                              # photobleach (:84-99)
        if live[k] and rnd() > per_cycle_b:
            live[k], loss_cycle[k], loss_cause[k] = False, 0, CAUSE_DESTRUCTION
    counts, nterm, fail = [sum(live)], 0, 0
    for c in range(1, num_mocks + num_edmans + 1):
        if c > num_mocks and nterm < length:                        # Edman (:47-75): draws only while residues remain
            if rnd() < p:
                for k in range(L):
                    if pos[k] == nterm and live[k]:
                        live[k], loss_cycle[k], loss_cause[k] = False, c, CAUSE_EDMAN
                nterm += 1
            else:
                fail |= 1 << c
        if rnd() < (s if c <= sc else s2):                          # strip (:153-169): one draw, every live dye goes
            for k in range(L):
                if live[k]:
                    live[k], loss_cycle[k], loss_cause[k] = False, c, CAUSE_STRIP
        for k in range(L):
            if live[k] and rnd() > per_cycle_b:
                live[k], loss_cycle[k], loss_cause[k] = False, c, CAUSE_DESTRUCTION
        counts.append(sum(live))
    return counts, loss_cycle, loss_cause, fail


def photometries(counts, log_beta, beta_sigma, ddif, superdye_rate, superdye_factor, rnd1, normals):
    """simulate_photometries(number=1) of one count row (:333-353, 405-434): the intensities, 0.0 where the count is 0."""
    F = len(counts)
    inc = [0] * F
    for d in range(1, F):
        for _ in range(counts[d - 1] - counts[d]):
            if rnd1() < superdye_rate:
                inc[d] += 1
    for _ in range(counts[-1]):
        if rnd1() < superdye_rate:
            inc[-1] += 1
    inc = [sum(inc[i:]) for i in range(F)]
    out = []
    for f, c in enumerate(counts):
        if c == 0:
            out.append(0.0)
            continue
        if superdye_rate == 0:
            mean = log_beta + math.log(c) - ddif[c - 1]
        else:
            mean = log_beta + math.log(c + inc[f] * superdye_factor) - ddif[c - 1]
        out.append(lognormal(normals, mean, beta_sigma))
    return out


def simulate(length, label_mask, num_mocks, num_edmans, p, per_cycle_b, u, s, sc, s2, log_beta, beta_sigma, ddif,
             superdye_rate=0.0, superdye_factor=1.0, seed=0, first_molecule=0, n_molecules=1):
    """The records of fsq_peptide_simulate as NumPy arrays: counts uint8 [n, frames], loss_cycle / loss_cause uint8
    [n, n_labelled], edman_fail uint64 [n] (bit c: the Edman of cycle c failed), intensity and log_intensity float64
    [n, frames], category uint64 [n] (bit f: count > 0 at frame f), n_draws int32 [n, 3]."""
    pos, F = check_shape(length, label_mask, num_mocks, num_edmans, ddif)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must be in 0 .. 2^64 - 1")
    if not 0 <= superdye_rate <= 1:
        raise ValueError("superdye_rate must be between 0 and 1 (inclusive).")
    n, L = int(n_molecules), len(pos)
    if n < 0 or first_molecule < 0 or first_molecule + n > 1 << 63:
        raise ValueError("molecule ids must be in 0 .. 2^63 - 1")
    ddif = [float(x) for x in ddif]
    mols = [first_molecule + i for i in range(n)]
    u0 = uniforms_np(seed, mols, 0, max_chemistry_draws(L, num_mocks, num_edmans)).tolist()
    u1 = uniforms_np(seed, mols, 1, L).tolist()
    u2 = uniforms_np(seed, mols, 2, 2 * F + 8).tolist() if L else [()] * n
    out = {"counts": np.zeros((n, F), np.uint8), "loss_cycle": np.zeros((n, L), np.uint8), "loss_cause": np.zeros((n, L), np.uint8),
           "edman_fail": np.zeros(n, np.uint64), "intensity": np.zeros((n, F)), "log_intensity": np.full((n, F), OFF_LOG),
           "category": np.zeros(n, np.uint64), "n_draws": np.zeros((n, 3), np.int32)}
    for i, mol in enumerate(mols):
        r0, r1, r2 = Stream(seed, mol, 0, u0[i]), Stream(seed, mol, 1, u1[i]), Stream(seed, mol, 2, u2[i])
        counts, lc, cause, fail = walk(pos, length, num_mocks, num_edmans, p, per_cycle_b, u, s, sc, s2, r0)
        inten = photometries(counts, log_beta, beta_sigma, ddif, superdye_rate, superdye_factor, r1, Normals(r2))
        out["counts"][i], out["loss_cycle"][i], out["loss_cause"][i] = counts, lc, cause
        out["edman_fail"][i] = fail
        out["intensity"][i] = inten
        out["log_intensity"][i] = [math.log(x) if x > 0 else OFF_LOG for x in inten]
        out["category"][i] = sum(1 << f for f, c in enumerate(counts) if c)
        out["n_draws"][i] = (r0.j, r1.j, r2.j)
    return out
