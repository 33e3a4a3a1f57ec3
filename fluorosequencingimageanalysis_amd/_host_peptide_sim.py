"""NumPy / math twin of the peptide Monte-Carlo kernel (include/fsq_peptide_sim.h): Philox4x32-10 draws, numpy's legacy polar
normals, and the per-molecule walk of the reference's peptide_simulator.py (simulate_dye_counts :44-169, 251-277 and
simulate_photometries :333-353, 405-434) for one label letter.  math.log / math.exp / math.sqrt are the libm calls the
reference makes, so every float here has the reference's bits under the same draws.

Draw j of a (molecule, stream) pair: Philox block j >> 1 at counter (block, molecule & 0xffffffff, molecule >> 32, stream)
and key (seed & 0xffffffff, seed >> 32); even j takes words (0, 1), odd j words (2, 3); the uniform is CPython's
((a >> 5) * 67108864 + (b >> 6)) / 2**53.  Stream 0: the chemistry (random.random() of simulate_dye_counts); stream 1: the
superdye draws; stream 2: the uniforms behind the normals.

Several label letters, one colour channel each (include/fsq_peptide_labels.h, `simulate_labels`).  Draw contract: stream 0
is the chemistry on the union of the channels' positions, in the same order - the reference draws once per residue whose
letter is in `labels`, whatever the letter; channel 0's photometry reads streams 1 and 2, channel k >= 1 streams 2 + 2k
(superdyes) and 3 + 2k (normals) - stream 3 is the proteome Monte-Carlo's; every channel of every molecule starts with an
empty Gaussian cache.  With one channel every table is `simulate`'s.  Order contract: the reference iterates a Python-2
dict of letters; the channels here are the sorted label letters, and a channel's draws do not depend on that order.

Also the engine of `python -m fluorosequencingimageanalysis_amd.simulate_peptide --host`."""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xffffffff
CAUSE_NONE, CAUSE_DUD, CAUSE_DESTRUCTION, CAUSE_EDMAN, CAUSE_STRIP = 0, 1, 2, 3, 4
CAUSE_NAMES = {CAUSE_DUD: 'dye dud', CAUSE_DESTRUCTION: 'dye destruction', CAUSE_EDMAN: 'edman', CAUSE_STRIP: 'surface strip'}
MAX_FRAMES, MAX_LENGTH, MAX_LABELLED, MAX_CHANNELS = 64, 64, 15, 4
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


def walk(pos, length, num_mocks, num_edmans, p, per_cycle_b, u, s, sc, s2, rnd, tap=None):
    """The chemistry of one molecule on the stream-0 draws `rnd`: (counts, loss_cycle, loss_cause, edman_fail).  tap(live), if
    given, sees the live flags of the labelled positions after every cycle (simulate_labels counts its channels there)."""
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
    if tap is not None:
        tap(live)
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
        if tap is not None:
            tap(live)
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


def superdye_stream(k):
    """The stream of channel k's superdye draws."""
    return 1 if k == 0 else 2 + 2 * k


def normal_stream(k):
    """The stream of the uniforms behind channel k's normals."""
    return 2 if k == 0 else 3 + 2 * k


def check_channels(length, channel_masks, num_mocks, num_edmans, ddif):
    """(union positions, the channel of each, frames) after the checks fsq_peptide_simulate_labels makes."""
    K = len(channel_masks)
    if not 1 <= K <= MAX_CHANNELS:
        raise ValueError("1 .. %d channels" % MAX_CHANNELS)
    if len(ddif) != K:
        raise ValueError("one ddif row per channel")
    union, F = 0, None
    for k, mask in enumerate(channel_masks):
        if mask & union:
            raise ValueError("a residue in two channels")
        union |= mask
        _, F = check_shape(length, mask, num_mocks, num_edmans, ddif[k])
    pos = [i for i in range(length) if (union >> i) & 1]
    return pos, [next(k for k, m in enumerate(channel_masks) if (m >> i) & 1) for i in pos], F


def counts_from_losses(channel_of, loss_cycle, loss_cause, K, frames):
    """The count rows [K][frames] the loss tables of one molecule imply: a dye is there at frame f iff its cause is none or
    its loss cycle is greater than f."""
    return [[sum(1 for j, ch in enumerate(channel_of) if ch == k and (loss_cause[j] == CAUSE_NONE or loss_cycle[j] > f))
             for f in range(frames)] for k in range(K)]


def simulate_labels(length, channel_masks, num_mocks, num_edmans, p, per_cycle_b, u, s, sc, s2, log_beta, beta_sigma, ddif,
                    superdye_rate, superdye_factor, seed=0, first_molecule=0, n_molecules=1):
    """The records of fsq_peptide_simulate_labels as NumPy arrays, K = len(channel_masks) and L the labelled residues of the
    union: counts uint8 [K, n, frames], loss_cycle / loss_cause uint8 [n, L], edman_fail uint64 [n], intensity and log_intensity
    float64 [K, n, frames], category uint64 [K, n], n_draws int32 [n, 1 + 2K].  log_beta, beta_sigma, ddif, superdye_rate and
    superdye_factor are sequences over the channels."""
    channel_masks = [int(m) for m in channel_masks]
    K = len(channel_masks)
    pos, channel_of, F = check_channels(length, channel_masks, num_mocks, num_edmans, ddif)
    if not (len(log_beta) == len(beta_sigma) == len(superdye_rate) == len(superdye_factor) == K):
        raise ValueError("one value per channel")
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must be in 0 .. 2^64 - 1")
    if not all(0 <= r <= 1 for r in superdye_rate):
        raise ValueError("superdye_rate must be between 0 and 1 (inclusive).")
    n, L = int(n_molecules), len(pos)
    if n < 0 or first_molecule < 0 or first_molecule + n > 1 << 63:
        raise ValueError("molecule ids must be in 0 .. 2^63 - 1")
    ddif = [[float(x) for x in row] for row in ddif]
    mols = [first_molecule + i for i in range(n)]
    u0 = uniforms_np(seed, mols, 0, max_chemistry_draws(L, num_mocks, num_edmans)).tolist()
    per = [bin(m).count("1") for m in channel_masks]
    u1 = [uniforms_np(seed, mols, superdye_stream(k), per[k]).tolist() for k in range(K)]
    u2 = [uniforms_np(seed, mols, normal_stream(k), 2 * F + 8).tolist() if per[k] else [()] * n for k in range(K)]
    out = {"counts": np.zeros((K, n, F), np.uint8), "loss_cycle": np.zeros((n, L), np.uint8), "loss_cause": np.zeros((n, L), np.uint8),
           "edman_fail": np.zeros(n, np.uint64), "intensity": np.zeros((K, n, F)), "log_intensity": np.full((K, n, F), OFF_LOG),
           "category": np.zeros((K, n), np.uint64), "n_draws": np.zeros((n, 1 + 2 * K), np.int32)}
    for i, mol in enumerate(mols):
        r0 = Stream(seed, mol, 0, u0[i])
        rows = [[] for _ in range(K)]

        def tap(live):
            for k in range(K):
                rows[k].append(sum(1 for j, on in enumerate(live) if on and channel_of[j] == k))
        _, lc, cause, fail = walk(pos, length, num_mocks, num_edmans, p, per_cycle_b, u, s, sc, s2, r0, tap)
        out["loss_cycle"][i], out["loss_cause"][i], out["edman_fail"][i] = lc, cause, fail
        out["n_draws"][i, 0] = r0.j
        for k in range(K):
            r1 = Stream(seed, mol, superdye_stream(k), u1[k][i])
            r2 = Stream(seed, mol, normal_stream(k), u2[k][i])
            inten = photometries(rows[k], log_beta[k], beta_sigma[k], ddif[k], superdye_rate[k], superdye_factor[k], r1, Normals(r2))
            out["counts"][k, i] = rows[k]
            out["intensity"][k, i] = inten
            out["log_intensity"][k, i] = [math.log(x) if x > 0 else OFF_LOG for x in inten]
            out["category"][k, i] = sum(1 << f for f, c in enumerate(rows[k]) if c)
            out["n_draws"][i, 1 + 2 * k:3 + 2 * k] = (r1.j, r2.j)
    return out
