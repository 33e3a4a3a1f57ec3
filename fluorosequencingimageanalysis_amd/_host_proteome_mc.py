"""NumPy / standard-library twin of the proteome Monte-Carlo (include/fsq_proteome_mc.h): the reference's MCsimlib.py from
proteins to the signals that identify them - cleave, attach, homogenize (:88-279), random_signal (:863-1074), the
(signal, protein) counts a SignalTrie holds and the scan of find_uniques (:1434-1474) and find_uniques_absolute (:1495-1514).

ORDER CONTRACTS.  Wherever the reference iterates `windows` (a dict, whose order Python 2 leaves open) the twin iterates
sorted(windows).  A signal is returned sorted by position, then by acid in that order (the reference leaves ties to the
iteration order of a set).  Proteins are scanned in ascending protein index: the insertion order of `peptides`, which is the
first-seen order of the reference's signal_count dicts when proteins are sampled one after the other.

DRAW CONTRACT.  Sample g = first_sample + peptide_index * sample_size + j reads stream 3 (STREAM) of item g under `seed`
through _host_peptide_sim.uniform, in the order in which the reference calls random.random():
  draw i, i < n_labels                    the dud draw of label i in "for acid in order: head occurrences by position, then
                                          tail occurrences";
  n_labels + r                            the Edman draw of the r-th surviving head label by position;
  n_labels + n_surviving_head + r         its bleach draw;
  n_labels + 2 n_surviving_head + r       the bleach draw of the r-th surviving tail label in acid-major order.

THE KEY.  Per acid a with windows W_a (positions 1 .. 63): exposures E_a = W_a | (W_a - 1), observable positions
O_a = {x : x in E_a and x - 1 in E_a}; the pair (x, a) is bit base_a + rank of x in O_a, acids in order.  Key 0 is the empty
signal, which no trie stores."""
import functools
import math
import random as _random

import numpy as np

from . import _host_peptide_sim as PSIM

STREAM = 3
MAX_PAIRS, MAX_LABELS, MAX_HEAD, MAX_POSITION, MAX_ACIDS, MAX_ROW = 64, 64, 255, 63, 8, 4096
MAX_EXPOSURES = 64
DUD = 'x'                                   # the reference's placeholder for a residue whose fluor is dead
RATIO_NONE, RATIO_NUMBER, RATIO_ABSENT = 0, 1, 2        # the ratio clause of the scan (ABSENT: find_uniques_absolute)


# ---- preprocessing (:88-279) ----

def homogenize(peptides, substitute_acid, target_acids):
    """:88-119.  Every replace starts from the original sequence, so only the last of target_acids is replaced."""
    out = {}
    for protein in peptides:
        sequence = peptides[protein]
        for acid in target_acids:
            homogenized_sequence = sequence.replace(acid, substitute_acid)
        out.setdefault(protein, homogenized_sequence)
    return out


def cleave(peptides, cleave_acid, silent=True):
    """:121-190.  Cuts after every cleave_acid; empty pieces and proteins without a piece are left out."""
    out = {}
    for protein in peptides:
        if not peptides[protein]:
            continue
        pieces = peptides[protein].split(cleave_acid)
        for index in range(len(pieces) - 1):
            pieces[index] += cleave_acid
        if pieces[-1] == '':
            pieces.pop()
        pieces = [piece for piece in pieces if piece]
        if pieces:
            out.setdefault(protein, tuple(pieces))
    return out


def attach(peptides, attach_acid, silent=True):
    """:192-263.  (head, tail) at the first attach_acid; 'cterm' attaches every peptide by its end (an empty tail)."""
    out = {}
    if attach_acid == 'cterm':
        for protein in peptides:
            for sequence in peptides[protein]:
                out.setdefault(protein, []).append((sequence, ''))
            out[protein] = tuple(out[protein])      # (a protein with no peptide raises KeyError, as the reference does)
        return out
    for protein in peptides:
        for sequence in peptides[protein]:
            if attach_acid in sequence:
                at = sequence.find(attach_acid)
                out.setdefault(protein, []).append((sequence[:at], sequence[at:]))
        if protein in out:
            out[protein] = tuple(out[protein])
    return out


def homogenize_attached(peptides, substitute_acid, target_acids):
    """:265-279.  Unlike homogenize, every target acid is replaced."""
    out = {}
    for protein, sequences in peptides.items():
        for head, tail in sequences:
            for acid in target_acids:
                head = head.replace(acid, substitute_acid)
                tail = tail.replace(acid, substitute_acid)
            out.setdefault(protein, []).append((head, tail))
    for protein in out:
        out[protein] = tuple(out[protein])
    return out


def _deprecated(name):
    def f(*args, **kwargs):
        raise DeprecationWarning("%s raises DeprecationWarning in the reference as well" % name)
    f.__name__ = name
    return f


discard = _deprecated("discard")
truncate_heads = _deprecated("truncate_heads")
edman_failure_gaps_MP = _deprecated("edman_failure_gaps_MP")
monte_carlo_dictionary = _deprecated("monte_carlo_dictionary")
monte_carlo_dictionary_MP = _deprecated("monte_carlo_dictionary_MP")
monte_carlo_trie_MP = _deprecated("monte_carlo_trie_MP")


# ---- the key ----

class Layout(object):
    """The key layout of a windows dict: order (acids, sorted), W / E / O (bit x: position x), base (first key bit of an acid),
    n_bits."""

    def __init__(self, windows):
        self.order = tuple(sorted(windows))
        if len(self.order) > MAX_ACIDS:
            raise NotImplementedError("at most %d labelled acids (got %d)" % (MAX_ACIDS, len(self.order)))
        self.W, self.E, self.O, self.base = [], [], [], []
        bits = 0
        for acid in self.order:
            if not isinstance(acid, str) or len(acid) != 1 or acid == DUD:
                raise ValueError("an acid is one letter other than %r (got %r)" % (DUD, acid))
            w = 0
            for x in windows[acid]:
                if int(x) != x or not 1 <= x <= MAX_POSITION:
                    raise ValueError("window positions must be integers in 1 .. %d (got %r for %s)" % (MAX_POSITION, x, acid))
                w |= 1 << int(x)
            e = w | (w >> 1)
            o = e & (e << 1) & ((1 << 64) - 1)
            self.W.append(w), self.E.append(e), self.O.append(o), self.base.append(bits)
            bits += bin(o).count("1")
        self.n_bits = bits
        if bits > MAX_PAIRS:
            raise NotImplementedError("the windows have %d observable (position, acid) pairs; a key holds at most %d" % (bits, MAX_PAIRS))
        self.windows = {a: tuple(sorted(set(int(x) for x in windows[a]))) for a in self.order}

    def bit(self, x, acid):
        """The key bit of (x, acid), or -1 where the pair is not observable."""
        a = self.order.index(acid)
        if not 0 <= x < 64 or not (self.O[a] >> x) & 1:
            return -1
        return self.base[a] + bin(self.O[a] & ((1 << x) - 1)).count("1")

    def exposures(self, a):
        return [x for x in range(64) if (self.E[a] >> x) & 1]

    def bit_table(self):
        """int8 [acids, 66]: bit(x, acid) for x = 0 .. 65 (-1 beyond 63)."""
        t = np.full((max(len(self.order), 1), 66), -1, np.int8)
        for a, acid in enumerate(self.order):
            for x in range(64):
                t[a, x] = self.bit(x, acid)
        return t


def layout_of(windows):
    return windows if isinstance(windows, Layout) else Layout(windows)


def key_of(signal, layout):
    key = 0
    for x, acid in signal:
        bit = layout.bit(x, acid) if acid in layout.order else -1
        if bit < 0:
            raise ValueError("(%r, %r) is not observable through these windows" % (x, acid))
        key |= 1 << bit
    return key


def signal_of(key, layout):
    key = int(key)
    if key < 0 or key >> layout.n_bits:
        raise ValueError("key %#x has bits beyond the layout's %d" % (key, layout.n_bits))
    out = []
    for a, acid in enumerate(layout.order):
        xs = [x for x in range(64) if (layout.O[a] >> x) & 1]
        out.extend((x, a, acid) for r, x in enumerate(xs) if (key >> (layout.base[a] + r)) & 1)
    return tuple((x, acid) for x, a, acid in sorted(out))


def canonical(signal, order):
    """A signal of the reference in the twin's order: by position, then by acid in `order`."""
    order = list(order)
    return tuple(sorted(signal, key=lambda g: (g[0], order.index(g[1]))))


# ---- the tables ----

def _dp(d, e, p):
    """:42-53 in Python 2's arithmetic: an exact integer binomial, then * p**d * q**e left to right."""
    q = 1.0 - p
    return (math.factorial(d - 1 + e) // (math.factorial(e) * math.factorial(d - 1)) * p**d * q**e)


def edman_row(p, d):
    """The running sums of _dp(d, e, p), e = 0, 1, ... as the loop of :979-989 forms them, up to and including the first that
    adds nothing.  The delay of a draw r is the first e with row[e] >= r, else len(row)."""
    p = float(p)
    q = 1.0 - p
    row, binom, e = [], 1, 0
    accumulator, prior = 0.0, -1.0
    try:
        pd = p**d
        while accumulator - prior > 0.0:
            prior = accumulator
            accumulator += binom * pd * q**e
            row.append(accumulator)
            e += 1
            binom = binom * (d - 1 + e) // e
            if len(row) > MAX_ROW:
                raise NotImplementedError("the Edman delay row of p=%r, d=%d has more than %d entries" % (p, d, MAX_ROW))
    except OverflowError:
        raise NotImplementedError("the Edman delay row of p=%r, d=%d overflows a double" % (p, d))
    return row


@functools.lru_cache(maxsize=8)
def _edman_table(p, max_d):
    rows = [[]] + [edman_row(p, d) for d in range(1, max_d + 1)]
    start = np.zeros(len(rows) + 1, np.int64)
    start[1:] = np.cumsum([len(r) for r in rows])
    values = np.array([v for r in rows for v in r], np.float64)
    start.setflags(write=False), values.setflags(write=False)
    return start, values


def edman_table(p, max_d):
    """(start int64 [max_d + 2], values float64): row d = values[start[d] : start[d + 1]], d = 1 .. max_d (row 0 is empty).
    Read-only arrays: the last few tables are kept."""
    if not 0.0 <= float(p) <= 1.0:
        raise ValueError("p must be in [0, 1]")
    if not 0 <= int(max_d) <= MAX_HEAD:
        raise NotImplementedError("a gap of %d residues; a head has at most %d" % (max_d, MAX_HEAD))
    return _edman_table(float(p), int(max_d))


def bleach_table(b, n=MAX_EXPOSURES):
    """T[s] = (sum over k <= s of e**(-b k)) * (1 - e**-b), summed in order (:1035-1038): a fluor bleaches at the first
    exposure s with T[s] >= r."""
    b = float(b)
    if not b >= 0.0:
        raise ValueError("b must not be negative")
    out, accumulator = np.empty(n, np.float64), 0.0
    for s in range(n):
        accumulator += math.e**(-b * s)
        out[s] = accumulator * (1 - math.e**-b)
    return out


def delay_of(row, r):
    for e, acc in enumerate(row):
        if acc >= r:
            return e
    return len(row)


# ---- one signal (:863-1074) ----

def random_signal(peptide, p, b, u, windows, draws=None):
    """The reference's random_signal on the draws of `draws` (a callable standing in for random.random)."""
    rnd = draws or _random.random
    p, b, u = float(p), float(b), float(u)
    order = sorted(windows)
    head, tail = peptide
    for acid in order:                                                      # duds (:910-933)
        head = ''.join(c if c != acid or rnd() > u else DUD for c in head)
        tail = ''.join(c if c != acid or rnd() > u else DUD for c in tail)
    gaps = tuple((index + 1, acid) for index, acid in enumerate(head) if acid in windows)
    modified = list(gaps)
    cumulative_e = 0
    for index, gap in enumerate(gaps):                                      # Edman delays (:960-995)
        d = gaps[index][0] - gaps[index - 1][0] if index > 0 else gaps[index][0]
        random_point = rnd()
        e, accumulator, prior = 0, 0.0, -1.0
        while accumulator - prior > 0.0:
            prior = accumulator
            accumulator += _dp(d, e, p)
            if accumulator >= random_point:
                break
            e += 1
        cumulative_e += e
        modified[index] = (gap[0] + cumulative_e, gap[1])
    gaps = tuple(modified)
    for index, gap in enumerate(gaps):                                      # head bleaching (:1007-1040)
        random_point = rnd()
        accumulator = 0.0
        exposures = sorted(set([x for x in windows[gap[1]] if x < gap[0] - 1] + [x - 1 for x in windows[gap[1]] if x - 1 < gap[0] - 1]))
        for survival, position in enumerate(exposures):
            accumulator += math.e**(-b * survival)
            if accumulator * (1 - math.e**-b) >= random_point:
                modified[index] = (position + 1, gap[1])
                break
    for acid in [acid for acid in order for _ in range(tail.count(acid))]:  # tail bleaching (:1044-1056)
        random_point = rnd()
        accumulator = 0.0
        exposures = sorted(set([x for x in windows[acid]] + [x - 1 for x in windows[acid]]))
        for survival, position in enumerate(exposures):
            accumulator += math.e**(-b * survival)
            if accumulator * (1 - math.e**-b) >= random_point:
                modified.append((position + 1, acid))
                break
    kept = set()
    for acid in order:                                                      # the windows (:1062-1071)
        exposures = set([x for x in windows[acid]] + [x - 1 for x in windows[acid]])
        kept.update(gap for gap in modified if gap[1] == acid and gap[0] in exposures and gap[0] - 1 in exposures)
    return canonical(kept, order)


def sample_signal(peptide, p, b, u, windows, seed, sample):
    """(signal, draws consumed) of sample id `sample` under the draw contract."""
    stream = PSIM.Stream(seed, sample, STREAM)
    return random_signal(peptide, p, b, u, windows, stream), stream.j


# ---- the table of peptides ----

def peptide_table(peptides, windows):
    """Attached peptides {protein: ((head, tail), ...)} as flat arrays: names (proteins in dict order), layout, protein int32
    [n], n_head int32 [n] (head labels), label_start int64 [n + 1] and labels uint32 [total].  A peptide's labels stand in walk
    order - head labels by position, then tail labels acid-major; entry k holds in bits 0-7 the position (0: tail), bits 8-15
    the acid's index, bits 16-23 the label's dud draw, and in bits 24-29 the walk index of the label whose dud draw is k."""
    layout = layout_of(windows)
    names = list(peptides)
    protein, n_head, start, labels, heads = [], [], [0], [], []
    for pi, name in enumerate(names):
        for head, tail in peptides[name]:
            if len(head) > MAX_HEAD:
                raise NotImplementedError("a head of %d residues (protein %r); at most %d" % (len(head), name, MAX_HEAD))
            dud, walk_head, walk_tail = 0, [], []
            for a, acid in enumerate(layout.order):
                for i, c in enumerate(head):
                    if c == acid:
                        walk_head.append((i + 1, a, dud))
                        dud += 1
                for c in tail:
                    if c == acid:
                        walk_tail.append((0, a, dud))
                        dud += 1
            if dud > MAX_LABELS:
                raise NotImplementedError("a peptide of protein %r has %d labelled residues, head and tail together; at most %d"
                                          % (name, dud, MAX_LABELS))
            walk = sorted(walk_head) + walk_tail
            walk_of_draw = [0] * dud
            for k, (_, _, j) in enumerate(walk):
                walk_of_draw[j] = k
            labels.extend(x | (a << 8) | (j << 16) | (walk_of_draw[k] << 24) for k, (x, a, j) in enumerate(walk))
            protein.append(pi), n_head.append(len(walk_head)), start.append(len(labels)), heads.append(len(head))
    return {"names": names, "layout": layout, "protein": np.array(protein, np.int32), "n_head": np.array(n_head, np.int32),
            "label_start": np.array(start, np.int64), "labels": np.array(labels, np.uint32), "head_len": np.array(heads, np.int32)}


def max_gap(table):
    """The largest position of a head label: no Edman row beyond it is needed."""
    head = table["labels"][(table["labels"] & 0xff) != 0]
    return int((head & 0xff).max()) if len(head) else 0


# ---- many signals ----

def signals(table, p, b, u, sample_size, seed, first_sample=0, first_row=0, n_rows=None):
    """Rows first_row .. first_row + n_rows - 1 of the flattened [peptides][sample_size] space: (keys uint64, n_draws int32),
    what random_signal + key_of give sample for sample, vectorised over a peptide's samples."""
    p, b, u, S = float(p), float(b), float(u), int(sample_size)
    layout = table["layout"]
    total = len(table["protein"]) * S
    n = total - first_row if n_rows is None else int(n_rows)
    if S < 1 or first_row < 0 or n < 0 or first_row + n > total:
        raise ValueError("rows beyond the [peptides][sample_size] space")
    if not 0 <= seed < 1 << 64 or first_sample < 0 or first_sample + total > 1 << 64:
        raise ValueError("seed and sample ids must be in 0 .. 2^64 - 1")
    start, values = edman_table(p, max_gap(table))
    T = bleach_table(b)
    bit_of = layout.bit_table().astype(np.int64)
    exps = [np.array(layout.exposures(a), np.int64) for a in range(len(layout.order))]
    keys, n_draws = np.zeros(n, np.uint64), np.zeros(n, np.int32)
    g = first_row
    while g < first_row + n:
        pep = g // S
        hi = min(first_row + n, (pep + 1) * S)
        lab = table["labels"][table["label_start"][pep]:table["label_start"][pep + 1]].astype(np.int64)
        L, H = len(lab), int(table["n_head"][pep])
        m = hi - g
        items = np.array([first_sample + i for i in range(g, hi)], np.uint64)
        U = PSIM.uniforms_np(seed, items, STREAM, 3 * L) if L else np.zeros((m, 0))
        rows = np.arange(m)
        surv = np.zeros((m, L), bool)
        for k in range(L):
            surv[:, k] = U[:, (lab[k] >> 16) & 0xff] > u
        nsh = surv[:, :H].sum(axis=1)
        key = np.zeros(m, np.uint64)
        cum, prev, rank = np.zeros(m, np.int64), np.zeros(m, np.int64), np.zeros(m, np.int64)

        def emit(mask, x, a):
            bit = bit_of[a][np.clip(x, 0, 65)]
            ok = mask & (bit >= 0)
            key[ok] |= np.uint64(1) << bit[ok].astype(np.uint64)

        for k in range(H):
            live, x0, a = surv[:, k], int(lab[k] & 0xff), int((lab[k] >> 8) & 0xff)
            d = x0 - prev
            r = U[rows, np.minimum(L + rank, 3 * L - 1)]
            e = np.zeros(m, np.int64)
            for dv in np.unique(d[live]):
                sel = live & (d == dv)
                e[sel] = np.searchsorted(values[start[dv]:start[dv + 1]], r[sel], side='left')
            cum += np.where(live, e, 0)
            prev = np.where(live, x0, prev)
            gap = x0 + cum
            r2 = U[rows, np.minimum(L + nsh + rank, 3 * L - 1)]
            n_exp = np.searchsorted(exps[a], gap - 1, side='left')
            s = np.searchsorted(T, r2, side='left')
            hit = s < n_exp
            x = np.where(hit, exps[a][np.minimum(s, max(len(exps[a]) - 1, 0))] + 1 if len(exps[a]) else gap, gap)
            emit(live, x, a)
            rank += live
        trank = np.zeros(m, np.int64)
        for k in range(H, L):
            live, a = surv[:, k], int((lab[k] >> 8) & 0xff)
            r = U[rows, np.minimum(L + 2 * nsh + trank, 3 * L - 1)]
            s = np.searchsorted(T, r, side='left')
            if len(exps[a]):
                emit(live & (s < len(exps[a])), exps[a][np.minimum(s, len(exps[a]) - 1)] + 1, a)
            trank += live
        keys[g - first_row:hi - first_row] = key
        n_draws[g - first_row:hi - first_row] = L + 2 * nsh + trank
        g = hi
    return keys, n_draws


def row_proteins(table, sample_size, first_row, n_rows):
    return table["protein"][np.arange(first_row, first_row + n_rows) // int(sample_size)]


# ---- the tally and the scan ----

def tally(keys, proteins):
    """Sorted (key uint64, protein int32, count int64) triples of the rows whose key is not 0."""
    keys, proteins = np.asarray(keys, np.uint64), np.asarray(proteins, np.int64)
    keep = keys != 0
    keys, proteins = keys[keep], proteins[keep]
    order = np.lexsort((proteins, keys))
    keys, proteins = keys[order], proteins[order]
    if not len(keys):
        return np.zeros(0, np.uint64), np.zeros(0, np.int32), np.zeros(0, np.int64)
    new = np.ones(len(keys), bool)
    new[1:] = (keys[1:] != keys[:-1]) | (proteins[1:] != proteins[:-1])
    at = np.flatnonzero(new)
    return keys[at], proteins[at].astype(np.int32), np.diff(np.append(at, len(keys))).astype(np.int64)


def merge_triples(a, b):
    """The sum of two tallies."""
    k, p, c = (np.concatenate([x, y]) for x, y in zip(a, b))
    order = np.lexsort((p, k))
    k, p, c = k[order], p[order], c[order]
    new = np.ones(len(k), bool)
    new[1:] = (k[1:] != k[:-1]) | (p[1:] != p[:-1])
    return k[new], p[new], np.add.reduceat(c, np.flatnonzero(new)) if len(k) else c


def scan_counts(counts, ratio_mode, worst_ratio, absolute_min, has_max, maximum_secondary, demote):
    """One signal's scan (:1436-1474, :1497-1514) over [(protein, count), ...] in the given order:
    (best protein, best count, second protein or -1, second count, further proteins tied with second, tertiary total, passes).
    demote=False is the reference: a displaced best is not demoted to second, and a best whose count equals second's is listed
    among the ties.  demote=True (an extension) is the true top two - among equal counts the lower protein index first - with
    ties and tertiary taken over the remaining proteins."""
    best, second = (-1, 0), (-1, 0)
    if demote:
        ranked = sorted(counts, key=lambda pc: (-pc[1], pc[0]))
        best = ranked[0]
        second = ranked[1] if len(ranked) > 1 else (-1, 0)
    else:
        for protein, count in counts:
            if count > best[1]:
                best = (protein, count)
            elif count > second[1]:
                second = (protein, count)
    ties = tertiary = 0
    for protein, count in counts:
        if demote and protein == best[0]:
            continue
        if count == second[1] and protein != second[0]:
            ties += 1
        elif count < second[1]:
            tertiary += count
    if ratio_mode == RATIO_NONE:
        ratio_ok = second[0] == -1
    elif ratio_mode == RATIO_NUMBER:
        ratio_ok = second[1] == 0 or float(best[1]) / second[1] >= worst_ratio
    else:
        ratio_ok = True
    if ratio_mode == RATIO_ABSENT:
        max_ok = second[1] <= maximum_secondary
    else:
        max_ok = (not has_max) or second[0] == -1 or second[1] <= maximum_secondary
    return best[0], best[1], second[0], second[1], ties, tertiary, bool(best[1] >= absolute_min and ratio_ok and max_ok)


def scan_modes(worst_ratio, absolute_min, maximum_secondary, absolute=False):
    """(ratio_mode, worst_ratio, absolute_min, has_max, maximum_secondary) as floats and flags, for the twin and the kernel."""
    if absolute:
        return RATIO_ABSENT, 0.0, float(absolute_min), 1, float(maximum_secondary)
    return (RATIO_NONE if worst_ratio is None else RATIO_NUMBER, 0.0 if worst_ratio is None else float(worst_ratio),
            float(absolute_min), int(maximum_secondary is not None), 0.0 if maximum_secondary is None else float(maximum_secondary))


def segments(keys):
    """Starts of the runs of equal keys, with the end appended: int64 [n_signals + 1]."""
    keys = np.asarray(keys)
    new = np.ones(len(keys), bool)
    new[1:] = keys[1:] != keys[:-1]
    return np.append(np.flatnonzero(new), len(keys)).astype(np.int64)


UNIQUE_FIELDS = (("best_protein", np.int32), ("best_count", np.int64), ("second_protein", np.int32), ("second_count", np.int64),
                 ("n_ties", np.int32), ("tertiary", np.int64), ("passed", np.uint8))


def _uniques(triples, modes, demote):
    keys, proteins, counts = triples
    seg = segments(keys)
    out = {"key": np.asarray(keys, np.uint64)[seg[:-1]], "segment": seg}
    cols = [[] for _ in UNIQUE_FIELDS]
    pl, cl = np.asarray(proteins).tolist(), np.asarray(counts).tolist()
    for lo, hi in zip(seg[:-1].tolist(), seg[1:].tolist()):
        for col, v in zip(cols, scan_counts(list(zip(pl[lo:hi], cl[lo:hi])), *modes, demote)):
            col.append(v)
    for (name, dtype), col in zip(UNIQUE_FIELDS, cols):
        out[name] = np.array(col, dtype)
    return out


def uniques(triples, worst_ratio, absolute_min, maximum_secondary=None, demote=False):
    """find_uniques' scan (:1434-1474) for every signal of sorted (key, protein, count) triples: a dict of arrays over the
    signals - key, best_protein, best_count, second_protein (-1: None), second_count, n_ties, tertiary, passed - and `segment`,
    the signals' starts in the triples.  demote=True is an extension of the reference: see scan_counts."""
    return _uniques(triples, scan_modes(worst_ratio, absolute_min, maximum_secondary), demote)


def uniques_absolute(triples, minimum_best, maximum_secondary, demote=False):
    """find_uniques_absolute's scan (:1495-1514): best >= minimum_best and second <= maximum_secondary."""
    return _uniques(triples, scan_modes(None, minimum_best, maximum_secondary, absolute=True), demote)


def unique_lists(result, triples, demote=False):
    """The passing signals of a scan with their tie lists read off the sorted triples: {signal index: ((best, count),
    [(second, count), ties ...], tertiary)}, proteins by index (-1 for no second), the ties in ascending protein index."""
    _, proteins, counts = triples
    seg, out = result["segment"], {}
    for i in np.flatnonzero(result["passed"]).tolist():
        bp, sp, sc = int(result["best_protein"][i]), int(result["second_protein"][i]), int(result["second_count"][i])
        listed = [(sp, sc)]
        for j in range(int(seg[i]), int(seg[i + 1])):
            pj, cj = int(proteins[j]), int(counts[j])
            if cj == sc and pj != sp and not (demote and pj == bp):
                listed.append((pj, cj))
        out[i] = ((bp, int(result["best_count"][i])), listed, int(result["tertiary"][i]))
    return out


def unique_dict(result, triples, layout, names, demote=False):
    """The reference's dict of the passing signals: {signal: [(best, count), [(second, count), ties ...], tertiary]}, proteins
    by name (None for no second)."""
    name = lambda i: None if i < 0 else names[i]
    return {signal_of(triples[0][result["segment"][i]], layout): [(name(b[0]), b[1]), [(name(q), c) for q, c in listed], tertiary]
            for i, (b, listed, tertiary) in unique_lists(result, triples, demote).items()}


# ---- shorter runs (:1674-1759) ----

PROJECT, WITHIN = 0, 1                      # FSQ_PMC_PROJECT, FSQ_PMC_WITHIN
MODES = {"project": PROJECT, "within": WITHIN}
ALL_ONES = (1 << 64) - 1


def last_position(layout):
    """The last observable position of a layout (0: none): no signal changes under a cycle count at or above it."""
    return max([o.bit_length() - 1 for o in layout.O if o] + [0])


def cycle_masks(layout, cycles):
    """uint64 [len(cycles)]: the key bits of the pairs (x, acid) with x <= c - per acid, bits base_a .. base_a +
    popcount(O_a & ((1 << (c + 1)) - 1)) - 1.  key & mask is the signal a run of c Edman cycles would have shown
    (truncating_projection, :1697-1759); c = 0 gives 0, c at or above the last position every bit of the layout."""
    out = []
    for c in cycles:
        if int(c) != c or c < 0:
            raise ValueError("a cycle count is a non-negative integer (got %r)" % (c,))
        c, mask = min(int(c), 63), 0
        for a in range(len(layout.order)):
            mask |= ((1 << bin(layout.O[a] & ((1 << (c + 1)) - 1)).count("1")) - 1) << layout.base[a]
        out.append(mask)
    return np.array(out, np.uint64)


def mode_of(mode):
    if mode not in MODES:
        raise ValueError("mode is 'project' or 'within' (got %r)" % (mode,))
    return MODES[mode]


def project(triples, mask, mode="project"):
    """Sorted (key, protein, count) triples under one mask: 'project' re-tallies key & mask (truncating_projection), 'within'
    keeps the triples with key & ~mask == 0 (merge's cycles= filter, :1694).  Empty keys, negative proteins and zero counts are
    counted nowhere.  Sorted triples as tally returns them."""
    which = mode_of(mode)
    k, p, c = np.asarray(triples[0], np.uint64), np.asarray(triples[1], np.int32), np.asarray(triples[2], np.int64)
    mask = np.uint64(int(mask))
    k = np.where((k & ~mask) == 0, k, np.uint64(0)) if which == WITHIN else k & mask
    keep = (k != 0) & (p >= 0) & (c != 0)
    empty = (np.zeros(0, np.uint64), np.zeros(0, np.int32), np.zeros(0, np.int64))
    if not keep.any():
        return empty
    return merge_triples((k[keep], p[keep], c[keep]), empty)


def merge(a, b, mask=None):
    """SignalTrie.merge (:1674-1696) on triples: a plus the triples of b within `mask` (None: all of b)."""
    return merge_triples(project(a, ALL_ONES), project(b, ALL_ONES if mask is None else mask, "project" if mask is None else "within"))


CURVE_FIELDS = ("n_signals", "n_pairs", "samples_detected", "n_passing_signals", "n_identifiable_proteins")


def cycle_curve(triples, layout, n_proteins, cycles, modes, demote=False):
    """The scan of find_uniques under every cycle count of `cycles`: a dict of int64 arrays over the cycle counts - cycles,
    n_signals, n_pairs, samples_detected (the sum of counts), n_passing_signals, n_identifiable_proteins - and identifiable
    uint8 [len(cycles)][n_proteins], 1 where the protein is best for a passing signal.  `modes` is scan_modes' tuple."""
    cycles = [int(c) for c in cycles]
    out = {name: np.zeros(len(cycles), np.int64) for name in CURVE_FIELDS}
    out["cycles"] = np.array(cycles, np.int64)
    out["identifiable"] = np.zeros((len(cycles), int(n_proteins)), np.uint8)
    for i, mask in enumerate(cycle_masks(layout, cycles).tolist()):
        t = project(triples, mask)
        u = _uniques(t, modes, demote)
        out["n_signals"][i], out["n_pairs"][i], out["samples_detected"][i] = len(u["key"]), len(t[0]), t[2].sum()
        out["n_passing_signals"][i] = np.count_nonzero(u["passed"])
        out["identifiable"][i, u["best_protein"][u["passed"] != 0]] = 1
    out["n_identifiable_proteins"] = out["identifiable"].sum(axis=1).astype(np.int64)
    return out


# ---- a grid of (p, b, u) points (fsq_proteome_signals_points, fsq_proteome_tally_points) ----

MAX_POINTS = 4096                           # FSQ_PMC_MAX_POINTS


def grid_points(ps, bs, us):
    """The product of the three axes in p-major order: [(p, b, u), ...], u running fastest."""
    return [(float(p), float(b), float(u)) for p in ps for b in bs for u in us]


def check_points(points, sample_stride=0):
    """The points as a list of float triples; raises for none, for more than MAX_POINTS, for a p or u outside [0, 1], a negative
    b or a negative stride."""
    points = [tuple(float(v) for v in point) for point in points]
    if not points:
        raise ValueError("no point")
    if len(points) > MAX_POINTS:
        raise ValueError("%d points; at most %d" % (len(points), MAX_POINTS))
    for i, point in enumerate(points):
        if len(point) != 3:
            raise ValueError("point %d is not (p, b, u)" % i)
        p, b, u = point
        if not (0.0 <= p <= 1.0 and 0.0 <= u <= 1.0 and b >= 0.0):
            raise ValueError("point %d (p=%r, b=%r, u=%r): p and u must be in [0, 1] and b must not be negative" % (i, p, b, u))
    if int(sample_stride) != sample_stride or sample_stride < 0:
        raise ValueError("sample_stride must be a non-negative integer")
    return points


def shared_tables(points):
    """The distinct p and b values of the points in first-seen order, and per point the index of its value: (ps, bs,
    edman_index int32 [n], bleach_index int32 [n]).  The same float gives the same table."""
    ps, bs = {}, {}
    edman = [ps.setdefault(p, len(ps)) for p, _, _ in points]
    bleach = [bs.setdefault(b, len(bs)) for _, b, _ in points]
    return list(ps), list(bs), np.array(edman, np.int32), np.array(bleach, np.int32)


def stacked_edman_tables(ps, max_d):
    """edman_table of every p under the same max_d as one array: (start int64 [len(ps)][max_d + 2], offsets into values;
    values float64)."""
    starts, values, at = [], [], 0
    for p in ps:
        start, v = edman_table(p, max_d)
        starts.append(start + at)
        values.append(v)
        at += len(v)
    return np.array(starts, np.int64).reshape(len(ps), max_d + 2), np.concatenate(values) if values else np.zeros(0, np.float64)


def grid_signals(table, points, sample_size, seed, first_sample=0, sample_stride=0, first_row=0, n_rows=None):
    """signals for every point: (keys uint64 [n_points][n_rows], n_draws int32 [n_points][n_rows]); row g of point k is sample
    first_sample + k * sample_stride + g.  The loop of the single-point twin."""
    points = check_points(points, sample_stride)
    got = [signals(table, p, b, u, sample_size, seed, first_sample + k * int(sample_stride), first_row, n_rows)
           for k, (p, b, u) in enumerate(points)]
    return np.stack([k for k, _ in got]), np.stack([d for _, d in got])


def grid_tally(keys, proteins):
    """tally of every point's row of keys [n_points][n_rows] against the rows' proteins [n_rows]: a list of sorted triples."""
    return [tally(row, proteins) for row in np.asarray(keys, np.uint64)]


def grid_curve(triples_of_point, points, n_proteins, modes, demote=False):
    """The scan of find_uniques at every point: float64 arrays p, b, u and int64 arrays named as CURVE_FIELDS over the points,
    and identifiable uint8 [n_points][n_proteins], 1 where the protein is best for a passing signal."""
    out = {name: np.zeros(len(points), np.int64) for name in CURVE_FIELDS}
    for j, name in enumerate("pbu"):
        out[name] = np.array([point[j] for point in points], np.float64)
    out["identifiable"] = np.zeros((len(points), int(n_proteins)), np.uint8)
    for i, t in enumerate(triples_of_point):
        u = _uniques(t, modes, demote)
        out["n_signals"][i], out["n_pairs"][i], out["samples_detected"][i] = len(u["key"]), len(t[0]), t[2].sum()
        out["n_passing_signals"][i] = np.count_nonzero(u["passed"])
        out["identifiable"][i, u["best_protein"][u["passed"] != 0]] = 1
    out["n_identifiable_proteins"] = out["identifiable"].sum(axis=1).astype(np.int64)
    return out
