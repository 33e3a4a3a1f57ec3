"""The host twin of the simulation parameter sweep (include/fsq_signal_sweep.h), NumPy and plain Python: the 64-bit signal
key and its codec, the classification and tally of count rows, the key table a scoring call is made over and
signal_correlation (jupyter_development.py:279-578) for many fit dicts at once, in the kernel's order of operations, so that
fsq_signal_scores can be compared with it bit for bit, and match_diagnostic's loop over signal pairs (:833-889) as
fsq_signal_pair_best and fsq_signal_pair_extremes run it.  No GPU and no torch are needed."""
import math

import numpy as np

MAX_DROPS, MAX_FRAMES, EMPTY, NEVER, MAX_COUNT = 10, 64, 0x400, 0x800, (1 << 31) - 1
METRICS = ('naive', 'my_euclidean', 'normalized_euclidean', 'my_std_normalized_euclidean', 'my_sim_std_normalized_euclidean',
           'log_rmsd', 'my_canberra', 'my_chebyshev', 'my_normalized_chebyshev', 'my_std_normalized_chebyshev')
# signal_correlation's other metrics: the signed and rank forms, the two `matching` forms, and what the reference itself stubs
OTHER_METRICS = ('pearson', 'euclidean', 'chebyshev', 'canberra', 'matching', 'matching_10p', 'kendalltau', 'scipy_canberra',
                 'my_weighted_std_normalized_euclidean', 'my_pearson', 'my_kendalltau', 'my_spearman_rho')
NORMALIZE_COUNTS, HEATMAP_NORMALIZE_COUNTS = 1, 2
SCORE_OK, SCORE_EMPTY, SCORE_DIVZERO, SCORE_DOMAIN = 0, 1, 2, 3
ROW_SIGNAL, ROW_NONE, ROW_UNKEYED = 0, 1, 2
NO_DROPS = (('A', 0),)


# ---- the key ----

def key_of(start, cycles):
    """The key of a starting count 0 .. 15 and up to MAX_DROPS drop cycles 1 .. 63 in ascending order."""
    key = int(start)
    for i, c in enumerate(cycles):
        key |= int(c) << (4 + 6 * i)
    return key


def key_of_signal(signal):
    """The key of the reference's (decrements, is_zero, start), or None where no count row has that signal or it has no key:
    a letter other than 'A', cycles that do not ascend within 1 .. 63, more than MAX_DROPS or more than `start` drops, a
    start outside 0 .. 15, an is_zero that is not (drops == start)."""
    try:
        s, z, start = signal
        s = tuple(s)
        cycles = [] if s == NO_DROPS else [c for _, c in s]
        if any(a != 'A' for a, _ in s) or int(start) != start or not 0 <= start <= 15 or len(cycles) > min(MAX_DROPS, start):
            return None
        if any(int(c) != c or not 1 <= c < MAX_FRAMES for c in cycles) or any(a > b for a, b in zip(cycles, cycles[1:])):
            return None
        if not s or bool(z) != (len(cycles) == start) or not isinstance(z, (bool, np.bool_)):
            return None
    except (TypeError, ValueError):
        return None
    return key_of(start, cycles)


def signal_of_key(key):
    """(decrements, is_zero, start) of a key: what lognormal.signal_of and _tracks.decrements_of_row give for its rows."""
    key = int(key) & 0xffffffffffffffff                         # (a key read from an int64 tensor may come signed)
    start, cycles = key & 15, []
    for i in range(MAX_DROPS):
        c = (key >> (4 + 6 * i)) & 63
        if c == 0:
            if key >> (4 + 6 * i):
                raise ValueError("0x%x is not a signal key" % key)
            break
        cycles.append(c)
    if len(cycles) > start or any(a > b for a, b in zip(cycles, cycles[1:])):
        raise ValueError("0x%x is not a signal key" % key)
    return (tuple(('A', c) for c in cycles) or NO_DROPS), len(cycles) == start, start


def classify_row(row):
    """(ROW_SIGNAL, key), (ROW_NONE, None) for a row with an upstep or (ROW_UNKEYED, None) for one with more than MAX_DROPS
    drops or a start above 15: kss_tally's row_key."""
    row = [int(c) for c in row]
    if not 1 <= len(row) <= MAX_FRAMES:
        raise ValueError("a row has 1 .. %d frames" % MAX_FRAMES)
    if any(b > a for a, b in zip(row, row[1:])):
        return ROW_NONE, None
    cycles = [f for f in range(1, len(row)) for _ in range(row[f - 1] - row[f])]
    if row[0] > 15 or len(cycles) > MAX_DROPS:
        return ROW_UNKEYED, None
    return ROW_SIGNAL, key_of(row[0], cycles)


def tally_rows(rows, points, valid, n_points):
    """fsq_signal_tally on the host: ([{key: count}] per point, none [n_points], unkeyed [n_points])."""
    tables = [{} for _ in range(n_points)]
    none, unkeyed = [0] * n_points, [0] * n_points
    rows = np.asarray(rows, dtype=np.uint8)
    uniq, inverse = np.unique(rows, axis=0, return_inverse=True) if len(rows) else (rows, np.zeros(0, np.int64))
    kinds = [classify_row(r) for r in uniq.tolist()]
    for i, u in enumerate(np.asarray(inverse).reshape(-1).tolist()):
        k = int(points[i])
        if (valid is not None and not valid[i]) or not 0 <= k < n_points:
            continue
        what, key = kinds[u]
        if what == ROW_SIGNAL:
            tables[k][key] = tables[k].get(key, 0) + 1
        elif what == ROW_NONE:
            none[k] += 1
        else:
            unkeyed[k] += 1
    return tables, none, unkeyed


# ---- the joint key of several colour channels (include/fsq_signal_sweep.h, THE JOINT KEY) ----

MAX_CHANNELS = 4
JOINT_DROP_BITS = {1: 6, 2: 7, 3: 8, 4: 8}      # B(K) = 6 + ceil(log2 K)
JOINT_MAX_DROPS = {1: 10, 2: 8, 3: 6, 4: 6}     # D(K)


def _start_shift(K, k):
    return 0 if k == 0 else 64 - 4 * (K - k)


def joint_key_of(starts, drops):
    """The joint key of K starting counts 0 .. 15 (K = 1 .. 4 channels, in sorted-letter order) and up to D(K) drops (cycle
    1 .. 63, channel) in ascending order.  With K = 1 it is key_of(starts[0], cycles)."""
    K = len(starts)
    B = JOINT_DROP_BITS[K]
    key = 0
    for k, start in enumerate(starts):
        key |= int(start) << _start_shift(K, k)
    for i, (c, k) in enumerate(drops):
        key |= (int(c) | int(k) << 6) << (4 + B * i)
    return key


def joint_key_of_signal(letters, signal):
    """The joint key of peptide_simulator.joint_signal's (decrements, zeros, starts) under the sorted `letters`, or None where
    no rows have that signal or it has no key: a letter outside `letters`, drops that do not ascend by (cycle, letter) within
    cycles 1 .. 63, more than D(K) drops in all or more of a letter than its start, a start outside 0 .. 15, a `zeros` entry
    that is not (the letter's drops == its start)."""
    try:
        dec, zeros, starts = signal
        letters, dec, zeros, starts = tuple(letters), tuple(dec), tuple(zeros), tuple(starts)
        K = len(letters)
        if not 1 <= K <= MAX_CHANNELS or len(zeros) != K or len(starts) != K or len(dec) > JOINT_MAX_DROPS[K]:
            return None
        if any(int(s) != s or not 0 <= s <= 15 for s in starts) or any(not isinstance(z, (bool, np.bool_)) for z in zeros):
            return None
        drops = []
        for a, c in dec:
            if a not in letters or int(c) != c or not 1 <= c < MAX_FRAMES:
                return None
            drops.append((int(c), letters.index(a)))
        if any(a > b for a, b in zip(drops, drops[1:])):
            return None
        for k in range(K):
            n = sum(1 for _, ch in drops if ch == k)
            if n > starts[k] or bool(zeros[k]) != (n == starts[k]):
                return None
    except (TypeError, ValueError):
        return None
    return joint_key_of(starts, drops)


def joint_signal_of_key(letters, key):
    """(decrements, zeros, starts) of a joint key under the sorted `letters`: what peptide_simulator.joint_signal gives for
    its rows.  ValueError for a bit pattern that is no molecule's key (EMPTY and NEVER among them)."""
    key = int(key) & 0xffffffffffffffff                         # (a key read from an int64 tensor may come signed)
    letters = tuple(letters)
    K = len(letters)
    B, D = JOINT_DROP_BITS[K], JOINT_MAX_DROPS[K]
    starts = [(key >> _start_shift(K, k)) & 15 for k in range(K)]
    drops, ended = [], False
    for i in range(D):
        field = (key >> (4 + B * i)) & ((1 << B) - 1)
        c, k = field & 63, field >> 6
        if field == 0:
            ended = True
        elif ended or c == 0 or k >= K:
            raise ValueError("0x%x is not a joint signal key of %d channels" % (key, K))
        else:
            drops.append((c, k))
    spare = (key >> (4 + B * D)) & ((1 << (60 - 4 * (K - 1) - B * D)) - 1)              # the bits between drops and top nibbles
    n = [sum(1 for _, ch in drops if ch == k) for k in range(K)]
    if spare or any(a > b for a, b in zip(drops, drops[1:])) or any(n[k] > starts[k] for k in range(K)):
        raise ValueError("0x%x is not a joint signal key of %d channels" % (key, K))
    return tuple((letters[k], c) for c, k in drops), tuple(n[k] == starts[k] for k in range(K)), tuple(starts)


def joint_signals_of_keys(letters, keys):
    """[joint_signal_of_key(letters, k) for k in keys] for keys a tally has made (they are not checked), the bit fields taken
    apart in NumPy: a table of 10^5 .. 10^6 occupied slots becomes its dict in seconds."""
    letters = tuple(letters)
    K = len(letters)
    B, D = JOINT_DROP_BITS[K], JOINT_MAX_DROPS[K]
    keys = np.ascontiguousarray(keys).view(np.uint64).reshape(-1)
    starts = np.stack([(keys >> np.uint64(_start_shift(K, k))) & np.uint64(15) for k in range(K)], axis=1).astype(np.int64)
    fields = np.stack([(keys >> np.uint64(4 + B * i)) & np.uint64((1 << B) - 1) for i in range(D)], axis=1).astype(np.int64)
    present = fields != 0
    per_channel = np.stack([(present & (fields >> 6 == k)).sum(axis=1) for k in range(K)], axis=1)
    pair = [(letters[f >> 6], f & 63) if f >> 6 < K else None for f in range(1 << B)]
    return [(tuple(pair[f] for f in row[:d]), tuple(z), tuple(st))
            for row, d, z, st in zip(fields.tolist(), present.sum(axis=1).tolist(), (per_channel == starts).tolist(), starts.tolist())]


def classify_joint_rows(rows):
    """(ROW_SIGNAL, key), (ROW_NONE, None) for a molecule with an upstep in any channel or (ROW_UNKEYED, None) for one with
    more than D(K) drops in all or a channel that starts above 15, of one molecule's K count rows [K][frames]: kss_tally_joint's
    joint_row_key."""
    rows = [[int(c) for c in row] for row in rows]
    K = len(rows)
    if not 1 <= K <= MAX_CHANNELS:
        raise ValueError("a molecule has 1 .. %d channels" % MAX_CHANNELS)
    if not 1 <= len(rows[0]) <= MAX_FRAMES or any(len(row) != len(rows[0]) for row in rows):
        raise ValueError("a row has 1 .. %d frames" % MAX_FRAMES)
    if any(b > a for row in rows for a, b in zip(row, row[1:])):
        return ROW_NONE, None
    drops = [(f, k) for f in range(1, len(rows[0])) for k in range(K) for _ in range(rows[k][f - 1] - rows[k][f])]
    if any(row[0] > 15 for row in rows) or len(drops) > JOINT_MAX_DROPS[K]:
        return ROW_UNKEYED, None
    return ROW_SIGNAL, joint_key_of([row[0] for row in rows], drops)


def tally_joint_rows(rows, points, valid, n_points):
    """fsq_signal_tally_joint on the host, rows uint8 [K][n][frames]: ([{key: count}] per point, none [n_points], unkeyed
    [n_points])."""
    tables = [{} for _ in range(n_points)]
    none, unkeyed = [0] * n_points, [0] * n_points
    rows = np.asarray(rows, dtype=np.uint8)
    K, n, F = rows.shape
    flat = np.ascontiguousarray(rows.transpose(1, 0, 2)).reshape(n, K * F)
    uniq, inverse = np.unique(flat, axis=0, return_inverse=True) if n else (flat, np.zeros(0, np.int64))
    kinds = [classify_joint_rows(np.reshape(r, (K, F)).tolist()) for r in uniq]
    for i, u in enumerate(np.asarray(inverse).reshape(-1).tolist()):
        k = int(points[i])
        if (valid is not None and not valid[i]) or not 0 <= k < n_points:
            continue
        what, key = kinds[u]
        if what == ROW_SIGNAL:
            tables[k][key] = tables[k].get(key, 0) + 1
        elif what == ROW_NONE:
            none[k] += 1
        else:
            unkeyed[k] += 1
    return tables, none, unkeyed


def is_joint(signal):
    """Whether a signal is a joint one, (decrements, zeros, starts) with a tuple per letter, and not the reference's."""
    return isinstance(signal[1], tuple)


def signal_flags(signal):
    """(z, drops, single) as the scores read them.  The reference's signal (s, z, start): z, len(s) - its drop-free NO_DROPS
    has length 1 -, no (letter, cycle) pair twice.  A joint signal (decrements, zeros, starts), by this package's definition:
    z = all(zeros); drops = len(decrements), the drop-free () counting as one as NO_DROPS does; single = no (letter, cycle)
    pair stands twice."""
    s, z, _ = signal
    if is_joint(signal):
        return all(z), max(len(s), 1), len(set(s)) == len(s)
    return bool(z), len(s), len(set(s)) == len(s)


# ---- the key table of a scoring call ----

def ordered_signals(signals, letters=None):
    """Signals in the order every sum runs in: ascending key, then those without a key by their repr.  With `letters` (the
    sorted label letters of a joint sweep) the signals are joint ones and the key is the joint key."""
    key = key_of_signal if letters is None else (lambda s: joint_key_of_signal(letters, s))
    keyed = sorted((key(s), s) for s in signals if key(s) is not None)
    return [s for _, s in keyed] + sorted((s for s in signals if key(s) is None), key=repr)


def check_metric(metric):
    if metric not in METRICS:
        raise NotImplementedError(metric) if metric in OTHER_METRICS else ValueError("Invalid metric chosen.")
    return METRICS.index(metric)


def key_table(observed_signals, signals, heatmap_only=True, zero_only=True, exclude_signals=None, select_signals=None,
              allow_multidrop=False):
    """What fsq_signal_scores reads about the keys: observed int64 [S], in_observed, admitted, heatmap uint8 [S] for the
    ordered `signals` (the union of the observed dict's and of every fit dict's), and the std metrics' n.  Joint signals are
    admitted by signal_flags' rules: z is all(zeros), single means no (letter, cycle) pair stands twice, the heat-map condition
    is one or two drops with the drop-free () counting as one."""
    S = len(signals)
    observed, in_observed = np.zeros(S, np.int64), np.zeros(S, np.uint8)
    admitted, heatmap = np.zeros(S, np.uint8), np.zeros(S, np.uint8)
    for i, sig in enumerate(signals):
        z, drops, single = signal_flags(sig)
        if sig in observed_signals:
            observed[i], in_observed[i] = _count(observed_signals[sig]), 1
        admitted[i] = ((select_signals is None or sig in select_signals) and (not zero_only or z)
                       and (not heatmap_only or drops in (1, 2)) and (allow_multidrop or single)
                       and (exclude_signals is None or sig not in exclude_signals))
        heatmap[i] = z and drops in (1, 2) and single
    n_observed = sum(_count(n) for sig, n in observed_signals.items()
                     if (not zero_only or signal_flags(sig)[0]) and (allow_multidrop or signal_flags(sig)[2]))
    if n_observed > MAX_COUNT:
        raise NotImplementedError("observed counts beyond 2^31 - 1")
    return {"signals": list(signals), "observed": observed, "in_observed": in_observed, "admitted": admitted, "heatmap": heatmap,
            "n_observed": int(n_observed)}


def _count(n):
    if int(n) != n or not 0 <= n <= MAX_COUNT:
        raise NotImplementedError("counts are integers in 0 .. 2^31 - 1, not %r" % (n,))
    return int(n)


def normalization_of(normalize_counts, heatmap_normalize_counts):
    return (NORMALIZE_COUNTS if normalize_counts else 0) | (HEATMAP_NORMALIZE_COUNTS if heatmap_normalize_counts else 0)


def fit_matrix(signals, fit_dicts):
    """int64 [S][P] of the fit dicts' counts over the ordered signals, and every dict's total [P]."""
    index = {s: i for i, s in enumerate(signals)}
    fit = np.zeros((len(signals), len(fit_dicts)), np.int64)
    for k, d in enumerate(fit_dicts):
        for s, n in d.items():
            fit[index[s], k] = _count(n)
    return fit, fit.sum(axis=0)


# ---- the scores ----

def term(m, oi, fi, nf, n_obs, n_fit):
    """One paired key's contribution under metric index m and the factor nf, as fsq_score_term.h's score_term: (c, is_max,
    error).  c is None where the metric takes no contribution from the key; error is 0, SCORE_DIVZERO or SCORE_DOMAIN."""
    o, f = float(oi), float(fi) * nf
    if m == 0:
        return o * f, False, 0
    if m == 1:
        return (f - o) ** 2, False, 0
    if m in (2, 8):
        if oi <= 0:
            return None, m == 8, 0
        return (((f - o) / o) ** 2 if m == 2 else abs(o - f) / o), m == 8, 0
    if m in (3, 4, 9):
        sd = 1.0
        if m == 4:
            if f > 0.0:
                v = f * (float(n_fit) - f) / float(n_fit)
                if v < 0.0:
                    return None, False, SCORE_DOMAIN
                sd = math.sqrt(v)
        elif oi > 0:
            if n_obs == 0:
                return None, False, SCORE_DIVZERO
            v = float(oi * (n_obs - oi)) / float(n_obs)
            if v < 0.0:
                return None, False, SCORE_DOMAIN
            sd = math.sqrt(v)
        if sd == 0.0:
            return None, False, SCORE_DIVZERO
        return (((f - o) / sd) ** 2 if m != 9 else abs(o - f) / sd), m == 9, 0
    if m == 5:
        return (math.log(float(oi + 1)) - math.log(f + 1.0)) ** 2, False, 0
    if m == 6:
        den = abs(o) + abs(f)
        if den == 0.0:
            return None, False, SCORE_DIVZERO
        return abs(o - f) / den, False, 0
    return abs(o - f), True, 0


def result(m, acc, n_contrib, divzero, domain):
    """(status, result) of the accumulated terms, as fsq_score_term.h's score_result after the error flags."""
    if domain or divzero or (m == 8 and n_contrib == 0):
        return (SCORE_DIVZERO if divzero and not domain else SCORE_DOMAIN), None
    return SCORE_OK, acc if m in (0, 6, 7, 8, 9) else math.sqrt(acc / float(n_contrib)) if m == 5 else math.sqrt(acc)


def is_paired(adm, in_obs, o, f, cutoff):
    return bool(adm and (in_obs or f > 0) and (cutoff is None or (float(o) >= cutoff and float(f) >= cutoff)))


def scores(table, fit, fit_total, metric, normalization=0, small_count_cutoff=None, contributions=True):
    """fsq_signal_scores on the host, operation for operation: (score float64 [P], factor float64 [P], status int32 [P],
    contributions float64 [S][P] or None), NaN where the kernel writes NaN."""
    m = check_metric(metric)
    obs, in_obs, adm, heat = (table[k].tolist() for k in ("observed", "in_observed", "admitted", "heatmap"))
    S, n_obs = len(obs), table["n_observed"]
    P = len(fit_total)
    fit = np.asarray(fit, dtype=np.int64).reshape(S, P)                 # (S = 0: no keys, P points all the same)
    score, factor = np.full(P, np.nan), np.full(P, np.nan)
    status = np.zeros(P, np.int32)
    contrib = np.full((S, P), np.nan) if contributions else None
    cutoff = None if small_count_cutoff is None else float(small_count_cutoff)
    for k in range(P):
        f_k, n_fit = fit[:, k].tolist(), int(fit_total[k])
        pairs = [i for i in range(S) if is_paired(adm[i], in_obs[i], obs[i], f_k[i], cutoff)]
        sum_o, sum_f = sum(obs[i] for i in pairs), sum(f_k[i] for i in pairs)
        nf = 1.0
        if (normalization & NORMALIZE_COUNTS) and pairs and sum_f > 0:
            nf = float(sum_o) / float(sum_f)
        elif normalization & HEATMAP_NORMALIZE_COUNTS:
            hot = [i for i in range(S) if heat[i] and (in_obs[i] or f_k[i] > 0)]
            heat_o, heat_f = sum(obs[i] for i in hot if in_obs[i]), sum(f_k[i] for i in hot)
            if heat_f == 0:
                status[k] = SCORE_DIVZERO
                continue
            nf = float(heat_o) / float(heat_f)
        factor[k] = nf
        if not pairs:
            status[k] = SCORE_EMPTY
            continue
        acc, n_contrib, divzero, domain = 0.0, 0, False, False
        for i in pairs:
            c, is_max, err = term(m, obs[i], f_k[i], nf, n_obs, n_fit)
            divzero, domain = divzero or err == SCORE_DIVZERO, domain or err == SCORE_DOMAIN
            if c is None:
                continue
            n_contrib += 1
            if contrib is not None:
                contrib[i, k] = c
            acc = max(acc, c) if is_max else acc + c
        status[k], r = result(m, acc, n_contrib, divzero, domain)
        if status[k] == SCORE_OK:
            score[k] = r
    return score, factor, status, contrib


def result_of(signals, score, factor, status, contrib, k):
    """signal_correlation's return value for point k, or its exception."""
    st = int(status[k])
    if st == SCORE_DIVZERO:
        raise ZeroDivisionError("float division by zero")
    if st == SCORE_DOMAIN:
        raise ValueError("signal_correlation: the maximum of no contributions, or the root of a negative variance")
    if st == SCORE_EMPTY:
        return None, (float(factor[k]), {})
    c = {} if contrib is None else {s: float(contrib[i][k]) for i, s in enumerate(signals) if contrib[i][k] == contrib[i][k]}
    return float(score[k]), (float(factor[k]), c)


# ---- the incompatibility loop over signal pairs (jupyter_development.py:838-889) ----

MAX_SEL = 2048                      # FSQ_SIGNAL_PAIR_MAX_SEL


def pair_index(i, j, n_sel):
    """The index of pair (i, j), i < j, in itertools.combinations' order."""
    return i * (2 * n_sel - i - 1) // 2 + j - i - 1


def heat_factors(table, fit, fit_total):
    """The points' heat-map factor and status, which do not depend on the pair: scores() with nothing admitted."""
    none = dict(table, admitted=np.zeros_like(table["admitted"]))
    _, factor, status, _ = scores(none, fit, fit_total, METRICS[0], HEATMAP_NORMALIZE_COUNTS, None, False)
    return factor, status


def pair_best(table, rows, fit, fit_total, metric, normalization=0, small_count_cutoff=None, reverse_order=False):
    """fsq_signal_pair_best on the host, operation for operation: a dict of best_point int32 [K], result, factor float64 [K],
    dist float64 [K, 2], error_point and error_status int32 [K] for the K pairs of the candidates whose rows in the key table
    are `rows` (-1: in no dict)."""
    m = check_metric(metric)
    obs, in_obs, adm = (table[k].tolist() for k in ("observed", "in_observed", "admitted"))
    S, n_obs, P = len(obs), table["n_observed"], len(fit_total)
    rows = [int(r) for r in rows]
    n_sel = len(rows)
    if not 2 <= n_sel <= MAX_SEL or P < 1 or any(not -1 <= r < S for r in rows):
        raise ValueError("2 .. %d candidate rows within -1 .. n_keys - 1 and at least one point are needed" % MAX_SEL)
    fit = np.asarray(fit, dtype=np.int64).reshape(S, P).tolist()
    totals = [int(n) for n in fit_total]
    cutoff = None if small_count_cutoff is None else float(small_count_cutoff)
    heat_f, heat_s = heat_factors(table, fit, fit_total) if normalization & HEATMAP_NORMALIZE_COUNTS else (None, None)
    K = n_sel * (n_sel - 1) // 2
    out = {"best_point": np.full(K, -1, np.int32), "result": np.full(K, np.nan), "factor": np.full(K, np.nan),
           "dist": np.full((K, 2), np.nan), "error_point": np.full(K, -1, np.int32), "error_status": np.zeros(K, np.int32)}
    t = -1
    for i in range(n_sel):
        for j in range(i + 1, n_sel):
            t += 1
            pair = [r for r in (rows[i], rows[j])]
            best = None
            for k in range(P):
                f = [fit[r][k] if r >= 0 and adm[r] else 0 for r in pair]
                pr = [r >= 0 and is_paired(adm[r], in_obs[r], obs[r], f[x], cutoff) for x, r in enumerate(pair)]
                sum_o, sum_f = sum(obs[r] for x, r in enumerate(pair) if pr[x]), sum(f[x] for x in range(2) if pr[x])
                nf, status = 1.0, SCORE_OK
                if (normalization & NORMALIZE_COUNTS) and any(pr) and sum_f > 0:
                    nf = float(sum_o) / float(sum_f)
                elif normalization & HEATMAP_NORMALIZE_COUNTS:
                    if heat_s[k] == SCORE_DIVZERO:
                        status = SCORE_DIVZERO
                    else:
                        nf = float(heat_f[k])
                if status == SCORE_OK and not any(pr):
                    status = SCORE_EMPTY
                d, r = [np.nan, np.nan], None
                if status == SCORE_OK:
                    acc, n_contrib, divzero, domain = 0.0, 0, False, False
                    for x in range(2):
                        if not pr[x]:
                            continue
                        c, is_max, err = term(m, obs[pair[x]], f[x], nf, n_obs, totals[k])
                        divzero, domain = divzero or err == SCORE_DIVZERO, domain or err == SCORE_DOMAIN
                        if c is None:
                            continue
                        n_contrib += 1
                        d[x] = c
                        acc = max(acc, c) if is_max else acc + c
                    status, r = result(m, acc, n_contrib, divzero, domain)
                if status == SCORE_OK:
                    if best is None or (r > best[0] if reverse_order else r < best[0]):
                        best = (r, k, nf, d)
                elif status != SCORE_EMPTY and out["error_point"][t] < 0:
                    out["error_point"][t], out["error_status"][t] = k, status
            if best is not None:
                out["result"][t], out["best_point"][t], out["factor"][t], out["dist"][t] = best
    return out


def pair_extremes(dist, n_sel, reverse_order=False):
    """fsq_signal_pair_extremes on the host: (score float64 [n_sel], n_distances int32 [n_sel]); the maximum (the minimum with
    reverse_order) of each candidate's n_sel - 1 distances, NaN skipped, NaN where there is none."""
    dist = np.asarray(dist, dtype=np.float64).reshape(-1, 2)
    if not 2 <= n_sel <= MAX_SEL or len(dist) != n_sel * (n_sel - 1) // 2:
        raise ValueError("2 .. %d candidates and a [n_sel (n_sel - 1) / 2, 2] array are needed" % MAX_SEL)
    i, j = np.triu_indices(n_sel, 1)                                    # combinations' order
    mine = np.full((n_sel, n_sel), np.nan)
    mine[i, j], mine[j, i] = dist[:, 0], dist[:, 1]
    score = (np.fmin if reverse_order else np.fmax).reduce(mine, axis=1)
    return score, (~np.isnan(mine)).sum(axis=1).astype(np.int32)
