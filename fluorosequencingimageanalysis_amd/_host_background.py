"""The iterative background correction with numpy on the host: what fsq_background_iterate (include/fsq_background.h)
computes, the `device=None` route of background.py.  A problem is the dict of arrays background.pack_problem gives; one of
background.joint_pack_problem carries "n_channels" and its codes are joint keys, whose neighbours joint_neighbour_lists
gives (the definition of include/fsq_background_joint.h and DESIGN.md 4.32; it runs on the host only)."""
import itertools
import math

import numpy as np

from . import _native_background as NB

INT64_MIN = -(1 << 63)


def decode(code):
    """(positions int64 [n, MAX_DROPS] with 0 beyond the drops, drops int64 [n]) of uint64 codes."""
    code = np.asarray(code, dtype=np.uint64)
    pos = np.stack([((code >> np.uint64(8 * i)) & np.uint64(255)).astype(np.int64) for i in range(NB.MAX_DROPS)], axis=1)
    return pos.reshape(-1, NB.MAX_DROPS), ((code >> np.uint64(48)) & np.uint64(7)).astype(np.int64)


def neighbour_lists(code, num_cycles, include_multidrop, rows=None, chunk=2048):
    """The neighbours of the keys `rows` (all by default) of a problem's codes, as the neighbour kernel lists them: a list of
    int64 arrays, one per row, each the index of a neighbour's key or -1 for an absent one, in itertools.product order, those
    out of 0 < pos <= num_cycles or (multidrop excluded) with a repeated position left out."""
    code = np.asarray(code, dtype=np.uint64)
    rows = np.arange(len(code)) if rows is None else np.asarray(rows, dtype=np.int64)
    order = np.argsort(code, kind='stable')
    sorted_code = code[order]
    pos, drops = decode(code[rows])
    out = [None] * len(rows)
    for d in np.unique(drops):
        d = int(d)
        E = np.array([e for e in itertools.product((-1, 0, 1), repeat=d) if any(e)], dtype=np.int64).reshape(-1, d)
        sel = np.flatnonzero(drops == d)
        shifts = np.array([8 * i for i in range(d)], dtype=np.uint64)
        for a in range(0, len(sel), chunk):
            part = sel[a:a + chunk]
            cand = pos[part, None, :d] + E[None, :, :]                              # [n, M, d]
            ok = ((cand > 0) & (cand <= num_cycles)).all(axis=2)
            if not include_multidrop and d > 1:
                s = np.sort(cand, axis=2)
                ok &= (s[:, :, 1:] != s[:, :, :-1]).all(axis=2)
            high = code[rows[part]] & ~np.uint64((1 << 48) - 1)
            c = high[:, None] | ((cand & 255).astype(np.uint64) << shifts[None, None, :]).sum(axis=2, dtype=np.uint64)
            at = np.searchsorted(sorted_code, c)
            at_c = np.minimum(at, max(len(code) - 1, 0))
            found = (at < len(code)) & (sorted_code[at_c] == c) if len(code) else np.zeros(c.shape, bool)
            idx = np.where(found, order[at_c], -1)
            for r, row in enumerate(part):
                out[row] = idx[r][ok[r]].astype(np.int64)
    return out


def joint_decode(code, n_channels):
    """(cycles int64 [n, JOINT_MAX_DROPS] with 0 beyond the drops, drops int64 [n]) of uint64 joint keys of n_channels letters:
    a key's drops are its non-zero drop fields, read from the first on."""
    from ._host_signal_sweep import JOINT_DROP_BITS, JOINT_MAX_DROPS
    code = np.asarray(code, dtype=np.uint64).reshape(-1)
    B, cap = JOINT_DROP_BITS[n_channels], min(NB.JOINT_MAX_DROPS, JOINT_MAX_DROPS[n_channels])
    fields = np.stack([(code >> np.uint64(4 + B * i)) & np.uint64((1 << B) - 1) for i in range(cap)], axis=1).astype(np.int64)
    drops = np.cumprod(fields != 0, axis=1).sum(axis=1)
    cycles = np.zeros((len(code), NB.JOINT_MAX_DROPS), np.int64)
    cycles[:, :cap] = np.where(np.arange(cap)[None, :] < drops[:, None], fields & 63, 0)
    return cycles, drops


def joint_neighbour_lists(code, n_channels, num_cycles, include_multidrop, rows=None, chunk=256):
    """neighbour_lists for joint keys of n_channels letters (include/fsq_background_joint.h): the cycles perturbed in
    itertools.product order, letters and starts kept, those out of 0 < cycle <= num_cycles or (multidrop excluded) with a repeated cycle left out, each looked up as it stands: a tuple that no longer ascends by
    (cycle, letter) is no key's code and gives -1."""
    from ._host_signal_sweep import JOINT_DROP_BITS
    code = np.asarray(code, dtype=np.uint64)
    rows = np.arange(len(code)) if rows is None else np.asarray(rows, dtype=np.int64)
    B = JOINT_DROP_BITS[n_channels]
    num_cycles = min(int(num_cycles), NB.JOINT_MAX_CYCLES)
    order = np.argsort(code, kind='stable')
    sorted_code = code[order]
    cyc, drops = joint_decode(code[rows], n_channels)
    out = [np.zeros(0, np.int64)] * len(rows)
    for d in np.unique(drops):
        d = int(d)
        if d < 1:
            continue
        E = np.array([e for e in itertools.product((-1, 0, 1), repeat=d) if any(e)], dtype=np.int64).reshape(-1, d)
        sel = np.flatnonzero(drops == d)
        shifts = np.array([4 + B * i for i in range(d)], dtype=np.uint64)
        clear = ~np.uint64(sum(63 << (4 + B * i) for i in range(d)))
        for a in range(0, len(sel), max(1, chunk * 728 // len(E))):
            part = sel[a:a + max(1, chunk * 728 // len(E))]
            cand = cyc[part, None, :d] + E[None, :, :]                              # [n, M, d]
            ok = ((cand > 0) & (cand <= num_cycles)).all(axis=2)
            if not include_multidrop and d > 1:
                s = np.sort(cand, axis=2)
                ok &= (s[:, :, 1:] != s[:, :, :-1]).all(axis=2)
            rest = code[rows[part]] & clear
            c = rest[:, None] | ((cand & 63).astype(np.uint64) << shifts[None, None, :]).sum(axis=2, dtype=np.uint64)
            at = np.searchsorted(sorted_code, c)
            at_c = np.minimum(at, max(len(code) - 1, 0))
            found = (at < len(code)) & (sorted_code[at_c] == c)
            idx = np.where(found, order[at_c], -1)
            for r, row in enumerate(part):
                out[row] = idx[r][ok[r]].astype(np.int64)
    return out


def _pow2(values):
    """libm's pow(v, 2.0) of every value (Python's float ** 2), inf where it overflows."""
    def one(v):
        try:
            return math.pow(v, 2.0)
        except OverflowError:
            return math.inf
    return np.array([one(float(v)) for v in values], dtype=np.float64)


def z_scores(bp, ap, sp):
    """(:5787-5790) on arrays."""
    d = bp - ap
    with np.errstate(all='ignore'):
        return np.copysign(np.sqrt(_pow2(d) / _pow2(sp)), d)


def first_argmax(a):
    """Python's max(d, key=d.get) on the values in order: the first largest; a NaN in first place stays."""
    if a[0] != a[0]:
        return 0
    return int(np.argmax(np.where(np.isnan(a), -np.inf, a)))


def _mean(count, idx):
    if len(idx) == 0:
        return np.float64(np.nan)
    return np.mean(np.where(idx >= 0, count[np.maximum(idx, 0)], 0.0))


def py2_rounded(count):
    """pflib._py2_round of every count as int64; INT64_MIN where that is no int64."""
    with np.errstate(all='ignore'):
        r = np.where(count >= 0.0, np.floor(count + 0.5), np.ceil(count - 0.5))
        ok = (r > -9.2e18) & (r < 9.2e18)
        return np.where(ok, np.where(ok, r, 0.0).astype(np.int64), INT64_MIN)


def iterate(prob, max_iterations, accepted_cap, undefined_cap, elements=1 << 22):
    """One problem to its stop -> dict of count, percent, rounded, stop_reason, n_passes, n_accepted, overflow, accepted_key,
    undefined_bp (the entries written)."""
    count = np.array(prob["count"], dtype=np.float64)
    percent = np.array(prob["percent"], dtype=np.float64)
    filt = np.asarray(prob["filter"]).astype(bool)
    def_key = np.asarray(prob["def_key"], dtype=np.int64)
    ap, sp = np.asarray(prob["def_avg"], dtype=np.float64), np.asarray(prob["def_std"], dtype=np.float64)
    thr = float(prob["sigma_threshold"])
    N, D = len(count), len(def_key)
    if prob.get("n_channels") is None:
        nbs = neighbour_lists(prob["code"], int(prob["num_cycles"]), bool(prob["include_multidrop"]))
    else:
        nbs = joint_neighbour_lists(prob["code"], int(prob["n_channels"]), int(prob["num_cycles"]), bool(prob["include_multidrop"]))
    fidx = np.flatnonzero(filt)
    fpos = np.full(N, -1, np.int64)
    fpos[fidx] = np.arange(len(fidx))
    present = def_key >= 0
    accepted_key, undefined_bp = [], []
    overflow, passes, accepted, reason, prior = 0, 0, 0, NB.RUNNING, None
    with np.errstate(all='ignore'):
        while True:
            if passes >= max_iterations:
                reason = NB.MAX_ITERATIONS
                break
            und = prob["und_first"] if passes == 0 else prob["und_rest"]
            passes += 1
            z = z_scores(np.where(present, percent[np.maximum(def_key, 0)], 0.0), ap, sp)
            for k in und:
                if undefined_cap <= 0:                                            # (no buffer: nothing recorded, nothing flagged)
                    pass
                elif len(undefined_bp) < undefined_cap:
                    undefined_bp.append(percent[k])
                else:
                    overflow |= NB.OVERFLOW_UNDEFINED
                count[k] = _mean(count, nbs[k])
            prefix = np.add.accumulate(np.concatenate([[0.0], count[fidx]]))      # (sequential: prefix[j] the sum before j)
            total = prefix[-1]
            if len(fidx) and total == 0.0:
                reason = NB.ZERO_TOTAL
                break
            percent = np.where(filt, count / total, 0.0)
            if D == 0:
                reason = NB.NO_DEFINED
                break
            if z[first_argmax(z)] <= thr:
                reason = NB.THRESHOLD
                break
            trials = np.flatnonzero(present & ~(z <= thr))
            if len(trials) == 0:
                reason = NB.NO_IMPROVEMENT
                break
            keys = def_key[trials]
            interp = np.array([_mean(count, nbs[k]) for k in keys], dtype=np.float64)
            totals = np.full(len(trials), total)
            walk = np.flatnonzero(filt[keys])
            cf = count[fidx]
            step = max(1, elements // max(len(fidx), 1))
            for a in range(0, len(walk), step):
                part = walk[a:a + step]
                fp = fpos[keys[part]]
                jmin = int(fp.min())
                M = np.empty((len(part), len(fidx) - jmin + 1))
                M[:, 0] = prefix[jmin]
                M[:, 1:] = cf[jmin:]
                M[np.arange(len(part)), fp - jmin + 1] = interp[part]
                totals[part] = np.add.accumulate(M, axis=1)[:, -1]
            if (totals[walk] == 0.0).any():                                        # (a trial's float(count) / 0)
                reason = NB.ZERO_TOTAL
                break
            bp = np.where(filt[keys], interp / totals, 0.0)
            diff = z[trials] - z_scores(bp, ap[trials], sp[trials])
            b = first_argmax(diff)
            if diff[b] <= 0:
                reason = NB.NO_IMPROVEMENT
                break
            k = int(keys[b])
            if accepted < accepted_cap:
                accepted_key.append(k)
            else:
                overflow |= NB.OVERFLOW_ACCEPTED
            count[k] = interp[b]
            accepted += 1
            if prior is not None:
                d = np.abs(count - prior)
                if not (d[0] != d[0] or (d >= 0.001).any()):
                    reason = NB.CONVERGED
                    break
            prior = count.copy()
            if filt[k]:
                total = totals[b]
            percent = np.where(filt, count / total, 0.0)
    return {"count": count, "percent": percent, "rounded": py2_rounded(count), "stop_reason": reason, "n_passes": passes,
            "n_accepted": accepted, "overflow": overflow, "accepted_key": np.array(accepted_key, dtype=np.int32),
            "undefined_bp": np.array(undefined_bp, dtype=np.float64)}
