"""NumPy twin of the colocalisation of tracks between colour channels (include/fsq_colocalize.h) and of colocalize's merge
over K channels: the same integers, without a GPU."""
import math

import numpy as np

MAX_CHANNELS = 4
MAX_FRAMES = 64
COORD_LIMIT = 1 << 30


def radius_sq_of(radius):
    """floor(radius^2) as an int, exactly (a float's square through integers); ValueError for a negative or non-finite one."""
    if isinstance(radius, (int, np.integer)):
        r2 = int(radius) * int(radius)
    else:
        radius = float(radius)
        if not math.isfinite(radius):
            raise ValueError("radius must be finite")
        num, den = radius.as_integer_ratio()
        r2 = (num * num) // (den * den)
    if radius < 0:
        raise ValueError("radius must not be negative")
    if r2 >= 1 << 63:
        raise ValueError("radius^2 must be below 2^63")
    return r2


def check_positions(hw, what="positions"):
    """int64 [n, 2] of integer positions with |coordinate| < 2^30 (ValueError)."""
    hw = np.asarray(hw)
    if hw.dtype.kind not in "iu":
        raise ValueError("%s must be integers" % what)
    if hw.size and (int(hw.max()) >= COORD_LIMIT or int(hw.min()) <= -COORD_LIMIT):
        raise ValueError("%s need |coordinate| < 2^30" % what)
    return hw.astype(np.int64).reshape(-1, 2)


def bad_lanes(a_seg, a_off, b_off, n_a, n_b):
    """(bool [n_a]: the a's that fsq_colocalize_match stores -1 for, whether d_bad is set) of segments and offsets as they come."""
    a_seg, a_off, b_off = (np.asarray(x, np.int64).reshape(-1) for x in (a_seg, a_off, b_off))
    n_seg = len(a_off) - 1
    if len(b_off) != len(a_off) or n_seg < 0 or len(a_seg) != n_a:
        raise ValueError("a_off and b_off need n_seg + 1 entries each and a_seg one per a")

    def ok_of(off, n):
        return (off[:-1] >= 0) & (off[:-1] <= off[1:]) & (off[1:] <= n)
    seg_ok = ok_of(a_off, n_a) & ok_of(b_off, n_b)
    ends_ok = n_seg == 0 or (a_off[0] == 0 and b_off[0] == 0 and a_off[-1] == n_a and b_off[-1] == n_b)
    in_range = (a_seg >= 0) & (a_seg < n_seg)
    s = np.where(in_range, a_seg, 0)
    i = np.arange(n_a)
    if n_seg:
        lane_ok = in_range & seg_ok[s] & (a_off[s] <= i) & (i < a_off[s + 1])
    else:
        lane_ok = np.zeros(n_a, bool)
    return ~lane_ok, bool((~lane_ok).any() or not seg_ok.all() or not ends_ok)


def match(a_hw, a_seg, a_off, b_hw, b_off, radius_sq):
    """fsq_colocalize_match with NumPy: (match_of_a int32 [n_a], match_of_b int32 [n_b], dist_sq_of_a int64 [n_a]).  a_seg or
    offsets that are not well formed raise ValueError."""
    a_hw, b_hw = check_positions(a_hw, "a_hw"), check_positions(b_hw, "b_hw")
    a_off, b_off = (np.asarray(x, np.int64).reshape(-1) for x in (a_off, b_off))
    radius_sq = int(radius_sq)
    if radius_sq < 0:
        raise ValueError("radius_sq must not be negative")
    n_a, n_b = len(a_hw), len(b_hw)
    if bad_lanes(a_seg, a_off, b_off, n_a, n_b)[1]:
        raise ValueError("a_seg or the offsets are not well formed")
    match_of_a, match_of_b = np.full(n_a, -1, np.int32), np.full(n_b, -1, np.int32)
    dist_sq_of_a = np.full(n_a, -1, np.int64)
    far = np.int64(np.iinfo(np.int64).max)
    for s in range(len(a_off) - 1):
        a0, a1, b0, b1 = int(a_off[s]), int(a_off[s + 1]), int(b_off[s]), int(b_off[s + 1])
        if a0 == a1 or b0 == b1:
            continue
        d = a_hw[a0:a1, None, :] - b_hw[None, b0:b1, :]
        d = d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]
        d = np.where(d <= radius_sq, d, far)
        best_b, best_a = np.argmin(d, axis=1), np.argmin(d, axis=0)       # (the first of equal minima: the lowest index)
        a = np.arange(a1 - a0)
        pair = (d[a, best_b] != far) & (best_a[best_b] == a)
        a, b = a[pair], best_b[pair]
        match_of_a[a0 + a], match_of_b[b0 + b], dist_sq_of_a[a0 + a] = b0 + b, a0 + a, d[a, b]
    return match_of_a, match_of_b, dist_sq_of_a


def grouped(field, field_ids):
    """(order, segment per sorted element, offsets int64 [n_seg + 1]) of one field per element: the stable order by field and
    the contiguous range of every field of field_ids (ascending, a superset of the elements' fields)."""
    field = np.asarray(field, np.int64).reshape(-1)
    order = np.argsort(field, kind='stable')
    seg = np.searchsorted(field_ids, field[order])
    off = np.searchsorted(seg, np.arange(len(field_ids) + 1)).astype(np.int64)
    return order, seg.astype(np.int32), off


def checked_tables(tables_hw_field, offsets):
    """[(hw + offset int64 [n, 2], field int64 [n])] per channel, after the checks: 1 .. 4 channels, integer positions below
    2^30 in magnitude after the offset, one field per track."""
    tables = list(tables_hw_field)
    K = len(tables)
    if not 1 <= K <= MAX_CHANNELS:
        raise ValueError("1 .. %d channels are needed, not %d" % (MAX_CHANNELS, K))
    offsets = [(0, 0)] * K if offsets is None else list(offsets)
    if len(offsets) != K:
        raise ValueError("one (dh, dw) offset per channel is needed")
    out = []
    for k, ((hw, field), off) in enumerate(zip(tables, offsets)):
        off = np.asarray(off)
        if off.shape != (2,) or off.dtype.kind not in "iu":
            raise ValueError("an offset is two integers (dh, dw)")
        hw = np.asarray(hw)
        if hw.dtype.kind not in "iu":
            raise ValueError("positions must be integers")
        error = "channel %d: positions need |coordinate| < 2^30 after the offset" % k
        hw = hw.reshape(-1, 2)
        # (both below 2^31 in magnitude before they are added, so the int64 sum is exact)
        if max(abs(int(off[0])), abs(int(off[1]))) >= 1 << 31 or (hw.size and (int(hw.max()) >= 1 << 31 or int(hw.min()) <= -(1 << 31))):
            raise ValueError(error)
        hw = hw.astype(np.int64) + off.astype(np.int64).reshape(1, 2)
        if hw.size and int(np.abs(hw).max()) >= COORD_LIMIT:
            raise ValueError(error)
        field = np.asarray(field)
        if field.dtype.kind not in "iu" and field.size:
            raise ValueError("fields must be integers")
        field = field.astype(np.int64).reshape(-1)
        if len(field) != len(hw):
            raise ValueError("one field per track")
        out.append((hw.astype(np.int64).reshape(-1, 2), field))
    return out


def molecules(tables_hw_field, radius, offsets=None):
    """The merge over K channels: {member int32 [K, M], field int64 [M], hw int64 [M, 2]}.  tables_hw_field: per channel (hw
    [n, 2], field [n]).  The molecules start as channel 0's tracks; channel k's tracks are matched against them, a matched
    track becomes the molecule's member k and the others are appended in track order; at the end the molecules are sorted
    stably by field.  They are kept in that order between the steps: a stable sort by field keeps the order of a field's
    molecules, which is all that the match's ties see."""
    r2 = radius_sq_of(radius)
    tables = checked_tables(tables_hw_field, offsets)
    K = len(tables)
    field_ids = np.unique(np.concatenate([f for _, f in tables]))
    hw0, f0 = tables[0]
    order, _, _ = grouped(f0, field_ids)
    mol_hw, mol_field = hw0[order], f0[order]
    member = np.full((K, len(order)), -1, np.int32)
    member[0] = order
    for k in range(1, K):
        hw, field = tables[k]
        b_order, _, b_off = grouped(field, field_ids)
        _, a_seg, a_off = grouped(mol_field, field_ids)                # (the molecules stand sorted: their order is the identity)
        match_of_a, match_of_b, _ = match(mol_hw, a_seg, a_off, hw[b_order], b_off, r2)
        paired = match_of_a >= 0
        member[k][paired] = b_order[match_of_a[paired]]
        new = np.sort(b_order[match_of_b < 0])                         # the unmatched tracks, in track order
        more = np.full((K, len(new)), -1, np.int32)
        more[k] = new
        member = np.concatenate([member, more], axis=1)
        mol_hw, mol_field = np.concatenate([mol_hw, hw[new]]), np.concatenate([mol_field, field[new]])
        order = np.argsort(mol_field, kind='stable')
        member, mol_hw, mol_field = member[:, order], mol_hw[order], mol_field[order]
    return {"member": np.ascontiguousarray(member), "field": mol_field, "hw": mol_hw}
