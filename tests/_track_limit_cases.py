"""Inputs of the limit tests of spot photometry and the two trackers (test_track_limits_host.py, test_gpu_track_limits.py) and of
the fixtures oracle/gen_golden.py --only phot_limits | track_limits | centroid_limits records from the reference: every array
is rebuilt here from a seed, so that the generator, the host tests and the GPU tests work on the same inputs.  Nothing here
needs a GPU or reads the reference.

Conditions the generator asserts before it writes a fixture:
  P1  at least a quarter of the spots have a negative stop and a non-empty wrapped window, at least a tenth an empty window
      (NaN), at least a quarter an ordinary clipped window (no negative stop)                            (phot_shares)
  G1  every field of the 65-frame launch has a trace with a spot in frame 63 and in frame 64
  G2  the extra spot of the 32 769-spot field changes at least one link of the 32 768-spot field
  G5  no case is skipped: spots of one frame lie in different cells, so the reference raises on none of the 300; at least one
      case has H = 1 and one W = 1; every radius 0..4 and every spot_radius of G5_SPOT_RADII occurs; at least a third of the
      cases discard a spot and at least a third contain a trace of length 2 or more
  C   every multi-frame centroid case has present and absent entries"""
import hashlib

import numpy as np

# ---- photometry ------------------------------------------------------------------------------------------------------------
PHOT_SHAPE = (40, 52)
PHOT_PAIRS = ((2, 0), (0, 0), (6, 9), (1, 1), (3, 15), (6, 16), (0, 3), (20, 3), (5, 4), (10, 40))      # (brim, radius)
PHOT_W = (-60, -42, -41, -20, -11, -10, -3, -1, 0, 7, 51, 52, 55, 70, 100)


def checksum(*arrays):
    """SHA-256 over dtype, shape and bytes of the arrays, as a hex string."""
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def phot_image():
    """40 x 52 uint16: noise, a ramp, two bright patches and a saturated corner (medians and sums differ window by window)."""
    rng = np.random.default_rng(7001)
    H, W = PHOT_SHAPE
    img = rng.integers(100, 900, (H, W)).astype(np.int64) + 40 * np.arange(H)[:, None] + 7 * np.arange(W)[None, :]
    img[5:9, 6:11] += 20000
    img[28:34, 40:47] += 9000
    img[:3, :3] = 65535
    img[-1, -1] = 0
    return img.astype(np.uint16)


def phot_spots():
    """(h, w) of the P1 grid: h in [-45, 5) and [36, 90), w in PHOT_W -> int64[1560, 2]."""
    hs = list(range(-45, 5)) + list(range(36, 90))
    return np.array([(h, w) for h in hs for w in PHOT_W], dtype=np.int64)


def phot_wide_stack():
    """P2: the image scaled into uint32 with its maximum at 2^31 - 1, and the same turned by 180 degrees as a second field."""
    img = phot_image().astype(np.int64)
    wide = (img * (2 ** 31 - 1)) // int(img.max())
    assert int(wide.max()) == 2 ** 31 - 1
    return np.stack([wide, wide[::-1, ::-1]]).astype(np.uint32)


def phot_wide_table():
    """P2: (field, h, w) rows in shuffled order: every 7th spot of the grid per field (7 and the 15 columns share no factor)."""
    sp = phot_spots()
    rows = np.concatenate([np.concatenate([np.full((len(sp[3 * f::7]), 1), f), sp[3 * f::7]], axis=1) for f in range(2)])
    return rows[np.random.default_rng(7002).permutation(len(rows))]


def phot_axis(c, r, n):
    """(start, stop, wrapped) of image[max(0, c - r):min(n, c + r + 1)] as numpy reads it; stop <= start: empty."""
    start, stop = max(0, c - r), min(n, c + r + 1)
    wrapped = stop < 0
    if wrapped:
        stop = max(0, stop + n)
    return start, stop, wrapped


def phot_window_classes(spots, radius, shape=PHOT_SHAPE):
    """Per spot: 'wrapped' (a negative stop and a non-empty window), 'wrapped_empty' (a negative stop, nothing left), and where no
    stop is negative - where clipping at the borders and numpy's slicing are the same thing - 'clipped_empty', 'clipped' (non-empty,
    smaller than the full square) or 'full'."""
    out = []
    for h, w in spots:
        a0, a1, wa = phot_axis(int(h), radius, shape[0])
        b0, b1, wb = phot_axis(int(w), radius, shape[1])
        empty = a1 <= a0 or b1 <= b0
        if wa or wb:
            out.append("wrapped_empty" if empty else "wrapped")
        elif empty:
            out.append("clipped_empty")
        else:
            out.append("clipped" if (a1 - a0, b1 - b0) != (2 * radius + 1, 2 * radius + 1) else "full")
    return np.array(out)


def phot_shares(classes):
    """The three shares of condition P1.  'ordinary' counts every window without a negative stop, those clipped to nothing
    included: on the grid the issue sets (15 600 spots) that is 6 809 spots, of which 2 296 are non-empty - the quarter the
    condition asks for can only be meant of the former, and they are exactly the spots on which the clamped reading and the
    reference agreed."""
    classes = np.asarray(classes)
    return {"wrapped": float((classes == "wrapped").mean()),
            "empty": float(np.isin(classes, ("wrapped_empty", "clipped_empty")).mean()),
            "ordinary": float(np.isin(classes, ("clipped_empty", "clipped", "full")).mean())}


# ---- greedy tracker --------------------------------------------------------------------------------------------------------
# a field is (frame_hw: list per frame of int32[n, 2], offsets: list of (d_h, d_w), shape, candidate_radius, spot_radius)
def _unique(hw):
    hw = np.asarray(hw, np.int32).reshape(-1, 2)
    return hw[np.unique(hw[:, 0].astype(np.int64) * 100000 + hw[:, 1], return_index=True)[1]]


def _drifting_field(seed, F, shape, n_spots, always_on=()):
    """Spots at least 3 px apart drifting on the 1/20-pixel grid with jitter and drop-outs; the stage returns every 9 frames."""
    rng = np.random.default_rng(seed)
    H, W = shape
    pts = []
    while len(pts) < n_spots:
        p = (int(rng.integers(3, H - 3)), int(rng.integers(3, W - 3)))
        if all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) > 2 for q in pts):
            pts.append(p)
    pts = np.array(pts, np.int64)
    frames, offs, cum = [pts.astype(np.int32)], [(0.0, 0.0)], np.zeros(2)
    for f in range(1, F):
        step = np.round(rng.uniform(-0.6, 0.6, 2) * 20) / 20
        if f % 9 == 0:
            step = -np.round(cum * 20) / 20
        offs.append((float(step[0]), float(step[1])))
        cum = cum + step
        alive = rng.uniform(size=len(pts)) > 0.2
        if f in always_on:
            alive[:] = True
        jit = rng.integers(-1, 2, pts.shape) * (rng.uniform(size=pts.shape) < 0.3)
        hw = (np.rint(pts - cum).astype(np.int64) + jit)[alive]
        hw = _unique(hw[(hw[:, 0] >= 0) & (hw[:, 0] < H) & (hw[:, 1] >= 0) & (hw[:, 1] < W)])
        frames.append(hw[rng.permutation(len(hw))])
    return frames, offs


G1_FRAMES = (63, 64, 65, 66)
G1_SHAPE = (24, 24)


def g1_fields(F):
    """Three 24 x 24 fields of one launch, cut to F <= 66 frames: fields 0 and 2 are the same, field 1 differs."""
    a = _drifting_field(8101, 66, G1_SHAPE, 12, always_on=(62, 63, 64, 65))
    b = _drifting_field(8102, 66, G1_SHAPE, 13, always_on=(62, 63, 64, 65))
    return [(fr[:F], of[:F], G1_SHAPE, 2, 0) for fr, of in (a, b, a)]


G2_SHAPE = (384, 384)


def g2_fields():
    """[32 769-spot field, 30-spot field, 32 768-spot field] of one launch: a 128 x 128 lattice 3 px apart and the same moved by
    (0, 1) in the next frame; the larger field has one more spot in frame 1, one pixel to the OTHER side of the ancestor at
    (193, 193) - an exact distance tie (1 and 1) that the smaller descendant bin wins."""
    lattice = np.array([(3 * i + 1, 3 * j + 1) for i in range(128) for j in range(128)], np.int32)
    moved = lattice + np.array([0, 1], np.int32)
    rng = np.random.default_rng(8201)
    f1 = moved[rng.permutation(len(moved))]
    extra = np.concatenate([f1[:9000], np.array([[193, 192]], np.int32), f1[9000:]])
    small0 = _unique(np.stack([rng.integers(3, 380, 15), rng.integers(3, 380, 15)], axis=1))
    small = [small0, small0 + rng.integers(-1, 2, small0.shape).astype(np.int32)]
    offs = [(0.0, 0.0), (0.0, 0.0)]
    return [([lattice, extra], offs, G2_SHAPE, 2, 0), ([small[0], _unique(small[1])], offs, G2_SHAPE, 2, 0),
            ([lattice, f1], offs, G2_SHAPE, 2, 0)]


def _a(*rows):
    return np.array(rows, np.int32).reshape(-1, 2)


def g3_cases():
    """name -> field: small radii and degenerate shapes."""
    z = (0.0, 0.0)
    c = {}
    three = [_a((3, 3), (3, 5), (8, 8), (10, 2)), _a((3, 3), (3, 4), (8, 9), (10, 2)), _a((3, 3), (4, 5), (8, 8))]
    c["radius0"] = (three, [z, z, z], (12, 12), 0, 0)
    c["radius1"] = (three, [z, (0.25, 0.0), (-0.25, 0.5)], (12, 12), 1, 0)
    c["radius9_on_16x20"] = ([_a((2, 2), (8, 10), (13, 17), (5, 15)), _a((3, 4), (9, 9), (12, 12), (1, 18)), _a((8, 8), (2, 3))],
                             [z, (0.5, -0.5), (1.0, 0.25)], (16, 20), 9, 0)
    c["strip_1x30"] = ([_a((0, 2), (0, 9), (0, 15), (0, 28)), _a((0, 3), (0, 9), (0, 17), (0, 27)), _a((0, 4), (0, 10), (0, 29))],
                       [z, (0.0, 0.5), (0.0, -0.25)], (1, 30), 2, 0)
    c["strip_30x1"] = ([_a((2, 0), (9, 0), (15, 0), (28, 0)), _a((3, 0), (9, 0), (17, 0), (27, 0)), _a((4, 0), (10, 0), (29, 0))],
                       [z, (0.5, 0.0), (-0.25, 0.0)], (30, 1), 2, 0)
    c["one_pixel"] = ([_a((0, 0)), _a((0, 0)), _a((0, 0))], [z, z, z], (1, 1), 2, 0)
    c["one_frame"] = ([_a((3, 3), (3, 4), (9, 9), (0, 0), (11, 11))], [z], (12, 12), 2, 0)
    return c


def g4_cases():
    """name -> field: accumulated offsets that land on +0.5 and on -0.5, fractional spot_radius, everything discarded."""
    z = (0.0, 0.0)
    frames = [_a((4, 4), (4, 9), (10, 5), (12, 12), (1, 1), (14, 14)), _a((4, 5), (5, 9), (10, 4), (12, 13), (0, 1), (15, 15)),
              _a((3, 4), (4, 10), (11, 5), (13, 12), (1, 0)), _a((4, 4), (4, 9), (10, 5), (12, 12), (2, 2), (14, 15))]
    c = {}
    c["half_plus"] = (frames, [z, (0.25, 0.25), (0.25, 0.25), (1.0, 1.0)], (16, 16), 2, 0)           # 0.5, 0.5 then 1.5, 1.5
    c["half_minus"] = (frames, [z, (-0.25, -0.25), (-0.25, -0.25), (-1.0, -1.0)], (16, 16), 2, 0)
    c["half_mixed"] = (frames, [z, (0.5, -0.5), (-1.0, 1.0), (0.5, -0.5)], (16, 16), 3, 0)           # +-0.5, -+0.5, 0
    for sr in (0.25, 0.5, 2.5, 9):
        c["spot_radius_%g" % sr] = (frames, [z, (0.5, -0.5), (-1.0, 1.0), (0.25, 0.0)], (16, 16), 2, sr)
    return c


G5_SPOT_RADII = (0, 0.25, 0.5, 1, 2.5)
G5_LAUNCHES, G5_PER_LAUNCH = 60, 5


def g5_launches():
    """60 launches of 5 tiny fields each (300 cases); the fields of a launch share shape, frame count, radius and spot_radius.
    H in 1..13, W in 1..17, 1..6 frames, radius 0..4, spot_radius of G5_SPOT_RADII, offsets on the 1/2, 1/4 or 1/20 grid.
    -> list of lists of fields."""
    rng = np.random.default_rng(8501)
    out = []
    for k in range(G5_LAUNCHES):
        H, W = int(rng.integers(1, 14)), int(rng.integers(1, 18))
        if k == 3:
            H = 1
        if k == 4:
            W = 1
        F = int(rng.integers(1, 7))
        radius, sr = k % 5, G5_SPOT_RADII[(k // 5) % 5]
        grid = (2, 4, 20)[k % 3]
        fields = []
        for _ in range(G5_PER_LAUNCH):
            n0 = int(rng.integers(1, max(2, min(H * W, 12))))
            cells = rng.permutation(H * W)[:n0]
            base = np.stack([cells // W, cells % W], axis=1).astype(np.int64)
            frames, offs, cum = [], [], np.zeros(2)
            for f in range(F):
                step = np.zeros(2) if f == 0 else np.round(rng.uniform(-0.6, 0.6, 2) * grid) / grid
                offs.append((float(step[0]), float(step[1])))
                cum = cum + step
                hw = np.rint(base - cum).astype(np.int64) + rng.integers(-1, 2, base.shape) * (rng.uniform(size=base.shape) < 0.1)
                hw = hw[rng.uniform(size=len(hw)) > 0.1]
                hw = _unique(hw[(hw[:, 0] >= 0) & (hw[:, 0] < H) & (hw[:, 1] >= 0) & (hw[:, 1] < W)])
                frames.append(hw[rng.permutation(len(hw))])
            fields.append((frames, offs, (H, W), radius, sr))
        out.append(fields)
    return out


def g6_fields():
    """[good, two spots of frame 1 in one bin, first offset not (0, 0), good again] on 12 x 12, three frames."""
    z = (0.0, 0.0)
    good = ([_a((3, 3), (8, 8), (5, 10)), _a((3, 4), (8, 7), (10, 10)), _a((4, 4), (8, 8))], [z, (0.25, 0.0), (0.0, 0.5)], (12, 12), 2, 0)
    twice = ([_a((3, 3), (8, 8)), _a((3, 4), (6, 6), (6, 6)), _a((4, 4))], [z, z, z], (12, 12), 2, 0)
    shifted = ([_a((3, 3), (8, 8)), _a((3, 4)), _a((4, 4))], [(1.0, 0.0), z, z], (12, 12), 2, 0)
    return [good, twice, shifted, good]


def g7_fields():
    """[two candidate pairs in frame 1, one candidate pair per frame] on 12 x 12, for pair_cap = 1."""
    z = (0.0, 0.0)
    two = ([_a((3, 3), (8, 8)), _a((3, 4), (8, 7)), _a((3, 3))], [z, z, z], (12, 12), 2, 0)
    one = ([_a((3, 3), (9, 9)), _a((3, 4)), _a((3, 3), (6, 9))], [z, z, z], (12, 12), 2, 0)
    return [two, one]


def field_tables(fields):
    """The flat arrays fsq_greedy_tracking takes: hw int32[n, 2], field_start int32[n_fields + 1], counts int32[n_fields, F],
    offsets float64[n_fields, F, 2]."""
    F = len(fields[0][0])
    counts = np.array([[len(x) for x in f[0]] for f in fields], np.int32).reshape(len(fields), F)
    parts = [np.asarray(x, np.int32).reshape(-1, 2) for f in fields for x in f[0]]
    hw = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, 2), np.int32)
    start = np.concatenate([[0], np.cumsum(counts.sum(axis=1))]).astype(np.int32)
    off = np.ascontiguousarray(np.array([f[1] for f in fields], np.float64).reshape(len(fields), F, 2))
    return hw, start, counts, off


def field_checksum(field):
    frames, offs, shape, radius, sr = field
    return checksum(*([np.asarray(x, np.int32).reshape(-1, 2) for x in frames] +
                      [np.asarray(offs, np.float64), np.array(shape, np.int64), np.array([radius, sr], np.float64)]))


def trace_digest(traces):
    return hashlib.sha256(np.ascontiguousarray(traces, dtype=np.int32).tobytes()).hexdigest()


# ---- centroid tracker ------------------------------------------------------------------------------------------------------
# a case is (frames uint[F, H, W], init_hw int32[n, 2], offsets int64[F, 2] or None, search_radius, s_n_cutoff)
C1_SHAPE = (24, 30)
C1_INIT = np.array([(2, 2), (2, 27), (21, 2), (21, 27), (12, 15), (11, 14), (12, 17)], np.int32)


def c1_stack():
    """Five 24 x 30 uint16 frames of noise with a bright patch that wanders by a pixel around (12, 15)."""
    rng = np.random.default_rng(9101)
    fr = rng.integers(90, 400, (5,) + C1_SHAPE).astype(np.uint16)
    for f, (dh, dw) in enumerate(((0, 0), (0, 1), (1, 1), (1, 0), (0, -1))):
        fr[f, 11 + dh:14 + dh, 14 + dw:17 + dw] += 3000
        fr[f, 12 + dh, 15 + dw] += 4000
    return fr


def _off(*rows):
    return np.array(rows, np.int64).reshape(-1, 2)


def centroid_cases():
    """name -> case: C1 (the stack under wrapped windows, offsets beyond the image, R of 0, 11 and 12, cut-offs of inf, -1 and
    NaN, one frame, no offsets), C2 (flat frames: S/N is 0/0), C3 (the launch of the all-zero frame without that frame)."""
    fr, init = c1_stack(), C1_INIT
    small = _off((0, 0), (1, 0), (-1, 2), (0, -1), (2, 1))
    c = {}
    c["no_offsets"] = (fr, init, None, 3, 3.0)
    c["wrap_rows"] = (fr, init, _off((0, 0), (30, 0), (0, 0), (26, 1), (0, 0)), 3, 3.0)         # window wholly beyond row 0
    c["wrap_cols"] = (fr, init, _off((0, 0), (0, 36), (0, 0), (-1, 33), (0, 0)), 3, 3.0)        # ... beyond column 0
    c["beyond_image"] = (fr, init, _off((0, 0), (100, 0), (0, 0), (0, -100), (-100, 100)), 3, 3.0)
    c["beyond_image_neg"] = (fr, init, _off((0, 0), (0, 100), (-100, -100), (0, 0), (100, -100)), 2, 3.0)
    c["R0"] = (fr, init, small, 0, 3.0)
    c["R11"] = (fr, init, _off((0, 0), (0, 1), (0, -1), (1, 0), (0, 0)), 11, 3.0)               # 23 of 24 rows
    c["R12"] = (fr, init, None, 12, 3.0)                                                        # 25 rows never fit
    c["cut_inf"] = (fr, init, small, 3, float("inf"))
    c["cut_minus1"] = (fr, init, small, 3, -1.0)
    c["cut_nan"] = (fr, init, small, 3, float("nan"))
    c["one_frame"] = (fr[:1], init, None, 3, 3.0)
    flat = np.full((4,) + C1_SHAPE, 500, np.uint16)
    c["flat"] = (flat, init, _off((0, 0), (1, -1), (0, 2), (-1, 0)), 3, 3.0)
    c["without_zero_frame"] = (fr[[0, 1, 3]], init, _off((0, 0), (1, 0), (0, -1)), 3, 3.0)
    return c


def c3_with_zero_frame():
    """C3: the case 'without_zero_frame' with an all-zero frame put in as frame 2 (whole-pixel offset (0, 0))."""
    fr, init, off, R, cut = centroid_cases()["without_zero_frame"]
    frames = np.stack([fr[0], fr[1], np.zeros_like(fr[0]), fr[2]])
    return frames, init, _off(off[0], off[1], (0, 0), off[2]), R, cut


def c4_case():
    """C4: three uint32 fields (the C1 stack scaled so that its maximum is 2^31 - 1, the same upside down, the same with its
    frames in reverse order), 257 spots with interleaved field numbers, whole-pixel offsets per field.
    -> (frames uint32[3, 5, 24, 30], init int32[257, 2], spot_field int32[257], offsets int64[3, 5, 2], R, cutoff)"""
    fr = c1_stack().astype(np.int64)
    wide = ((fr * (2 ** 31 - 1)) // int(fr.max())).astype(np.uint32)
    assert int(wide.max()) == 2 ** 31 - 1
    frames = np.stack([wide, wide[:, ::-1].copy(), wide[::-1].copy()])
    rng = np.random.default_rng(9401)
    init = np.stack([rng.integers(2, C1_SHAPE[0] - 2, 257), rng.integers(2, C1_SHAPE[1] - 2, 257)], axis=1).astype(np.int32)
    init[:7] = C1_INIT
    fld = (np.arange(257) % 3).astype(np.int32)
    fld[200:] = rng.integers(0, 3, 57)
    offs = rng.integers(-2, 3, (3, 5, 2)).astype(np.int64)
    offs[:, 0] = 0
    return frames, init, fld, offs, 3, 3.0


C5_SHAPE = (1025, 1025)


def c5_case():
    """C5: R = 512 on two 1025 x 1025 uint32 frames with pixels in [2^30, 2^31), one spot at the centre: the weighted sums of
    the window reach 2^61.  The cut-off is -1, so that the centroid itself is the result."""
    rng = np.random.default_rng(9501)
    fr = rng.integers(2 ** 30, 2 ** 31, (2,) + C5_SHAPE, dtype=np.int64).astype(np.uint32)
    fr[1, 400:520, 300:620] = 2 ** 31 - 1                          # a bright block up and to the left pulls the centroid
    fr[1, 700:, 700:] = 2 ** 30
    return fr, np.array([(512, 512)], np.int32), None, 512, -1.0


def centroid_checksum(case):
    frames, init, off, R, cut = case
    return checksum(frames, np.asarray(init, np.int32), np.zeros((0, 2), np.int64) if off is None else np.asarray(off, np.int64),
                    np.array([R], np.int64), np.array([cut], np.float64))
