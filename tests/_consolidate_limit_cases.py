"""Cases of the consolidation limit tests, and the one Python restatement of the reference's loops (pflib.py:466, 477-519).

tests/golden/consolidate_limits.npz (oracle/gen_golden.py --only consolidate_limits) holds, for every field of every recorded
case, what the unmodified find_peptides of the reference did with it: its candidate detector and its fitter are replaced at
run time by stand-ins that hand back the case's candidate pixels and crafted (h_0, w_0, ..., fit_img), and lines 441-520 run
as written.  No torch, no GPU here.

How a field is described.  A candidate is a pixel (h, w), 2 <= h < H - 2, in raster order, the fitter's centre in the 5 x 5
window (fh, fw) - the reference maps it to the frame as (fh + h) - 2.5, and so does centres() below, in the same order of
operations - and the integer q = the sum of squares of the fit's residual.  The frame is a checkerboard of 0 and 25: every
5 x 5 patch of it has mean 12 or 13 and a sum of squared deviations of exactly 3 900, so r_2 = 1.0 - q / 3900.0
(pflib.py:463-465) with every intermediate an exact integer; equal q means an exact tie.  A candidate marked `flat` gets an
all-zero patch: r_2 = 1 - 0 / 0 = NaN for q = 0 and 1 - q / 0 = -inf otherwise.  r_2 = +inf and -0.0 are no values of that
expression (a sum of squares over a sum of squares, taken from 1.0); the cases that hold them (`forced`) are not recorded and
are checked against the C oracle and the restatement alone.  One centre, 0.49999999999999994, is no value of (fh + h) - 2.5
in float64 for h >= 2; its stand-in hands back a numpy.longdouble, which the reference carries through unrounded (`exact`).

What the groups are for (csrc/fsq_consolidate.hip):
  turn_*      chains of overlapping windows of 63, 64, 65 and 130 candidates, R^2 rising, falling, alternating and tied: the
              64-member walk of k5c_turns (mb = root & ~63 .. last), the 64-entry survivor chunks and the 8 strips of k5_consolidate;
              a snake over several rows; two components whose index ranges interleave.
  stop_*      the scan's stopping rule: the first rival that is not smaller at a chosen cell of the (clipped) window, smaller
              rivals before it (they die) and after it (they must survive that turn).  A rival that is alive at a
              candidate's turn is raster-later than the candidate - a raster-earlier one had its own turn, which killed one
              of the two - so the stopping rival sits behind the centre cell: cells 127, 128 and the last one of the full
              13 x 13 and 15 x 15 windows, 191 and 192 (the seam of the two passes at radius 5), and 63 and 64 in windows
              clipped by the frame's top, where the centre cell's number is small.  Cell 0 never holds one.
  radius_*    centre distance exactly r (3-4-5), the next representable distance beyond, and pairs with full-mantissa
              centres within a few ulp of the circle.
  r2_*        ties, NaN on either side, -inf, 0.0, +inf and -0.0 (forced), under thresholds equal to an r_2, one ulp above
              it, NaN, +inf and -inf.
  rekey_*     the re-key (pflib.py:514-519) in both rounding modes: half-integer centres, -0.5, 0.49999999999999994, every
              kind of target cell, the asserting ones, keys outside the frame on all four sides; all of them between
              ordinary fields in one launch.  `outside_collision` is the documented deviation (two keys outside the frame
              that collide: the reference asserts, the library and the oracle keep both): host test only.
  layout_*    5 x 5, 5 x 64 and 64 x 5 frames, every pixel a survivor, one candidate, every candidate filtered, empty fields
              first, in the middle and last, 1, 257, 1 023 and 1 024 fields (the library's own choice of form switches at 1 024).
  wild_*      seeded fields with centres up to 3 px off their pixel (the existing test's "wild" kind, other seeds).
"""
import functools
import math
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLD, "consolidate_limits.npz")
SS_TOT = 3900.0             # sum of squared deviations of every 5 x 5 patch of the 0 / 25 checkerboard
NGW = 3                     # 64-lane groups per pass of a turn's window scan (csrc/fsq_consolidate.hip)


# ------------------------------------------------------------------------------------------------ the restatement
def py2_round(x):
    """Python 2's round(): half away from zero (C's round()), exact for |x| < 2^52."""
    x = float(x)
    t = math.trunc(x)
    return t + (1 if x - t >= 0.5 else 0) - (1 if t - x >= 0.5 else 0)


def py3_round(x):
    """Python 3's built-in round(): half to even."""
    return int(round(float(x)))


def consolidated_bins(h, w, h0, w0, r2, H, W, thr, radius):
    """The reference's dict {(h, w): candidate} after the R^2 filter and the consolidation loop, before the re-key."""
    bins = {}
    for i in range(len(h)):
        if not (r2[i] < thr):                                   # pflib.py:466 (NaN passes)
            bins.setdefault((int(h[i]), int(w[i])), i)
    for (hh, ww), i in list(bins.items()):                      # pflib.py:479-512
        if (hh, ww) not in bins:
            continue
        dead = False
        for hd in range(max(0, hh - radius - 2), min(hh + radius + 3, H)):
            for wd in range(max(0, ww - radius - 2), min(ww + radius + 3, W)):
                if (hd == hh and wd == ww) or (hd, wd) not in bins:
                    continue
                k = bins[(hd, wd)]
                if (h0[i] - h0[k]) ** 2 + (w0[i] - w0[k]) ** 2 > radius ** 2:
                    continue
                if r2[i] > r2[k]:
                    del bins[(hd, wd)]
                else:
                    del bins[(hh, ww)]
                    dead = True
                    break
            if dead:
                break
    return bins


def reference_consolidate(h, w, h0, w0, r2, H, W, thr, radius, py2=True):
    """-> (kept candidate numbers in the reference's dict order, their keys) or None when the assert of pflib.py:518 fires."""
    rnd = py2_round if py2 else py3_round
    bins = consolidated_bins(h, w, h0, w0, r2, H, W, thr, radius)
    for (hh, ww), i in list(bins.items()):                      # pflib.py:514-519
        hr, wr = rnd(h0[i]), rnd(w0[i])
        if hr != hh or wr != ww:
            del bins[(hh, ww)]
            if (hr, wr) in bins:
                return None
            bins.setdefault((hr, wr), i)
    return list(bins.values()), list(bins.keys())


def stopping_turns(f, H, W, thr, radius):
    """The turns of the consolidation loop that end at a rival that is not smaller: [(candidate, cell of that rival in the
    candidate's clipped window, rivals deleted before it, living rivals behind it in the window)] - the restatement's loop with
    a record of what it does."""
    h, w = f.h, f.w
    h0, w0 = f.centres()
    r2 = f.r2()
    bins, out = {}, []
    for i in range(len(h)):
        if not (r2[i] < thr):
            bins.setdefault((int(h[i]), int(w[i])), i)
    for (hh, ww), i in list(bins.items()):
        if (hh, ww) not in bins:
            continue
        h_lo, w_lo = max(0, hh - radius - 2), max(0, ww - radius - 2)
        w_hi = min(ww + radius + 3, W)
        cells = [(hd, wd) for hd in range(h_lo, min(hh + radius + 3, H)) for wd in range(w_lo, w_hi)]
        killed = 0
        for c, (hd, wd) in enumerate(cells):
            if (hd == hh and wd == ww) or (hd, wd) not in bins:
                continue
            k = bins[(hd, wd)]
            if (h0[i] - h0[k]) ** 2 + (w0[i] - w0[k]) ** 2 > radius ** 2:
                continue
            if r2[i] > r2[k]:
                del bins[(hd, wd)]
                killed += 1
            else:
                del bins[(hh, ww)]
                behind = sum(1 for c2 in cells[c + 1:] if c2 in bins and
                             not (h0[i] - h0[bins[c2]]) ** 2 + (w0[i] - w0[bins[c2]]) ** 2 > radius ** 2)
                out.append((i, c, killed, behind))
                break
    return out


# ------------------------------------------------------------------------------------------------ fields and cases
@functools.lru_cache(maxsize=None)
def four_squares(q):
    """q = a^2 + b^2 + c^2 + d^2 in integers (Lagrange): the residuals of the stand-in's fit_img."""
    a = math.isqrt(q)
    while a >= 0:
        r1 = q - a * a
        b = min(a, math.isqrt(r1))
        while b >= 0:
            r2 = r1 - b * b
            c = min(b, math.isqrt(r2))
            while c >= 0:
                d = math.isqrt(r2 - c * c)
                if d * d == r2 - c * c and d <= c:
                    return a, b, c, d
                c -= 1
            b -= 1
        a -= 1
    raise AssertionError(q)


class Field:
    """One field's candidate table.  cands: (h, w, dh, dw, q) or (h, w, dh, dw, q, flat) in raster order; the fitter's centre is
    (2.5 + dh, 2.5 + dw) in its window.  forced: {candidate: r_2} for the values the reference's expression cannot give;
    exact: {candidate: h0} for the centre that needs the long double stand-in."""

    def __init__(self, cands, forced=None, exact=None, fit=None):
        cands = [tuple(c) + (False,) * (6 - len(c)) for c in cands]
        self.h = np.array([c[0] for c in cands], np.int32)
        self.w = np.array([c[1] for c in cands], np.int32)
        self.fh = 2.5 + np.array([c[2] for c in cands], np.float64)
        self.fw = 2.5 + np.array([c[3] for c in cands], np.float64)
        if fit is not None:                                     # full-mantissa window coordinates, given as they are
            self.fh, self.fw = np.array(fit[0], np.float64), np.array(fit[1], np.float64)
        self.q = np.array([c[4] for c in cands], np.int64)
        self.flat = np.array([c[5] for c in cands], bool)
        self.forced = dict(forced or {})
        self.exact = dict(exact or {})
        order = self.h.astype(np.int64) * 100000 + self.w
        assert (np.diff(order) > 0).all(), "candidates must be in raster order, one per pixel"

    def __len__(self):
        return len(self.h)

    def centres(self):
        """(h0, w0) as the reference computes them: h_0 + h - 2.5 (pflib.py:461), left to right, in float64."""
        h0 = (self.fh + self.h.astype(np.float64)) - 2.5
        w0 = (self.fw + self.w.astype(np.float64)) - 2.5
        for i, v in self.exact.items():
            h0[i] = v
        return h0, w0

    def r2(self):
        with np.errstate(all="ignore"):
            r2 = np.where(self.flat, np.where(self.q == 0, np.nan, -np.inf), 1.0 - self.q.astype(np.float64) / SS_TOT)
        for i, v in self.forced.items():
            r2[i] = v
        return r2

    def image(self, H, W):
        """The frame: the checkerboard, zero under the patches of the flat candidates; no other candidate's patch may touch those."""
        yy, xx = np.mgrid[0:H, 0:W]
        board = (25 * ((yy + xx) & 1)).astype(np.uint16)
        img = board.copy()
        assert ((self.h >= 2) & (self.h < H - 2) & (self.w >= 2) & (self.w < W - 2)).all()
        for i in np.flatnonzero(self.flat):
            img[self.h[i] - 2:self.h[i] + 3, self.w[i] - 2:self.w[i] + 3] = 0
        for i in np.flatnonzero(~self.flat):
            sl = (slice(self.h[i] - 2, self.h[i] + 3), slice(self.w[i] - 2, self.w[i] + 3))
            assert np.array_equal(img[sl], board[sl]), "a flat patch reaches into the patch of candidate %d" % i
        return img

    def fit_image(self, i, sub_img):
        """fit_img of candidate i for the patch the reference hands the fitter: the patch itself, less residuals a, b, c, d with
        a^2 + b^2 + c^2 + d^2 = q on four of its zero pixels."""
        fit = np.array(sub_img, dtype=np.float64)
        zeros = np.argwhere(np.asarray(sub_img) == 0)
        for (y, x), e in zip(zeros, four_squares(int(self.q[i]))):
            fit[y, x] = -float(e)
        return fit


class Case:
    """One launch: frame shape, radius, threshold, the distinct fields and the order (`layout`, indices into them) in which the
    launch holds them.  default_form: also run with the library's own choice of form.  recorded: the fixture holds it.
    gpu: the GPU test runs it."""

    def __init__(self, name, H, W, radius, thr, fields, layout=None, default_form=False, gpu=True):
        self.name, self.H, self.W, self.radius, self.thr = name, int(H), int(W), int(radius), float(thr)
        self.fields = list(fields)
        self.layout = list(range(len(self.fields))) if layout is None else list(layout)
        self.default_form, self.gpu = default_form, gpu
        self.recorded = not any(f.forced for f in self.fields)

    def expected(self, py2):
        """Per distinct field, by the restatement."""
        out = []
        for f in self.fields:
            h0, w0 = f.centres()
            out.append(reference_consolidate(f.h, f.w, h0, w0, f.r2(), self.H, self.W, self.thr, self.radius, py2))
        return out


def launch_tables(case, row_dtype):
    """(counts int32[n + 1], offsets int32[n + 1], rows) of the launch, as fsq_detect and the fitter would leave them."""
    per = []
    for f in case.fields:
        h0, w0 = f.centres()
        per.append((f.h, f.w, h0, w0, f.r2()))
    n = len(case.layout)
    counts = np.array([len(case.fields[u]) for u in case.layout] + [0], np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts[:-1])]).astype(np.int32)
    total = int(counts[:-1].sum())
    counts[-1] = total
    rows = np.zeros(total, row_dtype)
    rows["key_h"] = rows["key_w"] = -1
    for s, u in enumerate(case.layout):
        h, w, h0, w0, r2 = per[u]
        a = slice(offsets[s], offsets[s] + len(h))
        rows["h"][a], rows["w"][a], rows["h0"][a], rows["w0"][a], rows["r2"][a], rows["field"][a] = h, w, h0, w0, r2, s
    assert n >= 1
    return counts, offsets, rows


# ---- turn order
def _pattern(kind, n):
    k = np.arange(n)
    if kind == "rising":                                        # R^2 rises along raster order: q falls
        return 1000 - 5 * k
    if kind == "falling":
        return 100 + 5 * k
    if kind == "alt":
        return np.where(k % 2 == 0, 300, 200) + 3 * (k % 7)
    if kind == "tied":
        return np.full(n, 400)
    if kind == "saw":                                           # rises for five, then drops: every turn both deletes and stops somewhere
        return 600 - 40 * (k % 5) + (k // 5) % 3
    raise KeyError(kind)


def _row_chain(n, kind, step=1):
    return Field([(2, 2 + step * k, 0.25 * ((k % 3) - 1), 0.25 * ((k % 5) - 2) / 2, int(q)) for k, q in enumerate(_pattern(kind, n))])


def _col_chain(n, kind):
    return Field([(2 + k, 2, 0.25 * ((k % 5) - 2) / 2, 0.25 * ((k % 3) - 1), int(q)) for k, q in enumerate(_pattern(kind, n))])


def _snake(n, per_row, step, rows_apart, kind):
    return Field([(2 + rows_apart * (k // per_row), 2 + step * (k % per_row), 0.25 * ((k % 3) - 1), 0.25 * (((k // per_row) % 3) - 1), int(q))
                  for k, q in enumerate(_pattern(kind, n))])


def _turn_cases():
    out = []
    kinds = ("rising", "falling", "alt", "tied", "saw")
    for n in (63, 64, 65):
        out.append(Case("turn_row_%d" % n, 5, n + 4, 4, 0.5, [_row_chain(n, k) for k in kinds]))
        out.append(Case("turn_col_%d" % n, n + 4, 5, 4, 0.5, [_col_chain(n, k) for k in kinds]))
    # 130 = two rows of 65, three pixels apart: one component, root 0, last 129
    out.append(Case("turn_rows_130", 10, 69, 4, 0.5, [_snake(130, 65, 1, 3, k) for k in kinds]))
    # a chain three pixels apart over the whole width: every strip border of the blocks form (strip_w = ceil(64 / 8) = 8) is crossed
    out.append(Case("turn_strips", 9, 64, 4, 0.5, [_row_chain(20, k, step=3) for k in kinds]))
    # a snake: 130 candidates, 20 to a row three pixels apart, the rows five apart (the windows of neighbouring rows overlap)
    out.append(Case("turn_snake_130", 40, 64, 4, 0.5, [_snake(130, 20, 3, 5, k) for k in kinds]))
    # two components whose index ranges interleave: the left ends and the right ends of rows, 30 columns apart (2 (r + 2) = 12 < 30)
    inter = []
    for kind in ("rising", "falling", "saw"):
        q = _pattern(kind, 80)
        cands = []
        for row in range(8):
            for half in range(2):
                for j in range(5):
                    k = len(cands)
                    cands.append((2 + 4 * row, 2 + 40 * half + 2 * j, 0.25 * ((k % 3) - 1), 0.0, int(q[k])))
        inter.append(Field(cands))
    out.append(Case("turn_interleaved", 36, 64, 4, 0.5, inter))
    return out


# ---- the stopping rule
def _stop_field(H, W, radius, ch, cw, stop_cell, tie):
    """Candidate C at (ch, cw); S, the first rival that is not smaller, at cell `stop_cell` of C's clipped window; smaller rivals
    B before S (C deletes them) and A behind S (they survive C's turn).  S and the A sit on a circle of 0.95 r around C's
    centre, 72 degrees apart: rivals of C, not of each other, so what C's turn leaves is what the field keeps."""
    rw = radius + 2
    h_lo, w_lo, h_hi, w_hi = max(0, ch - rw), max(0, cw - rw), min(ch + rw + 1, H), min(cw + rw + 1, W)
    ww = w_hi - w_lo
    ncell = (h_hi - h_lo) * ww
    centre = (ch - h_lo) * ww + (cw - w_lo)

    def ok(c):
        hd, wd = h_lo + c // ww, w_lo + c % ww
        return centre < c < ncell and 2 <= hd < H - 2 and 2 <= wd < W - 2
    assert ok(stop_cell), (stop_cell, centre, ncell)
    before = [c for c in (centre + 1, centre + 2, stop_cell - 64, stop_cell - 2, stop_cell - 1) if ok(c) and c < stop_cell]
    behind = [c for c in (stop_cell + 1, stop_cell + 2, stop_cell + 64, ncell - 1 - 2 * ww - 3, ncell - 1 - 2 * ww - 2) if ok(c) and c > stop_cell]
    before, behind = sorted(set(before)), sorted(set(behind))[:4]
    ring = [(0.95 * radius * math.cos(2 * math.pi * k / 5), 0.95 * radius * math.sin(2 * math.pi * k / 5)) for k in range(5)]
    ring = [(round(a * 4) / 4, round(b * 4) / 4) for a, b in ring]          # (multiples of 1/4: exact squares)
    cands = {centre: (0.0, 0.0, 300)}
    for k, c in enumerate(before):
        cands[c] = (0.25 * (k + 1), -0.25 * (k + 1), 400 + k)
    cands[stop_cell] = ring[0] + (300 if tie else 200,)
    for k, c in enumerate(behind):
        cands[c] = ring[1 + k] + (500 + k,)
    rows = []
    for c in sorted(cands):
        hd, wd = h_lo + c // ww, w_lo + c % ww
        th, tw, q = cands[c]
        rows.append((hd, wd, ch + th - hd, cw + tw - wd, q))
    return Field(rows)


STOPS = {   # name -> (H, W, radius, ch, cw, stopping cells)
    "stop_r4_full": (17, 17, 4, 8, 8, (85, 127, 128, 168)),                 # 13 x 13 = 169 cells, centre 84, one pass
    "stop_r5_full": (19, 19, 5, 9, 9, (113, 127, 128, 191, 192, 224)),      # 15 x 15 = 225 cells, centre 112, two passes
    "stop_r4_corner": (17, 17, 4, 2, 3, (63, 64, 89)),                      # 9 x 10 = 90 cells, centre 23
    "stop_r5_corner": (19, 19, 5, 2, 2, (63, 64, 99)),                      # 10 x 10 = 100 cells, centre 22
    "stop_r5_top": (19, 19, 5, 5, 9, (83, 127, 128, 191, 192, 194)),        # 13 x 15 = 195 cells, centre 82: both passes, clipped
    "stop_r4_top": (17, 17, 4, 3, 8, (63, 64, 127, 128, 129)),              # 10 x 13 = 130 cells, centre 45
}


def _stop_cases():
    out = []
    for name, (H, W, radius, ch, cw, cells) in STOPS.items():
        fields = [_stop_field(H, W, radius, ch, cw, c, tie) for c in cells for tie in (False, True)]
        out.append(Case(name, H, W, radius, 0.5, fields))
    return out


def stop_cells(name):
    """The stopping cell every field of a stop_* case is built for."""
    return [c for c in STOPS[name][5] for tie in (False, True)]


# ---- the radius test
def _radius_cases():
    # 3-4-5 at r = 5: C at pixel (2, 2), centre (2, 2); K at pixel (5, 6).  Its centre (5, 6): a rival (25 > 25 is false).
    # One ulp of 5.0 further down - 7.5 + 2^-50 and 5 + 2^-50 are both representable, so the reference holds exactly that: not one.
    on = Field([(2, 2, 0., 0., 100), (5, 6, 0., 0., 200)])
    ulp = float(np.spacing(5.0))
    off = Field([(2, 2, 0., 0., 100), (5, 6, 0., 0., 200)], fit=([2.5, 2.5 + ulp], [2.5, 2.5]))
    inside = Field([(2, 2, 0., 0., 100), (5, 6, 0., 0., 200)], fit=([2.5, 2.5 - ulp], [2.5, 2.5]))
    # the same with the better candidate second: the first one dies instead
    on2 = Field([(2, 2, 0., 0., 200), (5, 6, 0., 0., 100)])
    off2 = Field([(2, 2, 0., 0., 200), (5, 6, 0., 0., 100)], fit=([2.5, 2.5 + ulp], [2.5, 2.5]))
    out = [Case("radius_345", 10, 11, 5, 0.5, [on, off, inside, on2, off2])]
    rng = np.random.default_rng(20250505)
    fields = []
    for k in range(48):
        c = 9 + rng.uniform(-0.5, 0.5, 2)                       # C's centre around pixel (9, 9), full mantissa
        ang = rng.uniform(0, 2 * math.pi)
        d = 5.0 * (1.0 + float(rng.integers(-3, 4)) * 2.0 ** -52)
        t = c + d * np.array([math.sin(ang), math.cos(ang)])
        px = np.rint(t).astype(int)
        cands = sorted([(9, 9, c[0] - 9, c[1] - 9, 100 + k % 2 * 200), (int(px[0]), int(px[1]), t[0] - px[0], t[1] - px[1], 200)])
        fields.append(Field(cands))
    out.append(Case("radius_mantissa", 19, 19, 5, 0.5, fields))
    return out


# ---- R^2
def _r2_zoo():
    """Pairs and triples of rivals: pixels (4, 4), (4, 9) and (9, 4), five apart so that a flat patch touches no other patch,
    their centres moved to within 3 of each other (radius 4).  (q, flat) per candidate."""
    def f(*spec, **kw):
        pos = [(4, 4, 0., 1.), (4, 9, 0., -1.), (9, 4, -1., 1.)]
        return Field([p + s for p, s in zip(pos, spec)], **kw)
    return [
        f((400, False), (400, False)),                          # tie: the first one's turn finds "not smaller" and it dies
        f((400, False), (400, False), (400, False)),
        f((0, True), (400, False)),                             # NaN first: loses its comparison
        f((400, False), (0, True)),                             # NaN second: the first one is "not greater" and dies
        f((0, True), (0, True)),
        f((7, True), (400, False)),                             # -inf
        f((400, False), (7, True)),
        f((7, True), (9, True)),                                # -inf against -inf: a tie
        f((0, True), (7, True)),                                # NaN against -inf
        f((7, True), (0, True)),
        f((3900, False), (400, False)),                         # r_2 = 0.0 exactly
        f((400, False), (3900, False)),
        f((1000, False), (1001, False), (1002, False)),         # around the threshold of the r2_thr_equal cases
        f((1001, False), (1000, False)),
        f((3900, False), (7800, False), (0, True)),             # 0.0, -1.0 and NaN
    ]


def _r2_forced():
    def f(r2a, r2b):
        return Field([(4, 4, 0., 1., 400), (4, 9, 0., -1., 400)], forced={0: r2a, 1: r2b})
    return [f(np.inf, 0.9), f(0.9, np.inf), f(np.inf, np.inf), f(np.inf, np.nan), f(np.nan, np.inf), f(-np.inf, np.inf),
            f(-0.0, 0.0), f(0.0, -0.0), f(-0.0, -0.0), f(-0.0, -1e-300), f(1e-300, -0.0)]


def _r2_cases():
    at = 1.0 - 1000.0 / SS_TOT                                  # the r_2 of q = 1000
    thr = {"half": 0.5, "equal": at, "ulp_above": float(np.nextafter(at, np.inf)), "ulp_below": float(np.nextafter(at, -np.inf)),
           "zero": 0.0, "nan": float("nan"), "pinf": float("inf"), "ninf": float("-inf")}
    out = [Case("r2_thr_%s" % k, 14, 14, 4, v, _r2_zoo()) for k, v in thr.items()]
    out += [Case("r2_forced_thr_%s" % k, 14, 14, 4, thr[k], _r2_forced()) for k in ("zero", "pinf", "ninf", "nan")]
    out.append(Case("r2_forced_thr_negzero", 14, 14, 4, -0.0, _r2_forced()))
    return out


# ---- the re-key
# 17 x 17 frames at radius 2: the pixels 2, 7 and 12 are five apart, so no two candidates on them are ever compared (the window
# reaches 4) and every one of them is alive when the re-key starts - unless the case wants a deletion.
ORDINARY = [(2, 2, 0.25, -0.25, 100), (7, 7, 0., 0.25, 100), (12, 12, -0.25, 0., 2500)]


def rekey_fields():
    """name -> Field; the names say what each reaches (tests/test_consolidate_limits_host.py proves it)."""
    F = {}
    F["ordinary"] = Field(ORDINARY)
    # x.5 with even and odd integer parts, in h and in w, up and down: half away from zero and half to even part ways at the even ones
    F["half_even_odd"] = Field([(2, 2, 0.5, 0., 100), (2, 7, 0., 0.5, 100), (2, 12, -0.5, 0., 100),
                                (7, 2, 0.5, 0.5, 100), (7, 7, 0., -0.5, 100), (7, 12, 0.5, -0.5, 100),
                                (12, 2, -0.5, 0., 100), (12, 7, 0.5, 0., 100), (12, 12, 0., 0.5, 100)])
    F["half_odd_pixels"] = Field([(3, 3, 0.5, 0., 100), (3, 8, 0., 0.5, 100), (3, 13, -0.5, -0.5, 100),
                                  (8, 3, -0.5, 0., 100), (8, 8, 0.5, 0.5, 100), (13, 13, 0., -0.5, 100)])
    F["minus_half"] = Field([(2, 2, -2.5, 0., 100), (2, 7, 0., 0., 100), (7, 2, 0., -2.5, 100)])       # centres -0.5: -1 or 0
    F["just_below_half"] = Field([(2, 2, 0., 0., 100), (7, 7, 0., 0., 100)], exact={0: 0.49999999999999994})   # 0 in both modes; floor(x + 0.5) says 1
    F["into_empty"] = Field([(2, 2, 1.0, 2.0, 100), (7, 7, 0., 0., 100)])
    F["into_filtered"] = Field([(2, 2, 0., 5.0, 100), (2, 7, 0., 0., 2500), (7, 7, 0., 0., 100)])
    F["into_deleted"] = Field([(2, 2, 0., 2.0, 100), (2, 4, 0., 0.25, 300), (7, 7, 0., 0., 100)])       # candidate 0 deletes 1, then takes its cell
    F["into_left_by_earlier"] = Field([(2, 2, 5.0, 0., 100), (2, 7, 0., -5.0, 100)])                    # 0 -> (7, 2); 1 -> (2, 2)
    F["into_left_by_later"] = Field([(2, 2, 0., 5.0, 100), (2, 7, 5.0, 0., 100)])                       # 0 -> (2, 7) while 1 is still there: assert
    F["into_stayer"] = Field([(2, 2, 0., 5.0, 100), (2, 7, 0.25, 0., 100)])                             # assert
    F["into_stayer_later_mover"] = Field([(2, 2, 0.25, 0., 100), (2, 7, 0., -5.0, 100)])                # the mover is the later one: assert
    F["two_movers_one_target"] = Field([(2, 2, 0., 2.0, 100), (2, 7, 0., -3.0, 100)])                   # both -> (2, 4): assert
    F["swap"] = Field([(2, 2, 0., 5.0, 100), (2, 7, 0., -5.0, 100)])                                    # assert
    F["chain_of_three"] = Field([(2, 2, 5.0, 0., 100), (2, 7, 0., -5.0, 100), (2, 12, 0., -5.0, 100)])  # (2,2)->(7,2), (2,7)->(2,2), (2,12)->(2,7)
    F["chain_of_three_reversed"] = Field([(2, 2, 0., 5.0, 100), (2, 7, 0., 5.0, 100), (2, 12, 5.0, 0., 100)])   # each into a later mover's cell: assert
    F["out_top"] = Field([(2, 2, -3.0, 0., 100), (7, 7, 0., 0., 100)])                                   # key (-1, 2): the negative row
    F["out_top_far"] = Field([(2, 7, -5.0, 0.25, 100), (7, 7, 0., 0., 100)])                             # key (-3, 7)
    F["out_left"] = Field([(7, 2, 0., -3.0, 100), (7, 7, 0., 0., 100)])                                  # key (7, -1)
    F["out_bottom"] = Field([(7, 7, 0., 0., 100), (14, 7, 3.0, 0., 100)])                                # key (17, 7) = (H, 7)
    F["out_right"] = Field([(7, 7, 0., 0., 100), (7, 14, 0., 3.0, 100)])                                 # key (7, 17) = (7, W)
    F["out_corner"] = Field([(2, 2, -3.0, -3.0, 100), (7, 7, 0., 0., 100)])                              # key (-1, -1)
    F["out_all_sides"] = Field([(2, 7, -3.0, 0., 100), (7, 2, 0., -3.0, 100), (7, 7, 0.5, 0.5, 100), (7, 14, 0., 3.0, 100), (14, 7, 3.0, 0., 100)])
    F["out_half"] = Field([(2, 2, -2.5, -2.5, 100), (7, 7, 0., 0., 100)])                                # (-0.5, -0.5): (-1, -1) or (0, 0)
    F["into_left_for_negative_row"] = Field([(2, 2, -3.0, 0., 100), (2, 7, 0., -5.0, 100)])            # 0 -> (-1, 2); 1 -> (2, 2), which 0 has left
    F["into_left_for_right_of_frame"] = Field([(2, 12, 0., 5.0, 100), (7, 12, -5.0, 0., 100)])          # 0 -> (2, 17); 1 -> (2, 12)
    F["only_negative_rows"] =Field([(2, 2, -3.0, 0., 100), (2, 7, -4.0, 0., 100), (2, 12, -3.0, 0., 100)])
    return F


ASSERTING = ("into_left_by_later", "into_stayer", "into_stayer_later_mover", "two_movers_one_target", "swap", "chain_of_three_reversed")
HALF_INTEGER = ("half_even_odd", "half_odd_pixels", "minus_half", "out_half")


def _rekey_cases():
    F = rekey_fields()
    names = list(F)
    out = [Case("rekey_each", 17, 17, 2, 0.5, [F[n] for n in names])]
    # every one of them between two ordinary fields in one launch
    layout = [0]
    for k in range(1, len(names)):
        layout += [k, 0]
    out.append(Case("rekey_embedded", 17, 17, 2, 0.5, [F[n] for n in names], layout=layout))
    # two keys outside the frame that collide: the reference asserts, the library and the oracle do not look (host test only)
    out.append(Case("outside_collision", 17, 17, 2, 0.5, [Field([(2, 2, -3.0, 2.0, 100), (2, 7, -3.0, -3.0, 100)]),
                                                         Field([(7, 14, 0., 3.0, 100), (12, 14, -5.0, 3.0, 100)])], gpu=False))
    return out


REKEY_NAMES = tuple(rekey_fields())


# ---- field layout
def _every_pixel(H, W, seed):
    rng = np.random.default_rng(seed)
    hh, ww = np.mgrid[2:H - 2, 2:W - 2]
    n = hh.size
    off = rng.integers(-2, 3, (n, 2)) / 4.0
    q = rng.choice([100, 200, 300, 400, 500, 600, 700, 800], n)
    return Field([(int(a), int(b), float(o[0]), float(o[1]), int(c)) for a, b, o, c in zip(hh.ravel(), ww.ravel(), off, q)])


def _wild(H, W, seed, dens=0.08):
    """The existing test's "wild" kind: centres up to 3 px off their pixel on a 1/4 grid, few distinct R^2, some filtered."""
    rng = np.random.default_rng(seed)
    hh, ww = np.mgrid[2:H - 2, 2:W - 2]
    m = rng.random(hh.size) < dens
    h, w = hh.ravel()[m], ww.ravel()[m]
    off = rng.integers(-12, 13, (len(h), 2)) / 4.0
    q = rng.choice([100, 200, 300, 400, 500, 600, 700, 800, 2500], len(h))
    return Field([(int(a), int(b), float(o[0]), float(o[1]), int(c)) for a, b, o, c in zip(h, w, off, q)])


WILD_SEEDS = tuple(range(16))


def _layout_cases():
    out = []
    one = [Field([(2, 2, 0., 0., 100)]), Field([(2, 2, 0., 0., 2500)]), Field([(2, 2, 0.5, 0.5, 100)]), Field([(2, 2, -3.0, 0., 100)]),
           Field([(2, 2, 0., 3.0, 100)]), Field([])]
    out.append(Case("layout_5x5", 5, 5, 2, 0.5, one, layout=[5, 0, 1, 2, 5, 3, 4, 5]))
    out.append(Case("layout_5x64", 5, 64, 4, 0.5, [_every_pixel(5, 64, s) for s in (1, 2, 3)]))
    out.append(Case("layout_64x5", 64, 5, 4, 0.5, [_every_pixel(64, 5, s) for s in (4, 5, 6)]))
    out.append(Case("layout_every_pixel", 20, 20, 3, 0.5, [_every_pixel(20, 20, s) for s in (7, 8)]))
    out.append(Case("layout_every_pixel_r2", 12, 12, 2, 0.5, [_every_pixel(12, 12, s) for s in (9, 10, 11)]))
    F = rekey_fields()
    filtered = Field([(2, 2, 0., 0., 2500), (7, 7, 0.5, 0., 3000), (12, 12, 0., 0., 2000)])
    empty = Field([])
    out.append(Case("layout_one_field", 17, 17, 2, 0.5, [F["half_even_odd"]], default_form=True))
    out.append(Case("layout_one_field_filtered", 17, 17, 2, 0.5, [filtered], default_form=True))
    out.append(Case("layout_one_field_empty", 17, 17, 2, 0.5, [empty], default_form=True))
    out.append(Case("layout_empties", 17, 17, 2, 0.5, [empty, F["ordinary"], filtered, F["out_top"], F["swap"]],
                    layout=[0, 0, 1, 0, 2, 3, 0, 4, 2, 1, 0]))
    # many fields: the re-key fields and two dense ones in turn; 1 023 and 1 024 sit on the two sides of the library's switch
    many = [F[n] for n in REKEY_NAMES] + [_every_pixel(17, 17, 12), _every_pixel(17, 17, 13), empty, filtered]
    for n in (257, 1023, 1024):
        out.append(Case("layout_%d_fields" % n, 17, 17, 2, 0.5, many, layout=[(7 * k) % len(many) for k in range(n)], default_form=True))
    out.append(Case("wild_40x56", 40, 56, 4, 0.5, [_wild(40, 56, s) for s in WILD_SEEDS]))
    out.append(Case("wild_33x47_r2", 33, 47, 2, 0.5, [_wild(33, 47, 100 + s) for s in WILD_SEEDS]))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = _turn_cases() + _stop_cases() + _radius_cases() + _r2_cases() + _rekey_cases() + _layout_cases()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def by_name(name):
    return {c.name: c for c in cases()}[name]


# ------------------------------------------------------------------------------------------------ the fixture
class Fixture:
    """tests/golden/consolidate_limits.npz: per recorded case and distinct field the reference's h0, w0, r_2 (bit patterns) and, per
    rounding mode, the kept candidates in dict order with their keys, or that AssertionError was raised."""

    def __init__(self, path=FIXTURE):
        g = np.load(path)
        self.g = g
        self.names = [str(s) for s in g["names"]]
        self.f0 = np.concatenate([[0], np.cumsum(g["n_fields"])])
        self.c0 = np.concatenate([[0], np.cumsum(g["n_cand"])])
        self.k0 = {m: np.concatenate([[0], np.cumsum(np.maximum(g["nkeep_" + m], 0))]) for m in ("py2", "py3")}

    def field(self, name, u):
        """(h0 bits, w0 bits, r2 bits) of distinct field u of a case."""
        k = self.f0[self.names.index(name)] + u
        a = slice(self.c0[k], self.c0[k + 1])
        return self.g["h0_bits"][a], self.g["w0_bits"][a], self.g["r2_bits"][a]

    def expected(self, name, py2):
        """Per distinct field: (kept list, keys) or None - the shape of Case.expected()."""
        m = "py2" if py2 else "py3"
        c = self.names.index(name)
        out = []
        for k in range(self.f0[c], self.f0[c + 1]):
            if self.g["nkeep_" + m][k] < 0:
                out.append(None)
                continue
            a = slice(self.k0[m][k], self.k0[m][k + 1])
            out.append(([int(i) for i in self.g["kept_" + m][a]], [(int(p), int(q)) for p, q in self.g["keys_" + m][a]]))
        return out
