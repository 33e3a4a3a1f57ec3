"""Writes tests/golden/sequence_experiment.npz: seeded synthetic sequencing experiments run through the reference's own
MultifieldMultichannelSequenceExperiment (flexlibrary.py:1812-2231, 2384-3265), in the call order of
basic_experiment_script, with every intermediate result recorded.

Loads the reference at run time through oracle/refload.py (stepfitting_library before flexlibrary, so that _pairwise is the
real one).  The reference gets int64 copies of the frames (under NumPy 2 its Python sum() over uint16 scalars would wrap at
65 536); the golden keeps the uint16 originals ("wide": the same words and the factor the reference's int64 copy was scaled by).

  python tools/gen_sequence_golden.py [--reference DIR]
"""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNELS = ("ch1", "ch2")
MIN_DISTANCE = 7            # Chebyshev distance between truth positions: no two spots of one frame in one tracking bin
SPOT_SIZE = 5


def truth_positions(rng, n, H, W, edge_share):
    """n positions (frame-0 coordinates) at Chebyshev distance >= MIN_DISTANCE; a share of them is put close to a border."""
    pts = []
    tries = 0
    while len(pts) < n:
        tries += 1
        assert tries < 100000, "field too small for the requested number of spots"
        if rng.random() < edge_share:
            side = int(rng.integers(0, 4))
            d = int(rng.integers(2, 8))
            h = int(rng.integers(2, H - 2))
            w = int(rng.integers(2, W - 2))
            h, w = ((d, w), (H - 1 - d, w), (h, d), (h, W - 1 - d))[side]
        else:
            h, w = int(rng.integers(2, H - 2)), int(rng.integers(2, W - 2))
        if all(max(abs(h - p[0]), abs(w - p[1])) >= MIN_DISTANCE for p in pts):
            pts.append((h, w))
    return pts


def on_pattern(rng, F, k):
    """ON/OFF of one truth spot over the frames: fixed hole classes first, then Edman-like dropout with random misses."""
    fixed = [[1] * F,                                               # remainder
             [0] + [1] * (F - 1),                                   # leading hole
             [0, 0] + [1] * (F - 2),
             [1, 0] + [1] * (F - 2),                                # interior hole of length 1
             [1, 1, 0, 0, 0] + [1] * (F - 5),                       # interior hole of length > 1
             [1] * (F - 2) + [0, 0],                                # trailing hole
             [1, 0, 1, 0, 0, 1] + [0] * (F - 6),
             [0, 1, 0, 0] + [1] * (F - 5) + [0],
             [1] + [0] * (F - 1)]                                   # singleton
    if k < 3 * len(fixed):
        return list(fixed[k % len(fixed)])
    last = int(rng.integers(0, F + 2))
    first = 0 if rng.random() < 0.8 else int(rng.integers(1, 3))
    return [1 if first <= f <= last and rng.random() > 0.15 else 0 for f in range(F)]


def make_sequence(rng, F, H, W, n_spots):
    """-> (frames uint16 [F, H, W], offsets [(d_h, d_w)] * F, detected [(h, w)] per frame, truth positions)."""
    offsets = [(0, 0)] + [tuple(float(v) for v in np.round(rng.uniform(-1.6, 1.6, 2) * 20) / 20) for _ in range(F - 1)]
    cum = np.cumsum(np.array(offsets, dtype=np.float64), axis=0)
    pts = truth_positions(rng, n_spots, H, W, 0.45)
    # the three innermost positions take the remainder patterns (k = 0, 9, 18), so that all-ON traces survive the drift
    inner = sorted(range(n_spots), key=lambda i: -min(pts[i][0], H - 1 - pts[i][0], pts[i][1], W - 1 - pts[i][1]))[:3]
    for k, i in zip((0, 9, 18), inner):
        pts[k], pts[i] = pts[i], pts[k]
    frames = rng.normal(1000.0, 30.0, (F, H, W))
    r = (SPOT_SIZE - 1) // 2
    detected = [[] for _ in range(F)]
    hh, ww = np.mgrid[0:H, 0:W]
    for k, (h, w) in enumerate(pts):
        on = on_pattern(rng, F, k)
        amp = rng.uniform(1500.0, 6000.0)
        for f in range(F):
            ph, pw = h - cum[f, 0], w - cum[f, 1]          # (the sign greedy_particle_tracking links spots by)
            if on[f]:
                frames[f] += amp * np.exp(-((hh - ph) ** 2 + (ww - pw) ** 2) / (2 * 1.2 ** 2))
            ih = int(np.floor(ph + 0.5)) + (int(rng.integers(-1, 2)) if rng.random() < 0.3 else 0)
            iw = int(np.floor(pw + 0.5)) + (int(rng.integers(-1, 2)) if rng.random() < 0.3 else 0)
            if on[f] and r <= ih < H - r and r <= iw < W - r:
                detected[f].append((ih, iw))
    return np.clip(np.rint(frames), 0, 65535).astype(np.uint16), offsets, detected, pts


def hw_of(trace):
    return [(-1, -1) if s is None else (int(s.h), int(s.w)) for s in trace]


class Recorder(object):
    """Runs one experiment through the sequence classes of `fl` - the reference's flexlibrary here, the package's in the
    tests, which replay the same call sequence - and collects what the tests compare.

    sequences: per field, per channel (frames uint16 [F, H, W], offsets, detected [(h, w)] per frame, ...); pixels: what an
    Image gets for a frame; trace: stands in for trace_existing_spots where no tracker can run (called with the recorder)."""

    def __init__(self, fl, name, sequences, pixels, trace=None):
        self.fl, self.name, self.out, self.trace = fl, name, {}, trace
        self.stages = []
        self.n_fields = len(sequences)
        self.F = sequences[0][0][0].shape[0]
        fields = []
        for per_channel in sequences:
            chans = {}
            for c, (frames, offsets, detected, _) in zip(CHANNELS, per_channel):
                images = []
                for f in range(self.F):
                    im = fl.Image(image=pixels(frames[f]))
                    im.spots = [fl.Spot(im, h, w, SPOT_SIZE, gaussian_fit=None) for h, w in detected[f]]
                    images.append(im)
                ex = fl.SequenceExperiment(peptide_frames=images)
                ex.offsets = list(offsets)
                chans[c] = ex
            fields.append(fl.MultichannelSequenceExperiment(chans))
        self.mfmc = fl.MultifieldMultichannelSequenceExperiment(experimental_fields=fields)
        self.seqs = [(e, c, fields[e].channels[c]) for e in range(len(fields)) for c in fields[e].channels]

    def put(self, key, value):
        self.out[self.name + "_" + key] = value

    def stage(self, label):
        self.stages.append((label, [self.mfmc.spot_count()[c] for c in CHANNELS]))

    def text(self, key, s):
        self.put(key, np.frombuffer(s if isinstance(s, bytes) else s.encode(), dtype=np.uint8).copy())

    def traces(self, key, per_seq):
        hw, seq = [], []
        for s, traces in enumerate(per_seq):
            for t in traces:
                hw.append(hw_of(t))
                seq.append(s)
        self.put(key + "_hw", np.array(hw, dtype=np.int32).reshape(-1, self.F, 2))
        self.put(key + "_seq", np.array(seq, dtype=np.int32))

    def btcp(self, key, d):
        chan, field, cat, hw, ph = [], [], [], [], []
        for c, per_field in d.items():
            for e, cats in per_field.items():
                for category, rows in cats.items():
                    for row in rows:
                        chan.append(CHANNELS.index(c))
                        field.append(e)
                        cat.append(category)
                        hw.append([(-1, -1) if h is None else (int(h), int(w)) for h, w, _ in row])
                        ph.append([np.nan if h is None else float(v) for h, _, v in row])
        self.put(key + "_chan", np.array(chan, dtype=np.int32))
        self.put(key + "_field", np.array(field, dtype=np.int32))
        self.put(key + "_cat", np.array(cat, dtype=bool).reshape(-1, self.F))
        self.put(key + "_hw", np.array(hw, dtype=np.int32).reshape(-1, self.F, 2))
        self.put(key + "_phot", np.array(ph, dtype=np.float64).reshape(-1, self.F))

    def counts(self, key, d):
        chan, field, cat, n = [], [], [], []
        for c, per_field in d.items():
            for e, cats in per_field.items():
                for category, count in cats.items():
                    chan.append(CHANNELS.index(c))
                    field.append(e)
                    cat.append(category)
                    n.append(count)
        self.put(key + "_chan", np.array(chan, dtype=np.int32))
        self.put(key + "_field", np.array(field, dtype=np.int32))
        self.put(key + "_cat", np.array(cat, dtype=bool).reshape(-1, self.F))
        self.put(key + "_n", np.array(n, dtype=np.int64))

    def per_channel(self, key, d):
        self.put(key, np.array([d[c] for c in CHANNELS], dtype=np.int64))

    def csv(self, key, tmp, write):
        path = os.path.join(tmp, key + ".csv")
        ret = write(path)
        with open(path, "rb") as f:
            self.text(key, f.read())
        return ret

    def counters(self, tag):
        m = self.mfmc
        self.per_channel("trace_count_" + tag, m.trace_count())
        self.per_channel("singleton_count_" + tag, m.singleton_count())
        self.per_channel("discarded_" + tag, m.count_discarded_spots())
        self.put("remainders_" + tag, np.array([[r[c] for c in CHANNELS] for r in m.count_remainders()], dtype=np.int64))

    def run(self, small):
        fl, m = self.fl, self.mfmc
        mdma = fl.SequenceExperiment.mdma_adjustment
        self.stage("built")
        if self.trace is None:
            m.trace_existing_spots()
        else:
            self.trace(self)
        self.stage("traced")
        self.traces("traces", [ex.spot_traces for _, _, ex in self.seqs])
        self.counters("traced")
        self.traces("filled", [[ex.fill_in_trace(t) for t in ex.spot_traces] for _, _, ex in self.seqs])
        self.stage("filled")
        self.btcp("btcp_plain", m.binary_trace_categories_photometry(interpolate=False))
        self.stage("btcp_plain")
        self.btcp("btcp_interp", m.binary_trace_categories_photometry(interpolate=True))
        self.stage("btcp_interp")
        self.btcp("btcp_small_plain", m.binary_trace_categories_photometry(interpolate=False, **small))
        self.btcp("btcp_small_interp", m.binary_trace_categories_photometry(interpolate=True, **small))
        self.btcp("btcp_simple_interp", m.binary_trace_categories_photometry(method="simple", interpolate=True))
        self.stage("btcp_variants")
        with tempfile.TemporaryDirectory() as tmp:
            n = self.csv("csv_averages_all", tmp, lambda p: m.track_photometries_as_csv(p, save_averages=True))
            self.put("csv_averages_all_rows", np.int64(n))
            self.stage("csv_averages_all")
            # the split of the small hat setting, without keeping it
            kept = [ex.spot_traces for _, _, ex in self.seqs]
            self.traces("invalid_small", [ex.discard_invalid_traces(**small) for _, _, ex in self.seqs])
            self.traces("valid_small", [ex.spot_traces for _, _, ex in self.seqs])
            for (_, _, ex), k in zip(self.seqs, kept):
                ex.spot_traces = k
            self.stage("discard_small")
            invalid = m.discard_invalid_traces()
            self.traces("invalid", [invalid[e][c] for e, c, _ in self.seqs])
            self.traces("valid", [ex.spot_traces for _, _, ex in self.seqs])
            self.stage("discarded")
            self.counters("valid")
            counts, _ = m.count_binary_trace_categories()
            self.counts("counts", counts)
            self.counts("filtered_first", m.filtered_binary_trace_category_counts(include_first_frame_only=True))
            self.counts("filtered_nofirst", m.filtered_binary_trace_category_counts(include_first_frame_only=False))
            self.csv("csv_counts", tmp, lambda p: m.category_counts_as_csv(p, collate_fields=False))
            self.csv("csv_counts_collated", tmp, lambda p: m.category_counts_as_csv(p, collate_fields=True))
            self.text("counts_string", m.category_counts_as_string(collate_fields=False))
            self.text("counts_string_collated", m.category_counts_as_string(collate_fields=True))
            self.stage("counted")
            n = self.csv("csv_averages", tmp, lambda p: m.track_photometries_as_csv(p, save_averages=True))
            self.put("csv_averages_rows", np.int64(n))
            self.stage("csv_averages")
            n = self.csv("csv_frames", tmp, lambda p: m.track_photometries_as_csv(p, save_averages=False))
            self.put("csv_frames_rows", np.int64(n))
            self.stage("csv_frames")
            adj = m.multiplicative_delta_median_adjustments()
            self.put("mdma", np.array([[a[c] for c in CHANNELS] for a in adj], dtype=np.float64))
            self.stage("mdma")
            self.csv("csv_frames_mdma", tmp,
                     lambda p: m.track_photometries_as_csv(p, save_averages=False, adjustment_function=mdma))
            self.stage("csv_frames_mdma")
        self.text("offsets_string", m.offsets_as_string())
        self.put("stage_labels", np.array([s[0] for s in self.stages]))
        self.put("stage_spot_counts", np.array([s[1] for s in self.stages], dtype=np.int64))
        return self.out


def hole_classes(hw):
    """Occurrences of every case class among the traces (hw int [N, F, 2])."""
    det = hw[:, :, 0] >= 0
    n = dict(leading=0, interior1=0, interior_long=0, trailing=0, all_on=0, first_off=0, singleton=0)
    for row in det:
        F = len(row)
        on = np.flatnonzero(row)
        n["all_on"] += int(row.all())
        n["first_off"] += int(not row[0])
        n["singleton"] += int(len(on) == 1)
        n["leading"] += int(on[0] > 0)
        n["trailing"] += int(on[-1] < F - 1)
        gaps = np.diff(on) - 1
        n["interior1"] += int((gaps == 1).sum())
        n["interior_long"] += int((gaps > 1).sum())
    return n


def check_conditions(name, out, H, W, radius):
    """The conditions on the inputs (not measurements): every case class occurs at least 3 times."""
    hw, filled = out[name + "_traces_hw"], out[name + "_filled_hw"]
    n = hole_classes(hw)
    n["outside"] = int(((hw[:, :, 0] < 0) & (filled[:, :, 0] < 0)).sum())
    have = filled[:, :, 0] >= 0
    n["clip_top"] = int((have & (filled[:, :, 0] - radius < 0)).sum())
    n["clip_bottom"] = int((have & (filled[:, :, 0] + radius >= H)).sum())
    n["clip_left"] = int((have & (filled[:, :, 1] - radius < 0)).sum())
    n["clip_right"] = int((have & (filled[:, :, 1] + radius >= W)).sum())
    n["mdma_nonzero"] = int((out[name + "_mdma"] != 0).sum())
    print(name, len(hw), "traces", n, flush=True)
    for k, v in n.items():
        assert v >= 3, (name, k, v)
    assert 2 * n["singleton"] <= len(hw), (name, "more than half of the traces are singletons")


# ---- tests/golden/sequence_limits.npz: Spot.mexican_hat_photometry_metric around the 16-register window ---------------------
HAT_SIDE = 44                                # an unclipped radius-15 window (31 x 31) fits around (22, 22)
HAT_RADII = (12, 13, 14, 15, 16, 17)
HAT_FIELDS = ("random", "tied", "constant", "two_valued", "top")
HAT_POSITIONS = ((22, 22), (21, 23), (15, 15), (16, 28), (0, 22), (43, 22), (22, 0), (22, 43), (0, 0), (0, 43), (43, 0), (43, 43))


def hat_brims(radius):
    """0, a middle width, a crown of one pixel, no crown."""
    return (0, 6, radius, radius + 1)


def hat_frame(field, wide, radius):
    """One 44 x 44 frame (uint16, or uint32 with wide): random; heavily tied; constant; two values split so that the ring
    around (22, 22) holds as many low as high pixels (its median ends in .5); every pixel at the top of the uint32 range."""
    rng = np.random.default_rng(5000 + 100 * HAT_FIELDS.index(field) + 10 * int(wide) + radius)
    top = 2 ** 31 if wide else 65536
    if field == "random":
        fr = rng.integers(0, top, (HAT_SIDE, HAT_SIDE), dtype=np.int64)
    elif field == "tied":
        fr = rng.integers(0, top, (HAT_SIDE, HAT_SIDE), dtype=np.int64) // (top // 16)
    elif field == "constant":
        fr = np.full((HAT_SIDE, HAT_SIDE), int(rng.integers(1, top)), dtype=np.int64)
    elif field == "two_valued":
        lo = int(rng.integers(0, top // 2))
        hi = lo + 1 + 2 * int(rng.integers(0, top // 4))
        i = np.arange(HAT_SIDE * HAT_SIDE).reshape(HAT_SIDE, HAT_SIDE)
        fr = np.where(i < 22 * HAT_SIDE + 22, lo, hi).astype(np.int64)
    else:
        fr = np.full((HAT_SIDE, HAT_SIDE), top - 1, dtype=np.int64)
        fr[rng.random((HAT_SIDE, HAT_SIDE)) < 0.3] -= 1
    return fr.astype(np.uint32 if wide else np.uint16)


def gen_limits(fl, out_path):
    """phot [wide][radius][field][brim][position] float64: the reference's own hat on an int64 copy of every frame."""
    phot = np.zeros((2, len(HAT_RADII), len(HAT_FIELDS), 4, len(HAT_POSITIONS)))
    crc = np.zeros((2, len(HAT_RADII), len(HAT_FIELDS)), np.int64)
    import zlib
    for wide in (0, 1):
        for ri, radius in enumerate(HAT_RADII):
            for fi, field in enumerate(HAT_FIELDS):
                fr = hat_frame(field, bool(wide), radius)
                crc[wide, ri, fi] = zlib.crc32(fr.tobytes())
                im = fl.Image(image=fr.astype(np.int64))
                for bi, brim in enumerate(hat_brims(radius)):
                    for pi, (h, w) in enumerate(HAT_POSITIONS):
                        spot = fl.Spot(im, h, w, 1, gaussian_fit=None)      # (size 1 fits on every border)
                        phot[wide, ri, fi, bi, pi] = float(spot.mexican_hat_photometry_metric(brim_size=brim, radius=radius))
                if field == "two_valued":                           # the ring of width 6 around (22, 22): median ends in .5
                    v = phot[wide, ri, fi, 1, 0]
                    n_crown = (2 * radius + 1 - 12) ** 2
                    assert n_crown % 2 == 1 and v != np.floor(v), (wide, radius, v)
    np.savez_compressed(out_path, phot=phot, frame_crc=crc, radii=np.array(HAT_RADII), positions=np.array(HAT_POSITIONS),
                        fields=np.array(HAT_FIELDS), side=np.int64(HAT_SIDE))
    print(out_path, os.path.getsize(out_path), "bytes;", int(np.isnan(phot).sum()), "NaN of", phot.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("FSQ_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "sequence_experiment.npz"))
    ap.add_argument("--limits", action="store_true",
                    help="write only tests/golden/sequence_limits.npz (the hat at radii 12 - 17); the other fixture stays")
    a = ap.parse_args()
    os.environ["FSQ_REFERENCE"] = a.reference
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import refload
    refload.REF = a.reference
    ref = refload.load_reference()
    refload.load("stepfitting_library", "stepfitting_library.py")
    fl = refload.load_flexlibrary(ref).fl
    if a.limits:
        return gen_limits(fl, os.path.join(os.path.dirname(a.out), "sequence_limits.npz"))

    out = {"channels": np.array(CHANNELS), "spot_size": np.int64(SPOT_SIZE)}
    # (name, seed, fields, frames, H, W, spots per sequence, pixel scale, small hat setting)
    for name, seed, n_fields, F, H, W, n_spots, scale, small in (("main", 11, 2, 7, 96, 128, 40, 1, dict(radius=4, brim_size=2)),
                                                                  ("wide", 12, 1, 8, 64, 80, 30, 300, dict(radius=3, brim_size=1))):
        rng = np.random.default_rng(seed)
        sequences = [[make_sequence(rng, F, H, W, n_spots) for _ in CHANNELS] for _ in range(n_fields)]
        for per_channel in sequences:
            for _, _, _, pts in per_channel:
                d = np.abs(np.array(pts)[:, None, :] - np.array(pts)[None, :, :]).max(axis=2)
                assert (d + MIN_DISTANCE * np.eye(len(pts)) >= MIN_DISTANCE).all()
        rec = Recorder(fl, name, sequences, lambda a, scale=scale: a.astype(np.int64) * scale).run(small)
        flat = [s for per_channel in sequences for s in per_channel]
        rec[name + "_frames"] = np.stack([s[0] for s in flat])
        rec[name + "_offsets"] = np.array([s[1] for s in flat], dtype=np.float64)
        det = [(i, f, h, w) for i, s in enumerate(flat) for f in range(F) for h, w in s[2][f]]
        rec[name + "_detected"] = np.array(det, dtype=np.int32)                 # (sequence, frame, h, w) in Image.spots order
        rec[name + "_scale"] = np.int64(scale)
        rec[name + "_small"] = np.array([small["radius"], small["brim_size"]], dtype=np.int64)
        rec[name + "_n_fields"] = np.int64(n_fields)
        check_conditions(name, rec, H, W, 9)
        out.update(rec)
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
