"""Writes tests/golden/experiment_end_to_end.npz: a seeded synthetic sequencing experiment taken from its image files to the
two CSV files and the printed summary by the reference's own code, in the order of its basic_experiment_script.py
(:376-644), with what the records route has to reproduce recorded on the way.

The reference is loaded at run time through oracle/refload.py (numpy's AVX-512 paths disabled, as oracle/gen_golden.py does).
Its chain: pflib.find_peptides per frame -> save_psfs_pkl next to a PNG of the frame -> Experiment.easy_sort_target_images ->
easy_load_processed_image -> SequenceExperiment(peptide_frames, alignment_frames).offsets_from_frames() ->
MultichannelSequenceExperiment -> MultifieldMultichannelSequenceExperiment -> trace_existing_spots -> discard_invalid_traces ->
count_binary_trace_categories / filtered_binary_trace_category_counts -> category_counts_as_csv -> track_photometries_as_csv ->
the summary lines.  The frames (2 fields x 2 channels x 5 cycles of 64 x 80 uint16) come from the package's synthetic renderer
(tests/_experiment_cases.py:experiment_frames).  The loaded Images get int64 copies of their pixels (under NumPy 2 the
reference's sums over uint16 scalars would wrap at 65 536).

Recorded per run ("two": both channels, "one": the first channel alone, "alt": both channels with --keep_invalid
--not_all_photometries --collate_fields): the Spot tables and discard counts per frame, the offsets, the traces, the dropout
counts, the two stats dicts, the CSV texts, the summary text from "Total spots found" on; once: the frames, the key and fitted
centre of every PSF, and a crafted PSF dict that takes Spot.__init__ through all four outcomes of its two centre tests.

Conditions on the inputs, asserted on the reference's output (another seed is drawn otherwise): no field ends with the re-key
assertion; Spots are kept whose window leaves the image (keys on row H - 2 / column W - 2); spots drift out of a frame
(discard_dropouts); leading, interior and trailing holes; an invalid and an all-ON trace in every channel; for every registered
pair the two largest values of the upsampled correlation differ by more than 1e-9 relative, by magnitude and in numpy's
ordering of complex numbers (the one argmax uses).  A refusal by Spot.__init__ cannot come from pflib's own fits - the fitted
centre is confined to half a pixel around a candidate that lies two pixels inside the image (pflib.py:207-212), so a centre
outside [2, H - 2) never comes with a key whose window leaves the image - which is why the crafted dict is there.

  python tools/gen_experiment_golden.py [--reference DIR] [--seed N]
"""
import argparse
import contextlib
import io
import os
import subprocess
import sys
import tempfile

NPY_ENV = "AVX512F AVX512CD AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR"
if __name__ == "__main__" and os.environ.get("NPY_DISABLE_CPU_FEATURES") != NPY_ENV:
    os.environ["NPY_DISABLE_CPU_FEATURES"] = NPY_ENV
    sys.exit(subprocess.call([sys.executable] + sys.argv))         # a fresh child: numpy reads the variable at import

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gen_sequence_golden import CHANNELS, Recorder, hole_classes  # noqa: E402

EPOCH = 1450000000.4
RUNS = {"two": dict(channels=(0, 1)), "one": dict(channels=(0,)),
        "alt": dict(channels=(0, 1), keep_invalid=True, save_averages=True, collate_fields=True)}


class Unsuitable(Exception):
    """The seed's frames miss one of the conditions."""


def write_tree(frames, root):
    """PNG files <root>/ch<c>/cycle_<f>/field_<e>.png -> paths[c] (the file list of one channel, any order)."""
    from PIL import Image as PILImage
    n_fields, C, F = frames.shape[:3]
    paths = []
    for c in range(C):
        files = []
        for f in range(F):
            d = os.path.join(root, "ch%d" % (c + 1), "cycle_%d" % f)
            os.makedirs(d, exist_ok=True)
            for e in range(n_fields):
                p = os.path.join(d, "field_%d.png" % e)
                PILImage.fromarray(frames[e, c, f]).save(p)
                files.append(p)
        paths.append(files)
    return paths


class Chain(Recorder):
    """basic_experiment_script.py:376-644 on the classes of `fl`, recorded with gen_sequence_golden.Recorder's own writers."""

    def __init__(self, fl, name, channel_files, F, keep_invalid=False, save_averages=False, collate_fields=False):
        self.fl, self.name, self.out, self.F = fl, name, {}, F
        self.keep_invalid, self.save_averages, self.collate_fields = keep_invalid, save_averages, collate_fields
        E = fl.Experiment
        _, field_indexed_peptide = E.easy_sort_target_images(channel_files[0])
        _, field_indexed_alignment = E.easy_sort_target_images(channel_files[0])         # (self-alignment, :275-276)
        _, field_indexed_second = E.easy_sort_target_images(channel_files[1] if len(channel_files) > 1 else [])
        self.discarded = []

        def load(field_indexed, load_psfs=True):
            fields = {}
            for field, files in field_indexed.items():
                fields.setdefault(field, [])
                for f in files:
                    image_object, discarded_spots = E.easy_load_processed_image(f, load_psfs=load_psfs)
                    image_object.image = image_object.image.astype(np.int64)
                    if load_psfs:
                        self.discarded.append((field, f, discarded_spots))
                    fields[field].append(image_object)
            return fields
        peptide_fields, alignment_fields = load(field_indexed_peptide), load(field_indexed_alignment, load_psfs=False)
        second_channel_fields = load(field_indexed_second)
        combined = []
        for field, frames in peptide_fields.items():
            ex = fl.SequenceExperiment(peptide_frames=frames, alignment_frames=alignment_fields[field])
            ex.offsets_from_frames()
            if len(second_channel_fields) == 0:
                combined_channel_dict = {'ch1': ex}
            else:
                ex2 = fl.SequenceExperiment(peptide_frames=second_channel_fields[field], alignment_frames=alignment_fields[field])
                ex2.offsets_from_frames()
                combined_channel_dict = {'ch1': ex, 'ch2': ex2}
            combined.append(fl.MultichannelSequenceExperiment(combined_channel_dict))
        self.mfmc = fl.MultifieldMultichannelSequenceExperiment(experimental_fields=combined)
        self.seqs = [(e, c, combined[e].channels[c]) for e in range(len(combined)) for c in combined[e].channels]

    def run(self):
        m = self.mfmc
        tables = [[(int(s.h), int(s.w)) for s in im.spots] for _, _, ex in self.seqs for im in ex.peptide_frames]
        self.put("spot_counts", np.array([len(t) for t in tables], np.int32).reshape(len(self.seqs), self.F))
        self.put("spot_hw", np.array([p for t in tables for p in t], np.int32).reshape(-1, 2))
        by_file = {f: n for _, f, n in self.discarded}
        self.put("spots_discarded", np.array([by_file[im.metadata['filepath']] for _, _, ex in self.seqs for im in ex.peptide_frames],
                                             np.int32).reshape(len(self.seqs), self.F))
        self.put("offsets", np.array([[(float(a), float(b)) for a, b in ex.offsets] for _, _, ex in self.seqs], np.float64))
        m.trace_existing_spots()
        self.traces("traces", [ex.spot_traces for _, _, ex in self.seqs])
        self.put("n_dropouts", np.array([ex.num_discarded_spots for _, _, ex in self.seqs], np.int32))
        if not self.keep_invalid:
            invalid = m.discard_invalid_traces()
            self.traces("invalid", [invalid[e][c] for e, c, _ in self.seqs])
            self.traces("valid", [ex.spot_traces for _, _, ex in self.seqs])
        category_stats, _ = m.count_binary_trace_categories()
        self.counts("category_stats", category_stats)
        self.counts("filtered_stats", m.filtered_binary_trace_category_counts(include_first_frame_only=True))
        with tempfile.TemporaryDirectory() as tmp:
            self.csv("csv_counts", tmp, lambda p: m.category_counts_as_csv(p, collate_fields=self.collate_fields))
            n = self.csv("csv_photometries", tmp, lambda p: m.track_photometries_as_csv(filepath=p, save_averages=self.save_averages,
                                                                                          discard_invalid=False))
            self.put("csv_photometries_rows", np.int64(n))
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            print("Total spots found in all peptide frames: " + str(m.spot_count()))
            print("Number of spots discarded due to stage drift: " + str(m.count_discarded_spots()))
            print("Total number of traced spots: " + str(m.trace_count()))
            print("Singleton count: " + str(m.singleton_count()))
            print("Basic track breakdown:")
            print(m.category_counts_as_string(filtered=True, collate_fields=self.collate_fields))
        self.text("summary", buf.getvalue())
        self.put("flags", np.array([self.keep_invalid, self.save_averages, self.collate_fields]))
        return self.out


def crafted_psfs(H, W):
    """A PSF dict whose keys all leave the image while the fitted centres take the two range tests of Spot.__init__ through all
    four outcomes (and the bounds of the ranges themselves)."""
    sub, fit = np.zeros((5, 5), np.int64), np.zeros((5, 5))
    mk = lambda h0, w0: (np.float64(h0), np.float64(w0), np.float64(100.), np.float64(500.), np.float64(1.), np.float64(1.),  # noqa: E731
                         np.float64(0.), sub, fit, 1.0, np.float64(0.9), np.float64(5.))
    psfs = {}
    centres = [(0.4, 40.2), (2.2, 30.1), (40.3, 200.0), (-3.0, -1.0), (2.0, 2.0), (1.9999999999999998, W - 2.0), (H - 2.0, 77.9),
               (np.nextafter(H - 2.0, 0), 5.0), (30.0, np.nextafter(W - 2.0, 0)), (70.0, 1.0), (1.0, 1.0), (float("nan"), 9.0)]
    keys = [(0, 40), (1, 30), (40, W - 1), (-1, -2), (1, 1), (0, W - 2), (H - 1, 60), (H - 2, 5), (30, W - 2), (H, 1), (1, 0), (H - 1, 9)]
    for key, (h0, w0) in zip(keys, centres):
        psfs[(float(key[0]), float(key[1]))] = mk(h0, w0)
    psfs[(20.0, 20.0)] = mk(20.2, 19.9)                                 # (and one whose window lies inside)
    return psfs


def generate(ref, fl, seed):
    import _experiment_cases as C
    from PIL import Image as PILImage
    frames = C.experiment_frames(seed)
    n_fields, n_ch, F, H, W = frames.shape
    out = {"frames": frames, "seed": np.int64(seed), "channels": np.array(CHANNELS)}
    tops = []
    dftups = ref.pc._dftups

    def spy(data, upsampled_rows=None, upsampled_cols=None, upsample_factor=1, row_offset=0, col_offset=0):
        res = dftups(data, upsampled_rows, upsampled_cols, upsample_factor, row_offset, col_offset)
        if res.size > 1:
            tops.append(res.copy())
        return res
    with tempfile.TemporaryDirectory() as root:
        paths = write_tree(frames, root)
        keys, centres, counts = [], [], []
        for e in range(n_fields):
            for c in range(n_ch):
                for f in range(F):
                    try:
                        psfs = ref.pf.find_peptides(frames[e, c, f])
                    except AssertionError:
                        raise Unsuitable("re-key assertion in field %d channel %d frame %d" % (e, c, f))
                    ref.pf.save_psfs_pkl(psfs, image_path=os.path.join(root, "ch%d" % (c + 1), "cycle_%d" % f, "field_%d.png" % e),
                                         timestamp_epoch=EPOCH)
                    keys += [(int(h), int(w)) for h, w in psfs]
                    centres += [(float(v[0]), float(v[1])) for v in psfs.values()]
                    counts.append(len(psfs))
        out["psf_key"], out["psf_centre"] = np.array(keys, np.int32).reshape(-1, 2), np.array(centres, np.float64).reshape(-1, 2)
        out["psf_counts"] = np.array(counts, np.int32).reshape(n_fields * n_ch, F)
        ref.pc._dftups = spy
        try:
            for name, kw in RUNS.items():
                kw = dict(kw)
                chans = kw.pop("channels")
                out.update(Chain(fl, name, [paths[c] for c in chans], F, **kw).run())
        finally:
            ref.pc._dftups = dftups
        # the crafted dict through the reference's own loader
        png = os.path.join(root, "crafted.png")
        PILImage.fromarray(frames[0, 0, 0]).save(png)
        psfs = crafted_psfs(H, W)
        ref.pf.save_psfs_pkl(psfs, image_path=png, timestamp_epoch=EPOCH)
        im, discarded = fl.Experiment.easy_load_processed_image(png)
        out["crafted_key"] = np.array([(int(h), int(w)) for h, w in psfs], np.int32)
        out["crafted_centre"] = np.array([(float(v[0]), float(v[1])) for v in psfs.values()], np.float64)
        out["crafted_spot_hw"] = np.array([(int(s.h), int(s.w)) for s in im.spots], np.int32).reshape(-1, 2)
        out["crafted_discarded"] = np.int64(discarded)
    check_conditions(out, tops, H, W)
    return out


def check_conditions(out, tops, H, W):
    hw = out["two_spot_hw"]
    if not ((hw[:, 0] == H - 2) | (hw[:, 1] == W - 2)).any():
        raise Unsuitable("no kept Spot whose window leaves the image")
    if int(out["two_n_dropouts"].sum()) == 0:
        raise Unsuitable("no spot drifts out of a frame")
    n = hole_classes(out["two_traces_hw"])
    if not (n["leading"] and n["trailing"] and n["interior1"] + n["interior_long"]):
        raise Unsuitable("hole classes %r" % (n,))
    n_ch = len(CHANNELS)
    for c in range(n_ch):
        if not (out["two_invalid_seq"] % n_ch == c).any():
            raise Unsuitable("no invalid trace in channel %d" % c)
        on = (out["two_traces_hw"][:, :, 0] >= 0).all(axis=1) & (out["two_traces_seq"] % n_ch == c)
        if not on.any():
            raise Unsuitable("no all-ON trace in channel %d" % c)
    assert len(tops) > 0
    for k, cc in enumerate(tops):
        for values in (np.sort(np.abs(cc).ravel()), np.sort_complex(cc.ravel()).real):
            if not (values[-1] - values[-2]) > 1e-9 * abs(values[-1]):
                raise Unsuitable("registration %d: the two largest correlation values are closer than 1e-9 relative" % k)
    # the crafted dict reaches every outcome
    r = 2
    key, centre = out["crafted_key"], out["crafted_centre"]
    leaves = ~((r <= key[:, 0]) & (key[:, 0] < H - r) & (r <= key[:, 1]) & (key[:, 1] < W - r))
    in_h, in_w = (r <= centre[:, 0]) & (centre[:, 0] < H - r), (r <= centre[:, 1]) & (centre[:, 1] < W - r)
    for a in (False, True):
        for b in (False, True):
            assert (leaves & (in_h == a) & (in_w == b)).any(), (a, b)
    assert 0 < int(out["crafted_discarded"]) < len(key)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("FSQ_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "experiment_end_to_end.npz"))
    ap.add_argument("--seed", type=int, default=1, help="the first seed tried")
    a = ap.parse_args()
    os.environ["FSQ_REFERENCE"] = a.reference
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import refload
    from PIL import Image as PILImage
    refload.REF = a.reference
    ref = refload.load_reference()
    refload.load("stepfitting_library", "stepfitting_library.py")          # (before flexlibrary, so that _pairwise is the real one)
    fl = refload.load_flexlibrary(ref).fl
    fl.imread = lambda p: np.array(PILImage.open(p))
    seed = a.seed
    while True:
        try:
            out = generate(ref, fl, seed)
            break
        except Unsuitable as e:
            print("seed", seed, "rejected:", e, flush=True)
            seed += 1
            assert seed < a.seed + 200
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes; seed", seed, "; traces", len(out["two_traces_hw"]), "; classes",
          hole_classes(out["two_traces_hw"]))


if __name__ == "__main__":
    main()
