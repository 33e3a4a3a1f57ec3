"""Drop-in for the tracking entry points of the reference's `flexlibrary.Experiment`, computed on
the GPU from the peak tables:

    Experiment.accumulate_offsets        flexlibrary.py:567-593
    Experiment.discard_dropouts          flexlibrary.py:626-678
    Experiment.greedy_particle_tracking  flexlibrary.py:680-1027

Same names, arguments, return shapes and exceptions; `track_fields` is the batch form (many fields per launch) that
works directly on `(h, w)` tables such as the dict keys pflib.find_peptides returns.  The arithmetic is in
csrc/fsq_track.hip (fsq_greedy_tracking of include/fsq.h); there is no CPU fallback.

The sequence classes (SequenceExperiment, MultichannelSequenceExperiment, MultifieldMultichannelSequenceExperiment:
flexlibrary.py:1680-2231, 2471-3263) reduce the tracks to ON/OFF patterns and photometries and write the two CSV files of
basic_experiment_script; all their traces go through one fsq_sequence_photometry launch (sequencing.py,
include/fsq_sequence.h)."""
import ctypes

import numpy as np

from . import _native as N
from . import engine as _engine
from .pflib import _py2_round


def track_fields(fields, offsets, frame_shape, candidate_radius=2, spot_radius=0, device=None):
    """Track the spots of many independent fields in one launch.

    fields:  list (per field) of lists (per frame) of integer arrays [n, 2] = (Spot.h, Spot.w); every field has the same
             number of frames.
    offsets: list (per field) of lists (per frame) of (d_h, d_w) relative to the previous frame, offsets[k][0] == (0, 0).
    Returns a list (per field) of (traces int32[n_traces, n_frames], n_discarded, prev int32[n], next int32[n],
    kept bool[n]): spot numbers count through the field's frames in order, -1 = no spot.  Raises ValueError /
    AssertionError where the reference does (first offset not (0, 0); two spots of one frame in one bin)."""
    torch = _engine._torch()
    dev = torch.device(device or ("cuda:%d" % torch.cuda.current_device()))
    if int(candidate_radius) != candidate_radius:
        raise TypeError("slice indices must be integers")          # the reference slices with candidate_radius (:905)
    n_fields = len(fields)
    if n_fields == 0:
        return []
    F = len(fields[0])
    H, W = int(frame_shape[0]), int(frame_shape[1])
    counts = np.zeros((n_fields, F), np.int32)
    parts = []
    for k, frames in enumerate(fields):
        if len(frames) != F or len(offsets[k]) != F:
            raise ValueError("every field needs the same number of frames and one offset per frame")
        for f, hw in enumerate(frames):
            a = np.asarray(hw)
            if a.size and not np.array_equal(a, np.rint(a)):
                raise NotImplementedError("Spot.h / Spot.w must be whole numbers (flexlibrary.py:449 makes them so)")
            a = a.astype(np.int32).reshape(-1, 2)
            counts[k, f] = len(a)
            parts.append(a)
    hw = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0, 2), np.int32))
    start = np.concatenate([[0], np.cumsum(counts.sum(axis=1))]).astype(np.int32)
    total = int(start[-1])
    # (no limit on frames or spots since round 4: long time series keep their frame tables in the workspace, large fields read the
    # "has been paired" facts off the links instead of LDS bitmaps; the reference has no limit either)
    off = np.ascontiguousarray(np.array([[(float(o[0]), float(o[1])) for o in offs] for offs in offsets], dtype=np.float64))
    for k in range(n_fields):
        if off[k, 0, 0] != 0 or off[k, 0, 1] != 0:
            raise ValueError("The first image's offset must be (0, 0) by definiton.")           # flexlibrary.py:581-583
    L = N.lib()
    pair_cap = max(4096, 8 * int(counts.max()) if counts.size else 4096)
    while True:         # candidate pairs per frame are bounded only by the data: on overflow the list is doubled and the call repeated
        res = _track_launch(torch, dev, L, hw, start, counts, off, n_fields, F, H, W, candidate_radius, spot_radius, pair_cap, total)
        if not (res[0] == N.FSQ_ERANGE).any() or pair_cap >= (1 << 28):
            break
        pair_cap *= 4
    st, nt, nd, prev, nxt, kept, traces = res
    out = []
    for k in range(n_fields):
        if st[k] == N.FSQ_EASSERT:
            raise AssertionError("field %d: two spots of one frame round to the same bin of frame_bins "
                                 "(flexlibrary.py:851)" % k)
        N.check(int(st[k]), "fsq_greedy_tracking (field %d)" % k)
        a, b = int(start[k]), int(start[k + 1])
        out.append((traces[a:a + int(nt[k])].copy(), int(nd[k]), prev[a:b].copy(), nxt[a:b].copy(), kept[a:b].copy()))
    return out




def _track_launch(torch, dev, L, hw, start, counts, off, n_fields, F, H, W, candidate_radius, spot_radius, pair_cap, total):
    ws_bytes = L.fsq_track_workspace_bytes(n_fields, F, H, W, pair_cap)
    if ws_bytes < 0:
        raise ValueError("invalid tracking shape")
    t = lambda a: torch.from_numpy(a).to(dev)          # noqa: E731
    d_hw, d_start, d_counts, d_off = t(hw.reshape(-1)), t(start), t(counts.reshape(-1)), t(off.reshape(-1))
    d_prev = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    d_next = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    d_kept = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    d_traces = torch.empty(max(total, 1) * F, dtype=torch.int32, device=dev)
    d_nt = torch.empty(n_fields, dtype=torch.int32, device=dev)
    d_nd = torch.empty(n_fields, dtype=torch.int32, device=dev)
    d_st = torch.empty(n_fields, dtype=torch.int32, device=dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    rc = L.fsq_greedy_tracking(d_hw.data_ptr(), d_start.data_ptr(), d_counts.data_ptr(), d_off.data_ptr(), n_fields, F, H, W,
                               int(candidate_radius), float(spot_radius), d_prev.data_ptr(), d_next.data_ptr(),
                               d_kept.data_ptr(), d_traces.data_ptr(), d_nt.data_ptr(), d_nd.data_ptr(), d_st.data_ptr(),
                               pair_cap, ws.data_ptr(), ws_bytes, torch.cuda.current_stream(dev).cuda_stream)
    N.check(rc, "fsq_greedy_tracking")
    return (d_st.cpu().numpy(), d_nt.cpu().numpy(), d_nd.cpu().numpy(), d_prev.cpu().numpy(), d_next.cpu().numpy(),
            d_kept.cpu().numpy().astype(bool), d_traces.cpu().numpy().reshape(-1, F))


def centroid_track_fields(frames, init_hw, spot_field=None, search_radius=3, s_n_cutoff=3.0, offsets=None, device=None):
    """Luminosity-centroid tracking of many spots in many fields in one launch (fsq_centroid_tracking).

    frames integer[n_fields, F, H, W] (or [F, H, W] for one field; values below 2^31, beyond 65 535: fsq_centroid_tracking_u32); init_hw int[n, 2]; spot_field int[n] (default: all in
    field 0); offsets whole-pixel (d_h, d_w)[n_fields, F, 2] or None.  -> (hw int32[n, F, 2], present bool[n, F]);
    raises ValueError where the reference does (a search window that sums to zero)."""
    torch = _engine._torch()
    dev = torch.device(device or ("cuda:%d" % torch.cuda.current_device()))
    fr, fmt = _engine.as_integer_fields(frames)
    if fr.ndim == 3:
        fr = fr[None]
    if fr.ndim != 4:
        raise ValueError("frames must have shape (n_fields, F, H, W)")
    n_fields, F, H, W = fr.shape
    hw = np.ascontiguousarray(np.asarray(init_hw, dtype=np.int32).reshape(-1, 2))
    n = len(hw)
    sf = np.zeros(n, np.int32) if spot_field is None else np.ascontiguousarray(spot_field, dtype=np.int32)
    if len(sf) != n or (n and (sf.min() < 0 or sf.max() >= n_fields)):
        raise ValueError("spot_field must name a field for every spot")
    d_off = None
    if offsets is not None:
        off = np.asarray(offsets)
        if not np.array_equal(off, np.rint(off)):
            raise TypeError("slice indices must be integers")       # what the reference's image slicing raises (:1223)
        d_off = torch.from_numpy(np.ascontiguousarray(off.astype(np.int64).reshape(n_fields, F, 2))).to(dev)
    d_fr = _engine.to_device_pixels(fr, fmt, dev)
    d_hw, d_sf = torch.from_numpy(hw).to(dev), torch.from_numpy(sf).to(dev)
    d_out = torch.empty((max(n, 1), F, 2), dtype=torch.int32, device=dev)
    d_pres = torch.empty((max(n, 1), F), dtype=torch.uint8, device=dev)
    d_err = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = (N.lib().fsq_centroid_tracking_u32 if fmt == N.PIXELS_U32 else N.lib().fsq_centroid_tracking)(d_fr.data_ptr(), n_fields, F, H, W, d_hw.data_ptr(), d_sf.data_ptr(), n, int(search_radius),
                                       float(s_n_cutoff), d_off.data_ptr() if d_off is not None else None, d_out.data_ptr(),
                                       d_pres.data_ptr(), d_err.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    N.check(rc, "fsq_centroid_tracking")
    if int(d_err.item()):
        raise ValueError("cannot convert float NaN to integer")     # int(round(nan)) of an all-zero window's centroid
    return d_out[:n].cpu().numpy(), d_pres[:n].cpu().numpy().astype(bool)


class Spot(object):
    """A square of pixels in an image: the reference's Spot as far as tracking needs it (flexlibrary.py:74-112):
    `parent_Image` (anything with an `.image` array), integer centre (h, w), odd size, optional gaussian_fit tuple."""

    def __init__(self, parent_Image, h, w, size, gaussian_fit=None):
        self.parent_Image = parent_Image
        if size % 2 == 0:
            raise AttributeError("Spot.size must be odd.")
        self.size = size
        r, shape = (size - 1) // 2, parent_Image.image.shape
        if not (0 <= h - r and h + r < shape[0] and 0 <= w - r and w + r < shape[1]):
            if (gaussian_fit is None or not (r <= gaussian_fit[0] < shape[0] - r) and (r <= gaussian_fit[1] < shape[1] - r)):
                raise AttributeError("Spot area of size " + str(size) + " at " + str((h, w)) + " with gaussian_fit " +
                                     str(gaussian_fit) + " does not fit into parent_Image.image.shape of " + str(shape))
        self.h, self.w = h, w
        self.gaussian_fit = gaussian_fit

    def image_slice(self, radius=None):
        """The Spot's square of pixels as numpy slices it: clipped at the borders, except that a centre more than `radius`
        beyond row or column 0 gives a negative stop, which numpy counts from the far end (a wrapped window, as in the
        reference).  flexlibrary.py:113-146."""
        if radius is None:
            radius = (self.size - 1) // 2
        img = self.parent_Image.image
        return img[max(0, self.h - radius):min(img.shape[0], self.h + radius + 1),
                   max(0, self.w - radius):min(img.shape[1], self.w + radius + 1)]

    def valid_slice(self, radius=None):
        """Is the slice of the requested radius contained in the parent image.  flexlibrary.py:148-157."""
        if radius is None:
            radius = (self.size - 1) // 2
        sl = self.image_slice(radius=radius)
        return sl.shape[0] == sl.shape[1] == 2 * radius + 1

    def simple_photometry_metric(self, return_invalid=True):
        """Sum of the Spot's pixels.  flexlibrary.py:159-170."""
        if not return_invalid and not self.valid_slice():
            return None
        return np.sum(self.image_slice())

    def mexican_hat_photometry_metric(self, brim_size=6, radius=9, return_invalid=True):
        """sum(crown) - len(crown) * median(brim) over image_slice(radius), wrapped windows included.  flexlibrary.py:172-210
        (one spot through fsq_mexican_hat; photometry.mexican_hat_photometry_metric takes whole tables)."""
        from . import photometry as _ph
        if radius is None:
            radius = (self.size - 1) // 2
        if not return_invalid and not self.valid_slice(radius=radius):
            return None
        return _ph.mexican_hat_photometry_metric(self.parent_Image.image, [(self.h, self.w)], brim_size, radius)[0]

    def gaussian_volume_photometry_metric(self, scaling=10**6, default=0, return_invalid=True):
        """float(scaling) * A * sigma_h * sigma_w of the Gaussian fit.  flexlibrary.py:212-230."""
        if not return_invalid and not self.valid_slice():
            return None
        if self.gaussian_fit is None:
            return default
        return float(scaling) * self.gaussian_fit[3] * self.gaussian_fit[4] * self.gaussian_fit[5]

    def photometry(self, method='mexican_hat', photometry_method=None, return_invalid=True, **kwargs):
        """The Spot's photometry by the named method; None if return_invalid is False and the window leaves the image.
        flexlibrary.py:286-317.  sextractor, maximum and sigmas need photutils / are not built."""
        if photometry_method is not None:
            method = photometry_method
        if method == 'mexican_hat':
            return self.mexican_hat_photometry_metric(return_invalid=return_invalid, **kwargs)
        if method == 'gaussian_volume':
            return self.gaussian_volume_photometry_metric(return_invalid=return_invalid, **kwargs)
        if method == 'simple':
            return self.simple_photometry_metric(return_invalid=return_invalid, **kwargs)
        if method in ('sextractor', 'maximum', 'sigmas'):
            raise NotImplementedError("photometry method %r is not built" % (method,))
        raise ValueError("Uknown method specified.")

    def illumina_s_n(self):
        """pflib.illumina_s_n of the Spot's pixels.  flexlibrary.py:319-320."""
        from . import pflib as _pf
        return _pf.illumina_s_n(self.image_slice())


class Image(object):
    """A fluorosequencing image and its Spots: the reference's Image as far as the hot path needs it
    (flexlibrary.py:323-455): `image` (2-D array, or read from metadata['filepath'] with pflib.read_image), `metadata`,
    `spots`, and find_gaussian_psfs, which turns pflib.find_peptides' dict into Spot objects."""

    def __init__(self, image=None, metadata=None, spots=None):
        self.metadata = metadata if metadata is not None else {}
        if image is not None:
            self.image = image
        elif 'filepath' in self.metadata:
            from . import pflib as _pf
            self.image = _pf.read_image(self.metadata['filepath'])[1]
        else:
            raise AttributeError("Image.image must be defined: it was neither passed at initialization nor given a "
                                 "filepath to be read from.")
        self.spots = spots if spots is not None else []

    def _append_spots(self, new_fits, spots_append):
        if not spots_append:
            self.spots = []
        for (h, w), new_fit in new_fits.items():
            self.spots.append(Spot(self, int(_py2_round(h)), int(_py2_round(w)), 5, gaussian_fit=new_fit))
        return len(new_fits)

    def find_gaussian_psfs(self, pflib_args=None, spots_append=True):
        """Apply pflib.find_peptides to self.image and store the PSFs as Spots; returns their number.
        flexlibrary.py:426-455."""
        from . import pflib as _pf
        return self._append_spots(_pf.find_peptides(self.image, **(pflib_args or {})), spots_append)


def find_gaussian_psfs_batch(images, pflib_args=None, spots_append=True):
    """Image.find_gaussian_psfs for a list of same-shaped Images in one GPU pass (pflib.find_peptides_batch);
    returns the numbers of Spots found."""
    from . import pflib as _pf
    images = list(images)
    if not images:
        return []
    tables = _pf.find_peptides_batch(np.stack([np.asarray(im.image) for im in images]), **(pflib_args or {}))
    return [im._append_spots(t, spots_append) for im, t in zip(images, tables)]


class Experiment(object):
    """The static tracking helpers of the reference's Experiment class."""

    @staticmethod
    def easy_load_processed_image(image_filepath, psf_pkl_filepath=None, load_psfs=True):
        """Load a processed image and the PSF pickle pflib wrote for it into an Image with its Spots.
        Reference flexlibrary.py:516-564 (the resume mechanism of the experiment scripts: an image that has a
        `<image>*_psfs_*.pkl` next to it is not fitted again, basic_experiment_script.py:243-247, 377-399).

        image_filepath: path of the PNG image; psf_pkl_filepath: its pickle, or None to take the last of
        sorted(glob(image_filepath + '*_psfs_*.pkl')) - the file names end in the base-36 time stamp of
        pflib._psfs_filename, so that is the most recent one; load_psfs=False: the Image gets no Spots.
        Returns (Image, number of PSFs whose Spot could not be made): every PSF becomes a Spot at the Python-2-rounded
        dict key with size fit_img.shape[0]; a PSF for which Spot.__init__ raises is logged and counted."""
        import glob
        import logging
        import pickle
        from PIL import Image as _PILImage
        logger = logging.getLogger(__name__)
        with _PILImage.open(image_filepath) as f:
            image = np.array(f)
        image_object = Image(image=image, metadata={'filepath': image_filepath}, spots=None)
        discarded_spots = 0
        if load_psfs:
            if psf_pkl_filepath is None:
                pkl_files = sorted(glob.glob(image_filepath + '*_psfs_*.pkl'))
                if len(pkl_files) == 0:
                    raise ValueError("For image_filepath = " + image_filepath + " psf_pkl_filepath passed as None when " +
                                     "no pkl files available.")
                psf_pkl_filepath = pkl_files[-1]
            with open(psf_pkl_filepath, 'rb') as f:
                psfs = pickle.load(f, encoding='latin1')        # (latin1: files written by the reference's Python 2)
            spot_objects = []
            for (h, w), gaussian_fit in psfs.items():
                fit_img = gaussian_fit[8]
                try:
                    spot_objects.append(Spot(parent_Image=image_object, h=int(_py2_round(h)), w=int(_py2_round(w)),
                                             size=fit_img.shape[0], gaussian_fit=gaussian_fit))
                except Exception as e:      # noqa: BLE001 - as the reference: logged, counted, skipped
                    logger.info("flexlibrary.easy_load_processed_image: Ignoring Spot due to Spot.__init__ exception.")
                    logger.exception(e, exc_info=True)
                    discarded_spots += 1
            image_object.spots = spot_objects
        return image_object, discarded_spots

    @staticmethod
    def luminosity_centroid_particle_tracking(frames, initial_spots, search_radius=3, s_n_cutoff=3.0, offsets=None):
        """Follow Spots through frames by the centroid of pixel luminosity.  flexlibrary.py:1262-1317.
        frames: Images (objects with `.image`) of one shape; initial_spots: Spots of frames[0] (size 5).
        Returns one list per spot: its Spot in every frame, or None."""
        frames = list(frames)
        if not all(spot.parent_Image is frames[0] for spot in initial_spots):
            raise ValueError("All initial_spots must be in frames[0].")
        initial_spots = list(initial_spots)
        if not initial_spots:
            return []
        if any(s.size != 5 for s in initial_spots):
            raise NotImplementedError("luminosity-centroid tracking on the GPU handles Spots of size 5")
        stack = np.stack([np.asarray(f.image) for f in frames])
        off = None if offsets is None else np.asarray([(o[0], o[1]) for o in offsets])[None]
        hw, present = centroid_track_fields(stack, [(s.h, s.w) for s in initial_spots], None, search_radius, s_n_cutoff, off)
        tracks = []
        for spot, row, pr in zip(initial_spots, hw, present):
            tr = [spot]
            for f in range(1, len(frames)):
                tr.append(Spot(frames[f], int(row[f][0]), int(row[f][1]), spot.size) if pr[f] else None)
            tracks.append(tr)
        return tracks

    @staticmethod
    def easy_sort_target_images(filepath_list):
        """Sort image files by field of view and order taken: every directory is one experimental cycle (directories in
        sorted order), the sorted file names of a directory are its fields.  flexlibrary.py:1106-1154.
        Returns (frame_indexed {cycle: [absolute paths, one per field]}, field_indexed {field: [paths, one per cycle]})."""
        import os
        by_directory = {}
        for path in filepath_list:
            directory, name = os.path.split(os.path.abspath(path))
            by_directory.setdefault(directory, []).append(name)
        frame_indexed = {}
        for index, directory in enumerate(sorted(by_directory)):
            for name in sorted(by_directory[directory]):
                frame_indexed.setdefault(index, []).append(os.path.join(directory, name))
        field_indexed = {}
        for frame, fields in frame_indexed.items():
            for f, field in enumerate(fields):
                field_indexed.setdefault(f, []).append(field)
        return frame_indexed, field_indexed

    @staticmethod
    def trace_to_binary(trace):
        return [spot is not None for spot in trace]                 # flexlibrary.py:1157-1158

    @staticmethod
    def truefalse_to_onoff(pattern):
        return ' '.join(['[ON] ' if p else '[OFF]' for p in pattern])   # flexlibrary.py:1161-1162

    @staticmethod
    def trace_to_photometry(trace, method='mexican_hat', return_invalid=True, **kwargs):
        """[(h, w, photometry)] of a trace's Spots, (None, None, None) where it has none.  flexlibrary.py:1165-1170.
        Spot by Spot (one small launch each for the hat); the experiment classes measure whole experiments in one."""
        return [(spot.h, spot.w, spot.photometry(method=method, return_invalid=return_invalid, **kwargs))
                if spot is not None else (None, None, None) for spot in trace]

    @staticmethod
    def accumulate_offsets(offsets):
        """Offsets relative to the preceding image -> offsets relative to the first.  flexlibrary.py:567-593."""
        if offsets[0] != (0, 0):
            raise ValueError("The first image's offset must be (0, 0) by definiton.")
        return [(sum([o[0] for o in offsets[:f + 1]]), sum([o[1] for o in offsets[:f + 1]])) for f in range(len(offsets))]

    @staticmethod
    def get_cumulative_offset(offsets, f, g=0):
        """Cumulative offset of frame f with respect to frame g.  flexlibrary.py:595-601."""
        cf = Experiment.accumulate_offsets(offsets)[f]
        cg = Experiment.accumulate_offsets(offsets)[g]
        return (cf[0] - cg[0], cf[1] - cg[1])

    @staticmethod
    def round_coordinates(h, w):
        return int(_py2_round(h)), int(_py2_round(w))             # flexlibrary.py:603-605 (Python 2 round)

    @staticmethod
    def apply_offset(coordinates, offset):
        return coordinates[0] + offset[0], coordinates[1] + offset[1]

    @staticmethod
    def unapply_offset(offset_coordinates, offset):
        return offset_coordinates[0] - offset[0], offset_coordinates[1] - offset[1]

    @staticmethod
    def offset_frame_coordinates(offsets, coordinate, f, g):
        """Given a coordinate in frame g, its coordinate in frame f.  flexlibrary.py:619-624."""
        return Experiment.apply_offset(coordinate, Experiment.get_cumulative_offset(offsets=offsets, f=f, g=g))

    @staticmethod
    def discard_dropouts(spots, spot_cumulative_offsets, frame_cumulative_offsets, image_shape, spot_radius=0):
        """Drop the Spots whose position falls outside some frame of the sequence.  flexlibrary.py:626-678.
        (Host arithmetic: a handful of comparisons per spot; the tracking kernel applies the same rule itself.)"""
        filtered, discarded = [], 0
        for i, spot in enumerate(spots):
            oh, ow = Experiment.apply_offset((spot.h, spot.w), spot_cumulative_offsets[i])
            for offset in frame_cumulative_offsets:
                gh, gw = Experiment.unapply_offset((oh, ow), offset)
                if not (spot_radius <= gh < image_shape[0] - 0.5 - spot_radius and
                        spot_radius <= gw < image_shape[1] - 0.5 - spot_radius):
                    discarded += 1
                    break
            else:
                filtered.append(spot)
        return filtered, discarded

    @staticmethod
    def greedy_particle_tracking(frame_spots, frame_shape, candidate_radius=2, offsets=None, spot_radius=0):
        """Track Spots across frames.  flexlibrary.py:680-1027.

        frame_spots: iterable (frames) of iterables of objects with integer `.h` / `.w`; offsets: (delta_h, delta_w) of
        every frame relative to the one before.  Returns (traces, number of discarded spots): one list per tracked spot
        holding its Spot object (or None) for every frame, in the reference's order."""
        frame_spots = [list(fr) for fr in frame_spots]
        if offsets is None:
            raise TypeError("'int' object is not iterable")       # the reference's default branch fails the same way (:787)
        res = track_fields([[np.array([(s.h, s.w) for s in fr]).reshape(-1, 2) for fr in frame_spots]],
                           [list(offsets)], frame_shape, candidate_radius, spot_radius)[0]
        flat = [s for fr in frame_spots for s in fr]
        traces = [[(flat[i] if i >= 0 else None) for i in row] for row in res[0]]
        return traces, res[1]


# ---- sequence experiments: every track of every field and channel through one launch (sequencing.py, include/fsq_sequence.h) ----

def _photometry_plan(method, kwargs):
    """Spot.photometry's dispatch (flexlibrary.py:286-317) for a whole experiment -> dict(method, device, radius, brim_size,
    scaling, default).  `device` is the kernel's method: the hat, or the spot_size window ('simple'; it also gives
    gaussian_volume its positions and validity, the volumes come from the fit tuples on the host)."""
    kwargs = dict(kwargs or {})
    override = kwargs.pop('photometry_method', None)
    if override is not None:
        method = override
    plan = dict(method=method, device='simple', radius=None, brim_size=0, scaling=10 ** 6, default=0)
    if method == 'mexican_hat':
        plan.update(device='mexican_hat', brim_size=kwargs.pop('brim_size', 6), radius=kwargs.pop('radius', 9))
    elif method == 'gaussian_volume':
        plan.update(scaling=kwargs.pop('scaling', 10 ** 6), default=kwargs.pop('default', 0))
    elif method in ('sextractor', 'maximum', 'sigmas'):
        raise NotImplementedError("photometry method %r is not built" % (method,))
    elif method != 'simple':
        raise ValueError("Uknown method specified.")                   # flexlibrary.py:315
    if kwargs:
        raise TypeError("%s photometry got an unexpected keyword argument %r" % (method, sorted(kwargs)[0]))
    return plan


def _sequence_records(experiments, plan, interpolate):
    """The traces of many SequenceExperiments through sequencing.sequence_photometry_records: one launch per group of
    sequences with the same number of frames, frame shape and Spot size.  -> one dict per experiment: `hw` [n][F] of (h, w) or
    None, `values` [n][F] photometry or None, `flags` uint8 [n, F], `valid` bool [n], `size`."""
    from . import sequencing as _sq
    groups, out = {}, [None] * len(experiments)
    for k, ex in enumerate(experiments):
        F = len(ex.peptide_frames)
        shape = tuple(ex.peptide_frames[0].image.shape)
        if any(tuple(fr.image.shape) != shape for fr in ex.peptide_frames):
            raise ValueError("all frames of a SequenceExperiment must have one shape")
        traces = ex.spot_traces or []
        sizes = set(spot.size for trace in traces for spot in trace if spot is not None)
        if len(sizes) > 1:
            raise NotImplementedError("Spots of different sizes in one SequenceExperiment")
        size = sizes.pop() if sizes else 5
        if any(len(trace) != F for trace in traces):
            raise ValueError("every trace needs one entry per frame")
        offsets = ex.offsets if ex.offsets is not None else [(0, 0)] * F
        if len(offsets) != F:
            raise ValueError("offsets must have one entry per frame")
        groups.setdefault((F,) + shape + (size,), []).append((k, ex, traces, offsets))
    for (F, H, W, size), members in groups.items():
        hw_in, seq = [], []
        for s, (k, ex, traces, offsets) in enumerate(members):
            for trace in traces:
                hw_in.append([(-1, -1) if spot is None else (spot.h, spot.w) for spot in trace])
                seq.append(s)
        n = len(hw_in)
        off = np.array([[(float(o[0]), float(o[1])) for o in offsets] for _, _, _, offsets in members], dtype=np.float64)
        radius = plan['radius'] if plan['radius'] is not None else (size - 1) // 2
        if n:
            frames = np.stack([np.asarray(fr.image) for _, ex, _, _ in members for fr in ex.peptide_frames])
            rec = _sq.sequence_photometry_records(frames.reshape((len(members), F) + frames.shape[1:]),
                                                  np.asarray(hw_in).reshape(n, F, 2), seq, off, method=plan['device'], radius=radius,
                                                  brim_size=plan['brim_size'], spot_size=size, interpolate=interpolate, counts=False)
        else:
            _sq.check_arguments((len(members), F, H, W), np.zeros((0, F, 2), np.int32), [], off, plan['device'], radius,
                                plan['brim_size'], size)
        start = 0
        for s, (k, ex, traces, offsets) in enumerate(members):
            m = len(traces)
            if not m:
                out[k] = dict(hw=[], values=[], flags=np.zeros((0, F), np.uint8), valid=np.zeros(0, bool), size=size)
                continue
            sl = slice(start, start + m)
            start += m
            flags = rec['flags'][sl]
            have = (flags & 3) != 0
            hw = [[(h, w) if ok else None for (h, w), ok in zip(row, okrow)]
                  for row, okrow in zip(rec['hw'][sl].tolist(), have.tolist())]
            if plan['method'] == 'mexican_hat':
                values = [[v if ok else None for v, ok in zip(row, okrow)]
                          for row, okrow in zip(rec['photometry'][sl].tolist(), have.tolist())]
            elif plan['method'] == 'simple':
                values = [[int(v) if ok else None for v, ok in zip(row, okrow)]
                          for row, okrow in zip(rec['photometry'][sl].tolist(), have.tolist())]
            else:                                                       # gaussian_volume: from the fit tuples; an interpolated Spot has none
                values = []
                for trace, okrow in zip(traces, have.tolist()):
                    values.append([None if not ok else plan['default'] if (spot is None or spot.gaussian_fit is None) else
                                   float(plan['scaling']) * spot.gaussian_fit[3] * spot.gaussian_fit[4] * spot.gaussian_fit[5]
                                   for spot, ok in zip(trace, okrow)])
            out[k] = dict(hw=hw, values=values, flags=flags, valid=rec['trace_valid'][sl], size=size)
    return out


def _append_interpolated_spots(ex, trace, hw_row, size):
    """What fill_in_trace leaves behind (flexlibrary.py:1842-2032), given the filled-in positions: for every hole of the trace,
    interpolate_spots appends a new Spot to frame.spots for every position of the span that lies inside its frame - the
    bookend frames included, on every call.  Returns the merged trace (the trace's own Spots, new Spots or None in the holes)."""
    F, r = len(trace), (size - 1) // 2
    merged = list(trace)
    f = 0
    while f < F:
        if trace[f] is not None:
            f += 1
            continue
        g = f
        while g < F and trace[g] is None:
            g += 1
        for i in range(f - 1 if f > 0 else f, (g if g < F else g - 1) + 1):
            frame = ex.peptide_frames[i]
            if trace[i] is None:
                if hw_row[i] is None:
                    continue
                h, w = hw_row[i]
            else:                                                       # a bookend: copied if it passes the same frame test
                h, w = trace[i].h, trace[i].w
                if not (r <= h < frame.image.shape[0] - r and r <= w < frame.image.shape[1] - r):
                    continue
            spot = Spot(parent_Image=frame, h=h, w=w, size=size, gaussian_fit=None)
            frame.spots.append(spot)
            if trace[i] is None:
                merged[i] = spot
        f = g
    return merged


def _trace_existing_spots(experiments):
    """SequenceExperiment.trace_existing_spots for many experiments: one track_fields call per frame shape."""
    groups = {}
    for ex in experiments:
        key = (len(ex.peptide_frames),) + tuple(ex.peptide_frames[0].image.shape)
        groups.setdefault(key, []).append(ex)
    for key, members in groups.items():
        for ex in members:
            if ex.offsets is None:
                raise TypeError("'int' object is not iterable")         # (as greedy_particle_tracking without offsets)
        res = track_fields([[np.array([(s.h, s.w) for s in image.spots]).reshape(-1, 2) for image in ex.peptide_frames]
                            for ex in members], [list(ex.offsets) for ex in members], key[1:], 2, 0)
        for ex, r in zip(members, res):
            flat = [s for image in ex.peptide_frames for s in image.spots]
            ex.spot_traces = [[(flat[i] if i >= 0 else None) for i in row] for row in r[0]]
            ex.num_discarded_spots = r[1]


def _discard_invalid_traces(experiments, pparams):
    """SequenceExperiment.discard_invalid_traces (flexlibrary.py:2034-2063) for many experiments in one launch."""
    pparams = dict(pparams)
    plan = _photometry_plan(pparams.pop('method', 'mexican_hat'), pparams)
    recs = _sequence_records(experiments, plan, True)
    out = []
    for ex, rec in zip(experiments, recs):
        valid_traces, invalid_traces = [], []
        for t, trace in enumerate(ex.spot_traces or []):
            filled = _append_interpolated_spots(ex, trace, rec['hw'][t], rec['size'])
            if rec['valid'][t]:
                valid_traces.append(trace)
            else:
                invalid_traces.append(filled)
        ex.spot_traces = valid_traces
        out.append(invalid_traces)
    return out


def _binary_trace_categories_photometry(experiments, method, interpolate, discard_invalid, adjustment_function, kwargs):
    """SequenceExperiment.binary_trace_categories_photometry (flexlibrary.py:2065-2129) for many experiments in one launch."""
    if discard_invalid:
        raise DeprecationWarning("discard_invalid is deprecated. Use discard_invalid_traces() functions")
    plan = _photometry_plan(method, kwargs)
    recs = _sequence_records(experiments, plan, bool(interpolate))
    out = []
    for ex, rec in zip(experiments, recs):
        order, rows = {}, {}
        for t, trace in enumerate(ex.spot_traces or []):                # categories in order of first appearance, then their traces
            order.setdefault(tuple(Experiment.trace_to_binary(trace)), []).append(t)
        for category, members in order.items():
            for t in members:
                if interpolate:
                    _append_interpolated_spots(ex, ex.spot_traces[t], rec['hw'][t], rec['size'])
                p = [(hw[0], hw[1], v) if hw is not None else _NONE3 for hw, v in zip(rec['hw'][t], rec['values'][t])]
                if adjustment_function is not None:
                    p = [(h, w, adjustment_function(photometry=ph, frame=frame, adjustments=ex.photometry_adjustments))
                         for frame, (h, w, ph) in enumerate(p)]
                rows.setdefault(category, []).append(p)
        out.append(rows)
    return out


_NONE3 = (None, None, None)         # the placeholder of trace_to_photometry; track_photometries_as_csv tells it by identity


def _mdma(experiments, tag, method, kwargs):
    """SequenceExperiment.multiplicative_delta_median_adjustments (flexlibrary.py:2131-2200) for many experiments."""
    btcps = _binary_trace_categories_photometry(experiments, method, False, False, None, kwargs)
    out = []
    for ex, btcp in zip(experiments, btcps):
        F = len(ex.peptide_frames)
        all_on = [p for p in btcp.get(tuple([True] * F), []) if all(ph is not None for h, w, ph in p)]
        ratios = [[] for _ in range(F)]
        for p in all_on:
            m = np.median([ph for h, w, ph in p])
            for i, (h, w, ph) in enumerate(p):
                ratios[i].append(float(ph - m) / m)
        if ex.photometry_adjustments is None:
            ex.photometry_adjustments = {}
        ex.photometry_adjustments['mdma'] = tuple(np.median(r) if len(r) > 0 else 0.0 for r in ratios)   # (`tag` is not used, :2198)
        out.append(ex.photometry_adjustments['mdma'])
    return out


class SequenceExperiment(Experiment):
    """A sequence of frames of one field: the reference's SequenceExperiment as far as registration and tracking go
    (flexlibrary.py:1680-1810): `peptide_frames` / `alignment_frames` (Images), `offsets`, `spot_traces`."""

    def __init__(self, peptide_frames, alignment_frames=None, offsets=None, spot_traces=None, num_discarded_spots=0,
                 photometry_adjustments=None):
        self.peptide_frames = peptide_frames
        self.alignment_frames = alignment_frames
        self.offsets = offsets
        self.spot_traces = spot_traces
        self.num_discarded_spots = num_discarded_spots
        self.photometry_adjustments = photometry_adjustments

    def offsets_from_frames(self, upsample_factor=20):
        """Frame-to-frame alignment by phase correlation, all pairs in one GPU call.  flexlibrary.py:1717-1741."""
        from . import phase_correlate as _pc
        if self.alignment_frames is None:
            raise AttributeError("Calling offsets_from_frames without alignment_frames defined.")
        self.offsets = _pc.offsets_from_frames(self.alignment_frames, upsample_factor=upsample_factor)
        return self.offsets

    def trace_existing_spots(self, spot_radius=None):
        """greedy_particle_tracking over the Spots the frames already hold.  flexlibrary.py:1770-1809."""
        if spot_radius is not None:
            raise NotImplementedError("spot_radius currently not implemented")
        self.spot_traces, self.num_discarded_spots = Experiment.greedy_particle_tracking(
            frame_spots=[image.spots for image in self.peptide_frames], frame_shape=self.peptide_frames[0].image.shape,
            offsets=self.offsets, spot_radius=0)
        return self.spot_traces

    def binary_trace_categories(self):
        """{ON/OFF pattern: [traces]} of self.spot_traces, patterns in order of first appearance.  flexlibrary.py:1812-1840."""
        categories = {}
        for trace in self.spot_traces:
            categories.setdefault(tuple(Experiment.trace_to_binary(trace)), []).append(trace)
        return categories

    def interpolate_spots(self, start, stop):
        """New Spots along the line between (start_spot, start_frame) and (stop_spot, stop_frame); one of the two Spots may be
        None, then the other's position is used throughout.  flexlibrary.py:1842-1974 (host arithmetic: a few operations per
        frame; whole experiments go through fsq_sequence_photometry).  Every Spot made is appended to its frame's spots; a
        position outside its frame gives None."""
        (start_spot, start_frame), (stop_spot, stop_frame) = start, stop
        if not start_frame < stop_frame:
            raise ValueError("start_frame must come before stop_frame")
        if start_spot is not None and stop_spot is not None and not start_frame + 1 < stop_frame:
            raise ValueError("If neither start_spot or stop_spot are None, stop_frame must have at least one frame between it "
                             "and start_frame.")
        if start_spot is None and stop_spot is None:
            raise ValueError("Both start_spot and stop_spot are None.")
        offsets = self.offsets if self.offsets is not None else [(0, 0) for _ in self.peptide_frames]
        if stop_spot is not None:
            stop_h, stop_w = Experiment.offset_frame_coordinates(offsets=offsets, coordinate=(stop_spot.h, stop_spot.w),
                                                                 f=start_frame, g=stop_frame)
        if start_spot is not None:
            start_h, start_w = start_spot.h, start_spot.w
        else:
            start_h, start_w = stop_h, stop_w
        if stop_spot is None:
            stop_h, stop_w = start_h, start_w
        if start_spot is not None and stop_spot is not None and start_spot.size != stop_spot.size:
            raise ValueError("start_spot.size != stop_spot.size")
        size = start_spot.size if start_spot is not None else stop_spot.size
        n, r = stop_frame - start_frame, (size - 1) // 2
        inc_h, inc_w = float(stop_h - start_h) / n, float(stop_w - start_w) / n
        assert abs(start_h + inc_h * n - stop_h) < 0.01 and abs(start_w + inc_w * n - stop_w) < 0.01
        spots = []
        for i in range(n + 1):
            frame = self.peptide_frames[start_frame + i]
            h, w = Experiment.apply_offset((start_h + inc_h * i, start_w + inc_w * i),
                                           Experiment.get_cumulative_offset(offsets=offsets, f=i + start_frame, g=start_frame))
            h, w = Experiment.round_coordinates(h, w)
            if r <= h < frame.image.shape[0] - r and r <= w < frame.image.shape[1] - r:
                spot = Spot(parent_Image=frame, h=h, w=w, size=size, gaussian_fit=None)
                frame.spots.append(spot)
            else:
                spot = None
            spots.append(spot)
        return spots

    def fill_in_trace(self, trace):
        """The trace with its None entries replaced by interpolated Spots (None where the position leaves the frame).
        flexlibrary.py:1976-2032; the positions come from fsq_sequence_photometry (one trace, one launch)."""
        kept, self.spot_traces = self.spot_traces, [trace]
        try:
            rec = _sequence_records([self], _photometry_plan('simple', {}), True)[0]
        finally:
            self.spot_traces = kept
        return _append_interpolated_spots(self, trace, rec['hw'][0], rec['size'])

    def discard_invalid_traces(self, **pparams):
        """Removes from self.spot_traces every trace that, filled in, has a Spot outside its frame or a photometry window
        that leaves it; returns the removed traces, filled in.  flexlibrary.py:2034-2063."""
        return _discard_invalid_traces([self], pparams)[0]

    def binary_trace_categories_photometry(self, method='mexican_hat', interpolate=False, discard_invalid=False,
                                           adjustment_function=None, **kwargs):
        """binary_trace_categories with every trace replaced by its [(h, w, photometry)] per frame; (None, None, None) where
        it has no Spot (interpolate=True: only where the filled-in position leaves the frame).  flexlibrary.py:2065-2129."""
        return _binary_trace_categories_photometry([self], method, interpolate, discard_invalid, adjustment_function, kwargs)[0]

    def multiplicative_delta_median_adjustments(self, tag='mdma', method='mexican_hat', **kwargs):
        """Per-frame medians of (photometry - median) / median over the traces that are ON in every frame, stored in
        self.photometry_adjustments['mdma'] and returned; zeros without such traces.  flexlibrary.py:2131-2200."""
        return _mdma([self], tag, method, kwargs)[0]

    @staticmethod
    def mdma_adjustment(photometry, frame, adjustments):
        """photometry * (1 - adjustments['mdma'][frame]).  flexlibrary.py:2202-2221."""
        if 'mdma' in adjustments:
            return photometry * (1.0 - adjustments['mdma'][frame])
        return photometry

    def count_remainders(self):
        """Number of traces that are ON in every frame.  flexlibrary.py:2223-2231."""
        return len(self.binary_trace_categories().get(tuple([True] * len(self.peptide_frames)), []))

    def spot_count(self):
        return sum(len(frame.spots) for frame in self.peptide_frames)             # flexlibrary.py:2285-2293

    def singleton_count(self):
        return sum(1 for trace in self.spot_traces if len([t for t in trace if t is not None]) == 1)    # :2295-2301


def _frame_counts_agree(channels):
    """The constructors' test (flexlibrary.py:2495-2503, 2652-2663): one number of peptide_frames and of alignment_frames over
    all channels.  (alignment_frames None counts as the reference's list of None placeholders, one per peptide frame.)"""
    n_peptide = set(len(chan.peptide_frames) for chan in channels)
    n_alignment = set(len(chan.alignment_frames if chan.alignment_frames is not None else chan.peptide_frames)
                      for chan in channels)
    return len(n_peptide) == len(n_alignment) and len(n_alignment) == 1


def _filtered_counts(counts, include_first_frame_only):
    """Patterns with a single ON -> OFF transition (flexlibrary.py:2935-2946): all ON frames come first."""
    return {bt: count for bt, count in counts.items()
            if tuple(sorted(bt, reverse=True)) == bt and (include_first_frame_only or bt[1])}


# ---- the text of the two CSV files and of the summary: shared by the classes below and by the records route (experiment.py) ----

def _track_photometries_header(save_averages, n_frames):
    if save_averages:
        return ['CHANNEL', 'FIELD', 'H', 'W', 'CATEGORY', 'AVERAGE_INTENSITY']
    return ['CHANNEL', 'FIELD', 'H', 'W', 'CATEGORY'] + ['FRAME ' + str(i) for i in range(n_frames)]


def _track_photometries_row(chan, e, h, w, category, values, save_averages):
    """One row of track_photometries_as_csv: `values` holds the trace's photometry per frame, None where it has no Spot."""
    if save_averages:
        mean = np.mean([v for v in values if v is not None])
        return [str(chan), str(e), str(h), str(w), str(category), str(mean)]
    return [str(chan), str(e), str(h), str(w), str(category)] + [str(v) if v is not None else '0' for v in values]


def _write_category_counts_csv(filepath, to_save, collate_fields, dialect='excel'):
    """{channel: {field: {pattern: count}}} as category_counts_as_csv writes it (flexlibrary.py:2948-3024)."""
    import csv
    channels = sorted(to_save.keys())            # (filtered=False: a tuple has no keys - the reference fails the same way)
    patterns = sorted(set(pattern for fields in to_save.values() for counts in fields.values() for pattern in counts))
    with open(filepath, 'w') as output_file:
        writer = csv.writer(output_file, dialect=dialect)
        writer.writerow(["Pattern", "Field", "Channel", "Count"] if collate_fields else ["Pattern", "Channel", "Count"])
        for pattern in patterns:
            onoff = Experiment.truefalse_to_onoff(pattern)
            for chan in channels:
                if collate_fields:
                    for e, ex in to_save[chan].items():
                        writer.writerow([onoff, str(e), str(chan), str(ex[pattern]) if pattern in ex else '0'])
                else:
                    writer.writerow([onoff, str(chan), str(sum(ex[pattern] for ex in to_save[chan].values() if pattern in ex))])
    return filepath


def _category_counts_string(to_string, collate_fields):
    """{channel: {field: {pattern: count}}} as the text of category_counts_as_string (flexlibrary.py:3026-3077)."""
    out = ''
    for chan, ex in sorted(to_string.items(), key=lambda x: x[0]):
        if collate_fields:
            for e, patterns in ex.items():
                out += " Channel " + str(chan) + " Frame " + str(e) + "\n"
                for pattern, count in sorted(patterns.items(), key=lambda x: x[0]):
                    out += "    " + Experiment.truefalse_to_onoff(pattern) + "    " + str(count) + "\n"
        else:
            merged = {}
            for patterns in ex.values():
                for pattern, count in patterns.items():
                    merged[pattern] = merged.get(pattern, 0) + count
            out += str(chan) + "\n"
            for pattern, count in sorted(merged.items(), key=lambda x: x[0]):
                out += "    " + Experiment.truefalse_to_onoff(pattern) + "    " + str(count) + "\n"
    return out


def _offsets_string(by_frame):
    """{frame: {field: {channel: (d_h, d_w)}}} as the text of offsets_as_string."""
    out = ''
    for f, frame_offsets in sorted(by_frame.items()):
        out += "Frame " + str(f) + "\n"
        for e, ex_offsets in sorted(frame_offsets.items(), key=lambda x: x[0]):
            out += "    Field " + str(e) + "\n"
            for c, (h, w) in sorted(ex_offsets.items(), key=lambda x: x[0]):
                out += "        Channel " + str(c) + " " + str((h, w)) + "\n"
            all_h, all_w = [h for h, w in ex_offsets.values()], [w for h, w in ex_offsets.values()]
            out += "        Mean Offsets for Field " + str(e) + " = " + str((np.mean(all_h), np.mean(all_w))) + "\n"
            out += "        Std.Dev. Offsets for Field " + str(e) + " = " + str((np.std(all_h), np.std(all_w))) + "\n"
        all_h = [h for ex_offsets in frame_offsets.values() for h, w in ex_offsets.values()]
        all_w = [w for ex_offsets in frame_offsets.values() for h, w in ex_offsets.values()]
        out += "    Mean Offsets for Frame " + str(f) + str((np.mean(all_h), np.mean(all_w))) + "\n"
        out += "        Std.Dev. Offsets for Field " + str(f) + " = " + str((np.std(all_h), np.std(all_w))) + "\n"
    return out


class MultifieldSequenceExperiment(Experiment):
    """SequenceExperiments over several fields (flexlibrary.py:2384-2468).  As in the reference, the class only serves as
    the base of MultifieldMultichannelSequenceExperiment: its own constructor raises DeprecationWarning."""

    def __init__(self, experimental_fields):
        self.experimental_fields = experimental_fields
        raise DeprecationWarning("This class is no longer maintained. Use MultifieldMultichannelSequenceExperiment instead.")


class MultichannelSequenceExperiment(SequenceExperiment):
    """One field of view in several colour channels: `channels` {name: SequenceExperiment}.  flexlibrary.py:2471-2629.
    Every method that measures gathers all channels into one launch."""

    def __init__(self, channels):
        if not _frame_counts_agree(list(channels.values())):
            raise AttributeError("Number of peptide_frames and alignment_framesdoes not match across channels.")
        self.channels = channels

    def _experiments(self):
        return list(self.channels.values())

    def _per_channel(self, results):
        return dict(zip(self.channels.keys(), results))

    def trace_existing_spots(self):
        _trace_existing_spots(self._experiments())

    def binary_trace_categories(self):
        return {c: chan.binary_trace_categories() for c, chan in self.channels.items()}

    def binary_trace_categories_photometry(self, method='mexican_hat', interpolate=False, discard_invalid=False,
                                           adjustment_function=None, **kwargs):
        return self._per_channel(_binary_trace_categories_photometry(self._experiments(), method, interpolate, discard_invalid,
                                                                     adjustment_function, kwargs))

    def count_binary_trace_categories(self):
        merged = self.binary_trace_categories()
        return {c: {k: len(v) for k, v in chan.items()} for c, chan in merged.items()}, merged

    def filtered_binary_trace_category_counts(self):
        counts, merged = self.count_binary_trace_categories()
        return {c: _filtered_counts(chan, False) for c, chan in counts.items()}

    def plot_filtered_binary_trace_counts(self, output_filepaths):
        raise DeprecationWarning("Deprecating for now in favor of outputting CSV files. Assume this function is no longer "
                                 "maintained.")

    def count_discarded_spots(self):
        return {c: chan.num_discarded_spots for c, chan in self.channels.items()}

    def spot_count(self):
        return {c: chan.spot_count() for c, chan in self.channels.items()}

    def trace_count(self):
        return {c: len(chan.spot_traces) for c, chan in self.channels.items()}

    def singleton_count(self):
        return {c: chan.singleton_count() for c, chan in self.channels.items()}

    def get_offsets(self):
        return {c: chan.offsets for c, chan in self.channels.items()}

    def discard_invalid_traces(self, **pparams):
        return self._per_channel(_discard_invalid_traces(self._experiments(), pparams))

    def multiplicative_delta_median_adjustments(self, tag='mdma', method='mexican_hat', channels=None, **kwargs):
        names = [c for c in self.channels if channels is None or c in channels]
        return dict(zip(names, _mdma([self.channels[c] for c in names], tag, method, kwargs)))

    def count_remainders(self):
        return {c: chan.count_remainders() for c, chan in self.channels.items()}


class MultifieldMultichannelSequenceExperiment(MultifieldSequenceExperiment):
    """A sequencing experiment: `experimental_fields`, a list of MultichannelSequenceExperiments, and `invalid_fields_mask`
    (False = the field is left out where ignore_invalid_fields is set).  flexlibrary.py:2632-3263.

    trace_existing_spots, discard_invalid_traces, binary_trace_categories_photometry, track_photometries_as_csv and
    multiplicative_delta_median_adjustments gather every field and channel and run one tracking call / one
    fsq_sequence_photometry launch (per frame shape).  Nested results keep the reference's layout
    {channel: {field: {pattern: ...}}}: channels in the order of the fields' `channels` dicts, fields ascending, patterns in
    order of first appearance in spot_traces."""

    def __init__(self, experimental_fields, invalid_fields_mask=None):
        if not _frame_counts_agree([chan for ex in experimental_fields for chan in ex.channels.values()]):
            raise AttributeError("Number of peptide_frames and alignment_framesdoes not match across fields and channels.")
        self.experimental_fields = experimental_fields
        if invalid_fields_mask is not None:
            if len(invalid_fields_mask) != len(self.experimental_fields):
                raise AttributeError("invalid_fields_mask must be the same length as experimental_fields.")
            self.invalid_fields_mask = invalid_fields_mask
        else:
            self.invalid_fields_mask = [True] * len(self.experimental_fields)

    def _fields(self, ignore_invalid_fields=False):
        return [(e, ex) for e, ex in enumerate(self.experimental_fields)
                if not (ignore_invalid_fields and not self.invalid_fields_mask[e])]

    def _sequences(self, ignore_invalid_fields=False):
        """[(field index, channel name, SequenceExperiment)] of the fields in use."""
        return [(e, c, chan) for e, ex in self._fields(ignore_invalid_fields) for c, chan in ex.channels.items()]

    def _per_field(self, sequences, results, ignore_invalid_fields):
        """Results per sequence -> the reference's list over ALL fields of {channel: result} (False for a field left out)."""
        out = [False if (ignore_invalid_fields and not self.invalid_fields_mask[e]) else {}
               for e in range(len(self.experimental_fields))]
        for (e, c, _), r in zip(sequences, results):
            out[e][c] = r
        return out

    @staticmethod
    def _merge(sequences, results):
        merged = {}
        for (e, c, _), categories in zip(sequences, results):
            per_field = merged.setdefault(c, {}).setdefault(e, {})
            for k, v in categories.items():
                per_field.setdefault(k, [])
                per_field[k] += v
        return merged

    def trace_existing_spots(self, parallel=False, ignore_invalid_fields=False):
        if parallel:
            raise NotImplementedError("Classes in multiple processes do not share state, therefore if we want to parallelize "
                                      "this function, we will need to shuttle information between instances.")
        _trace_existing_spots([chan for _, _, chan in self._sequences(ignore_invalid_fields)])

    def binary_trace_categories(self, ignore_invalid_fields=False):
        seqs = self._sequences(ignore_invalid_fields)
        return self._merge(seqs, [chan.binary_trace_categories() for _, _, chan in seqs])

    def binary_trace_categories_photometry(self, method='mexican_hat', interpolate=False, discard_invalid=False,
                                           adjustment_function=None, ignore_invalid_fields=False, **kwargs):
        seqs = self._sequences(ignore_invalid_fields)
        return self._merge(seqs, _binary_trace_categories_photometry([chan for _, _, chan in seqs], method, interpolate,
                                                                     discard_invalid, adjustment_function, kwargs))

    def track_photometries_as_csv(self, filepath, dialect='excel', photometry_method='mexican_hat', save_averages=True,
                                  discard_invalid=False, ignore_invalid_fields=False, adjustment_function=None, **kwargs):
        """One row per track: CHANNEL, FIELD, H, W, CATEGORY and either AVERAGE_INTENSITY (numpy.mean over the frames the Spot
        was detected in) or, with save_averages=False, FRAME 0 .. FRAME n-1 with holes filled in by interpolation ('0' where
        the filled-in position leaves the frame).  H, W are those of the first frame that has a Spot.  Returns the number of
        rows.  flexlibrary.py:2755-2892."""
        import csv
        if discard_invalid:
            raise DeprecationWarning("discard_invalid is deprecated. Use discard_invalid_traces() functions")
        btcp = self.binary_trace_categories_photometry(method=photometry_method, interpolate=not save_averages,
                                                       discard_invalid=discard_invalid, ignore_invalid_fields=ignore_invalid_fields,
                                                       adjustment_function=adjustment_function, **kwargs)
        rows = 0
        with open(filepath, 'w') as output_file:
            writer = csv.writer(output_file, dialect=dialect)
            n_frames = None if save_averages else len(list(self.experimental_fields[0].channels.values())[0].peptide_frames)
            writer.writerow(_track_photometries_header(save_averages, n_frames))
            for chan, categories in btcp.items():
                for e, ex in categories.items():
                    for category, trace_photometries in ex.items():
                        for photometry in trace_photometries:
                            # (the placeholder is told by identity, as the reference does: an adjustment_function builds new
                            #  tuples, and then the first frame's entry is taken whatever it holds, flexlibrary.py:2872-2874)
                            h, w = [fp[:2] for fp in photometry if fp is not _NONE3][0]
                            writer.writerow(_track_photometries_row(chan, e, h, w, category, [fp[2] for fp in photometry],
                                                                    save_averages))
                            rows += 1
        return rows

    def count_binary_trace_categories(self, ignore_invalid_fields=False):
        merged = self.binary_trace_categories(ignore_invalid_fields=ignore_invalid_fields)
        counts = {c: {e: {k: len(v) for k, v in ex.items()} for e, ex in chan.items()} for c, chan in merged.items()}
        return counts, merged

    def filtered_binary_trace_category_counts(self, include_first_frame_only=True, ignore_invalid_fields=False):
        """Counts of the patterns with a single ON -> OFF transition; include_first_frame_only=False leaves out the
        pattern that is ON in the first frame only.  flexlibrary.py:2911-2946."""
        counts, merged = self.count_binary_trace_categories(ignore_invalid_fields=ignore_invalid_fields)
        return {c: {e: _filtered_counts(ex, include_first_frame_only) for e, ex in chan.items()} for c, chan in counts.items()}

    def category_counts_as_csv(self, filepath, filtered=True, collate_fields=False, dialect='excel',
                               ignore_invalid_fields=False):
        """Pattern, (Field,) Channel, Count rows of filtered_binary_trace_category_counts; patterns and channels sorted,
        fields summed unless collate_fields.  Returns filepath.  flexlibrary.py:2948-3024."""
        if filtered:
            to_save = self.filtered_binary_trace_category_counts(ignore_invalid_fields=ignore_invalid_fields)
        else:
            to_save = self.count_binary_trace_categories(ignore_invalid_fields=ignore_invalid_fields)
        return _write_category_counts_csv(filepath, to_save, collate_fields, dialect)

    def category_counts_as_string(self, filtered=True, collate_fields=False, ignore_invalid_fields=False):
        """The filtered counts as a multi-line string.  flexlibrary.py:3026-3077."""
        if not filtered:
            raise NotImplementedError("filtered=False not yet implemented.")
        to_string = self.filtered_binary_trace_category_counts(ignore_invalid_fields=ignore_invalid_fields)
        return _category_counts_string(to_string, collate_fields)

    def _summed(self, name, ignore_invalid_fields):
        count = {}
        for e, ex in self._fields(ignore_invalid_fields):
            for c, num in getattr(ex, name)().items():
                count[c] = count.get(c, 0) + num
        return count

    def count_discarded_spots(self, ignore_invalid_fields=False):
        return self._summed('count_discarded_spots', ignore_invalid_fields)

    def spot_count(self, ignore_invalid_fields=False):
        return self._summed('spot_count', ignore_invalid_fields)

    def trace_count(self, ignore_invalid_fields=False):
        return self._summed('trace_count', ignore_invalid_fields)

    def singleton_count(self, ignore_invalid_fields=False):
        return self._summed('singleton_count', ignore_invalid_fields)

    def get_offsets(self, ignore_invalid_fields=False):
        return {e: ex.get_offsets() for e, ex in self._fields(ignore_invalid_fields)}

    def get_offsets_by_frame(self, ignore_invalid_fields=False):
        """{frame: {field: {channel: (d_h, d_w)}}}.  flexlibrary.py:3142-3157."""
        by_frame = {}
        for e, ex_offsets in self.get_offsets().items():
            if ignore_invalid_fields and not self.invalid_fields_mask[e]:
                continue
            for c, chan_offsets in ex_offsets.items():
                for f, frame_offset in enumerate(chan_offsets):
                    by_frame.setdefault(f, {}).setdefault(e, {}).setdefault(c, (frame_offset[0], frame_offset[1]))
        return by_frame

    def save_offsets_as_dict(self, filename, ignore_invalid_fields=False):
        import pickle
        with open(filename, 'wb') as f:
            pickle.dump(self.get_offsets_by_frame(ignore_invalid_fields=ignore_invalid_fields), f)

    def offsets_as_string(self, ignore_invalid_fields=False):
        """get_offsets_by_frame as text, with mean and standard deviation per field and per frame.  flexlibrary.py:3168-3201
        (the labels of the per-frame lines are the reference's)."""
        return _offsets_string(self.get_offsets_by_frame(ignore_invalid_fields=ignore_invalid_fields))


    def discard_invalid_traces(self, ignore_invalid_fields=False, **pparams):
        seqs = self._sequences(ignore_invalid_fields)
        return self._per_field(seqs, _discard_invalid_traces([chan for _, _, chan in seqs], pparams), ignore_invalid_fields)

    def multiplicative_delta_median_adjustments(self, tag='mdma', method='mexican_hat', channels=None,
                                                ignore_invalid_fields=False, **kwargs):
        seqs = self._sequences(ignore_invalid_fields)           # (`channels` is not passed on, flexlibrary.py:3215-3218)
        return self._per_field(seqs, _mdma([chan for _, _, chan in seqs], tag, method, kwargs), ignore_invalid_fields)

    def count_remainders(self, ignore_invalid_fields=False):
        return [ex.count_remainders() if not (ignore_invalid_fields and not self.invalid_fields_mask[e]) else False
                for e, ex in enumerate(self.experimental_fields)]

    def remainder_threshold_fields(self, channels=None, min_remainders=5):
        """Marks the fields that have fewer than min_remainders remainders in one of the channels (all of them, or those
        named) as invalid; returns self.invalid_fields_mask.  flexlibrary.py:3231-3263."""
        for e, counts in enumerate(self.count_remainders(ignore_invalid_fields=True)):
            if counts is False:
                continue
            if any(n < min_remainders for c, n in counts.items() if channels is None or c in channels):
                self.invalid_fields_mask[e] = False
        return self.invalid_fields_mask


from .stepfitting import PhotometryTrace, PlateauTrace, Trace  # noqa: E402  (flexlibrary.py:1320-1662; re-exported here)


class SimpleTrace(Trace):
    """A Trace that is a list of Spots (or None) through frames (flexlibrary.py:1536-1593); (h, w) is that of the first
    non-None Spot."""

    def __init__(self, trace):
        self.trace = trace
        for spot in trace:
            if spot is not None:
                self.h, self.w = spot.h, spot.w
                break
        else:
            raise Exception("flexlibrary.Trace.trace_hw: this Trace is composed entirely of None's.")
        self.num_frames = len(trace)

    def photometry(self, frame, photometry_method='mexican_hat', **kwargs):
        """The photometry of the Spot in frame; the int 0 where the trace has none."""
        spot = self.trace[frame]
        return 0 if spot is None else spot.photometry(method=photometry_method, **kwargs)

    def coordinates(self, frame):
        spot = self.trace[frame]
        return (None, None) if spot is None else (spot.h, spot.w)

    def plateau_starts(self):
        return set(range(self.num_frames))


def _spot_photometries(frames, traces, photometry_method, kwargs):
    """trace.photometry(f) for every frame of every SimpleTrace / PhotometryTrace, one list per trace (the int 0 for a None Spot).
    The mexican-hat photometries of all Spots that lie in `frames` come from one fsq_mexican_hat call."""
    from . import photometry as _ph
    index = {id(frame): f for f, frame in enumerate(frames or [])}
    rows, fhw, where = [], [], []
    batch = photometry_method == 'mexican_hat' and not set(kwargs) - {"brim_size", "radius", "return_invalid"} and \
        kwargs.get("return_invalid", True) and kwargs.get("radius", 9) is not None
    for t, trace in enumerate(traces):
        if isinstance(trace, PhotometryTrace):
            rows.append([trace.photometry(f) for f in range(trace.num_frames)])
            continue
        if not isinstance(trace, SimpleTrace):
            raise NotImplementedError("spot traces must be SimpleTrace or PhotometryTrace objects")
        row = []
        for f, spot in enumerate(trace.trace):
            if spot is None:
                row.append(0)
            elif batch and isinstance(spot, Spot) and id(spot.parent_Image) in index:
                fhw.append((index[id(spot.parent_Image)], spot.h, spot.w))
                where.append((t, f))
                row.append(None)
            else:
                row.append(spot.photometry(method=photometry_method, **kwargs))
        rows.append(row)
    if fhw:
        stack = np.stack([np.asarray(fr.image) for fr in frames])
        phot = _ph.mexican_hat_photometry_metric(stack, np.asarray(fhw, np.int64).reshape(-1, 3), kwargs.get("brim_size", 6),
                                                 kwargs.get("radius", 9))
        for (t, f), v in zip(where, phot):
            rows[t][f] = v
    return rows


class TimetraceExperiment(Experiment):
    """One field of view filmed continuously (flexlibrary.py:3266-3307): frames (Images), spot_traces (SimpleTraces),
    step_fits {(h, w): PlateauTrace} and step_fit_intermediates {(h, w): {name: Trace}}."""

    def __init__(self, frames, spot_traces=None, step_fits=None, step_fit_intermediates=None):
        self.frames = frames
        self.spot_traces = spot_traces
        self.step_fits = step_fits
        self.step_fit_intermediates = {} if step_fit_intermediates is None else step_fit_intermediates

    def lc_create_traces(self, initial_spots=None, search_radius=3.0, s_n_cutoff=3.0):
        """Tracks initial_spots (default: the Spots of the first frame) through the frames from theirs on by luminosity
        centroid (flexlibrary.py:3309-3384, fsq_centroid_tracking).  Returns the new self.spot_traces."""
        first_index = None
        if initial_spots is not None:
            parent = initial_spots[0].parent_Image if len(initial_spots) else None
            for f, frame in enumerate(self.frames):
                if parent is not None and frame is parent:
                    first_index = f
                    break
            else:
                raise ValueError("All initial_spots must have the same parent_image, and it must be one of the frames in "
                                 "this experiment.")
        elif self.frames[0].spots is not None:
            initial_spots, first_index = self.frames[0].spots, 0
        else:
            raise ValueError("Cannot create traces unless either the first frame does has Spots, or initial_spots are "
                             "specified via argument.")
        if not all(s.parent_Image is self.frames[first_index] for s in initial_spots):
            raise ValueError("All initial_spots must have the same parent_image, and it must be one of the frames in this "
                             "experiment.")
        raw = Experiment.luminosity_centroid_particle_tracking(self.frames[first_index:], initial_spots,
                                                               search_radius=search_radius, s_n_cutoff=s_n_cutoff)
        for trace in raw:
            for spot in trace[1:]:                   # (the initial Spots already belong to their Image)
                if spot is None:
                    continue
                if spot.parent_Image.spots is None:
                    spot.parent_Image.spots = []
                spot.parent_Image.spots.append(spot)
        self.spot_traces = [SimpleTrace(trace) for trace in raw]
        return self.spot_traces

    def stepfit_tracks(self, photometry_min=None, photometry_method='mexican_hat', mirror_start=0, chung_kennedy=0,
                       p_threshold=0.01, **kwargs):
        """Step fit of every track's photometries (flexlibrary.py:3449-3530): all mexican-hat photometries in one
        fsq_mexican_hat call, all traces in one fsq_stepfit_traces call.  Returns and stores (step_fits,
        step_fit_intermediates), keyed by each track's (h, w); raises if two tracks share one."""
        from . import photometry as _ph
        from . import stepfitting as _sf
        if photometry_method != 'mexican_hat':
            raise NotImplementedError("stepfit_tracks: only photometry_method='mexican_hat' is built")
        unknown = set(kwargs) - {"brim_size", "radius", "return_invalid"}
        if unknown or not kwargs.get("return_invalid", True):
            raise NotImplementedError("stepfit_tracks: unsupported photometry arguments %s" % sorted(unknown or ["return_invalid"]))
        brim_size, radius = kwargs.get("brim_size", 6), kwargs.get("radius", 9)
        traces = list(self.spot_traces or [])
        keys = []
        for trace in traces:
            if (trace.h, trace.w) in keys:
                raise Exception("Two tracks have initial Spots with identical (h, w).")
            keys.append((trace.h, trace.w))
        if not traces:
            self.step_fits = {}
            return self.step_fits, self.step_fit_intermediates
        index = {id(frame): f for f, frame in enumerate(self.frames)}
        fhw, where = [], []
        for t, trace in enumerate(traces):
            for f, spot in enumerate(trace.trace):
                if spot is not None:
                    fhw.append((index[id(spot.parent_Image)], spot.h, spot.w))
                    where.append((t, f))
        stack = np.stack([np.asarray(fr.image) for fr in self.frames])
        phot = _ph.mexican_hat_photometry_metric(stack, np.asarray(fhw, np.int64).reshape(-1, 3), brim_size, radius)
        rows = [[0.0] * trace.num_frames for trace in traces]          # (a None Spot's photometry is 0)
        for (t, f), v in zip(where, phot.tolist()):
            rows[t][f] = v
        # (photometry_min is accepted and not handed on: the reference's stepfit_tracks drops it on the way to
        # Trace.stepfit_photometries, flexlibrary.py:3499-3508, and its recorded CSV shows unclamped fits - DESIGN.md 4.13)
        fits = _sf.stepfit_photometries(rows, mirror_start=mirror_start, chung_kennedy=chung_kennedy, p_threshold=p_threshold,
                                        photometry_min=None, keys=keys)
        step_fits = {}
        for trace, key, (ph, ck, pl, tf) in zip(traces, keys, fits):
            if any(spot is None for spot in trace.trace):
                # (Trace.photometries counts a None Spot as the int 0; unfiltered it reaches the CSV as '0')
                ph.trace = tuple(0 if spot is None else v for spot, v in zip(trace.trace, ph.trace))
                if chung_kennedy == 0:
                    ck.trace = [0 if spot is None else v for spot, v in zip(trace.trace[trace.num_frames - len(ck.trace):], ck.trace)]
            step_fits[key] = tf
            self.step_fit_intermediates.setdefault(key, {}).update(
                {'photometries': ph, 'ck_filtered_photometries': ck, 'plateaus': pl, 't_filtered_plateaus': tf})
        self.step_fits = step_fits
        return self.step_fits, self.step_fit_intermediates

    def _get_all_intermediates(self):
        """The set of intermediates every trace has (flexlibrary.py:3538-3548); raises unless all traces have the same."""
        key_sets = [set(d.keys()) for d in self.step_fit_intermediates.values()]
        first = key_sets.pop()
        if not all(first == k for k in key_sets):
            raise Exception("All traces must have identical intermediates.")
        return first

    def save_experiment_as_csv(self, output_path, dialect='excel', include_step_fits=False, photometry_method='mexican_hat',
                               include_intermediates=None, **kwargs):
        """spot_traces, step_fits and step_fit_intermediates as one CSV, a row per trace and frame (flexlibrary.py:3550-3709);
        returns the number of rows written including the header.

        All mexican-hat photometries come from one fsq_mexican_hat call, and the plateau of every frame, `Step #` and R^2 of
        all traces from one fsq_timetrace_table call (timetrace.py); PlateauTrace intermediates are expanded
        by fsq_plateau_values.  Everything is validated before the file is opened: where the reference raises halfway and
        leaves a truncated file, this raises the same exception type and writes nothing.  Strings are made once per
        plateau; floats are Python 2's str(), as pflib.save_psfs_csv writes them.  Step fits and PlateauTrace intermediates
        must be consecutive plateaus from frame 0 (ValueError otherwise)."""
        import csv
        from . import timetrace as _tt
        from .pflib import _py2_str
        traces = list(self.spot_traces)
        if include_intermediates is True:
            include_intermediates = list(self._get_all_intermediates())
        if include_intermediates is not None:
            include_intermediates = sorted(include_intermediates)
        header = list(_tt.HEADER) + (_tt.STEP_FIT_HEADER if include_step_fits else []) + \
            [str(i) for i in (include_intermediates or [])]
        inter = [self.step_fit_intermediates[(trace.h, trace.w)] for trace in traces]        # (KeyError as in the reference)
        phot = _spot_photometries(self.frames, traces, photometry_method, kwargs)
        fits = []
        if include_step_fits and traces:
            fits = [self.step_fits[(trace.h, trace.w)] for trace in traces]
            if not all(isinstance(sf, PlateauTrace) for sf in fits):
                raise NotImplementedError("step fits must be PlateauTrace objects")
            table = _tt.timetrace_table(phot, [sf.trace for sf in fits])
        columns = []                                               # per intermediate: per trace a function frame -> cell
        for name in include_intermediates or []:
            objs = [d[name] for d in inter]
            plateau_like = [t for t, o in enumerate(objs) if isinstance(o, PlateauTrace)]
            if not all(isinstance(o, (PlateauTrace, PhotometryTrace)) for o in objs):
                raise NotImplementedError("intermediates must be PhotometryTrace or PlateauTrace objects")
            index = {}
            if plateau_like:
                torch = _engine._torch()
                for t in plateau_like:
                    if objs[t].num_frames != traces[t].num_frames:
                        raise ValueError("intermediate %r of trace %d does not cover the trace's frames" % (name, t))
                mf = max(traces[t].num_frames for t in plateau_like)
                rows = _tt.plateau_rows([objs[t].trace for t in plateau_like], mf)
                out = _tt.plateau_values_device(*(torch.from_numpy(a).cuda() for a in rows), want_index=True)
                status, idx = out["status"].cpu().numpy(), out["index"].cpu().numpy()
                if status.any():
                    raise ValueError("intermediate %r of trace %d: plateaus must be consecutive from frame 0" %
                                     (name, plateau_like[int(np.flatnonzero(status)[0])]))
                index = {t: idx[i] for i, t in enumerate(plateau_like)}
            cells = []
            for t, o in enumerate(objs):
                if t in index:
                    text = [_py2_str(p[2]) for p in o.trace]
                    cells.append([text[k] for k in index[t][:traces[t].num_frames].tolist()])
                else:
                    text = [_py2_str(v) for v in o.trace]
                    cells.append([text[min(f, len(text) - 1)] for f in range(traces[t].num_frames)])
            columns.append(cells)
        rows_written = 1
        with open(output_path, 'w', newline='') as f:
            wr = csv.writer(f, dialect=dialect)
            wr.writerow(header)
            for t, trace in enumerate(traces):
                base = [str(t), str(trace.h), str(trace.w)]
                n = trace.num_frames
                if include_step_fits:
                    heights = [_py2_str(p[2]) for p in fits[t].trace]
                    r2 = _py2_str(float(table["r2"][t]))
                    k_row, s_row = table["plateau_index"][t, :n].tolist(), table["step_num"][t, :n].tolist()
                    l_row = table["plateau_length"][t, :n].tolist()
                for fi in range(n):
                    v = phot[t][fi]
                    row = base + [str(fi), repr(float(v)) if isinstance(v, (float, np.floating)) else str(v)]
                    if include_step_fits:
                        sn = s_row[fi]
                        row += ['None' if sn < 0 else str(sn), heights[k_row[fi]], 'None' if sn < 0 else heights[sn], str(l_row[fi]), r2]
                    row += [cells[t][fi] for cells in columns]
                    wr.writerow(row)
                rows_written += n
        return rows_written

    def save_traces_pkl(self, path):
        """self.spot_traces as a protocol-0 pickle (flexlibrary.py:3711-3713), written as the project's other pickles."""
        from . import pflib as _pf
        with open(path, 'wb') as f:
            f.write(_pf._py2_pickle_bytes(self.spot_traces))

    def wildcolor_plot_tracks(self, filepath_prefix, color_list=('red', 'blue', 'yellow', 'purple', 'orange', 'pink', 'lightblue',
                                                                 'green'), num_colors=8):
        """One PNG per frame with a square on every track's Spot, a random colour per track (flexlibrary.py:3384-3447):
        filepath_prefix + the zero-filled frame index + '.png', through pflib.save_psfs_png.  Returns the paths."""
        import math
        import random
        from . import pflib as _pf
        saved = []
        if self.spot_traces is None:
            return tuple(saved)
        colors = {t: random.choice(color_list[:num_colors]) for t, _ in enumerate(self.spot_traces)}
        zfill = int(np.ceil(math.log(len(self.frames), 10)))
        for f, frame in enumerate(self.frames):
            psfs, square_colors = {}, {}
            for t, track in enumerate(self.spot_traces):
                h, w = track.coordinates(f)
                if h is None or w is None:
                    continue
                psfs.setdefault((h, w), tuple([0] * 12))
                square_colors.setdefault((h, w), colors[t])
            saved.append(_pf.save_psfs_png(psfs=psfs, image_path=frame.metadata['filepath'], timestamp_epoch=None,
                                           output_path=filepath_prefix + str(f).zfill(zfill) + '.png', square_size=9,
                                           square_color=None, square_colors=square_colors))
        return tuple(saved)
