#!/usr/bin/env python3
"""
Step fitting of one continuously filmed field of view, on an MI355X GPU.

The frames are given in chronological order.  The Spots of the first frame are read from the PSF pickle pflib wrote for it
(`<frame0>*_psfs_*.pkl`), or the first frame is fitted through pflib.parallel_image_batch when there is none; every Spot is
tracked through the frames by luminosity centroid, its photometry is measured in every frame, steps are fitted to the
photometry traces, and the output directory receives

    test_<frame index>.png   one sanity image per frame with a square on every tracked Spot (unless --no_sanity_check_images)
    test.pkl                 (step_fits, step_fit_intermediates)
    test.csv                 one row per trace and frame: photometry, step fit, R^2 and all intermediates
    traces.pkl               the traces themselves (with --save_traces_pkl)

Drop-in for the reference's basic_timetrace_script.py (:32-283: same options, same flow, same files):
    python -m fluorosequencingimageanalysis_amd.basic_timetrace_script [options] FRAME [FRAME ...]
"""
import argparse
import ast
import datetime
import glob
import logging
import os
import pickle
import sys
import time

from . import flexlibrary, pflib


class _Formatter(argparse.ArgumentDefaultsHelpFormatter, argparse.RawDescriptionHelpFormatter):
    pass


def build_parser(timestamp_datetime):
    """The reference's command line (basic_timetrace_script.py:38-153)."""
    p = argparse.ArgumentParser(description=__doc__, formatter_class=_Formatter)
    p.add_argument('-D', '--debug', action='store_true', default=False, help="Log debugging output.")
    default_log = os.path.join('/home', 'basic_timetrace_script_' + str(timestamp_datetime) + '.log')
    p.add_argument('-L', '--log_path', nargs=1, default=[default_log], help="Log file (appended to when it exists).")
    p.add_argument('--output_directory', nargs=1, default=[os.getcwd()],
                   help="All output files are saved to this directory; use a fresh one, existing files are overwritten.")
    p.add_argument('--no_sanity_check_images', action='store_true', default=False, help="Don't make sanity check images.")
    p.add_argument('--save_traces_pkl', action='store_true', default=False, help="Save the found traces to a pickle file.")
    p.add_argument('--sextractor', action='store_true', default=False,
                   help="Use sextractor photometry algorithm (not built here: stepfit_tracks raises NotImplementedError).")
    p.add_argument('--photometry_parameters', type=str, nargs=1, default=[None],
                   help="Keyword arguments of Spot.photometry as a quoted Python dict literal, e.g. "
                        "--photometry_parameters=\"{'brim_size': 4, 'radius': 5}\"; whatever is not named keeps its default.")
    p.add_argument('--photometry_minimum', type=float, nargs=1, default=[None],
                   help="If given, photometries below this value are raised to it before the step fit.")
    p.add_argument('--p_threshold', type=float, nargs=1, default=[0.01], help="p threshold of the t-tests that decide whether a step exists.")
    p.add_argument('--linear_fit_threshold', type=float, nargs=1, default=[1.0], help="Accepted and unused, as in the reference.")
    p.add_argument('--chung_kennedy', type=int, nargs=1, default=[0],
                   help="Number of times to apply the Chung-Kennedy filter to the photometries before fitting steps.")
    p.add_argument('--mirror_start', type=int, nargs=1, default=[0], help="Number of first frames to mirror.")
    p.add_argument('timetrace_frames', nargs='+', type=str, help="The frames of the time trace, in chronological order.")
    return p


def initial_spots(frame_image, frame_path, timestamp_epoch, logger):
    """The Spots of the first frame, from its PSF pickle or from a fresh fit (basic_timetrace_script.py:187-207)."""
    pkls = glob.glob(frame_path + '*_psfs_*.pkl')
    if len(pkls) == 0:
        logger.info("Could not find PSF pkl files for " + frame_path + "; it will be submitted to pflib.")
        processed = pflib.parallel_image_batch(image_paths=[frame_path], find_peptides_parameters=None,
                                               timestamp_epoch=timestamp_epoch)
        psfs_pkl_path = processed[frame_path][1]
    else:
        psfs_pkl_path = pkls[0]
    with open(psfs_pkl_path, 'rb') as f:
        psfs = pickle.load(f, encoding='latin1')
    return [flexlibrary.Spot(parent_Image=frame_image, h=int(pflib._py2_round(h_0)), w=int(pflib._py2_round(w_0)), size=fit[7].shape[0],
                             gaussian_fit=fit)
            for (h_0, w_0), fit in psfs.items()]


def main(argv=None):
    timestamp_epoch = time.time()
    timestamp_datetime = datetime.datetime.fromtimestamp(timestamp_epoch)
    args = build_parser(timestamp_datetime).parse_args(argv)
    logging.basicConfig(filename=args.log_path[0], level=logging.DEBUG if args.debug else logging.INFO, force=True)
    logger = logging.getLogger()
    logger.info("basic_timetrace_script starting at " + str(timestamp_datetime))
    logger.info("args = " + str(args))
    timetrace_frames = [os.path.abspath(f) for f in args.timetrace_frames]
    out_dir = args.output_directory[0]
    os.makedirs(out_dir, exist_ok=True)
    arrays = [pflib.read_image(f) for f in timetrace_frames]
    frame_images = [flexlibrary.Image(image=arrays[f][1], metadata={'filepath': frame}, spots=None)
                    for f, frame in enumerate(timetrace_frames)]
    frame_images[0].spots = initial_spots(frame_images[0], timetrace_frames[0], timestamp_epoch, logger)
    tte = flexlibrary.TimetraceExperiment(frames=frame_images, spot_traces=None, step_fits=None, step_fit_intermediates=None)
    tte.lc_create_traces()
    if not args.no_sanity_check_images:
        tte.wildcolor_plot_tracks(filepath_prefix=os.path.join(out_dir, 'test_'))
    if args.photometry_parameters[0] is not None:
        p_params = ast.literal_eval(args.photometry_parameters[0])
    else:
        p_params = {'photometry_method': 'sextractor'} if args.sextractor else {}
    step_fits, step_fit_intermediates = tte.stepfit_tracks(photometry_min=args.photometry_minimum[0],
                                                           mirror_start=args.mirror_start[0],
                                                           chung_kennedy=args.chung_kennedy[0],
                                                           p_threshold=args.p_threshold[0], **p_params)
    with open(os.path.join(out_dir, 'test.pkl'), 'wb') as f:
        f.write(pflib._py2_pickle_bytes((step_fits, step_fit_intermediates)))
    rows = tte.save_experiment_as_csv(output_path=os.path.join(out_dir, 'test.csv'), include_step_fits=True,
                                      include_intermediates=True, **p_params)
    if args.save_traces_pkl:
        tte.save_traces_pkl(path=os.path.join(out_dir, 'traces.pkl'))
    logger.info("basic_timetrace_script wrote %d rows; finished at %s" % (rows, datetime.datetime.now()))
    return tte


if __name__ == "__main__":
    try:
        main()
    except BaseException as e:      # noqa: BLE001
        if isinstance(e, SystemExit):
            raise
        import traceback
        traceback.print_exc()
        logging.getLogger().exception(e)
        logging.shutdown()
        sys.exit(1)
    sys.exit(0)
