#!/usr/bin/env python3
"""
A fluorosequencing experiment from its image files to category counts and track photometries, on an MI355X GPU.

Images are grouped by directory: every directory is one experimental cycle (directories in alphanumeric order), the sorted
file names of a directory are its fields of view.  Images without a `<image>*_psfs_*.pkl` next to them are fitted through
pflib.parallel_image_batch (which writes the per-image pkl / csv / png files); images that have one are not fitted again.  The
Spots are loaded from the pkl files, consecutive cycles are registered by phase correlation, Spots are tracked across cycles,
holes are filled in, photometries measured and ON/OFF categories counted - all of it after the loading in one call of
experiment.sequence_experiment_records.  The output directory receives

    category_stats_<hash>.pkl, filtered_stats_<hash>.pkl    counts per channel, field and ON/OFF pattern
    category_counts_<hash>.csv                              the filtered counts as a table
    track_photometries[_NO_NONES]_<hash>.csv                one row per track
    offsets_dict_<hash>.pkl                                 stage drift per frame, field and channel

and the summary is printed.  Drop-in for the reference's basic_experiment_script.py (:70-644: same options, same flow, same
files):
    python -m fluorosequencingimageanalysis_amd.basic_experiment_script [options] --peptide_files IMAGE [IMAGE ...]

Not built (NotImplementedError before any work is done): --recompute and --all_categories (the reference raises for them
too), --save_tracks (extract_tracks samples without a seed), --pkl_invalid, --sextractor, and sanity check images: pass
--no_sanity_check_images.
"""
import argparse
import ast
import datetime
import glob
import logging
import multiprocessing
import os
import pickle
import sys
import time

import numpy as np

from . import experiment, flexlibrary, pflib


class _Formatter(argparse.ArgumentDefaultsHelpFormatter, argparse.RawDescriptionHelpFormatter):
    pass


def build_parser(timestamp_datetime):
    """The reference's command line (basic_experiment_script.py:70-219)."""
    p = argparse.ArgumentParser(description=__doc__, formatter_class=_Formatter)
    p.add_argument('-D', '--debug', action='store_true', default=False, help="Log debugging output.")
    p.add_argument('-n', '--num_processes', type=int, nargs=1, default=[multiprocessing.cpu_count()],
                   help="Number of host processes that read the images and write the per-image files.")
    default_log = os.path.join('/home', 'basic_experiment_script_' + str(timestamp_datetime) + '.log')
    p.add_argument('-L', '--log_path', nargs=1, default=[default_log], help="Log file (appended to when it exists).")
    p.add_argument('--output_directory', nargs=1, default=None,
                   help="All output files are saved to this directory; use a fresh one, existing files may be overwritten.")
    p.add_argument('-r', '--recompute', action='store_true', default=False, help="Recompute peak fitting on the images (not implemented).")
    p.add_argument('--keep_invalid', action='store_true', default=False,
                   help="Keep tracks that leave the field of view or come too close to the edge for the photometry requested. "
                        "Without it those tracks are discarded and the photometries are saved as track_photometries_NO_NONES_<hash>.csv.")
    p.add_argument('--pkl_invalid', action='store_true', default=False, help="Save the discarded tracks as a pkl file (not built).")
    p.add_argument('-ns', '--no_self_align', action='store_true', default=False,
                   help="Do not use peptide_files as alignment frames when alignment_files is not given: no alignment is performed.")
    p.add_argument('--no_sanity_check_images', action='store_true', default=False, help="Don't make sanity check images (required here).")
    p.add_argument('-en', '--extraction_number', type=int, default=10, help="Tracks to extract per pattern (with --save_tracks).")
    p.add_argument('-es', '--extraction_size', type=int, default=9, help="Side of the extracted track images; odd (with --save_tracks).")
    p.add_argument('--save_tracks', action='store_true', default=False, help="Save tracks to pkl files and PNGs (not built).")
    p.add_argument('--sextractor', action='store_true', default=False, help="Use sextractor photometry algorithm (not built).")
    p.add_argument('--photometry_parameters', type=str, nargs=1, default=[None],
                   help="Keyword arguments of Spot.photometry as a quoted Python dict literal, e.g. --photometry_parameters=\""
                        "{'photometry_method': 'mexican_hat', 'brim_size': 4, 'radius': 5}\"; whatever is not named keeps its default.")
    p.add_argument('--save_photometries', action='store_true', default=True, help="Save tracks' photometries as csv file.")
    p.add_argument('--not_all_photometries', action='store_true', default=False,
                   help="Save only the average photometry of a track's found Spots; by default every frame's photometry is "
                        "saved, with holes filled in by interpolation between found Spots.")
    p.add_argument('--collate_fields', action='store_true', default=False, help="Collate data by fields in CSV and string output.")
    p.add_argument('--all_categories', action='store_true', default=False, help="Print all category combinations (not implemented).")
    p.add_argument('--alignment_files', nargs='+', type=str, default=None, required=False,
                   help="Images of the alignment channel, grouped like peptide_files: one for every peptide image.")
    p.add_argument('--peptide_files', nargs='+', type=str, required=True,
                   help="Images of the peptide channel: every directory is one cycle, its sorted file names are the fields.")
    p.add_argument('--second_channel', nargs='+', type=str, default=None,
                   help="Images of the second peptide channel, grouped like peptide_files: one for every peptide image.")
    return p


def refuse_unsupported(args):
    """The options that end the run before any work is done."""
    if args.recompute:
        raise NotImplementedError("--recompute option not currently implemented.")
    if args.all_categories:
        raise NotImplementedError("--all_categories option not currently implemented.")
    if args.save_tracks:
        raise NotImplementedError("--save_tracks is not built: extract_tracks samples the tracks without a seed.")
    if args.pkl_invalid:
        raise NotImplementedError("--pkl_invalid is not built.")
    if not args.no_sanity_check_images:
        raise NotImplementedError("sanity check images (plot_traces) are not built: pass --no_sanity_check_images.")
    if args.sextractor:
        raise NotImplementedError("--sextractor: the sextractor photometry is not built.")


def fit_unfitted(paths, timestamp_epoch, num_processes, logger):
    """basic_experiment_script.py:240-257: the images without a PSF pkl go through pflib; their converted paths take their place."""
    need_fitting, need_fitting_map = [], {}
    for f, fullpath in enumerate(paths):
        if len(sorted(glob.glob(fullpath + '*_psfs_*.pkl'))) == 0:
            need_fitting.append(fullpath)
            need_fitting_map.setdefault(fullpath, f)
    logger.info("Could not find PSF pkl files for these images; they will be submitted to pflib: " + str(need_fitting))
    processed = pflib.parallel_image_batch(image_paths=need_fitting, find_peptides_parameters=None, timestamp_epoch=timestamp_epoch,
                                           num_processes=num_processes)
    for original_path, (converted_path, _, _, _) in processed.items():
        paths[need_fitting_map[original_path]] = converted_path
    return paths


def load_fields(field_indexed_files, what, logger, load_psfs=True):
    """{field: [Image per cycle]} through easy_load_processed_image (:376-413)."""
    fields = {}
    for field, files in field_indexed_files.items():
        fields.setdefault(field, [])
        for f in files:
            image_object, discarded_spots = flexlibrary.Experiment.easy_load_processed_image(f, load_psfs=load_psfs)
            if discarded_spots > 0:
                logger.info("For file " + str(f) + " in " + what + ", discarded " + str(discarded_spots) + " Spots.")
            fields[field].append(image_object)
    return fields


def main(argv=None):
    timestamp_epoch = time.time()
    timestamp_datetime = datetime.datetime.fromtimestamp(timestamp_epoch)
    epoch_hash = pflib._epoch_to_hash(timestamp_epoch)
    args = build_parser(timestamp_datetime).parse_args(argv)
    refuse_unsupported(args)
    logging.basicConfig(filename=args.log_path[0], level=logging.DEBUG if args.debug else logging.INFO, force=True)
    logger = logging.getLogger()
    logger.info("basic_experiment_script starting at " + str(timestamp_datetime))
    logger.info("args = " + str(args))

    peptide_files = fit_unfitted([os.path.abspath(f) for f in args.peptide_files], timestamp_epoch, args.num_processes[0], logger)
    by_directory = {}
    for f in peptide_files:
        head, tail = os.path.split(f)
        by_directory.setdefault(head, []).append(tail)
    if len(set(len(tails) for tails in by_directory.values())) != 1:
        raise Exception("For peptide_files, each directory must have the same number of files specified.")
    frame_indexed_peptide_files, field_indexed_peptide_files = flexlibrary.Experiment.easy_sort_target_images(peptide_files)
    if args.alignment_files is not None:
        alignment_files = [os.path.abspath(f) for f in args.alignment_files]
    elif not args.no_self_align:
        alignment_files = [os.path.abspath(f) for f in args.peptide_files]
    else:
        alignment_files = []
    frame_indexed_alignment_files, field_indexed_alignment_files = flexlibrary.Experiment.easy_sort_target_images(alignment_files)
    if (args.alignment_files is not None and
            (set(frame_indexed_peptide_files.keys()) != set(frame_indexed_alignment_files.keys()) or
             not all(len(files) == len(frame_indexed_alignment_files[d]) for d, files in frame_indexed_peptide_files.items()))):
        raise Exception("Alignment files given, but not every peptide image file has one.")
    if args.second_channel is not None:
        second_channel_files = fit_unfitted([os.path.abspath(f) for f in args.second_channel], timestamp_epoch,
                                            args.num_processes[0], logger)
    else:
        second_channel_files = []
    frame_indexed_second_channel_files, field_indexed_second_channel_files = \
        flexlibrary.Experiment.easy_sort_target_images(second_channel_files)
    # (as the reference, :317-328: the second channel's grouping is compared with itself)
    if (args.second_channel is not None and
            (set(frame_indexed_second_channel_files.keys()) != set(frame_indexed_second_channel_files.keys()) or
             not all(len(files) == len(frame_indexed_second_channel_files[d])
                     for d, files in frame_indexed_second_channel_files.items()))):
        raise Exception("Second channel files given, but not every peptide image file has one.")
    for name, value in (("frame_indexed_peptide_files", frame_indexed_peptide_files),
                        ("field_indexed_peptide_files", field_indexed_peptide_files),
                        ("frame_indexed_alignment_files", frame_indexed_alignment_files),
                        ("field_indexed_alignment_files", field_indexed_alignment_files),
                        ("frame_indexed_second_channel_files", frame_indexed_second_channel_files),
                        ("field_indexed_second_channel_files", field_indexed_second_channel_files)):
        logger.info(name + " " + str(value))

    # (as the reference, :342: --output_directory is dereferenced before its None check at :460)
    output_directory = os.path.abspath(args.output_directory[0])
    if not os.path.exists(output_directory):
        os.makedirs(output_directory)

    peptide_fields = load_fields(field_indexed_peptide_files, "peptide_fields", logger)
    alignment_fields = load_fields(field_indexed_alignment_files, "alignment_fields", logger, load_psfs=False)
    second_channel_fields = load_fields(field_indexed_second_channel_files, "second_channel_fields", logger)

    # everything from here to the counts in one call: frames [fields, channels, F, H, W] and the Spot tables of the pkl files
    channel_fields = [peptide_fields] + ([second_channel_fields] if len(second_channel_fields) > 0 else [])
    fields = list(peptide_fields.keys())
    frames = np.stack([np.stack([np.stack([np.asarray(im.image) for im in chan[field]]) for chan in channel_fields])
                       for field in fields])
    spots = [[[np.array([(s.h, s.w) for s in im.spots]).reshape(-1, 2) for im in chan[field]] for chan in channel_fields]
             for field in fields]
    if len(alignment_fields) > 0:
        alignment_frames = np.stack([np.stack([np.asarray(im.image) for im in alignment_fields[field]]) for field in fields])
    else:
        alignment_frames = None        # (the reference indexes alignment_fields[field] all the same, :430; here: no alignment)
    if args.photometry_parameters[0] is not None:
        p_params = ast.literal_eval(args.photometry_parameters[0])
    else:
        p_params = {}
    output_directory = args.output_directory[0]
    records = experiment.sequence_experiment_records(frames, alignment_frames=alignment_frames, self_align=False, spots=spots,
                                                     keep_invalid=args.keep_invalid, **p_params)

    category_stats = experiment.category_stats(records)
    filtered_stats = experiment.category_stats(records, filtered=True, include_first_frame_only=True)
    for name, stats in (("category_stats_", category_stats), ("filtered_stats_", filtered_stats)):
        with open(os.path.join(output_directory, name + str(epoch_hash) + '.pkl'), 'wb') as f:
            f.write(pflib._py2_pickle_bytes(stats))
    experiment.write_category_counts_csv(os.path.join(output_directory, 'category_counts_' + str(epoch_hash) + '.csv'), records,
                                         collate_fields=args.collate_fields)
    if args.save_photometries:
        name = 'track_photometries_' if args.keep_invalid else 'track_photometries_NO_NONES_'
        experiment.write_track_photometries_csv(os.path.join(output_directory, name + str(epoch_hash) + '.csv'), records,
                                                save_averages=args.not_all_photometries)
    summary = experiment.summary_text(records, save_averages=args.not_all_photometries or not args.save_photometries,
                                      collate_fields=args.collate_fields)
    sys.stdout.write(summary)
    with open(os.path.join(output_directory, 'offsets_dict_' + str(epoch_hash) + '.pkl'), 'wb') as f:
        pickle.dump(experiment.offsets_by_frame(records), f)
    return records


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
