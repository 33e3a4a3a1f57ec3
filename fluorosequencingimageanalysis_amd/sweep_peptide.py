"""Sweep the simulation of one labelled peptide over a grid of chemistry parameters on the GPU and score every point against
an experiment's observed signals: simulate_peptide.py once per point, collected and scored as jupyter_development.py's
match_diagnostic does, in one run.

  python -m fluorosequencingimageanalysis_amd.sweep_peptide SEQUENCE LABEL --observed SIGNALS.pkl
         --edman_efficiency LO:HI:N --dye_destruction LO:HI:N --dud_dyes LO:HI:N [options]

A range LO:HI:N is N evenly spaced values from LO to HI, both included; a single number is that value alone.  dye_destruction
is the rate per cycle, as in simulate_peptide.  SIGNALS.pkl holds the observed {(signal, is_zero, start): count}, or the
(args, signals, molecular_error_signals) that simulate_peptide writes.  The other options of simulate_peptide are taken with
their defaults.  Writes Sweep_<hash>.pkl, a pickle (protocol 2) of a dict: args, points (the (edman_efficiency,
dye_destruction, dud_dyes) triples in grid order), all_simulations {point: (signals, molecular_signals)}, total_count,
none_count, scores {point: (result, (normalization_factor, contributions))} and best_point (point, result,
normalization_factor, contributions); prints the best point and its score.  --incompatibility adds `diagnostic`,
signal_sweep.match_diagnostic's dict (the incompatibility scores of the heat-map signals over all their pairs, the signals
above --incompatibility_threshold united with those before --split_cycle as exclude_signals, the best point's counts scaled to
the observed total and the twelve heat-map tables), and prints the number of excluded signals and the five highest scores; it
needs --heatmap_normalize_counts, or --all_signals with --normalize_counts.  --host runs the NumPy twins; no GPU needed.

Several label letters (LABEL "KC", up to 4, one colour channel each) run signal_sweep's joint path: SIGNALS.pkl then holds
{(decrements, zeros, starts): count} of joint signals (python -m fluorosequencingimageanalysis_amd.joint_signals writes one
from a two-channel track table; signal_sweep.joint_signals_of_fits makes one from aligned fits), --fluor_intensity,
--beta_sigma, --superdye_rate and --superdye_factor take one number or K=..,C=.., and the pickle gains `labels`, the sorted
letters; `diagnostic` then has no heat-map tables.  One letter runs and writes what it did before."""
import argparse
import itertools
import os
import pickle
import sys
from datetime import datetime
from math import log
from time import time

import numpy as np

from . import _host_signal_sweep, peptide_simulator, signal_sweep
from .pflib import _epoch_to_hash
from .simulate_peptide import MAX_DEVIATION, MAX_POSSIBLE


def value_range(text):
    """'LO:HI:N' -> N evenly spaced floats from LO to HI; 'X' -> [X]."""
    parts = text.split(':')
    try:
        if len(parts) == 1:
            return [float(parts[0])]
        if len(parts) != 3:
            raise ValueError
        lo, hi, n = float(parts[0]), float(parts[1]), int(parts[2])
        if n < 1 or (n == 1 and lo != hi):
            raise ValueError
    except ValueError:
        raise argparse.ArgumentTypeError("%r is not LO:HI:N (N >= 1; LO = HI where N = 1) or a number" % text)
    return [float(x) for x in np.linspace(lo, hi, n)]


def per_letter(text):
    """'X' -> the float X; 'K=X,C=Y' -> {'K': X, 'C': Y}."""
    try:
        if '=' not in text:
            return float(text)
        out = {}
        for part in text.split(','):
            letter, value = part.split('=')
            if len(letter.strip()) != 1 or letter.strip() in out:
                raise ValueError
            out[letter.strip()] = float(value)
        return out
    except ValueError:
        raise argparse.ArgumentTypeError("%r is neither a number nor LETTER=NUMBER,LETTER=NUMBER" % text)


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('sequence', nargs=1, type=str, help="The peptide as a string of amino acids.")
    p.add_argument('labels', nargs=1, type=str, help="The labelled amino acid; several letters (up to 4): one colour each.")
    p.add_argument('--observed', required=True, help="Pickle of the observed signals.")
    p.add_argument('--edman_efficiency', type=value_range, default=[0.90], help="LO:HI:N or a number.")
    p.add_argument('--dye_destruction', type=value_range, default=[0.1], help="Rate per cycle: LO:HI:N or a number.")
    p.add_argument('--dud_dyes', type=value_range, default=[0.50], help="LO:HI:N or a number.")
    p.add_argument('-N', '--num_sims', type=int, default=100000, help="Number of molecules to simulate at every point.")
    p.add_argument('-m', '--num_mocks', type=int, default=4, help="Number of mocks performed.")
    p.add_argument('-o', '--num_mocks_omitted', type=int, default=1, help="Number of mocks not imaged.")
    p.add_argument('-e', '--num_edmans', type=int, default=8, help="Number of Edmans performed.")
    p.add_argument('--surface_degradation_1', type=float, default=0.30)
    p.add_argument('--surface_degradation_1_num_cycles', type=int, default=3)
    p.add_argument('--surface_degradation_2', type=float, default=0.10)
    p.add_argument('--fluor_intensity', type=per_letter, default=70000, help="Intensity of one fluor: a number, or K=..,C=..")
    p.add_argument('--ddif_2', type=float, default=0.30)
    p.add_argument('--ddif_3', type=float, default=0.30)
    p.add_argument('--beta_sigma', type=per_letter, default=0.20, help="A number, or K=..,C=..")
    p.add_argument('--no_multidrop', action='store_true', default=False, help="No drops of more than one dye in the fit.")
    p.add_argument('--superdye_rate', type=per_letter, default=0.0, help="A number, or K=..,C=..")
    p.add_argument('--superdye_factor', type=per_letter, default=1.0, help="A number, or K=..,C=..")
    p.add_argument('--output_directory', nargs=1, default=[os.getcwd()], help="Created if it does not exist.")
    p.add_argument('--metric', default='my_euclidean', choices=_host_signal_sweep.METRICS)
    norm = p.add_mutually_exclusive_group()
    norm.add_argument('--normalize_counts', action='store_true', default=False)
    norm.add_argument('--heatmap_normalize_counts', action='store_true', default=False)
    p.add_argument('--reverse_order', action='store_true', default=False, help="The largest score is the best (e.g. naive).")
    p.add_argument('--all_signals', action='store_true', default=False, help="Score beyond the heatmap (heatmap_only=False).")
    p.add_argument('--nonzero_signals', action='store_true', default=False, help="Score signals that do not end at zero (zero_only=False).")
    p.add_argument('--score_multidrop', action='store_true', default=False, help="Score signals with repeated drops (allow_multidrop).")
    p.add_argument('--small_count_cutoff', type=float, default=None)
    p.add_argument('--incompatibility', action='store_true', default=False, help="Add match_diagnostic's dict under 'diagnostic'.")
    p.add_argument('--incompatibility_threshold', type=float, default=None, help="Signals scoring above it are excluded.")
    p.add_argument('--split_cycle', type=int, default=0, help="Heat-map signals that end before this cycle are excluded.")
    p.add_argument('--molecule_stride', type=int, default=0, help="0: every point sees the same draws.")
    p.add_argument('--table_slots', type=int, default=1024, help="Distinct signals a point can hold: a power of two.")
    p.add_argument('--chunk_rows', type=int, default=1 << 22)
    p.add_argument('--seed', type=int, default=None, help="Seed of the draws, 0 .. 2^64 - 1 (default: a fresh one).")
    p.add_argument('--host', action='store_true', default=False, help="Run the NumPy twins; no GPU needed.")
    p.add_argument('--device', default=None, help="The torch device (default: cuda).")
    return p


def load_observed(path):
    with open(path, 'rb') as f:
        data = pickle.load(f, encoding='latin1')
    if isinstance(data, tuple) and len(data) == 3 and isinstance(data[1], dict):
        data = data[1]
    if not isinstance(data, dict):
        raise ValueError("%s holds neither a dict of signals nor simulate_peptide's tuple" % path)
    return data


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    joint = len(set(args.labels[0])) > 1
    if not joint and any(isinstance(getattr(args, k), dict) for k in ("fluor_intensity", "beta_sigma", "superdye_rate", "superdye_factor")):
        parser.error("LETTER=NUMBER values need several label letters")
    if args.incompatibility:                                     # (before the sweep is run, not after it)
        try:
            signal_sweep.check_diagnostic_options(args.normalize_counts, args.heatmap_normalize_counts, not args.all_signals,
                                                  args.score_multidrop, args.incompatibility_threshold, True)
        except ValueError as e:
            parser.error("--incompatibility: " + str(e))
    if args.seed is None:
        args.seed = peptide_simulator.fresh_seed()
    observed = load_observed(args.observed)
    output_directory = os.path.abspath(args.output_directory[0])
    if not os.path.exists(output_directory):
        os.makedirs(output_directory)
    output_filepath = os.path.join(output_directory, "Sweep_" + str(_epoch_to_hash(round(time()))) + ".pkl")
    ddif = [0, args.ddif_2] + [args.ddif_3] * 5
    grid = list(itertools.product(args.edman_efficiency, args.dye_destruction, args.dud_dyes))
    points = [(p, -log(1.0 - d), u) for p, d, u in grid]
    fixed = dict(s=args.surface_degradation_1, sc=args.surface_degradation_1_num_cycles, s2=args.surface_degradation_2,
                 beta=args.fluor_intensity, beta_sigma=args.beta_sigma, ddif=ddif, superdye_rate=args.superdye_rate,
                 superdye_factor=args.superdye_factor)
    print("Seed: " + str(args.seed))
    print("Parameters loaded. Sweeping " + str(len(grid)) + " points at " + str(datetime.now()))
    run = signal_sweep.joint_sweep_records if joint else signal_sweep.sweep_records
    sweep = run(args.sequence[0], args.labels[0], args.num_mocks - args.num_mocks_omitted, args.num_edmans, points, args.num_sims,
                seed=args.seed, molecule_stride=args.molecule_stride, max_possible=MAX_POSSIBLE, allow_multidrop=not args.no_multidrop,
                max_deviation=MAX_DEVIATION, quench_factors=ddif, table_slots=args.table_slots, chunk_rows=args.chunk_rows,
                device=args.device, host=args.host, **fixed)
    print("Sweep complete. Scoring at " + str(datetime.now()))
    scores = signal_sweep.score_records(observed, sweep, metric=args.metric, normalize_counts=args.normalize_counts,
                                        heatmap_normalize_counts=args.heatmap_normalize_counts,
                                        small_count_cutoff=args.small_count_cutoff, host=args.host, on_error='none', device=args.device,
                                        heatmap_only=not args.all_signals, zero_only=not args.nonzero_signals,
                                        allow_multidrop=args.score_multidrop)
    name = dict(zip(sweep["points"], grid))                      # the grid's triples in place of the simulator's (p, b, u)
    out = {"args": args, "points": grid,
           "all_simulations": {name[k]: v for k, v in sweep["all_simulations"].items()},
           "total_count": {name[k]: v for k, v in sweep["total_count"].items()},
           "none_count": {name[k]: v for k, v in sweep["none_count"].items()},
           "scores": {name[k]: v for k, v in scores.items()}}
    if joint:
        out["labels"] = sweep["labels"]
    out["best_point"] = signal_sweep.best_point(out["scores"], args.reverse_order)
    if args.incompatibility:
        print("Scoring the signal pairs at " + str(datetime.now()))
        named = {"points": grid, "all_simulations": out["all_simulations"]}
        if joint:
            named["labels"] = sweep["labels"]
        out["diagnostic"] = signal_sweep.match_diagnostic(
            named, observed, args.metric, args.reverse_order, args.normalize_counts, args.heatmap_normalize_counts,
            not args.all_signals, not args.nonzero_signals, args.score_multidrop, args.small_count_cutoff, 0.10, args.split_cycle,
            args.incompatibility_threshold, True, args.num_mocks, args.num_mocks_omitted, args.num_edmans, host=args.host,
            on_error='none', device=args.device)
        ranked = sorted(out["diagnostic"]["incompatibility_scores"].items(), key=lambda x: x[1], reverse=True)
        print("Excluded signals: " + str(len(out["diagnostic"]["exclude_signals"])))
        print("Highest incompatibility scores:")
        for signal, score in ranked[:5]:
            print("  " + str(signal) + ": " + repr(score))
    with open(output_filepath, 'wb') as f:
        pickle.dump(out, f, protocol=2)
    point, result, factor, _ = out["best_point"]
    print("Best point (edman_efficiency, dye_destruction, dud_dyes): " + str(point))
    print("Score (" + args.metric + "): " + repr(result) + ", normalization factor " + repr(factor))
    print("Saved results to " + str(output_filepath))
    return output_filepath


if __name__ == "__main__":
    main()
    sys.exit(0)
