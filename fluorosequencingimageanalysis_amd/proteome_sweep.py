"""Identifiable proteins over a grid of Edman efficiency p, photobleaching b and dud rate u (MCsimlib.grid_curve_records).

    python -m fluorosequencingimageanalysis_amd.proteome_sweep PROTEOME --cleave E --attach C --label K:1-30 --label D:1-30
        -p LO:HI:N -b LO:HI:N -u LO:HI:N --sample_size 100 --seed 7 --worst_ratio 10 --absolute_min 5
        [--maximum_secondary X --sample_stride N --host --device D --output_directory DIR]

PROTEOME is a pickle of {name: sequence} (MCsimlib.load_proteome) or a FASTA file.  A range LO:HI:N is N evenly spaced values
from LO to HI, both included; a single number is that value alone (as sweep_peptide reads them).  The proteome is cleaved after
--cleave, attached by --attach ('cterm': by every peptide's end) and sampled --sample_size times per attached peptide at every
point of the grid, p-major (u runs fastest); every point's tally is scanned as SignalTrie.find_uniques scans.  With
--sample_stride 0 (the default) every point sees the same draws; with N, point k starts N samples after point k - 1.  Writes
ProteomeSweep_HASH.csv, one row per point in grid order, and prints the seed, the table and the path."""
import argparse
import os
from time import time

from . import MCsimlib
from .pflib import _epoch_to_hash
from .proteome_cycles import label, load, read_fasta      # noqa: F401
from .sweep_peptide import value_range

COLUMNS = ("p", "b", "u", "n_signals", "n_pairs", "samples_detected", "n_passing_signals", "n_identifiable_proteins")


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('proteome', help="A pickle of {name: sequence} or a FASTA file.")
    p.add_argument('--cleave', required=True, help="The acid after which the proteins are cut.")
    p.add_argument('--attach', required=True, help="The acid by which a peptide is attached, or 'cterm'.")
    p.add_argument('--label', type=label, action='append', required=True, help="ACID:LO-HI, the acid's windows; may be repeated.")
    p.add_argument('-p', type=value_range, required=True, help="Edman efficiency: LO:HI:N or a number.")
    p.add_argument('-b', type=value_range, required=True, help="Photobleaching rate per exposure: LO:HI:N or a number.")
    p.add_argument('-u', type=value_range, required=True, help="Dud rate: LO:HI:N or a number.")
    p.add_argument('--sample_size', type=int, required=True, help="Samples per attached peptide and point.")
    p.add_argument('--seed', type=int, default=None, help="Seed of the draws (default: a fresh one).")
    p.add_argument('--sample_stride', type=int, default=0, help="Samples between the first samples of two points (default 0).")
    p.add_argument('--worst_ratio', type=float, default=None)
    p.add_argument('--absolute_min', type=float, required=True)
    p.add_argument('--maximum_secondary', type=float, default=None)
    p.add_argument('--host', action='store_true', default=False, help="Run the NumPy twins; no GPU needed.")
    p.add_argument('--device', default=None, help="The torch device (default: cuda).")
    p.add_argument('--output_directory', default=os.getcwd(), help="Created if it does not exist.")
    return p


def csv_text(curve):
    lines = [",".join(COLUMNS)]
    for i in range(len(curve["p"])):
        lines.append(",".join([repr(float(curve[name][i])) for name in COLUMNS[:3]] + [str(int(curve[name][i])) for name in COLUMNS[3:]]))
    return "\n".join(lines) + "\n"


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    windows = {}
    for acid, positions in args.label:
        if acid in windows:
            parser.error("--label: %s twice" % acid)
        windows[acid] = positions
    seed = MCsimlib.fresh_seed() if args.seed is None else args.seed
    peptides = MCsimlib.attach(MCsimlib.cleave(load(args.proteome), args.cleave), args.attach)
    table = MCsimlib.proteome_table(peptides, windows)
    print("Seed: " + str(seed))
    curve = MCsimlib.grid_curve_records(table, MCsimlib.grid_points(args.p, args.b, args.u), args.worst_ratio, args.absolute_min,
                                        args.maximum_secondary, sample_size=args.sample_size, seed=seed,
                                        sample_stride=args.sample_stride, host=args.host, device=args.device)
    output_directory = os.path.abspath(args.output_directory)
    if not os.path.exists(output_directory):
        os.makedirs(output_directory)
    path = os.path.join(output_directory, "ProteomeSweep_" + str(_epoch_to_hash(round(time()))) + ".csv")
    text = csv_text(curve)
    with open(path, "w") as f:
        f.write(text)
    print(text, end="")
    print("Wrote " + path)
    return path


if __name__ == "__main__":
    main()
