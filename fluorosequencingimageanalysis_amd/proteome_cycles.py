"""Identifiable proteins against the number of Edman cycles, from one proteome Monte-Carlo (MCsimlib.cycle_curve_records).

    python -m fluorosequencingimageanalysis_amd.proteome_cycles PROTEOME --cleave E --attach C --label K:1-30 --label D:1-30
        -p 0.9 -b 0.05 -u 0.1 --sample_size 1000 --seed 7 --worst_ratio 10 --absolute_min 5
        [--maximum_secondary X --cycles A:B --host --output_directory DIR]

PROTEOME is a pickle of {name: sequence} (MCsimlib.load_proteome) or a FASTA file.  The proteome is cleaved after --cleave,
attached by --attach ('cterm': by every peptide's end) and sampled --sample_size times per attached peptide at the longest
experiment the labels' windows allow; the tally is then projected onto every cycle count of --cycles (default: 1 .. the last
observable position) and scanned as SignalTrie.find_uniques scans.  Writes Cycles_HASH.csv, one row per cycle count, and
prints it."""
import argparse
import os
from time import time

from . import MCsimlib
from .pflib import _epoch_to_hash

COLUMNS = ("cycles", "n_signals", "n_pairs", "samples_detected", "n_passing_signals", "n_identifiable_proteins")


def label(text):
    """'K:1-30' -> ('K', (1, ..., 30)); 'K:3,4,7' -> ('K', (3, 4, 7))."""
    try:
        acid, spec = text.split(':')
        positions = []
        for part in spec.split(','):
            lo, _, hi = part.partition('-')
            positions.extend(range(int(lo), int(hi or lo) + 1))
        if len(acid) != 1 or not positions:
            raise ValueError
    except ValueError:
        raise argparse.ArgumentTypeError("%r is not ACID:LO-HI or ACID:X,Y,..." % text)
    return acid, tuple(positions)


def cycle_range(text):
    """'A:B' -> A .. B; 'A' -> [A]."""
    try:
        lo, _, hi = text.partition(':')
        lo, hi = int(lo), int(hi or lo)
        if lo < 0 or hi < lo:
            raise ValueError
    except ValueError:
        raise argparse.ArgumentTypeError("%r is not A:B with 0 <= A <= B" % text)
    return list(range(lo, hi + 1))


def read_fasta(path):
    """{the header's first word: the sequence} of a FASTA file, in file order."""
    out, name = {}, None
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith('>'):
                name = (line[1:].split() or [""])[0]
                if not name or name in out:
                    raise ValueError("%s: a record without a name, or %r twice" % (path, name))
                out[name] = []
            elif line:
                if name is None:
                    raise ValueError("%s: a sequence before the first '>' header" % path)
                out[name].append(line.rstrip('*'))
    if not out:
        raise ValueError("%s holds no FASTA record" % path)
    return {k: "".join(v) for k, v in out.items()}


def load(path):
    with open(path, 'rb') as f:
        first = f.read(1)
    return read_fasta(path) if first == b'>' else MCsimlib.load_proteome(path)


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('proteome', help="A pickle of {name: sequence} or a FASTA file.")
    p.add_argument('--cleave', required=True, help="The acid after which the proteins are cut.")
    p.add_argument('--attach', required=True, help="The acid by which a peptide is attached, or 'cterm'.")
    p.add_argument('--label', type=label, action='append', required=True, help="ACID:LO-HI, the acid's windows; may be repeated.")
    p.add_argument('-p', type=float, required=True, help="Edman efficiency.")
    p.add_argument('-b', type=float, required=True, help="Photobleaching rate per exposure.")
    p.add_argument('-u', type=float, required=True, help="Dud rate.")
    p.add_argument('--sample_size', type=int, required=True, help="Samples per attached peptide.")
    p.add_argument('--seed', type=int, default=None, help="Seed of the draws (default: a fresh one).")
    p.add_argument('--worst_ratio', type=float, default=None)
    p.add_argument('--absolute_min', type=float, required=True)
    p.add_argument('--maximum_secondary', type=float, default=None)
    p.add_argument('--cycles', type=cycle_range, default=None, help="A:B (default: 1 .. the last observable position).")
    p.add_argument('--host', action='store_true', default=False, help="Run the NumPy twins; no GPU needed.")
    p.add_argument('--device', default=None, help="The torch device (default: cuda).")
    p.add_argument('--output_directory', default=os.getcwd(), help="Created if it does not exist.")
    return p


def csv_text(curve):
    lines = [",".join(COLUMNS)]
    lines += [",".join(str(int(curve[name][i])) for name in COLUMNS) for i in range(len(curve["cycles"]))]
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
    if args.host:
        source = MCsimlib.monte_carlo_records(table, args.p, args.b, args.u, sample_size=args.sample_size, seed=seed, host=True)
    else:
        source = MCsimlib.monte_carlo_device(table, args.p, args.b, args.u, args.sample_size, seed, device=args.device)
    curve = MCsimlib.cycle_curve_records(source, args.worst_ratio, args.absolute_min, args.maximum_secondary, cycles=args.cycles,
                                         host=args.host, device=args.device)
    output_directory = os.path.abspath(args.output_directory)
    if not os.path.exists(output_directory):
        os.makedirs(output_directory)
    path = os.path.join(output_directory, "Cycles_" + str(_epoch_to_hash(round(time()))) + ".csv")
    text = csv_text(curve)
    with open(path, "w") as f:
        f.write(text)
    print(text, end="")
    print("Wrote " + path)
    return path


if __name__ == "__main__":
    main()
