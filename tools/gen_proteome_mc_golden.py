"""Writes tests/golden/proteome_mc.npz: recorded runs of the reference's MCsimlib.py - random_signal (:863-1074) under the
draw contract of _host_proteome_mc, the preprocessing functions (:88-279) and SignalTrie.find_uniques /
find_uniques_absolute (:1398-1532).  Data only: signals, draw counts and JSON text of inputs and results.

The reference's functions and the SignalTrie class are taken out of its file at run time through oracle/refload.py (the
function extraction of gen_lognormal_golden.load_functions, extended to class definitions) and nothing of it is written to
disk.  Two things are set as Python 2 had them: _dp's division of integers is a floor division, and time.clock exists.  The
module's `random` is an object that reads stream 3 of the sample; `windows` dicts are passed in sorted order (the twin's
order contract) and signals are canonicalised to the twin's tie rule (by position, then acid).

Also prints the reference's own random_signal rate on one core.

    python tools/gen_proteome_mc_golden.py"""
import ast
import json
import math
import os
import random
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from fluorosequencingimageanalysis_amd import _host_peptide_sim as PSIM          # noqa: E402
from fluorosequencingimageanalysis_amd import _host_proteome_mc as H             # noqa: E402

N_SAMPLES = 300
FULL = tuple(range(1, 17))
GAPPED = {'E': (3, 4, 7), 'K': (7, 8, 9)}


class _FloorDiv(ast.NodeTransformer):
    def visit_BinOp(self, node):
        self.generic_visit(node)
        if isinstance(node.op, ast.Div):
            node.op = ast.FloorDiv()
        return node


def load_definitions(refload, rel, names, namespace):
    """The named top-level functions and classes of a reference file, converted as refload.load converts a module."""
    if refload._RT is None:
        refload._RT = refload._refactor_tool()
    src = open(os.path.join(refload.REF, rel)).read().expandtabs(8)
    out = str(refload._RT.refactor_string(src if src.endswith("\n") else src + "\n", rel))
    tree = ast.parse(out)
    keep = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert {n.name for n in keep} == set(names), names
    keep = [ast.fix_missing_locations(_FloorDiv().visit(n)) if n.name == "_dp" else n for n in keep]
    exec(compile(ast.Module(body=keep, type_ignores=[]), os.path.join(refload.REF, rel), "exec"), namespace)
    return namespace


def reference():
    import refload
    clock = types.SimpleNamespace(clock=time.perf_counter)
    ns = {"math": math, "random": random, "time": clock, "sys": sys}
    return load_definitions(refload, "MCsimlib.py", ["_dp", "random_signal", "cleave", "attach", "homogenize", "homogenize_attached",
                                                    "SignalTrie"], ns)


def signal_cases():
    two = {'D': FULL, 'K': FULL}
    return [
        dict(name="one_label", peptide=("AKAAKAAAKA", "CAKA"), windows={'K': FULL}, p=0.9, b=0.05, u=0.3),
        dict(name="two_labels_full", peptide=("AKDAAKDAADKAA", "CKAD"), windows=two, p=0.9, b=0.05, u=0.3),
        dict(name="gapped", peptide=("AEKAEAKEAK", "CEK"), windows=GAPPED, p=0.5, b=0.05, u=0.0),
        dict(name="gapped_duds", peptide=("EKEAKKEAEKAE", "CKEE"), windows=GAPPED, p=0.9, b=5.0, u=0.3),
        dict(name="head_of_one", peptide=("K", "CKD"), windows=two, p=0.9, b=5.0, u=0.3),
        dict(name="empty_head", peptide=("", "CKKD"), windows=two, p=1.0, b=0.05, u=0.3),
        dict(name="empty_tail", peptide=("AKDAK", ""), windows=two, p=0.5, b=0.0, u=0.0),
        dict(name="no_label", peptide=("AAGA", "CAA"), windows=two, p=0.9, b=0.05, u=0.3),
        dict(name="p_zero", peptide=("AKDAAK", "CK"), windows=two, p=0.0, b=0.05, u=0.0),
        dict(name="all_duds", peptide=("AKDAAK", "CK"), windows=two, p=0.9, b=0.05, u=1.0),
        dict(name="p_one_hard_bleach", peptide=("DKADKAAKD", "CDK"), windows=two, p=1.0, b=5.0, u=0.0),
        dict(name="half_edman", peptide=("AAKAADAAAAKD", "CKD"), windows=two, p=0.5, b=0.05, u=0.3),
    ]


PROTEINS = {
    "plain": "AKCDEKAACK", "doubled": "AKKCAKKKC", "at_end": "ACKDCK", "absent": "ACDEC", "only": "K", "only_two": "KK",
    "empty": "", "no_attach": "AKDEKA", "attach_first": "CAKCAK", "starts": "KACKA", "long": "ADECKKACDNEKCCKADNK", "one": "C",
}

COUNT_CASES = [("five_seven", (5, 7)), ("seven_five", (7, 5)), ("three_three", (3, 3)), ("four_four_one", (4, 4, 1)),
               ("single", (6,)), ("second_above", (9, 5, 2)), ("late_best", (2, 8, 8, 3)), ("all_ones", (1, 1, 1))]
UNIQUE_ARGS = [(None, 1, None), (None, 5, None), (2.0, 1, None), (1.0, 3, None), (1.4, 1, 4), (None, 1, 3), (2.0, 6, 2), (1.8, 9, 5)]
ABSOLUTE_ARGS = [(5, 3), (1, 10), (3, 0), (7, 5)]


def count_signal(i):
    """A distinct two-label signal per count case (nested prefixes among them)."""
    return tuple((x, 'K' if (x + i) % 2 else 'D') for x in range(1, 2 + i % 3)) + ((4 + i, 'K'),)


def listed(result):
    return [[[list(g) for g in signal], list(best), [list(s) for s in second], tertiary]
            for signal, (best, second, tertiary) in sorted(result.items())]


def main():
    ref = reference()
    out, meta = {}, []
    starts, pos, acid, draws = [0], [], [], []
    for ci, case in enumerate(signal_cases()):
        windows = {a: tuple(case["windows"][a]) for a in sorted(case["windows"])}
        order = sorted(windows)
        seed, first = 20260000 + ci, 1000 * ci
        for j in range(N_SAMPLES):
            stream = PSIM.Stream(seed, first + j, H.STREAM)
            ref["random"] = stream
            signal = H.canonical(ref["random_signal"](case["peptide"], case["p"], case["b"], case["u"], windows), order)
            pos.extend(x for x, _ in signal), acid.extend(order.index(a) for _, a in signal)
            starts.append(len(pos)), draws.append(stream.j)
        meta.append(dict(case, windows={a: list(windows[a]) for a in order}, seed=seed, first_sample=first))
    out["signal_cases"] = np.array(json.dumps(meta))
    out["signal_start"] = np.array(starts, np.int32)
    out["signal_pos"] = np.array(pos, np.int32)
    out["signal_acid"] = np.array(acid, np.uint8)
    out["n_draws"] = np.array(draws, np.int32).reshape(len(meta), N_SAMPLES)

    ref["random"] = random
    cleaved = ref["cleave"](dict(PROTEINS), 'K')
    pre = {"proteins": PROTEINS, "cleave_K": cleaved, "attach_C": ref["attach"](cleaved, 'C'),
           "attach_cterm": ref["attach"](cleaved, 'cterm'), "homogenize_E_DN": ref["homogenize"](dict(PROTEINS), 'E', ['D', 'N']),
           "homogenize_E_D": ref["homogenize"](dict(PROTEINS), 'E', ['D'])}
    pre["homogenize_attached_E_DN"] = ref["homogenize_attached"](pre["attach_C"], 'E', ['D', 'N'])
    out["preprocessing"] = np.array(json.dumps(pre))

    trie = ref["SignalTrie"]((None, None))
    n_proteins = max(len(c) for _, c in COUNT_CASES)
    for pi in range(n_proteins):                                # protein-major, as monte_carlo_trie samples
        for i, (_, counts) in enumerate(COUNT_CASES):
            for _ in range(counts[pi] if pi < len(counts) else 0):
                trie.add_descendant(count_signal(i), "P%d" % pi)
    uniq = {"cases": [[name, [list(g) for g in count_signal(i)], list(c)] for i, (name, c) in enumerate(COUNT_CASES)],
            "count_nodes": list(trie.count_nodes()),
            "find_uniques": [[list(a), listed(trie.find_uniques(*a))] for a in UNIQUE_ARGS],
            "find_uniques_absolute": [[list(a), listed(trie.find_uniques_absolute(*a))] for a in ABSOLUTE_ARGS]}
    out["uniques"] = np.array(json.dumps(uniq))

    path = os.path.join(ROOT, "tests", "golden", "proteome_mc.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes): %d cases x %d samples" % (path, os.path.getsize(path), len(meta), N_SAMPLES))

    peptide, windows = ("AKDAAKDAADKAA", "CKAD"), {'D': FULL, 'K': FULL}
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < 2.0:
        for _ in range(500):
            ref["random_signal"](peptide, 0.9, 0.05, 0.1, windows)
        n += 500
    print("reference random_signal, one core of Python: %.3g signals/s (%d signals)" % (n / (time.perf_counter() - t0), n))


if __name__ == "__main__":
    main()
