"""Writes tests/golden/proteome_cycles.npz: recorded runs of the reference's SignalTrie.truncating_projection, merge, prune and
graft (MCsimlib.py:1560-1759).  Data only: JSON text of the input triples and of what the reference's trie holds afterwards.

The reference's class is taken out of its file at run time as tools/gen_proteome_mc_golden.py takes it (nothing of it is
written to disk), with one more thing set as Python 2 had it: in truncating_projection the root node's block position is None,
and `None <= cycles` was true; under Python 3 it raises TypeError.  An AST rewrite at load time turns every `<=` of that method
into a call that answers True for None on the left.

Recorded, for two cases (two acids with full windows 1 .. 8; the gapped windows {'E': (3, 4, 7), 'K': (7, 8, 9)}):
  triples            (signal, protein, count), inserted protein-major with add_descendant, nested prefixes among the signals;
  projections        for c = 0 .. one past the last position: the leaf dicts and count_nodes after truncating_projection(c) of a
                     fresh copy, and find_uniques / find_uniques_absolute of a reference trie rebuilt from those leaves in
                     ascending protein order (the reference's own dict order after graft is not the order contract, and its
                     scan is order dependent);
  merge              the leaves of a.merge(b) and a.merge(b, cycles) for two halves of the triples;
  edit               a prune / graft sequence with what each call returns and the leaves and count_nodes after each.

    python tools/gen_proteome_cycles_golden.py"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_proteome_mc_golden as G                                               # noqa: E402

GAPPED = {'E': (3, 4, 7), 'K': (7, 8, 9)}
FULL = {'D': tuple(range(1, 9)), 'K': tuple(range(1, 9))}
N_PROTEINS = 7
UNIQUE_ARGS = [(None, 1, None), (2.0, 1, None), (1.5, 3, 4), (3.0, 5, None)]
ABSOLUTE_ARGS = [(3, 1), (5, 0)]


class _NoneBelow(ast.NodeTransformer):
    """a <= b -> _le(a, b) inside truncating_projection."""

    def visit_FunctionDef(self, node):
        if node.name == "truncating_projection":
            for i, stmt in enumerate(node.body):
                node.body[i] = _Le().visit(stmt)
        return node


class _Le(ast.NodeTransformer):
    def visit_Compare(self, node):
        self.generic_visit(node)
        if len(node.ops) == 1 and isinstance(node.ops[0], ast.LtE):
            return ast.Call(func=ast.Name(id="_le", ctx=ast.Load()), args=[node.left, node.comparators[0]], keywords=[])
        return node


def reference_trie():
    import refload
    if refload._RT is None:
        refload._RT = refload._refactor_tool()
    rel = "MCsimlib.py"
    src = open(os.path.join(refload.REF, rel)).read().expandtabs(8)
    tree = ast.parse(str(refload._RT.refactor_string(src if src.endswith("\n") else src + "\n", rel)))
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "SignalTrie"]
    assert len(keep) == 1
    keep = [ast.fix_missing_locations(_NoneBelow().visit(keep[0]))]
    ns = {"math": math, "random": random, "time": types.SimpleNamespace(clock=time.perf_counter), "sys": sys,
          "_le": lambda a, b: True if a is None else a <= b}
    exec(compile(ast.Module(body=keep, type_ignores=[]), os.path.join(refload.REF, rel), "exec"), ns)
    return ns["SignalTrie"]


def observable(windows):
    """The (position, acid) pairs a signal under these windows can hold, by position then acid."""
    out = []
    for acid in sorted(windows):
        e = set(windows[acid]) | set(x - 1 for x in windows[acid])
        out.extend((x, acid) for x in sorted(e) if x - 1 in e and x >= 1)
    return sorted(out)


def triples_of(windows, n_signals, seed):
    """Random signals (subsets of the observable pairs, sorted by position then acid), each prefix of the longest ones among them
    (nested prefixes), with 1 .. 3 proteins each; listed protein-major."""
    rng = np.random.default_rng(seed)
    pairs = observable(windows)
    signals = set()
    while len(signals) < n_signals:
        m = int(rng.integers(1, min(len(pairs), 6) + 1))
        s = tuple(pairs[i] for i in sorted(rng.choice(len(pairs), m, replace=False).tolist()))
        signals.add(s)
        if len(s) > 2 and len(signals) % 3 == 0:
            signals.add(s[:len(s) // 2]), signals.add(s[:-1])
    out = []
    for s in sorted(signals):
        for p in sorted(rng.choice(N_PROTEINS, int(rng.integers(1, 4)), replace=False).tolist()):
            out.append((s, int(p), int(rng.integers(1, 9))))
    return sorted(out, key=lambda t: (t[1], t[0]))


def build(Trie, triples):
    trie = Trie((None, None))
    for signal, protein, count in triples:
        for _ in range(count):
            trie.add_descendant(signal, "P%d" % protein)
    return trie


def leaves(trie):
    return sorted([[list(g) for g in leaf[0]], dict(sorted(leaf[1].items()))] for leaf in trie.leaf_iterator())


def case(Trie, name, windows, n_signals, seed):
    triples = triples_of(windows, n_signals, seed)
    last = max(x for x, _ in observable(windows))
    out = {"name": name, "windows": {a: list(windows[a]) for a in sorted(windows)}, "n_proteins": N_PROTEINS,
           "triples": [[[list(g) for g in s], p, c] for s, p, c in triples], "last_position": last, "projections": []}
    for c in range(0, last + 2):
        trie = build(Trie, triples).truncating_projection(c)
        held = leaves(trie)
        ordered = Trie((None, None))
        for p in range(N_PROTEINS):                                  # ascending protein order: the order contract
            for signal, counts in held:
                if "P%d" % p in counts:
                    ordered.graft(tuple(tuple(g) for g in signal), {"P%d" % p: counts["P%d" % p]})
        assert leaves(ordered) == held
        out["projections"].append({"cycles": c, "leaves": held, "count_nodes": list(trie.count_nodes()),
                                   "find_uniques": [[list(a), G.listed(ordered.find_uniques(*a))] for a in UNIQUE_ARGS],
                                   "find_uniques_absolute": [[list(a), G.listed(ordered.find_uniques_absolute(*a))]
                                                             for a in ABSOLUTE_ARGS]})
    half_a, half_b = triples[::2], triples[1::2]
    out["merge"] = {"a": [i for i in range(0, len(triples), 2)], "b": [i for i in range(1, len(triples), 2)], "results": []}
    for cycles in (None, 0, last // 2, last):
        merged = build(Trie, half_a).merge(build(Trie, half_b), cycles)
        out["merge"]["results"].append({"cycles": cycles, "leaves": leaves(merged), "count_nodes": list(merged.count_nodes())})
    trie, steps = build(Trie, triples), []
    signals = sorted(set(s for s, _, _ in triples))
    inner = [s for s in signals if any(t != s and t[:len(s)] == s for t in signals)]
    outer = [s for s in signals if s not in inner]
    for op, signal in (("prune", inner[0]), ("prune", outer[0]), ("prune", outer[-1]), ("graft", outer[0]), ("prune", inner[-1]),
                       ("graft", inner[0]), ("graft", outer[0][:1] + ((last, sorted(windows)[-1]),))):
        if op == "prune":
            got = trie.prune(signal)
            returned = [[list(g) for g in got[0]], dict(sorted(got[1].items()))]
            counts = None
        else:
            counts = {"P1": 3, "P5": 2}
            returned = trie.graft(signal, dict(counts)) is trie
        steps.append({"op": op, "signal": [list(g) for g in signal], "counts": counts, "returned": returned, "leaves": leaves(trie),
                      "count_nodes": list(trie.count_nodes())})
    out["edit"] = steps
    return out


def main():
    Trie = reference_trie()
    cases = [case(Trie, "full", FULL, 60, 1), case(Trie, "gapped", GAPPED, 30, 2)]
    path = os.path.join(ROOT, "tests", "golden", "proteome_cycles.npz")
    np.savez_compressed(path, cases=np.array(json.dumps(cases)))
    print("wrote %s (%d bytes): %s" % (path, os.path.getsize(path),
                                      ", ".join("%s: %d triples, cycles 0 .. %d" % (c["name"], len(c["triples"]), c["last_position"] + 1)
                                                for c in cases)))


if __name__ == "__main__":
    main()
