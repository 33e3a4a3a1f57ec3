"""The recorded bin-search cases of tests/golden/binsearch.npz (tools/gen_binsearch_golden.py), shared by the host and GPU
tests, and the three wrong restatements that show the fixture is not vacuous."""
import functools
import math
import os
import pickle

import numpy as np

import _binsearch_reference as B
from _util import GOLD

FIXED_BIN_COUNTS = list(range(1, 21)) + [127, 128, 129, 136, 255, 256, 257, 1023, 4097, 8191, 8192, 8193, 9999, 10000]
SEEDED_SIZES = (2, 7, 300, 5000)


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLD, "binsearch.npz"))


@functools.lru_cache(maxsize=None)
def value_sets():
    """Every recorded set: dict(name, values float64 in recorded order, sorted, lo, hi, is_int)."""
    g = golden()
    off = g["set_off"]
    out = []
    for i in range(len(off) - 1):
        v = g["set_values"][int(off[i]):int(off[i + 1])]
        out.append(dict(name=str(g["set_name"][i]), values=v, sorted=np.sort(v), lo=float(v.min()), hi=float(v.max()),
                        is_int=bool(g["set_is_int"][i])))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """Every recorded (set, bin count): dict(set, nb, cost, hist int64)."""
    g = golden()
    off = g["case_off"]
    return [dict(set=int(g["case_set"][i]), nb=int(g["case_nb"][i]), cost=float(g["case_cost"][i]),
                 hist=g["case_hist"][int(off[i]):int(off[i + 1])].astype(np.int64)) for i in range(len(off) - 1)]


def raw_of(s):
    """The values of a set as the reference took them: a tuple of Python ints or floats."""
    return tuple(int(x) for x in s["values"]) if s["is_int"] else tuple(float(x) for x in s["values"])


def searches():
    """The two full searches: (name, values float64, first bin count, recorded costs)."""
    g = golden()
    return [("full", g["full_values"], 10, g["full_cost"]), ("last_drop", g["ld_values"], 10, g["ld_cost"])]


def non_vacuity_counts(case_list, sets, search_list):
    """(cases whose counts change with a fused edge, cases whose counts change with <= at the inner edges, costs that change
    without the 8192 chunking, costs that change with step * step for pow(step, 2.0)), each against the recorded value.  The fused edges are exact fractions, so they are tried
    where they can matter at a bearable price: up to 136 bins; of the searches, the first 150 bin counts above 8192 are tried."""
    fused = le = chunk = product = 0
    for c in case_list:
        s = sets[c["set"]]
        if c["nb"] <= 136:
            fused += not np.array_equal(B.counts(s["sorted"], s["lo"], s["hi"], c["nb"], fused=True), c["hist"])
        le += not np.array_equal(B.counts(s["sorted"], s["lo"], s["hi"], c["nb"], inner_le=True), c["hist"])
        product += B.cost_of(c["hist"], len(s["sorted"]), s["lo"], s["hi"], c["nb"], product=True) != c["cost"]
        if c["nb"] > B.CHUNK:
            chunk += B.cost_of(c["hist"], len(s["sorted"]), s["lo"], s["hi"], c["nb"], chunk=None) != c["cost"]
    for name, values, first, cost in search_list:
        a = np.sort(values)
        for nb in range(first, min(first + len(cost), B.CHUNK + 151)):
            if nb <= B.CHUNK:                                      # (the sum is the recorded one: only the divisor can differ)
                step = (float(a[-1]) - float(a[0])) / float(nb)
                product += step * step != math.pow(step, 2.0)
            else:
                hist = B.counts(a, a[0], a[-1], nb)
                chunk += B.cost_of(hist, len(a), a[0], a[-1], nb, chunk=None) != float(cost[nb - first])
                product += B.cost_of(hist, len(a), a[0], a[-1], nb, product=True) != float(cost[nb - first])
    return int(fused), int(le), int(chunk), int(product)


def same_files_but_for_the_flag(dev, host):
    """The files of a run with the device search and of one with --host_bin_search, same path and timestamp: byte for byte
    equal, but for the flag itself where a file records the command line (one more argument, one digit of the parsed flag)."""
    assert sorted(dev) == sorted(host)
    for n in dev:
        if n == "COMMANDLINE.pkl":
            assert pickle.loads(host[n]) == pickle.loads(dev[n]) + ["--host_bin_search"]
        elif n == "INTERMEDIATES_v2.pkl":
            assert len(dev[n]) == len(host[n]) and sum(x != y for x, y in zip(dev[n], host[n])) == 1
            assert pickle.loads(host[n])[2].host_bin_search is True and pickle.loads(dev[n])[2].host_bin_search is False
        else:
            assert dev[n] == host[n], n
