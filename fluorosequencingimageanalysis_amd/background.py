"""Iterative background correction of signal counts: the reference's iterative_background_v2 step, on the GPU.

MCsimlib.iterative_peak_finding_v3 (:5932-6040) takes the signal counts of a boc- experiment and the average and standard
deviation of the percents of ac- control experiments.  Pass after pass it gives every key whose z-score against the controls
is above `sigma_threshold` a trial - its count replaced by the mean of its neighbours' counts, everything renormalised - and
keeps the one trial that lowers its own z-score most, until nothing is above the threshold or nothing improves.  What is left
is the background; the experiment minus it is the corrected experiment.  The passes run on the device as one call of
fsq_background_iterate (include/fsq_background.h; `background_device`, `background_records`) with the reference's bits, and
with numpy on the host with `device=None`.  The functions below `# ---- the reference's call surface` are drop-ins under the
reference's names.

Key order is part of the result (the total is a left-to-right float sum, undefined keys are interpolated one after the other,
and `max` keeps the first of equal values), and the reference walks Python 2 dicts and `tuple(set(...))` in hash order, which
no other interpreter reproduces.  The contract here: every dict is walked in insertion order, and every `tuple(set(keys))` is
`tuple(sorted(set(keys)))`.  The golden fixture was recorded from the reference patched to exactly that.

Checks, each raised on the host before anything is launched, on either route: keys of more than one label letter, keys with a
false is_zero, differing key sets of boc_raw and boc_percent (ValueError, as the reference); a negative sigma_threshold
(ValueError: a key that boc lacks could be chosen, and the reference then fails its own assert at :6006); an ac- key that boc
lacks whose z-score at a percent of 0 is above the threshold (ValueError, the same assert); filtered counts that add up to 0
(ZeroDivisionError); an undefined key without a neighbour in range (ValueError: the reference ends with `cannot convert float
NaN to integer`); more than MAX_DROPS drops per key, positions outside 0 .. MAX_POSITION, more than MAX_GROUPS starting
intensities (NotImplementedError); counts that are not finite or whose magnitudes add up to more than 2^53, beyond which the
reference's integer total is no float sum (ValueError).  `max_iterations` passes without a stop raise RuntimeError; the
reference has no such cap.  `background_device` takes device tensors as they are and checks their shapes and types only.

Two-colour experiments: joint signals (decrements, zeros, starts) of several label letters, by this package's definition
(the reference stops at one letter).  A key is a remainder when not all(zeros), multidrop when a cycle repeats
whatever the letters, and its neighbours are its own tuple with the cycles perturbed, looked up as they stand.
`joint_pack_problem` and `joint_background_records` run the iteration on joint keys with numpy on the host (a device raises
NotImplementedError); `neighbour_means_records` is the interpolation of many targets in one launch of
fsq_background_neighbour_means (include/fsq_background_joint.h).  The reference-named functions accept joint keys; their
one-letter results do not change."""
import ctypes

import numpy as np

from . import _host_background as HB
from . import _host_signal_sweep as HS
from . import _native_background as NB
from . import engine as _engine
from .pflib import _py2_round

MAX_DROPS, MAX_POSITION, MAX_GROUPS = NB.MAX_DROPS, NB.MAX_POSITION, NB.MAX_GROUPS
DEFAULT_MAX_ITERATIONS = 1 << 20
STOP_REASONS = {NB.NO_DEFINED: "no defined z-score", NB.THRESHOLD: "threshold", NB.NO_IMPROVEMENT: "no improvement",
                NB.CONVERGED: "converged", NB.MAX_ITERATIONS: "max_iterations", NB.ZERO_TOTAL: "zero total"}
_INPUTS = {"key_off": "int64", "def_off": "int64", "first_off": "int64", "rest_off": "int64", "num_cycles": "int32",
           "include_multidrop": "int32", "sigma_threshold": "float64", "code": "int64", "sorted_code": "int64",
           "sorted_index": "int32", "filter": "uint8", "nb_off": "int64", "def_key": "int32", "def_avg": "float64",
           "def_std": "float64", "und_first": "int32", "und_rest": "int32", "count": "float64", "percent": "float64"}
_PER_KEY = ("code", "sorted_code", "sorted_index", "filter", "count", "percent")


def _seq_sum(values):
    """Python 2's sum(): from int 0, left to right, nothing compensated."""
    total = 0
    for v in values:
        total = total + v
    return total


# ---- packing one problem ----

def _checked_key(key):
    s, z, si = key
    if len(s) == 0:
        raise ValueError("Not defined for empty signal.")
    if not z:
        raise ValueError("Not defined for remainders.")
    if len(s) > MAX_DROPS:
        raise NotImplementedError("keys are limited to %d drops" % MAX_DROPS)
    for aa, pos in s:
        if int(pos) != pos or not 0 <= pos <= MAX_POSITION:
            raise NotImplementedError("positions are limited to 0 .. %d" % MAX_POSITION)
    return s, si


def pack_problem(boc_raw, boc_percent, ac_average, ac_std, num_cycles, sigma_threshold=3, include_multidrop=False):
    """One problem of background_records from the dicts of iterative_peak_finding_v3, after the checks the module docstring
    names.  Returns a dict of arrays (include/fsq_background.h names them) plus "keys", the key universe in order."""
    return _pack(boc_raw, boc_percent, ac_average, ac_std, num_cycles, sigma_threshold, include_multidrop, None)


def _joint_limits(n_channels):
    return min(NB.JOINT_MAX_DROPS, HS.JOINT_MAX_DROPS[n_channels])


def _joint_letters(all_keys, labels):
    """The sorted label letters of a joint problem, after the checks on its keys that need no code."""
    all_keys = list(all_keys)
    if not all(HS.is_joint(k) for k in all_keys):
        raise ValueError("joint and one-letter keys are mixed")
    widths = set(len(k[1]) for k in all_keys) | set(len(k[2]) for k in all_keys)
    found = sorted(set(aa for k in all_keys for aa, c in k[0]))
    if labels is None:
        if len(widths) != 1 or len(found) != next(iter(widths)):
            raise ValueError("the keys differ in their label letters, or a letter never drops: name the letters with `labels`")
        labels = found
    letters = tuple(sorted(set(labels)))
    if not 1 <= len(letters) <= HS.MAX_CHANNELS:
        raise ValueError("a joint signal has 1 .. %d label letters" % HS.MAX_CHANNELS)
    if widths != {len(letters)} or not set(found) <= set(letters):
        raise ValueError("the keys differ in their label letters: %r are expected" % (letters,))
    return letters


def _checked_joint_key(key, letters):
    """The joint key (the 64-bit code) of a signal after the checks of _checked_key, each limit under its name."""
    s, zeros, starts = key
    if len(s) == 0:
        raise ValueError("Not defined for empty signal.")
    if not all(zeros):
        raise ValueError("Not defined for remainders.")
    if len(s) > _joint_limits(len(letters)):
        raise NotImplementedError("joint keys of %d letters are limited to %d drops (FSQ_BACKGROUND_JOINT_MAX_DROPS, "
                                  "FSQ_SIGNAL_JOINT_MAX_DROPS)" % (len(letters), _joint_limits(len(letters))))
    if any(int(st) != st or not 0 <= st <= 15 for st in starts):
        raise NotImplementedError("starting counts are limited to 0 .. 15 (the joint key's nibble)")
    if any(int(c) != c or not 1 <= c <= NB.JOINT_MAX_CYCLES for aa, c in s):
        raise NotImplementedError("cycles are limited to 1 .. %d (FSQ_BACKGROUND_JOINT_MAX_CYCLES)" % NB.JOINT_MAX_CYCLES)
    code = HS.joint_key_of_signal(letters, key)
    if code is None:
        raise ValueError("%r is no joint signal of the letters %r" % (key, letters))
    return code


def joint_pack_problem(boc_raw, boc_percent, ac_average, ac_std, num_cycles, sigma_threshold=3, include_multidrop=False, labels=None):
    """pack_problem for joint signals (decrements, zeros, starts) of several label letters: one problem of
    joint_background_records, its codes the joint keys of _host_signal_sweep.joint_key_of_signal under the sorted letters
    `labels` (by default the letters that drop), and "n_channels" their number.  All checks of pack_problem are carried over;
    the limits (1 <= num_cycles <= 63, at most min(8, FSQ_SIGNAL_JOINT_MAX_DROPS(K)) drops, starts of at most 15) raise
    NotImplementedError, mixed joint and one-letter keys or differing letter sets ValueError."""
    num_cycles = int(num_cycles)
    if not 1 <= num_cycles <= NB.JOINT_MAX_CYCLES:
        raise NotImplementedError("num_cycles is limited to 1 .. %d (FSQ_BACKGROUND_JOINT_MAX_CYCLES)" % NB.JOINT_MAX_CYCLES)
    letters = _joint_letters(list(boc_raw.keys()) + list(boc_percent.keys()) + list(ac_average.keys()) + list(ac_std.keys()), labels)
    return _pack(boc_raw, boc_percent, ac_average, ac_std, num_cycles, sigma_threshold, include_multidrop, letters)


def _pack(boc_raw, boc_percent, ac_average, ac_std, num_cycles, sigma_threshold, include_multidrop, letters):
    """pack_problem (letters None) and joint_pack_problem (the sorted letters)."""
    if set(boc_raw.keys()) != set(boc_percent.keys()):
        raise ValueError("boc_raw and boc_percent don't have matching keys.")
    if set(ac_average.keys()) != set(ac_std.keys()):
        raise Exception()                                              # (:5776-5777)
    if not sigma_threshold >= 0:
        raise ValueError("sigma_threshold must not be negative: a key that boc lacks could be chosen, on which the reference "
                         "fails its own assert (MCsimlib.py:6006)")
    num_cycles = int(num_cycles)
    if not -(1 << 31) < num_cycles < (1 << 31):
        raise ValueError("num_cycles must fit 32 bits")
    include_multidrop = bool(include_multidrop)
    keys = list(boc_raw.keys())
    index = {k: i for i, k in enumerate(keys)}
    undefined_ac = [k for k in ac_average.keys() if ac_std[k] == 0]
    for k in undefined_ac:
        if k not in index:
            index[k] = len(keys)
            keys.append(k)
    seen, groups, code = set(), {}, np.zeros(len(keys), np.uint64)
    positions = []
    for k in list(keys) + [k for k in ac_average.keys() if k not in index]:
        if letters is not None:
            _checked_joint_key(k, letters)
            continue
        s, si = _checked_key(k)
        seen.update(aa for aa, pos in s)
    if len(seen) > 1:
        raise ValueError("Currently only implemented for one label.")

    def code_of(k):
        if letters is not None:
            return _checked_joint_key(k, letters)
        s, si = k[0], k[2]
        g = groups.setdefault(si, len(groups))
        if g >= MAX_GROUPS:
            raise NotImplementedError("a problem is limited to %d starting intensities" % MAX_GROUPS)
        c = (g << 51) | (len(s) << 48)
        for i, (aa, pos) in enumerate(s):
            c |= int(pos) << (8 * i)
        return c
    for i, k in enumerate(keys):
        code[i] = code_of(k)
        positions.append([int(pos) for aa, pos in k[0]])
    filt = np.array([(include_multidrop or len(set(p)) == len(p)) and max(p) <= num_cycles for p in positions] or [], dtype=np.uint8)
    count = np.array([float(boc_raw.get(k, 0)) for k in keys], dtype=np.float64)
    if not np.isfinite(count).all() or np.abs(count).sum() > float(1 << 53):
        raise ValueError("counts must be finite and their magnitudes add up to at most 2^53")
    percent = np.array([float(boc_percent.get(k, 0)) for k in keys], dtype=np.float64)
    defined = [k for k in ac_average.keys() if ac_std[k] != 0]
    def_key = np.array([index.get(k, -1) for k in defined], dtype=np.int32)
    def_avg = np.array([float(ac_average[k]) for k in defined], dtype=np.float64)
    def_std = np.array([float(ac_std[k]) for k in defined], dtype=np.float64)
    lacking = def_key < 0
    if lacking.any() and not (HB.z_scores(np.zeros(int(lacking.sum())), def_avg[lacking], def_std[lacking]) <= sigma_threshold).all():
        raise ValueError("an ac- key that boc lacks has a z-score above sigma_threshold: the reference would choose it and fail its "
                         "own assert (MCsimlib.py:6006)")
    und_first = [index[k] for k in undefined_ac] + [index[k] for k in boc_percent.keys() if k not in ac_average]
    und_rest = [index[k] for k in undefined_ac] + [i for i, k in enumerate(keys) if filt[i] and k not in ac_average]
    if len(filt) and filt.any() and not (count < 0).any() and _seq_sum(count[filt.astype(bool)]) == 0:
        raise ZeroDivisionError("float division by zero")
    targets = np.array(sorted(set(und_first)), dtype=np.int64)
    lists = (HB.neighbour_lists(code, num_cycles, include_multidrop, rows=targets) if letters is None else
             HB.joint_neighbour_lists(code, len(letters), num_cycles, include_multidrop, rows=targets))
    for row, nb in zip(targets, lists):
        if len(nb) == 0:
            raise ValueError("cannot convert float NaN to integer: %r has no neighbour within %d cycles to interpolate from"
                             % (keys[row], num_cycles))
    return {"keys": keys, "code": code, "filter": filt, "count": count, "percent": percent, "def_key": def_key, "def_avg": def_avg,
            "def_std": def_std, "und_first": np.array(und_first, dtype=np.int32), "und_rest": np.array(und_rest, dtype=np.int32),
            "num_cycles": num_cycles, "include_multidrop": int(include_multidrop), "sigma_threshold": float(sigma_threshold),
            **({} if letters is None else {"n_channels": len(letters), "letters": letters})}


# ---- the device route ----

def concatenate_problems(problems):
    """The host arrays of fsq_background_iterate's inputs for a list of problems, and max_defined."""
    def offsets(name):
        off = np.zeros(len(problems) + 1, np.int64)
        np.cumsum([len(p[name]) for p in problems], out=off[1:])
        return off

    def cat(name, dtype):
        return np.ascontiguousarray(np.concatenate([np.asarray(p[name]).reshape(-1) for p in problems] or [np.zeros(0)]).astype(dtype))
    a = {"key_off": offsets("code"), "def_off": offsets("def_key"), "first_off": offsets("und_first"), "rest_off": offsets("und_rest"),
         "num_cycles": np.array([p["num_cycles"] for p in problems], dtype=np.int32),
         "include_multidrop": np.array([p["include_multidrop"] for p in problems], dtype=np.int32),
         "sigma_threshold": np.array([p["sigma_threshold"] for p in problems], dtype=np.float64),
         "code": cat("code", np.uint64), "filter": cat("filter", np.uint8), "count": cat("count", np.float64),
         "percent": cat("percent", np.float64), "def_key": cat("def_key", np.int32), "def_avg": cat("def_avg", np.float64),
         "def_std": cat("def_std", np.float64), "und_first": cat("und_first", np.int32), "und_rest": cat("und_rest", np.int32)}
    orders = [np.argsort(np.asarray(p["code"], dtype=np.uint64), kind='stable') for p in problems]
    a["sorted_index"] = np.ascontiguousarray(np.concatenate(orders or [np.zeros(0)]).astype(np.int32))
    a["sorted_code"] = np.ascontiguousarray(np.concatenate([np.asarray(p["code"], dtype=np.uint64)[o] for p, o in zip(problems, orders)]
                                                           or [np.zeros(0)]).astype(np.uint64))
    drops = ((a["code"] >> np.uint64(48)) & np.uint64(7)).astype(np.int64)
    a["nb_off"] = np.zeros(len(a["code"]) + 1, np.int64)
    np.cumsum(3 ** drops - 1, out=a["nb_off"][1:])
    return a, max([len(p["def_key"]) for p in problems] or [0])


def background_device(tensors, max_defined, n_neighbours, max_iterations=DEFAULT_MAX_ITERATIONS, accepted_cap=1024,
                      undefined_cap=0):
    """fsq_background_iterate on device tensors: `tensors` maps the input names of include/fsq_background.h (FsqBackgroundArgs,
    key_off .. percent) to contiguous tensors on one GPU, codes as 64-bit words; max_defined and n_neighbours are the
    host's knowledge of the largest defined list and of nb_off's last entry.  count and percent are updated in place.
    Returns a dict of device tensors: count, percent, rounded int64 [N], stop_reason, n_passes, n_accepted, overflow int32 [P],
    accepted_key int32 [P, accepted_cap] and, for undefined_cap > 0, undefined_bp float64 [P, undefined_cap].  The call
    synchronises the current stream after every batch of passes; the values of the tensors are not checked."""
    torch = _engine._torch()
    dev = tensors["count"].device
    for name, dtype in _INPUTS.items():
        t = tensors[name]
        if t.dim() != 1 or not t.is_contiguous() or not t.is_cuda or t.device != dev:
            raise ValueError("%s: a contiguous 1-D tensor on one GPU is needed" % name)
        if str(t.dtype) != "torch." + dtype and not (dtype == "int64" and t.element_size() == 8 and name.endswith("code")):
            raise ValueError("%s: %s is needed" % (name, dtype))
    P = int(tensors["num_cycles"].numel())
    N, D = int(tensors["count"].numel()), int(tensors["def_key"].numel())
    for name in ("key_off", "def_off", "first_off", "rest_off"):
        if int(tensors[name].numel()) != P + 1:
            raise ValueError("%s: P + 1 offsets are needed" % name)
    if any(int(tensors[name].numel()) != P for name in ("include_multidrop", "sigma_threshold")):
        raise ValueError("one num_cycles, include_multidrop and sigma_threshold per problem")
    if any(int(tensors[name].numel()) != N for name in _PER_KEY) or int(tensors["nb_off"].numel()) != N + 1:
        raise ValueError("one entry per key is needed in %s, and N + 1 in nb_off" % ", ".join(_PER_KEY))
    if int(tensors["def_avg"].numel()) != D or int(tensors["def_std"].numel()) != D:
        raise ValueError("one def_avg and def_std per defined key")
    max_iterations, accepted_cap, undefined_cap = int(max_iterations), int(accepted_cap), int(undefined_cap)
    if not (0 <= max_iterations < 1 << 31 and 0 <= accepted_cap and 0 <= undefined_cap and 0 <= int(max_defined) <= D
            and P * max(accepted_cap, undefined_cap, 1) < 1 << 31):
        raise ValueError("max_iterations, the capacities and max_defined are out of range")
    L = NB.lib()
    ws_bytes = L.fsq_background_workspace_bytes(P, N, D, int(n_neighbours))
    if ws_bytes < 0:
        raise ValueError("fsq_background_workspace_bytes: invalid sizes")
    out = {"count": tensors["count"], "percent": tensors["percent"],
           "rounded": torch.empty(N, dtype=torch.int64, device=dev),
           "stop_reason": torch.empty(P, dtype=torch.int32, device=dev), "n_passes": torch.empty(P, dtype=torch.int32, device=dev),
           "n_accepted": torch.empty(P, dtype=torch.int32, device=dev), "overflow": torch.empty(P, dtype=torch.int32, device=dev),
           "accepted_key": torch.empty((P, accepted_cap), dtype=torch.int32, device=dev)}
    if undefined_cap > 0:
        out["undefined_bp"] = torch.empty((P, undefined_cap), dtype=torch.float64, device=dev)
    args = NB.FsqBackgroundArgs(n_problems=P, max_iterations=max_iterations, max_defined=int(max_defined), accepted_cap=accepted_cap,
                                undefined_cap=undefined_cap, n_keys=N, n_defined=D, n_first=int(tensors["und_first"].numel()),
                                n_rest=int(tensors["und_rest"].numel()), n_neighbours=int(n_neighbours))
    for name in NB.POINTER_FIELDS:
        t = out.get(name, tensors.get(name))
        setattr(args, name, None if t is None or t.numel() == 0 else t.data_ptr())
    ws = _engine.workspace(dev, ws_bytes)
    _engine.launch(L.fsq_background_iterate, "fsq_background_iterate", dev, ctypes.byref(args), ws.data_ptr(), ws_bytes)
    return out


# ---- arrays ----

def background_records(problems, max_iterations=DEFAULT_MAX_ITERATIONS, accepted_cap=1024, undefined_cap=0, device="cuda"):
    """P problems (the dicts of pack_problem, or arrays of their names built otherwise) to their stops in one call.
    device  where it runs; None: with numpy on the host.  Returns one dict per problem: count float64 [N], percent float64 [N]
    (0 on the keys outside the filter), rounded int64 [N], stop_reason, n_passes, n_accepted, overflow, accepted_key (the key
    index accepted by each accepting pass, up to accepted_cap) and undefined_bp (bp of every undefined key, pass after pass, up
    to undefined_cap)."""
    problems = list(problems)
    if any(p.get("n_channels") is not None for p in problems):
        raise ValueError("joint problems go through joint_background_records")
    return _records(problems, max_iterations, accepted_cap, undefined_cap, device)


def joint_background_records(problems, max_iterations=DEFAULT_MAX_ITERATIONS, accepted_cap=1024, undefined_cap=0, device=None):
    """background_records for joint problems (the dicts of joint_pack_problem, or arrays of their names with "n_channels"), all
    of the same number of letters, with numpy on the host (_host_background.iterate with joint_neighbour_lists).  There is no
    device kernel for the iteration on joint keys: any device but None raises NotImplementedError; it is not quietly run on
    the host.  The limits (num_cycles, drops, sum(3^d - 1) < 2^31) are checked before anything runs."""
    problems = list(problems)
    channels = set(int(p["n_channels"]) if p.get("n_channels") is not None else None for p in problems)
    if len(channels) > 1 or None in channels:
        raise ValueError("joint problems of one number of label letters are needed, not %r" % sorted(channels, key=repr))
    n_channels = channels.pop() if channels else 1
    if not 1 <= n_channels <= HS.MAX_CHANNELS:
        raise ValueError("a joint signal has 1 .. %d label letters" % HS.MAX_CHANNELS)
    for p in problems:
        if not 1 <= int(p["num_cycles"]) <= NB.JOINT_MAX_CYCLES:
            raise NotImplementedError("num_cycles is limited to 1 .. %d (FSQ_BACKGROUND_JOINT_MAX_CYCLES)" % NB.JOINT_MAX_CYCLES)
        code = np.asarray(p["code"], dtype=np.uint64)
        B, cap = HS.JOINT_DROP_BITS[n_channels], _joint_limits(n_channels)
        if cap < HS.JOINT_MAX_DROPS[n_channels] and len(code) and ((code >> np.uint64(4 + B * cap)) & np.uint64((1 << B) - 1)).any():
            raise NotImplementedError("joint keys of %d letters are limited to %d drops (FSQ_BACKGROUND_JOINT_MAX_DROPS)"
                                      % (n_channels, cap))
    total = sum(int((3 ** HB.joint_decode(p["code"], n_channels)[1] - 1).sum()) for p in problems)
    if total >= 1 << 31:
        raise ValueError("the neighbour table of one call is limited to sum(3^d - 1) < 2^31 entries; %d are asked for" % total)
    if device is not None:
        raise NotImplementedError("the iteration on joint signals runs on the host only: pass device=None (command line: --host)")
    return _records(problems, max_iterations, accepted_cap, undefined_cap, None)


def _records(problems, max_iterations, accepted_cap, undefined_cap, device):
    max_iterations, accepted_cap, undefined_cap = int(max_iterations), int(accepted_cap), int(undefined_cap)
    if device is None:
        return [HB.iterate(p, max_iterations, accepted_cap, undefined_cap) for p in problems]
    if not problems:
        return []
    torch = _engine._torch()
    dev = torch.device(device)
    a, max_defined = concatenate_problems(problems)
    tensors = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to(dev) for k, v in a.items()}
    out = _engine.to_host(background_device(tensors, max_defined, int(a["nb_off"][-1]), max_iterations, accepted_cap, undefined_cap))
    res = []
    for p, prob in enumerate(problems):
        k0, k1 = int(a["key_off"][p]), int(a["key_off"][p + 1])
        n_und = len(prob["und_first"]) + (int(out["n_passes"][p]) - 1) * len(prob["und_rest"]) if int(out["n_passes"][p]) else 0
        res.append({"count": out["count"][k0:k1], "percent": out["percent"][k0:k1], "rounded": out["rounded"][k0:k1],
                    "stop_reason": int(out["stop_reason"][p]), "n_passes": int(out["n_passes"][p]),
                    "n_accepted": int(out["n_accepted"][p]), "overflow": int(out["overflow"][p]),
                    "accepted_key": out["accepted_key"][p, :min(int(out["n_accepted"][p]), accepted_cap)].copy(),
                    "undefined_bp": (out["undefined_bp"][p, :min(n_und, undefined_cap)].copy() if undefined_cap > 0
                                     else np.zeros(0, np.float64))})
    return res


def neighbour_means_records(lists, count, device="cuda"):
    """np.mean of count over every index list of `lists` (an index outside 0 .. len(count) - 1 counts 0, an empty list gives
    NaN) in one launch of fsq_background_neighbour_means, one wavefront per list: interpolate_signal for many targets at once.
    device=None: with numpy on the host.  A list longer than 6 560 entries raises ValueError.  Returns float64 [len(lists)]."""
    lists = [np.asarray(l, dtype=np.int64).reshape(-1) for l in lists]
    count = np.ascontiguousarray(count, dtype=np.float64).reshape(-1)
    if any(len(l) > NB.JOINT_MAX_NEIGHBOURS for l in lists):
        raise ValueError("a list is limited to %d entries (FSQ_BACKGROUND_JOINT_MAX_NEIGHBOURS)" % NB.JOINT_MAX_NEIGHBOURS)
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(l) for l in lists], out=off[1:])
    flat = np.concatenate(lists) if lists else np.zeros(0, np.int64)
    if device is None:
        padded = np.concatenate([count, [0.0]])                                    # (an absent entry reads the 0.0 behind the counts)
        flat = np.where((flat >= 0) & (flat < len(count)), flat, len(count))
        with np.errstate(all='ignore'):
            return np.array([np.mean(padded[flat[a:b]]) if b > a else np.nan for a, b in zip(off[:-1], off[1:])], dtype=np.float64)
    flat = np.where((flat >= -(1 << 31)) & (flat < 1 << 31), flat, -1).astype(np.int32)    # (the kernel tests the range itself)
    if not lists:
        return np.zeros(0, np.float64)
    torch = _engine._torch()
    dev = torch.device(device)
    d_nb, d_off, d_count = (torch.from_numpy(v).to(dev) for v in (flat, off, count))
    d_out = torch.empty(len(lists), dtype=torch.float64, device=dev)
    _engine.launch(NB.lib().fsq_background_neighbour_means, "fsq_background_neighbour_means", dev,
                   d_nb.data_ptr() if len(flat) else None, d_off.data_ptr(), len(lists), d_count.data_ptr() if len(count) else None,
                   len(count), d_out.data_ptr())
    return d_out.cpu().numpy()


# ---- the reference's call surface ----

def ends_at_zero(z):
    """is_zero of a reference signal, all(zeros) of a joint one."""
    return all(z) if isinstance(z, tuple) else z


def _one_kind(keys):
    """Whether the keys are joint signals; mixed kinds raise ValueError."""
    kinds = set(HS.is_joint(k) for k in keys)
    if len(kinds) > 1:
        raise ValueError("joint and one-letter keys are mixed")
    return bool(kinds) and kinds.pop()


def is_multidrop(signal):
    """MCsimlib.is_multidrop (:5589-5597)."""
    positions = [pos for aa, pos in signal]
    return len(positions) > len(set(positions))


def discard_late_signals(signals, max_cycle=None):
    """MCsimlib.discard_late_signals (:5600-5614)."""
    if max_cycle is None:
        return dict(signals)
    return {(s, z, si): count for (s, z, si), count in signals.items() if max([pos for aa, pos in s]) <= max_cycle}


def head_truncate(signals, num_cycles=None):
    """MCsimlib.head_truncate (:5617-5632)."""
    if num_cycles is None or num_cycles == 0:
        return dict(signals)
    if not num_cycles > 0:
        raise ValueError("num_cycles must be None or a non-negative integer.")
    truncated_signals = {}
    for (s, z, si), f in signals.items():
        if min([pos for aa, pos in s]) <= num_cycles:
            continue
        truncated_signals.setdefault((tuple([(aa, pos - num_cycles) for aa, pos in s]), z, si), f)
    return truncated_signals


def counts_to_percent(signals, include_remainders=False, include_multidrop=True, max_cycle=None):
    """MCsimlib.counts_to_percent (:5635-5659): the total is a left-to-right sum in the dict's order."""
    filtered_signals = {(s, z, si): count for (s, z, si), count in signals.items()
                        if (include_remainders or ends_at_zero(z)) and (include_multidrop or not is_multidrop(s))}
    filtered_signals = discard_late_signals(signals=filtered_signals, max_cycle=max_cycle)
    total_count = _seq_sum(filtered_signals.values())
    return {k: float(count) / total_count for k, count in filtered_signals.items()}


def sum_signals(experiments):
    """MCsimlib.sum_signals (:5662-5671)."""
    summed_signals = {}
    for signals in experiments:
        for k, num in signals.items():
            summed_signals.setdefault(k, 0)
            summed_signals[k] += num
    return summed_signals


def _combined_keys(experiments_percent):
    """`tuple(set(...))` of :5686 and :5710 under the key-order contract: sorted."""
    return tuple(sorted(set(k for signals in experiments_percent for k in signals)))


def average_signals(experiments, include_remainders=False, include_multidrop=True, max_cycle=None):
    """MCsimlib.average_signals (:5673-5693), its keys sorted."""
    experiments = list(experiments)
    experiments_percent = [counts_to_percent(signals, include_remainders, include_multidrop, max_cycle) for signals in experiments]
    summed_signals = sum_signals(experiments_percent)
    return {k: float(summed_signals[k]) / len(experiments) for k in _combined_keys(experiments_percent)}


def signals_std(experiments, include_remainders=False, include_multidrop=True, max_cycle=None):
    """MCsimlib.signals_std (:5696-5719), its keys sorted; np.std is host work."""
    experiments_percent = [counts_to_percent(signals, include_remainders, include_multidrop, max_cycle) for signals in experiments]
    combined_keys = _combined_keys(experiments_percent)
    return {k: np.std([percents.get(k, 0) for percents in experiments_percent]) for k in combined_keys}


def generate_adjacent_positions(signal, include_multidrop=False):
    """MCsimlib.generate_adjacent_positions (:5722-5744).  A joint signal (decrements, zeros, starts) of several letters has
    the perturbed cycles of its decrements, in their order, whatever their letters; it is a remainder when not all(zeros)."""
    import itertools
    if len(signal) == 0 or (HS.is_joint(signal) and len(signal[0]) == 0):
        raise ValueError("Not defined for empty signal.")
    if not ends_at_zero(signal[1]):
        raise ValueError("Not defined for remainders.")
    if not HS.is_joint(signal) and len(set([aa for aa, pos in signal[0]])) != 1:
        raise ValueError("Currently only implemented for one label.")
    positions = tuple([pos for aa, pos in signal[0]])
    adjacent_positions = []
    for perturbation in itertools.product((-1, 0, 1), repeat=len(positions)):
        if all([p == 0 for p in perturbation]):
            continue
        perturbed_positions = [pos + perturbation[p] for p, pos in enumerate(positions)]
        if not include_multidrop and len(set(perturbed_positions)) < len(perturbed_positions):
            continue
        adjacent_positions.append(tuple(perturbed_positions))
    return adjacent_positions


def interpolate_signal(signals, interpolation_target, num_cycles, include_multidrop=False):
    """MCsimlib.interpolate_signal (:5747-5768): np.mean of the neighbours' values, 0 for an absent one.  For joint signals
    every neighbour keeps the target's letters, zeros and starts and is looked up as it stands: a perturbed tuple that no longer
    ascends by (cycle, letter) is no experiment's key and counts 0."""
    if _one_kind(list(signals) + [interpolation_target]):
        if len(set(len(signal[1]) for signal in list(signals) + [interpolation_target])) != 1:
            raise ValueError("the keys differ in their label letters")
        adjacent_positions = generate_adjacent_positions(signal=interpolation_target, include_multidrop=include_multidrop)
        adjacent_signals = [(tuple([(aa, pos) for (aa, _), pos in zip(interpolation_target[0], adj)]), interpolation_target[1],
                             interpolation_target[2]) for adj in adjacent_positions if all([0 < pos <= num_cycles for pos in adj])]
    else:
        amino_acid_set = set([aa for signal in signals for aa, pos in signal[0]])
        if len(amino_acid_set) != 1:
            raise ValueError("Currently only implemented for one label.")
        used_amino_acid = amino_acid_set.pop()
        adjacent_positions = generate_adjacent_positions(signal=interpolation_target, include_multidrop=include_multidrop)
        adjacent_signals = [(tuple([(used_amino_acid, pos) for pos in adj]), interpolation_target[1], interpolation_target[2])
                            for adj in adjacent_positions if all([0 < pos <= num_cycles for pos in adj])]
    with np.errstate(all='ignore'):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return np.mean([signals.get(s, 0) for s in adjacent_signals])


def outlier_z_scores(boc, ac_average, ac_std):
    """MCsimlib.outlier_z_scores (:5771-5792): (z_scores, undefined_z_scores), both in the order of ac_average's keys, then
    boc's."""
    import math
    if set(ac_average.keys()) != set(ac_std.keys()):
        raise Exception()
    z_scores, undefined_z_scores = {}, {}
    for k in list(ac_average.keys()) + list(boc.keys()):
        bp, ap, sp = boc.get(k, 0), ac_average.get(k, 0), ac_std.get(k, 0)
        if sp == 0:
            undefined_z_scores.setdefault(k, (bp, ap, sp))
        else:
            z_scores.setdefault(k, float(bp - ap) ** 2 / float(sp) ** 2)
    z_scores = {k: math.copysign(math.sqrt(m), boc.get(k, 0) - ac_average.get(k, 0)) for k, m in z_scores.items()}
    return z_scores, undefined_z_scores


def iterative_peak_finding_v3(boc_raw, boc_percent, ac_average, ac_std, num_cycles, sigma_threshold=3, include_multidrop=False,
                              sigma_subtract=None, device=None, max_iterations=DEFAULT_MAX_ITERATIONS, info=None, labels=None):
    """MCsimlib.iterative_peak_finding_v3 (:5932-6040): (peak_list, undefined_peaks, updated_boc_raw, updated_boc_percent).
    peak_list is always [], as in the reference.  device=None: numpy on the host; else the GPU to use.  max_iterations passes
    without a stop raise RuntimeError.  A dict given as `info` receives stop_reason, n_passes, n_accepted and accepted_keys.
    Joint signals (decrements, zeros, starts) of several label letters take the joint route (joint_pack_problem with the
    sorted letters `labels`, joint_background_records), which runs on the host: device must be None for them.  Mixed joint
    and one-letter keys raise ValueError."""
    joint = _one_kind(list(boc_raw.keys()) + list(boc_percent.keys()) + list(ac_average.keys()) + list(ac_std.keys()))
    if joint:
        prob = joint_pack_problem(boc_raw, boc_percent, ac_average, ac_std, num_cycles, sigma_threshold, include_multidrop, labels)
    else:
        prob = pack_problem(boc_raw, boc_percent, ac_average, ac_std, num_cycles, sigma_threshold, include_multidrop)
    records = joint_background_records if joint else background_records
    keys = prob["keys"]
    n_first, n_rest = len(prob["und_first"]), len(prob["und_rest"])
    undefined_cap = n_first + 64 * n_rest
    while True:
        (res,) = records([prob], max_iterations, accepted_cap=4096, undefined_cap=undefined_cap, device=device)
        if not res["overflow"] & NB.OVERFLOW_UNDEFINED:
            break
        undefined_cap = n_first + max(res["n_passes"] - 1, 0) * n_rest            # (the passes are the same the second time)
    if res["stop_reason"] == NB.ZERO_TOTAL:
        raise ZeroDivisionError("float division by zero")
    if res["stop_reason"] == NB.MAX_ITERATIONS:
        raise RuntimeError("iterative_peak_finding_v3: no stop within max_iterations = %d passes" % max_iterations)
    if np.isnan(res["count"]).any():
        raise ValueError("cannot convert float NaN to integer")
    if (res["rounded"] == HB.INT64_MIN).any():
        raise OverflowError("cannot convert float infinity to integer")
    undefined_peaks = []
    for r, bp in enumerate(res["undefined_bp"]):
        first = r < n_first
        k = keys[prob["und_first"][r] if first else prob["und_rest"][(r - n_first) % n_rest]]
        bp = boc_percent.get(k, 0) if first else float(bp)                       # (0.0 for a key outside the filter: == the reference's 0)
        undefined_peaks.append((k[0], k[1], k[2], bp, ac_average.get(k, 0), ac_std.get(k, 0)))
    updated_boc_raw = {k: int(v) for k, v in zip(keys, res["rounded"])}
    updated_boc_percent = {k: float(v) for k, v, f in zip(keys, res["percent"], prob["filter"]) if f}
    if info is not None:
        info.update(stop_reason=res["stop_reason"], n_passes=res["n_passes"], n_accepted=res["n_accepted"],
                    accepted_keys=[keys[i] for i in res["accepted_key"]])
    if sigma_subtract is not None:                                                 # (:6020-6039)
        assert set(updated_boc_percent.keys()) == set(updated_boc_raw.keys())
        for k, percent in list(updated_boc_percent.items()):
            if percent == 0:
                continue
            plus_sigma_ratio = float(percent + ac_std.get(k, 0)) / percent
            updated_boc_raw[k] = int(_py2_round(updated_boc_raw[k] * plus_sigma_ratio))
        updated_boc_percent = counts_to_percent(updated_boc_raw, include_remainders=False, include_multidrop=include_multidrop,
                                                max_cycle=num_cycles)
    return [], undefined_peaks, updated_boc_raw, updated_boc_percent
