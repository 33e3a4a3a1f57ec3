"""Simulation parameter sweeps scored against observed signals on the GPU: the loop of the reference's
jupyter_development.py that turns simulations into an answer.

There, simulate_peptide.py runs once per point of an (Edman efficiency p, dye destruction b, dud rate u) grid, the pickles are
collected into all_simulations = {(p, b, u): (signals, molecular_signals)}, and match_diagnostic (:786-948) scores every point
against the experiment's signals with signal_correlation (:279-578) and takes the best.  Here that is two calls,

    sweep = sweep_device(sequence, labels, num_mocks, num_edmans, points, num_simulations, seed=..., **fixed_parameters)
    point, result, factor, contributions = best_point(score_records(observed_signals, sweep, metric=...), reverse_order)

and one device path (include/fsq_signal_sweep.h): fsq_peptide_simulate_points simulates every point's molecules in one
flattened space, lognormal.lognormal_device fits them, fsq_signal_tally counts the molecules' and the fits' signals into one
hash table per point without leaving the device, fsq_signal_lookup makes the dense count matrix and fsq_signal_scores scores
all points at once.

`points` are (p, b, u) triples - peptide_simulation's p, b and u - or dicts with those keys and optionally s, s2 or
per_cycle_b; everything else is fixed_parameters.  Point k simulates molecules first_molecule + k * molecule_stride + i; with
molecule_stride = 0 every point sees the same draws (common random numbers), and each point's result is then what
peptide_simulator.simulate_and_fit_records gives for that point alone.

Limits, each an error and never a wrong count: a signal has at most 10 drops and starts at 15 dyes or fewer (the 64-bit key;
NotImplementedError), a point has at most `table_slots` distinct signals (ValueError naming table_slots=), counts are below 2^31.
Ten of signal_correlation's metrics are built (METRICS: those whose terms are non-negative sums or maxima); the others raise
NotImplementedError with the metric's name.  Sums run in ascending key order where the reference's run in dict order: a sum of
S non-negative terms differs by at most a relative 2 S 2^-53.  best_point's tie rule: the first point in grid order (the
reference's: its dict order); points without a result (None) are never chosen.

The rest of match_diagnostic stands at the end of this file: its incompatibility loop over all pairs of heat-map signals
(:833-889) as fsq_signal_pair_best and fsq_signal_pair_extremes on the same count matrix (incompatibility_device,
incompatibility_records), the heat-map tables without plotly (single_drops_table, double_drops_table) and match_diagnostic
itself, which returns what the notebook cell plots.

Several label letters (two-colour labelling): joint_sweep_device and joint_sweep_records run the same sweep over
peptide_simulator.joint_signal's (decrements, zeros, starts), a definition of this package - the reference stops at one
letter - under the joint 64-bit key of include/fsq_signal_sweep.h: fsq_peptide_simulate_labels_points, one lognormal fit per
colour channel, fsq_signal_tally_joint.  The sweep's dict carries `labels`, and score_device, score_records,
incompatibility_device, incompatibility_records and match_diagnostic then read joint signals, through the same lookup, score
and pair kernels.  joint_signals_of_fits gives the observed dict.  Limits: at most 4 letters; 10, 8, 6, 6 drops over all
channels for 1, 2, 3, 4 letters; a channel starts at 15 dyes or fewer.  sweep_device and sweep_records keep refusing several
letters."""
import ctypes
import decimal
import itertools
import math

import numpy as np

from . import _host_signal_sweep as H
from . import _native_signal_sweep as NS
from . import _tracks
from . import engine as _engine
from . import peptide_simulator as PS

METRICS = H.METRICS
_SCORE_KW = ("heatmap_only", "zero_only", "exclude_signals", "select_signals", "allow_multidrop")


# ---- points ----

def _point_dict(point):
    if isinstance(point, dict):
        return dict(point)
    p, b, u = point
    return {"p": p, "b": b, "u": u}


def _point_params(sequence, labels, num_mocks, num_edmans, seed, first_molecule, points, fixed):
    """(the base FsqPeptideSimParams, float64 [P][5] of FsqSweepPoint values, the points as dict keys).  Every point goes through
    peptide_simulator._params: its checks, and per_cycle_b = e ** -b as a single simulation computes it."""
    points = list(points)
    if not points:
        raise ValueError("at least one point is needed")
    values, base = np.empty((len(points), 5)), None
    for k, point in enumerate(points):
        ep = dict(fixed)
        ep.update(_point_dict(point))
        if 'per_cycle_b' in ep and 'b' in _point_dict(point):
            del ep['per_cycle_b']
        prm, _ = PS._params(sequence, labels, num_mocks, num_edmans, seed, first_molecule, ep)
        values[k] = (prm.p, prm.per_cycle_b, prm.u, prm.s, prm.s2)
        base = base or prm
    keys = [tuple(sorted(p.items())) if isinstance(p, dict) else tuple(p) for p in points]
    if len(set(keys)) != len(keys):
        raise ValueError("a point stands twice")
    return base, values, keys


def _check_sweep_shape(num_simulations, molecule_stride, table_slots, chunk_rows):
    n, stride, slots, chunk = int(num_simulations), int(molecule_stride), int(table_slots), int(chunk_rows)
    if n < 1 or stride < 0 or chunk < 1:
        raise ValueError("num_simulations and chunk_rows must be positive and molecule_stride must not be negative")
    if slots < 1 or slots & (slots - 1) or slots > NS.MAX_SLOTS:
        raise ValueError("table_slots=%d must be a power of two up to 2^24" % slots)
    return n, stride, slots, chunk


# ---- the device path ----

def simulate_points_device(prm, d_points, n_points, n_per_point, molecule_stride=0, first_row=0, n_rows=None):
    """fsq_peptide_simulate_points: counts uint8 [n_rows, frames], intensity float64 [n_rows, frames] and category int64 [n_rows]
    of rows first_row .. first_row + n_rows - 1 of the flattened [n_points][n_per_point] space; d_points is a float64 CUDA
    tensor [n_points, 5] of (p, per_cycle_b, u, s, s2).  Enqueued on the current stream, not synchronised."""
    torch = _engine._torch()
    if d_points.dtype != torch.float64 or tuple(d_points.shape) != (int(n_points), 5) or not d_points.is_contiguous():
        raise ValueError("a contiguous float64 tensor [n_points, 5] is needed")
    n = int(n_points) * int(n_per_point) - int(first_row) if n_rows is None else int(n_rows)
    dev, F = d_points.device, prm.num_mocks + prm.num_edmans + 1
    out = {"counts": torch.empty((max(n, 0), F), dtype=torch.uint8, device=dev),
           "intensity": torch.empty((max(n, 0), F), dtype=torch.float64, device=dev),
           "category": torch.empty(max(n, 0), dtype=torch.int64, device=dev)}
    _engine.launch(NS.lib().fsq_peptide_simulate_points, "fsq_peptide_simulate_points", dev, ctypes.byref(prm), d_points.data_ptr(),
                   int(n_points), int(n_per_point), int(molecule_stride), int(first_row), n,
                   *[out[k].data_ptr() if out[k].numel() else None for k in ("counts", "intensity", "category")])
    return out


def new_tables(n_points, slots, device):
    """The empty tables of fsq_signal_tally: keys int64 [n_points, slots] (the uint64 keys' bits), counts int64 [n_points, slots],
    none and unkeyed int64 [n_points], overflow int32 [n_points]."""
    torch = _engine._torch()
    return {"keys": torch.full((n_points, slots), NS.EMPTY, dtype=torch.int64, device=device),
            "counts": torch.zeros((n_points, slots), dtype=torch.int64, device=device),
            "none": torch.zeros(n_points, dtype=torch.int64, device=device),
            "unkeyed": torch.zeros(n_points, dtype=torch.int64, device=device),
            "overflow": torch.zeros(n_points, dtype=torch.int32, device=device)}


def tally_device(tables, d_rows, d_point, d_valid=None):
    """fsq_signal_tally: adds the signals of uint8 [n, frames] rows to the tables of their points (int32 [n]); d_valid uint8 [n]
    or None.  Enqueued, not synchronised."""
    torch = _engine._torch()
    n, frames = int(d_rows.shape[0]), int(d_rows.shape[1])
    if d_rows.dtype != torch.uint8 or d_point.dtype != torch.int32 or tuple(d_point.shape) != (n,):
        raise ValueError("uint8 rows [n, frames] and int32 points [n] are needed")
    if d_valid is not None and (d_valid.dtype != torch.uint8 or tuple(d_valid.shape) != (n,)):
        raise ValueError("a uint8 mask [n] is needed")
    if not 1 <= frames <= NS.MAX_FRAMES:
        raise ValueError("rows have 1 .. %d frames" % NS.MAX_FRAMES)
    if not (d_rows.is_contiguous() and d_point.is_contiguous() and (d_valid is None or d_valid.is_contiguous())):
        raise ValueError("contiguous tensors are needed")
    n_points, slots = (int(x) for x in tables["keys"].shape)
    _engine.launch(NS.lib().fsq_signal_tally, "fsq_signal_tally", d_rows.device, d_rows.data_ptr() if n else None, frames,
                   d_point.data_ptr() if n else None, None if d_valid is None or not n else d_valid.data_ptr(), n, n_points, slots,
                   tables["keys"].data_ptr(), tables["counts"].data_ptr(), tables["none"].data_ptr(), tables["unkeyed"].data_ptr(),
                   tables["overflow"].data_ptr())


def lookup_device(tables, d_wanted):
    """fsq_signal_lookup: int64 [n_wanted, n_points] counts of the int64-viewed keys d_wanted in every point's table."""
    torch = _engine._torch()
    n_points, slots = (int(x) for x in tables["keys"].shape)
    if d_wanted.dtype != torch.int64 or d_wanted.dim() != 1 or not d_wanted.is_contiguous():
        raise ValueError("a contiguous int64 tensor [n_wanted] is needed")
    out = torch.empty((int(d_wanted.shape[0]), n_points), dtype=torch.int64, device=d_wanted.device)
    _engine.launch(NS.lib().fsq_signal_lookup, "fsq_signal_lookup", d_wanted.device, tables["keys"].data_ptr(),
                   tables["counts"].data_ptr(), n_points, slots, d_wanted.data_ptr() if out.numel() else None, int(d_wanted.shape[0]),
                   out.data_ptr() if out.numel() else None)
    return out


def _check_tables(tables, what, slots, max_drops=NS.MAX_DROPS):
    if bool(tables["overflow"].any()):
        k = int(tables["overflow"].nonzero()[0])
        raise ValueError("point %d has more distinct %s than table_slots=%d: pass a larger power of two" % (k, what, slots))
    if bool(tables["unkeyed"].any()):
        k = int(tables["unkeyed"].nonzero()[0])
        raise NotImplementedError("point %d has %s with more than %d drops, or that start above 15 dyes: they have no 64-bit key"
                                  % (k, what, max_drops))


def sweep_device(sequence, labels, num_mocks, num_edmans, points, num_simulations, seed=0, first_molecule=0, molecule_stride=0,
                 fit=True, max_possible=5, allow_multidrop=True, max_deviation=3, quench_factors=None, solver=None, table_slots=1024,
                 chunk_rows=1 << 22, device=None, **fixed_parameters):
    """Simulate num_simulations molecules at every point, drop the molecules without dyes at any frame, fit the rest with
    lognormal.lognormal_device and tally the molecules' count rows and the fits' best_seq rows per point, in chunks of at most
    chunk_rows rows (the result does not depend on it).  Returns a dict: `points` (the points as dict keys, in grid order),
    `molecular` and `signals` (the tables of new_tables; `signals` is None with fit=False), total_count and none_count (int64
    CUDA tensors [n_points]; as lognormal.photometries_lognormal_fit counts the kept tracks), num_simulations, table_slots."""
    torch = _engine._torch()
    from . import lognormal as LN
    n, stride, slots, chunk = _check_sweep_shape(num_simulations, molecule_stride, table_slots, chunk_rows)
    base, values, keys = _point_params(sequence, labels, num_mocks, num_edmans, seed, first_molecule, points, fixed_parameters)
    P, F = len(keys), base.num_mocks + base.num_edmans + 1
    dev = torch.device(device or "cuda")
    fit_kw = {}
    if fit:
        means = _tracks.log_fluor_means(fixed_parameters['beta'], quench_factors, max_possible)
        fit_kw = dict(prm=LN.fit_params(means, fixed_parameters['beta_sigma'], max_possible, allow_multidrop, max_deviation,
                                        LN.DEFAULT_BUDGET), **LN._solver_kw(solver or 'enumerate'))
        if not allow_multidrop and F == 1:
            raise ValueError("max() arg is an empty sequence")        # (as lognormal.photometries_lognormal_fit, :5442)
    d_points = torch.from_numpy(values).to(dev)
    molecular, signals = new_tables(P, slots, dev), new_tables(P, slots, dev) if fit else None
    total, found_n = torch.zeros(P, dtype=torch.int64, device=dev), torch.zeros(P, dtype=torch.int64, device=dev)
    bad = torch.zeros((), dtype=torch.bool, device=dev)
    for first in range(0, P * n, chunk):
        rows = min(chunk, P * n - first)
        sim = simulate_points_device(base, d_points, P, n, stride, first, rows)
        d_point = torch.div(torch.arange(first, first + rows, device=dev), n, rounding_mode="floor").to(torch.int32)
        keep = sim["category"] != 0
        tally_device(molecular, sim["counts"], d_point, keep.to(torch.uint8))
        if not fit:
            total += torch.bincount(d_point[keep], minlength=P)
            continue
        d_int, d_cat, d_pt = sim["intensity"][keep].contiguous(), sim["category"][keep].contiguous(), d_point[keep].contiguous()
        kept = int(d_int.shape[0])
        if not kept:
            continue
        d_len = torch.full((kept,), F, dtype=torch.int32, device=dev)
        out = LN.lognormal_device(d_int, d_cat, d_len, None, None, **fit_kw)
        found = out["status"] == LN.STATUS_FOUND
        bad |= (out["status"] > LN.STATUS_NONE).any()
        tally_device(signals, out["best_seq"], d_pt, found.to(torch.uint8))
        total += torch.bincount(d_pt, minlength=P)
        found_n += torch.bincount(d_pt[found], minlength=P)
    if bool(bad):
        raise NotImplementedError("a simulated track has more surviving sequences than the budget, or an invalid length")
    _check_tables(molecular, "molecular signals", slots)
    if fit:
        _check_tables(signals, "fitted signals", slots)
    return {"points": keys, "molecular": molecular, "signals": signals, "total_count": total,
            "none_count": total - found_n if fit else None, "num_simulations": n, "table_slots": slots}


def _codec(sweep):
    """(key_of_signal, signal_of_key, letters) of a sweep: the joint key's under the sweep's `labels`, else the one-letter key's
    (letters None)."""
    letters = sweep.get("labels")
    if letters is None:
        return H.key_of_signal, H.signal_of_key, None
    letters = tuple(letters)
    return (lambda s: H.joint_key_of_signal(letters, s)), (lambda k: H.joint_signal_of_key(letters, k)), letters


def _decode_tables(tables, letters=None):
    """[{signal: count}] per point: only the occupied slots reach Python.  With `letters` the keys are joint keys."""
    keys, counts = tables["keys"].cpu().numpy().view(np.uint64), tables["counts"].cpu().numpy()
    out = []
    for k in range(keys.shape[0]):
        at = np.flatnonzero(keys[k] != NS.EMPTY)
        signals = [H.signal_of_key(key) for key in keys[k][at].tolist()] if letters is None else H.joint_signals_of_keys(letters, keys[k][at])
        out.append(dict(zip(signals, counts[k][at].tolist())))
    return out


# ---- the host path ----

def _sweep_host(sequence, labels, num_mocks, num_edmans, points, n, seed, first_molecule, stride, fit, max_possible, allow_multidrop,
                max_deviation, quench_factors, fixed):
    """The sweep through the host twins, a point at a time: simulation_records(host=True), the restated fit of
    simulate_peptide.host_fit, the twin's tally."""
    from . import _host_lognormal
    base, values, keys = _point_params(sequence, labels, num_mocks, num_edmans, seed, first_molecule, points, fixed)
    sims, totals, nones = {}, {}, {}
    if fit:
        means = _tracks.log_fluor_means(fixed['beta'], quench_factors, max_possible)
    for k, key in enumerate(keys):
        ep = {x: v for x, v in fixed.items() if x != 'b'}
        ep.update(zip(("p", "per_cycle_b", "u", "s", "s2"), values[k].tolist()))
        rec = PS.simulation_records(sequence, labels, num_mocks, num_edmans, n, seed, first_molecule + k * stride, host=True, **ep)
        kept = np.flatnonzero(rec["category"] != 0)
        rows = rec["counts"][kept]
        (mol,), _, unkeyed = H.tally_rows(rows, np.zeros(len(rows), np.int32), None, 1)
        signals, total, none_count = ({}, len(kept), 0) if fit else (None, len(kept), None)
        if fit and len(kept):
            fits = [_host_lognormal.intensities_to_signal(rec["intensity"][i].tolist(), fixed['beta_sigma'], max_possible, allow_multidrop,
                                                          max_deviation, tuple(c != 0 for c in rec["counts"][i].tolist()), means)
                    for i in kept.tolist()]
            best = [f[2] for f in fits if f[2] is not None]
            none_count = len(fits) - len(best)
            (signals,), _, more = H.tally_rows(np.array(best, np.uint8).reshape(len(best), rows.shape[1]),
                                               np.zeros(len(best), np.int32), None, 1)
            unkeyed[0] += more[0]
            signals = {H.signal_of_key(x): c for x, c in signals.items()}
        if unkeyed[0]:
            raise NotImplementedError("point %d has signals with more than %d drops, or that start above 15 dyes" % (k, H.MAX_DROPS))
        sims[key] = (signals, {H.signal_of_key(x): c for x, c in mol.items()})
        totals[key], nones[key] = total, none_count
    return {"points": keys, "all_simulations": sims, "total_count": totals, "none_count": nones}


def sweep_records(sequence, labels, num_mocks, num_edmans, points, num_simulations, seed=0, first_molecule=0, molecule_stride=0,
                  fit=True, max_possible=5, allow_multidrop=True, max_deviation=3, quench_factors=None, solver=None, table_slots=1024,
                  chunk_rows=1 << 22, device=None, host=False, **fixed_parameters):
    """sweep_device's result as the reference's dicts: `all_simulations` {point: (signals, molecular_signals)} as
    jupyter_development.py collects the pickles of simulate_peptide.py, `total_count` and `none_count` {point: n}, and `points`
    in grid order.  host=True: the same through the host twins, without a GPU."""
    if host:
        n, stride, _, _ = _check_sweep_shape(num_simulations, molecule_stride, table_slots, chunk_rows)
        return _sweep_host(sequence, labels, num_mocks, num_edmans, points, n, seed, first_molecule, stride, fit, max_possible,
                           allow_multidrop, max_deviation, quench_factors, fixed_parameters)
    sweep = sweep_device(sequence, labels, num_mocks, num_edmans, points, num_simulations, seed, first_molecule, molecule_stride, fit,
                         max_possible, allow_multidrop, max_deviation, quench_factors, solver, table_slots, chunk_rows, device,
                         **fixed_parameters)
    return records_of_sweep(sweep)


def records_of_sweep(sweep):
    """sweep_records' dict of sweep_device's."""
    keys = sweep["points"]
    letters = _codec(sweep)[2]
    mol = _decode_tables(sweep["molecular"], letters)
    sig = _decode_tables(sweep["signals"], letters) if sweep["signals"] is not None else [None] * len(keys)
    total = sweep["total_count"].cpu().tolist()
    none = sweep["none_count"].cpu().tolist() if sweep["none_count"] is not None else [None] * len(keys)
    out = {"points": keys, "all_simulations": {key: (sig[k], mol[k]) for k, key in enumerate(keys)},
           "total_count": dict(zip(keys, total)), "none_count": dict(zip(keys, none))}
    if letters is not None:
        out["labels"] = letters
    return out


# ---- sweeps over several label letters: joint signals (include/fsq_signal_sweep.h, THE JOINT KEY) ----
# A joint signal is peptide_simulator.joint_signal's (decrements, zeros, starts), a definition of this package.  Its limits:
# at most 4 letters, D(K) = 10, 8, 6, 6 drops over all channels, a channel starts at 15 dyes or fewer.

def _joint_point_params(sequence, labels, num_mocks, num_edmans, seed, first_molecule, points, fixed):
    """_point_params for several letters: (the base FsqPeptideLabelsParams, float64 [P][5], the points as dict keys, the
    sorted letters), every point through peptide_simulator._labels_params."""
    points = list(points)
    if not points:
        raise ValueError("at least one point is needed")
    values, base, letters = np.empty((len(points), 5)), None, None
    for k, point in enumerate(points):
        ep = dict(fixed)
        ep.update(_point_dict(point))
        if 'per_cycle_b' in ep and 'b' in _point_dict(point):
            del ep['per_cycle_b']
        prm, meta = PS._labels_params(sequence, labels, num_mocks, num_edmans, seed, first_molecule, ep)
        values[k] = (prm.p, prm.per_cycle_b, prm.u, prm.s, prm.s2)
        base, letters = base or prm, meta["labels"]
    keys = [tuple(sorted(p.items())) if isinstance(p, dict) else tuple(p) for p in points]
    if len(set(keys)) != len(keys):
        raise ValueError("a point stands twice")
    return base, values, keys, letters


def simulate_labels_points_device(prm, d_points, n_points, n_per_point, molecule_stride=0, first_row=0, n_rows=None):
    """fsq_peptide_simulate_labels_points: counts uint8 [K, n_rows, frames], intensity float64 [K, n_rows, frames] and category
    int64 [K, n_rows] of rows first_row .. first_row + n_rows - 1 of the flattened [n_points][n_per_point] space, channel-major;
    prm is a FsqPeptideLabelsParams, d_points a float64 CUDA tensor [n_points, 5] of (p, per_cycle_b, u, s, s2).  Enqueued on
    the current stream, not synchronised."""
    torch = _engine._torch()
    if d_points.dtype != torch.float64 or tuple(d_points.shape) != (int(n_points), 5) or not d_points.is_contiguous():
        raise ValueError("a contiguous float64 tensor [n_points, 5] is needed")
    n = int(n_points) * int(n_per_point) - int(first_row) if n_rows is None else int(n_rows)
    dev, K, F = d_points.device, prm.n_channels, prm.num_mocks + prm.num_edmans + 1
    out = {"counts": torch.empty((K, max(n, 0), F), dtype=torch.uint8, device=dev),
           "intensity": torch.empty((K, max(n, 0), F), dtype=torch.float64, device=dev),
           "category": torch.empty((K, max(n, 0)), dtype=torch.int64, device=dev)}
    _engine.launch(NS.lib().fsq_peptide_simulate_labels_points, "fsq_peptide_simulate_labels_points", dev, ctypes.byref(prm),
                   d_points.data_ptr(), int(n_points), int(n_per_point), int(molecule_stride), int(first_row), n,
                   *[out[k].data_ptr() if out[k].numel() else None for k in ("counts", "intensity", "category")])
    return out


def tally_joint_device(tables, d_rows, d_point, d_valid=None):
    """fsq_signal_tally_joint: adds the joint signals of uint8 [K, n, frames] rows (channel-major, K = 1 .. 4) to the tables of
    their points (int32 [n]); d_valid uint8 [n] or None.  The tables are new_tables'.  Enqueued, not synchronised."""
    torch = _engine._torch()
    if d_rows.dim() != 3:
        raise ValueError("uint8 rows [K, n, frames] are needed")
    K, n, frames = (int(x) for x in d_rows.shape)
    if d_rows.dtype != torch.uint8 or d_point.dtype != torch.int32 or tuple(d_point.shape) != (n,):
        raise ValueError("uint8 rows [K, n, frames] and int32 points [n] are needed")
    if d_valid is not None and (d_valid.dtype != torch.uint8 or tuple(d_valid.shape) != (n,)):
        raise ValueError("a uint8 mask [n] is needed")
    if not 1 <= frames <= NS.MAX_FRAMES or not 1 <= K <= H.MAX_CHANNELS:
        raise ValueError("rows have 1 .. %d frames and 1 .. %d channels" % (NS.MAX_FRAMES, H.MAX_CHANNELS))
    if not (d_rows.is_contiguous() and d_point.is_contiguous() and (d_valid is None or d_valid.is_contiguous())):
        raise ValueError("contiguous tensors are needed")
    n_points, slots = (int(x) for x in tables["keys"].shape)
    _engine.launch(NS.lib().fsq_signal_tally_joint, "fsq_signal_tally_joint", d_rows.device, d_rows.data_ptr() if n else None, K, frames,
                   d_point.data_ptr() if n else None, None if d_valid is None or not n else d_valid.data_ptr(), n, n_points, slots,
                   tables["keys"].data_ptr(), tables["counts"].data_ptr(), tables["none"].data_ptr(), tables["unkeyed"].data_ptr(),
                   tables["overflow"].data_ptr())


def _joint_fit_means(letters, fixed, quench_factors, max_possible):
    """Per letter (log_fluor_means, beta_sigma): beta, beta_sigma and quench_factors are one value for all letters or a dict
    {letter: value}, as peptide_simulator.multilabel_and_fit_records takes them."""
    betas, sigmas = PS._per_letter(fixed, 'beta', letters, None), PS._per_letter(fixed, 'beta_sigma', letters, None)
    quench = PS._per_letter({'quench_factors': quench_factors}, 'quench_factors', letters, None)
    return [(_tracks.log_fluor_means(betas[k], quench[k], max_possible), sigmas[k]) for k in range(len(letters))]


def joint_sweep_device(sequence, labels, num_mocks, num_edmans, points, num_simulations, seed=0, first_molecule=0, molecule_stride=0,
                       fit=True, max_possible=5, allow_multidrop=True, max_deviation=3, quench_factors=None, solver=None,
                       table_slots=1024, chunk_rows=1 << 22, device=None, **fixed_parameters):
    """sweep_device for up to 4 label letters, one colour channel each: the tables hold joint signals under the joint key.
    beta, beta_sigma, ddif, superdye_rate, superdye_factor and quench_factors are one value for all letters or a dict {letter:
    value}.  Per chunk of at most chunk_rows rows (the result does not depend on it): simulate (fsq_peptide_simulate_labels_points);
    tally the molecules with any lit channel into `molecular`; per channel fit the molecules whose channel is lit with
    lognormal.lognormal_device under that letter's parameters, best_seq into a zeroed [K, rows, frames] buffer so that a dark
    channel stays a row of zeros; tally into `signals` every molecule with a lit channel whose lit channels were all found.
    total_count: the molecules with a lit channel; none_count: total_count minus the tallied ones.  Returns sweep_device's dict
    plus `labels`, the sorted letters."""
    torch = _engine._torch()
    from . import lognormal as LN
    n, stride, slots, chunk = _check_sweep_shape(num_simulations, molecule_stride, table_slots, chunk_rows)
    base, values, keys, letters = _joint_point_params(sequence, labels, num_mocks, num_edmans, seed, first_molecule, points,
                                                      fixed_parameters)
    P, K, F = len(keys), len(letters), base.num_mocks + base.num_edmans + 1
    dev = torch.device(device or "cuda")
    fit_kw = []
    if fit:
        fit_kw = [dict(prm=LN.fit_params(means, sigma, max_possible, allow_multidrop, max_deviation, LN.DEFAULT_BUDGET),
                       **LN._solver_kw(solver or 'enumerate'))
                  for means, sigma in _joint_fit_means(letters, fixed_parameters, quench_factors, max_possible)]
        if not allow_multidrop and F == 1:
            raise ValueError("max() arg is an empty sequence")        # (as lognormal.photometries_lognormal_fit, :5442)
    d_points = torch.from_numpy(values).to(dev)
    molecular, signals = new_tables(P, slots, dev), new_tables(P, slots, dev) if fit else None
    total, found_n = torch.zeros(P, dtype=torch.int64, device=dev), torch.zeros(P, dtype=torch.int64, device=dev)
    bad = torch.zeros((), dtype=torch.bool, device=dev)
    for first in range(0, P * n, chunk):
        rows = min(chunk, P * n - first)
        sim = simulate_labels_points_device(base, d_points, P, n, stride, first, rows)
        d_point = torch.div(torch.arange(first, first + rows, device=dev), n, rounding_mode="floor").to(torch.int32)
        lit = (sim["category"] != 0).any(dim=0)
        tally_joint_device(molecular, sim["counts"], d_point, lit.to(torch.uint8))
        total += torch.bincount(d_point[lit], minlength=P)
        if not fit:
            continue
        best, ok = torch.zeros((K, rows, F), dtype=torch.uint8, device=dev), lit.clone()
        for k in range(K):
            at = (sim["category"][k] != 0).nonzero().reshape(-1)
            kept = int(at.shape[0])
            if not kept:
                continue
            d_len = torch.full((kept,), F, dtype=torch.int32, device=dev)
            out = LN.lognormal_device(sim["intensity"][k][at].contiguous(), sim["category"][k][at].contiguous(), d_len, None, None,
                                      **fit_kw[k])
            found = out["status"] == LN.STATUS_FOUND
            bad |= (out["status"] > LN.STATUS_NONE).any()
            best[k][at[found]] = out["best_seq"][found]
            ok[at[~found]] = False
        tally_joint_device(signals, best, d_point, ok.to(torch.uint8))
        found_n += torch.bincount(d_point[ok], minlength=P)
    if bool(bad):
        raise NotImplementedError("a simulated track has more surviving sequences than the budget, or an invalid length")
    _check_tables(molecular, "molecular joint signals", slots, NS.JOINT_MAX_DROPS[K])
    if fit:
        _check_tables(signals, "fitted joint signals", slots, NS.JOINT_MAX_DROPS[K])
    return {"points": keys, "molecular": molecular, "signals": signals, "total_count": total,
            "none_count": total - found_n if fit else None, "num_simulations": n, "table_slots": slots, "labels": letters}


def _host_joint_fits(intensity, category, counts, fits_of, allow_multidrop, max_deviation, max_possible):
    """(best uint8 [K][m][F], ok bool [m]) of the host lognormal fit of every lit channel of m molecules: a dark channel stays a
    row of zeros, ok is False where a lit channel was not found.  fits_of[k] is (log_fluor_means, beta_sigma)."""
    from . import _host_lognormal
    K, m, F = counts.shape
    best, ok = np.zeros((K, m, F), np.uint8), np.ones(m, bool)
    for k in range(K):
        means, sigma = fits_of[k]
        for i in np.flatnonzero(category[k] != 0).tolist():
            f = _host_lognormal.intensities_to_signal(intensity[k][i].tolist(), sigma, max_possible, allow_multidrop, max_deviation,
                                                      tuple(c != 0 for c in counts[k][i].tolist()), means)
            if f[2] is None:
                ok[i] = False
            else:
                best[k][i] = f[2]
    return best, ok


def _joint_sweep_host(sequence, labels, num_mocks, num_edmans, points, n, seed, first_molecule, stride, fit, max_possible,
                      allow_multidrop, max_deviation, quench_factors, fixed):
    """The joint sweep through the host twins, a point at a time: multilabel_records(host=True), the restated fit, the twin's
    joint tally."""
    base, values, keys, letters = _joint_point_params(sequence, labels, num_mocks, num_edmans, seed, first_molecule, points, fixed)
    K = len(letters)
    sims, totals, nones = {}, {}, {}
    fits_of = _joint_fit_means(letters, fixed, quench_factors, max_possible) if fit else None
    decode = lambda table: {H.joint_signal_of_key(letters, x): c for x, c in table.items()}         # noqa: E731
    for k, key in enumerate(keys):
        ep = {x: v for x, v in fixed.items() if x != 'b'}
        ep.update(zip(("p", "per_cycle_b", "u", "s", "s2"), values[k].tolist()))
        rec = PS.multilabel_records(sequence, labels, num_mocks, num_edmans, n, seed, first_molecule + k * stride, host=True, **ep)
        lit = np.flatnonzero((rec["category"] != 0).any(axis=0))
        counts = rec["counts"][:, lit]
        zero = np.zeros(len(lit), np.int32)
        (mol,), _, unkeyed = H.tally_joint_rows(counts, zero, None, 1)
        signals, none_count = ({}, 0) if fit else (None, None)
        if fit and len(lit):
            best, ok = _host_joint_fits(rec["intensity"][:, lit], rec["category"][:, lit], counts, fits_of, allow_multidrop,
                                        max_deviation, max_possible)
            (signals,), _, more = H.tally_joint_rows(best, zero, ok, 1)
            unkeyed[0] += more[0]
            signals, none_count = decode(signals), int(len(lit) - ok.sum())
        if unkeyed[0]:
            raise NotImplementedError("point %d has joint signals with more than %d drops, or that start above 15 dyes"
                                      % (k, H.JOINT_MAX_DROPS[K]))
        sims[key] = (signals, decode(mol))
        totals[key], nones[key] = len(lit), none_count
    return {"points": keys, "all_simulations": sims, "total_count": totals, "none_count": nones, "labels": letters}


def joint_sweep_records(sequence, labels, num_mocks, num_edmans, points, num_simulations, seed=0, first_molecule=0, molecule_stride=0,
                        fit=True, max_possible=5, allow_multidrop=True, max_deviation=3, quench_factors=None, solver=None,
                        table_slots=1024, chunk_rows=1 << 22, device=None, host=False, **fixed_parameters):
    """joint_sweep_device's result as sweep_records gives sweep_device's: `all_simulations` {point: (signals,
    molecular_signals)} keyed by joint signals, `total_count`, `none_count`, `points` and `labels`.  host=True: the same through
    multilabel_records(host=True), the host lognormal fit and the twin's joint tally, without a GPU."""
    if host:
        n, stride, _, _ = _check_sweep_shape(num_simulations, molecule_stride, table_slots, chunk_rows)
        return _joint_sweep_host(sequence, labels, num_mocks, num_edmans, points, n, seed, first_molecule, stride, fit, max_possible,
                                 allow_multidrop, max_deviation, quench_factors, fixed_parameters)
    return records_of_sweep(joint_sweep_device(sequence, labels, num_mocks, num_edmans, points, num_simulations, seed, first_molecule,
                                               molecule_stride, fit, max_possible, allow_multidrop, max_deviation, quench_factors,
                                               solver, table_slots, chunk_rows, device, **fixed_parameters))


def joint_signals_of_fits(letters, best_seq, found, category, host=False, table_slots=1024, device=None):
    """The observed side of a joint sweep: {joint_signal: n} of row-aligned per-channel lognormal fits of the same tracks.
    best_seq uint8 [K][n][F], found and category [K][n] (non-zero: the channel's fit was found; the channel is lit), NumPy
    arrays or tensors, the channels in sorted-letter order.  A track counts when it has a lit channel and every lit channel was
    found; a dark channel counts as a row of zeros.  Through fsq_signal_tally_joint, or the twin with host=True.  From a
    two-channel track table: colocalize.joint_observed_records, which aligns the channels' tracks and calls this."""
    letters = tuple(letters)
    if host:
        best, found, category = (np.asarray(x.cpu() if hasattr(x, "cpu") else x) for x in (best_seq, found, category))
        lit = category != 0
        ok = lit.any(axis=0) & ~(lit & (found == 0)).any(axis=0)
        rows = np.where(lit[:, :, None], best, 0).astype(np.uint8)
        (table,), _, unkeyed = H.tally_joint_rows(rows, np.zeros(rows.shape[1], np.int32), ok, 1)
        if unkeyed[0]:
            raise NotImplementedError("tracks with more than %d drops, or that start above 15 dyes: they have no 64-bit key"
                                      % H.JOINT_MAX_DROPS[len(letters)])
        return {H.joint_signal_of_key(letters, x): c for x, c in table.items()}
    torch = _engine._torch()
    dev = torch.device(device or "cuda")
    best, found, category = (torch.as_tensor(x).to(dev) for x in (best_seq, found, category))
    lit = category != 0
    ok = lit.any(dim=0) & ~(lit & (found == 0)).any(dim=0)
    rows = torch.where(lit[:, :, None], best, torch.zeros_like(best)).to(torch.uint8).contiguous()
    tables = new_tables(1, int(table_slots), dev)
    tally_joint_device(tables, rows, torch.zeros(int(rows.shape[1]), dtype=torch.int32, device=dev), ok.to(torch.uint8))
    _check_tables(tables, "joint signals", int(table_slots), NS.JOINT_MAX_DROPS[len(letters)])
    return _decode_tables(tables, letters)[0]


def joint_split_heatmap(letters, num_cycles, cycle):
    """split_heatmap for joint signals: the heat-map signals - one or two single drops that leave every channel at zero -
    whose last drop is before `cycle`, and the others, as two tuples; each the single drops by (cycle, letter), then the
    double drops by their last, then their first drop."""
    letters = tuple(letters)
    drops = [(c, k) for c in range(1, num_cycles + 1) for k in range(len(letters))]

    def signal(ds):
        starts = tuple(sum(1 for _, k in ds if k == j) for j in range(len(letters)))
        return tuple((letters[k], c) for c, k in ds), (True,) * len(letters), starts
    each = [(ds[-1][0], signal(ds)) for ds in [(d,) for d in drops] + [(a, b) for b in drops for a in drops if a < b]]
    return tuple(s for last, s in each if last < cycle), tuple(s for last, s in each if last >= cycle)


# ---- scoring ----

def _score_options(kw):
    unknown = set(kw) - set(_SCORE_KW) - {"matching_p", "print_included_signals", "euclidean_weights"}
    if unknown:
        raise TypeError("unexpected keyword %r" % sorted(unknown)[0])
    return {k: v for k, v in kw.items() if k in _SCORE_KW}


def _scores_on_device(table, d_fit, d_fit_total, metric, normalization, small_count_cutoff, contributions):
    torch = _engine._torch()
    dev = d_fit.device
    S, P = (int(x) for x in d_fit.shape)
    prm = NS.FsqScoreParams()
    prm.n_observed, prm.metric, prm.normalization = table["n_observed"], H.check_metric(metric), normalization
    prm.has_cutoff, prm.small_count_cutoff = (0, 0.0) if small_count_cutoff is None else (1, float(small_count_cutoff))
    d = {k: torch.from_numpy(table[k]).to(dev) for k in ("observed", "in_observed", "admitted", "heatmap")}
    out = {"score": torch.empty(P, dtype=torch.float64, device=dev), "factor": torch.empty(P, dtype=torch.float64, device=dev),
           "status": torch.empty(P, dtype=torch.int32, device=dev),
           "contributions": torch.empty((S, P), dtype=torch.float64, device=dev) if contributions else None}
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None       # noqa: E731
    _engine.launch(NS.lib().fsq_signal_scores, "fsq_signal_scores", dev, ptr(d["observed"]), ptr(d["in_observed"]), ptr(d["admitted"]),
                   ptr(d["heatmap"]), ptr(d_fit), d_fit_total.data_ptr(), S, P, ctypes.byref(prm), out["score"].data_ptr(),
                   out["factor"].data_ptr(), out["status"].data_ptr(), ptr(out["contributions"]))
    out["signals"] = table["signals"]
    return out


def _counts_on_host(observed_signals, sweep, molecular):
    """(the ordered signals, the count matrix int64 [S, P], the points' totals int64 [P]) of sweep_records' dict, or of
    joint_sweep_records' (it carries `labels`, and the order is then the joint key's)."""
    dicts = [sweep["all_simulations"][key][1 if molecular else 0] for key in sweep["points"]]
    signals = H.ordered_signals(set(observed_signals).union(*dicts), _codec(sweep)[2])
    return (signals,) + H.fit_matrix(signals, dicts)


def _counts_on_device(observed_signals, sweep, molecular, device):
    """(the ordered signals of the observed dict and every point's dict, the count matrix int64 [S, P] and the points' totals
    int64 [P] as CUDA tensors) of sweep_device's dict (its tables are read where they are) or sweep_records'."""
    torch = _engine._torch()
    key_of_signal, signal_of_key, letters = _codec(sweep)
    if "all_simulations" in sweep:
        signals, fit, fit_total = _counts_on_host(observed_signals, sweep, molecular)
        dev = torch.device(device or "cuda")
        return signals, torch.from_numpy(fit).to(dev), torch.from_numpy(fit_total).to(dev)
    tables = sweep["molecular" if molecular else "signals"]
    if tables is None:
        raise ValueError("the sweep was run with fit=False: pass molecular=True")
    occupied = torch.unique(tables["keys"][tables["keys"] != NS.EMPTY]).cpu().tolist()
    signals = H.ordered_signals(set(observed_signals) | {signal_of_key(k) for k in occupied}, letters)
    wanted = [key_of_signal(s) for s in signals]
    d_wanted = torch.from_numpy(np.array([NS.NEVER if k is None else k for k in wanted], np.uint64).view(np.int64)).to(tables["keys"].device)
    d_fit, d_total = lookup_device(tables, d_wanted), tables["counts"].sum(dim=1)
    if int(d_total.max()) > NS.MAX_COUNT:
        raise NotImplementedError("counts beyond 2^31 - 1")
    return signals, d_fit, d_total


def score_device(observed_signals, sweep, metric='naive', normalize_counts=False, heatmap_normalize_counts=False,
                 small_count_cutoff=None, contributions=True, molecular=False, device=None, **kw):
    """signal_correlation of observed_signals against every point of a sweep, on the device: a dict of CUDA tensors score and
    factor float64 [P], status int32 [P] (0 ok, 1 nothing pairs, 2 ZeroDivisionError, 3 ValueError), contributions float64
    [S, P] (NaN: none) or None, and `signals`, the S signals in the order of the sums.  `sweep` is sweep_device's dict (its
    tables are read where they are) or sweep_records' (its dicts are uploaded as a count matrix); molecular=True scores the
    molecular signals instead of the fitted ones.  The keywords are signal_correlation's."""
    opts, norm = _score_options(kw), H.normalization_of(normalize_counts, heatmap_normalize_counts)
    H.check_metric(metric)
    signals, d_fit, d_total = _counts_on_device(observed_signals, sweep, molecular, device)
    table = H.key_table(observed_signals, signals, **opts)
    return _scores_on_device(table, d_fit, d_total, metric, norm, small_count_cutoff, contributions)


def score_records(observed_signals, sweep, metric='naive', normalize_counts=False, heatmap_normalize_counts=False,
                  small_count_cutoff=None, contributions=True, molecular=False, host=False, on_error='raise', device=None, **kw):
    """{point: (result, (normalization_factor, contributions))} as match_diagnostic's all_correlations (:921-936).  A point at
    which the reference raises (a heatmap total of zero, a zero variance) raises here as well, or with on_error='none' gets the
    result None.  host=True: the NumPy twin (sweep_records' dict is then needed)."""
    if on_error not in ('raise', 'none'):
        raise ValueError("on_error must be 'raise' or 'none'")
    if host:
        opts, norm = _score_options(kw), H.normalization_of(normalize_counts, heatmap_normalize_counts)
        signals, fit, fit_total = _counts_on_host(observed_signals, sweep, molecular)
        score, factor, status, contrib = H.scores(H.key_table(observed_signals, signals, **opts), fit, fit_total, metric, norm,
                                                  small_count_cutoff, contributions)
    else:
        out = score_device(observed_signals, sweep, metric, normalize_counts, heatmap_normalize_counts, small_count_cutoff,
                           contributions, molecular, device, **kw)
        signals = out["signals"]
        score, factor, status = (out[k].cpu().numpy() for k in ("score", "factor", "status"))
        contrib = out["contributions"].cpu().numpy() if contributions else None
    results = {}
    for k, key in enumerate(sweep["points"]):
        if on_error == 'none' and status[k] in (H.SCORE_DIVZERO, H.SCORE_DOMAIN):
            results[key] = (None, (None, {}))
        else:
            results[key] = H.result_of(signals, score, factor, status, contrib, k)
    return results


def best_point(scores, reverse_order=False):
    """(point, result, normalization_factor, contributions) of the best point of score_records' dict, as match_diagnostic takes
    it (:938-948): the smallest result, or with reverse_order the largest.  Ties go to the first point in grid order; a point
    whose result is None is never chosen."""
    best = None
    for key, (result, (factor, contrib)) in scores.items():
        if result is None:
            continue
        if best is None or (result > best[1] if reverse_order else result < best[1]):
            best = (key, result, factor, contrib)
    if best is None:
        raise ValueError("no point has a result")
    return best


def signal_correlation(observed_signals, fit_signals, heatmap_only=True, zero_only=True, metric='naive', normalize_counts=False,
                       matching_p=0.10, exclude_signals=None, print_included_signals=False, select_signals=None,
                       heatmap_normalize_counts=False, allow_multidrop=False, small_count_cutoff=None, euclidean_weights=None,
                       host=False, device=None):
    """jupyter_development.signal_correlation (:279-578) for one pair of dicts: (result, (normalization_factor,
    contributions)).  A fit signal counts as present when its count is positive.  host=True runs the NumPy twin without a GPU."""
    sweep = {"points": [0], "all_simulations": {0: (fit_signals, None)}}
    return score_records(observed_signals, sweep, metric, normalize_counts, heatmap_normalize_counts, small_count_cutoff, True, False,
                         host, 'raise', device, heatmap_only=heatmap_only, zero_only=zero_only, exclude_signals=exclude_signals,
                         select_signals=select_signals, allow_multidrop=allow_multidrop)[0]


# ---- match_diagnostic: the incompatibility scores of signal pairs (jupyter_development.py:786-1259) ----

def split_heatmap(num_cycles, cycle):
    """jupyter_development.split_heatmap (:227-248): the heat-map signals whose last drop is before `cycle`, and the others,
    as two tuples; each the single drops ((('A', c),), True, 1) by c, then the double drops ((('A', b), ('A', c)), True, 2) by
    c, then b."""
    singles = [((('A', c),), True, 1) for c in range(1, num_cycles + 1)]
    doubles = [((('A', b), ('A', c)), True, 2) for c in range(1, num_cycles + 1) for b in range(1, c)]
    last = lambda sig: sig[0][-1][1]                                                   # noqa: E731
    return (tuple(s for s in singles + doubles if last(s) < cycle), tuple(s for s in singles + doubles if last(s) >= cycle))


def py2_round(x):
    """Python 2's round(x): to the nearest integer, halves away from zero, as a float."""
    x = float(x)
    whole = math.floor(abs(x))
    return math.copysign(whole + (1.0 if abs(x) - whole >= 0.5 else 0.0), x)       # (abs(x) - whole is exact)


def py2_round2(x):
    """Python 2's round(x, 2): the exact value of the float to two decimals, halves away from zero (0.125 -> 0.13, where
    Python 3 gives 0.12; 2.675, a little below the half, -> 2.67 in both)."""
    x = float(x)
    if x != x or x in (float("inf"), float("-inf")):
        return x
    return float(decimal.Decimal(x).quantize(decimal.Decimal("0.01"), rounding=decimal.ROUND_HALF_UP))


def _candidates(select_signals, num_cycles):
    if select_signals is None:
        if num_cycles is None:
            raise ValueError("num_cycles or select_signals is needed")
        select_signals = split_heatmap(int(num_cycles), 0)[1]
    L = list(select_signals)
    if len(set(L)) != len(L):
        raise ValueError("a candidate signal stands twice")
    if not 2 <= len(L) <= H.MAX_SEL:
        raise ValueError("2 .. %d candidate signals are needed, not %d" % (H.MAX_SEL, len(L)))
    return L


def _candidate_rows(signals, L):
    index = {s: i for i, s in enumerate(signals)}
    return np.array([index.get(s, -1) for s in L], np.int32)


def pair_best_device(table, rows, d_fit, d_fit_total, metric, normalization=0, small_count_cutoff=None, reverse_order=False):
    """fsq_signal_pair_best for the candidates whose rows in the key table are `rows` (int32 [n_sel], -1: in no dict), over the
    count matrix d_fit int64 [S, P] and the totals d_fit_total int64 [P] on the device: a dict of CUDA tensors best_point int32
    [K], result and factor float64 [K], dist float64 [K, 2], error_point and error_status int32 [K].  Under
    heatmap_normalize_counts the points' heat-map factor comes from one fsq_signal_scores call with nothing admitted."""
    torch = _engine._torch()
    dev = d_fit.device
    S, P = (int(x) for x in d_fit.shape)
    rows = np.ascontiguousarray(rows, np.int32)
    n_sel = int(rows.shape[0])
    if rows.ndim != 1 or not 2 <= n_sel <= NS.MAX_SEL:
        raise ValueError("2 .. %d candidate rows are needed" % NS.MAX_SEL)
    prm = NS.FsqScoreParams()
    prm.n_observed, prm.metric, prm.normalization = table["n_observed"], H.check_metric(metric), normalization
    prm.has_cutoff, prm.small_count_cutoff = (0, 0.0) if small_count_cutoff is None else (1, float(small_count_cutoff))
    heat = None
    if normalization & NS.HEATMAP_NORMALIZE_COUNTS:
        heat = _scores_on_device(dict(table, admitted=np.zeros_like(table["admitted"])), d_fit, d_fit_total, H.METRICS[0],
                                 NS.HEATMAP_NORMALIZE_COUNTS, None, False)
    d = {k: torch.from_numpy(table[k]).to(dev) for k in ("observed", "in_observed", "admitted")}
    d_rows = torch.from_numpy(rows).to(dev)
    K = n_sel * (n_sel - 1) // 2
    out = {"best_point": torch.empty(K, dtype=torch.int32, device=dev), "result": torch.empty(K, dtype=torch.float64, device=dev),
           "factor": torch.empty(K, dtype=torch.float64, device=dev), "dist": torch.empty((K, 2), dtype=torch.float64, device=dev),
           "error_point": torch.empty(K, dtype=torch.int32, device=dev), "error_status": torch.empty(K, dtype=torch.int32, device=dev)}
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None       # noqa: E731
    _engine.launch(NS.lib().fsq_signal_pair_best, "fsq_signal_pair_best", dev, ptr(d["observed"]), ptr(d["in_observed"]),
                   ptr(d["admitted"]), ptr(d_fit), d_fit_total.data_ptr(), S, P, ctypes.byref(prm), d_rows.data_ptr(), n_sel,
                   int(bool(reverse_order)), heat["factor"].data_ptr() if heat else None, heat["status"].data_ptr() if heat else None,
                   *[out[k].data_ptr() for k in ("best_point", "result", "factor", "dist", "error_point", "error_status")])
    return out


def pair_extremes_device(d_dist, n_sel, reverse_order=False):
    """fsq_signal_pair_extremes: (score float64 [n_sel], n_distances int32 [n_sel]) of fsq_signal_pair_best's dist."""
    torch = _engine._torch()
    n_sel = int(n_sel)
    if d_dist.dtype != torch.float64 or not d_dist.is_contiguous() or not 2 <= n_sel <= NS.MAX_SEL \
            or d_dist.numel() != n_sel * (n_sel - 1):
        raise ValueError("a contiguous float64 tensor [n_sel (n_sel - 1) / 2, 2] is needed, 2 <= n_sel <= %d" % NS.MAX_SEL)
    score = torch.empty(n_sel, dtype=torch.float64, device=d_dist.device)
    n = torch.empty(n_sel, dtype=torch.int32, device=d_dist.device)
    _engine.launch(NS.lib().fsq_signal_pair_extremes, "fsq_signal_pair_extremes", d_dist.device, d_dist.data_ptr(), n_sel,
                   int(bool(reverse_order)), score.data_ptr(), n.data_ptr())
    return score, n


def incompatibility_device(observed_signals, sweep, select_signals=None, num_cycles=None, metric='naive', normalize_counts=False,
                           heatmap_normalize_counts=False, small_count_cutoff=None, reverse_order=False, molecular=False,
                           device=None, **signal_correlation_keywords):
    """match_diagnostic's incompatibility loop (:833-889) on the device.  For every pair of the candidate signals - select_signals
    in its order, by default split_heatmap(num_cycles, 0)[1] - and every point of the sweep, signal_correlation with
    select_signals = the pair; per pair the best point, its result and factor and the two signals' contributions there; per
    signal the largest of its contributions over its pairs (the smallest with reverse_order), None skipped.  Returns a dict of
    CUDA tensors - best_point int32 [K] (-1: no point has a result), result, factor float64 [K], dist float64 [K, 2] (NaN:
    None), error_point, error_status int32 [K], score float64 [n_sel] (NaN: none), n_distances int32 [n_sel] - with `signals`
    (the candidates) and `points`.  Pairs stand in itertools.combinations' order.  `sweep` is sweep_device's or sweep_records'
    dict, as for score_device; the other keywords are signal_correlation's."""
    opts, norm = _score_options(signal_correlation_keywords), H.normalization_of(normalize_counts, heatmap_normalize_counts)
    if opts.get("select_signals") is not None:
        raise TypeError("select_signals is the candidate list")
    H.check_metric(metric)
    L = _candidates(select_signals, num_cycles)
    signals, d_fit, d_total = _counts_on_device(observed_signals, sweep, molecular, device)
    table = H.key_table(observed_signals, signals, **opts)
    out = pair_best_device(table, _candidate_rows(signals, L), d_fit, d_total, metric, norm, small_count_cutoff, reverse_order)
    out["score"], out["n_distances"] = pair_extremes_device(out["dist"], len(L), reverse_order)
    out["signals"], out["points"] = L, list(sweep["points"])
    return out


def incompatibility_records(observed_signals, sweep, select_signals=None, num_cycles=None, metric='naive', normalize_counts=False,
                            heatmap_normalize_counts=False, small_count_cutoff=None, reverse_order=False, molecular=False,
                            device=None, host=False, on_error='raise', pairs=True, **signal_correlation_keywords):
    """incompatibility_device's result in the reference's shapes: {"pairs": {(ss1, ss2): (point, (d1, d2), factor)} - its
    select_signal_distances (:872); a pair without a best point has (None, (None, None), None) - and "scores": {signal: value} -
    its max_incompatibilities (:887); a signal without a distance is left out}.  pairs=False leaves "pairs" out (None): at 2 *
    10^6 pairs the dict is the slow part.  Where a (pair, point) ends in the reference's ZeroDivisionError or ValueError,
    on_error='raise' raises it, naming the pair and the point, and on_error='none' takes that point as one without a result.
    host=True: the NumPy twin (sweep_records' dict is then needed)."""
    if on_error not in ('raise', 'none'):
        raise ValueError("on_error must be 'raise' or 'none'")
    if host:
        opts, norm = _score_options(signal_correlation_keywords), H.normalization_of(normalize_counts, heatmap_normalize_counts)
        if opts.get("select_signals") is not None:
            raise TypeError("select_signals is the candidate list")
        L = _candidates(select_signals, num_cycles)
        signals, fit, fit_total = _counts_on_host(observed_signals, sweep, molecular)
        out = H.pair_best(H.key_table(observed_signals, signals, **opts), _candidate_rows(signals, L), fit, fit_total, metric, norm,
                          small_count_cutoff, reverse_order)
        out["score"], out["n_distances"] = H.pair_extremes(out["dist"], len(L), reverse_order)
        points = list(sweep["points"])
    else:
        dev = incompatibility_device(observed_signals, sweep, select_signals, num_cycles, metric, normalize_counts,
                                     heatmap_normalize_counts, small_count_cutoff, reverse_order, molecular, device,
                                     **signal_correlation_keywords)
        L, points = dev["signals"], dev["points"]
        wanted = ("error_point", "error_status", "score") + (("best_point", "factor", "dist") if pairs else ())
        out = {k: dev[k].cpu().numpy() for k in wanted}
    n_sel = len(L)
    bad = np.flatnonzero(out["error_point"] >= 0)
    if on_error == 'raise' and len(bad):
        t = int(bad[0])
        i, j = next(itertools.islice(itertools.combinations(range(n_sel), 2), t, None))
        where = " (pair %r, point %r)" % ((L[i], L[j]), points[int(out["error_point"][t])])
        if int(out["error_status"][t]) == H.SCORE_DIVZERO:
            raise ZeroDivisionError("float division by zero" + where)
        raise ValueError("signal_correlation: the maximum of no contributions, or the root of a negative variance" + where)
    score = out["score"].tolist()
    result = {"pairs": None, "scores": {s: v for s, v in zip(L, score) if v == v}}
    if pairs:
        none = lambda v: v if v == v else None                                     # noqa: E731
        best, factor, dist = out["best_point"].tolist(), out["factor"].tolist(), out["dist"].tolist()
        result["pairs"] = {}
        for t, (i, j) in enumerate(itertools.combinations(range(n_sel), 2)):
            k = best[t]
            result["pairs"][(L[i], L[j])] = ((points[k], (none(dist[t][0]), none(dist[t][1])), factor[t]) if k >= 0
                                             else (None, (None, None), None))
    return result


def _cycles_header(num_mocks, num_edmans, num_mocks_omitted):
    return (["M" + str(i + 1 + num_mocks_omitted) for i in range(num_mocks - num_mocks_omitted)]
            + ["E" + str(i + 1) for i in range(num_edmans)])


def _one_letter_only(signals):
    if any(H.is_joint(s) for s in signals):
        raise NotImplementedError("the heat-map tables are built for one label letter, not for joint signals")


def single_drops_table(signals, num_mocks, num_edmans, num_mocks_omitted, plot_remainders=True, float_data=False):
    """The heatmap_array of single_drops_heatmap_v2 (:585-620) and its header: (int64 or float64 [1, cycles (+ 1)], the column
    names M.., E.., R).  Only signals that start at one dye or none count: a drop at cycle c that ends at zero in column c - 1,
    and with plot_remainders the dye that never drops in the last column.  float_data rounds to two decimals as Python 2
    does.  A cell written twice with a non-zero first value is the reference's AssertionError."""
    total_cycles = num_mocks - num_mocks_omitted + num_edmans
    size = total_cycles + 1 if plot_remainders else total_cycles
    array = np.zeros((1, size), np.float64 if float_data else np.int64)
    _one_letter_only(signals)
    for (signal, is_zero, starting_intensity), count in signals.items():
        if starting_intensity > 1 or len(signal) != 1:
            continue
        if tuple(signal) == H.NO_DROPS:
            if not plot_remainders or is_zero:
                continue
            y = size - 1
        elif not is_zero:
            continue
        else:
            y = signal[0][1] - 1
        assert array[0, y] == 0
        array[0, y] = py2_round2(count) if float_data else count
    return array, _cycles_header(num_mocks, num_edmans, num_mocks_omitted) + ["R"]


def double_drops_table(signals, num_mocks, num_edmans, num_mocks_omitted, plot_multidrops=False, plot_remainders=True,
                       float_data=False):
    """The heatmap_array of double_drops_heatmap_v2 (:674-713) and its headers: (int64 or float64 [cycles, cycles (+ 1)], the
    column names, the row names).  Only signals that start at two dyes or fewer count: drops at cycles b <= c that end at zero
    in cell [b - 1, c - 1] (b == c only with plot_multidrops), and with plot_remainders one drop at b that leaves a dye in
    the last column of row b - 1."""
    total_cycles = num_mocks - num_mocks_omitted + num_edmans
    size_x, size_y = total_cycles, total_cycles + 1 if plot_remainders else total_cycles
    array = np.zeros((size_x, size_y), np.float64 if float_data else np.int64)
    _one_letter_only(signals)
    for (signal, is_zero, starting_intensity), count in signals.items():
        if starting_intensity > 2:
            continue
        if len(signal) == 1:
            if tuple(signal) == H.NO_DROPS or not plot_remainders or is_zero:
                continue
            x, y = signal[0][1] - 1, size_y - 1
        elif len(signal) == 2:
            if (not plot_multidrops and len(signal) > len(set(signal))) or not is_zero:
                continue
            x, y = signal[0][1] - 1, signal[1][1] - 1
        else:
            continue
        assert array[x, y] == 0
        array[x, y] = py2_round2(count) if float_data else count
    rows = _cycles_header(num_mocks, num_edmans, num_mocks_omitted)
    return array, rows + ["R"] if plot_remainders else list(rows), rows


TABLE_NAMES = ("single_observed", "single_fit", "single_diff", "double_observed", "double_fit", "double_diff",
               "single_contributions", "single_molecular", "single_incompatibility",
               "double_contributions", "double_molecular", "double_incompatibility")


def check_diagnostic_options(normalize_counts, heatmap_normalize_counts, heatmap_only, allow_multidrop, incompatibility_threshold,
                             compute_incompatibility_scores):
    """match_diagnostic's three ValueErrors (:806-815)."""
    if normalize_counts == heatmap_normalize_counts:
        raise ValueError("normalize_counts == heatmap_normalize_counts")
    if heatmap_only and (not heatmap_normalize_counts or allow_multidrop):
        raise ValueError("If heatmap_only, then heatmap_normalize_counts and not allow_multidrop")
    if incompatibility_threshold is not None and not compute_incompatibility_scores:
        raise ValueError("If incompatibility_threshold is not None, then compute_incompatibility_scores")


def match_diagnostic(all_simulations, observed_signals, metric, reverse_order, normalize_counts, heatmap_normalize_counts,
                     heatmap_only, zero_only, allow_multidrop, small_count_cutoff, matching_p, split_cycle,
                     incompatibility_threshold, compute_incompatibility_scores, num_mocks, num_mocks_omitted, num_edmans,
                     num_cycles=None, apply_exclusion=False, host=False, on_error='raise', device=None):
    """jupyter_development.match_diagnostic (:786-1259) without its figure, its shelf file and its module-level cache.
    all_simulations is the reference's {point: (signals, molecular_signals)}, or sweep_records' or sweep_device's dict.  Returns
    a dict: optimal_pbu, result, normalization_factor and optimal_contributions of the best point (:921-948);
    normalized_plot_signals and normalized_plot_molecular_signals, its counts scaled to the observed total (:949-953);
    diff_plot_signals (:956-959); incompatibility_scores ({} when not computed); exclude_signals (:907-916); `tables`, the
    twelve heat-map arrays of :1005-1190 under TABLE_NAMES, and `z_ranges` (:993-1003; None where the reference's max() would
    have nothing to take).  reference_tuple() gives the reference's return value.  For a joint sweep (joint_sweep_device's or
    joint_sweep_records' dict, observed_signals keyed by joint signals) the candidates and the split are joint_split_heatmap's,
    and `tables`, `z_ranges` and `headers` are None: the heat-map tables stay one-letter (single_drops_table and
    double_drops_table raise NotImplementedError for joint signals).

    Where this differs from the reference, on purpose: the incompatibility loop scores `observed_signals`, not a notebook
    global (:846); num_cycles=None means num_mocks - num_mocks_omitted + num_edmans, the heat maps' own count (:590-591), not
    :805's num_mocks + num_mocks_omitted - num_edmans; the exclusion set is returned, and goes into the final scoring only
    with apply_exclusion=True (the reference prints it and passes None, :928).  As in the reference, allow_multidrop is
    checked (:808-812) and not passed on to signal_correlation (:845-859, :921-935)."""
    check_diagnostic_options(normalize_counts, heatmap_normalize_counts, heatmap_only, allow_multidrop, incompatibility_threshold,
                             compute_incompatibility_scores)
    sweep = all_simulations if "points" in all_simulations else {"points": list(all_simulations), "all_simulations": all_simulations}
    records = sweep if "all_simulations" in sweep else records_of_sweep(sweep)
    if num_cycles is None:
        num_cycles = num_mocks - num_mocks_omitted + num_edmans
    kw = dict(metric=metric, normalize_counts=normalize_counts, heatmap_normalize_counts=heatmap_normalize_counts,
              small_count_cutoff=small_count_cutoff, host=host, on_error=on_error, device=device, heatmap_only=heatmap_only,
              zero_only=zero_only, matching_p=matching_p)
    letters = _codec(sweep)[2]                                      # a joint sweep: its heat-map signals are joint_split_heatmap's
    split = split_heatmap if letters is None else (lambda cycles, cycle: joint_split_heatmap(letters, cycles, cycle))
    incompatibility_scores = {}
    if compute_incompatibility_scores:
        incompatibility_scores = incompatibility_records(observed_signals, records if host else sweep,
                                                         None if letters is None else split(num_cycles, 0)[1], num_cycles,
                                                         reverse_order=reverse_order, pairs=False, **kw)["scores"]
    exclude = set()
    if incompatibility_threshold is not None:
        exclude = {s for s, mi in incompatibility_scores.items() if mi > incompatibility_threshold}
    exclude_signals = exclude | set(split(num_cycles, split_cycle)[0])
    scores = score_records(observed_signals, records if host else sweep, exclude_signals=exclude_signals if apply_exclusion else None,
                           **kw)
    optimal_pbu, result, factor, contributions = best_point(scores, reverse_order)
    plot_signals, plot_molecular = records["all_simulations"][optimal_pbu]
    scaled = lambda d: {s: int(py2_round(n * factor)) for s, n in d.items()}       # noqa: E731
    normalized, normalized_molecular = scaled(plot_signals), scaled(plot_molecular)
    diff = {s: float(n - normalized[s]) / n for s, n in observed_signals.items() if s in normalized and n > 0}
    if letters is not None:                                         # the heat maps have one axis per drop of one letter
        return {"optimal_pbu": optimal_pbu, "result": result, "normalization_factor": factor, "optimal_contributions": contributions,
                "normalized_plot_signals": normalized, "normalized_plot_molecular_signals": normalized_molecular,
                "diff_plot_signals": diff, "incompatibility_scores": incompatibility_scores, "exclude_signals": exclude_signals,
                "tables": None, "z_ranges": None, "num_cycles": num_cycles, "headers": None, "labels": letters}
    single, double = [], []
    for (s, z, si), count in itertools.chain(observed_signals.items(), normalized.items(), normalized_molecular.items()):
        if not z or len(s) > len(set(s)):
            continue
        if len(s) == 1:
            assert si == 1, "si != 1"
            single.append(count)
        elif len(s) == 2:
            assert si == 2
            double.append(count)
        else:
            assert si > 2, "si <= 2"
    both = list(incompatibility_scores.values()) + list(contributions.values())
    z_ranges = {"single_drop": (0, max(single)) if single else None, "double_drop": (0, max(double)) if double else None,
                "incompatibility": (min(0, min(both)), max(both)) if both else None,
                "diff": (min(diff.values()), max(diff.values())) if diff else None}
    shape = (num_mocks, num_edmans, num_mocks_omitted)
    sources = (observed_signals, normalized, diff, observed_signals, normalized, diff, contributions, normalized_molecular,
               incompatibility_scores, contributions, normalized_molecular, incompatibility_scores)
    tables = {}
    for name, source in zip(TABLE_NAMES, sources):
        table = single_drops_table if name.startswith("single") else double_drops_table
        tables[name] = table(source, *shape, plot_remainders=True,
                             float_data=name.split("_")[1] in ("diff", "contributions", "incompatibility"))[0]
    return {"optimal_pbu": optimal_pbu, "result": result, "normalization_factor": factor, "optimal_contributions": contributions,
            "normalized_plot_signals": normalized, "normalized_plot_molecular_signals": normalized_molecular,
            "diff_plot_signals": diff, "incompatibility_scores": incompatibility_scores, "exclude_signals": exclude_signals,
            "tables": tables, "z_ranges": z_ranges, "num_cycles": num_cycles,
            "headers": {"single": single_drops_table({}, *shape)[1], "double": double_drops_table({}, *shape)[1:]}}


def reference_tuple(diagnostic):
    """The reference's return value (:1259) of match_diagnostic's dict."""
    return (diagnostic["normalized_plot_signals"], diagnostic["optimal_contributions"], diagnostic["incompatibility_scores"])
