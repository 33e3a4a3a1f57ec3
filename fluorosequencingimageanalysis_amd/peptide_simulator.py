"""Peptide Monte-Carlo simulation on the GPU: the reference's peptide_simulator.py for one label letter.

N molecules of one labelled peptide go through duds, mocks, Edman cycles, photobleaching and surface loss, one lane per
molecule, and get one lognormal intensity per frame (`simulate_device`, `simulation_records`; include/fsq_peptide_sim.h).
`simulate_and_fit_records` hands the intensities to the lognormal fluor-count fit without leaving the device and returns
what the reference's simulate_peptide.py pickles.

The reference is unseeded (peptide_simulation ignores its random_seed and seeds every worker with random.random(); the
intensities come from numpy's global RandomState).  Here the draws are explicit - Philox4x32-10 keyed by (seed, molecule,
stream), DESIGN 4.18 - and everything computed from them has the reference's bits; `random_seed=int` therefore reproduces
a run, `None` draws a fresh seed.  Molecules come back in molecule order (the reference returns its workers' results last
to first).

The drop-ins with the reference's signatures (`simulate_dye_counts`, `simulate_photometries`, `peptide_simulation`,
`convert_to_oldstyle`, `FluorEvent`) are built from the records, one Python object per event: the slow path, for code that
wants the reference's tuples.  Not built, each NotImplementedError: more than one label letter (the reference's own command
line stops there, simulate_peptide.py:249) and distance_ddif (the reference never records dye positions - the event is
created under the name None, :244-249, :304 - so its branch is dead, or a NameError, :371)."""
import ctypes
import math
import os
from collections import deque, namedtuple
from string import ascii_letters, digits

import numpy as np

from . import _host_peptide_sim
from . import _native_peptide_sim as NP
from . import _tracks
from . import engine as _engine

FluorEvent = namedtuple('FluorEvent', ['original_position', 'original_amino_acid', 'event_name', 'cycle_number', 'message'])

CAUSE_NONE, CAUSE_DUD, CAUSE_DESTRUCTION, CAUSE_EDMAN, CAUSE_STRIP = (NP.CAUSE_NONE, NP.CAUSE_DUD, NP.CAUSE_DESTRUCTION,
                                                                      NP.CAUSE_EDMAN, NP.CAUSE_STRIP)
CAUSE_NAMES = {CAUSE_DUD: 'dye dud', CAUSE_DESTRUCTION: 'dye destruction', CAUSE_EDMAN: 'edman', CAUSE_STRIP: 'surface strip'}
TABLES = ("counts", "loss_cycle", "loss_cause", "edman_fail", "intensity", "log_intensity", "category", "n_draws")


def fresh_seed():
    return int.from_bytes(os.urandom(8), "little")


def _define_reserved_character(sequence, labels):
    """A letter or digit neither the sequence nor the labels use (:22-34); the first one, where the reference pops any."""
    used = set(sequence) | set(labels)
    for ch in ascii_letters + digits:
        if ch not in used:
            return ch
    raise ValueError("sequence and labels use all possible string.letters and string.digits. At least one must remain "
                     "available as a reserved letter for simulation purposes.")


def _label_of(labels):
    letters = sorted(set(labels))
    if len(letters) > 1:
        raise NotImplementedError("This part currently only works for one label.")
    if not letters:
        raise ValueError("a label letter is needed")
    return letters[0]


def _params(sequence, labels, num_mocks, num_edmans, seed, first_molecule, ep):
    """FsqPeptideSimParams of the reference's arguments, after the checks fsq_peptide_simulate makes."""
    label = _label_of(labels)
    ep = dict(ep)
    if ep.get('distance_ddif') is not None:
        raise NotImplementedError("distance_ddif is not built (the reference never records dye positions)")
    length = len(sequence)
    if not 1 <= length <= NP.MAX_LENGTH:
        raise ValueError("the peptide's length must be in 1 .. %d" % NP.MAX_LENGTH)
    mask = sum(1 << i for i, ch in enumerate(sequence) if ch == label)
    n_labelled = bin(mask).count("1")
    if n_labelled > NP.MAX_LABELLED:
        raise ValueError("at most %d labelled residues" % NP.MAX_LABELLED)
    num_mocks, num_edmans = int(num_mocks), int(num_edmans)
    if num_mocks < 0 or num_edmans < 0 or num_mocks + num_edmans + 1 > NP.MAX_FRAMES:
        raise ValueError("num_mocks + num_edmans + 1 must be in 1 .. %d frames" % NP.MAX_FRAMES)
    ddif = ep.get('ddif')
    ddif = [0.0] * NP.MAX_LABELLED if ddif is None else [float(x) for x in ddif][:NP.MAX_LABELLED]
    if len(ddif) < n_labelled:
        raise ValueError("ddif is shorter than the number of labelled residues")
    seed, first_molecule = int(seed), int(first_molecule)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must be in 0 .. 2^64 - 1")
    rate = float(ep.get('superdye_rate', 0))
    if not (0 <= rate <= 1):
        raise ValueError("superdye_rate must be between 0 and 1 (inclusive).")
    prm = NP.FsqPeptideSimParams()
    prm.label_mask, prm.seed, prm.first_molecule = mask, seed, first_molecule
    prm.p, prm.u, prm.s, prm.s2 = float(ep['p']), float(ep['u']), float(ep['s']), float(ep['s2'])
    prm.per_cycle_b = float(ep['per_cycle_b']) if 'per_cycle_b' in ep else math.e ** -ep['b']           # (:82-83)
    prm.log_beta, prm.beta_sigma = math.log(ep.get('beta', 1.0)), float(ep.get('beta_sigma', 1.0))
    prm.superdye_rate, prm.superdye_factor = rate, float(ep.get('superdye_factor', 2))
    for i, x in enumerate(ddif):
        prm.ddif[i] = x
    prm.n_ddif, prm.length, prm.num_mocks, prm.num_edmans = len(ddif), length, num_mocks, num_edmans
    prm.sc = int(max(-1, min(NP.MAX_FRAMES, math.floor(ep['sc']))))                  # (cycle <= sc for integer cycles)
    values = [prm.p, prm.u, prm.s, prm.s2, prm.per_cycle_b, prm.log_beta, prm.beta_sigma, prm.superdye_factor] + ddif
    if not all(math.isfinite(x) for x in values):
        raise ValueError("finite parameters are needed")
    meta = {"sequence": sequence, "label": label, "num_mocks": num_mocks, "num_edmans": num_edmans, "seed": seed,
            "first_molecule": first_molecule}
    return prm, meta


def philox_words_device(d_counters, d_keys):
    """fsq_philox_words: Philox4x32-10 of int32-viewed uint32 [n, 4] counters under [n, 2] keys, as a CUDA tensor [n, 4]."""
    torch = _engine._torch()
    n = int(d_counters.shape[0])
    if d_counters.dtype != torch.int32 or d_keys.dtype != torch.int32 or tuple(d_counters.shape) != (n, 4) or tuple(d_keys.shape) != (n, 2):
        raise ValueError("int32 tensors [n, 4] and [n, 2] are needed")
    d_counters, d_keys = d_counters.contiguous(), d_keys.contiguous()
    out = torch.empty((n, 4), dtype=torch.int32, device=d_counters.device)
    _engine.launch(NP.lib().fsq_philox_words, "fsq_philox_words", d_counters.device, d_counters.data_ptr(), d_keys.data_ptr(), n,
                   out.data_ptr())
    return out


def simulate_device_prm(prm, n_molecules, device=None):
    """fsq_peptide_simulate for parameters already built: the dict of device tensors of simulate_device (TABLES).  Enqueued
    on the current stream, not synchronised."""
    torch = _engine._torch()
    dev = torch.device(device or "cuda")
    n = int(n_molecules)
    if n < 0:
        raise ValueError("num_simulations must not be negative")
    F, L = prm.num_mocks + prm.num_edmans + 1, bin(prm.label_mask).count("1")
    out = {"counts": torch.empty((n, F), dtype=torch.uint8, device=dev),
           "loss_cycle": torch.empty((n, L), dtype=torch.uint8, device=dev),
           "loss_cause": torch.empty((n, L), dtype=torch.uint8, device=dev),
           "edman_fail": torch.empty(n, dtype=torch.int64, device=dev),
           "intensity": torch.empty((n, F), dtype=torch.float64, device=dev),
           "log_intensity": torch.empty((n, F), dtype=torch.float64, device=dev),
           "category": torch.empty(n, dtype=torch.int64, device=dev),
           "n_draws": torch.empty((n, 3), dtype=torch.int32, device=dev)}
    _engine.launch(NP.lib().fsq_peptide_simulate, "fsq_peptide_simulate", dev, ctypes.byref(prm), n,
                   *[out[k].data_ptr() if out[k].numel() else None for k in TABLES])
    return out


def simulate_device(sequence, labels, num_mocks, num_edmans, num_simulations=1, seed=0, first_molecule=0, device=None,
                    **experimental_parameters):
    """The simulation of num_simulations molecules with ids first_molecule + i, as device tensors: counts uint8 [n, frames],
    loss_cycle and loss_cause uint8 [n, labelled], edman_fail int64 [n] (bit c: the Edman of cycle c failed), intensity and
    log_intensity float64 [n, frames], category int64 [n] (bit f: frame f has dyes; the uint64 word of lognormal.py),
    n_draws int32 [n, 3]; and the plain values sequence, label, num_mocks, num_edmans, seed, first_molecule.
    experimental_parameters are peptide_simulation's: p, b (or per_cycle_b), u, s, sc, s2, beta, beta_sigma, ddif,
    superdye_rate, superdye_factor."""
    prm, meta = _params(sequence, labels, num_mocks, num_edmans, seed, first_molecule, experimental_parameters)
    out = simulate_device_prm(prm, num_simulations, device)
    out.update(meta)
    return out


def simulation_records(sequence, labels, num_mocks, num_edmans, num_simulations=1, seed=0, first_molecule=0, device=None,
                       host=False, **experimental_parameters):
    """simulate_device's dict as NumPy arrays (edman_fail and category as uint64).  host=True: the same records from the
    NumPy twin of the kernel, without a GPU."""
    prm, meta = _params(sequence, labels, num_mocks, num_edmans, seed, first_molecule, experimental_parameters)
    if host:
        out = _host_peptide_sim.simulate(prm.length, prm.label_mask, prm.num_mocks, prm.num_edmans, prm.p, prm.per_cycle_b, prm.u,
                                         prm.s, prm.sc, prm.s2, prm.log_beta, prm.beta_sigma, list(prm.ddif)[:prm.n_ddif],
                                         prm.superdye_rate, prm.superdye_factor, prm.seed, prm.first_molecule, int(num_simulations))
    else:
        out = _engine.to_host(simulate_device_prm(prm, num_simulations, device))
        out["edman_fail"], out["category"] = out["edman_fail"].view(np.uint64), out["category"].view(np.uint64)
    out.update(meta)
    return out


# ---- the reference's tuples, from the records ----

def events_from_records(records, i, reserved_character=None):
    """The reference's event_buffer of molecule i (:281-289): the loss and Edman-failure events, and after every cycle the
    'dye count' event and the dye-position event (created under the name None, :244-249)."""
    seq, label = records["sequence"], records["label"]
    if reserved_character is None:
        reserved_character = records.get("reserved_character") or _define_reserved_character(seq, label)
    pos = [k for k, ch in enumerate(seq) if ch == label]
    lcyc, cause = records["loss_cycle"][i].tolist(), records["loss_cause"][i].tolist()
    counts, fail = records["counts"][i].tolist(), int(records["edman_fail"][i])
    num_mocks = records["num_mocks"]
    events, nterm = [], 0

    def lost(cycle, what):
        for k, p in enumerate(pos):
            if cause[k] == what and lcyc[k] == cycle:
                events.append(FluorEvent(p + 1, label, CAUSE_NAMES[what], cycle, None))

    for c in range(len(counts)):
        if c == 0:
            lost(0, CAUSE_DUD)
        else:
            if c > num_mocks and nterm < len(seq):
                if (fail >> c) & 1:
                    k = pos.index(nterm) if nterm in pos else None
                    if k is not None and cause[k] != CAUSE_NONE and lcyc[k] < c:
                        # (a residue that lost its dye sits in the molecule as (reserved_character, position), :98)
                        events.append(FluorEvent(reserved_character, nterm + 1, 'edman failure', c, None))
                    else:
                        events.append(FluorEvent(nterm + 1, seq[nterm], 'edman failure', c, None))
                else:
                    lost(c, CAUSE_EDMAN)
                    nterm += 1
            lost(c, CAUSE_STRIP)
        lost(c, CAUSE_DESTRUCTION)
        events.append(FluorEvent(None, None, 'dye count', c, {label: counts[c]}))
        live = tuple((p + 1, label) for k, p in enumerate(pos) if cause[k] == CAUSE_NONE or lcyc[k] > c)
        events.append(FluorEvent(None, None, None, c, live))
    return events


class _CountRow(tuple):
    """A molecule's counts as the reference's tuple, remembering where its intensities are (simulate_photometries)."""
    records = molecule = None


def _dye_count_result(records, i, reserved_character):
    events = events_from_records(records, i, reserved_character)
    decrements = tuple(sorted([(e.original_amino_acid, e.cycle_number) for e in events if e.event_name in CAUSE_NAMES.values()],
                              key=lambda x: x[1]))
    row = _CountRow(records["counts"][i].tolist())
    row.records, row.molecule = records, i
    return decrements, {records["label"]: row}, events, ()


def simulate_dye_counts(sequence, labels, num_mocks, num_edmans, num_simulations=1, random_seed=None, reserved_character=None,
                        first_molecule=0, device=None, host=False, **experimental_parameters):
    """peptide_simulator.simulate_dye_counts (:190-319): [(dye_decrements, dye_counts, event_buffer, dye_position_tracker)].
    dye_position_tracker is () as in the reference, which looks for an event name nothing carries (:304)."""
    seed = fresh_seed() if random_seed is None else int(random_seed)
    records = simulation_records(sequence, labels, num_mocks, num_edmans, num_simulations, seed, first_molecule, device, host,
                                 **experimental_parameters)
    if reserved_character is None:
        reserved_character = _define_reserved_character(sequence, labels)
    records["reserved_character"] = reserved_character
    return [_dye_count_result(records, i, reserved_character) for i in range(int(num_simulations))]


def _category_and_intensities(records, i):
    counts = records["counts"][i].tolist()
    return tuple([False if c == 0 else True for c in counts]), (tuple(records["intensity"][i].tolist()),)


def simulate_photometries(dye_counts, beta, beta_sigma, number, ddif=None, dye_position_tracker=None, distance_ddif=None,
                          superdye_rate=0, superdye_factor=1, records=None, molecule=None):
    """peptide_simulator.simulate_photometries (:322-435) for number = 1: (category, (intensities,)).  The device draws a
    molecule's intensities in the launch that draws its counts, so dye_counts must be a count row simulate_dye_counts
    returned (or `records` and `molecule` are given), simulated with the same beta, beta_sigma, ddif and superdye values."""
    if distance_ddif is not None:
        raise NotImplementedError("distance_ddif is not built (the reference never records dye positions)")
    if not (0 <= superdye_rate <= 1):
        raise ValueError("superdye_rate must be between 0 and 1 (inclusive).")
    if number != 1:
        raise NotImplementedError("one intensity row per molecule (number=1), as peptide_simulation asks for")
    if records is None:
        records, molecule = getattr(dye_counts, "records", None), getattr(dye_counts, "molecule", None)
    if records is None or molecule is None:
        raise NotImplementedError("dye_counts must come from simulate_dye_counts: intensities are drawn with the counts")
    if tuple(dye_counts) != tuple(records["counts"][molecule].tolist()):
        raise ValueError("dye_counts is not the count row of that molecule")
    return _category_and_intensities(records, molecule)


def peptide_simulation(sequence, labels, num_mocks, num_edmans, num_simulations=1, random_seed=None, num_processes=None,
                       reserved_character=None, first_molecule=0, device=None, host=False, **experimental_parameters):
    """peptide_simulator.peptide_simulation (:438-502): a deque of (dye_decrements, dye_counts, event_buffer,
    {label: (category, (intensities,))}), in molecule order.  random_seed=int reproduces (the reference ignores it);
    num_processes is accepted and unused."""
    results = simulate_dye_counts(sequence, labels, num_mocks, num_edmans, num_simulations, random_seed, reserved_character,
                                  first_molecule, device, host, **experimental_parameters)
    merged = deque()
    for decrements, dye_counts, events, _ in results:
        merged.append((decrements, dye_counts, events,
                       {L: _category_and_intensities(row.records, row.molecule) for L, row in dye_counts.items()}))
    return merged


def convert_to_oldstyle(merged_dye_count_results):
    """peptide_simulator.convert_to_oldstyle (:505-568): the one label becomes 'A', decrements of cycle 0 are dropped,
    (('A', 0),) stands for none, molecules without dyes at frame 0 are omitted."""
    oldstyle_results = deque()
    for dye_decrements, dye_counts, event_buffer, categories_and_intensities in merged_dye_count_results:
        if len(set(amino_acid for amino_acid, position in dye_decrements)) > 1:
            raise Exception("Oldstyle only works with one label.")
        oldstyle = tuple([('A', position) for amino_acid, position in dye_decrements if position != 0])
        if len(dye_counts) > 1:
            raise Exception("Oldstyle only works with one label.")
        counts = next(iter(dye_counts.values()))
        drops = sum(c1 - c2 for c1, c2 in zip(counts[:-1], counts[1:]))
        if len(oldstyle) == 0:
            oldstyle = (('A', 0),)
            assert drops == 0, "dye_counts_drops != 0 when oldstyle_dye_decrements is (('A', 0),)"
        else:
            assert drops == len(oldstyle), "%s != %s; must be dye_counts_drops == len(oldstyle_dye_decrements)" % (drops, len(oldstyle))
        old_ci = {'A': (category, (intensities,)) for label, (category, (intensities,)) in categories_and_intensities.items()
                  if True in category}
        if old_ci:
            oldstyle_results.append((oldstyle, dye_counts, event_buffer, old_ci))
    return oldstyle_results


# ---- the chain on the device ----

def signals_from_device(sim, fit=None):
    """(molecular_error_signals, signals, total_count, none_count) of a simulation on the device and, if given, the fit of
    its kept molecules: torch.unique over the count rows and over the winning rows; only the unique rows reach Python."""
    torch = _engine._torch()
    from . import lognormal as LN
    keep = sim["category"] != 0
    rows, n = torch.unique(sim["counts"][keep], dim=0, return_counts=True)
    mes, _ = _tracks.tally_signals(((_tracks.decrements_of_row(row), row[-1] == 0, row[0]) for row in rows.cpu().tolist()),
                                   n.cpu().tolist())
    if fit is None:
        return mes, None, int(keep.sum()), None
    found = fit["status"] == LN.STATUS_FOUND
    bad = fit["status"] > LN.STATUS_NONE
    if bool(bad.any()):
        raise NotImplementedError("a simulated track has more surviving sequences than the budget, or an invalid length")
    rows, n = torch.unique(fit["best_seq"][found], dim=0, return_counts=True)
    signals, _ = _tracks.tally_signals((LN.signal_of(tuple(row)) for row in rows.cpu().tolist()), n.cpu().tolist())
    total = int(fit["status"].numel())
    return mes, signals, total, total - int(found.sum())


def simulate_and_fit_records(sequence, labels, num_mocks, num_edmans, num_simulations=1, seed=0, first_molecule=0, device=None,
                             max_possible=5, allow_multidrop=True, max_deviation=3, quench_factors=None, budget=None,
                             **experimental_parameters):
    """Simulate, drop the molecules without dyes at any frame (convert_to_oldstyle omits them) and fit the rest with
    lognormal.lognormal_device, all on the device.  Returns a dict: signals, total_count and none_count as
    lognormal.photometries_lognormal_fit gives them for the kept tracks, molecular_error_signals as simulate_peptide.py
    counts them ({(decrements, counts[-1] == 0, counts[0]): n}), `kept` (a bool CUDA tensor over the molecules), and the
    device tensors `simulation` and `fit`."""
    torch = _engine._torch()
    from . import lognormal as LN
    beta, beta_sigma = experimental_parameters['beta'], experimental_parameters['beta_sigma']
    means = _tracks.log_fluor_means(beta, quench_factors, max_possible)
    fit_prm = LN.fit_params(means, beta_sigma, max_possible, allow_multidrop, max_deviation, LN.DEFAULT_BUDGET if budget is None else budget)
    sim = simulate_device(sequence, labels, num_mocks, num_edmans, num_simulations, seed, first_molecule, device,
                          **experimental_parameters)
    if not allow_multidrop and sim["counts"].shape[1] == 1:
        raise ValueError("max() arg is an empty sequence")        # (as lognormal.photometries_lognormal_fit, :5442)
    keep = sim["category"] != 0
    d_int = sim["intensity"][keep].contiguous()       # (the fit takes log(I) itself: fsq_lognormal_fit's pre-pass)
    d_cat = sim["category"][keep].contiguous()
    n = int(d_int.shape[0])
    if n:
        d_len = torch.full((n,), int(d_int.shape[1]), dtype=torch.int32, device=d_int.device)
        fit = LN.lognormal_device(d_int, d_cat, d_len, None, None, prm=fit_prm)
        mes, signals, total, none_count = signals_from_device(sim, fit)
    else:
        fit = None
        (mes, _, _, _), signals, total, none_count = signals_from_device(sim), {}, 0, 0
    return {"signals": signals, "total_count": total, "none_count": none_count, "molecular_error_signals": mes, "kept": keep,
            "simulation": sim, "fit": fit}
