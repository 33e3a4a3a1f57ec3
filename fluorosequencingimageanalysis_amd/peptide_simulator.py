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

Several label letters, one colour channel each (`multilabel_device`, `multilabel_records`, `multilabel_and_fit_records`;
include/fsq_peptide_labels.h): the chemistry is the same walk on the union of the labelled positions - the
reference draws once per residue whose letter is in `labels`, whatever the letter - with the dyes counted per letter and one
intensity row per letter on that channel's own streams.  The channels are the sorted label letters (the reference iterates
a Python-2 dict, an order nobody can pin).  `simulate_device`, `simulation_records` and `_params` keep serving one letter:
their tables have no channel axis.

The drop-ins with the reference's signatures (`simulate_dye_counts`, `simulate_photometries`, `peptide_simulation`,
`convert_to_oldstyle`, `FluorEvent`) are built from the records, one Python object per event: the slow path, for code that
wants the reference's tuples.  With several letters they go through `multilabel_records`; dicts over the letters are in
sorted-letter order.  Not built, each an error saying so: distance_ddif (the reference never records dye positions - the
event is created under the name None, :244-249, :304 - so its branch is dead, or a NameError, :371), more than 4 label
letters, more than 15 labelled residues of one letter, and more than one letter in signal_sweep."""
import ctypes
import math
import os
from collections import deque, namedtuple
from string import ascii_letters, digits

import numpy as np

from . import _host_peptide_sim
from . import _native_peptide_labels as NL
from . import _native_peptide_sim as NP
from . import _tracks
from . import engine as _engine

FluorEvent = namedtuple('FluorEvent', ['original_position', 'original_amino_acid', 'event_name', 'cycle_number', 'message'])

CAUSE_NONE, CAUSE_DUD, CAUSE_DESTRUCTION, CAUSE_EDMAN, CAUSE_STRIP = (NP.CAUSE_NONE, NP.CAUSE_DUD, NP.CAUSE_DESTRUCTION,
                                                                      NP.CAUSE_EDMAN, NP.CAUSE_STRIP)
CAUSE_NAMES = {CAUSE_DUD: 'dye dud', CAUSE_DESTRUCTION: 'dye destruction', CAUSE_EDMAN: 'edman', CAUSE_STRIP: 'surface strip'}
TABLES = ("counts", "loss_cycle", "loss_cause", "edman_fail", "intensity", "log_intensity", "category", "n_draws")
PER_LETTER = ("beta", "beta_sigma", "ddif", "superdye_rate", "superdye_factor")      # one value for all letters, or {letter: value}
JOINT_TALLY_SLOTS = 1 << 24     # the largest table of joint_signals_from_device's tally (FSQ_SIGNAL_MAX_SLOTS)


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
        raise NotImplementedError("This part currently only works for one label (several letters: multilabel_records; "
                                  "parameter sweeps over several letters: signal_sweep.joint_sweep_records).")
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


# ---- several label letters, one colour channel each ----

def _per_letter(ep, name, letters, default):
    """The value of experimental parameter `name` for every letter: one value for all, or a dict {letter: value}."""
    value = ep.get(name, default)
    if isinstance(value, dict):
        missing = [L for L in letters if L not in value]
        if missing:
            raise ValueError("%s has no value for the label letters %s" % (name, missing))
        return [value[L] for L in letters]
    return [value] * len(letters)


def _labels_params(sequence, labels, num_mocks, num_edmans, seed, first_molecule, ep):
    """FsqPeptideLabelsParams of the reference's arguments, after the checks fsq_peptide_simulate_labels makes; beta,
    beta_sigma, ddif, superdye_rate and superdye_factor are one value for all letters or a dict {letter: value}."""
    letters = sorted(set(labels))
    if not letters:
        raise ValueError("a label letter is needed")
    if len(letters) > NL.MAX_CHANNELS:
        raise NotImplementedError("at most %d label letters, one colour channel each" % NL.MAX_CHANNELS)
    ep = dict(ep)
    if ep.get('distance_ddif') is not None:
        raise NotImplementedError("distance_ddif is not built (the reference never records dye positions)")
    length, K = len(sequence), len(letters)
    if not 1 <= length <= NL.MAX_LENGTH:
        raise ValueError("the peptide's length must be in 1 .. %d" % NL.MAX_LENGTH)
    num_mocks, num_edmans = int(num_mocks), int(num_edmans)
    if num_mocks < 0 or num_edmans < 0 or num_mocks + num_edmans + 1 > NL.MAX_FRAMES:
        raise ValueError("num_mocks + num_edmans + 1 must be in 1 .. %d frames" % NL.MAX_FRAMES)
    seed, first_molecule = int(seed), int(first_molecule)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must be in 0 .. 2^64 - 1")
    prm = NL.FsqPeptideLabelsParams()
    prm.n_channels, prm.seed, prm.first_molecule = K, seed, first_molecule
    prm.p, prm.u, prm.s, prm.s2 = float(ep['p']), float(ep['u']), float(ep['s']), float(ep['s2'])
    prm.per_cycle_b = float(ep['per_cycle_b']) if 'per_cycle_b' in ep else math.e ** -ep['b']           # (:82-83)
    prm.length, prm.num_mocks, prm.num_edmans = length, num_mocks, num_edmans
    prm.sc = int(max(-1, min(NL.MAX_FRAMES, math.floor(ep['sc']))))                  # (cycle <= sc for integer cycles)
    values = [prm.p, prm.u, prm.s, prm.s2, prm.per_cycle_b]
    betas, sigmas = _per_letter(ep, 'beta', letters, 1.0), _per_letter(ep, 'beta_sigma', letters, 1.0)
    ddifs, rates = _per_letter(ep, 'ddif', letters, None), _per_letter(ep, 'superdye_rate', letters, 0)
    factors = _per_letter(ep, 'superdye_factor', letters, 2)
    for k, letter in enumerate(letters):
        mask = sum(1 << i for i, ch in enumerate(sequence) if ch == letter)
        n_labelled = bin(mask).count("1")
        if n_labelled > NL.MAX_LABELLED:
            raise ValueError("at most %d labelled residues of one letter (%d of %r)" % (NL.MAX_LABELLED, n_labelled, letter))
        ddif = [0.0] * NL.MAX_LABELLED if ddifs[k] is None else [float(x) for x in ddifs[k]][:NL.MAX_LABELLED]
        if len(ddif) < n_labelled:
            raise ValueError("ddif is shorter than the number of labelled residues")
        rate = float(rates[k])
        if not (0 <= rate <= 1):
            raise ValueError("superdye_rate must be between 0 and 1 (inclusive).")
        prm.channel_mask[k], prm.n_ddif[k] = mask, len(ddif)
        prm.log_beta[k], prm.beta_sigma[k] = math.log(betas[k]), float(sigmas[k])
        prm.superdye_rate[k], prm.superdye_factor[k] = rate, float(factors[k])
        for i, x in enumerate(ddif):
            prm.ddif[k][i] = x
        values += [prm.log_beta[k], prm.beta_sigma[k], prm.superdye_factor[k]] + ddif
    if not all(math.isfinite(x) for x in values):
        raise ValueError("finite parameters are needed")
    positions = tuple((i, letters.index(ch)) for i, ch in enumerate(sequence) if ch in letters)
    meta = {"sequence": sequence, "labels": tuple(letters), "positions": positions, "num_mocks": num_mocks, "num_edmans": num_edmans,
            "seed": seed, "first_molecule": first_molecule}
    return prm, meta


def multilabel_device_prm(prm, n_molecules, device=None):
    """fsq_peptide_simulate_labels for parameters already built: the dict of device tensors of multilabel_device (TABLES).
    Enqueued on the current stream, not synchronised."""
    torch = _engine._torch()
    dev = torch.device(device or "cuda")
    n = int(n_molecules)
    if n < 0:
        raise ValueError("num_simulations must not be negative")
    K, F = prm.n_channels, prm.num_mocks + prm.num_edmans + 1
    L = sum(bin(prm.channel_mask[k]).count("1") for k in range(K))
    out = {"counts": torch.empty((K, n, F), dtype=torch.uint8, device=dev),
           "loss_cycle": torch.empty((n, L), dtype=torch.uint8, device=dev),
           "loss_cause": torch.empty((n, L), dtype=torch.uint8, device=dev),
           "edman_fail": torch.empty(n, dtype=torch.int64, device=dev),
           "intensity": torch.empty((K, n, F), dtype=torch.float64, device=dev),
           "log_intensity": torch.empty((K, n, F), dtype=torch.float64, device=dev),
           "category": torch.empty((K, n), dtype=torch.int64, device=dev),
           "n_draws": torch.empty((n, 1 + 2 * K), dtype=torch.int32, device=dev)}
    _engine.launch(NL.lib().fsq_peptide_simulate_labels, "fsq_peptide_simulate_labels", dev, ctypes.byref(prm), n,
                   *[out[k].data_ptr() if out[k].numel() else None for k in TABLES])
    return out


def multilabel_device(sequence, labels, num_mocks, num_edmans, num_simulations=1, seed=0, first_molecule=0, device=None,
                      **experimental_parameters):
    """simulate_device for any set of up to 4 label letters (one is allowed), K colour channels in sorted-letter order, as
    device tensors: counts uint8 [K, n, frames], loss_cycle and loss_cause uint8 [n, labelled residues of all letters, in
    position order], edman_fail int64 [n], intensity and log_intensity float64 [K, n, frames] (a channel's table is one
    contiguous block), category int64 [K, n], n_draws int32 [n, 1 + 2K]; and the plain values sequence, labels (the sorted
    letters), positions ((residue, channel) of every labelled residue), num_mocks, num_edmans, seed, first_molecule.
    experimental_parameters are peptide_simulation's; beta, beta_sigma, ddif, superdye_rate and superdye_factor may each
    be a dict {letter: value}."""
    prm, meta = _labels_params(sequence, labels, num_mocks, num_edmans, seed, first_molecule, experimental_parameters)
    out = multilabel_device_prm(prm, num_simulations, device)
    out.update(meta)
    return out


def multilabel_records(sequence, labels, num_mocks, num_edmans, num_simulations=1, seed=0, first_molecule=0, device=None,
                       host=False, **experimental_parameters):
    """multilabel_device's dict as NumPy arrays (edman_fail and category as uint64).  host=True: the same records from the
    NumPy twin of the kernel (_host_peptide_sim.simulate_labels), without a GPU."""
    prm, meta = _labels_params(sequence, labels, num_mocks, num_edmans, seed, first_molecule, experimental_parameters)
    if host:
        K = prm.n_channels
        out = _host_peptide_sim.simulate_labels(
            prm.length, list(prm.channel_mask)[:K], prm.num_mocks, prm.num_edmans, prm.p, prm.per_cycle_b, prm.u, prm.s, prm.sc,
            prm.s2, list(prm.log_beta)[:K], list(prm.beta_sigma)[:K], [list(prm.ddif[k])[:prm.n_ddif[k]] for k in range(K)],
            list(prm.superdye_rate)[:K], list(prm.superdye_factor)[:K], prm.seed, prm.first_molecule, int(num_simulations))
    else:
        out = _engine.to_host(multilabel_device_prm(prm, num_simulations, device))
        out["edman_fail"], out["category"] = out["edman_fail"].view(np.uint64), out["category"].view(np.uint64)
    out.update(meta)
    return out


def joint_signal(letters, rows):
    """The joint molecular-error key of one molecule's count rows (one per letter, the sorted letters): (decrements, zeros,
    starts).  decrements: a (letter, cycle) pair per dye lost after frame 0, sorted by (cycle, letter), () for none; zeros
    and starts: per letter, whether its last count is 0 and its count at frame 0.  A definition of this package: the
    reference has none for two letters (its command line stops at one)."""
    dec = sorted((c, L) for L, row in zip(letters, rows) for c in range(1, len(row)) for _ in range(row[c - 1] - row[c]))
    return tuple((L, c) for c, L in dec), tuple(row[-1] == 0 for row in rows), tuple(row[0] for row in rows)


def joint_signals_of_records(records):
    """{joint_signal: n} over the molecules of multilabel records with any dye at frame 0, in plain Python."""
    letters, counts, out = records["labels"], np.asarray(records["counts"]), {}
    for i in range(counts.shape[1]):
        rows = counts[:, i].tolist()
        if any(row[0] for row in rows):
            key = joint_signal(letters, rows)
            out[key] = out.get(key, 0) + 1
    return out


# ---- the reference's tuples, from the records ----

def events_from_records(records, i, reserved_character=None):
    """The reference's event_buffer of molecule i (:281-289): the loss and Edman-failure events, and after every cycle the
    'dye count' event and the dye-position event (created under the name None, :244-249)."""
    seq = records["sequence"]
    if "labels" in records:                                     # several letters: every residue's own letter
        letters = records["labels"]
        rows = [records["counts"][k][i].tolist() for k in range(len(letters))]
    else:
        letters, rows = (records["label"],), [records["counts"][i].tolist()]
    if reserved_character is None:
        reserved_character = records.get("reserved_character") or _define_reserved_character(seq, letters)
    pos = [k for k, ch in enumerate(seq) if ch in letters]
    lcyc, cause = records["loss_cycle"][i].tolist(), records["loss_cause"][i].tolist()
    fail = int(records["edman_fail"][i])
    num_mocks = records["num_mocks"]
    events, nterm = [], 0

    def lost(cycle, what):
        for k, p in enumerate(pos):
            if cause[k] == what and lcyc[k] == cycle:
                events.append(FluorEvent(p + 1, seq[p], CAUSE_NAMES[what], cycle, None))

    for c in range(len(rows[0])):
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
        events.append(FluorEvent(None, None, 'dye count', c, {L: row[c] for L, row in zip(letters, rows)}))
        live = tuple((p + 1, seq[p]) for k, p in enumerate(pos) if cause[k] == CAUSE_NONE or lcyc[k] > c)
        events.append(FluorEvent(None, None, None, c, live))
    return events


class _CountRow(tuple):
    """A molecule's counts as the reference's tuple, remembering where its intensities are (simulate_photometries)."""
    records = molecule = channel = None


def _count_row(records, i, channel=None):
    row = _CountRow((records["counts"][i] if channel is None else records["counts"][channel][i]).tolist())
    row.records, row.molecule, row.channel = records, i, channel
    return row


def _dye_count_result(records, i, reserved_character):
    events = events_from_records(records, i, reserved_character)
    decrements = tuple(sorted([(e.original_amino_acid, e.cycle_number) for e in events if e.event_name in CAUSE_NAMES.values()],
                              key=lambda x: x[1]))
    if "labels" in records:
        return decrements, {L: _count_row(records, i, k) for k, L in enumerate(records["labels"])}, events, ()
    return decrements, {records["label"]: _count_row(records, i)}, events, ()


def simulate_dye_counts(sequence, labels, num_mocks, num_edmans, num_simulations=1, random_seed=None, reserved_character=None,
                        first_molecule=0, device=None, host=False, **experimental_parameters):
    """peptide_simulator.simulate_dye_counts (:190-319): [(dye_decrements, dye_counts, event_buffer, dye_position_tracker)].
    dye_position_tracker is () as in the reference, which looks for an event name nothing carries (:304).  With several
    letters dye_counts is {letter: count row} and every event carries its residue's own letter; dye_decrements keep the
    reference's order, a stable sort by cycle of the event order (dud, Edman, strip, destruction, each in position order)."""
    seed = fresh_seed() if random_seed is None else int(random_seed)
    several = len(set(labels)) > 1 or any(isinstance(experimental_parameters.get(k), dict) for k in PER_LETTER)
    records = (multilabel_records if several else simulation_records)(sequence, labels, num_mocks, num_edmans, num_simulations,
                                                                      seed, first_molecule, device, host, **experimental_parameters)
    if reserved_character is None:
        reserved_character = _define_reserved_character(sequence, labels)
    records["reserved_character"] = reserved_character
    return [_dye_count_result(records, i, reserved_character) for i in range(int(num_simulations))]


def _category_and_intensities(records, i, channel=None):
    at = (lambda t: t[i]) if channel is None else (lambda t: t[channel][i])
    return tuple([False if c == 0 else True for c in at(records["counts"]).tolist()]), (tuple(at(records["intensity"]).tolist()),)


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
    channel = getattr(dye_counts, "channel", None)
    if records is None:
        records, molecule = getattr(dye_counts, "records", None), getattr(dye_counts, "molecule", None)
    if records is None or molecule is None:
        raise NotImplementedError("dye_counts must come from simulate_dye_counts: intensities are drawn with the counts")
    if "labels" in records and channel is None:
        raise NotImplementedError("dye_counts must be a letter's count row from simulate_dye_counts: it names the channel")
    if tuple(dye_counts) != tuple(_count_row(records, molecule, channel)):
        raise ValueError("dye_counts is not the count row of that molecule")
    return _category_and_intensities(records, molecule, channel)


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
                       {L: _category_and_intensities(row.records, row.molecule, row.channel) for L, row in dye_counts.items()}))
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


def joint_signals_from_device(sim):
    """joint_signals_of_records of a multilabel simulation on the device, over the molecules with any dye at frame 0: the joint
    key tally of signal_sweep (fsq_signal_tally_joint, one point), whose occupied slots alone reach Python.  The molecules
    without a 64-bit key (more drops in all than the key holds - a simulated row never steps up, so its drops are its first
    count minus its last -, a start above 15) go the other way: torch.unique over their K * frames count rows, and only the
    unique rows reach Python.  So do all of them where the table overflows.  The result is the same."""
    torch = _engine._torch()
    from . import _host_signal_sweep as H
    from . import signal_sweep as SW
    counts = sim["counts"]
    K, n, F = (int(x) for x in counts.shape)
    keep = (counts[:, :, 0] != 0).any(dim=0)
    out, rest = {}, keep
    if F <= H.MAX_FRAMES and counts.is_contiguous():
        drops = (counts[:, :, 0].to(torch.int32) - counts[:, :, F - 1].to(torch.int32)).sum(dim=0)
        keyed = keep & (drops <= H.JOINT_MAX_DROPS[K]) & (counts[:, :, 0] <= 15).all(dim=0)
        slots = 64                                                  # twice the keyed molecules: the table cannot fill up below the cap
        while slots < min(2 * int(keyed.sum()), JOINT_TALLY_SLOTS):
            slots *= 2
        tables = SW.new_tables(1, slots, counts.device)
        SW.tally_joint_device(tables, counts, torch.zeros(n, dtype=torch.int32, device=counts.device), keyed.to(torch.uint8))
        if not bool(tables["unkeyed"].any() | tables["overflow"].any() | tables["none"].any()):
            out, rest = SW._decode_tables(tables, tuple(sim["labels"]))[0], keep & ~keyed
    if bool(rest.any()):
        rows, m = torch.unique(counts.permute(1, 0, 2)[rest].reshape(-1, K * F), dim=0, return_counts=True)
        for row, count in zip(rows.cpu().tolist(), m.cpu().tolist()):
            key = joint_signal(sim["labels"], [row[k * F:(k + 1) * F] for k in range(K)])
            out[key] = out.get(key, 0) + count
    return out


def multilabel_and_fit_records(sequence, labels, num_mocks, num_edmans, num_simulations=1, seed=0, first_molecule=0, device=None,
                               max_possible=5, allow_multidrop=True, max_deviation=3, quench_factors=None, budget=None,
                               **experimental_parameters):
    """simulate_and_fit_records for several label letters: simulate, then per colour channel drop the molecules whose channel
    is dark at every frame and fit the rest with lognormal.lognormal_device under that letter's beta, beta_sigma and
    quench_factors (each one value for all letters or a dict {letter: value}), reading the channel's block of the intensity
    table on the device.  Returns {letter: {signals, total_count, none_count, kept, fit}} for every letter, `simulation` (the
    device tensors of multilabel_device) and `molecular_error_signals`: {joint_signal: n}, tallied on the device over the
    molecules with any dye at frame 0 - a definition of this package, see joint_signal."""
    torch = _engine._torch()
    from . import lognormal as LN
    sim = multilabel_device(sequence, labels, num_mocks, num_edmans, num_simulations, seed, first_molecule, device,
                            **experimental_parameters)
    letters = sim["labels"]
    if not allow_multidrop and sim["counts"].shape[2] == 1:
        raise ValueError("max() arg is an empty sequence")        # (as lognormal.photometries_lognormal_fit, :5442)
    betas, sigmas = _per_letter(experimental_parameters, 'beta', letters, None), _per_letter(experimental_parameters, 'beta_sigma', letters, None)
    quench = _per_letter({'quench_factors': quench_factors}, 'quench_factors', letters, None)
    out = {"simulation": sim, "molecular_error_signals": joint_signals_from_device(sim)}
    for k, letter in enumerate(letters):
        means = _tracks.log_fluor_means(betas[k], quench[k], max_possible)
        fit_prm = LN.fit_params(means, sigmas[k], max_possible, allow_multidrop, max_deviation, LN.DEFAULT_BUDGET if budget is None else budget)
        keep = sim["category"][k] != 0
        d_int = sim["intensity"][k][keep].contiguous()
        d_cat = sim["category"][k][keep].contiguous()
        m = int(d_int.shape[0])
        signals, total, none_count, fit = {}, 0, 0, None
        if m:
            d_len = torch.full((m,), int(d_int.shape[1]), dtype=torch.int32, device=d_int.device)
            fit = LN.lognormal_device(d_int, d_cat, d_len, None, None, prm=fit_prm)
            if bool((fit["status"] > LN.STATUS_NONE).any()):
                raise NotImplementedError("a simulated track has more surviving sequences than the budget, or an invalid length")
            found = fit["status"] == LN.STATUS_FOUND
            rows, cnt = torch.unique(fit["best_seq"][found], dim=0, return_counts=True)
            signals, _ = _tracks.tally_signals((LN.signal_of(tuple(row)) for row in rows.cpu().tolist()), cnt.cpu().tolist())
            total, none_count = m, m - int(found.sum())
        out[letter] = {"signals": signals, "total_count": total, "none_count": none_count, "kept": keep, "fit": fit}
    return out
