"""The proteome-scale Monte-Carlo of the reference's MCsimlib.py on the GPU: with these labels, this many Edman cycles and
these error rates, which proteins of a proteome give a signal that no other protein gives?

    peptides = attach(cleave(proteome, 'E'), 'C')                     # {protein: ((head, tail), ...)}
    records = monte_carlo_records(peptides, p, b, u, windows, sample_size=1000, seed=7)
    uniq = uniques_records(records, worst_ratio=10.0, absolute_min=5)
    identifiable_proteins(uniq)                                       # {protein: number of its passing signals}

WHAT IS BUILT.  cleave, attach, homogenize, homogenize_attached (:88-279), random_signal (:863-1074), SignalTrie (:1224-1547:
add_descendant, get_descendant, leaf_iterator, count_nodes, find_uniques, find_uniques_absolute) and monte_carlo_trie
(:1787-1849).  The device path (include/fsq_proteome_mc.h) is three kernels: fsq_proteome_signals samples every attached
peptide sample_size times, one lane per sample, into 64-bit signal keys; fsq_proteome_tally counts (signal, protein) pairs in
two open-addressing tables that stay on the device; fsq_proteome_uniques scans every signal's proteins as find_uniques does.
host=True runs the NumPy twins of _host_proteome_mc instead; both give the same integers.  SignalTrie, monte_carlo_trie and
random_signal are drop-ins built from the records, one Python object per signal: the slow path.
Shorter runs from the same simulation (:1560-1759): fsq_proteome_project re-tallies the counted pairs under one key mask per
cycle count - key & mask is the signal a run of c cycles would have shown, which is what SignalTrie.truncating_projection
leaves in a trie - for many cycle counts in one launch (project_device, projection_records), adds one run into another as
SignalTrie.merge does (merge_device, merge_records) and feeds the same compaction, sorts and scan for the whole curve of
identifiable proteins against cycle count (cycle_curve_records; the command line is proteome_cycles).  SignalTrie.graft,
prune, merge and truncating_projection are host methods of the drop-in; load_proteome (:55-86) reads a proteome pickle.
A grid of chemistries over the same peptides: fsq_proteome_signals_points and fsq_proteome_tally_points run every point
(p, b, u) of a grid in one launch each, one lane per (point, row), into per-point tables (grid_points, grid_device, point_tables,
grid_records); grid_curve_records gives the identifiable proteins at every point through one compaction, three sorts and one
scan per group of points (the command line is proteome_sweep).  Row g of point k is sample first_sample + k * sample_stride + g:
with sample_stride = 0, the default, every point sees the same draws.

ORDER CONTRACTS.  (1) Wherever the reference iterates `windows` - a dict, whose order Python 2 leaves open - this module
iterates sorted(windows); a signal is a tuple sorted by position, then by acid in that order.  (2) Proteins are scanned in
ascending protein index, the insertion order of `peptides`: the first-seen order of the reference's signal_count dicts when
proteins are sampled one after the other, as monte_carlo_trie does.

DRAW CONTRACT.  Sample first_sample + peptide_index * sample_size + j reads stream 3 of that item under `seed`
(_host_peptide_sim.uniform; the peptide simulator uses streams 0 .. 2), in the order of the reference's random.random()
calls: see _host_proteome_mc.  A result depends on (seed, first_sample, the order of peptides, sample_size) and on nothing
else: not on chunk_rows, not on the table sizes.  The reference's monte_carlo_trie cannot run as shipped (its randsiggen C
extension is not in its tree), so there is no draw-for-draw comparison with it; random_signal is compared draw for draw.

LIMITS, each a NotImplementedError or ValueError that names it: the windows have at most 64 observable (position, acid)
pairs (the 64-bit key) at positions 1 .. 63 for at most 8 acids; a peptide has at most 64 labelled residues, head and tail
together, and a head of at most 255 residues; an Edman delay row (one per gap length d, under p) has at most 4 096 entries;
signal_slots <= 2^27 and pair_slots <= 2^28, a table too small for the run raises ValueError naming the keyword.

NOT BUILT: edman_failure_gaps, perfect, window_filter (the enumerating, non-Monte-Carlo route) and the Polyfluor* classes
(peptide_simulator covers the chemistry, for several label letters too: multilabel_records); each raises NotImplementedError saying so.  SlimSignalTrie is not there at
all, and a shorter run is a projection of the long run's draws, not a new photobleaching simulation.  discard, truncate_heads and the
*_MP / monte_carlo_dictionary functions raise DeprecationWarning, as in the reference."""
import ctypes
import random as _random

import numpy as np

from . import _host_proteome_mc as H
from ._host_proteome_mc import (attach, cleave, discard, edman_failure_gaps_MP, homogenize, homogenize_attached,     # noqa: F401
                                monte_carlo_dictionary, monte_carlo_dictionary_MP, monte_carlo_trie_MP, truncate_heads,
                                key_of, signal_of)

DEFAULT_CHUNK_ROWS = 1 << 22


def _not_built(name, why):
    def f(*args, **kwargs):
        raise NotImplementedError("%s is not built: %s" % (name, why))
    f.__name__ = name
    return f


edman_failure_gaps = _not_built("edman_failure_gaps", "the enumerating route is out of scope; use monte_carlo_records")
perfect = _not_built("perfect", "the enumerating route is out of scope (and perfect raises DeprecationWarning in the reference)")
window_filter = _not_built("window_filter", "random_signal already applies the windows")
PolyfluorSignal = _not_built("PolyfluorSignal", "peptide_simulator covers the chemistry (several label letters: multilabel_records)")
PolyfluorSignalTrie = _not_built("PolyfluorSignalTrie", "peptide_simulator covers the chemistry (several label letters: multilabel_records)")
PolyfluorPeptide = _not_built("PolyfluorPeptide", "peptide_simulator covers the chemistry (several label letters: multilabel_records)")
PolyfluorPeptide_v2 = _not_built("PolyfluorPeptide_v2", "peptide_simulator covers the chemistry (several label letters: multilabel_records)")


def _engine():
    from . import engine
    return engine


def _native():
    from . import _native_proteome_mc
    return _native_proteome_mc


def fresh_seed():
    return _random.SystemRandom().getrandbits(63)


# ---- tables ----

def proteome_table(peptides, windows):
    """Attached peptides {protein: ((head, tail), ...)} as the flat layout of _host_proteome_mc.peptide_table, proteins indexed
    in dict order.  Raises for a peptide or windows beyond the limits."""
    table = H.peptide_table(peptides, windows)
    if not len(table["protein"]):
        raise ValueError("no attached peptide")
    return table


def _as_table(peptides, windows):
    return peptides if isinstance(peptides, dict) and "label_start" in peptides else proteome_table(peptides, windows)


def _check_run(table, p, b, u, sample_size, seed, first_sample):
    p, b, u, S = float(p), float(b), float(u), int(sample_size)
    if not (0.0 <= p <= 1.0 and 0.0 <= u <= 1.0 and b >= 0.0):
        raise ValueError("p and u must be in [0, 1] and b must not be negative")
    if S < 1:
        raise ValueError("sample_size must be positive")
    total = len(table["protein"]) * S
    if not 0 <= int(seed) < 1 << 64 or first_sample < 0 or first_sample + total > 1 << 64:
        raise ValueError("seed and sample ids must be in 0 .. 2^64 - 1")
    return p, b, u, S, total


def _pow2_at_least(n):
    return 1 << max(int(n) - 1, 0).bit_length()


def device_table(table, p, b, device=None):
    """The peptide table and the two chemistry tables (edman_table under p, bleach_table under b) as CUDA tensors."""
    torch = _engine()._torch()
    dev = torch.device(device or "cuda")
    max_d = H.max_gap(table)
    start, values = H.edman_table(p, max_d)
    up = lambda a: torch.from_numpy(np.array(a)).to(dev)           # (a copy: the cached tables are read-only)
    return {"protein": up(table["protein"]), "n_head": up(table["n_head"]), "label_start": up(table["label_start"]),
            "labels": up(np.append(table["labels"], np.uint32(0)).view(np.int32)), "edman_start": up(start),
            "edman": up(np.append(values, 0.0)), "bleach": up(H.bleach_table(b)), "max_d": max_d, "n_peptides": len(table["protein"]),
            "layout": table["layout"], "device": dev}


def signals_device(dtable, u, sample_size, seed, first_sample=0, first_row=0, n_rows=None, with_draws=False):
    """fsq_proteome_signals: (key int64 [n_rows] holding the uint64 keys' bits, protein int32 [n_rows], n_draws int32 [n_rows] or
    None).  Enqueued on the current stream, not synchronised."""
    torch, NP = _engine()._torch(), _native()
    layout, dev = dtable["layout"], dtable["device"]
    n = dtable["n_peptides"] * int(sample_size) - int(first_row) if n_rows is None else int(n_rows)
    prm = NP.FsqProteomeParams()
    for a in range(len(layout.order)):
        prm.E[a], prm.O[a], prm.base[a] = layout.E[a], layout.O[a], layout.base[a]
    prm.n_acids, prm.max_d, prm.u = len(layout.order), dtable["max_d"], float(u)
    prm.seed, prm.first_sample, prm.sample_size = int(seed), int(first_sample), int(sample_size)
    key = torch.empty(max(n, 0), dtype=torch.int64, device=dev)
    protein = torch.empty(max(n, 0), dtype=torch.int32, device=dev)
    draws = torch.empty(max(n, 0), dtype=torch.int32, device=dev) if with_draws else None
    _engine().launch(NP.lib().fsq_proteome_signals, "fsq_proteome_signals", dev, ctypes.byref(prm), dtable["protein"].data_ptr(),
                     dtable["n_head"].data_ptr(), dtable["label_start"].data_ptr(), dtable["labels"].data_ptr(), dtable["n_peptides"],
                     dtable["edman_start"].data_ptr(), dtable["edman"].data_ptr(), dtable["bleach"].data_ptr(), int(first_row), n,
                     key.data_ptr() if n > 0 else None, protein.data_ptr() if n > 0 else None,
                     draws.data_ptr() if with_draws and n > 0 else None)
    return key, protein, draws


def new_tables(signal_slots, pair_slots, device, n_masks=None):
    """The empty tables of fsq_proteome_tally: signals int64 [signal_slots] (0: free), pairs int64 [pair_slots] (-1: free), counts
    int64 [pair_slots], overflow int32 [2].  With n_masks, fsq_proteome_project's: each with a leading [n_masks]."""
    torch, NP = _engine()._torch(), _native()
    sa, sb = int(signal_slots), int(pair_slots)
    if sa < 1 or sa & (sa - 1) or sa > NP.MAX_SIGNAL_SLOTS:
        raise ValueError("signal_slots=%d must be a power of two up to 2^27" % sa)
    if sb < 1 or sb & (sb - 1) or sb > NP.MAX_PAIR_SLOTS:
        raise ValueError("pair_slots=%d must be a power of two up to 2^28" % sb)
    lead = () if n_masks is None else (int(n_masks),)
    return {"signals": torch.zeros(lead + (sa,), dtype=torch.int64, device=device),
            "pairs": torch.full(lead + (sb,), -1, dtype=torch.int64, device=device),
            "counts": torch.zeros(lead + (sb,), dtype=torch.int64, device=device),
            "overflow": torch.zeros(lead + (2,), dtype=torch.int32, device=device)}


def tally_device(tables, d_key, d_protein):
    """fsq_proteome_tally: adds (key, protein) rows (int64 key bits [n], int32 [n]) to the tables.  Enqueued, not synchronised."""
    torch, NP = _engine()._torch(), _native()
    n = int(d_key.shape[0])
    if d_key.dtype != torch.int64 or d_protein.dtype != torch.int32 or tuple(d_protein.shape) != (n,) or d_key.dim() != 1:
        raise ValueError("int64 keys [n] and int32 proteins [n] are needed")
    if not (d_key.is_contiguous() and d_protein.is_contiguous()):
        raise ValueError("contiguous tensors are needed")
    _engine().launch(NP.lib().fsq_proteome_tally, "fsq_proteome_tally", d_key.device, d_key.data_ptr() if n else None,
                     d_protein.data_ptr() if n else None, n, tables["signals"].data_ptr(), int(tables["signals"].shape[0]),
                     tables["pairs"].data_ptr(), tables["counts"].data_ptr(), int(tables["pairs"].shape[0]),
                     tables["overflow"].data_ptr())


def check_tables(tables):
    over = tables["overflow"].cpu().tolist()
    if over[0]:
        raise ValueError("more distinct signals than signal_slots=%d: pass a larger power of two" % int(tables["signals"].shape[0]))
    if over[1]:
        raise ValueError("more distinct (signal, protein) pairs than pair_slots=%d: pass a larger power of two" % int(tables["pairs"].shape[0]))


def pairs_device(tables):
    """The occupied pairs of table B, sorted by (key as uint64, protein): key int64 (bits), protein int32, count int64, and
    segment int64 [n_signals + 1], the starts of the signals."""
    torch = _engine()._torch()
    occupied = tables["pairs"] != -1
    pair, count = tables["pairs"][occupied], tables["counts"][occupied]
    key, protein = tables["signals"][pair >> 32], pair & 0xffffffff
    order = torch.sort(protein, stable=True)[1]
    order = order[torch.sort((key ^ (-1 << 63))[order], stable=True)[1]]
    key, protein, count = key[order].contiguous(), protein[order].to(torch.int32).contiguous(), count[order].contiguous()
    n = int(key.shape[0])
    new = torch.ones(n, dtype=torch.bool, device=key.device)
    if n > 1:
        new[1:] = key[1:] != key[:-1]
    segment = torch.cat([new.nonzero().reshape(-1), torch.tensor([n], dtype=torch.int64, device=key.device)]).contiguous()
    return key, protein, count, segment


def uniques_device(d_protein, d_count, d_segment, modes, demote=False):
    """fsq_proteome_uniques over sorted pairs: a dict of CUDA tensors [n_signals] named as _host_proteome_mc.UNIQUE_FIELDS."""
    torch, NP = _engine()._torch(), _native()
    n = int(d_segment.shape[0]) - 1
    dev = d_segment.device
    prm = NP.FsqUniquesParams()
    prm.ratio_mode, prm.worst_ratio, prm.absolute_min, prm.has_maximum_secondary, prm.maximum_secondary = modes
    prm.demote = int(bool(demote))
    tt = {np.int32: torch.int32, np.int64: torch.int64, np.uint8: torch.uint8}
    out = {name: torch.empty(max(n, 0), dtype=tt[dtype], device=dev) for name, dtype in H.UNIQUE_FIELDS}
    ptr = lambda t: t.data_ptr() if n > 0 else None
    _engine().launch(NP.lib().fsq_proteome_uniques, "fsq_proteome_uniques", dev, ptr(d_protein), ptr(d_count), ptr(d_segment), n,
                     ctypes.byref(prm), *[ptr(out[name]) for name, _ in H.UNIQUE_FIELDS])
    return out


# ---- the run ----

def monte_carlo_device(table, p, b, u, sample_size, seed, first_sample=0, chunk_rows=DEFAULT_CHUNK_ROWS, signal_slots=None,
                       pair_slots=None, device=None):
    """Sample every peptide of `table` (proteome_table) sample_size times and count (signal, protein) pairs, in chunks of at most
    chunk_rows samples (the result does not depend on it); everything stays on the device.  Returns a dict: `tables`
    (new_tables), `names`, `layout`, `rows`.
    signal_slots (table A, 8 bytes a slot) and pair_slots (table B, 16 bytes a slot) are powers of two; by default both are the
    power of two at or above twice the number of samples, A at most 2^26 (512 MiB) and B at most 2^26 (1 GiB): a run cannot
    have more distinct signals or pairs than samples, so the defaults overflow only beyond 2^25 samples.  A table that turns
    out too small raises ValueError naming its keyword."""
    torch = _engine()._torch()
    p, b, u, S, total = _check_run(table, p, b, u, sample_size, seed, first_sample)
    chunk = int(chunk_rows)
    if chunk < 1:
        raise ValueError("chunk_rows must be positive")
    dtable = device_table(table, p, b, device)
    default = min(max(_pow2_at_least(2 * total), 1024), 1 << 26)
    tables = new_tables(default if signal_slots is None else signal_slots, default if pair_slots is None else pair_slots,
                        dtable["device"])
    for first in range(0, total, chunk):
        key, protein, _ = signals_device(dtable, u, S, seed, first_sample, first, min(chunk, total - first))
        tally_device(tables, key, protein)
    check_tables(tables)
    return {"tables": tables, "names": table["names"], "layout": table["layout"], "rows": total}


def monte_carlo_records(peptides, p, b, u, windows=None, sample_size=100, seed=0, first_sample=0, chunk_rows=DEFAULT_CHUNK_ROWS,
                        signal_slots=None, pair_slots=None, device=None, host=False):
    """The (signal, protein) counts of a run as NumPy arrays sorted by (key, protein): a dict with key uint64, protein int32,
    count int64, names (proteins in index order) and layout (the key's).  `peptides` is an attached-peptide dict (with
    `windows`) or a proteome_table."""
    table = _as_table(peptides, windows)
    if host:
        p, b, u, S, total = _check_run(table, p, b, u, sample_size, seed, first_sample)
        keys, _ = H.signals(table, p, b, u, S, seed, first_sample)
        k, pr, c = H.tally(keys, H.row_proteins(table, S, 0, total))
    else:
        run = monte_carlo_device(table, p, b, u, sample_size, seed, first_sample, chunk_rows, signal_slots, pair_slots, device)
        key, protein, count, _ = pairs_device(run["tables"])
        k, pr, c = key.cpu().numpy().view(np.uint64), protein.cpu().numpy(), count.cpu().numpy()
    return {"key": k, "protein": pr, "count": c, "names": list(table["names"]), "layout": table["layout"]}


def _uniques_any(source, modes, demote, host, device):
    if "tables" in source:                                  # a monte_carlo_device result
        if host:
            raise ValueError("host=True needs records, not a device result")
        key, protein, count, segment = pairs_device(source["tables"])
    elif host:
        out = H._uniques((source["key"], source["protein"], source["count"]), modes, demote)
        out.update(names=source["names"], layout=source["layout"], demote=bool(demote),
                   triples=(source["key"], source["protein"], source["count"]))
        return out
    else:
        torch = _engine()._torch()
        dev = torch.device(device or "cuda")
        key = torch.from_numpy(np.ascontiguousarray(source["key"]).view(np.int64)).to(dev)
        protein = torch.from_numpy(np.ascontiguousarray(source["protein"], np.int32)).to(dev)
        count = torch.from_numpy(np.ascontiguousarray(source["count"], np.int64)).to(dev)
        segment = torch.from_numpy(H.segments(source["key"])).to(dev)
    got = uniques_device(protein, count, segment, modes, demote)
    out = {name: t.cpu().numpy() for name, t in got.items()}
    triples = (key.cpu().numpy().view(np.uint64), protein.cpu().numpy(), count.cpu().numpy())
    out["segment"] = segment.cpu().numpy()
    out["key"] = triples[0][out["segment"][:-1]]
    out.update(names=source["names"], layout=source["layout"], demote=bool(demote), triples=triples)
    return out


def uniques_records(records_or_device, worst_ratio, absolute_min, maximum_secondary=None, demote=False, host=False, device=None):
    """find_uniques' scan for every signal of monte_carlo_records' or monte_carlo_device's result: the arrays of
    _host_proteome_mc.uniques (key, best_protein, best_count, second_protein, second_count, n_ties, tertiary, passed, segment)
    plus names, layout and the sorted triples.  demote=True is an extension: the true top two."""
    return _uniques_any(records_or_device, H.scan_modes(worst_ratio, absolute_min, maximum_secondary), demote, host, device)


def uniques_absolute_records(records_or_device, minimum_best, maximum_secondary, demote=False, host=False, device=None):
    """find_uniques_absolute's scan, as uniques_records."""
    return _uniques_any(records_or_device, H.scan_modes(None, minimum_best, maximum_secondary, absolute=True), demote, host, device)


def uniques_dict(uniq):
    """The reference's dict of the passing signals of a uniques_records result."""
    return H.unique_dict(uniq, uniq["triples"], uniq["layout"], uniq["names"], uniq["demote"])


def identifiable_proteins(uniq):
    """{protein: the number of passing signals for which it is best}, proteins in index order."""
    best = uniq["best_protein"][uniq["passed"] != 0]
    n = np.bincount(best, minlength=len(uniq["names"]))
    return {uniq["names"][i]: int(n[i]) for i in np.flatnonzero(n).tolist()}


# ---- shorter runs: projections, merges and the cycle curve (:1674-1759) ----

def last_position(layout):
    """The layout's last observable position: a cycle count at or above it changes no signal."""
    return H.last_position(layout)


def _same_space(a, b):
    if list(a["names"]) != list(b["names"]):
        raise ValueError("the two runs have different names: their protein indices do not mean the same proteins")
    if a["layout"].windows != b["layout"].windows:
        raise ValueError("the two runs have different layouts (windows): their keys do not mean the same signals")


def _source_pairs(source, device=None):
    """The sorted pairs of a run (monte_carlo_device, cycle_tables) or of records on the device: key int64 (bits), protein int32,
    count int64 and the number of distinct signals."""
    torch = _engine()._torch()
    if "tables" in source:
        if source["tables"]["pairs"].dim() != 1:
            raise ValueError("the tables of one cycle count are needed: cycle_tables(projection, i)")
        key, protein, count, segment = pairs_device(source["tables"])
        return key, protein, count, int(segment.shape[0]) - 1
    dev = torch.device(device or "cuda")
    k = np.ascontiguousarray(source["key"], np.uint64)
    key = torch.from_numpy(k.view(np.int64)).to(dev)
    protein = torch.from_numpy(np.ascontiguousarray(source["protein"], np.int32)).to(dev)
    count = torch.from_numpy(np.ascontiguousarray(source["count"], np.int64)).to(dev)
    return key, protein, count, len(np.unique(k))


def project_into(tables, d_key, d_protein, d_count, d_mask, mode=H.PROJECT):
    """fsq_proteome_project: the counted pairs (int64 key bits [n], int32 [n], int64 [n] or None for weight 1) under the masks
    d_mask (int64 bits [n_masks]) into `tables` - new_tables(..., n_masks=n_masks), or one table where n_masks is 1.  Enqueued,
    not synchronised."""
    torch, NP = _engine()._torch(), _native()
    n, n_masks = int(d_key.shape[0]), int(d_mask.shape[0])
    if d_key.dtype != torch.int64 or d_protein.dtype != torch.int32 or d_key.dim() != 1 or tuple(d_protein.shape) != (n,):
        raise ValueError("int64 keys [n] and int32 proteins [n] are needed")
    if d_count is not None and (d_count.dtype != torch.int64 or tuple(d_count.shape) != (n,)):
        raise ValueError("int64 counts [n] are needed")
    if d_mask.dtype != torch.int64 or d_mask.dim() != 1:
        raise ValueError("int64 masks [n_masks] are needed")
    if not all(t is None or t.is_contiguous() for t in (d_key, d_protein, d_count, d_mask) + tuple(tables.values())):
        raise ValueError("contiguous tensors are needed")
    sa, sb = int(tables["signals"].shape[-1]), int(tables["pairs"].shape[-1])
    if (tables["signals"].numel(), tables["pairs"].numel(), tables["counts"].numel(), tables["overflow"].numel()) != \
            (n_masks * sa, n_masks * sb, n_masks * sb, n_masks * 2):
        raise ValueError("the tables do not hold %d masks" % n_masks)
    _engine().launch(NP.lib().fsq_proteome_project, "fsq_proteome_project", d_key.device, d_key.data_ptr() if n else None,
                     d_protein.data_ptr() if n else None, d_count.data_ptr() if n and d_count is not None else None, n,
                     d_mask.data_ptr(), n_masks, int(mode), tables["signals"].data_ptr(), sa, tables["pairs"].data_ptr(),
                     tables["counts"].data_ptr(), sb, tables["overflow"].data_ptr())


def cycle_tables(projection, i):
    """The tables of the i-th cycle count of a project_device result, in the form of new_tables: pairs_device reads them,
    tally_device and project_into go on adding to them.  With names and layout, so that it serves where a run does."""
    return {"tables": {k: v[i] for k, v in projection["tables"].items()}, "names": projection["names"], "layout": projection["layout"]}


def check_projection(projection):
    """Raises ValueError for the first cycle count whose tables were too small."""
    t = projection["tables"]
    for i, (a, b) in enumerate(t["overflow"].cpu().tolist()):
        if a:
            raise ValueError("more distinct signals than signal_slots=%d at cycles=%d: pass a larger power of two"
                             % (int(t["signals"].shape[-1]), projection["cycles"][i]))
        if b:
            raise ValueError("more distinct (signal, protein) pairs than pair_slots=%d at cycles=%d: pass a larger power of two"
                             % (int(t["pairs"].shape[-1]), projection["cycles"][i]))


def project_device(run_or_records, cycles, mode="project", signal_slots=None, pair_slots=None, masks_per_launch=None, device=None,
                   mask_major=False):
    """The tally of a run (monte_carlo_device, cycle_tables) or of records under every cycle count of `cycles`, on the device:
    mode 'project' folds every signal onto what a run of c cycles would have shown (truncating_projection, :1697-1759), 'within'
    keeps the signals whose last position is at most c (merge's cycles=, :1694).  Returns a dict: `tables` (new_tables with
    n_masks=len(cycles): row i is the tally of cycles[i]; see cycle_tables), `cycles`, `masks`, `names`, `layout`, `mode`.
    signal_slots / pair_slots are powers of two; by default the power of two at or above twice the source's distinct signals and
    twice its pairs, which a projection cannot exceed.  At most masks_per_launch cycle counts go into one launch (None: all; the
    entry takes 4 096), which bounds a launch's items, not the tables: they are held for every cycle count asked for.  The result
    does not depend on it, nor on mask_major (the item order of the kernel, there to be timed).  A table that is too small raises
    ValueError naming its keyword and the cycle count."""
    torch, NP = _engine()._torch(), _native()
    which = H.mode_of(mode) | (NP.MASK_MAJOR if mask_major else 0)
    layout = run_or_records["layout"]
    masks = H.cycle_masks(layout, cycles)
    cycles = [int(c) for c in cycles]
    if not cycles:
        raise ValueError("no cycle count")
    per = len(cycles) if masks_per_launch is None else int(masks_per_launch)
    if per < 1:
        raise ValueError("masks_per_launch must be positive")
    per = min(per, NP.MAX_MASKS)
    key, protein, count, n_signals = _source_pairs(run_or_records, device)
    tables = new_tables(_pow2_at_least(2 * n_signals) if signal_slots is None else signal_slots,
                        _pow2_at_least(2 * int(key.shape[0])) if pair_slots is None else pair_slots, key.device, n_masks=len(cycles))
    d_mask = torch.from_numpy(masks.view(np.int64)).to(key.device)
    for lo in range(0, len(cycles), per):
        project_into({k: v[lo:lo + per] for k, v in tables.items()}, key, protein, count, d_mask[lo:lo + per], which)
    out = {"tables": tables, "cycles": cycles, "masks": masks, "names": list(run_or_records["names"]), "layout": layout, "mode": mode}
    check_projection(out)
    return out


def _records(triples, source):
    k, p, c = triples
    return {"key": k, "protein": p, "count": c, "names": list(source["names"]), "layout": source["layout"]}


def _records_of_tables(run):
    key, protein, count, _ = pairs_device(run["tables"])
    return _records((key.cpu().numpy().view(np.uint64), protein.cpu().numpy(), count.cpu().numpy()), run)


def projection_records(source, cycles, host=False, mode="project", device=None):
    """The records of `source` (records, or a run on the device) as a run of `cycles` Edman cycles would have given them, in the
    shape of monte_carlo_records: uniques_records, uniques_dict and trie_of_records take them unchanged."""
    if host:
        if "tables" in source:
            raise ValueError("host=True needs records, not a device result")
        mask = H.cycle_masks(source["layout"], [cycles])[0]
        return _records(H.project((source["key"], source["protein"], source["count"]), mask, mode), source)
    return _records_of_tables(cycle_tables(project_device(source, [cycles], mode, device=device), 0))


def merge_device(run_a, run_b, cycles=None):
    """SignalTrie.merge (:1674-1696) on the device: adds the pairs of run_b - with cycles, those whose last position is at most
    cycles - into run_a's tables, and returns run_a.  A table of run_a that is too small raises ValueError naming its keyword."""
    torch = _engine()._torch()
    _same_space(run_a, run_b)
    key, protein, count, _ = _source_pairs(run_b, run_a["tables"]["pairs"].device)
    mask = np.array([H.ALL_ONES], np.uint64) if cycles is None else H.cycle_masks(run_a["layout"], [cycles])
    project_into(run_a["tables"], key, protein, count, torch.from_numpy(mask.view(np.int64)).to(key.device),
                 H.PROJECT if cycles is None else H.WITHIN)
    check_tables(run_a["tables"])
    if "rows" in run_a and "rows" in run_b:
        run_a["rows"] += run_b["rows"]
    return run_a


def merge_records(a, b, cycles=None, host=False, device=None):
    """The records of a plus those of b (with cycles: those of b whose last position is at most cycles), as merge leaves a trie."""
    _same_space(a, b)
    if host:
        mask = None if cycles is None else H.cycle_masks(a["layout"], [cycles])[0]
        return _records(H.merge(*[(r["key"], r["protein"], r["count"]) for r in (a, b)], mask=mask), a)
    torch = _engine()._torch()
    key, protein, count, n_signals = _source_pairs(a, device)
    tables = new_tables(_pow2_at_least(2 * (n_signals + len(np.unique(b["key"])))), _pow2_at_least(2 * (len(a["key"]) + len(b["key"]))),
                        key.device)
    project_into(tables, key, protein, count, torch.full((1,), -1, dtype=torch.int64, device=key.device))
    run = {"tables": tables, "names": list(a["names"]), "layout": a["layout"]}
    return _records_of_tables(merge_device(run, b, cycles))


def _sorted_projection(projection):
    """Every cycle count's occupied pairs in one pass, sorted by (cycle index, key as uint64, protein): cycle int64, key int64
    (bits), protein int32, count int64 and segment int64 [signals + 1] over all cycle counts.  Reads any tables with a leading
    dimension: a grid_device result's just as well, the point's index standing for the cycle index."""
    torch = _engine()._torch()
    t = projection["tables"]
    occupied = t["pairs"] != -1
    cyc = occupied.nonzero(as_tuple=True)[0]
    pair, count = t["pairs"][occupied], t["counts"][occupied]
    key, protein = t["signals"][cyc, pair >> 32], pair & 0xffffffff
    order = torch.sort(protein, stable=True)[1]
    order = order[torch.sort((key ^ (-1 << 63))[order], stable=True)[1]]
    order = order[torch.sort(cyc[order], stable=True)[1]]
    cyc, key, protein, count = cyc[order], key[order].contiguous(), protein[order].to(torch.int32).contiguous(), count[order].contiguous()
    n = int(key.shape[0])
    new = torch.ones(n, dtype=torch.bool, device=key.device)
    if n > 1:
        new[1:] = (key[1:] != key[:-1]) | (cyc[1:] != cyc[:-1])
    segment = torch.cat([new.nonzero().reshape(-1), torch.tensor([n], dtype=torch.int64, device=key.device)]).contiguous()
    return cyc, key, protein, count, segment


def cycle_curve_records(source, worst_ratio, absolute_min, maximum_secondary=None, cycles=None, absolute=False, demote=False,
                        host=False, device=None):
    """Identifiable proteins against the number of Edman cycles, from one simulation: find_uniques' scan (absolute=True:
    find_uniques_absolute's, absolute_min its minimum_best) of `source` (records, or a run on the device) projected onto every
    cycle count of `cycles` (None: 1 .. the layout's last observable position).  Proteins are scanned in ascending index (order
    contract (2)).  Returns int64 arrays over the cycle counts - cycles, n_signals, n_pairs, samples_detected (the sum of counts),
    n_passing_signals, n_identifiable_proteins - with identifiable uint8 [len(cycles)][n_proteins] (1: best for a passing signal)
    and names.  The long run's draws are kept, as the reference's projection keeps them; the curve need not be monotone.
    On the device all cycle counts go through one projection launch, one compaction, three sorts and one fsq_proteome_uniques
    launch over the concatenated segments."""
    layout, names = source["layout"], list(source["names"])
    if cycles is None:
        cycles = range(1, H.last_position(layout) + 1)
    cycles = [int(c) for c in cycles]
    H.cycle_masks(layout, cycles)
    if not cycles:
        raise ValueError("no cycle count: the layout has no observable position")
    modes = H.scan_modes(None if absolute else worst_ratio, absolute_min, maximum_secondary, absolute=absolute)
    if host:
        if "tables" in source:
            raise ValueError("host=True needs records, not a device result")
        out = H.cycle_curve((source["key"], source["protein"], source["count"]), layout, len(names), cycles, modes, demote)
        out["names"] = names
        return out
    out = _curve_of_tables(project_device(source, cycles, device=device), len(cycles), len(names), modes, demote)
    out = dict(cycles=np.array(cycles, np.int64), **out)
    out["names"] = names
    return out


def _curve_of_tables(stacked, C, P, modes, demote):
    """The curve's arrays over the C leading tables of `stacked` (a projection's cycle counts, a grid's points) for P proteins:
    one compaction, three sorts and one fsq_proteome_uniques launch over the concatenated segments."""
    torch = _engine()._torch()
    cyc, _, protein, count, segment = _sorted_projection(stacked)
    got = uniques_device(protein, count, segment, modes, demote)
    dev = cyc.device
    of_signal = cyc[segment[:-1]]
    passed = got["passed"] != 0
    zeros = lambda: torch.zeros(C, dtype=torch.int64, device=dev)               # noqa: E731
    identifiable = torch.zeros(C * max(P, 1), dtype=torch.uint8, device=dev)
    identifiable[(of_signal * max(P, 1) + got["best_protein"].to(torch.int64))[passed]] = 1
    identifiable = identifiable.reshape(C, max(P, 1))[:, :P]
    out = {"n_signals": torch.bincount(of_signal, minlength=C),
           "n_pairs": torch.bincount(cyc, minlength=C), "samples_detected": zeros().index_add_(0, cyc, count),
           "n_passing_signals": zeros().index_add_(0, of_signal, passed.to(torch.int64)),
           "n_identifiable_proteins": identifiable.sum(dim=1, dtype=torch.int64), "identifiable": identifiable.contiguous()}
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- a grid of (p, b, u) points over the same peptides (fsq_proteome_signals_points, fsq_proteome_tally_points) ----

DEFAULT_TABLE_BYTES = 1 << 33


def grid_points(ps, bs, us):
    """The product of the three axes in p-major order, as a list of (p, b, u): u runs fastest."""
    return H.grid_points(ps, bs, us)


def _check_grid(table, points, sample_size, seed, first_sample, sample_stride):
    """_check_run for every point under its own first sample: (points as float triples, sample_size, rows per point, stride)."""
    points = H.check_points(points, sample_stride)
    stride = int(sample_stride)
    for k, (p, b, u) in enumerate(points):
        _, _, _, S, total = _check_run(table, p, b, u, sample_size, seed, int(first_sample) + k * stride)
    return points, S, total, stride


def grid_device_table(table, points, device=None):
    """device_table for a grid: the peptide table, one Edman table per distinct p (all under the same max_d) and one bleach
    table per distinct b as CUDA tensors, and `points`, the FsqProteomePoint records (uint8 [n_points][16]) that name them."""
    torch, NP = _engine()._torch(), _native()
    dev = torch.device(device or "cuda")
    max_d = H.max_gap(table)
    ps, bs, edman_index, bleach_index = H.shared_tables(points)
    start, values = H.stacked_edman_tables(ps, max_d)
    records = np.zeros(len(points), np.dtype([("u", "<f8"), ("edman_table", "<i4"), ("bleach_table", "<i4")]))
    records["u"], records["edman_table"], records["bleach_table"] = [u for _, _, u in points], edman_index, bleach_index
    assert records.dtype.itemsize == ctypes.sizeof(NP.FsqProteomePoint)
    up = lambda a: torch.from_numpy(np.array(a)).to(dev)           # (a copy: the cached tables are read-only)
    return {"protein": up(table["protein"]), "n_head": up(table["n_head"]), "label_start": up(table["label_start"]),
            "labels": up(np.append(table["labels"], np.uint32(0)).view(np.int32)), "edman_start": up(start),
            "edman": up(np.append(values, 0.0)), "bleach": up(np.stack([H.bleach_table(b) for b in bs])),
            "points": up(records.view(np.uint8).reshape(len(points), 16)), "n_edman_tables": len(ps), "n_bleach_tables": len(bs),
            "max_d": max_d, "n_peptides": len(table["protein"]), "layout": table["layout"], "device": dev}


def signals_points_device(gtable, sample_size, seed, first_sample=0, sample_stride=0, first_row=0, n_rows=None, with_draws=False,
                          first_point=0, n_points=None):
    """fsq_proteome_signals_points for points first_point .. first_point + n_points - 1 of a grid_device_table (default: all):
    (key int64 [n_points][n_rows] holding the uint64 keys' bits, protein int32 [n_rows], n_draws int32 [n_points][n_rows] or
    None).  Row g of the k-th of these points is sample first_sample + k * sample_stride + g.  Enqueued, not synchronised."""
    torch, NP = _engine()._torch(), _native()
    layout, dev = gtable["layout"], gtable["device"]
    lo = int(first_point)
    K = int(gtable["points"].shape[0]) - lo if n_points is None else int(n_points)
    if lo < 0 or K < 0 or lo + K > int(gtable["points"].shape[0]):
        raise ValueError("points beyond the table's %d" % int(gtable["points"].shape[0]))
    n = gtable["n_peptides"] * int(sample_size) - int(first_row) if n_rows is None else int(n_rows)
    prm = NP.FsqProteomeParams()
    for a in range(len(layout.order)):
        prm.E[a], prm.O[a], prm.base[a] = layout.E[a], layout.O[a], layout.base[a]
    prm.n_acids, prm.max_d, prm.u = len(layout.order), gtable["max_d"], 0.0
    prm.seed, prm.first_sample, prm.sample_size = int(seed), int(first_sample), int(sample_size)
    shape = (max(K, 0), max(n, 0))
    key = torch.empty(shape, dtype=torch.int64, device=dev)
    protein = torch.empty(max(n, 0), dtype=torch.int32, device=dev)
    draws = torch.empty(shape, dtype=torch.int32, device=dev) if with_draws else None
    some = n > 0 and K > 0
    _engine().launch(NP.lib().fsq_proteome_signals_points, "fsq_proteome_signals_points", dev, ctypes.byref(prm),
                     gtable["points"][lo:].data_ptr() if K > 0 else None, K, int(sample_stride), gtable["protein"].data_ptr(),
                     gtable["n_head"].data_ptr(), gtable["label_start"].data_ptr(), gtable["labels"].data_ptr(), gtable["n_peptides"],
                     gtable["edman_start"].data_ptr(), gtable["edman"].data_ptr(), gtable["n_edman_tables"],
                     gtable["bleach"].data_ptr(), gtable["n_bleach_tables"], int(first_row), n,
                     key.data_ptr() if some else None, protein.data_ptr() if some else None,
                     draws.data_ptr() if with_draws and some else None)
    return key, protein, draws


def tally_points_device(tables, d_key, d_protein):
    """fsq_proteome_tally_points: adds row t of point k (int64 key bits [n_points][n], int32 proteins [n]) to table k of `tables`
    (new_tables(..., n_masks=n_points)).  Enqueued, not synchronised."""
    torch, NP = _engine()._torch(), _native()
    if d_key.dim() != 2 or d_key.dtype != torch.int64 or d_protein.dtype != torch.int32 or tuple(d_protein.shape) != (int(d_key.shape[1]),):
        raise ValueError("int64 keys [n_points][n] and int32 proteins [n] are needed")
    K, n = int(d_key.shape[0]), int(d_key.shape[1])
    if not all(t.is_contiguous() for t in (d_key, d_protein) + tuple(tables.values())):
        raise ValueError("contiguous tensors are needed")
    sa, sb = int(tables["signals"].shape[-1]), int(tables["pairs"].shape[-1])
    if tables["signals"].dim() != 2 or (tables["signals"].numel(), tables["pairs"].numel(), tables["counts"].numel(),
                                        tables["overflow"].numel()) != (K * sa, K * sb, K * sb, K * 2):
        raise ValueError("the tables do not hold %d points" % K)
    _engine().launch(NP.lib().fsq_proteome_tally_points, "fsq_proteome_tally_points", d_key.device, d_key.data_ptr() if n else None,
                     d_protein.data_ptr() if n else None, K, n, tables["signals"].data_ptr(), sa, tables["pairs"].data_ptr(),
                     tables["counts"].data_ptr(), sb, tables["overflow"].data_ptr())


def check_grid(grid):
    """Raises ValueError for the first point whose tables were too small."""
    t = grid["tables"]
    for i, (a, b) in enumerate(t["overflow"].cpu().tolist()):
        where = "point %d (p=%r, b=%r, u=%r)" % ((grid.get("first_point", 0) + i,) + tuple(grid["points"][i]))
        if a:
            raise ValueError("more distinct signals than signal_slots=%d at %s: pass a larger power of two"
                             % (int(t["signals"].shape[-1]), where))
        if b:
            raise ValueError("more distinct (signal, protein) pairs than pair_slots=%d at %s: pass a larger power of two"
                             % (int(t["pairs"].shape[-1]), where))


def _default_slots(total):
    return min(max(_pow2_at_least(2 * total), 1024), 1 << 26)


def _grid_pass(table, gtable, points, lo, hi, S, total, seed, first_sample, stride, chunk, signal_slots, pair_slots):
    """Points lo .. hi - 1 of a grid_device_table sampled and tallied into fresh tables: a grid_device result."""
    K = hi - lo
    tables = new_tables(signal_slots, pair_slots, gtable["device"], n_masks=K)
    for first in range(0, total, chunk):
        key, protein, _ = signals_points_device(gtable, S, seed, first_sample + lo * stride, stride, first, min(chunk, total - first),
                                                first_point=lo, n_points=K)
        tally_points_device(tables, key, protein)
    grid = {"tables": tables, "points": list(points[lo:hi]), "names": table["names"], "layout": table["layout"], "rows": total,
            "first_point": lo}
    check_grid(grid)
    return grid


def grid_device(table, points, sample_size, seed, first_sample=0, sample_stride=0, chunk_rows=DEFAULT_CHUNK_ROWS, signal_slots=None,
                pair_slots=None, device=None):
    """monte_carlo_device at every point (p, b, u) of `points` in one pass: every peptide of `table` sampled sample_size times a
    point and counted into that point's own tables, all on the device.  Row g of point k is sample first_sample + k *
    sample_stride + g: with sample_stride = 0 (the default) every point sees the same draws (common random numbers).  Points with
    the same p share an Edman table, points with the same b a bleach table; a point may appear twice, each copy gets its tables.
    A launch covers at most chunk_rows rows of every point (8 bytes of key a point and row) and the result does not depend on
    it.  Returns a dict: `tables` (new_tables(..., n_masks=len(points)): row i is the tally of points[i]; see
    point_tables), `points`, `names`, `layout`, `rows` (per point).  signal_slots / pair_slots are per point, by default
    monte_carlo_device's.  A table that is too small raises ValueError naming its keyword and the first such point."""
    points, S, total, stride = _check_grid(table, points, sample_size, seed, first_sample, sample_stride)
    chunk = int(chunk_rows)
    if chunk < 1:
        raise ValueError("chunk_rows must be positive")
    default = _default_slots(total)
    grid = _grid_pass(table, grid_device_table(table, points, device), points, 0, len(points), S, total, seed, int(first_sample),
                      stride, chunk, default if signal_slots is None else signal_slots, default if pair_slots is None else pair_slots)
    del grid["first_point"]
    return grid


def point_tables(grid, i):
    """The tables of the i-th point of a grid_device result, in the form of a run: pairs_device, uniques_records,
    cycle_curve_records, project_device and merge_device take it unchanged (the cycle_tables of a grid)."""
    return {"tables": {k: v[i] for k, v in grid["tables"].items()}, "names": grid["names"], "layout": grid["layout"],
            "rows": grid["rows"]}


def _grid_groups(n_points, total, points_per_pass, table_bytes, signal_slots, pair_slots):
    default = _default_slots(total)
    sa, sb = default if signal_slots is None else int(signal_slots), default if pair_slots is None else int(pair_slots)
    if points_per_pass is None:
        per = max(int(table_bytes) // (8 * sa + 16 * sb + 8), 1)
    else:
        per = int(points_per_pass)
        if per < 1:
            raise ValueError("points_per_pass must be positive")
    per = min(per, _native().MAX_POINTS, n_points)
    return sa, sb, [(lo, min(lo + per, n_points)) for lo in range(0, n_points, per)]


def grid_curve_records(peptides_or_table, points, worst_ratio, absolute_min, maximum_secondary=None, windows=None, sample_size=100,
                       seed=0, first_sample=0, sample_stride=0, absolute=False, demote=False, points_per_pass=None,
                       table_bytes=DEFAULT_TABLE_BYTES, host=False, chunk_rows=DEFAULT_CHUNK_ROWS, signal_slots=None, pair_slots=None,
                       device=None):
    """Identifiable proteins against the chemistry: the proteome Monte-Carlo and find_uniques' scan (absolute=True:
    find_uniques_absolute's, absolute_min its minimum_best) at every point (p, b, u) of `points`, what monte_carlo_device +
    uniques_records + identifiable_proteins give point by point.  `peptides_or_table` is an attached-peptide dict (with `windows`)
    or a proteome_table; draws as grid_device.  Returns arrays over the points - p, b, u (float64) and the int64 n_signals, n_pairs,
    samples_detected, n_passing_signals, n_identifiable_proteins - with identifiable uint8 [n_points][n_proteins] (1: best for a
    passing signal) and names.
    The points go through the device in groups of points_per_pass; by default as many as table_bytes of tables hold (8 bytes a
    signal slot, 16 a pair slot, per point), table_bytes by default 2^33 (8 GiB: 85 points at a million samples a point).  A
    group is one or more fsq_proteome_signals_points + fsq_proteome_tally_points launches, one compaction, three sorts and one
    fsq_proteome_uniques launch, and is reduced to its rows of the curve before the next group allocates.  The result does not
    depend on points_per_pass, table_bytes or chunk_rows.  host=True runs the NumPy twins point by point."""
    table = _as_table(peptides_or_table, windows)
    points, S, total, stride = _check_grid(table, points, sample_size, seed, first_sample, sample_stride)
    names = list(table["names"])
    modes = H.scan_modes(None if absolute else worst_ratio, absolute_min, maximum_secondary, absolute=absolute)
    if host:
        proteins = H.row_proteins(table, S, 0, total)
        triples = (H.tally(H.signals(table, p, b, u, S, seed, int(first_sample) + k * stride)[0], proteins)
                   for k, (p, b, u) in enumerate(points))
        out = H.grid_curve(triples, points, len(names), modes, demote)
        out["names"] = names
        return out
    chunk = int(chunk_rows)
    if chunk < 1:
        raise ValueError("chunk_rows must be positive")
    sa, sb, groups = _grid_groups(len(points), total, points_per_pass, table_bytes, signal_slots, pair_slots)
    gtable = grid_device_table(table, points, device)
    parts = []
    for lo, hi in groups:
        grid = _grid_pass(table, gtable, points, lo, hi, S, total, seed, int(first_sample), stride, chunk, sa, sb)
        parts.append(_curve_of_tables(grid, hi - lo, len(names), modes, demote))
        del grid
    out = {name: np.array([point[j] for point in points], np.float64) for j, name in enumerate("pbu")}
    out.update({name: np.concatenate([part[name] for part in parts]) for name in parts[0]})
    out["names"] = names
    return out


def grid_records(peptides_or_table, points, windows=None, sample_size=100, seed=0, first_sample=0, sample_stride=0,
                 chunk_rows=DEFAULT_CHUNK_ROWS, signal_slots=None, pair_slots=None, device=None, host=False):
    """{point: records}, each in the shape of monte_carlo_records, for small grids: all points go through one grid_device pass.
    Where a point stands twice its last copy is kept."""
    table = _as_table(peptides_or_table, windows)
    points, S, total, stride = _check_grid(table, points, sample_size, seed, first_sample, sample_stride)
    record = lambda k, pr, c: {"key": k, "protein": pr, "count": c, "names": list(table["names"]), "layout": table["layout"]}  # noqa: E731
    if host:
        proteins = H.row_proteins(table, S, 0, total)
        return {point: record(*H.tally(H.signals(table, *point, S, seed, int(first_sample) + k * stride)[0], proteins))
                for k, point in enumerate(points)}
    grid = grid_device(table, points, S, seed, first_sample, stride, chunk_rows, signal_slots, pair_slots, device)
    of_point, key, protein, count, _ = (t.cpu().numpy() for t in _sorted_projection(grid))
    edges = np.searchsorted(of_point, np.arange(len(points) + 1))
    return {point: record(key[lo:hi].view(np.uint64), protein[lo:hi], count[lo:hi])
            for point, lo, hi in zip(points, edges[:-1], edges[1:])}


def load_proteome(filename, silent=True):
    """:55-86: a pickle of {protein name: amino-acid sequence}.  Python 2's text pickles are read with encoding='latin1'."""
    import pickle
    import time
    t0 = time.perf_counter()
    if not silent:
        print("")
        print("unpickling proteome from " + str(filename))
    try:
        with open(filename, 'rb') as f:
            proteome = pickle.load(f, encoding="latin1")
    except Exception:
        print("Proteome unpickling error.")
        raise
    if not isinstance(proteome, dict) or not all(isinstance(k, str) and isinstance(v, str) for k, v in proteome.items()):
        raise ValueError("%s does not hold a dict of {name: sequence} strings" % filename)
    if not silent:
        print("proteome loaded in " + str(time.perf_counter() - t0) + " sec")
        print("...")
    return proteome


# ---- drop-ins ----

class SignalTrie(object):
    """The reference's prefix tree of signals (:1224-1547): a node is a (position, acid) block, holds its descendants and
    signal_count = {protein: count}.  The root is SignalTrie((None, None))."""

    def __init__(self, block):
        self.signal_block = tuple(block)
        self.descendants = {}
        self.signal_count = {}

    def add_descendant(self, subsignal, source_protein, count=1):
        """:1252-1281 (`count` more at once is this module's: the records arrive counted)."""
        if len(subsignal) == 0:
            return
        elif self.signal_block == (None, None):
            self.descendants.setdefault(subsignal[0], SignalTrie(subsignal[0]))
            self.descendants[subsignal[0]].add_descendant(subsignal, source_protein, count)
        elif len(subsignal) == 1:
            self.signal_count.setdefault(source_protein, 0)
            self.signal_count[source_protein] += count
        else:
            self.descendants.setdefault(subsignal[1], SignalTrie(subsignal[1]))
            self.descendants[subsignal[1]].add_descendant(subsignal[1:], source_protein, count)
        return self

    def get_descendant(self, subsignal):
        """:1308-1335."""
        if len(subsignal) == 0:
            return
        elif self.signal_block == (None, None):
            if subsignal[0] in self.descendants:
                return self.descendants[subsignal[0]].get_descendant(subsignal)
            return None
        elif len(subsignal) == 1:
            return self
        elif subsignal[1] in self.descendants:
            return self.descendants[subsignal[1]].get_descendant(subsignal[1:])
        return None

    def _iterate(self, every):
        for d_trie in self.descendants.values():
            for node in d_trie._iterate(every):
                if self.signal_block == (None, None):
                    yield node
                else:
                    yield ((self.signal_block,) + node[0], node[1], node[2])
        if every or len(self.signal_count) > 0:
            yield ((self.signal_block,), self.signal_count, self)

    def node_iterator(self):
        """:1336-1357."""
        return self._iterate(True)

    def leaf_iterator(self):
        """:1375-1397."""
        return self._iterate(False)

    def count_nodes(self):
        """:1533-1547: (empty nodes, used nodes)."""
        empty = used = 0
        for leaf in self.node_iterator():
            if len(leaf[1]) == 0:
                empty += 1
            else:
                used += 1
        return empty, used

    def graft(self, signal, signal_count):
        """:1630-1673: adds signal_count = {protein: count} to `signal`'s node, made if it is not there.  Returns self."""
        assert len(signal) > 0
        assert signal[0] == self.signal_block or self.signal_block == (None, None), \
            ('signal: ' + str(signal) + '; self.signal_block: ' + str(self.signal_block))
        assert len(signal_count) > 0
        if self.signal_block == (None, None):
            self.descendants.setdefault(signal[0], SignalTrie(signal[0])).graft(signal, signal_count)
        elif len(signal) == 1:
            for protein in signal_count:
                self.signal_count[protein] = self.signal_count.get(protein, 0) + signal_count[protein]
        else:
            self.descendants.setdefault(signal[1], SignalTrie(signal[1])).graft(signal[1:], signal_count)
        return self

    def _detach(self, block):
        """The counts of the descendant `block`, which leaves the trie if nothing hangs below it and is emptied otherwise."""
        child = self.descendants[block]
        if len(child.descendants) == 0:
            return self.descendants.pop(block).signal_count
        counts, child.signal_count = child.signal_count, {}
        return counts

    def prune(self, signal):
        """:1560-1629: takes `signal` out of the trie and returns (signal, its signal_count).  Called on the root."""
        assert len(signal) > 0
        root = self.signal_block == (None, None)
        if len(signal) == 1:
            assert root
            return (signal, self._detach(signal[0]))
        if root:
            assert signal[0] in self.descendants
            return self.descendants[signal[0]].prune(signal)
        assert signal[0] == self.signal_block, ('self.signal_block ' + str(self.signal_block) + '; signal ' + str(signal))
        assert signal[1] in self.descendants
        if len(signal) == 2:
            return (signal, self._detach(signal[1]))
        rest = self.descendants[signal[1]].prune(signal[1:])
        return ((self.signal_block,) + rest[0], rest[1])

    def merge(self, trie, cycles=None):
        """:1674-1696: grafts every leaf of `trie` (with cycles: those whose last position is at most cycles) onto this root."""
        assert self.signal_block == (None, None), 'merge can only be called on the root node'
        for signal, signal_count, _ in list(trie.leaf_iterator()):
            if cycles is None or signal[-1][0] <= cycles:
                self.graft(signal, signal_count)
        return self

    def _has_leaf(self):
        return next(self.leaf_iterator(), None) is not None

    def truncating_projection(self, cycles):
        """:1697-1759: folds every signal onto what `cycles` Edman cycles would have shown, in place.  Returns self.  (The root's
        block position is None, which Python 2 orders below every number: the root counts as within `cycles`.)"""
        for signal, signal_count, _ in list(self.leaf_iterator()):
            if signal[-1][0] > cycles:
                projected = tuple(block for block in signal if block[0] <= cycles)
                if projected:
                    self.graft(projected, signal_count)
        beyond = [(node, block) for signal, _, node in self.node_iterator() for block in node.descendants
                  if (signal[-1][0] is None or signal[-1][0] <= cycles) and block[0] > cycles]
        for node, block in beyond:
            del node.descendants[block]
        bare = [(node, block) for _, _, node in self.leaf_iterator() for block, child in node.descendants.items()
                if not child._has_leaf()]
        bare += [(self, block) for block, child in self.descendants.items() if not child._has_leaf()]
        for node, block in bare:
            del node.descendants[block]
        return self

    def _find(self, modes):
        out = {}
        for signal, signal_count, _ in self.leaf_iterator():
            names = list(signal_count)
            bp, bc, sp, sc, _, tertiary, passed = H.scan_counts(list(enumerate(signal_count.values())), *modes, False)
            if passed:
                second = (names[sp] if sp >= 0 else None, sc)
                ties = [(name, c) for name, c in signal_count.items() if c == sc and name != second[0]]
                out[signal] = [(names[bp], bc), [second] + ties, tertiary]
        return out

    def find_uniques(self, worst_ratio, absolute_min, maximum_secondary=None):
        """:1398-1486, every node's signal_count scanned in its dict's order."""
        return self._find(H.scan_modes(worst_ratio, absolute_min, maximum_secondary))

    def find_uniques_absolute(self, minimum_best, maximum_secondary):
        """:1487-1532."""
        return self._find(H.scan_modes(None, minimum_best, maximum_secondary, absolute=True))


def trie_of_records(records):
    """A SignalTrie holding the records' counts, signals added in (key, protein) order."""
    trie = SignalTrie((None, None))
    layout, names = records["layout"], records["names"]
    signal, last = None, None
    for key, protein, count in zip(records["key"].tolist(), records["protein"].tolist(), records["count"].tolist()):
        if key != last:
            signal, last = signal_of(key, layout), key
        trie.add_descendant(signal, names[protein], count)
    return trie


def monte_carlo_trie(peptides, p, b, u, windows, sample_size=100, random_seed=None, silent=True, host=False, **run):
    """:1787-1849: the SignalTrie of sample_size signals per attached peptide.  random_seed=None draws a fresh seed; an int
    reproduces a run (under this module's draw contract, not the reference's random.seed)."""
    seed = fresh_seed() if random_seed is None else int(random_seed)
    if not silent:
        print("monte_carlo_trie: seed %d" % seed)
    return trie_of_records(monte_carlo_records(peptides, p, b, u, windows, sample_size, seed, host=host, **run))


def random_signal(peptide, p=1.0, b=0.0, u=0.0, windows={}, seed=None, sample=0, host=False, device=None):
    """:863-1074 for one sample: the signal of sample id `sample` under `seed` (None: a fresh seed)."""
    seed = fresh_seed() if seed is None else int(seed)
    if host:
        H.layout_of(windows)
        return H.sample_signal(peptide, p, b, u, windows, seed, int(sample))[0]
    table = proteome_table({"": (tuple(peptide),)}, windows)
    p, b, u, _, _ = _check_run(table, p, b, u, 1, seed, int(sample))
    key, _, _ = signals_device(device_table(table, p, b, device), u, 1, seed, int(sample))
    return signal_of(int(key.cpu().numpy().view(np.uint64)[0]), table["layout"])
