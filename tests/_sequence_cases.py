"""Shared by test_sequence_host.py and test_gpu_sequence.py: tests/golden/sequence_experiment.npz back into experiments, the
replay of the recorded call sequence (the generator's own Recorder, run on the package's classes) and the comparison."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sequence_experiment.npz")
NAMES = ("main", "wide")


def recorder_module():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_sequence_golden
    return gen_sequence_golden


def load():
    return np.load(GOLDEN)


def frames_of(g, name):
    """The frames as the GPU side gets them: the uint16 originals, or uint32 words where the reference's copy was scaled."""
    scale = int(g[name + "_scale"])
    fr = g[name + "_frames"]
    return fr if scale == 1 else fr.astype(np.uint32) * np.uint32(scale)


def sequences_of(g, name):
    """per field, per channel: (frames uint16 [F, H, W], offsets [(d_h, d_w)], detected [(h, w)] per frame, None)."""
    frames, off, det = g[name + "_frames"], g[name + "_offsets"], g[name + "_detected"]
    n_channels = len(g["channels"])
    flat = []
    for s in range(len(frames)):
        detected = [[] for _ in range(frames.shape[1])]
        for _, f, h, w in det[det[:, 0] == s].tolist():
            detected[f].append((h, w))
        offsets = [(0, 0)] + [(float(a), float(b)) for a, b in off[s, 1:]]
        flat.append((frames[s], offsets, detected, None))
    return [flat[e * n_channels:(e + 1) * n_channels] for e in range(int(g[name + "_n_fields"]))]


def pixels_of(g, name):
    scale = int(g[name + "_scale"])
    return (lambda a: a) if scale == 1 else (lambda a: a.astype(np.uint32) * np.uint32(scale))


def golden_tracer(g, name):
    """Stands in for trace_existing_spots (which needs the GPU tracker): the recorded traces, as the frames' own Spots."""
    def trace(rec):
        hw, seq = g[name + "_traces_hw"], g[name + "_traces_seq"]
        discarded = g[name + "_discarded_traced"].tolist()
        for s, (e, c, ex) in enumerate(rec.seqs):
            lookup = [{(sp.h, sp.w): sp for sp in im.spots} for im in ex.peptide_frames]
            ex.spot_traces = [[lookup[f][(h, w)] if h >= 0 else None for f, (h, w) in enumerate(row)]
                              for row in hw[seq == s].tolist()]
            ex.num_discarded_spots = discarded[list(g["channels"]).index(c)] if e == 0 else 0
    return trace


def replay(fl, g, name, trace=None):
    """The generator's call sequence on the classes of `fl` -> the same dictionary of records."""
    G = recorder_module()
    small = dict(radius=int(g[name + "_small"][0]), brim_size=int(g[name + "_small"][1]))
    return G.Recorder(fl, name, sequences_of(g, name), pixels_of(g, name), trace=trace).run(small)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        a, b = a.astype(np.float64), b.astype(np.float64)
        return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


def assert_replay_equals_golden(out, g, name):
    """Every recorded item: equality (bit patterns for doubles, bytes for the texts)."""
    assert len(out) > 40
    for key, value in out.items():
        assert key in g.files, key
        exp = g[key]
        if exp.dtype == np.uint8 and exp.ndim == 1:                 # a text
            assert bytes(np.asarray(value, dtype=np.uint8)) == bytes(exp), \
                "%s differs:\n%s\n--- expected ---\n%s" % (key, bytes(value).decode()[:1500], bytes(exp).decode()[:1500])
        else:
            assert same(value, exp), key


def btcp_order(traces_hw, traces_seq, n_fields, n_channels):
    """Trace indices in the order binary_trace_categories_photometry lists them: channel, field, pattern in order of first
    appearance, trace."""
    order = []
    det = traces_hw[:, :, 0] >= 0
    for c in range(n_channels):
        for e in range(n_fields):
            groups = {}
            for t in np.flatnonzero(traces_seq == e * n_channels + c).tolist():
                groups.setdefault(tuple(det[t].tolist()), []).append(t)
            for members in groups.values():
                order += members
    return np.array(order, dtype=np.int64)
