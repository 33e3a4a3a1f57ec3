"""Host checks of the sequence-experiment path (no GPU): the NumPy restatement of the kernel against the reference's
records, the C header against the binding and the cross-compiled library, argument checking, and the host side of the
flexlibrary classes - replayed on the golden experiment with the restatement standing in for the device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _sequence_cases as C  # noqa: E402
import _sequence_reference as R  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return C.load()


def _records(g, name, **kw):
    return R.records(C.frames_of(g, name), g[name + "_traces_hw"], g[name + "_traces_seq"], g[name + "_offsets"], **kw)


@pytest.mark.parametrize("name", C.NAMES)
def test_restatement_equals_reference_records(golden, name):
    g = golden
    hw, seq = g[name + "_traces_hw"], g[name + "_traces_seq"]
    order = C.btcp_order(hw, seq, int(g[name + "_n_fields"]), len(g["channels"]))
    small = dict(radius=int(g[name + "_small"][0]), brim_size=int(g[name + "_small"][1]))
    for key, kw in (("btcp_plain", dict(interpolate=False)), ("btcp_interp", dict(interpolate=True)),
                    ("btcp_small_plain", dict(interpolate=False, **small)), ("btcp_small_interp", dict(interpolate=True, **small)),
                    ("btcp_simple_interp", dict(interpolate=True, method="simple"))):
        r = _records(g, name, **kw)
        assert np.array_equal(r["hw"][order], g[name + "_" + key + "_hw"]), key
        assert C.same(r["photometry"][order], g[name + "_" + key + "_phot"]), key
        cat = np.array([[(int(c) >> f) & 1 for f in range(hw.shape[1])] for c in r["category"]], dtype=bool)
        assert np.array_equal(cat[order], g[name + "_" + key + "_cat"]), key
        if kw["interpolate"]:
            assert np.array_equal(r["hw"], g[name + "_filled_hw"]), key
    # the discard_invalid_traces split, at the default hat and at the small one
    for tag, kw in (("", {}), ("_small", small)):
        r = _records(g, name, interpolate=True, **kw)
        assert np.array_equal(hw[r["trace_valid"]], g[name + "_valid%s_hw" % tag])
        assert np.array_equal(seq[r["trace_valid"]], g[name + "_valid%s_seq" % tag])
        assert np.array_equal(r["hw"][~r["trace_valid"]], g[name + "_invalid%s_hw" % tag])
        assert np.array_equal(seq[~r["trace_valid"]], g[name + "_invalid%s_seq" % tag])
    # counts per (sequence, pattern) of the traces that stay
    r = _records(g, name, interpolate=True)
    n_ch = len(g["channels"])
    counts = R.category_counts(r["category"], seq, select=r["trace_valid"])
    got = {}
    for s, p, n in zip(counts["seq"].tolist(), counts["pattern"].tolist(), counts["count"].tolist()):
        got[(s % n_ch, s // n_ch, tuple(bool((p >> f) & 1) for f in range(hw.shape[1])))] = n
    exp = {(c, e, tuple(cat)): n for c, e, cat, n in zip(g[name + "_counts_chan"].tolist(), g[name + "_counts_field"].tolist(),
                                                         g[name + "_counts_cat"].tolist(), g[name + "_counts_n"].tolist())}
    assert got == exp


def test_header_matches_binding_and_library():
    from fluorosequencingimageanalysis_amd import _native, _native_sequence
    hdr = open(os.path.join(ROOT, "include", "fsq_sequence.h")).read()
    declared = set(re.findall(r"\b(fsq_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_native_sequence.EXPORTED)
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    L = ctypes.CDLL(_native.LIB_PATH)
    for name in declared:
        getattr(L, name)
    for name, value in (("FSQ_SEQUENCE_MAX_FRAMES", _native_sequence.MAX_FRAMES), ("FSQ_SEQUENCE_MEXICAN_HAT", 0),
                        ("FSQ_SEQUENCE_SIMPLE", _native_sequence.METHOD_SIMPLE), ("FSQ_SEQUENCE_DETECTED", _native_sequence.DETECTED),
                        ("FSQ_SEQUENCE_INTERPOLATED", _native_sequence.INTERPOLATED),
                        ("FSQ_SEQUENCE_WINDOW_INSIDE", _native_sequence.WINDOW_INSIDE)):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == value
    # every argument list has the header's length
    for name, (_, args) in _native_sequence._SIGS.items():
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, hdr).group(1)
        assert len(args) == decl.count(",") + 1, name
    L.fsq_sequence_workspace_bytes.restype = ctypes.c_int64
    L.fsq_sequence_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32]
    assert L.fsq_sequence_workspace_bytes(3, 7) == 3 * 7 * 2 * 8
    assert L.fsq_sequence_workspace_bytes(0, 7) < 0
    L.fsq_sequence_category_counts_workspace_bytes.restype = ctypes.c_int64
    L.fsq_sequence_category_counts_workspace_bytes.argtypes = [ctypes.c_int64]
    assert L.fsq_sequence_category_counts_workspace_bytes(100) == 3 * 256 * 4
    assert L.fsq_sequence_category_counts_workspace_bytes(-1) < 0


def test_argument_checking():
    from fluorosequencingimageanalysis_amd import sequencing as S
    hw = np.full((3, 4, 2), -1, np.int32)
    hw[:, 0] = (5, 5)
    off = np.zeros((2, 4, 2))
    ok = S.check_arguments((2, 4, 16, 16), hw, [0, 1, 1], off)
    assert ok[0].dtype == np.int32 and ok[1].dtype == np.int32 and ok[2].dtype == np.float64 and ok[3] == 0
    assert S.check_arguments((2, 4, 16, 16), hw, [0, 1, 1], off, method="simple")[3] == 1
    with pytest.raises(ValueError):
        S.check_arguments((2, 4, 16, 16), hw[:, :3], [0, 1, 1], off)                # frames of the traces
    with pytest.raises(ValueError):
        S.check_arguments((2, 4, 16, 16), hw, [0, 1], off)                          # one sequence per trace
    with pytest.raises(ValueError):
        S.check_arguments((2, 4, 16, 16), hw, [0, 1, 2], off)                       # sequence out of range
    with pytest.raises(ValueError):
        S.check_arguments((2, 4, 16, 16), hw, [0, 1, 1], off[:1])                   # offsets per sequence
    bad = off.copy()
    bad[1, 0, 1] = 0.5
    with pytest.raises(ValueError, match=r"The first image's offset must be \(0, 0\) by definiton\."):
        S.check_arguments((2, 4, 16, 16), hw, [0, 1, 1], bad)
    with pytest.raises(NotImplementedError):
        S.check_arguments((1, 65, 16, 16), np.full((1, 65, 2), 1), [0], np.zeros((1, 65, 2)))
    with pytest.raises(ValueError, match="Uknown method specified."):
        S.check_arguments((2, 4, 16, 16), hw, [0, 1, 1], off, method="other")
    with pytest.raises(NotImplementedError):
        S.check_arguments((2, 4, 16, 16), hw, [0, 1, 1], off, method="sextractor")
    with pytest.raises(ValueError):
        S.check_arguments((2, 4, 16, 16), hw, [0, 1, 1], off, spot_size=4)
    with pytest.raises(ValueError):
        S.check_arguments((2, 4, 16, 16), hw + 0.5, [0, 1, 1], off)
    assert S.pattern_to_tuple(0b0101, 4) == (True, False, True, False)


def test_static_helpers(tmp_path):
    from fluorosequencingimageanalysis_amd import flexlibrary as fl
    E = fl.Experiment
    assert E.trace_to_binary([None, 1, None, "x"]) == [False, True, False, True]
    assert E.truefalse_to_onoff((True, False, True)) == "[ON]  [OFF] [ON] "
    paths = [str(tmp_path / d / f) for d in ("c2", "c0", "c1") for f in ("b.png", "a.png")]
    frame_indexed, field_indexed = E.easy_sort_target_images(paths)
    base = str(tmp_path)
    assert frame_indexed == {i: [os.path.join(base, "c%d" % i, n) for n in ("a.png", "b.png")] for i in range(3)}
    assert field_indexed == {k: [os.path.join(base, "c%d" % i, n) for i in range(3)] for k, n in enumerate(("a.png", "b.png"))}
    assert fl._filtered_counts({(True, False): 1, (False, True): 2, (True, True): 3}, True) == {(True, False): 1, (True, True): 3}
    assert fl._filtered_counts({(True, False): 1, (False, True): 2, (True, True): 3}, False) == {(True, True): 3}
    with pytest.raises(ValueError, match="Uknown method specified."):
        fl._photometry_plan("other", {})
    for method in ("sextractor", "maximum", "sigmas"):
        with pytest.raises(NotImplementedError):
            fl._photometry_plan(method, {})
    assert fl._photometry_plan("simple", {"photometry_method": "mexican_hat", "radius": 4})["radius"] == 4
    with pytest.raises(DeprecationWarning):
        fl.MultifieldSequenceExperiment([])
    assert fl.SequenceExperiment.mdma_adjustment(100.0, 1, {"mdma": (0.0, 0.25)}) == 75.0
    assert fl.SequenceExperiment.mdma_adjustment(100.0, 1, {}) == 100.0


@pytest.mark.parametrize("name", C.NAMES)
def test_interpolate_spots_on_the_host_equals_reference(golden, name):
    """SequenceExperiment.interpolate_spots (host arithmetic) on every hole of every trace == the recorded fill_in_trace."""
    from fluorosequencingimageanalysis_amd import flexlibrary as fl
    g = golden
    hw, seq, filled = g[name + "_traces_hw"], g[name + "_traces_seq"], g[name + "_filled_hw"]
    frames = C.frames_of(g, name)
    F = hw.shape[1]
    for s in range(len(frames)):
        images = [fl.Image(image=frames[s, f]) for f in range(F)]
        ex = fl.SequenceExperiment(peptide_frames=images)
        ex.offsets = [(0, 0)] + [(float(a), float(b)) for a, b in g[name + "_offsets"][s, 1:]]
        for t in np.flatnonzero(seq == s):
            trace = [fl.Spot(images[f], int(h), int(w), 5) if h >= 0 else None for f, (h, w) in enumerate(hw[t])]
            f = 0
            while f < F:
                if trace[f] is not None:
                    f += 1
                    continue
                e = f
                while e < F and trace[e] is None:
                    e += 1
                a, b = (f - 1 if f > 0 else 0), (e if e < F else F - 1)
                spots = ex.interpolate_spots((trace[a], a), (trace[b], b))
                got = [(-1, -1) if sp is None else (sp.h, sp.w) for sp in spots]
                for i in range(f, e):
                    assert got[i - a] == tuple(filled[t, i]), (name, s, t, i)
                f = e
        n_new = sum(len(im.spots) for im in images)
        assert n_new > 0


@pytest.mark.parametrize("name", C.NAMES)
def test_classes_replay_the_recorded_call_sequence(golden, name, monkeypatch):
    """The flexlibrary classes through the script's call sequence, with the NumPy restatement standing in for the kernel and the
    recorded traces for the tracker: every recorded item is equal - counters, spot_count() after every stage, MDMA tuples, the
    CSV and string texts byte for byte."""
    from fluorosequencingimageanalysis_amd import flexlibrary as fl
    from fluorosequencingimageanalysis_amd import sequencing as S

    def records(frames, trace_hw, trace_seq, offsets, method='mexican_hat', radius=9, brim_size=6, spot_size=5, interpolate=True,
                device=None, counts=True):
        hw, seq, off, _ = S.check_arguments(np.shape(frames), trace_hw, trace_seq, offsets, method, radius, brim_size, spot_size)
        return R.records(np.asarray(frames).astype(np.int64), hw, seq, off, method, radius, brim_size, spot_size, interpolate)
    monkeypatch.setattr(S, "sequence_photometry_records", records)
    out = C.replay(fl, golden, name, trace=C.golden_tracer(golden, name))
    C.assert_replay_equals_golden(out, golden, name)
