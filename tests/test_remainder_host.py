"""Remainder correction of track photometries, host side: the fixture against the numpy restatement and against the library's
host route, bit for bit; the C ABI declarations; the dict the reader would give on the written file; the command line with
--host; and every refusal made before a launch.  No GPU needed."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

import _remainder_reference as RR
from _remainder_cases import MODES, arrays_of, cases, counts, same_adjusted, same_arrays, same_medians
from _util import ROOT


def _library(key):
    from fluorosequencingimageanalysis_amd import remainder as RM
    return RM.remainder_adjust_2 if key == "r2" else RM.remainder_adjust


def test_fixture_is_not_vacuous():
    cs = cases()
    kept, dropped, split, nans = counts(cs)
    assert kept >= 0.25 * (kept + dropped) and dropped >= 0.25 * (kept + dropped) and split >= 10 and nans >= 5, (kept, dropped, split, nans)
    assert {c["F"] for c in cs} == {1, 2, 3, 5, 7, 8, 64} and {c["min"] for c in cs} >= {0, 1, 5}
    csvs = [c for c in cs if c["csv"] is not None]
    assert len(csvs) == 4 and all(".5," in c["csv"] and ",None,None," in c["csv"] for c in csvs)
    for c in csvs:
        assert list(c["photometries"]) == ["ch1", "ch2"] and all(len(d) == 6 for d in c["photometries"].values())
        if c["min"] == 5:                                          # a channel without a kept field is in neither output
            assert list(c["r2"][0]) == list(c["r2"][1]) == list(c["r1"][0]) == list(c["r1"][1]) == ["ch1"]
    assert any(np.isinf(m).any() for c in cs for f in c["r2"][1].values() for m in f.values())


def test_reader_gives_the_recorded_photometries(tmp_path):
    from fluorosequencingimageanalysis_amd import lognormal as LN
    for c in cases():
        if c["csv"] is None:
            continue
        path = tmp_path / (c["name"] + ".csv")
        path.write_text(c["csv"])
        got = LN.read_track_photometries_csv(str(path), downstep_filtered=False)[0]
        assert got == c["photometries"] and [list(d) for d in got.values()] == [list(d) for d in c["photometries"].values()], c["name"]


def test_restatement_equals_golden():
    for c in cases():
        for key, mode in MODES:
            adjusted, medians = RR.adjust_dict(c["photometries"], c["F"], c["min"], mode)
            same_adjusted(adjusted, c[key][0], (c["name"], key))
            same_medians(medians, c[key][1], (c["name"], key))


def test_host_route_equals_golden():
    for c in cases():
        for key, _ in MODES:
            adjusted, medians = _library(key)(c["photometries"], c["F"], minimum_r_per_field=c["min"], device=None)
            same_adjusted(adjusted, c[key][0], (c["name"], key))
            same_medians(medians, c[key][1], (c["name"], key))


def test_host_records_equal_restatement_in_any_order():
    """The array interface on the host: shuffled tracks with arbitrary segment ids, results in the caller's order."""
    from fluorosequencingimageanalysis_amd import remainder as RM
    rng = np.random.default_rng(5)
    for c in cases()[::3]:
        rows, cats, seg, keys = arrays_of(c["photometries"], c["F"])
        perm = rng.permutation(len(rows))
        ids = (seg * 7 - 3)[perm]
        for _, mode in MODES:
            got = RM.remainder_adjust_records(rows[perm], cats[perm], ids, mode, c["min"], device=None)
            exp = RR.adjust_records(rows[perm], cats[perm], ids, mode, c["min"])
            same_arrays(got, exp, (c["name"], mode))
            assert np.array_equal(got["segment_ids"], exp["segment_ids"])


def test_header_matches_binding_and_library():
    from fluorosequencingimageanalysis_amd import _native, _native_remainder as NR, remainder as RM
    hdr = open(os.path.join(ROOT, "include", "fsq_remainder.h")).read()
    declared = set(re.findall(r"\b(fsq_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(NR.EXPORTED) == {"fsq_remainder_workspace_bytes", "fsq_remainder_adjust"}
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    L = ctypes.CDLL(_native.LIB_PATH)
    for name in declared:
        getattr(L, name)
    assert int(re.search(r"#define FSQ_REMAINDER_LDS_MAX (\d+)", hdr).group(1)) == NR.LDS_MAX == RM.LDS_MAX
    assert int(re.search(r"#define FSQ_REMAINDER_MAX_FRAMES (\d+)", hdr).group(1)) == NR.MAX_FRAMES == 64
    assert (int(re.search(r"#define FSQ_REMAINDER_RATIO (\d+)", hdr).group(1)), int(re.search(r"#define FSQ_REMAINDER_ADDITIVE (\d+)", hdr).group(1))) \
        == (NR.MODE_RATIO, NR.MODE_ADDITIVE)
    assert ctypes.sizeof(NR.FsqRemainderParams) == 8
    assert "fsq_remainder.h" in open(os.path.join(ROOT, "fluorosequencingimageanalysis_amd", "csrc", "Makefile")).read()


def test_c_abi_refuses_bad_arguments_before_a_launch():
    """Every refusal is made on the host; the pointers are never touched (they point nowhere)."""
    from fluorosequencingimageanalysis_amd import _native, _native_remainder as NR
    L = NR.lib()
    p = ctypes.c_void_p(4096)
    ok = NR.FsqRemainderParams(NR.MODE_RATIO, 5)
    assert L.fsq_remainder_workspace_bytes(10, 8, 2) >= 10 * 8 * 8 + 10 * 4
    assert L.fsq_remainder_workspace_bytes(0, 8, 0) > 0
    for n, F, S in ((-1, 8, 1), (1 << 31, 8, 1), (10, 0, 1), (10, -1, 1), (10, 65, 1), (10, 8, -1), (10, 8, 1 << 28)):
        assert L.fsq_remainder_workspace_bytes(n, F, S) == _native.FSQ_EINVAL, (n, F, S)
        expected = _native.FSQ_ENOTIMPL if F > 64 else _native.FSQ_EINVAL
        assert L.fsq_remainder_adjust(p, p, p, n, F, S, ctypes.byref(ok), p, p, p, p, p, 1 << 40, None) == expected, (n, F, S)
    call = lambda prm, *ptrs, ws_bytes=1 << 20: L.fsq_remainder_adjust(ptrs[0], ptrs[1], ptrs[2], 10, 8, 2, prm, ptrs[3], ptrs[4], ptrs[5],
                                                                         ptrs[6], ptrs[7], ws_bytes, None)
    for missing in range(8):
        ptrs = [None if i == missing else p for i in range(8)]
        assert call(ctypes.byref(ok), *ptrs) == _native.FSQ_EINVAL, missing
    assert call(None, *[p] * 8) == _native.FSQ_EINVAL
    assert call(ctypes.byref(NR.FsqRemainderParams(2, 5)), *[p] * 8) == _native.FSQ_EINVAL
    assert call(ctypes.byref(ok), *[p] * 8, ws_bytes=L.fsq_remainder_workspace_bytes(10, 8, 2) - 1) == _native.FSQ_EINVAL
    assert call(ctypes.byref(ok), *([p] * 7 + [ctypes.c_void_p(4100)])) == _native.FSQ_EINVAL      # a workspace off 8 bytes


def test_as_read_equals_writing_and_reading(tmp_path):
    from fluorosequencingimageanalysis_amd import lognormal as LN, remainder as RM
    done = 0
    for c in cases():
        for key, _ in MODES:
            adjusted = c[key][0]
            finite = all(np.isfinite(v[1]).all() for cd in adjusted.values() for fd in cd.values() for v in fd.values())
            if not finite:
                with pytest.raises((ValueError, OverflowError)):
                    RM.adjusted_photometries_as_read(adjusted)
                continue
            path = str(tmp_path / ("%s_%s.csv" % (c["name"], key)))
            RM.write_adjusted_csv(adjusted, c["F"], path)
            back = LN.read_track_photometries_csv(path, downstep_filtered=False)[0]
            got = RM.adjusted_photometries_as_read(adjusted)
            assert got == back and list(got) == list(back), (c["name"], key)
            for channel in back:
                assert list(got[channel]) == list(back[channel])
                assert all(list(got[channel][f]) == list(back[channel][f]) for f in back[channel])
            done += bool(back)
    assert done >= 20


def _expected_csv(adjusted, F):
    from fluorosequencingimageanalysis_amd.pflib import _py2_str
    lines = [",".join(["CHANNEL", "FIELD", "H", "W", "CATEGORY"] + ["FRAME %d" % f for f in range(F)])]
    for channel, cdict in adjusted.items():
        for field, fdict in cdict.items():
            for (h, w), (category, values, _) in fdict.items():
                cat = str(tuple(category))
                lines.append(",".join([channel, str(field), str(h), str(w), '"%s"' % cat if "," in cat else cat] +
                                      [_py2_str(np.float64(v)) for v in values]))
    return ("\r\n".join(lines) + "\r\n").encode()


def test_command_line_on_the_host(tmp_path, capsys):
    from fluorosequencingimageanalysis_amd import remainder_correction as CLI
    for c in cases():
        if c["csv"] is None:
            continue
        path = str(tmp_path / ("track_photometries_%s.csv" % c["name"]))
        with open(path, "w") as f:
            f.write(c["csv"])
        out = CLI.main(["remainder_correction", path, "--min", str(c["min"]), "--host", "--save_adjustments", "--print_adjustments"])
        assert out["num_frames"] == c["F"] and out["output_filepath"] == path + "_adjusted.csv"
        assert open(path + "_adjusted.csv", "rb").read() == _expected_csv(c["r2"][0], c["F"]), c["name"]
        raw = open(path + "_adjustments.pkl", "rb").read()
        assert raw.endswith(b".") and b"numpy._core" not in raw                     # protocol 0, numpy 1.x module paths
        same_medians(pickle.loads(raw), c["r2"][1], c["name"])
        printed = capsys.readouterr().out
        assert printed.startswith("{'ch1': {") and "np.float64" not in printed
    # without the flag nothing but the CSV is written, and the default minimum is the reference's 5
    c = next(c for c in cases() if c["csv"] is not None and c["min"] == 5)
    path = str(tmp_path / "plain.csv")
    with open(path, "w") as f:
        f.write(c["csv"])
    out = CLI.main(["remainder_correction", path, "--host"])
    assert out["args"].min == 5 and out["adjustments_output_filepath"] is None and not os.path.exists(path + "_adjustments.pkl")
    assert open(path + "_adjusted.csv", "rb").read() == _expected_csv(c["r2"][0], c["F"])
    with pytest.raises(Exception, match="Older methods not supported."):
        CLI.main(["remainder_correction", path, "--host", "--method", "2"])


def test_refusals_before_any_launch():
    from fluorosequencingimageanalysis_amd import remainder as RM
    on = lambda F: (True,) * F
    good = {"ch1": {0: {(1, 1): (on(3), (10, 20, 30), 1), (2, 2): (on(3), (11, 21, 31), 2)}}}
    for fn in (RM.remainder_adjust_2, RM.remainder_adjust):
        for device in (None, "cuda"):
            kw = dict(minimum_r_per_field=1, device=device)
            with pytest.raises(ValueError):                                         # a track of another length
                fn({"ch1": {0: {(1, 1): (on(3), (10, 20, 30), 1), (2, 2): (on(3), (11, 21), 2)}}}, 3, **kw)
            with pytest.raises(ValueError):                                         # a category of another length
                fn({"ch1": {0: {(1, 1): (on(2), (10, 20, 30), 1)}}}, 3, **kw)
            with pytest.raises(ValueError):                                         # num_frames is not the tracks'
                fn(good, 4, **kw)
            with pytest.raises(ValueError):
                fn({"ch1": {0: {(1, 1): ((), (), 1)}}}, 0, **kw)
            with pytest.raises(NotImplementedError):
                fn({"ch1": {0: {(1, 1): (on(65), tuple(range(1, 66)), 1)}}}, 65, **kw)
            for bad in (float("nan"), float("inf"), -float("inf"), 2.0 ** 52 + 2, -(2.0 ** 53)):
                with pytest.raises(ValueError):
                    fn({"ch1": {0: {(1, 1): (on(3), (10, bad, 30), 1)}}}, 3, **kw)
        fn({"ch1": {0: {(1, 1): (on(3), (10, 2.0 ** 52, -2.0 ** 52), 1)}}}, 3, minimum_r_per_field=1, device=None)   # the limit itself
    for device in (None, "cuda"):
        with pytest.raises(ValueError):
            RM.remainder_adjust_records(np.zeros((3, 0)), np.zeros(3, np.uint64), np.zeros(3, np.int64), device=device)
        with pytest.raises(NotImplementedError):
            RM.remainder_adjust_records(np.ones((3, 65)), np.zeros(3, np.uint64), np.zeros(3, np.int64), device=device)
        with pytest.raises(ValueError):
            RM.remainder_adjust_records(np.ones((3, 4)), np.zeros(2, np.uint64), np.zeros(3, np.int64), device=device)
        with pytest.raises(ValueError):
            RM.remainder_adjust_records(np.ones((3, 4)), np.zeros(3, np.uint64), np.zeros(4, np.int64), device=device)
        with pytest.raises(ValueError):
            RM.remainder_adjust_records([[1, 2, 3], [1, 2]], [on(3), on(2)], [0, 0], device=device)
        with pytest.raises(ValueError):
            RM.remainder_adjust_records(np.ones((3, 4)), np.zeros(3, np.uint64), np.zeros(3, np.int64), mode="other", device=device)
