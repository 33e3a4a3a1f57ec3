"""The timetrace experiment table on the GPU (include/fsq_timetrace.h): bit for bit against the reference's recorded CSV columns
(tests/golden/timetrace_experiment.npz) and, at the limits, against the NumPy restatement (tests/_timetrace_reference.py); the
frame stack -> table path, the object path and the command line against each other and against the reference's CSV text.
Nothing is compared with a tolerance."""
import os
import pickle

import numpy as np
import pytest

import _timetrace_reference as T
from _util import _bits
from test_timetrace_host import crafted_experiment

pytestmark = pytest.mark.gpu

SENTINEL = 77
PER_FRAME = ("plateau_index", "plateau_height", "plateau_length", "step_num", "step_size")


def _run(phots, plateaus, max_frames=None, lens=None, counts=None):
    """fsq_timetrace_table through table_device on host lists; every output is pre-filled with SENTINEL."""
    import torch
    from fluorosequencingimageanalysis_amd import timetrace as TT
    n = len(phots)
    mf = max_frames or max(max(len(p) for p in phots), 1)
    rows = np.zeros((n, mf))
    for i, p in enumerate(phots):
        rows[i, :len(p)] = p
    ln = np.array([len(p) for p in phots] if lens is None else lens, np.int32)
    st, so, hh, cnt = TT.plateau_rows(plateaus, mf)
    if counts is not None:
        cnt = np.array(counts, np.int32)
    out = TT.table_out(n, mf, torch.device("cuda"))
    for v in out.values():
        v.fill_(SENTINEL)
    TT.table_device(*(torch.from_numpy(a).cuda() for a in (rows, ln, st, so, hh, cnt)), out=out)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(h, t, phot, plateaus, what=None):
    """Row t of the device's result against the restatement; everything beyond the trace's frames is untouched."""
    r = T.table(phot, plateaus)
    n = len(phot)
    assert h["status"][t] == r["status"], what
    if r["status"] == T.INVALID:
        for k in PER_FRAME:
            assert (h[k][t] == SENTINEL).all(), (what, k)
        assert h["rss"][t] == h["tss"][t] == h["r2"][t] == SENTINEL, what
        return r
    for k in PER_FRAME:
        same = np.array_equal(_bits(h[k][t, :n]), _bits(r[k])) if h[k].dtype == np.float64 else np.array_equal(h[k][t, :n], r[k])
        assert same and (h[k][t, n:] == SENTINEL).all(), (what, k)
    assert np.array_equal(_bits([h["rss"][t], h["tss"][t]]), _bits([r["rss"], r["tss"]])), what
    if r["status"] == T.ZERO_TSS:
        assert h["r2"][t] == SENTINEL, what
    else:
        assert np.array_equal(_bits([h["r2"][t]]), _bits([r["r2"]])), what
    return r


def _random_plateaus(rng, phot, k, refit=True):
    n = len(phot)
    cuts = np.sort(rng.choice(np.arange(1, n), k - 1, replace=False)) if k > 1 else np.zeros(0, np.int64)
    a = [0] + cuts.tolist()
    o = [c - 1 for c in cuts.tolist()] + [n - 1]
    return [(s, e, float(np.mean(phot[s:e + 1])) if refit else float(rng.normal(0, 3000))) for s, e in zip(a, o)]


@pytest.mark.parametrize("prefix", ("s0_", "s1_", "cr_"))
def test_table_equals_golden(prefix):
    """Every trace of the three recorded experiments in one launch: status OK, every per-frame column, rss, tss and r_2."""
    e = T.experiment(prefix)
    lens = e["len"].tolist()
    h = _run([e["photometry"][t, :n] for t, n in enumerate(lens)], e["tf"])
    assert (h["status"] == 0).all()
    for t, n in enumerate(lens):
        c = e["cols"][t]
        assert np.array_equal(_bits(h["plateau_height"][t, :n]), _bits(c["plateau_height"])), t
        assert np.array_equal(h["step_num"][t, :n], c["step_num"]) and np.array_equal(h["step_num"][t, :n] < 0, c["step_none"]), t
        assert np.array_equal(_bits(h["step_size"][t, :n]), _bits(c["step_size"])), t
        assert np.array_equal(h["plateau_length"][t, :n], c["plateau_length"]), t
        assert np.array_equal(h["plateau_index"][t, :n], T.expand(e["tf"][t])[0]), t
        assert np.array_equal(_bits(np.full(n, h["r2"][t])), _bits(c["r2"])), t
    assert np.array_equal(_bits(h["rss"]), _bits(e["rss"])) and np.array_equal(_bits(h["tss"]), _bits(e["tss"]))
    assert np.array_equal(_bits(h["r2"]), _bits(e["r_2"]))


def test_trace_lengths_and_plateau_counts_at_the_limits():
    """Lengths 1 .. 8192 with one plateau, with `len` plateaus, with a first plateau of one frame and with a few plateaus."""
    rng = np.random.default_rng(8192)
    phots, pls = [], []
    for n in (1, 2, 7, 8, 9, 127, 128, 129, 8192):
        p = rng.integers(0, 4, n) * 9000.0 + rng.normal(0.0, 3000.0, n)
        variants = [[(0, n - 1, float(np.mean(p)))], [(f, f, float(p[f]) + 0.25) for f in range(n)]]
        if n >= 2:
            variants.append([(0, 0, float(p[0]))] + [(1, n - 1, float(np.mean(p[1:])))])
        if n >= 7:
            variants.append(_random_plateaus(rng, p, 5))
            variants.append(_random_plateaus(rng, p, 3, refit=False))
        for v in variants:
            phots.append(p)
            pls.append(v)
    h = _run(phots, pls)
    statuses = set()
    for t, (p, v) in enumerate(zip(phots, pls)):
        statuses.add(_check(h, t, p, v, (len(p), len(v)))["status"])
    assert statuses == {T.OK, T.ZERO_TSS}                              # (a one-frame trace has no variance)


@pytest.mark.parametrize("n_traces", (63, 64, 65))
def test_ragged_batches(n_traces):
    rng = np.random.default_rng(n_traces)
    phots = [rng.normal(20000.0, 3000.0, int(rng.integers(2, 41))) for _ in range(n_traces)]
    phots[0], phots[-1] = rng.normal(0.0, 3000.0, 40), rng.normal(0.0, 3000.0, 2)
    pls = [_random_plateaus(rng, p, int(rng.integers(1, min(len(p), 6) + 1))) for p in phots]
    h = _run(phots, pls, max_frames=40)
    for t, (p, v) in enumerate(zip(phots, pls)):
        assert _check(h, t, p, v, t)["status"] == T.OK


def test_no_trace_launches_nothing():
    import torch
    from fluorosequencingimageanalysis_amd import timetrace as TT
    z = lambda dt: torch.zeros((0, 40), dtype=dt, device="cuda")
    c = torch.zeros(0, dtype=torch.int32, device="cuda")
    out = TT.table_device(z(torch.float64), c, z(torch.int32), z(torch.int32), z(torch.float64), c)
    assert out["r2"].shape == (0,) and out["plateau_height"].shape == (0, 40)
    assert TT.timetrace_table([], [])["lengths"].shape == (0,)


def test_residuals_go_through_pow():
    """24 576 residual terms drawn from N(0, 3000^2) in traces of six frames: pow(x, 2.0) and x * x differ in the last bit for
    about one value in a thousand, and a sum of a few terms of one size keeps that bit."""
    rng = np.random.default_rng(3000)
    phots = [rng.normal(0.0, 3000.0, 6) for _ in range(4096)]
    pls = [_random_plateaus(rng, p, int(rng.integers(1, 3))) for p in phots]
    differ = sum(int(T.table(p, v)["rss"] != T.table(p, v, pow2=T.mul2)["rss"]) for p, v in zip(phots, pls))
    assert differ >= 1                                                 # (on the CPU: the multiply would not pass below)
    h = _run(phots, pls)
    for t, (p, v) in enumerate(zip(phots, pls)):
        assert _check(h, t, p, v, t)["status"] == T.OK


def test_invalid_tables_leave_their_rows_untouched():
    rng = np.random.default_rng(5)
    p = rng.normal(10000.0, 3000.0, 12)
    good = [(0, 4, 1.5), (5, 11, 2.5)]
    bad = {"gap": [(0, 4, 1.0), (6, 11, 2.0)], "start_1": [(1, 4, 1.0), (5, 11, 2.0)], "short": [(0, 4, 1.0), (5, 10, 2.0)],
           "overlap": [(0, 5, 1.0), (5, 11, 2.0)], "count_0": [], "reversed": [(0, 4, 1.0), (7, 6, 2.0), (7, 11, 1.0)]}
    phots, pls = [p], [good]
    for v in bad.values():
        phots += [p, p]
        pls += [v, good]
    h = _run(phots, pls, max_frames=16)
    for t, (q, v) in enumerate(zip(phots, pls)):
        assert _check(h, t, q, v, t)["status"] == (T.OK if v is good else T.INVALID), t
    # counts and lengths a Python list cannot state
    h = _run([p] * 5, [good] * 5, max_frames=16, lens=[12, 0, 17, 12, 12], counts=[2, 2, 2, 17, -1])
    assert h["status"].tolist() == [0, 2, 2, 2, 2]
    assert all((h[k][1:] == SENTINEL).all() for k in PER_FRAME + ("rss", "tss", "r2"))
    _check(h, 0, p, good)


def test_constant_trace():
    from fluorosequencingimageanalysis_amd import timetrace as TT
    rng = np.random.default_rng(6)
    p = rng.normal(10000.0, 3000.0, 9)
    flat = np.full(9, 4321.5)
    pls = [(0, 3, 4321.5), (4, 8, 4000.0)]
    h = _run([p, flat, p], [pls] * 3)
    assert h["status"].tolist() == [0, T.ZERO_TSS, 0]
    for t, q in enumerate((p, flat, p)):
        _check(h, t, q, pls, t)
    with pytest.raises(ZeroDivisionError):
        TT.timetrace_table([p, flat], [pls, pls])
    with pytest.raises(ValueError):
        TT.timetrace_table([p], [[(0, 3, 1.0), (5, 8, 2.0)]])
    with pytest.raises(Exception) as mismatch:
        TT.timetrace_table([p], [[(0, 3, 1.0), (4, 7, 2.0)]])
    assert type(mismatch.value) is Exception
    got = TT.timetrace_table([p, list(p[:5]) + [None]], [pls, [(0, 5, 3.0)]])
    assert np.array_equal(_bits([got["r2"][0]]), _bits([T.table(p, pls)["r2"]]))
    assert np.array_equal(_bits([got["rss"][1]]), _bits([T.table(list(p[:5]) + [0.0], [(0, 5, 3.0)])["rss"]]))


def test_plateau_values():
    import torch
    from fluorosequencingimageanalysis_amd import timetrace as TT
    rng = np.random.default_rng(7)
    lists = [[(0, 8191, 2.5)], [(f, f, float(f)) for f in range(8192)], [(0, 0, 1.0), (1, 129, 2.0)], [(0, 62, 1.0), (63, 64, 3.0)],
             [(0, 3, 1.0), (5, 9, 2.0)], [(1, 9, 2.0)], [], [(0, 6, 1.5)], _random_plateaus(rng, np.zeros(300), 40, refit=False)]
    out = TT.plateau_values_device(*(torch.from_numpy(a).cuda() for a in TT.plateau_rows(lists, 8192)), want_index=True)
    height, index, status = (out[k].cpu().numpy() for k in ("height", "index", "status"))
    for t, pls in enumerate(lists):
        if not pls or not T.valid(pls[-1][1] + 1, pls):
            assert status[t] == T.INVALID and not height[t].any() and not index[t].any(), t
            continue
        idx, hh = T.expand(pls)
        assert status[t] == 0 and np.array_equal(index[t, :len(idx)], idx) and np.array_equal(_bits(height[t, :len(idx)]), _bits(hh)), t
        assert not height[t, len(idx):].any()
    only = TT.plateau_values_device(*(torch.from_numpy(a).cuda() for a in TT.plateau_rows(lists[2:4], 130)))
    assert only["index"] is None and np.array_equal(only["height"].cpu().numpy()[1, :65], T.expand(lists[3])[1])


def test_spot_rows_and_photometry_rows():
    import torch
    from fluorosequencingimageanalysis_amd import _native as N
    from fluorosequencingimageanalysis_amd import _native_timetrace as NT
    rng = np.random.default_rng(8)
    n, F = 70, 9
    hw = rng.integers(0, 50, (n, F, 2)).astype(np.int32)
    present = rng.random((n, F)) < 0.7
    present[:, 0] = True
    present[3, :4] = False                                             # the first present position is frame 4
    present[5] = False                                                 # present nowhere
    vals = rng.normal(0.0, 1000.0, n * F)
    d_hw, d_pr, d_val = torch.from_numpy(hw).cuda(), torch.from_numpy(present.astype(np.uint8)).cuda(), torch.from_numpy(vals).cuda()
    d_fhw = torch.full((n * F, 3), SENTINEL, dtype=torch.int32, device="cuda")
    d_rows = torch.full((n, F), float(SENTINEL), dtype=torch.float64, device="cuda")
    d_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert NT.lib().fsq_timetrace_spot_rows(d_hw.data_ptr(), d_pr.data_ptr(), n, F, d_fhw.data_ptr(), s) == N.FSQ_OK
    assert NT.lib().fsq_timetrace_photometry_rows(d_val.data_ptr(), d_pr.data_ptr(), n, F, d_rows.data_ptr(), d_len.data_ptr(), s) == N.FSQ_OK
    exp = np.zeros((n, F, 3), np.int32)
    for t in range(n):
        first = np.flatnonzero(present[t])
        for f in range(F):
            exp[t, f] = (f,) + (tuple(hw[t, f]) if present[t, f] else tuple(hw[t, first[0]]) if len(first) else (0, 0))
    assert np.array_equal(d_fhw.cpu().numpy().reshape(n, F, 3), exp)
    assert np.array_equal(_bits(d_rows.cpu().numpy()), _bits(np.where(present, vals.reshape(n, F), 0.0)))
    assert (d_len.cpu().numpy() == F).all()


@pytest.fixture(scope="module")
def stack():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stepfit_timetrace.npz"))
    return g["frames"], g["init_hw"]


def _object_path(frames, init_hw, mirror, ck, pmin, path):
    from fluorosequencingimageanalysis_amd import flexlibrary as fl
    imgs = [fl.Image(image=f) for f in frames]
    ex = fl.TimetraceExperiment(imgs)
    ex.lc_create_traces(initial_spots=[fl.Spot(imgs[0], int(h), int(w), 5) for h, w in init_hw], search_radius=3)
    ex.stepfit_tracks(photometry_min=pmin, mirror_start=mirror, chung_kennedy=ck)
    rows = ex.save_experiment_as_csv(path, include_step_fits=True, include_intermediates=True)
    with open(path, newline="") as f:
        return ex, rows, f.read()


@pytest.mark.parametrize("k", (0, 1))
def test_records_from_the_frame_stack(k, stack, tmp_path):
    """timetrace_records on the recorded stack: the golden's numbers, the object path's numbers, and one CSV from both paths."""
    from fluorosequencingimageanalysis_amd import timetrace as TT
    frames, init_hw = stack
    mirror, ck, pmin = T.set_params(k)
    e = T.experiment("s%d_" % k)
    rec = TT.timetrace_records(frames, init_hw, photometry_min=pmin, mirror_start=mirror, chung_kennedy=ck)
    n, F = e["photometry"].shape
    assert np.array_equal(rec["hw"], e["hw"]) and np.array_equal(rec["present"], e["present"]) and (rec["lengths"] == F).all()
    assert np.array_equal(_bits(rec["photometry"]), _bits(e["photometry"]))
    assert np.array_equal(_bits(rec["photometries"]), _bits(e["photometries"]))
    assert np.array_equal(_bits(rec["ck_filtered"]), _bits(e["ck_filtered"]))
    assert (rec["status"] == 0).all()
    for pre, name in (("pl", "plateaus"), ("tf", "t_filtered_plateaus")):
        flat = rec[name]
        assert flat["counts"].tolist() == [len(p) for p in e[pre]]
        assert flat["start"].tolist() == [p[0] for pl in e[pre] for p in pl] and flat["stop"].tolist() == [p[1] for pl in e[pre] for p in pl]
        assert np.array_equal(_bits(flat["height"]), _bits([p[2] for pl in e[pre] for p in pl]))
    for t in range(n):
        c = e["cols"][t]
        for key in ("plateau_height", "step_size"):
            assert np.array_equal(_bits(rec[key][t]), _bits(c[key])), (t, key)
        assert np.array_equal(rec["step_num"][t], c["step_num"]) and np.array_equal(rec["plateau_length"][t], c["plateau_length"]), t
        assert np.array_equal(_bits(rec["plateaus_height"][t]), _bits(c["inter_plateaus"])), t
    assert np.array_equal(_bits(rec["r_squared"]), _bits(e["r_2"])) and np.array_equal(_bits(rec["rss"]), _bits(e["rss"]))
    path = str(tmp_path / "records.csv")
    assert TT.write_csv(path, rec) == 1 + n * F
    with open(path, newline="") as f:
        text = f.read()
    ex, rows, obj_text = _object_path(frames, init_hw, mirror, ck, pmin, str(tmp_path / "objects.csv"))
    assert rows == 1 + n * F and obj_text == text
    T.check_csv_text(text, e["csv"])
    for t, tr in enumerate(ex.spot_traces):                            # the object path's own numbers
        assert (tr.h, tr.w) == tuple(e["keys"][t])
        assert [(a, o) for a, o, _ in ex.step_fits[(tr.h, tr.w)].trace] == [(a, o) for a, o, _ in e["tf"][t]]


def test_wide_frames_take_the_u32_entries(stack, tmp_path):
    """The stack as uint32 with every pixel scaled by 4096 (beyond 16 bits): the records path and the object path agree."""
    from fluorosequencingimageanalysis_amd import timetrace as TT
    frames, init_hw = stack
    wide = frames[:12].astype(np.uint32) * 4096
    rec = TT.timetrace_records(wide, init_hw[:6], mirror_start=2)
    assert (rec["status"] == 0).all() and rec["photometry"].max() > 2.0 ** 24
    ex, rows, obj_text = _object_path(wide, init_hw[:6], 2, 0, None, str(tmp_path / "objects.csv"))
    for t, tr in enumerate(ex.spot_traces):
        assert [None if s is None else (s.h, s.w) for s in tr.trace] == \
            [tuple(rec["hw"][t, f]) if rec["present"][t, f] else None for f in range(12)], t
        k = int(rec["tf_n"][t])
        assert [(a, o) for a, o, _ in ex.step_fits[(tr.h, tr.w)].trace] == list(zip(rec["tf_start"][t, :k].tolist(), rec["tf_stop"][t, :k].tolist()))
    path = str(tmp_path / "records.csv")
    assert TT.write_csv(path, rec) == rows == 1 + 6 * 12
    with open(path, newline="") as f:
        assert f.read() == obj_text
    narrow = TT.timetrace_records(frames[:12], init_hw[:6], include_intermediates=False)
    assert "plateaus_height" not in narrow and "plateaus_height" in rec
    if np.array_equal(narrow["hw"], rec["hw"]) and np.array_equal(narrow["present"], rec["present"]):
        assert np.array_equal(_bits(rec["photometry"]), _bits(narrow["photometry"] * 4096.0))      # (sums of pixels scale exactly)


def test_crafted_experiment_through_the_object_path(tmp_path):
    """save_experiment_as_csv on the crafted experiment (None Spots, stop_0 == 0, every frame a plateau): the reference's text."""
    ex, e = crafted_experiment()
    path = str(tmp_path / "crafted.csv")
    rows = ex.save_experiment_as_csv(path, include_step_fits=True, include_intermediates=True)
    assert rows == 1 + int(e["len"].sum())
    with open(path, newline="") as f:
        text = f.read()
    T.check_csv_text(text, e["csv"])
    assert text.split("\r\n")[1].split(",")[4] == "0"                  # the None Spot of frame 0
    # chosen intermediates in sorted order; no step fits
    assert ex.save_experiment_as_csv(path, include_intermediates=["plateaus", "photometries"]) == rows
    with open(path, newline="") as f:
        lines = f.read().split("\r\n")
    assert lines[0] == "Trace #,Hcoord,Wcoord,Frame #,Photometry,photometries,plateaus"
    ref = text.split("\r\n")
    assert all(a.split(",") == [b.split(",")[j] for j in (0, 1, 2, 3, 4, 11, 12)] for a, b in zip(lines[1:-1], ref[1:-1]))
    # the reference's exceptions, raised before the file is opened
    err = T.errors()
    tr = ex.spot_traces[1]
    key = (tr.h, tr.w)
    from fluorosequencingimageanalysis_amd import flexlibrary as fl
    good = ex.step_fits[key]
    missing = str(tmp_path / "missing.csv")
    for name, pls in (("gap", [(0, 2, 1.0), (4, 7, 2.0)]), ("length", [(0, 2, 1.0), (3, 6, 2.0)])):
        ex.step_fits[key] = fl.PlateauTrace(pls, *key)
        with pytest.raises(Exception) as got:
            ex.save_experiment_as_csv(missing, include_step_fits=True, include_intermediates=True)
        assert type(got.value).__name__ == err[name], name
    ex.step_fits[key] = good
    saved = ex.step_fit_intermediates.pop(key)
    with pytest.raises(KeyError):
        ex.save_experiment_as_csv(missing)
    ex.step_fit_intermediates[key] = {k: v for k, v in saved.items() if k != "plateaus"}
    with pytest.raises(Exception, match="All traces must have identical intermediates."):
        ex.save_experiment_as_csv(missing, include_intermediates=True)
    assert not os.path.exists(missing)


def test_command_line(tmp_path):
    """main() in this process on eight 64 x 64 16-bit frames whose first frame has its PSF pickle."""
    from PIL import Image
    from fluorosequencingimageanalysis_amd import basic_timetrace_script as B
    from fluorosequencingimageanalysis_amd import flexlibrary as fl
    from fluorosequencingimageanalysis_amd import pflib
    rng = np.random.default_rng(64)
    centres = [(h, w) for h in (14, 32, 50) for w in (14, 32, 50)]
    yy, xx = np.mgrid[:64, :64]
    frames = rng.normal(120.0, 12.0, (8, 64, 64))
    for i, (h, w) in enumerate(centres):
        g = np.exp(-((yy - h) ** 2 + (xx - w) ** 2) / (2 * 1.4 ** 2))
        for f in range(8):
            frames[f] += 500.0 * (2 if f < 2 + i % 5 else 1) * g
    frames = np.clip(np.round(frames), 0, 65535).astype(np.uint16)
    paths = []
    for f in range(8):
        paths.append(str(tmp_path / ("frame_%d.png" % f)))
        Image.fromarray(frames[f]).save(paths[-1])
    psfs = {(h, w): (float(h), float(w), 120.0, 500.0, 1.4, 1.4, 0.0, frames[0][h - 2:h + 3, w - 2:w + 3].astype(np.int64),
                     np.zeros((5, 5)), 1.0, 0.9, 10.0) for h, w in centres}
    pflib.save_psfs_pkl(psfs, output_path=paths[0] + "_psfs_test.pkl")
    out = tmp_path / "out"
    ex = B.main(["-L", str(tmp_path / "log.txt"), "--output_directory", str(out), "--save_traces_pkl", "--mirror_start", "2"] + paths)
    assert sorted(os.listdir(out)) == ["test.csv", "test.pkl"] + ["test_%d.png" % f for f in range(8)] + ["traces.pkl"]
    assert len(ex.spot_traces) == len(centres) and os.path.getsize(tmp_path / "log.txt") > 0
    # the object path by hand
    imgs = [fl.Image(image=pflib.read_image(p)[1], metadata={"filepath": p}) for p in paths]
    imgs[0].spots = [fl.Spot(imgs[0], h, w, 5, gaussian_fit=psfs[(h, w)]) for h, w in psfs]
    by_hand = fl.TimetraceExperiment(imgs)
    by_hand.lc_create_traces()
    by_hand.stepfit_tracks(mirror_start=2)
    rows = by_hand.save_experiment_as_csv(str(tmp_path / "by_hand.csv"), include_step_fits=True, include_intermediates=True)
    assert rows == 1 + 8 * len(centres)
    assert open(out / "test.csv", "rb").read() == open(tmp_path / "by_hand.csv", "rb").read()
    with open(out / "test.pkl", "rb") as f:
        step_fits, inter = pickle.load(f, encoding="latin1")
    assert set(step_fits) == set(psfs) and set(inter[centres[0]]) == set(T.INTERMEDIATES)
    assert [tuple(p) for p in step_fits[centres[0]].trace] == [tuple(p) for p in by_hand.step_fits[centres[0]].trace]
    with open(out / "traces.pkl", "rb") as f:
        traces = pickle.load(f, encoding="latin1")
    assert [(t.h, t.w) for t in traces] == [(t.h, t.w) for t in by_hand.spot_traces]
    # without sanity images and traces pickle
    out2 = tmp_path / "out2"
    B.main(["-L", str(tmp_path / "log.txt"), "--output_directory", str(out2), "--no_sanity_check_images", "--mirror_start", "2"] + paths)
    assert sorted(os.listdir(out2)) == ["test.csv", "test.pkl"]
    assert open(out2 / "test.csv", "rb").read() == open(out / "test.csv", "rb").read()
    with pytest.raises(NotImplementedError):
        B.main(["-L", str(tmp_path / "log.txt"), "--output_directory", str(out2), "--no_sanity_check_images", "--sextractor"] + paths)
