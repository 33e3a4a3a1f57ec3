"""Spot photometry (csrc/fsq_photometry.hip) and the two trackers (csrc/fsq_track.hip) on the GPU at their limits: the inputs of
tests/_track_limit_cases.py against what the reference gave on them (tests/golden/photometry_limits.npz, tracking_limits.npz,
centroid_limits.npz, checked against the oracle without a GPU by tests/test_track_limits_host.py) and against the oracle.
Every output tensor starts as the byte pattern 0xA5; nothing is compared with a tolerance, NaN matches NaN only.

  P  mexican-hat photometry: windows whose stop is negative (numpy counts it from the far end), empty and clipped windows on
     both sides of the register form's radius limit, uint32 pixels up to 2^31 - 1 in a shuffled two-field table, tail waves,
     the radius limit and the argument rules of the C ABI
  G  greedy tracking: 63 .. 66 frames (frame tables in LDS up to 64), 32 768 against 32 769 spots (pairing flags in LDS up to
     32 768) next to a 30-spot field, radius 0 and 1, one-pixel-wide fields, half-pixel offsets, fractional spot radii, 300
     tiny fields, failing fields beside good ones, pair_cap overflow in one field, the argument rules
  C  centroid tracking: wrapped search windows, offsets beyond the image, R of 0, 11, 12 and 512, flat and all-zero frames,
     cut-offs of inf, -1 and NaN, 257 spots over three uint32 fields, the argument rules

Run time of this file on an MI355X: 3.3 s for its 46 tests (1.5 s of them the first import of torch); the slowest is
test_g2_pairing_flags_on_both_sides_of_lds with 0.51 s, oracle included: k8_track ranks the 16 384 and 16 385 candidate pairs
of its two large fields (O(pairs^2) comparisons over 256 threads) and accepts them on one thread well inside that time."""
import contextlib
import ctypes

import numpy as np
import pytest

import _track_limit_cases as LC
from test_track_limits_host import load_centroid, load_photometry, load_tracking, same

pytestmark = pytest.mark.gpu

PATTERN32 = int(np.array([0xA5A5A5A5], np.uint32).view(np.int32)[0])


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from fluorosequencingimageanalysis_amd import _native, flexlibrary, photometry
    import oracle as O
    O.build()
    return torch, _native, flexlibrary, photometry, O


@pytest.fixture(scope="module")
def phot():
    return load_photometry()


@pytest.fixture(scope="module")
def track():
    return load_tracking()


@pytest.fixture(scope="module")
def centroid():
    return load_centroid()


@contextlib.contextmanager
def _prefilled():
    """Every output tensor a binding allocates starts as a byte pattern, not as zeros: what a kernel leaves unwritten shows."""
    import torch
    real = torch.empty

    def filled(*a, **k):
        t = real(*a, **k)
        if t.is_cuda:
            t.view(torch.uint8).fill_(0xA5)
        return t
    torch.empty = filled
    try:
        yield
    finally:
        torch.empty = real


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pattern(n, dtype):
    import torch
    t = torch.empty(n, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(0xA5)
    return t


def _untouched(t):
    import torch
    return bool((t.view(torch.uint8) == 0xA5).all())


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ---- P: photometry ----------------------------------------------------------------------------------------------------------
def _hat_abi(N, img, fhw, brim, radius, n=None, pad=8, null=()):
    """fsq_mexican_hat / _u32 on a stack [n_fields, H, W] and (field, h, w) rows -> (rc, out[n], the pad after it is untouched)."""
    import torch
    img = np.asarray(img)
    fn = N.lib().fsq_mexican_hat_u32 if img.dtype == np.uint32 else N.lib().fsq_mexican_hat
    d_img, d_sp = _dev(img), _dev(np.asarray(fhw, np.int32).reshape(-1, 3))
    n = len(fhw) if n is None else n
    d_out = _pattern(max(n, 0) + pad, torch.float64)
    p = lambda name, t: None if name in null else t.data_ptr()          # noqa: E731
    rc = fn(p("img", d_img), img.shape[0], img.shape[1], img.shape[2], p("spots", d_sp), n, brim, radius, p("out", d_out), _stream())
    torch.cuda.synchronize()
    return rc, d_out[:max(n, 0)].cpu().numpy(), _untouched(d_out[max(n, 0):])


def test_p1_windows_beyond_the_borders_equal_reference(env, phot):
    torch, N, fl, ph, O = env
    img, spots, wide, table, exp = phot
    with _prefilled():
        for (brim, radius), (p1, p2) in exp.items():
            got = ph.mexican_hat_photometry_metric(img, spots, brim_size=brim, radius=radius)
            assert same(got, p1), ((brim, radius), int((~np.isnan(p1)).sum()))
            assert same(got, O.mexican_hat(img, spots, brim, radius)), (brim, radius)
    # one object, one answer: Spot.image_slice (numpy) and Spot.mexican_hat_photometry_metric (the kernel) see the same window
    class Img(object):
        image = img
    sp = fl.Spot.__new__(fl.Spot)
    sp.parent_Image, sp.h, sp.w, sp.size, sp.gaussian_fit = Img(), -12, 7, 5, None
    assert sp.image_slice(radius=9).shape == (38, 17)
    assert same([sp.mexican_hat_photometry_metric(brim_size=6, radius=9)], exp[(6, 9)][0][[i for i, s in enumerate(spots) if tuple(s) == (-12, 7)]])


def test_p2_wide_pixels_in_a_shuffled_two_field_table(env, phot):
    torch, N, fl, ph, O = env
    img, spots, wide, table, exp = phot
    assert wide.dtype == np.uint32 and int(wide.max()) == 2 ** 31 - 1 and (np.diff(table[:, 0]) < 0).any()
    with _prefilled():
        for (brim, radius), (p1, p2) in exp.items():
            got = ph.mexican_hat_photometry_metric(wide, table, brim_size=brim, radius=radius)
            assert same(got, p2), (brim, radius)
            rc, got_abi, clean = _hat_abi(N, wide, table, brim, radius)
            assert rc == N.FSQ_OK and clean and same(got_abi, p2), (brim, radius)


def test_p3_tail_waves_leave_no_stray_write(env, phot):
    """Four spots per block: tables of 1, 3, 4 and 5 spots end inside a block; the doubles behind the table stay as they were."""
    torch, N, fl, ph, O = env
    img, spots, wide, table, exp = phot
    rows = np.array([(0, -12, 7), (0, 3, 51), (0, 38, 0), (0, 20, 20), (0, -45, -60)], np.int32)
    for brim, radius in ((6, 9), (6, 16)):
        ref = O.mexican_hat(img, rows[:, 1:], brim, radius)
        for n in (1, 3, 4, 5):
            rc, got, clean = _hat_abi(N, img[None], rows[:n], brim, radius)
            assert rc == N.FSQ_OK and clean and same(got, ref[:n]), (brim, radius, n)


def test_p4_the_largest_radius(env, phot):
    torch, N, fl, ph, O = env
    img, spots, wide, table, exp = phot
    rows = np.array([(0, 20, 20), (0, -3, 60), (0, -16400, 5), (0, 10, -16390), (0, -16425, 3), (0, 16400, 16400)], np.int32)
    rc, got, clean = _hat_abi(N, img[None], rows, 5, 16383)
    ref = O.mexican_hat(img, rows[:, 1:], 5, 16383)
    assert rc == N.FSQ_OK and clean and same(got, ref) and np.isnan(ref).any() and not np.isnan(ref).all()
    rc, got, clean = _hat_abi(N, img[None], rows, 5, 16384)
    assert rc == N.FSQ_EINVAL and clean


def test_p5_argument_rules(env, phot):
    torch, N, fl, ph, O = env
    img = phot[0]
    rows = np.array([(0, 20, 20), (0, 3, 3)], np.int32)
    for kw in (dict(brim=-1, radius=9), dict(brim=6, radius=-1), dict(brim=6, radius=9, n=-1), dict(brim=6, radius=9, null=("img",)),
               dict(brim=6, radius=9, null=("spots",)), dict(brim=6, radius=9, null=("out",))):
        rc, got, clean = _hat_abi(N, img[None], rows, **kw)
        assert rc == N.FSQ_EINVAL and clean, kw
    rc, got, clean = _hat_abi(N, img[None], rows, 6, 9, n=0, null=("img", "spots", "out"))
    assert rc == N.FSQ_OK and clean


# ---- G: greedy tracker ------------------------------------------------------------------------------------------------------
def _equals_oracle(O, field, res, what):
    tr, nd, prev, nxt, kept = res
    o_tr, o_nd, o_prev, o_next, o_kept = O.greedy_tracking(*field)
    assert nd == o_nd and np.array_equal(kept, o_kept), what
    assert np.array_equal(prev, o_prev) and np.array_equal(nxt, o_next), what
    assert tr.shape == o_tr.shape and np.array_equal(tr, o_tr), what
    return o_tr


def _launch(fl, fields):
    with _prefilled():
        return fl.track_fields([f[0] for f in fields], [f[1] for f in fields], fields[0][2], fields[0][3], fields[0][4])


@pytest.mark.parametrize("F", LC.G1_FRAMES)
def test_g1_frame_tables_on_both_sides_of_lds(env, track, F):
    torch, N, fl, ph, O = env
    fields = LC.g1_fields(F)
    res = _launch(fl, fields)
    for k in range(3):
        tr = _equals_oracle(O, fields[k], res[k], (F, k))
        assert tr.shape[1] == F and len(tr) > 12
    for a, b in zip(res[0], res[2]):
        assert np.array_equal(a, b)
    assert not np.array_equal(res[0][0], res[1][0])
    if F == 65:
        for k in range(3):
            f, traces, nd = track[0]["g1_f%d" % k]
            assert res[k][1] == nd and np.array_equal(res[k][0], traces), k
            assert ((traces[:, 63] >= 0) & (traces[:, 64] >= 0)).any()


def test_g2_pairing_flags_on_both_sides_of_lds(env, track):
    """32 769 spots (links), 30 spots, 32 768 spots (LDS bitmaps) in one launch; 16 384 and 16 385 candidate pairs are ranked."""
    torch, N, fl, ph, O = env
    fields = LC.g2_fields()
    assert [sum(len(x) for x in f[0]) for f in fields] == [32769, 30, 32768]
    res = _launch(fl, fields)
    for k, name in ((0, "g2_32769"), (2, "g2_32768")):
        _equals_oracle(O, fields[k], res[k], name)
        f, nt, nd, digest = track[1][name]
        assert (len(res[k][0]), res[k][1], LC.trace_digest(res[k][0])) == (nt, nd, digest), name
    _equals_oracle(O, fields[1], res[1], "g2_small")
    assert np.array_equal(res[1][0], track[0]["g2_small"][1])
    hw = np.concatenate(fields[0][0])                           # the exact tie: the ancestor at (193, 193) takes the smaller bin
    a = int(np.nonzero((hw[:16384] == (193, 193)).all(axis=1))[0][0])
    assert tuple(hw[res[0][3][a]]) == (193, 192)


@pytest.mark.parametrize("name", list(LC.g3_cases()) + list(LC.g4_cases()))
def test_g3_g4_small_radii_shapes_borders_and_rounding(env, track, name):
    torch, N, fl, ph, O = env
    field, traces, nd = track[0][name]
    res = _launch(fl, [field])[0]
    _equals_oracle(O, field, res, name)
    assert res[1] == nd and res[0].shape == traces.shape and np.array_equal(res[0], traces)
    n = sum(len(x) for x in field[0])
    if name == "radius0":
        assert len(res[0]) == n - nd and ((res[0] >= 0).sum(axis=1) == 1).all() and (res[2] == -1).all()
    if name == "spot_radius_9":
        assert len(res[0]) == 0 and nd == n and not res[4].any()
    if name == "one_pixel":
        assert res[0].tolist() == [[0, 1, 2]]


def test_g5_three_hundred_tiny_fields(env, track):
    torch, N, fl, ph, O = env
    n = 0
    for i, one in enumerate(track[2]):
        res = _launch(fl, [c[0] for c in one])
        for k, (field, traces, nd) in enumerate(one):
            _equals_oracle(O, field, res[k], (i, k))
            assert res[k][1] == nd and res[k][0].shape == traces.shape and np.array_equal(res[k][0], traces), (i, k)
            n += 1
    assert n == 300


def _track_abi(N, fields, pair_cap, pad=4, null=(), short=0, **over):
    """fsq_greedy_tracking on patterned outputs -> (rc, dict of host arrays without their pad, pads untouched)."""
    import torch
    hw, start, counts, off = LC.field_tables(fields)
    n_fields, F = counts.shape
    a = dict(n_fields=n_fields, n_frames=F, H=fields[0][2][0], W=fields[0][2][1], radius=fields[0][3], spot_radius=fields[0][4],
             pair_cap=pair_cap)
    total = int(start[-1])
    L = N.lib()
    ws_bytes = L.fsq_track_workspace_bytes(n_fields, F, a["H"], a["W"], max(1, min(pair_cap, 1 << 20)))
    a.update(over)
    t = dict(hw=_dev(hw.reshape(-1)), start=_dev(start), counts=_dev(counts.reshape(-1)), off=_dev(off.reshape(-1)),
             prev=_pattern(total + pad, torch.int32), next=_pattern(total + pad, torch.int32), kept=_pattern(total + pad, torch.uint8),
             traces=_pattern(total * F + pad, torch.int32), nt=_pattern(n_fields + pad, torch.int32),
             nd=_pattern(n_fields + pad, torch.int32), st=_pattern(n_fields + pad, torch.int32), ws=_pattern(max(ws_bytes, 8), torch.uint8))
    p = lambda name: None if name in null else t[name].data_ptr()       # noqa: E731
    rc = L.fsq_greedy_tracking(p("hw"), p("start"), p("counts"), p("off"), a["n_fields"], a["n_frames"], a["H"], a["W"], a["radius"],
                               ctypes.c_double(a["spot_radius"]), p("prev"), p("next"), p("kept"), p("traces"), p("nt"), p("nd"), p("st"),
                               a["pair_cap"], p("ws"), ws_bytes - short, _stream())
    torch.cuda.synchronize()
    sizes = dict(prev=total, next=total, kept=total, traces=total * F, nt=n_fields, nd=n_fields, st=n_fields)
    clean = all(_untouched(t[k][n:]) for k, n in sizes.items())
    host = {k: t[k][:n].cpu().numpy() for k, n in sizes.items()}
    host["traces"], host["start"] = host["traces"].reshape(-1, F), start
    host["all_untouched"] = all(_untouched(t[k]) for k in sizes)
    return rc, host, clean


def _field_of(host, k):
    a, b = int(host["start"][k]), int(host["start"][k + 1])
    nt = int(host["nt"][k])
    return host["traces"][a:a + nt], int(host["nd"][k]), host["prev"][a:b], host["next"][a:b], host["kept"][a:b].astype(bool)


def test_g6_failing_fields_beside_good_ones(env):
    torch, N, fl, ph, O = env
    fields = LC.g6_fields()
    rc, host, clean = _track_abi(N, fields, 4096)
    assert rc == N.FSQ_OK and clean
    assert host["st"].tolist() == [0, N.FSQ_EASSERT, N.FSQ_EINVAL, 0] and host["nt"][1] == 0 and host["nt"][2] == 0
    rc1, alone, clean1 = _track_abi(N, fields[:1], 4096)
    assert rc1 == N.FSQ_OK and clean1 and alone["st"].tolist() == [0]
    for k in (0, 3):
        for x, y in zip(_field_of(host, k), _field_of(alone, 0)):
            assert np.array_equal(x, y), k
        _equals_oracle(O, fields[k], _field_of(host, k), k)


def test_g7_pair_list_overflow_in_one_field_only(env):
    torch, N, fl, ph, O = env
    fields = LC.g7_fields()
    rc, host, clean = _track_abi(N, fields, 1)
    assert rc == N.FSQ_OK and clean
    assert host["st"].tolist() == [N.FSQ_ERANGE, 0] and host["nt"][0] == 0
    _equals_oracle(O, fields[1], _field_of(host, 1), "one pair per frame")
    assert (_field_of(host, 1)[3] >= 0).sum() == 2                         # one link per frame was made through the list of one


def test_g8_argument_rules(env):
    torch, N, fl, ph, O = env
    fields = LC.g6_fields()[:1]
    L = N.lib()
    for kw in (dict(n_fields=0), dict(n_frames=0), dict(H=0), dict(W=0), dict(radius=-1), dict(spot_radius=-1.0),
               dict(spot_radius=float("nan"))):
        rc, host, clean = _track_abi(N, fields, 4096, **kw)
        assert rc == N.FSQ_EINVAL and host["all_untouched"], kw
    for cap in (0, 2000000001):
        rc, host, clean = _track_abi(N, fields, cap)
        assert rc == N.FSQ_EINVAL and host["all_untouched"], cap
    for name in ("start", "counts", "off", "nt", "nd", "st", "ws"):
        rc, host, clean = _track_abi(N, fields, 4096, null=(name,))
        assert rc == N.FSQ_EINVAL and host["all_untouched"], name
    rc, host, clean = _track_abi(N, fields, 4096, short=1)
    assert rc == N.FSQ_ENOMEM and host["all_untouched"]
    rc, host, clean = _track_abi(N, fields, 4096, H=65536, W=32768)           # refused before anything is touched
    assert rc == N.FSQ_ENOTIMPL and host["all_untouched"]
    for args in ((0, 3, 12, 12, 4096), (1, 0, 12, 12, 4096), (1, 3, 0, 12, 4096), (1, 3, 12, 0, 4096), (1, 3, 12, 12, 0)):
        assert L.fsq_track_workspace_bytes(*args) == N.FSQ_EINVAL, args
    assert L.fsq_track_workspace_bytes(3, 65, 12, 12, 4096) - L.fsq_track_workspace_bytes(3, 64, 12, 12, 4096) == 3 * 8 * (130 + 33 + 1 + 33)


# ---- C: centroid tracker ----------------------------------------------------------------------------------------------------
def _centroid(fl, frames, init, fld, R, cut, off):
    with _prefilled():
        return fl.centroid_track_fields(frames, init, fld, R, cut, off)


@pytest.mark.parametrize("name", list(LC.centroid_cases()))
def test_c1_c2_windows_radii_and_cutoffs_equal_reference(env, centroid, name):
    torch, N, fl, ph, O = env
    (frames, init, off, R, cut), hw = centroid[0][name]
    got, present = _centroid(fl, frames, init, None, R, cut, None if off is None else off[None])
    assert np.array_equal(got, hw) and np.array_equal(present, hw[:, :, 0] >= 0)
    o_hw, o_pr = O.centroid_tracking(frames, init, R, cut, off)
    assert np.array_equal(got, o_hw) and np.array_equal(present, o_pr)
    if name == "flat":                                   # S/N = 0/0: kept at its new position, not dropped and not moved back
        assert present[4:, 1:].all() and np.array_equal(got[4, 1], got[4, 0] - off[1])
    if name == "R12":
        assert not present[:, 1:].any()


def test_c3_an_all_zero_frame_raises(env, centroid):
    torch, N, fl, ph, O = env
    frames, init, off, R, cut = LC.c3_with_zero_frame()
    with pytest.raises(ValueError):
        _centroid(fl, frames, init, None, R, cut, off[None])
    (frames, init, off, R, cut), hw = centroid[0]["without_zero_frame"]
    got, present = _centroid(fl, frames, init, None, R, cut, off[None])
    assert np.array_equal(got, hw)


def test_c4_three_wide_fields_with_interleaved_spots(env, centroid):
    torch, N, fl, ph, O = env
    (frames, init, fld, offs, R, cut), hw = centroid[1]
    assert len(init) == 257 and frames.dtype == np.uint32
    got, present = _centroid(fl, frames, init, fld, R, cut, offs)
    assert np.array_equal(got, hw) and np.array_equal(present, hw[:, :, 0] >= 0)
    for k in range(3):
        o_hw, o_pr = O.centroid_tracking(frames[k], init[fld == k], R, cut, offs[k])
        assert np.array_equal(got[fld == k], o_hw), k


def test_c5_the_widest_window_on_wide_pixels(env, centroid):
    """R = 512 on pixels in [2^30, 2^31): the weighted sums of the 1025 x 1025 window reach 2^61."""
    torch, N, fl, ph, O = env
    (frames, init, off, R, cut), hw = centroid[2]
    got, present = _centroid(fl, frames, init, None, R, cut, None)
    assert np.array_equal(got, hw) and present.all()
    with pytest.raises(NotImplementedError):
        fl.centroid_track_fields(frames, init, None, 513, cut, None)


def test_c6_argument_rules(env):
    import torch
    _, N, fl, ph, O = env
    fr = LC.c1_stack()
    d_fr, d_hw, d_sf = _dev(fr), _dev(LC.C1_INIT.reshape(-1)), _dev(np.zeros(len(LC.C1_INIT), np.int32))
    n, F = len(LC.C1_INIT), len(fr)

    def call(null=(), **over):
        a = dict(n_fields=1, F=F, H=fr.shape[1], W=fr.shape[2], n=n, R=3)
        a.update(over)
        out, pres, err = _pattern(n * F * 2, torch.int32), _pattern(n * F, torch.uint8), _pattern(1, torch.int32)
        p = lambda name, t: None if name in null else t.data_ptr()          # noqa: E731
        rc = N.lib().fsq_centroid_tracking(p("frames", d_fr), a["n_fields"], a["F"], a["H"], a["W"], p("hw", d_hw), p("sf", d_sf), a["n"],
                                           a["R"], 3.0, None, p("out", out), p("pres", pres), err.data_ptr(), _stream())
        torch.cuda.synchronize()
        return rc, _untouched(out) and _untouched(pres)
    for kw in (dict(n=-1), dict(R=-1), dict(n_fields=0), dict(F=0), dict(H=0), dict(W=0), dict(null=("frames",)), dict(null=("hw",)),
               dict(null=("sf",)), dict(null=("out",)), dict(null=("pres",))):
        rc, clean = call(**kw)
        assert rc == N.FSQ_EINVAL and clean, kw
    rc, clean = call(n=0, null=("hw", "sf", "out", "pres"))
    assert rc == N.FSQ_OK and clean
    rc, clean = call(n=0)
    assert rc == N.FSQ_OK and clean
    rc, clean = call()
    assert rc == N.FSQ_OK and not clean
