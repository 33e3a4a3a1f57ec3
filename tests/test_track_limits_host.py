"""CPU tests (-m "not gpu") of the oracle's spot photometry and of its two trackers at their limits, against what the reference
itself gave on the inputs of tests/_track_limit_cases.py (oracle/gen_golden.py --only phot_limits | track_limits |
centroid_limits -> tests/golden/photometry_limits.npz, tracking_limits.npz, centroid_limits.npz).  Everything is compared
exactly: NaN matches NaN only, finite numbers by their bit pattern.

The photometry fixture is where the reference's Spot.image_slice gets a negative stop, which numpy counts from the far end;
an oracle that clamps such a window to nothing instead fails test_oracle_photometry_equals_reference on exactly those spots."""
import os

import numpy as np
import pytest

import _track_limit_cases as LC
import oracle as O
from _util import GOLD


@pytest.fixture(scope="module", autouse=True)
def _build():
    O.build()


def same(got, exp):
    """float64 arrays: NaN where and only where the other has NaN, the same bits everywhere else."""
    got, exp = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(exp, np.float64)
    nan = np.isnan(exp)
    return got.shape == exp.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got[~nan].view(np.uint64), exp[~nan].view(np.uint64))


def load_photometry():
    """-> (image, spots, wide stack, (field, h, w) table, {(brim, radius): (P1 values, P2 values)}), inputs checked against the
    fixture's checksums."""
    g = np.load(os.path.join(GOLD, "photometry_limits.npz"))
    img, spots, wide, table = LC.phot_image(), LC.phot_spots(), LC.phot_wide_stack(), LC.phot_wide_table()
    for key, arr in (("image_sha", img), ("spots_sha", spots), ("wide_sha", wide), ("table_sha", table)):
        assert str(g[key]) == LC.checksum(arr), "the seeded case builder drifted from the fixture: " + key
    assert [tuple(int(x) for x in p) for p in g["pairs"]] == list(LC.PHOT_PAIRS)
    return img, spots, wide, table, {(b, r): (g["p1_b%d_r%d" % (b, r)], g["p2_b%d_r%d" % (b, r)]) for b, r in LC.PHOT_PAIRS}


def load_tracking():
    """-> ({name: (field, traces, n_discarded)}, {name: (field, n_traces, n_discarded, digest)} for the two large G2 fields,
    [[(field, traces, n_discarded)]] per G5 launch), inputs checked against the fixture's checksums."""
    g = np.load(os.path.join(GOLD, "tracking_limits.npz"))
    fields = {"g1_f%d" % k: f for k, f in enumerate(LC.g1_fields(65))}
    big, small, base = LC.g2_fields()
    fields["g2_small"] = small
    fields.update(LC.g3_cases())
    fields.update(LC.g4_cases())
    assert sorted(fields) == sorted(str(n) for n in g["names"])
    named = {}
    for name, f in fields.items():
        assert str(g[name + "_sha"]) == LC.field_checksum(f), "the seeded case builder drifted from the fixture: " + name
        named[name] = (f, g[name + "_traces"], int(g[name + "_discarded"]))
    large = {}
    for name, f in (("g2_32769", big), ("g2_32768", base)):
        assert str(g[name + "_sha"]) == LC.field_checksum(f), "the seeded case builder drifted from the fixture: " + name
        large[name] = (f, int(g[name + "_n_traces"]), int(g[name + "_discarded"]), str(g[name + "_digest"]))
    launches, k, at = [], 0, 0
    for i, fs in enumerate(LC.g5_launches()):
        assert str(g["g5_sha"][i]) == LC.checksum(*[np.frombuffer(LC.field_checksum(f).encode(), np.uint8) for f in fs]), i
        one = []
        for f in fs:
            n = int(g["g5_rows"][k]) * int(g["g5_frames"][k])
            one.append((f, g["g5_traces"][at:at + n].reshape(int(g["g5_rows"][k]), int(g["g5_frames"][k])), int(g["g5_discarded"][k])))
            at += n
            k += 1
        launches.append(one)
    assert at == len(g["g5_traces"]) and k == 300
    return named, large, launches


def load_centroid():
    """-> ({name: (case, hw)}, (C4 case, hw), (C5 case, hw)), inputs checked against the fixture's checksums."""
    g = np.load(os.path.join(GOLD, "centroid_limits.npz"))
    cases = LC.centroid_cases()
    assert sorted(cases) == sorted(str(n) for n in g["names"])
    named = {}
    for name, c in cases.items():
        assert str(g[name + "_sha"]) == LC.centroid_checksum(c), "the seeded case builder drifted from the fixture: " + name
        named[name] = (c, g[name + "_hw"])
    c4, c5 = LC.c4_case(), LC.c5_case()
    assert str(g["c4_sha"]) == LC.checksum(*c4[:4]) and str(g["c5_sha"]) == LC.centroid_checksum(c5)
    return named, (c4, g["c4_hw"]), (c5, g["c5_hw"])


def test_case_builder_reproduces_the_stored_checksums():
    load_photometry()
    load_tracking()
    load_centroid()
    for name in ("photometry_limits.npz", "tracking_limits.npz", "centroid_limits.npz"):
        assert os.path.getsize(os.path.join(GOLD, name)) < 300000, name


def test_oracle_photometry_equals_reference():
    """P1 and P2: 15 600 + 4 460 spots.  Lists the spots that differ, so that a wrong window rule shows which windows it gets wrong."""
    img, spots, wide, table, exp = load_photometry()
    for (brim, radius), (p1, p2) in exp.items():
        got = O.mexican_hat(img, spots, brim, radius)
        bad = [i for i in range(len(spots)) if not same(got[i:i + 1], p1[i:i + 1])]
        assert not bad, ((brim, radius), len(bad), LC.phot_window_classes(spots[bad], radius).tolist()[:20], spots[bad][:20].tolist())
        got2 = np.zeros(len(table))
        for f in range(2):
            m = table[:, 0] == f
            got2[m] = O.mexican_hat(wide[f], table[m][:, 1:], brim, radius)
        assert same(got2, p2), (brim, radius)


def hat_restated(img, h, w, brim, radius):
    """The bound rule in NumPy: start = max(0, c - r), stop = min(n, c + r + 1), a negative stop has n added and is held at 0,
    the window is empty when stop <= start, the crown mask is taken in the coordinates of that window."""
    def axis(c, n):
        start, stop = max(0, c - radius), min(n, c + radius + 1)
        if stop < 0:
            stop = max(0, stop + n)
        return start, max(stop, start)
    (a0, a1), (b0, b1) = axis(h, img.shape[0]), axis(w, img.shape[1])
    win = img[a0:a1, b0:b1].astype(np.int64)
    hh, ww = np.indices(win.shape)
    d = 2 * radius + 1
    crown = (brim <= hh) & (hh < d - brim) & (brim <= ww) & (ww < d - brim)
    med = float(np.median(win[~crown])) if (~crown).any() else float("nan")
    return float(int(win[crown].sum())) - float(int(crown.sum())) * med


def test_restated_bound_rule_equals_reference():
    img, spots, wide, table, exp = load_photometry()
    for (brim, radius), (p1, p2) in exp.items():
        assert same([hat_restated(img, int(h), int(w), brim, radius) for h, w in spots], p1), (brim, radius)
        assert same([hat_restated(wide[f], int(h), int(w), brim, radius) for f, h, w in table], p2), (brim, radius)


def test_photometry_fixture_covers_the_windows():
    """The shares set for P1: wrapped >= 1/4, empty >= 1/10, no negative stop >= 1/4; both sides of the register form's limit."""
    spots = LC.phot_spots()
    share = LC.phot_shares(np.concatenate([LC.phot_window_classes(spots, r) for b, r in LC.PHOT_PAIRS]))
    assert share["wrapped"] >= 0.25 and share["empty"] >= 0.10 and share["ordinary"] >= 0.25, share
    assert {15, 16} <= {r for b, r in LC.PHOT_PAIRS}
    wrapped15 = spots[LC.phot_window_classes(spots, 15) == "wrapped"]
    sizes = [(LC.phot_axis(int(h), 15, 40), LC.phot_axis(int(w), 15, 52)) for h, w in wrapped15]
    assert max((a[1] - a[0]) * (b[1] - b[0]) for a, b in sizes) > 1024          # more pixels than the register form holds


def test_oracle_greedy_tracking_equals_reference():
    named, large, launches = load_tracking()
    for name, (f, traces, nd) in named.items():
        got, got_nd, prev, nxt, kept = O.greedy_tracking(*f)
        assert got_nd == nd and got.shape == traces.shape and np.array_equal(got, traces), name
        assert int((~kept).sum()) == nd, name
    for name, (f, nt, nd, digest) in large.items():
        got, got_nd, prev, nxt, kept = O.greedy_tracking(*f)
        assert (len(got), got_nd, LC.trace_digest(got)) == (nt, nd, digest), name
    for i, one in enumerate(launches):
        for k, (f, traces, nd) in enumerate(one):
            got, got_nd, prev, nxt, kept = O.greedy_tracking(*f)
            assert got_nd == nd and got.shape == traces.shape and np.array_equal(got, traces), (i, k)


def test_tracking_fixture_covers_the_cases():
    named, large, launches = load_tracking()
    for k in range(3):
        t = named["g1_f%d" % k][1]
        assert t.shape[1] == 65 and ((t[:, 63] >= 0) & (t[:, 64] >= 0)).any()
    assert np.array_equal(named["g1_f0"][1], named["g1_f2"][1]) and not np.array_equal(named["g1_f0"][1], named["g1_f1"][1])
    assert sum(len(x) for x in large["g2_32769"][0][0]) == 32769 and sum(len(x) for x in large["g2_32768"][0][0]) == 32768
    assert large["g2_32769"][1] == large["g2_32768"][1] + 1 and large["g2_32769"][3] != large["g2_32768"][3]
    f, t, nd = named["radius0"]
    assert len(t) == sum(len(x) for x in f[0]) - nd and ((t >= 0).sum(axis=1) == 1).all()
    f, t, nd = named["spot_radius_9"]
    assert len(t) == 0 and nd == sum(len(x) for x in f[0])
    flat = [c for one in launches for c in one]
    assert len(flat) == 300 and any(c[0][2][0] == 1 for c in flat) and any(c[0][2][1] == 1 for c in flat)
    assert {c[0][3] for c in flat} == set(range(5)) and {c[0][4] for c in flat} == set(LC.G5_SPOT_RADII)
    assert 3 * sum(c[2] > 0 for c in flat) >= 300
    assert 3 * sum(bool(len(c[1]) and (c[1] >= 0).sum(axis=1).max() >= 2) for c in flat) >= 300


def test_oracle_centroid_tracking_equals_reference():
    named, (c4, c4_hw), (c5, c5_hw) = load_centroid()
    for name, ((frames, init, off, R, cut), hw) in named.items():
        got, present = O.centroid_tracking(frames, init, R, cut, off)
        assert np.array_equal(got, hw) and np.array_equal(present, hw[:, :, 0] >= 0), name
        assert frames.shape[0] == 1 or ((hw[:, :, 0] >= 0).any() and not (hw[:, :, 0] >= 0).all()), name
    frames, init, off, R, cut = LC.c3_with_zero_frame()
    with pytest.raises(ValueError):
        O.centroid_tracking(frames, init, R, cut, off)
    hw = named["flat"][1]
    assert (hw[:, 1:, 0] >= 0).any()                    # S/N = 0/0 is not below the cut-off: the spot is kept where it was found
    frames, init, fld, offs, R, cut = c4
    assert frames.dtype == np.uint32 and int(frames.max()) == 2 ** 31 - 1 and len(init) == 257 and (np.diff(fld) < 0).any()
    for k in range(3):
        got, present = O.centroid_tracking(frames[k], init[fld == k], R, cut, offs[k])
        assert np.array_equal(got, c4_hw[fld == k]), k
    frames, init, off, R, cut = c5
    assert R == 512 and frames.dtype == np.uint32 and int(frames.min()) >= 2 ** 30
    got, present = O.centroid_tracking(frames, init, R, cut, off)
    assert np.array_equal(got, c5_hw) and present.all() and tuple(c5_hw[0, 1]) != (512, 512)
