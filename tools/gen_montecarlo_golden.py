"""Writes tests/golden/montecarlo.npz: the reference's Monte-Carlo PSF fitter (pflib._fit_2d_gaussian_monte_carlo and
find_peptides(fit_type='monte_carlo')) run, unchanged, under the explicit Philox draws of _host_montecarlo.py.  Data only:
ROIs, images, seeds and recorded results.

The reference is loaded at run time through oracle/refload.py.  Its module-level `scipy` is replaced by a stand-in whose
random.normal(loc, scale) is loc + scale * z on the polar normals of the current (iteration, pixel, field) and whose
random.exponential() ends the iteration (the reference multiplies its value by zero).  Before that the generator asserts, on
numpy itself, that this is what numpy computes: RandomState(seed).normal(loc, scale) has the bits of
loc + scale * RandomState(seed).standard_normal(), and the twin's polar method on RandomState(seed).random_sample() has the
bits of RandomState(seed).standard_normal().

Run with NPY_DISABLE_CPU_FEATURES="AVX512F AVX512CD AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR" so that
numpy.exp is glibc's.  It also times the reference with numpy's own generator (one core) and prints the time per candidate.

  python tools/gen_montecarlo_golden.py [--reference DIR]
"""
import argparse
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ITERS = (1, 2, 63, 64, 65, 1000)
ROI_SEED = 0x5eed0fc0ffee
FIELD_SEED = 20261019
FIELD_N_ITER = 200
LOW_THRESHOLD = -100.0


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def numpy_identities(T, PS):
    rng = np.random.default_rng(12)
    for _ in range(10000):
        loc, scale, seed = float(rng.uniform(-1, 5)), float(rng.uniform(0.05, 0.4)), int(rng.integers(0, 2 ** 32))
        a = np.random.RandomState(seed).normal(loc, scale)
        z = np.random.RandomState(seed).standard_normal()
        assert bits(a) == bits(loc + scale * z), (loc, scale, seed)
    for loc in (0, 1, 2, 3, 4):                             # (h0mean / w0mean reach normal() as numpy integers)
        for seed in range(50):
            a = np.random.RandomState(seed).normal(np.int64(loc), 0.3)
            assert bits(a) == bits(float(loc) + 0.3 * np.random.RandomState(seed).standard_normal())
    for seed in range(300):
        rs = np.random.RandomState(seed)
        g = PS.Normals(lambda: float(rs.random_sample()))
        mine = [g() for _ in range(6)]
        theirs = np.random.RandomState(seed).standard_normal(6)
        assert [bits(x) for x in mine] == [bits(x) for x in theirs], seed
    # the vectorised draws of the twin against its scalar ones
    for seed, pixel, field in ((1, 0, 0), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1), (77, 4711, 3)):
        tab = T.normals_np(seed, 0, 300, pixel, field)
        for it in range(300):
            assert [bits(x) for x in tab[it]] == [bits(x) for x in T.normals(seed, it, pixel, field)], (seed, it)


class Draws(object):
    """What stands in for scipy.random in the reference's module."""

    def __init__(self, T):
        self.T, self.seed, self.pixel, self.field = T, 0, 0, 0
        self.table, self.iteration, self.k, self.log = None, 0, 0, []

    def begin(self, seed, pixel, field, n_iter):
        self.seed, self.pixel, self.field = seed, pixel, field
        self.table = self.T.normals_np(seed, 0, max(1, n_iter), pixel, field).tolist()
        self.iteration, self.k, self.log = 0, 0, []

    def normal(self, loc, scale):
        z = self.table[self.iteration][self.k]
        self.k += 1
        v = float(loc) + float(scale) * z
        if self.k == 1:
            self.log.append([])
        self.log[-1].append(v)
        return v

    def exponential(self):
        assert self.k == 6
        self.iteration += 1
        self.k = 0
        return 1.0


class Scipy(object):
    def __init__(self, real, draws):
        self._real, self.random = real, draws

    def __getattr__(self, k):
        return getattr(self._real, k)


def rois_from(image, rng):
    """The ROI set of the issue: cuts of the field (normalised as the caller does and raw), the clip and tie cases, negative
    values, and the three failing / degenerate ROIs."""
    out, names = [], []
    H, W = image.shape
    for i in range(14):
        h, w = int(rng.integers(2, H - 2)), int(rng.integers(2, W - 2))
        sub = image[h - 2:h + 3, w - 2:w + 3].astype(np.int64)
        sub = sub - np.min(sub)
        out.append(sub / float(np.max(sub)))
        names.append("cut_norm_%d_%d" % (h, w))
    for i in range(8):
        h, w = int(rng.integers(2, H - 2)), int(rng.integers(2, W - 2))
        out.append(image[h - 2:h + 3, w - 2:w + 3].astype(np.float64))
        names.append("cut_raw_%d_%d" % (h, w))
    for corner in ((0, 0), (4, 4), (0, 4), (4, 0)):
        a = rng.uniform(0.0, 0.6, (5, 5))
        a[corner] = 1.0
        out.append(a)
        names.append("max_at_%d_%d" % corner)
    for k in range(3):
        a = rng.uniform(0.0, 0.5, (5, 5))
        a[3, 1] = a[1, 2 + k % 2] = 1.0                     # two equal maxima: the first in raster order is the centre
        out.append(a)
        names.append("two_maxima_%d" % k)
    for k in range(4):
        a = rng.normal(0.2, 0.4, (5, 5))
        a[2, 2] = 1.5 + k
        out.append(a)
        names.append("negative_values_%d" % k)
    out.append(-rng.uniform(0.5, 1.0, (5, 5)))              # every value negative: the start value is below every residual
    names.append("all_negative")
    for k in range(3):
        y, x = np.mgrid[0:5, 0:5]
        a = 0.05 + np.exp(-((y - 2.2 - 0.2 * k) ** 2 + (x - 1.9) ** 2) / (2 * 1.1 ** 2)) + rng.normal(0, 0.01, (5, 5))
        out.append(a / a.max())
        names.append("gaussian_%d" % k)
    out.append(np.full((5, 5), np.nan))
    names.append("constant_normalised")                     # what the caller makes of a constant ROI: 0 / 0.0
    out.append(np.full((5, 5), 1e150))
    names.append("all_1e150")
    out.append(np.full((5, 5), 1e200))
    names.append("all_1e200")
    return np.array(out), names


def winner_of(log, res, clip):
    """The first iteration whose draws are the returned parameters."""
    h0, w0, H, A, sh, sw = [float(x) for x in res[:6]]
    for it, v in enumerate(log):
        if (bits(abs(v[0])) == bits(H) and bits(abs(v[1])) == bits(A) and bits(clip(v[2])) == bits(h0) and bits(clip(v[3])) == bits(w0)
                and bits(abs(v[4])) == bits(sh) and bits(abs(v[5])) == bits(sw)):
            return it
    raise AssertionError("the returned parameters were drawn in no iteration")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("FSQ_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "montecarlo.npz"))
    a = ap.parse_args()
    os.environ["FSQ_REFERENCE"] = a.reference
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, ROOT)
    import refload
    refload.REF = a.reference
    from fluorosequencingimageanalysis_amd import _host_montecarlo as T
    from fluorosequencingimageanalysis_amd import _host_peptide_sim as PS
    numpy_identities(T, PS)
    print("numpy: normal = loc + scale * z and the polar normals hold bit for bit")
    pf = refload.load_reference().pf
    import scipy as real_scipy
    if not hasattr(real_scipy, "random"):
        real_scipy.random = np.random                       # (scipy.random was numpy.random: what the reference calls)
    field = np.load(os.path.join(ROOT, "tests", "golden", "field_f5_small_96.npz"))["image"]

    # ---- the reference's own rate, with numpy's generator --------------------------------------------------------------
    sub = field[40:45, 40:45].astype(np.int64)
    sub = (sub - sub.min()) / float((sub - sub.min()).max())
    t0 = time.time()
    for _ in range(20):
        pf._fit_2d_gaussian_monte_carlo(sub, 1000)
    per = (time.time() - t0) / 20
    print("reference, numpy's generator, one core, N_iter = 1000: %.1f ms per candidate" % (per * 1e3))

    draws = Draws(T)
    pf.scipy = Scipy(real_scipy, draws)
    out = {"reference_ms_per_candidate": np.array(per * 1e3)}
    clip = lambda v: float(np.clip(v, 0.01, 4.99))          # noqa: E731

    # ---- ROIs through _fit_2d_gaussian_monte_carlo -------------------------------------------------------------------
    rng = np.random.default_rng(7)
    rois, names = rois_from(field, rng)
    K = len(rois)
    ids = np.stack([rng.integers(0, 2 ** 32, K, dtype=np.uint64), rng.integers(0, 2 ** 32, K, dtype=np.uint64)], axis=1).astype(np.uint32)
    ids[0], ids[1], ids[2] = (0, 0), (0xffffffff, 0xffffffff), (0xffffffff, 0)
    out.update(roi=rois, roi_names=np.array(names), roi_ids=ids, roi_seed=np.array([ROI_SEED], np.uint64),
               n_iters=np.array(N_ITERS, np.int64))
    y = np.array([np.arange(5) for _ in range(5)])
    x = y.T
    for n_iter in N_ITERS:
        params, fit, rms, win = np.zeros((K, 7)), np.zeros((K, 5, 5)), np.zeros(K), np.full(K, -1, np.int64)
        exc_type, exc_text, types = [], [], []
        for k in range(K):
            draws.begin(ROI_SEED, int(ids[k, 0]), int(ids[k, 1]), n_iter)
            try:
                res = pf._fit_2d_gaussian_monte_carlo(rois[k].copy(), n_iter)
            except Exception as e:                          # noqa: BLE001 - recorded
                exc_type.append(type(e).__name__)
                exc_text.append(str(e))
                types.append("")
                continue
            exc_type.append("")
            exc_text.append("")
            types.append(",".join(type(v).__name__ for v in res))
            params[k] = [float(v) for v in res[:7]]
            fit[k] = res[7]
            win[k] = winner_of(draws.log, res, clip)
            g = pf._2d_gaussian_function(res[2], res[3], res[0], res[1], res[4], res[5], res[6], x, y)
            g = g / np.max(g)
            rms[k] = np.sqrt(np.sum((rois[k] - g) ** 2))
        pre = "n%d_" % n_iter
        out.update({pre + "params": params, pre + "fit": fit, pre + "rms": rms, pre + "niter": win,
                    pre + "exc_type": np.array(exc_type), pre + "exc_text": np.array(exc_text), pre + "types": np.array(types)})
        print("N_iter %4d: %d ROIs, %d raise (%s)" % (n_iter, K, sum(1 for t in exc_type if t), ", ".join(sorted(set(t for t in exc_type if t)))))
    # N_iter = 0: the loop never runs
    for k in (0, K - 3):
        draws.begin(ROI_SEED, 0, 0, 1)
        try:
            pf._fit_2d_gaussian_monte_carlo(rois[k].copy(), 0)
            raise SystemExit("N_iter = 0 returned")
        except (UnboundLocalError, IndexError) as e:
            out["n0_exc_%d" % k] = np.array([type(e).__name__, str(e)])

    # ---- find_peptides ---------------------------------------------------------------------------------------------
    def run_field(image, tag, first_field=0, **kw):
        cands = [(int(h), int(w)) for h, w in pf._psf_candidates(image)]
        state = {"i": 0}
        fitted = []                                          # what the fitter returned, candidate by candidate
        inner = pf._fit_2d_gaussian_monte_carlo
        out[tag + "_candidates"] = np.array(cands, np.int64).reshape(-1, 2)

        def fit(sub_img, n_iter):
            h, w = cands[state["i"]]
            state["i"] += 1
            draws.begin(FIELD_SEED, h * image.shape[1] + w, first_field, n_iter)
            res = inner(sub_img, n_iter)
            fitted.append(([float(v) for v in res[:7]], np.array(res[7], np.float64)))
            return res
        pf._fit_2d_gaussian_monte_carlo = fit
        try:
            try:
                d = pf.find_peptides(image, fit_type='monte_carlo', N_iter=FIELD_N_ITER, **kw)
            except Exception as e:                          # noqa: BLE001 - recorded
                out[tag + "_exc"] = np.array([type(e).__name__, str(e)])
                out[tag + "_n_candidates"] = np.array(len(cands))
                print("%s: %d candidates, raises %s" % (tag, len(cands), type(e).__name__))
                return
        finally:
            pf._fit_2d_gaussian_monte_carlo = inner
        keys = list(d.keys())
        vals = [d[k] for k in keys]
        n = len(keys)
        out[tag + "_exc"] = np.array(["", ""])
        out[tag + "_cand_t7"] = np.array([f[0] for f in fitted]).reshape(-1, 7)
        out[tag + "_cand_fit"] = np.array([f[1] for f in fitted]).reshape(-1, 5, 5)
        out[tag + "_n_candidates"] = np.array(len(cands))
        out[tag + "_keys"] = np.array(keys, np.int64).reshape(n, 2)
        out[tag + "_t7"] = np.array([[float(v[i]) for i in range(7)] for v in vals]).reshape(n, 7)
        out[tag + "_sub"] = np.array([v[7] for v in vals], np.float64).reshape(n, 5, 5)
        out[tag + "_fit"] = np.array([v[8] for v in vals], np.float64).reshape(n, 5, 5)
        out[tag + "_metrics"] = np.array([[float(v[9]), float(v[10]), float(v[11])] for v in vals]).reshape(n, 3)
        out[tag + "_types"] = np.array([",".join(type(x).__name__ for x in v) for v in vals[:1]])
        out[tag + "_key_types"] = np.array([",".join(type(x).__name__ for x in k) for k in keys[:1]])
        print("%s: %d candidates, %d peaks" % (tag, len(cands), n))

    out.update(field_seed=np.array([FIELD_SEED], np.uint64), field_n_iter=np.array(FIELD_N_ITER), low_threshold=np.array(LOW_THRESHOLD))
    run_field(field, "f5_default")
    run_field(field, "f5_low", r_2_threshold=LOW_THRESHOLD)
    run_field(field, "f5_low_field7", first_field=7, r_2_threshold=LOW_THRESHOLD)
    flat = np.full((16, 16), 100, np.uint16)
    out["flat_image"] = flat
    run_field(flat, "flat")
    tiny = np.load(os.path.join(ROOT, "tests", "golden", "tiny_t0_5x5.npz"))["image"]
    out["tiny_image"] = tiny
    run_field(tiny, "tiny", r_2_threshold=LOW_THRESHOLD)
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
