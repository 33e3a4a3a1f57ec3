"""Seeded Monte-Carlo PSF fit, host side (no GPU needed): the NumPy twin (_host_montecarlo.py) against the reference's
recorded runs under the same draws (tests/golden/montecarlo.npz), the prefix property, independence from batching, the
refusals, --seed on the command line, and the header against the binding.  Nothing is compared with a tolerance."""
import math
import os
import re

import numpy as np
import pytest

from fluorosequencingimageanalysis_amd import _host_montecarlo as T
from fluorosequencingimageanalysis_amd import _host_peptide_sim as PS
from _montecarlo_cases import (FIELD_TAGS, bits, dict_matches_golden, field_image, field_kwargs, golden, golden_roi_case,
                               rows_match_golden, same, twin_rois, upper_clip_case)
from _util import ROOT


def test_fixture_is_not_vacuous():
    g = golden()
    assert len(g["roi"]) >= 40 and g["n_iters"].tolist() == [1, 2, 63, 64, 65, 1000]
    c = golden_roi_case(1000)
    assert set(c["status"].tolist()) == {T.OK, T.NEVER_IMPROVED, T.NO_MAXIMUM}
    names = [str(n) for n in g["roi_names"]]
    ok = c["status"] == T.OK
    # both clips engage, the tie keeps the earliest iteration, the winners are spread over the lanes of a wavefront
    # (the lower clip, N(0, .3) < 0.01, engages in every other draw and shows in the winners; the upper one, N(4, .3) > 4.99, is a
    # 3.3 sigma event: upper_clip_case() finds an iteration that has it and makes it the last one, whose image is returned)
    assert (c["params"][ok, :2] == 0.01).any() and c["params"][ok, :2].max() > 4.5
    assert c["niter"][names.index("all_1e150")] == 0 and c["status"][names.index("all_1e200")] == T.NEVER_IMPROVED
    assert len(set((c["niter"][ok] % 64).tolist())) >= 16 and c["niter"][ok].max() >= 900
    assert c["exc_text"][names.index("constant_normalised")] == T.INDEX_ERROR_TEXT
    assert c["exc_text"][names.index("all_1e200")] == T.UNBOUND_TEXT
    assert c["types"][0] == "float64,float64,float64,float64,float64,float64,float64,ndarray"
    assert (g["roi_ids"] == 0xffffffff).any()
    # the low threshold lets every candidate through the filter, so consolidation and re-keying have work
    assert len(g["f5_low_candidates"]) > 100 and 0 < len(g["f5_low_keys"]) < 20
    assert str(g["flat_exc"][0]) == "IndexError" and int(g["flat_n_candidates"]) > 0 and int(g["tiny_n_candidates"]) == 1
    assert not same(g["f5_low_t7"], g["f5_low_field7_t7"])


def test_draws_vectorised_equal_scalar_and_start_every_iteration_afresh():
    for seed, pixel, field in ((1, 0, 0), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1), (77, 4711, 3)):
        tab = T.normals_np(seed, 5, 200, pixel, field)
        for it in (5, 6, 63, 64, 204):
            assert bits(tab[it - 5]).tolist() == bits(T.normals(seed, it, pixel, field)).tolist()
    # draw j of a triple is Philox block j >> 1, words (0, 1) or (2, 3), at counter (block, iteration, pixel, field)
    w = PS.philox((1, 9, 8, 7), (5, 0))
    assert T.uniform(5, 9, 8, 7, 2) == PS._uniform(w[0], w[1]) and T.uniform(5, 9, 8, 7, 3) == PS._uniform(w[2], w[3])
    # one block is one attempt of the polar method: a rejected one moves on to the next block; H comes from x2, A from x1
    z = T.normals_np(3, 0, 2000, 1, 1)
    rejected = 0
    for it in range(80):
        block = 0
        while True:
            w = PS.philox((block, it, 1, 1), (3, 0))
            x1, x2 = 2.0 * PS._uniform(w[0], w[1]) - 1.0, 2.0 * PS._uniform(w[2], w[3]) - 1.0
            r2 = x1 * x1 + x2 * x2
            block += 1
            if 0.0 < r2 < 1.0:
                break
        rejected += block > 1
        f = math.sqrt(-2.0 * math.log(r2) / r2)
        assert z[it, 0] == f * x2 and z[it, 1] == f * x1
    assert rejected >= 8 and np.isfinite(z).all() and abs(z.mean()) < 0.05 and abs(z.std() - 1.0) < 0.05


@pytest.mark.parametrize("n_iter", [1, 2, 63, 64, 65, 1000])
def test_twin_reproduces_the_reference_on_every_golden_roi(n_iter):
    g = golden()
    t = twin_rois(g["roi"], g["roi_ids"], n_iter, int(g["roi_seed"][0]))
    rows_match_golden(t["rows"], t["fit"], t["rms"], t["status"], golden_roi_case(n_iter))
    assert (t["rows"]["nfev"] == n_iter).all() and (t["rows"]["theta"] == 0.0).all()


def test_fitter_returns_the_reference_tuple_or_its_exception():
    g = golden()
    c = golden_roi_case(65)
    seed = int(g["roi_seed"][0])
    for k in range(len(g["roi"])):
        cand = (int(g["roi_ids"][k, 0]), int(g["roi_ids"][k, 1]))
        if c["exc_type"][k]:
            with pytest.raises({"IndexError": IndexError, "UnboundLocalError": UnboundLocalError}[c["exc_type"][k]]) as e:
                T.fit_2d_gaussian_monte_carlo(g["roi"][k], 65, seed, cand)
            assert str(e.value) == c["exc_text"][k]
        else:
            res = T.fit_2d_gaussian_monte_carlo(g["roi"][k], 65, seed, cand)
            assert ",".join(type(v).__name__ for v in res) == c["types"][k]
            assert same(np.array([float(v) for v in res[:7]]), c["params"][k]) and same(res[7], c["fit"][k].reshape(5, 5))
    for k in (0, len(g["roi"]) - 3):                        # N_iter = 0: the loop never runs
        name, text = [str(x) for x in g["n0_exc_%d" % k]]
        with pytest.raises({"IndexError": IndexError, "UnboundLocalError": UnboundLocalError}[name]) as e:
            T.fit_2d_gaussian_monte_carlo(g["roi"][k], 0, seed)
        assert str(e.value) == text


@pytest.mark.parametrize("tag", FIELD_TAGS)
def test_twin_reproduces_the_reference_candidate_by_candidate(tag):
    """find_peptides(fit_type='monte_carlo'): what the reference's fitter returned for every candidate of the field, and the
    metrics and sub_img of the peaks its dict kept."""
    g = golden()
    img, kw = field_image(tag), field_kwargs(tag)
    cands = g[tag + "_candidates"]
    W = img.shape[1]
    fitted = []
    for (h, w) in cands:
        roi = T.normalise(img[h - 2:h + 3, w - 2:w + 3])
        fitted.append((roi, T.fit_roi(roi.reshape(25), kw["N_iter"], kw["seed"], int(h) * W + int(w), kw.get("first_field", 0), int(h), int(w))))
    got7 = np.array([[r["row"][k] for k in ("p2", "p3", "H", "A", "sigma_h", "sigma_w", "theta")] for _, r in fitted])
    assert same(got7, g[tag + "_cand_t7"]) and same(np.array([r["fit"] for _, r in fitted]).reshape(-1, 5, 5), g[tag + "_cand_fit"])
    by_centre = {(bits(r["row"]["h0"]).item(), bits(r["row"]["w0"]).item()): i for i, (_, r) in enumerate(fitted)}
    assert len(by_centre) == len(fitted)
    for k in range(len(g[tag + "_keys"])):
        i = by_centre[(bits(g[tag + "_t7"][k, 0]).item(), bits(g[tag + "_t7"][k, 1]).item())]
        roi, r = fitted[i]
        assert same(roi, g[tag + "_sub"][k]) and same(r["fit"].reshape(5, 5), g[tag + "_fit"][k])
        assert same([r["row"]["rmse"], r["row"]["r2"], r["row"]["s_n"]], g[tag + "_metrics"][k])


def test_upper_clip_shows_in_the_last_image():
    roi, ids, n_iter, seed = upper_clip_case()
    z = T.normals_np(seed, n_iter - 1, 1, int(ids[0, 0]), int(ids[0, 1]))
    p = T.parameters_np(z, 4, 4)
    assert 4.0 + 0.3 * z[0, 2] > 4.99 and p[0, 2] == 4.99
    g, _ = T.trials_np(p, roi.reshape(25))
    t = twin_rois(roi, ids, n_iter, seed)
    assert same(t["fit"][0], g[0]) and t["status"][0] == T.OK


def test_prefix_property():
    """The result at N_iter = n is the running best over the first n iterations of a longer run with the same seed."""
    g = golden()
    seed = int(g["roi_seed"][0])
    for k in (0, 5, 17, 23, 30):
        pixel, field = int(g["roi_ids"][k, 0]), int(g["roi_ids"][k, 1])
        long = T.fit_roi(g["roi"][k].reshape(25), 300, seed, pixel, field)
        assert long["running"][-1] == long["row"]["niter"]
        for n in (1, 2, 63, 64, 65, 299):
            short = T.fit_roi(g["roi"][k].reshape(25), n, seed, pixel, field)
            assert short["row"]["niter"] == long["running"][n - 1]
        assert (np.diff(long["running"]) >= 0).all()
    # across the twin's own chunk boundary
    a = T.best_of(g["roi"][0].reshape(25), T.CHUNK + 10, seed, 1, 2)
    b = T.best_of(g["roi"][0].reshape(25), T.CHUNK, seed, 1, 2)
    assert b["niter"] == a["running"][T.CHUNK - 1] and a["niter"] >= b["niter"]


def test_a_candidate_does_not_depend_on_its_neighbours_or_on_how_fields_are_numbered():
    g = golden()
    # field 0 of a stack that starts at first_field = 7 is field 7 of a stack that starts at 0: one recorded run, two readings
    img, W = field_image("f5_low_field7"), 96
    h, w = [int(x) for x in g["f5_low_field7_candidates"][10]]
    roi = T.normalise(img[h - 2:h + 3, w - 2:w + 3]).reshape(25)
    a = T.fit_roi(roi, 200, int(g["field_seed"][0]), h * W + w, 7)
    b = T.fit_roi(roi, 200, int(g["field_seed"][0]), h * W + w, 3 + 4)
    c = T.fit_roi(roi, 200, int(g["field_seed"][0]), h * W + w, 0)
    assert a["row"] == b["row"] and a["row"]["niter"] >= 0
    assert same([a["row"]["p2"], a["row"]["H"]], g["f5_low_field7_cand_t7"][10, [0, 2]])
    assert same([c["row"]["p2"], c["row"]["H"]], g["f5_low_cand_t7"][10, [0, 2]]) and a["row"]["H"] != c["row"]["H"]


def test_refusals_need_no_gpu():
    from fluorosequencingimageanalysis_amd import pflib
    img = field_image("f5_default")
    for call in (lambda: pflib.find_peptides(img, fit_type='monte_carlo'),
                 lambda: pflib.find_peptides_batch(img[None], fit_type='monte_carlo', N_iter=5),
                 lambda: pflib.find_peptides_records(img[None], fit_type='monte_carlo'),
                 lambda: pflib._fit_2d_gaussian_monte_carlo(np.ones((5, 5)))):
        with pytest.raises(NotImplementedError, match="seed="):
            call()
    with pytest.raises(NotImplementedError):
        pflib.find_peptides(img, fit_type='other', seed=1)
    for n_iter in (0, -1, 2 ** 31):
        with pytest.raises(ValueError, match="N_iter"):
            pflib.find_peptides(img, fit_type='monte_carlo', N_iter=n_iter, seed=1)
    for seed in (-1, 2 ** 64):
        with pytest.raises(ValueError, match="seed"):
            pflib.find_peptides(img, fit_type='monte_carlo', seed=seed)
    with pytest.raises(ValueError, match="first_field"):
        pflib.find_peptides(img, fit_type='monte_carlo', seed=1, first_field=2 ** 32)
    for bad in (img.astype(np.float16), img.astype(np.uint32) + 70000, img.astype(np.uint32)):
        with pytest.raises(NotImplementedError, match="16-bit"):
            pflib.find_peptides(bad, fit_type='monte_carlo', seed=1)
    # N_iter <= 0 on the fitter itself is the reference's own failure, found without a launch
    with pytest.raises(UnboundLocalError) as e:
        pflib._fit_2d_gaussian_monte_carlo(np.arange(25.0).reshape(5, 5), 0, seed=1)
    assert str(e.value) == T.UNBOUND_TEXT
    with pytest.raises(IndexError) as e:
        pflib._fit_2d_gaussian_monte_carlo(np.full((5, 5), np.nan), 0, seed=1)
    assert str(e.value) == T.INDEX_ERROR_TEXT
    with pytest.raises(AssertionError):
        pflib._fit_2d_gaussian_monte_carlo(np.ones((5, 4)), 10, seed=1)


def test_records_to_dicts_rebuilds_the_float_sub_image_and_the_exceptions():
    """The records fsq_find_peptides_mc writes, made here from the recorded run: row, fit_img, raw pixel words."""
    from fluorosequencingimageanalysis_amd import engine, montecarlo, pflib
    g = golden()
    tag = "f5_low"
    img, W = field_image(tag), 96
    cands, c7 = g[tag + "_candidates"], g[tag + "_cand_t7"]
    n = len(g[tag + "_keys"])
    rec = np.zeros(n, engine.RECORD_DTYPE)
    for k in range(n):
        i = [j for j, (h, w) in enumerate(cands) if c7[j, 0] + h - 2.5 == g[tag + "_t7"][k, 0] and c7[j, 1] + w - 2.5 == g[tag + "_t7"][k, 1]]
        assert len(i) == 1
        h, w = [int(x) for x in cands[i[0]]]
        for j, name in enumerate(("h0", "w0", "H", "A", "sigma_h", "sigma_w", "theta")):
            rec[name][k] = g[tag + "_t7"][k, j]
        rec["rmse"][k], rec["r2"][k], rec["s_n"][k] = g[tag + "_metrics"][k]
        rec["key_h"][k], rec["key_w"][k] = g[tag + "_keys"][k]
        rec["fit"][k], rec["sub"][k] = g[tag + "_fit"][k], img[h - 2:h + 3, w - 2:w + 3]
    raw = rec.view(np.uint8).reshape(n, engine.PEAK_RECORD_BYTES)
    counts = montecarlo.encode_counts([n, 0, 0, -1, 0], [0, 2, 1, 0, 0])
    assert counts.tolist() == [n, -3, -2, -1, 0]
    out = pflib.records_to_dicts(raw, counts, fit_type='monte_carlo')
    dict_matches_golden(out[0], tag)
    assert isinstance(out[1], IndexError) and str(out[1]) == T.INDEX_ERROR_TEXT
    assert isinstance(out[2], UnboundLocalError) and str(out[2]) == T.UNBOUND_TEXT
    assert isinstance(out[3], AssertionError) and out[4] == {}
    # the default stays what it was: integer sub_img
    assert pflib.records_to_dicts(raw, [n])[0][tuple(int(x) for x in g[tag + "_keys"][0])][7].dtype == np.int64


def test_command_line_seed(tmp_path, monkeypatch):
    from fluorosequencingimageanalysis_amd import basic_image_script as cli, pflib
    seen = {}

    def spy(paths, find_peptides_parameters=None, timestamp_epoch=None, num_processes=None):
        seen.update(fp=find_peptides_parameters)
        return {}
    monkeypatch.setattr(pflib, "parallel_image_batch", spy)
    (tmp_path / "p").mkdir()
    log = str(tmp_path / "run.log")
    cli.main(["-mc", "--N_iter", "50", "--seed", "12345678901234567890", "-L", log, str(tmp_path / "p")])
    assert seen["fp"] == {"fit_type": "monte_carlo", "N_iter": 50, "seed": 12345678901234567890}
    cli.main(["-mc", "--seed", "3", "--parameters", "{'seed': 4}", "-L", log, str(tmp_path / "p")])
    assert seen["fp"] == {"fit_type": "monte_carlo", "N_iter": 1000, "seed": 4}
    cli.main(["-mc", "-L", log, str(tmp_path / "p")])        # without --seed the parameters are what they were
    assert seen["fp"] == {"fit_type": "monte_carlo", "N_iter": 1000}
    cli.main(["--seed", "3", "-L", log, str(tmp_path / "p")])  # --seed alone names no fit type
    assert seen["fp"] is None
    pflib._check_find_peptides_parameters({"seed": 1, "first_field": 2, "fit_type": "monte_carlo"})


def test_binding_declares_the_header():
    from fluorosequencingimageanalysis_amd import _native as N
    from fluorosequencingimageanalysis_amd import _native_montecarlo as NM
    text = open(os.path.join(ROOT, "include", "fsq_montecarlo.h")).read()
    decl = re.findall(r"^(int|int64_t) (fsq_\w+)\((.*?)\);", text, re.M | re.S)
    assert [d[1] for d in decl] == list(NM.EXPORTED)
    for ret, name, args in decl:
        assert len(NM._SIGS[name][1]) == len(args.split(",")), name
        assert NM._SIGS[name][0] is {"int": __import__("ctypes").c_int, "int64_t": __import__("ctypes").c_int64}[ret]
    assert not set(NM.EXPORTED) & set(N.EXPORTED)
    for k, v in (("FSQ_MC_OK", NM.MC_OK), ("FSQ_MC_NEVER_IMPROVED", NM.MC_NEVER_IMPROVED), ("FSQ_MC_NO_MAXIMUM", NM.MC_NO_MAXIMUM)):
        assert int(re.search(r"#define %s (\d+)" % k, text).group(1)) == v
    assert (NM.MC_OK, NM.MC_NEVER_IMPROVED, NM.MC_NO_MAXIMUM) == (T.OK, T.NEVER_IMPROVED, T.NO_MAXIMUM) and NM.MAX_N_ITER == T.MAX_N_ITER
    mk = open(os.path.join(ROOT, "fluorosequencingimageanalysis_amd", "csrc", "Makefile")).read()
    assert "fsq_montecarlo.h" in mk and "$(wildcard simulate/*.hip)" in mk
    hip = open(os.path.join(ROOT, "fluorosequencingimageanalysis_amd", "csrc", "simulate", "fsq_peptide_sim.hip")).read()
    assert '#include "fsq_philox.h"' in hip and "PHILOX_M0" not in hip
