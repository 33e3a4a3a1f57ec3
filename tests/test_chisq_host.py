"""Chi-squared step fitter, merge filters and R^2, host side: the NumPy restatement against the reference's recorded outputs,
argument validation of the Python surface, and the C ABI declarations (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

import _chisq_reference as R
from _chisq_cases import filter_cases, fit_cases, golden
from _util import ROOT, _bits, same_plateaus


def test_fixture_is_not_vacuous():
    g = golden()
    assert int(g["case_tie_within"].sum()) >= 5 and int(g["case_tie_across"].sum()) >= 5
    cases = fit_cases()
    assert sum(1 for c in cases if (c["counter_n"] != np.arange(1, len(c["counter_n"]) + 1) + 1).any()) >= 5
    assert {len(c["lum"]) for c in cases} >= {3, 4, 5, 6, 7, 8, 50, 200, 512, 1023, 1024}
    assert sum(1 for c in cases if (c["S"] == 1e10).any()) >= 5
    # at least 20 recorded residual sums change when the power becomes a multiply
    changed = 0
    for c in cases:
        if c["name"] != "powsens":
            continue
        real = R.pow2
        try:
            R.pow2 = lambda x: np.asarray(x, dtype=np.float64) * np.asarray(x, dtype=np.float64)
            _, recs = R.chi_squared(c["lum"].tolist(), c["mult"], c["num_steps"], c["L"], c["mag"], c["ignore"])
        finally:
            R.pow2 = real
        k = min(len(recs), len(c["best"]))
        changed += int((_bits([r[0] for r in recs[:k]]) != _bits(c["best"][:k])).sum())
        changed += int((_bits([r[1] for r in recs[:k]]) != _bits(c["counter"][:k])).sum())
    assert changed >= 20, changed


def test_restatement_equals_golden_fits():
    for i, c in enumerate(fit_cases()):
        fit, recs = R.chi_squared(c["lum"].tolist(), c["mult"], c["num_steps"], c["L"], c["mag"], c["ignore"])
        same_plateaus(fit, c["fit"], i)
        assert len(recs) == len(c["best"]), i
        assert np.array_equal(_bits([r[0] for r in recs]), _bits(c["best"])), i
        assert np.array_equal(_bits([r[1] for r in recs]), _bits(c["counter"])), i
        assert [r[2] for r in recs] == c["counter_n"].tolist(), i
        assert np.array_equal(_bits([r[3] for r in recs]), _bits(c["S"])), i


def test_restatement_equals_golden_filters():
    for i, c in enumerate(filter_cases()):
        lum = c["lum"].tolist()
        if c["mode"] == 0:
            got = R.filter_upsteps(lum, c["pin"])
        else:
            got = R.filter_small_steps(lum, c["pin"], c["mag"], c["ratio"])
        same_plateaus(got, c["pout"], i)
        assert np.array_equal(_bits([R.r_squared(lum, c["pin"])]), _bits([c["r2"]])), i


def test_restatement_errors():
    with pytest.raises(ValueError, match="num_steps_multiplier has an invalid value of 0"):
        R.chi_squared([1.0] * 5, num_steps_multiplier=0)
    with pytest.raises(ValueError, match="num_steps has an invalid value of 5 vs"):
        R.chi_squared([1.0] * 5, num_steps=5)
    with pytest.raises(IndexError):
        R.chi_squared([1.0])                                  # (recorded: the reference sorts an empty list of fits)
    assert R.chi_squared([1.0, 3.0])[0] == [(0, 1, 2.0)]       # (recorded: two frames give the one plateau)
    with pytest.raises(ValueError, match="is greater than len"):
        R.chi_squared([1.0, 5.0, 2.0], num_steps=2, min_step_length=0)


def test_header_matches_binding_and_library():
    from fluorosequencingimageanalysis_amd import _native, _native_chisq
    hdr = open(os.path.join(ROOT, "include", "fsq_chisq.h")).read()
    declared = set(re.findall(r"\b(fsq_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_native_chisq.EXPORTED)
    assert {"fsq_chisq_step_fit", "fsq_stepfit_merge_filter", "fsq_stepfit_r_squared"} <= declared
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    L = ctypes.CDLL(_native.LIB_PATH)
    for name in declared:
        getattr(L, name)
    P = _native_chisq.FsqChisqParams
    assert (P.num_steps_multiplier.offset, P.min_step_magnitude.offset, ctypes.sizeof(P)) == (16, 24, 32)
    assert int(re.search(r"#define FSQ_CHISQ_MAX_FRAMES (\d+)", hdr).group(1)) == _native_chisq.MAX_FRAMES


def test_workspace_bytes_validates():
    from fluorosequencingimageanalysis_amd import _native_chisq as NC
    L = NC.lib()
    assert L.fsq_chisq_workspace_bytes(1000, 200) > 0
    assert L.fsq_chisq_workspace_bytes(1000, 1024) > 0
    assert L.fsq_chisq_workspace_bytes(1000, 1025) == L.fsq_chisq_workspace_bytes(1000, 1024)     # (rows may be wider than the cap)
    assert L.fsq_chisq_workspace_bytes(1000, 0) < 0
    # the workspace belongs to the resident blocks, not to the traces
    assert L.fsq_chisq_workspace_bytes(10 ** 6, 200) == L.fsq_chisq_workspace_bytes(10 ** 5, 200)
    assert L.fsq_stepfit_merge_filter_workspace_bytes(10, 9000) < 0 and L.fsq_stepfit_merge_filter_workspace_bytes(10, 100) == 0
    assert L.fsq_stepfit_r_squared_workspace_bytes(10, 0) < 0 and L.fsq_stepfit_r_squared_workspace_bytes(10, 100) == 0


def test_argument_validation():
    """The reference's ValueErrors for the same arguments, raised before any device work."""
    from fluorosequencingimageanalysis_amd import stepfitting as S
    for mult in (0, -0.5, 1.5):
        with pytest.raises(ValueError, match="num_steps_multiplier has an invalid value of"):
            S.chi_squared_step_fitter([1.0] * 10, num_steps_multiplier=mult)
    for ns in (0, -1, 10, 11):
        with pytest.raises(ValueError, match="num_steps has an invalid value of"):
            S.chi_squared_step_fitter([1.0] * 10, num_steps=ns)
    with pytest.raises(IndexError):
        S.chi_squared_step_fitter([1.0])
    with pytest.raises(ValueError, match="NaN"):
        S.chi_squared_step_fitter([1.0, float("nan"), 2.0])
    with pytest.raises(ValueError, match="limited to 1024 frames"):
        S.chi_squared_step_fitter([1.0] * 1025, num_steps=3)
    with pytest.raises(ValueError, match="min_step_magnitude < 0 makes no sense"):
        S.filter_small_steps([1.0] * 10, [(0, 4, 1.0), (5, 9, 1.0)], min_magnitude=-1.0)
    with pytest.raises(ValueError, match="min_step_noise_ratio < 0 makes no sense"):
        S.filter_small_steps([1.0] * 10, [(0, 4, 1.0), (5, 9, 1.0)], min_noise_ratio=-0.1)
    for f in (S.filter_upsteps, S.filter_small_steps, S.stepfit_r_squared):
        with pytest.raises(ValueError, match="consecutive"):
            f([1.0] * 10, [(0, 3, 1.0), (5, 9, 2.0)])
    # fewer than two plateaus come back as given, as in the reference
    assert S.filter_upsteps([1.0, 2.0], [(0, 1, 1.5)]) == [(0, 1, 1.5)]
    assert S.filter_small_steps([1.0, 2.0], [(0, 1, 1.5)], min_magnitude=3.0) == [(0, 1, 1.5)]
    # sliding_t_fitter keeps refusing the arguments this feature leaves alone
    with pytest.raises(NotImplementedError):
        S.sliding_t_fitter([1.0] * 20, downsteps_only=True)


def test_split_scan_kernel_needs_no_scratch(tmp_path):
    """The compiler's resource report for gfx950: the split-scan kernel spills no VGPR and uses no scratch memory."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "fluorosequencingimageanalysis_amd", "csrc", "stepfit", "fsq_chisq.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "k.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, check=True)
    rep = r.stdout[r.stdout.index("kcs_split_scan"):]
    rep = rep[:rep.index("LDS Size")]
    assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", rep).group(1)) == 0, rep
    assert int(re.search(r"VGPRs Spill: (\d+)", rep).group(1)) == 0, rep
    assert int(re.search(r" VGPRs: (\d+)", rep).group(1)) <= 168, rep     # three waves per SIMD
