"""The proof behind csrc/fsq_evalguard.h, pinned on the CPU: the header is plain C++, tests/evalguard_check.cpp includes it and
draws 10^7 parameter tuples - (c, s) as doubles in [-1, 1] (not through sin: exact 0, +-1, subnormals, 2^-1000 .. 2^-380, one ulp
either side of the guard's limits, NaN / infinity), centres and sigmas across and far beyond the fit's box - and, for every tuple
the predicate accepts, evaluates every condition the kernels used to check per pixel on all 25 pixels of all six model evaluations
of a Jacobian round (the step round's trial evaluation is the first of them)."""
import os
import subprocess

from _util import ROOT


def test_range_predicate_implies_every_per_pixel_condition(tmp_path):
    exe = str(tmp_path / "evalguard_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "evalguard_check.cpp")])
    out = subprocess.check_output([exe, "10000000"]).decode()
    f = dict(kv.split("=") for kv in out.split())
    assert int(f["tuples"]) >= 10 ** 7 and int(f["accepted"]) > 10 ** 6 and int(f["inbox"]) > 10 ** 6, out
    assert int(f["bad"]) == 0, out                     # accepted => every per-pixel condition holds
    assert int(f["inbox_rejected"]) == 0, out          # no tuple inside the fit's box is sent to the exact path by the predicate
    assert int(f["trig_bad"]) == 0, out                # real sin / cos of the box's angles: 0 or >= 2^-400
    assert int(f["trig_rounds"]) > 10 ** 5 and int(f["trig_rejected"]) == 0, out   # whole rounds on the real sin / cos with box centres / sigmas
