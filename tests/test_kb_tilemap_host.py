"""The step round's tile map (csrc/fsq_kb_tilemap.h) on the CPU: the header is plain C++, tests/kb_tilemap_check.cpp includes it
and walks every combination of the six list counts drawn from {0, 1, 63, 64, 65, 130} - the blocks 0 .. sum(ceil(n / 64)) + 5 must
cover every position of every list exactly once, in the launch order C3, B10, C1, B3, B1, B0, and blocks past the end must map to
"return".  The program is a plain host program built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

from _util import ROOT


def test_blocks_cover_every_list_position_exactly_once(tmp_path):
    exe = str(tmp_path / "kb_tilemap_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "kb_tilemap_check.cpp")])
    out = subprocess.check_output([exe]).decode()
    f = dict(kv.split("=") for kv in out.split())
    assert int(f["combos"]) == 6 ** 6, out
    assert int(f["blocks"]) > 6 ** 6 * 6 and int(f["positions"]) > 0, out
    assert int(f["bad"]) == 0, out
