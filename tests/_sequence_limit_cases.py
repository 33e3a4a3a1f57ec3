"""Inputs of test_gpu_sequence_limits.py that test_limits_host.py checks on the host: the hat fixture
(tests/golden/sequence_limits.npz, recorded from the reference) with its frames rebuilt from their seeds, and keys crafted
to collide in the counting table (hash_key of csrc/sequence/fsq_sequence.hip restated)."""
import os
import zlib

import numpy as np

import _sequence_cases as C

M64 = (1 << 64) - 1


def hash_key(pattern, seq):
    """hash_key of fsq_sequence.hip: the low 32 bits of a 64-bit mix of the pattern and the sequence."""
    x = (int(pattern) ^ ((int(seq) & 0xffffffff) * 0x9E3779B97F4A7C15)) & M64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x & 0xffffffff


def hash_key_np(pattern, seq):
    with np.errstate(over="ignore"):
        x = pattern.astype(np.uint64) ^ (np.uint64(int(seq) & 0xffffffff) * np.uint64(0x9E3779B97F4A7C15))
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
    return (x & np.uint64(0xffffffff)).astype(np.uint64)


def table_capacity(n):
    cap = 64
    while cap < 2 * n + 1:
        cap <<= 1
    return cap


def keys_in_slot(slot, cap, count, seed=1, n_seq=3):
    """`count` distinct (pattern, seq) whose home slot in a table of `cap` slots is `slot`; patterns with bit 63 among them."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        pat = rng.integers(0, 1 << 63, 1 << 18, dtype=np.uint64) | (rng.integers(0, 2, 1 << 18, dtype=np.uint64) << np.uint64(63))
        for s in range(n_seq):
            hit = pat[(hash_key_np(pat, s) & np.uint64(cap - 1)) == np.uint64(slot)]
            out += [(int(p), s) for p in hit.tolist()]
    return out[:count]


def load_fixture():
    return np.load(os.path.join(C.ROOT, "tests", "golden", "sequence_limits.npz"))


def hat_cases(g):
    """One dict per (pixel type, radius, field, brim): the frame, the positions and the reference's values."""
    G = C.recorder_module()
    assert tuple(g["radii"].tolist()) == G.HAT_RADII and tuple(map(tuple, g["positions"].tolist())) == G.HAT_POSITIONS
    out = []
    for wide in (0, 1):
        for ri, radius in enumerate(G.HAT_RADII):
            for fi, field in enumerate(G.HAT_FIELDS):
                fr = G.hat_frame(field, bool(wide), radius)
                assert zlib.crc32(fr.tobytes()) == int(g["frame_crc"][wide, ri, fi]), "the seeded frames drifted from the fixture"
                for bi, brim in enumerate(G.hat_brims(radius)):
                    out.append(dict(name="%s r%d %s brim %d" % (("u16", "u32")[wide], radius, field, brim), wide=bool(wide),
                                    radius=radius, brim=brim, field=field, frame=fr, hw=np.array(G.HAT_POSITIONS, np.int32),
                                    phot=g["phot"][wide, ri, fi, bi]))
    return out
