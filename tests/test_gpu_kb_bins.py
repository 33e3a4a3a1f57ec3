"""GPU tests (-m gpu) of the step round's four history lists (csrc/fsq_kb_tilemap.h, kB_step / kA_jacobian of
csrc/fsq_fit_rounds.hip): which fits share a tile and how far a tile runs lmpar change nothing a fit computes, so every case
asks for BIT equality with the oracle (stand-alone ROIs) or with the stand-alone engine run (fit queues; that run is pinned to
the oracle by test_gpu_fit.py / test_gpu_pipeline.py).  FSQ_TWO_PASS_MIN=0 makes the rounds staged at these sizes (tiles stop at
their list's limit and park unfinished fits), FSQ_SYNC_EVERY=1 makes the host look at the counters after every round and
FSQ_DEBUG_TRACE prints them, which is how the tests know that the lists they mean to exercise were in use."""
import re

import numpy as np
import pytest

from _util import rois_of
from test_gpu_ka_compact import MODE_REF, MODE_TEXTBOOK, assert_equals_oracle, gpu_fit

pytestmark = pytest.mark.gpu

LISTS = ("B0", "B1", "B3", "B10", "C1", "C3")
TRACE = re.compile(r"round (\d+): left .* stepped B=(\d+)\+(\d+)\+(\d+)\+(\d+) C=(\d+)\+(\d+)")


@pytest.fixture(scope="module")
def env():
    import torch
    from fluorosequencingimageanalysis_amd import _native
    import oracle as O
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    O.build()
    return torch, _native, O


@pytest.fixture(scope="module")
def rois(env):
    """1 500 ROIs: the first 500 candidates of three synthetic 256 x 256 fields of 120 spots."""
    torch, N, O = env
    from fluorosequencingimageanalysis_amd import synth
    out = []
    for seed in (40, 41, 42):
        img = synth.make_field(seed, (256, 256), 120)
        cand = O.candidates(img)
        assert len(cand) >= 500
        out.append(rois_of(img, cand[:500]))
    r = np.concatenate(out)
    r.setflags(write=False)
    return r


@pytest.fixture(scope="module")
def refs(env, rois):
    """The oracle's fits in both solver modes, computed once."""
    torch, N, O = env
    out = {}
    for mode in (MODE_REF, MODE_TEXTBOOK):
        out[mode] = O.fit_rois(rois, mode=mode, n_threads=16)
        out[mode].setflags(write=False)
    return out


def staged(monkeypatch, **more):
    monkeypatch.setenv("FSQ_TWO_PASS_MIN", "0")
    monkeypatch.setenv("FSQ_SYNC_EVERY", "1")
    monkeypatch.setenv("FSQ_DEBUG_TRACE", "1")
    for k, v in more.items():
        monkeypatch.setenv(k, str(v))


def list_counts(capfd):
    """[(B0, B1, B3, B10, C1, C3) per traced round]: the lists as that round's step round consumed them (the trace's "stepped"
    part: queue B after the Jacobian round's appends, queue C as the round before left it)."""
    err = capfd.readouterr().err
    rounds = [tuple(int(x) for x in m.groups()[1:]) for m in TRACE.finditer(err)]
    assert rounds, "no trace lines: %r" % err[:300]
    return rounds


def used(rounds):
    return {name: max(r[k] for r in rounds) for k, name in enumerate(LISTS)}


@pytest.mark.parametrize("mode", [MODE_REF, MODE_TEXTBOOK])
def test_all_lists_in_use_equals_oracle(env, rois, refs, monkeypatch, capfd, mode):
    torch, N, O = env
    staged(monkeypatch)
    capfd.readouterr()
    got = gpu_fit(torch, N, rois, mode=mode)
    rounds = list_counts(capfd)
    assert any(all(x > 0 for x in r) for r in rounds), "no round with all four B lists and both C lists non-empty: %r" % (rounds[:12],)
    assert_equals_oracle(got, refs[mode], "mode=%d" % mode)


@pytest.mark.parametrize("case", ["park_everywhere", "never_park", "forced_slow"])
def test_limit_overrides_and_slow_queue(env, rois, refs, monkeypatch, capfd, case):
    """park_everywhere: B3 tiles stop after 2 and B10 tiles after 5 iterations, so every B list parks fits (B0 and B1 do by
    default) and B10's go straight to the late list.  never_park: every limit 10 - queue C stays empty.  forced_slow: every
    third fit takes the plain-division Jacobian kernel, whose queue-B appends pick their list the same way."""
    torch, N, O = env
    more = {"park_everywhere": dict(FSQ_LMPAR_B0_ITERS=0, FSQ_LMPAR_B1_ITERS=1, FSQ_LMPAR_B3_ITERS=2, FSQ_LMPAR_B10_ITERS=5, FSQ_LMPAR_C1_ITERS=3),
            "never_park": dict(FSQ_LMPAR_B0_ITERS=10, FSQ_LMPAR_B1_ITERS=10, FSQ_LMPAR_B3_ITERS=10, FSQ_LMPAR_B10_ITERS=10, FSQ_LMPAR_C1_ITERS=10),
            "forced_slow": dict(FSQ_DEBUG_FORCE_SLOW=3)}[case]
    staged(monkeypatch, **more)
    capfd.readouterr()
    got = gpu_fit(torch, N, rois)
    u = used(list_counts(capfd))
    if case == "never_park":
        assert u["C1"] == 0 and u["C3"] == 0, u
    else:
        assert u["C1"] > 0 and u["C3"] > 0, u
    if case == "forced_slow":
        assert N.lib().fsq_fit_last_slow_count() >= len(rois) // 3
    assert_equals_oracle(got, refs[MODE_REF], case)


@pytest.mark.parametrize("n", [65, 129])
def test_partial_tiles_in_every_list(env, rois, refs, monkeypatch, capfd, n):
    """65 and 129 fits: one resp. two tiles and one fit - every list that holds anything ends in a partial tile, and most hold
    nothing but one."""
    torch, N, O = env
    staged(monkeypatch)
    capfd.readouterr()
    got = gpu_fit(torch, N, rois[:n])
    u = used(list_counts(capfd))
    assert all(0 < u[k] <= n for k in LISTS), u
    assert_equals_oracle(got, refs[MODE_REF][:n], "n=%d" % n)


def test_dirty_workspace(env, rois, refs, monkeypatch):
    """A workspace of random bits (what FSQ_TEST_DIRTY_ALLOC=1 hands to every test of a session): the second queue-B array,
    the counters' own cache lines and the dead slots of four lists hold nothing the rounds did not write."""
    torch, N, O = env
    staged(monkeypatch)
    assert_equals_oracle(gpu_fit(torch, N, rois[:129], ws_fill="random"), refs[MODE_REF][:129], "random workspace")


@pytest.fixture(scope="module")
def fields(env):
    """Three 96 x 96 fields on the device, their candidates and the rows of the stand-alone engine run."""
    torch, N, O = env
    from fluorosequencingimageanalysis_amd import engine as E, pflib, synth
    H = W = 96
    prm = E.detect_params(5, pflib.default_correlation_matrix, 2)
    d = E.to_device_u16(np.stack([synth.make_field(170 + i, (H, W), 25) for i in range(3)]))
    eng = E.Engine(3, H, W)
    total = eng.run(d, prm)
    assert total >= 100 + 256
    ref = eng.rows[:total].cpu().numpy().view(N.ROW_DTYPE).reshape(-1).copy()
    ref["key_h"] = ref["key_w"] = -1                    # (consolidation writes the dict keys into kept rows)
    ref.setflags(write=False)
    return E, d, prm, H, W, total, ref


def _rows(N, eng, n):
    r = eng.rows[:n].cpu().numpy().view(N.ROW_DTYPE).reshape(-1).copy()
    r["key_h"] = r["key_w"] = -1
    return r


def _drain(torch, q, tickets):
    cur = torch.cuda.current_stream()
    done = set()
    while len(done) < len(tickets):
        q.advance(0, 0)                                 # (raises RuntimeError on FSQ_EINTERNAL)
        for t in tickets:
            if t not in done and q.take(t, cur):
                done.add(t)
    torch.cuda.synchronize()


@pytest.mark.parametrize("spread", [False, True])
def test_queue_of_256_positions_filled_exactly(env, fields, monkeypatch, capfd, spread):
    """256 positions, 256 live fits, neither batch a multiple of 64.  spread=False: 100 + 156 fresh fits, all of them in B0 in
    round 1 - one list exactly full.  spread=True: the first 100 run three rounds first, then as many fresh fits join as make
    256 alive - the queue is exactly full with fits in every list."""
    torch, N, O = env
    E, d, prm, H, W, total, ref = fields
    staged(monkeypatch)
    e1, e2 = E.Engine(3, H, W, fit_workspace=False), E.Engine(3, H, W, fit_workspace=False)
    for e in (e1, e2):
        assert e.detect(d, prm) == total
    torch.cuda.synchronize()
    q = E.FitQueue(pool_slots=512, queue_cap=256)
    assert q.queue_cap == 256
    capfd.readouterr()
    t1 = q.submit(d, 3, H, W, e1.cand, 100, e1.rows)
    assert t1 is not None
    if spread:
        q.advance(3, 0)
        assert 0 < q.alive <= 100
    k = 256 - q.alive
    t2 = q.submit(d, 3, H, W, e2.cand[100:], k, e2.rows)
    assert t2 is not None and q.alive == 256
    assert q.submit(d, 3, H, W, e2.cand, 1, e2.rows) is None          # not one more
    _drain(torch, q, (t1, t2))
    rounds = list_counts(capfd)
    u = used(rounds)
    assert all(u[name] > 0 for name in LISTS), u
    if spread:          # the round after the fill: 256 fits in the six lists and the Jacobian queue, the older ones past B0
        assert any(sum(r) > 200 and sum(1 for x in r if x > 0) >= 3 for r in rounds), rounds[:8]
    assert _rows(N, e1, 100).tobytes() == ref[:100].tobytes()
    assert _rows(N, e2, k).tobytes() == ref[100:100 + k].tobytes()
    q.close()


def test_batches_of_different_ages_share_lists(env, fields, monkeypatch, capfd):
    """Two batches through one fit queue, the second submitted when the first is three rounds old: their fits sit in the same
    lists and tiles, and each batch equals its stand-alone run."""
    torch, N, O = env
    E, d, prm, H, W, total, ref = fields
    staged(monkeypatch)
    e1, e2 = E.Engine(3, H, W, fit_workspace=False), E.Engine(3, H, W, fit_workspace=False)
    for e in (e1, e2):
        assert e.detect(d, prm) == total
    torch.cuda.synchronize()
    q = E.FitQueue(pool_slots=2 * total, queue_cap=2 * total)
    capfd.readouterr()
    t1 = q.submit(d, 3, H, W, e1.cand, total, e1.rows)
    q.advance(3, 0)
    t2 = q.submit(d, 3, H, W, e2.cand, total, e2.rows)
    assert t1 is not None and t2 is not None
    _drain(torch, q, (t1, t2))
    rounds = list_counts(capfd)
    assert any(all(x > 0 for x in r) for r in rounds), rounds[:12]
    for e in (e1, e2):
        assert _rows(N, e, total).tobytes() == ref.tobytes()
    q.close()
