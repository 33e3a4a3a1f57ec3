"""GPU tests (-m gpu) of fsq_consolidate and fsq_kept_rows at their limits: every case of tests/_consolidate_limit_cases.py through
Engine.consolidate in both of the kernel's forms (and the library's own choice where the case says so), in both rounding modes,
three runs each, against tests/golden/consolidate_limits.npz - what the reference's own loops did with the same fields
(test_consolidate_limits_host.py ties the cases to it on the CPU).  Integers and bit patterns only: no tolerance anywhere."""
import ctypes

import numpy as np
import pytest

import _consolidate_limit_cases as C

pytestmark = pytest.mark.gpu

GPU_CASES = [c for c in C.cases() if c.gpu]
INT32_MIN = -2 ** 31


@pytest.fixture(scope="module")
def fx():
    return C.Fixture()


def _expected(case, fx, py2):
    return fx.expected(case.name, py2) if case.recorded else case.expected(py2)


def _check_launch(case, form, fx, monkeypatch):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from fluorosequencingimageanalysis_amd import _native as N, engine as E
    monkeypatch.delenv("FSQ_CONSOLIDATE_BLOCKS", raising=False)
    monkeypatch.delenv("FSQ_CONSOLIDATE_COMPONENTS", raising=False)
    if form != "default":
        monkeypatch.setenv("FSQ_CONSOLIDATE_" + form.upper(), "1")
    counts, offsets, rows = C.launch_tables(case, N.ROW_DTYPE)
    n, total = len(case.layout), int(counts[-1])
    eng = E.Engine(n, case.H, case.W, fit_workspace=False, cand_per_field=case.H * case.W)
    d_rows = torch.from_numpy(rows.view(np.uint8).reshape(total, 128)) if total else None
    eng.counts.copy_(torch.from_numpy(counts))
    eng.offsets.copy_(torch.from_numpy(offsets))
    for py2 in (True, False):
        exp = _expected(case, fx, py2)
        for rep in range(3):                                    # (the schedule of the waves differs from run to run; the result must not)
            if total:
                eng.rows[:total].copy_(d_rows)
            eng.consolidate(case.thr, case.radius, py2)
            torch.cuda.synchronize()
            nkeep = eng.nkeep.cpu().numpy()
            keep = eng.keep[:max(total, 1)].cpu().numpy()
            out = eng.rows[:max(total, 1)].cpu().numpy().view(N.ROW_DTYPE).reshape(-1)
            where = "%s, %s form, py2_round=%d, run %d" % (case.name, form, py2, rep)
            for s, u in enumerate(case.layout):
                e = exp[u]
                if e is None:
                    assert nkeep[s] == -1, "%s, field %d: the reference's assert fires, the kernel reports %d peaks" % (where, s, nkeep[s])
                    continue
                idx, keys = e
                assert nkeep[s] == len(idx), "%s, field %d: %d kept, the reference keeps %d" % (where, s, nkeep[s], len(idx))
                got = keep[offsets[s]:offsets[s] + nkeep[s]]
                assert np.array_equal(got - offsets[s], np.array(idx, dtype=np.int64)), "%s, field %d: kept set / order differs" % (where, s)
                kk = out[got]
                assert [(int(a), int(b)) for a, b in zip(kk["key_h"], kk["key_w"])] == keys, "%s, field %d: keys" % (where, s)
            # include/fsq.h: a row that is not alive at the re-key holds key_h = INT32_MIN, key_w = -1
            for s, u in enumerate(case.layout):
                if exp[u] is None:
                    continue
                idx = exp[u][0]
                dead = np.ones(counts[s], bool)
                dead[np.array(idx, dtype=np.int64)] = False
                rest = out[offsets[s]:offsets[s] + counts[s]][dead]
                assert (rest["key_h"] == INT32_MIN).all() and (rest["key_w"] == -1).all(), "%s, field %d: keys of rows not kept" % (where, s)
            # the -1 of an asserting field stays in its field: the total counts the others
            assert nkeep[n] == int(np.maximum(nkeep[:n], 0).sum()), where
            # nothing but the keys is written to the rows
            if total:
                a, b = out.copy(), rows.copy()
                a["key_h"] = a["key_w"] = b["key_h"] = b["key_w"] = 0
                assert a.tobytes() == b.tobytes(), where


@pytest.mark.parametrize("form", ["components", "blocks"])
@pytest.mark.parametrize("case", GPU_CASES, ids=lambda c: c.name)
def test_consolidation_equals_the_reference_at_its_limits(case, form, fx, monkeypatch):
    _check_launch(case, form, fx, monkeypatch)


@pytest.mark.parametrize("case", [c for c in GPU_CASES if c.default_form], ids=lambda c: c.name)
def test_the_library_s_own_choice_of_form_gives_the_same_tables(case, fx, monkeypatch):
    """No environment variable: 1 024 fields of 8 waves take the blocks form, 1 023 the components form (csrc/fsq_consolidate.hip)."""
    _check_launch(case, "default", fx, monkeypatch)


def _small_launch(torch, N):
    case = C.by_name("layout_empties")
    counts, offsets, rows = C.launch_tables(case, N.ROW_DTYPE)
    n, total = len(case.layout), int(counts[-1])
    dev = torch.device("cuda")
    t = dict(rows=torch.from_numpy(rows.view(np.uint8).reshape(total, 128).copy()).to(dev), counts=torch.from_numpy(counts).to(dev),
             offsets=torch.from_numpy(offsets).to(dev), keep=torch.full((total,), -77, dtype=torch.int32, device=dev),
             nkeep=torch.full((n + 1,), -77, dtype=torch.int32, device=dev))
    return case, n, total, t


def test_consolidate_refuses_and_writes_nothing():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from fluorosequencingimageanalysis_amd import _native as N
    L = N.lib()
    case, n, total, t = _small_launch(torch, N)
    need = L.fsq_consolidate_workspace_bytes(n, case.H, case.W)
    assert need > 0
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    before = {k: v.clone() for k, v in t.items()}

    def call(rows=t["rows"], counts=t["counts"], offsets=t["offsets"], n_fields=n, H=case.H, W=case.W, radius=case.radius,
             keep=t["keep"], nkeep=t["nkeep"], work=ws, nbytes=need):
        p = lambda x: None if x is None else x.data_ptr()      # noqa: E731
        return L.fsq_consolidate(p(rows), p(counts), p(offsets), n_fields, H, W, case.thr, radius, 1, p(keep), p(nkeep), p(work), nbytes,
                                 torch.cuda.current_stream().cuda_stream)
    refused = {"radius 1": call(radius=1), "radius 0": call(radius=0), "radius -1": call(radius=-1), "H 4": call(H=4), "W 4": call(W=4),
               "n_fields 0": call(n_fields=0), "n_fields -1": call(n_fields=-1), "rows": call(rows=None), "counts": call(counts=None),
               "offsets": call(offsets=None), "keep": call(keep=None), "nkeep": call(nkeep=None), "workspace": call(work=None)}
    assert refused == {k: N.FSQ_EINVAL for k in refused}
    assert call(nbytes=need - 1) == N.FSQ_ENOMEM and call(nbytes=0) == N.FSQ_ENOMEM
    torch.cuda.synchronize()
    for k, v in t.items():
        assert torch.equal(v, before[k]), k
    assert bool((ws == 0x5A).all())
    # and the same arguments, complete, are accepted
    assert call() == N.FSQ_OK
    torch.cuda.synchronize()
    nk = t["nkeep"].cpu().numpy()
    exp = [None if e is None else len(e[0]) for e in case.expected(True)]
    assert [int(x) for x in nk[:n]] == [-1 if exp[u] is None else exp[u] for u in case.layout]


@pytest.mark.parametrize("n_fields", [257, 600])
def test_kept_rows_gather(n_fields):
    """fsq_kept_rows alone on a table of its own: more fields than the 256 threads of its partial sum (600: three rounds of it), a -1
    field and empty fields among them; out_offsets against a host cumulative sum, the rows byte for byte, and `cap` at the total,
    one below, in the middle of a field and 0 - rows at and beyond cap keep what they held."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from fluorosequencingimageanalysis_amd import _native as N
    L = N.lib()
    rng = np.random.default_rng(n_fields)
    counts = rng.integers(0, 7, n_fields).astype(np.int32)
    counts[[0, 5, n_fields - 1]] = [0, 6, 4]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    total = int(offsets[-1])
    nkeep = np.array([rng.integers(0, c + 1) for c in counts] + [0], np.int32)
    nkeep[5], nkeep[n_fields - 1] = 6, 3
    nkeep[[3, 130, 256 if n_fields > 257 else 200]] = -1            # fields whose re-key assertion fired
    nkeep[n_fields] = np.maximum(nkeep[:n_fields], 0).sum()
    keep = np.full(total, -1, np.int32)                              # (the scratch beyond nkeep[f] is never read)
    for f in range(n_fields):
        k = max(int(nkeep[f]), 0)
        keep[offsets[f]:offsets[f] + k] = offsets[f] + rng.permutation(counts[f])[:k]
    rows = rng.integers(0, 256, (total, 128), dtype=np.uint8)
    exp_off = np.concatenate([[0], np.cumsum(np.maximum(nkeep[:n_fields], 0))]).astype(np.int32)
    exp_rows = np.concatenate([rows[keep[offsets[f]:offsets[f] + max(int(nkeep[f]), 0)]] for f in range(n_fields)])
    k_total = int(exp_off[-1])
    assert k_total == nkeep[n_fields] and k_total > n_fields and (nkeep[:n_fields] == 0).any()
    dev = torch.device("cuda")
    d = {k: torch.from_numpy(v).to(dev) for k, v in dict(rows=rows, keep=keep, offsets=offsets, nkeep=nkeep).items()}
    stream = torch.cuda.current_stream().cuda_stream
    mid = int(exp_off[6]) - 3                                        # inside field 5, which keeps 6
    assert exp_off[5] < mid < exp_off[6]
    for cap in (k_total, k_total - 1, mid, 0, k_total + 5):
        out = torch.full((k_total + 8, 128), 0xAB, dtype=torch.uint8, device=dev)
        offs = torch.full((n_fields + 3,), -99, dtype=torch.int32, device=dev)
        rc = L.fsq_kept_rows(d["rows"].data_ptr(), d["keep"].data_ptr(), d["offsets"].data_ptr(), d["nkeep"].data_ptr(), n_fields,
                             out.data_ptr(), cap, offs.data_ptr(), stream)
        assert rc == N.FSQ_OK
        torch.cuda.synchronize()
        got, got_off = out.cpu().numpy(), offs.cpu().numpy()
        assert np.array_equal(got_off[:n_fields + 1], exp_off) and (got_off[n_fields + 1:] == -99).all(), cap
        m = min(cap, k_total)
        assert got[:m].tobytes() == exp_rows[:m].tobytes(), cap
        assert (got[m:] == 0xAB).all(), cap
    # refusals write nothing
    out = torch.full((k_total, 128), 0xAB, dtype=torch.uint8, device=dev)
    offs = torch.full((n_fields + 1,), -99, dtype=torch.int32, device=dev)

    def call(rows=d["rows"], keep=d["keep"], offsets=d["offsets"], nkeep=d["nkeep"], n=n_fields, o=out, cap=k_total, oo=offs):
        p = lambda x: None if x is None else x.data_ptr()      # noqa: E731
        return L.fsq_kept_rows(p(rows), p(keep), p(offsets), p(nkeep), n, p(o), cap, p(oo), stream)
    refused = {"n 0": call(n=0), "n -1": call(n=-1), "rows": call(rows=None), "keep": call(keep=None), "offsets": call(offsets=None),
               "nkeep": call(nkeep=None), "out with cap": call(o=None), "out_offsets": call(oo=None), "cap -1": call(cap=-1)}
    assert refused == {k: N.FSQ_EINVAL for k in refused}
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all()) and bool((offs == -99).all())
    assert call(o=None, cap=0) == N.FSQ_OK                          # (no table asked for: the offsets alone)
    torch.cuda.synchronize()
    assert np.array_equal(offs.cpu().numpy(), exp_off)
