"""Multi-query fusion on the device: ``crh_fuse_select`` against the CPU restatement (tests/fuse_cases.py), bit for bit -- rows,
fused bits, cos bits, lists, first and ``out_info``; and ``HipVectorStore.search_fused`` / ``search_fused_batch`` end to end
against the brute-force best match (``fusion="max"``) and the restatement applied to the oracle's own lists (``fusion="rrf"``),
both run with ``oracle.search`` on ``read_rows`` of the whole collection.  No tolerance appears anywhere.

The restatement's ``k``-output result is the prefix of its ``m * c``-output result (tests/test_fused_host.py pins that): the
sweeps run it once per input at ``k = m * c`` and compare every ``k`` of the device against that prefix."""
import asyncio

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U32, F32 = np.uint32, np.float32
NAMES = ("rows", "fused", "cos", "lists", "first", "info")
CONFIGS = (("rrf", 60, None), ("rrf", 0, None), ("rrf", 60, "uneven"), ("rrf", 0, "uneven"), ("max", 60, None))


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(U32)


def _weights(kind, m):
    return None if kind is None else (np.arange(m, dtype=F32) % 5 * F32(0.37) + F32(0.1) * (np.arange(m) % 2)).astype(F32)   # (list 0 weighs nothing)


def _assert_equal(got, want, k, what):
    for g, w, name in zip(got, want, NAMES):
        w = w if name == "info" else w[:, :k]
        if name in ("fused", "cos"):
            bad = np.flatnonzero((_bits(g) != _bits(w)).any(1)) if g.size else []
            assert len(bad) == 0, f"{what}: {name} bits differ at query {bad[:4]}\n{g[bad[:1]]}\n{w[bad[:1]]}"
        else:
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f"{what}: {name} differ\n{g}\n{w}"


# ------------------------------------------------------------------ crh_fuse_select against the restatement
@pytest.mark.parametrize("m,c", [(1, 1), (1, 7), (2, 64), (3, 100), (5, 200), (16, 64), (8, 128), (4, 256), (1, 1024)])
def test_fuse_select_equals_the_restatement(gpu, m, c):
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from tests import fuse_cases
    launches = 0
    for nq in (0, 1, 64, 200):
        for mode in ("mixed", "disjoint", "identical", "overlap"):
            if nq == 200 and mode != "mixed":
                continue
            scores, rows = fuse_cases.lists(nq, m, c, mode, seed=m * 100000 + c * 10 + nq)
            sd, rd = torch.from_numpy(scores).cuda(), torch.from_numpy(rows).cuda()
            for method, rrf_k, wkind in CONFIGS:
                w = _weights(wkind, m)
                want = fuse_cases.fuse_select(scores, rows, m, m * c, method, rrf_k, w)
                for k in sorted({1, m * c}):
                    shaped = (sd, rd) if k == 1 else (sd.reshape(nq * m, c), rd.reshape(nq * m, c))      # both accepted layouts
                    out = ffi.fuse_select(*shaped, m, k, method, rrf_k, w)
                    torch.cuda.synchronize()
                    launches += 1
                    _assert_equal([o.cpu().numpy() for o in out], want, k, f"m={m} c={c} nq={nq} {mode} {method} rrf_k={rrf_k} w={wkind} k={k}")
                if m == 1 and nq and method == "max":                    # one list: the list itself
                    assert np.array_equal(want[0], rows[:, 0]) and np.array_equal(_bits(want[2]), _bits(scores[:, 0]))
    assert launches == 13 * len(CONFIGS) * len({1, m * c})


def test_fuse_select_a_row_named_twice_inside_one_list(gpu):
    """Searches and merges never name a row twice in one list, but the C entry accepts such lists: every entry still adds its
    contribution in ascending u, the list's bit is set once and ``first`` is the earlier entry -- the entry-by-entry walk of
    the restatement (``fuse_select`` takes it for such lists), bit for bit."""
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from tests import fuse_cases
    for m, c in ((1, 7), (3, 100), (4, 256)):
        scores, rows = fuse_cases.lists(9, m, c, "overlap", seed=m + c)
        rng = np.random.default_rng(c)
        for q in range(9):                                             # copy some entries' rows over later entries of the same list
            for j in range(m):
                src, dst = rng.integers(0, c, 6), rng.integers(0, c, 6)
                keep = (rows[q, j, src] >= 0) & (rows[q, j, dst] >= 0)
                rows[q, j, dst[keep]] = rows[q, j, src[keep]]
        srt = np.sort(rows, axis=2)
        assert ((srt[:, :, 1:] == srt[:, :, :-1]) & (srt[:, :, 1:] >= 0)).any((1, 2)).sum() >= 3
        sd, rd = torch.from_numpy(scores).cuda(), torch.from_numpy(rows).cuda()
        for method, rrf_k, wkind in CONFIGS:
            w = _weights(wkind, m)
            want = fuse_cases.fuse_select(scores, rows, m, m * c, method, rrf_k, w)
            for k in sorted({1, 10, m * c} & set(range(1, m * c + 1))):
                out = ffi.fuse_select(sd, rd, m, k, method, rrf_k, w)
                torch.cuda.synchronize()
                _assert_equal([o.cpu().numpy() for o in out], want, k, f"repeated rows m={m} c={c} {method} rrf_k={rrf_k} w={wkind} k={k}")


def test_fuse_select_neighbouring_buffers_and_arguments(gpu):
    """nq = 3 inside buffers sized for 5: the neighbours' slots keep their sentinels; refused arguments launch nothing."""
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from tests import fuse_cases
    L = ffi.lib()
    m, c, k = 3, 100, 12
    scores, rows = fuse_cases.lists(3, m, c, "overlap", seed=5)
    want = fuse_cases.fuse_select(scores, rows, m, k, "rrf", 60)
    dev = "cuda:0"
    ins = [torch.from_numpy(a).to(dev) for a in (scores, rows)]
    outs = [torch.full((5, k), -77, dtype=t, device=dev) for t in (torch.int64, torch.float32, torch.float32, torch.int32, torch.int32)]
    info = torch.full((5, 2), -77, dtype=torch.int32, device=dev)
    ptr = [int(o[1:4].data_ptr()) for o in outs] + [int(info[1:4].data_ptr())]
    inp = [int(t.data_ptr()) for t in ins]
    assert L.crh_fuse_select(3, m, c, k, ffi.FUSE_RRF, 60, None, *inp, *ptr, None) == ffi.OK
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in outs] + [info.cpu().numpy()]
    _assert_equal([h[1:4] for h in host], want, k, "inside larger buffers")
    assert all((h[0] == -77).all() and (h[4] == -77).all() for h in host)
    for o in outs + [info]:
        o.fill_(-77)
    w = np.ones((m,), F32)
    neg = np.asarray([1, -1, 1], F32)
    for nq_, m_, c_, k_, method, rrf_k, wt in ((3, m, c, 0, 0, 60, None), (3, m, c, m * c + 1, 0, 60, None), (3, 0, c, k, 0, 60, None), (3, 17, 60, k, 0, 60, None),
                                               (3, 4, 257, k, 0, 60, None), (-1, m, c, k, 0, 60, None), (3, m, c, k, 2, 60, None), (3, m, c, k, 0, -1, None),
                                               (3, m, c, k, 1, 60, w), (3, m, c, k, 0, 60, neg)):
        rc = L.crh_fuse_select(nq_, m_, c_, k_, method, rrf_k, None if wt is None else wt.ctypes.data, *inp, *ptr, None)
        assert rc == ffi.E_INVALID, (nq_, m_, c_, k_, method, rrf_k)
    with pytest.raises(ffi.NativeError, match="int64"):
        ffi.fuse_select(ins[0], ins[1].int(), m, k)
    with pytest.raises(ffi.NativeError, match="shape"):
        ffi.fuse_select(ins[0], ins[1][:, :, :7].contiguous(), m, 4)
    with pytest.raises(ffi.NativeError, match="whole sets"):
        ffi.fuse_select(ins[0].reshape(9, c)[:8].contiguous(), ins[1].reshape(9, c)[:8].contiguous(), m, 4)
    with pytest.raises(ValueError):
        ffi.fuse_select(ins[0], ins[1], m, k, "borda")
    with pytest.raises(ValueError):
        ffi.fuse_select(ins[0], ins[1], m, k, "max", weights=[1, 1, 1])
    torch.cuda.synchronize()
    assert all((o.cpu().numpy() == -77).all() for o in outs + [info])


# ------------------------------------------------------------------ end to end through the store
def _payloads(n):
    return [{"file_path": f"/proj/f{i % 9}.py", "entity_type": "function", "entity_name": f"ent{i}", "language": ("python", "go", "rust")[i % 3],
             "start_line": i, "end_line": i + 3, "content": f"def ent{i}(): pass", "graph_node_id": f"mod.ent{i}", "content_hash": "h",
             "project_name": "p1"} for i in range(n)]


def _quads(hits):
    return [(h["id"], _bits(h["score"]).item(), _bits(h["cosine"]).item(), h["matched"]) for h in hits]


async def _filled(s, ids, raw, payloads, shards):
    """The collection in four appends (the blocks go round the shards); returns the stored rows in slot order and every
    slot's GLOBAL row (the order ties follow)."""
    from coderag_amd.shards import STRIDE
    n = len(raw)
    await s.create_collections()
    step = (n + 3) // 4
    for a in range(0, n, step):
        await s.upsert("code_chunks", ids[a:a + step], raw[a:a + step], payloads[a:a + step])
    col = s._col("code_chunks")
    assert all(r > 0 for r in col.shards.rows)
    sh, lo = col.rows_of(np.arange(n))
    stored = {t: col.shards.index[t].read_rows(0, col.shards.rows[t]) for t in range(shards)}
    return np.stack([stored[int(sh[i])][int(lo[i])] for i in range(n)]), np.asarray(sh, np.int64) * STRIDE + np.asarray(lo, np.int64)


@pytest.mark.parametrize("shards", [1, 2])
@pytest.mark.parametrize("dtype_name", ["bf16", "f32"])
def test_store_fused_search_equals_the_oracle(gpu, dtype_name, shards):
    """900 rows of which 60 are exact copies (ties), three query sets (four random vectors; three ON stored rows, two of them
    a duplicated pair's; one alone), without and with a filter + tombstones.  ``max``: ids, score bits and matched of the
    brute force over every row's oracle score; ``rrf``: the restatement on the oracle's own top-``candidates`` lists."""
    import coderag_amd  # noqa: F401
    from coderag_amd.store import HipVectorStore
    from oracle import search as orc
    from tests import fuse_cases
    raw, sets = fuse_cases.corpus()
    n = len(raw)
    ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(n)]
    bf16 = dtype_name == "bf16"

    async def run():
        async with HipVectorStore(dim=raw.shape[1], dtype=dtype_name, initial_capacity=2048, device=0, shards=shards, compact_dead_fraction=0.0) as s:
            stored, gid = await _filled(s, ids, raw, _payloads(n), shards)
            order = np.argsort(gid)
            passing = None
            for round_ in range(2):
                kw = {} if round_ == 0 else {"filters": {"language": ["python", "rust"]}, "must_not": {"file_path": "/proj/f2.py"}}
                if round_ == 1:
                    await s.delete("code_chunks", {"file_path": "/proj/f4.py"})                    # tombstones
                    i = np.arange(n)
                    passing = (i % 3 != 1) & (i % 9 != 2) & (i % 9 != 4)
                for qi, qs in enumerate(sets):
                    qp = orc.preprocess(qs, to_bf16=bf16)
                    m = len(qs)
                    for limit, cand in ((10, None), (25, 25), (1, 1)):
                        c = cand if cand is not None else 40
                        what = f"{dtype_name} shards={shards} round {round_} set {qi} limit {limit} candidates {c}"
                        got = await s.search_fused("code_chunks", qs, limit=limit, fusion="max", candidates=cand, **kw)
                        ef, er = fuse_cases.brute_force_max(stored[order], qp, limit, None if passing is None else passing[order])
                        ls, lr = fuse_cases.oracle_lists(stored[order], qp, c, None if passing is None else passing[order])
                        matched = [[j for j in range(m) if r in lr[j]] for r in er]
                        assert _quads(got) == [(ids[order[r]], _bits(f).item(), _bits(f).item(), mt) for f, r, mt in zip(ef, er, matched)], what
                        assert len(got) == limit
                        for rrf_k, w in ((60, None), (0, None), (2, (np.arange(m) + 1.0) / 2)):
                            got = await s.search_fused("code_chunks", qs.tolist(), limit=limit, fusion="rrf", rrf_k=rrf_k, weights=w, candidates=cand, **kw)
                            want = fuse_cases.expected(stored, gid, qp, limit, c, "rrf", rrf_k=rrf_k, weights=w, passing=passing)
                            assert _quads(got) == [(ids[t], f, cv, mt) for t, f, cv, mt in want], f"{what} rrf_k={rrf_k} w={w}"
                # ragged sets in one batch: every set's answer is its lone call's
                for bkw in ({}, {"fusion": "max"}, {"rrf_k": 3, "candidates": 30}):
                    batch = await s.search_fused_batch("code_chunks", sets, limit=10, **bkw, **kw)
                    alone = [await s.search_fused("code_chunks", one, limit=10, **bkw, **kw) for one in sets]
                    assert [_quads(b) for b in batch] == [_quads(a) for a in alone] and all(len(b) == 10 for b in batch)
            assert await s.search_fused("code_chunks", sets[0], limit=5, filters={"language": "cobol"}) == []

    asyncio.run(run())
