"""Multi-query fusion (RRF / best match) above the device: the CPU restatement of ``crh_fuse_select`` (tests/fuse_cases.py) and the
properties DESIGN.md 3.16 states; the new C entry's export and argument checks; the store's ``search_fused`` /
``search_fused_batch`` on 1 and 2 local shards over a fake index with ``ffi.fuse_select`` replaced by the restatement; two gloo
ranks returning identical fused lists; the searchers' and the MCP tool's forwarding of ``extra_queries``; ``plan_query_texts``."""
import asyncio
import os
import socket
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest

from oracle import search as orc
from tests import fuse_cases
from tests.fake_index import fake_device
from tests.test_filter_sets_host import SetFakeIndex, _corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, F32 = np.uint32, np.float32
NAMES = ("rows", "fused", "cos", "lists", "first", "info")


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(U32)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) if x.dtype == F32 else np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("method", ["rrf", "max"])
def test_restatement_list_by_list_equals_the_walk_and_prefixes_hold(method):
    for (m, c), mode in (((3, 20), "overlap"), ((5, 13), "mixed"), ((2, 32), "identical"), ((4, 9), "disjoint")):
        scores, rows = fuse_cases.lists(7, m, c, mode, seed=m * c)
        w = None if method == "max" else np.linspace(0.5, 2.0, m).astype(F32)
        full = fuse_cases.fuse_select(scores, rows, m, m * c, method, 60, w)
        for q in range(7):                                            # the entry-by-entry walk IS the definition
            one = fuse_cases.fuse_select_one(scores[q], rows[q], m * c, method, 60, w)
            assert _same([a[q] for a in full], one), (mode, q)
        for j in (1, 5, m * c):                                       # the first j outputs of a k-output call are the j-output call
            part = fuse_cases.fuse_select(scores.reshape(7 * m, c), rows.reshape(7 * m, c), m, j, method, 60, w)
            assert _same(part[:5], [a[:, :j] for a in full[:5]]) and np.array_equal(part[5], full[5])
        real = rows >= 0
        assert np.array_equal(full[5][:, 1], real.sum((1, 2)))
        assert np.array_equal(full[5][:, 0], [np.unique(rows[q][real[q]]).size for q in range(7)])
        assert (full[5][4] == 0).all() and (full[0][4] == -1).all() and np.isneginf(full[1][4]).all() and (full[4][4] == -1).all()   # an all-padding query
        for q in range(7):                                            # descending in the ord order, ties to the lower row
            d = int(full[5][q, 0])
            key = fuse_cases.ord_f32(full[1][q, :d]).astype(np.int64)
            assert ((np.diff(key) < 0) | ((np.diff(key) == 0) & (np.diff(full[0][q, :d]) > 0))).all()


def test_restatement_one_list_is_the_list_itself():
    scores, rows = fuse_cases.lists(6, 1, 50, "mixed", seed=2)
    for method in ("rrf", "max"):
        r, fused, cos, lists, first, info = fuse_cases.fuse_select(scores, rows, 1, 50, method)
        assert np.array_equal(r, rows[:, 0]) and np.array_equal(_bits(cos), _bits(scores[:, 0]))
        real = rows[:, 0] >= 0
        assert np.array_equal(lists, real.astype(np.int32)) and np.array_equal(first, np.where(real, np.arange(50), -1))
        if method == "max":
            assert np.array_equal(_bits(fused), _bits(scores[:, 0]))
        else:
            assert np.array_equal(_bits(fused[real]), _bits((F32(1) / (np.arange(50) + 61).astype(F32))[np.nonzero(real)[1]]))


def test_restatement_ties_weights_padding_shard_bits_and_signed_zero():
    big = 5 << 32
    # the symmetric tie: A at positions (0, 1), B at (1, 0) -- equal bits, the lower row first
    scores = np.asarray([[[0.9, 0.8, 0.1], [0.7, 0.6, 0.2]]], F32)
    rows = np.asarray([[[big + 9, big + 4, 1], [big + 4, big + 9, 2]]], np.int64)
    r, fused, cos, lists, first, info = fuse_cases.fuse_select(scores, rows, 2, 6)
    assert r[0].tolist() == [big + 4, big + 9, 1, 2, -1, -1] and _bits(fused[0, 0]) == _bits(fused[0, 1]) and info.tolist() == [[4, 6]]
    assert _bits(fused[0, 0]) == _bits(F32(F32(0) + F32(1) / F32(62)) + F32(1) / F32(61))          # ascending u: list 0's entry first
    assert cos[0, :4].tolist() == [F32(0.8), F32(0.9), F32(0.1), F32(0.2)] and lists[0].tolist() == [3, 3, 1, 2, 0, 0]
    assert first[0].tolist() == [1, 0, 2, 5, -1, -1]
    # weights that reorder: list 1 alone outweighs list 0
    r2 = fuse_cases.fuse_select(scores, rows, 2, 2, "rrf", 0, [1.0, 3.0])[0]
    assert r2[0].tolist() == [big + 4, big + 9]
    r3 = fuse_cases.fuse_select(scores, rows, 2, 2, "rrf", 0, [3.0, 1.0])[0]
    assert r3[0].tolist() == [big + 9, big + 4]
    w0 = fuse_cases.fuse_select(scores, rows, 2, 6, "rrf", 60, [0.0, 1.0])
    assert w0[0][0].tolist() == [big + 4, big + 9, 2, 1, -1, -1] and w0[1][0, 3] == 0.0           # a weightless list still names its rows
    # MAX: the best cosine; -0.0 sorts below +0.0
    z = np.asarray([[[0.0, -0.0], [-0.0, -1.0]]], F32)
    zr = np.asarray([[[7, 3], [5, 7]]], np.int64)
    r, fused, cos, lists, first, info = fuse_cases.fuse_select(z, zr, 2, 4, "max")
    assert r[0].tolist() == [7, 3, 5, -1] and _bits(fused[0, :3]).tolist() == [0, 0x80000000, 0x80000000] and lists[0].tolist() == [3, 1, 2, 0]
    assert np.array_equal(_bits(fused), _bits(cos))
    # one list all padding, and a query that is nothing else
    scores = np.asarray([[[0.5, 0.4], [-np.inf, -np.inf]], [[-np.inf] * 2] * 2], F32)
    rows = np.asarray([[[3, 8], [-1, -1]], [[-1, -1], [-1, -1]]], np.int64)
    r, fused, cos, lists, first, info = fuse_cases.fuse_select(scores, rows, 2, 3)
    assert r.tolist() == [[3, 8, -1], [-1, -1, -1]] and info.tolist() == [[2, 2], [0, 0]] and lists.tolist() == [[1, 1, 0], [0, 0, 0]]
    assert np.isneginf(fused[1]).all() and np.isneginf(cos[1]).all() and first[1].tolist() == [-1, -1, -1]


def test_restatement_max_is_the_exact_best_match_of_the_corpus():
    raw, sets = fuse_cases.corpus()
    x = orc.preprocess(raw)
    passing = np.random.default_rng(1).random(len(x)) > 0.2
    for qs in sets:
        qp = orc.preprocess(qs)
        for limit, c in ((1, 1), (10, 10), (10, 40), (64, 64)):
            for pas in (None, passing):
                s, r = fuse_cases.oracle_lists(x, qp, c, pas)
                got = fuse_cases.fuse_select(s[None], r[None], len(qp), limit, "max")
                ef, er = fuse_cases.brute_force_max(x, qp, limit, pas)
                assert np.array_equal(got[0][0], er) and np.array_equal(_bits(got[1][0]), _bits(ef)), (len(qp), limit, c)


# ------------------------------------------------------------------ ABI
def test_new_entry_is_exported_and_checks_its_arguments():
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    L = ffi.lib()
    assert "crh_fuse_select" in ffi.EXPORTS and hasattr(L, "crh_fuse_select")
    assert L.crh_abi_version() == 4 and ffi.MAX_LISTS == 16 and (ffi.FUSE_RRF, ffi.FUSE_MAX) == (0, 1)
    one = 16   # (a non-NULL, never dereferenced pointer: every case below is refused before a launch)
    ok_w = np.ones((16,), F32)

    def call(nq, m, c, k, method, rrf_k, w=None, p=one):
        return L.crh_fuse_select(nq, m, c, k, method, rrf_k, None if w is None else w.ctypes.data, p, p, p, p, p, p, p, p, None)
    for args, word in (((1, 0, 8, 1, 0, 60), b"m="), ((1, 17, 8, 1, 0, 60), b"m="), ((1, 2, 0, 1, 0, 60), b"c="), ((1, 2, 513, 1, 0, 60), b"m * c"),
                       ((1, 16, 65, 1, 0, 60), b"m * c"), ((1, 1, 2048, 1, 0, 60), b"c="), ((1, 2, 8, 0, 0, 60), b"k="), ((1, 2, 8, 17, 0, 60), b"k="),
                       ((-1, 2, 8, 4, 0, 60), b"nq="), ((1, 2, 8, 4, 2, 60), b"method"), ((1, 2, 8, 4, -1, 60), b"method"),
                       ((1, 2, 8, 4, 0, -1), b"rrf_k"), ((0, 2, 8, 4, 0, -1), b"rrf_k")):
        assert call(*args) == ffi.E_INVALID, args
        assert word in L.crh_last_error(), (args, L.crh_last_error())
    for bad in (np.nan, np.inf, -1.0, -np.inf):
        w = ok_w.copy()
        w[1] = bad
        assert call(1, 2, 8, 4, 0, 60, w) == ffi.E_INVALID and b"weights" in L.crh_last_error()
    assert call(1, 2, 8, 4, 1, 60, ok_w) == ffi.E_INVALID and b"MAX" in L.crh_last_error()          # weights with MAX
    assert call(1, 2, 8, 4, 0, 60, p=None) == ffi.E_INVALID and b"NULL" in L.crh_last_error()
    assert call(0, 2, 8, 4, 0, 60, p=None) == ffi.OK and call(0, 16, 64, 1024, 1, 0, p=None) == ffi.OK       # nothing to do
    with pytest.raises(ffi.NativeError, match="device tensor"):
        ffi.fuse_select(np.zeros((2, 4), F32), np.zeros((2, 4), np.int64), 2, 2)
    with pytest.raises(ValueError, match="fusion"):
        ffi.fuse_method("borda")


# ------------------------------------------------------------------ store plumbing over the fake index
def _fake_device(monkeypatch):
    ffi = fake_device(monkeypatch, SetFakeIndex)
    monkeypatch.setattr(ffi, "fuse_select", fuse_cases.fuse_select)
    return ffi


def _quads(hits):
    return [(h["id"], _bits(h["score"]).item(), _bits(h["cosine"]).item(), h["matched"]) for h in hits]


@pytest.mark.parametrize("shards", [1, 2])
def test_store_fused_search_hits_ragged_sets_and_arguments(monkeypatch, shards):
    from coderag_amd.errors import VectorStoreError
    from coderag_amd.shards import STRIDE
    from coderag_amd.store import HipVectorStore
    ffi = _fake_device(monkeypatch)
    rng, vecs, payloads, ids = _corpus()
    vecs[200:220] = vecs[20:40]                                                    # duplicated rows: ties in every list
    qs = np.concatenate([rng.standard_normal((3, 768)).astype(F32), vecs[25:26]])
    stored = orc.preprocess(vecs)
    lang = np.asarray([p["language"] for p in payloads])
    proj = np.asarray([p["project_name"] for p in payloads])

    async def run():
        kw = {"shards": shards, "_merge_fn": orc.merge_topk} if shards > 1 else {}
        async with HipVectorStore(dim=768, dtype="f32", initial_capacity=512, device=0, compact_dead_fraction=0.0, **kw) as s:
            await s.create_collections()
            for a in range(0, 240, 60):
                await s.upsert("code_chunks", ids[a:a + 60], vecs[a:a + 60], payloads[a:a + 60])
            col = s._col("code_chunks")
            sh, lo = col.rows_of(np.arange(240))
            gid = np.asarray(sh, np.int64) * STRIDE + np.asarray(lo, np.int64)

            def want(q, limit, c, method, passing=None, **kw):
                return [(ids[t], f, cv, m) for t, f, cv, m in fuse_cases.expected(stored, gid, orc.preprocess(q), limit, c, method, passing=passing, **kw)]
            before = s.search_passes
            got = await s.search_fused("code_chunks", qs, limit=10)
            assert s.search_passes - before == 1
            assert _quads(got) == want(qs, 10, 40, "rrf") and len(got) == 10
            assert all(set(h) == {"id", "score", "payload", "cosine", "matched"} and h["payload"]["entity_name"] for h in got)
            assert all(m == sorted(m) and m and set(m) <= {0, 1, 2, 3} for _, _, _, m in _quads(got))
            assert _quads(await s.search_fused("code_chunks", qs.tolist(), limit=10, fusion="max", candidates=10)) == want(qs, 10, 10, "max")
            mx = await s.search_fused("code_chunks", qs, limit=7, fusion="MAX")
            ef, er = fuse_cases.brute_force_max(stored[np.argsort(gid)], orc.preprocess(qs), 7)
            assert [(h["id"], _bits(h["score"]).item()) for h in mx] == [(ids[np.argsort(gid)[r]], _bits(f).item()) for f, r in zip(ef, er)]
            got = await s.search_fused("code_chunks", qs, limit=12, filters={"language": ["python", "go"]}, must_not={"project_name": "p2"},
                                       rrf_k=0, weights=[1, 2, 0.5, 0], candidates=30)
            passing = np.isin(lang, ["python", "go"]) & (proj != "p2")
            assert _quads(got) == want(qs, 12, 30, "rrf", passing, rrf_k=0, weights=[1, 2, 0.5, 0])
            assert await s.search_fused("code_chunks", qs, limit=5, filters={"language": "cobol"}) == []
            one = await s.search_fused("code_chunks", qs[:1], limit=10, fusion="max")              # m = 1: the plain search
            plain = await s.search("code_chunks", qs[0].tolist(), limit=10)
            assert [(h["id"], h["score"]) for h in one] == [(h["id"], h["score"]) for h in plain] and all(h["matched"] == [0] for h in one)
            # ragged sets: every set fuses its own lists, as a lone call with that set does
            sets = [qs, qs[1:2], qs[[3, 0]], vecs[7:10].tolist()]
            for kwargs in ({}, {"fusion": "max"}, {"rrf_k": 5, "candidates": 25, "filters": {"language": "go"}}):
                batch = await s.search_fused_batch("code_chunks", sets, limit=10, **kwargs)
                alone = [await s.search_fused("code_chunks", one, limit=10, **kwargs) for one in sets]
                assert [_quads(b) for b in batch] == [_quads(a) for a in alone] and len(batch) == 4
            assert await s.search_fused_batch("code_chunks", [], limit=10) == []
            # every bad value fails its own caller only, with a ValueError behind it
            bad = [s.search_fused("code_chunks", qs, limit=10, candidates=9),
                   s.search_fused("code_chunks", np.tile(qs, (5, 1))[:17], limit=10),
                   s.search_fused("code_chunks", qs, limit=10, candidates=257),
                   s.search_fused("code_chunks", qs, limit=300),
                   s.search_fused("code_chunks", qs, limit=10, fusion="borda"),
                   s.search_fused("code_chunks", qs, limit=10, fusion=None),
                   s.search_fused("code_chunks", qs, limit=10, weights=[1, 1, 1]),
                   s.search_fused("code_chunks", qs, limit=10, weights=[1, 1, 1, -1]),
                   s.search_fused("code_chunks", qs, limit=10, weights=[1, 1, 1, float("nan")]),
                   s.search_fused("code_chunks", qs, limit=10, fusion="max", weights=[1, 1, 1, 1]),
                   s.search_fused("code_chunks", qs, limit=10, rrf_k=-1),
                   s.search_fused("code_chunks", qs[:, :700], limit=10),
                   s.search_fused("code_chunks", qs[0], limit=10),
                   s.search_fused("code_chunks", [], limit=10),
                   s.search_fused_batch("code_chunks", [qs, []], limit=10),
                   s.search_fused("nope", qs, limit=10)]
            res = await asyncio.gather(s.search_fused("code_chunks", qs, limit=10), *bad, return_exceptions=True)
            assert _quads(res[0]) == want(qs, 10, 40, "rrf")
            assert all(isinstance(r, VectorStoreError) for r in res[1:]), res[1:]
            assert all(isinstance(r.cause, ValueError) for r in res[1:-1]), [r.cause for r in res[1:-1]]
            # the fused calls never join the coalescer: a plain call beside two of them is three passes
            before = s.search_passes
            await asyncio.gather(s.search_fused("code_chunks", qs, limit=4), s.search("code_chunks", qs[0].tolist(), limit=4),
                                 s.search_fused("code_chunks", qs, limit=4))
            assert s.search_passes - before == 3

    asyncio.run(run())


# ------------------------------------------------------------------ two ranks: the same merged lists, the same fusion, no collective
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gloo_worker(rank: int, world: int, port: int, out_dir: str) -> None:
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from coderag_amd.shards import STRIDE, ShardSet
    from tests import fuse_cases
    ffi.fuse_select = fuse_cases.fuse_select
    raw, sets = fuse_cases.corpus(dim=64)                               # the same on every rank
    dim = raw.shape[1]
    sh = ShardSet(world, lambda s: SetFakeIndex(dim=dim, capacity_rows=2048, n_code_cols=1), backend="dist", block=50, merge_fn=orc.merge_topk)
    shard = sh.route(len(raw))
    sh.append({rank: raw[shard == rank]}, np.zeros((len(raw), 1), np.int32), shard=shard)
    assert all(r > 0 for r in sh.rows)
    gid = np.empty(len(raw), np.int64)
    for s in range(world):
        sel = np.flatnonzero(shard == s)
        gid[sel] = s * STRIDE + np.arange(sel.size)
    stored = orc.preprocess(raw)
    m = max(len(q) for q in sets)
    queries = np.zeros((len(sets), m, dim), np.float32)
    live = np.zeros((len(sets), m), bool)
    for i, q in enumerate(sets):
        queries[i, :len(q)], live[i, :len(q)] = q, True
    for method, kw in (("rrf", {"rrf_k": 60, "weights": None}), ("rrf", {"rrf_k": 1, "weights": [2.0, 1.0, 1.0, 0.5]}), ("max", {"rrf_k": 60, "weights": None})):
        rows, fused, cos, lists, first, info = sh.search_fused(queries, 20, 50, None, method, kw["rrf_k"], kw["weights"], live)
        for i, q in enumerate(sets):
            w = None if kw["weights"] is None else kw["weights"][:len(q)]
            exp = fuse_cases.expected(stored, gid, orc.preprocess(q), 20, 50, method, rrf_k=kw["rrf_k"], weights=w)
            got = [(int(np.flatnonzero(gid == r)[0]), _bits(f).item(), _bits(c).item(), [j for j in range(16) if b >> j & 1])
                   for r, f, c, b in zip(rows[i], fused[i], cos[i], lists[i]) if r >= 0]
            assert got == exp, f"rank {rank}: {method} set {i} differs"
        np.save(os.path.join(out_dir, f"rows{rank}_{method}_{kw['rrf_k']}.npy"), rows)
        np.save(os.path.join(out_dir, f"fused{rank}_{method}_{kw['rrf_k']}.npy"), fused)
    dist.destroy_process_group()


def test_two_gloo_ranks_return_identical_fused_lists(tmp_path):
    import torch.multiprocessing as mp
    port = _free_port()
    mp.spawn(_gloo_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    names = sorted(os.listdir(tmp_path))
    assert len(names) == 12
    for n in names:
        if n.startswith(("rows0", "fused0")):
            a, b = np.load(os.path.join(tmp_path, n)), np.load(os.path.join(tmp_path, n.replace("0_", "1_", 1)))
            assert a.tobytes() == b.tobytes() and a.shape[1] == 20, n


# ------------------------------------------------------------------ searchers, the MCP tool, the planner's texts
class _Recorder:
    def __init__(self):
        self.calls = []

    async def search(self, **kw):
        self.calls.append(("search", kw))
        return []

    async def search_fused(self, **kw):
        self.calls.append(("search_fused", kw))
        return [{"id": "a", "score": 0.03, "cosine": 0.5, "matched": [0, 2],
                 "payload": {"file_path": "f.py", "entity_type": "function", "entity_name": "e", "content": "x", "summary": "s"}}]


class _Embedder:
    def __init__(self):
        self.batches = []

    async def embed(self, text):
        return [0.0] * 4

    async def embed_batch(self, texts):
        self.batches.append(list(texts))
        return [[float(i)] * 4 for i, _ in enumerate(texts)]


def test_searcher_fuses_only_when_extra_queries_are_given():
    from coderag_amd import mcp_tools, vector_search
    from coderag_amd.errors import QueryError

    async def run():
        rec, emb = _Recorder(), _Embedder()
        vs = vector_search.VectorSearcher(rec, emb)
        for extra in ({}, {"extra_queries": None}, {"extra_queries": [], "fusion": "max"}, {"extra_queries": ["", "  "]}, {"fusion": None}):
            await vs.search_code("q", limit=3, language="python", **extra)
            await vs.search_summaries("q", limit=3, **extra)
        assert [name for name, _ in rec.calls] == ["search"] * 10 and not emb.batches
        assert [set(kw) for _, kw in rec.calls] == [{"collection", "query_vector", "limit", "filters"}] * 10       # today's call shape
        rec.calls.clear()
        code = await vs.search_code("q", limit=3, language="python", extra_queries=["q2", " ", "q3"])
        summ = await vs.search_summaries("q", limit=3, extra_queries=["q2"], fusion="max", candidates=9)
        assert emb.batches == [["q", "q2", "q3"], ["q", "q2"]]                                      # ONE provider batch per call
        (n1, k1), (n2, k2) = rec.calls
        assert n1 == n2 == "search_fused" and set(k1) == {"collection", "query_vectors", "limit", "fusion", "filters"}
        assert k1["fusion"] == "rrf" and k1["filters"] == {"language": "python"} and np.asarray(k1["query_vectors"]).shape == (3, 4)
        assert k2["fusion"] == "max" and k2["candidates"] == 9 and k2["collection"] == "summaries" and np.asarray(k2["query_vectors"]).shape == (2, 4)
        assert code[0]["score"] == 0.03 and code[0]["cosine"] == 0.5 and code[0]["matched"] == [0, 2] and code[0]["entity_name"] == "e"
        assert summ[0]["summary"] == "s" and summ[0]["matched"] == [0, 2]
        for kw in ({"diversity": 0.5}, {"max_per_file": 2}):
            with pytest.raises(ValueError):
                await vs.search_code("q", extra_queries=["q2"], **kw)
        with pytest.raises(QueryError):
            await vs.search_code(" ", extra_queries=["q2"])

        class Searcher:
            def __init__(self):
                self.kw = []

            async def search_code(self, **kw):
                self.kw.append(kw)
                return []
        sr = Searcher()
        tool = mcp_tools.create_semantic_search_tool(lambda: sr)
        assert (await tool["function"]("find it")).success and (await tool["function"]("find it", extra_queries=["locate it"], fusion="max")).success
        assert (await tool["function"]("find it", extra_queries=[])).success
        assert sr.kw == [{"query": "find it", "limit": 5, "entity_type": None},
                         {"query": "find it", "limit": 5, "entity_type": None, "extra_queries": ["locate it"], "fusion": "max"},
                         {"query": "find it", "limit": 5, "entity_type": None}]
        assert "extra_queries" in tool["parameters"] and "fusion" in tool["parameters"]

    asyncio.run(run())


def test_plan_query_texts():
    from coderag_amd.engine_helpers import plan_query_texts
    from coderag_amd.query_types import QueryIntent, QueryPlan
    intent = list(QueryIntent)[0]

    def plan(subs):
        return QueryPlan(original_query="how is auth done", primary_intent=intent, sub_queries=subs)
    sq = lambda text, kind, prio=1: NS(query_text=text, search_type=kind, priority=prio)   # noqa: E731
    assert plan_query_texts(plan([]), "how is auth done") == ["how is auth done"]
    subs = [sq("token check", "vector", 2), sq("who calls login", "graph", 0), sq("login flow", "hybrid", 1), sq("", "vector"), sq("  ", "vector"),
            sq("how is auth done", "vector", 0), sq("token check", "hybrid", 0), {"query_text": "session store", "search_type": "VECTOR", "priority": 2},
            sq(None, "vector"), sq("no kind", None)]
    assert plan_query_texts(plan(subs), "how is auth done") == ["how is auth done", "token check", "login flow", "session store"]
    many = [sq(f"rewrite {i}", "vector", i % 3) for i in range(40)]
    got = plan_query_texts(plan(many), "q")
    assert len(got) == 16 and got[0] == "q" and got[1:] == [f"rewrite {i}" for i in range(0, 40, 3)][:14] + ["rewrite 1"]
    assert plan_query_texts(NS(), "q") == ["q"]
