"""Score threshold and in-range counts above the device: the properties of the CPU restatement (tests/range_cases.py) that
DESIGN.md 3.18 states; the new C entry's export and argument checks; the store's ``score_threshold`` / ``search_range`` /
``count_similar`` on 1 and 2 local shards over a fake index; two gloo ranks agreeing on lists and counts; the searchers' and the
MCP tool's forwarding of ``min_score``; the refusals of combinations; calls without the new arguments unchanged."""
import asyncio
import os
import socket
import sys

import numpy as np
import pytest

from oracle import search as orc
from tests import range_cases
from tests.fake_index import fake_device
from tests.test_filter_sets_host import _corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, F32 = np.uint32, np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(U32)


# ------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("bf16", [False, True])
def test_restatement_prefix_monotone_and_inclusive(bf16):
    n, k, nq = 1500, 10, 32
    raw, codes, block = range_cases.corpus(n, 384)
    passing = (codes[:, 0] != 3)
    q, thr, scores, x_pre, (ws, wr, wc) = range_cases.batch(raw, block, nq, k, bf16, passing)
    assert set(range_cases.KINDS) <= range_cases.kinds_of(wc, k)                     # (what batch() asserted: no kind is missing)
    ps, pr = orc.search(x_pre, orc.preprocess(q, bf16), k, alive=passing.astype(np.uint8))
    for i in range(nq):                                                              # the list is a prefix of the plain top-k ...
        m = int(min(k, wc[i]))
        assert np.array_equal(wr[i, :m], pr[i, :m]) and np.array_equal(_bits(ws[i, :m]), _bits(ps[i, :m]))
        assert (wr[i, m:] == -1).all() and np.isneginf(ws[i, m:]).all()              # ... padded behind its last in-range entry
        assert wc[i] == int((passing & (scores[i] >= thr[i])).sum())                 # the count is the comparison, unclipped
    assert wc.max() > range_cases.MAX_K
    # monotone in the threshold: raising it can only shorten the list (a prefix again) and lower the count
    up = np.nextafter(thr, F32(4))
    s2, r2, c2 = range_cases.select(scores, up, k, passing)
    assert (c2 <= wc).all() and (c2 < wc).any()
    for i in range(nq):
        m = int(min(k, c2[i]))
        assert np.array_equal(r2[i, :m], wr[i, :m]) and (r2[i, m:] == -1).all()
    # ties are inclusive: at the block's exact score the whole block is in, one ulp above all of it is out
    b0, size = block
    at = scores[:, b0].copy()
    _, _, c_at = range_cases.select(scores, at, k, None)
    _, _, c_up = range_cases.select(scores, np.nextafter(at, F32(4)), k, None)
    assert (c_at - c_up == size).all() and size == range_cases.BLOCK
    one = range_cases.select(scores[:1], at[:1], n, None)
    rows = one[1][0, :c_at[0]]
    assert set(range(b0, b0 + size)) <= set(rows.tolist()) and (np.diff(rows[-size:]) == 1).all()   # equal scores: lower row first
    # row_base moves the rows of real entries only
    sb = range_cases.select(scores, thr, k, passing, row_base=1 << 32)
    assert np.array_equal(sb[1], np.where(wr >= 0, wr + (1 << 32), -1)) and np.array_equal(sb[2], wc)


def test_generator_refuses_a_degenerate_batch():
    raw, _, block = range_cases.corpus(400, 384)
    with pytest.raises(AssertionError, match="degenerate"):                          # five passing rows: no query can count k = 10
        range_cases.batch(raw, block, 16, 10, False, np.arange(400) < 5)
    q, thr, scores, _, want = range_cases.batch(raw, block, 16, 10, False)           # 400 rows cannot exceed CRH_MAX_K and are not asked to
    assert {"zero", "short", "full", "more"} <= range_cases.kinds_of(want[2], 10) and "huge" not in range_cases.kinds_of(want[2], 10)


# ------------------------------------------------------------------ ABI and binding
def test_new_entry_is_exported_and_checks_its_arguments():
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    L = ffi.lib()
    assert "crh_search_range" in ffi.EXPORTS and hasattr(L, "crh_search_range") and L.crh_abi_version() == 4
    thr = np.zeros((4,), F32)
    assert L.crh_search_range(None, 4, 16, 0, 10, thr.ctypes.data, None, 0, 0, 16, 16, None, 0, None) == ffi.E_INVALID      # no index
    assert b"NULL" in L.crh_last_error()
    for bad in (np.nan, np.inf, -np.inf, [0.1, np.nan]):
        with pytest.raises(ffi.NativeError, match="finite"):
            ffi.range_thresholds(bad, 2)
    with pytest.raises(ffi.NativeError, match="3 thresholds for 2"):
        ffi.range_thresholds([0.1, 0.2, 0.3], 2)
    assert ffi.range_thresholds(0.25, 3).tolist() == [0.25] * 3 and ffi.range_thresholds(np.float64(0.5), 0).shape == (0,)
    assert ffi.range_thresholds([0.1, 0.2], 2).dtype == F32


# ------------------------------------------------------------------ store plumbing over the fake index
def _fake_device(monkeypatch):
    ffi = fake_device(monkeypatch, range_cases.RangeFakeIndex)
    return ffi


def _pairs(hits):
    return [(h["id"], _bits(h["score"]).item()) for h in hits]


@pytest.mark.parametrize("shards", [1, 2])
def test_store_threshold_lists_counts_and_refusals(monkeypatch, shards):
    from coderag_amd.errors import VectorStoreError
    from coderag_amd.store import HipVectorStore
    _fake_device(monkeypatch)
    rng, vecs, payloads, ids = _corpus()
    vecs[200:220] = vecs[20]                                                         # 21 identical rows, spread over the upserts
    stored = orc.preprocess(vecs)
    qs = np.stack([vecs[20] + 0.4 * rng.standard_normal(768).astype(F32), rng.standard_normal(768).astype(F32)])
    scores = orc.scores(stored, orc.preprocess(qs))
    lang = np.asarray([p["language"] for p in payloads])
    proj = np.asarray([p["project_name"] for p in payloads])

    async def run():
        kw = {"shards": shards, "_merge_fn": orc.merge_topk} if shards > 1 else {}
        async with HipVectorStore(dim=768, dtype="f32", initial_capacity=512, device=0, compact_dead_fraction=0.0, **kw) as s:
            await s.create_collections()
            for a in range(0, 240, 60):
                await s.upsert("code_chunks", ids[a:a + 60], vecs[a:a + 60], payloads[a:a + 60])
            everything = [await s.search("code_chunks", q.tolist(), limit=240) for q in qs]
            thr = float(scores[0, 20])                                               # the duplicates' own score: inclusive

            def want(qi, t, limit, pred=None):
                return [(h["id"], _bits(h["score"]).item()) for h in everything[qi] if F32(h["score"]) >= F32(t) and (pred is None or pred(h["payload"]))][:limit]
            n_in = int((scores[0] >= F32(thr)).sum())
            assert 21 <= n_in < 60
            range_cases.RangeFakeIndex.range_calls.clear()
            before = s.search_passes
            got = await s.search("code_chunks", qs[0].tolist(), limit=100, score_threshold=thr)
            assert s.search_passes - before == 1 and _pairs(got) == want(0, thr, 100) and len(got) == n_in
            assert all(c == (1, 100, False) for c in range_cases.RangeFakeIndex.range_calls)              # list-only mode, one query
            assert _pairs(await s.search("code_chunks", qs[0].tolist(), limit=5, score_threshold=thr)) == want(0, thr, 5)
            up = float(np.nextafter(F32(thr), F32(4)))
            assert len(await s.search("code_chunks", qs[0].tolist(), limit=100, score_threshold=up)) == n_in - 21
            assert await s.search("code_chunks", qs[0].tolist(), limit=10, score_threshold=1.5) == []
            res = await s.search_range("code_chunks", qs[0].tolist(), thr, limit=4)
            assert set(res) == {"hits", "count"} and res["count"] == n_in and _pairs(res["hits"]) == want(0, thr, 4)
            assert all(set(h) == {"id", "score", "payload"} for h in res["hits"])
            assert await s.count_similar("code_chunks", qs[0].tolist(), thr) == n_in
            assert await s.count_similar("code_chunks", qs[0].tolist(), -2.0) == 240
            flt, mn = {"language": ["python", "go"]}, {"project_name": "p2"}
            ok = np.isin(lang, ["python", "go"]) & (proj != "p2")
            assert await s.count_similar("code_chunks", qs[1].tolist(), -0.01, filters=flt, must_not=mn) == int((ok & (scores[1] >= F32(-0.01))).sum())
            res = await s.search_range("code_chunks", qs[1].tolist(), -0.01, limit=6, filters=flt, must_not=mn)
            assert _pairs(res["hits"]) == want(1, -0.01, 6, lambda p: p["language"] in ("python", "go") and p["project_name"] != "p2")
            assert await s.search_range("code_chunks", qs[1].tolist(), 0.0, filters={"language": "cobol"}) == {"hits": [], "count": 0}
            both = await s.search_range_batch("code_chunks", qs, [thr, 0.0], limit=3)
            assert [b["count"] for b in both] == [n_in, int((scores[1] >= 0).sum())] and _pairs(both[1]["hits"]) == want(1, 0.0, 3)
            per = await s.search_batch("code_chunks", qs, limit=8, score_threshold=[thr, 0.05])
            assert [_pairs(p) for p in per] == [want(0, thr, 8), want(1, 0.05, 8)]
            one = await s.search_batch("code_chunks", qs, limit=8, score_threshold=0.05)
            assert [_pairs(p) for p in one] == [want(0, 0.05, 8), want(1, 0.05, 8)]
            # refusals: the store's usual argument error, for the caller alone
            q0 = qs[0].tolist()
            for call in (lambda: s.search("code_chunks", q0, score_threshold=0.1, diversity=0.5),
                         lambda: s.search("code_chunks", q0, score_threshold=0.1, group_by="file_path"),
                         lambda: s.search("code_chunks", q0, score_threshold=float("nan")),
                         lambda: s.search("code_chunks", q0, score_threshold=float("inf")),
                         lambda: s.search("code_chunks", None, score_threshold=0.1),
                         lambda: s.search("code_chunks", q0, limit=2000, score_threshold=0.1),
                         lambda: s.search_batch("code_chunks", qs, score_threshold=0.1, filters=[None, {"language": "go"}]),
                         lambda: s.search_batch("code_chunks", qs, score_threshold=[0.1, 0.2, 0.3]),
                         lambda: s.search_batch("code_chunks", qs, score_threshold=0.1, diversity=0.2),
                         lambda: s.search_fused("code_chunks", qs, score_threshold=0.1),
                         lambda: s.search_range("code_chunks", q0[:10], 0.1),
                         lambda: s.count_similar("code_chunks", q0, "high")):
                with pytest.raises(VectorStoreError) as e:
                    await call()
                assert isinstance(e.value.__cause__ or e.value.cause, ValueError), e.value
            # without the new argument: the plain pass, the plain entry of the index, coalesced as before
            range_cases.RangeFakeIndex.range_calls.clear()
            before = s.search_passes
            a, b = await asyncio.gather(s.search("code_chunks", qs[0].tolist(), limit=5), s.search("code_chunks", qs[1].tolist(), limit=5))
            assert s.search_passes - before == 1 and not range_cases.RangeFakeIndex.range_calls
            assert _pairs(a) == _pairs(everything[0][:5]) and _pairs(b) == _pairs(everything[1][:5])
            # thresholded calls never join the coalescer: each its own pass, the plain one beside them untouched
            before = s.search_passes
            a, b, c = await asyncio.gather(s.search("code_chunks", qs[0].tolist(), limit=5, score_threshold=thr),
                                           s.search("code_chunks", qs[0].tolist(), limit=5, score_threshold=thr),
                                           s.search("code_chunks", qs[0].tolist(), limit=5))
            assert s.search_passes - before == 3 and _pairs(a) == _pairs(b) == want(0, thr, 5) and _pairs(c) == _pairs(everything[0][:5])
    asyncio.run(run())


# ------------------------------------------------------------------ two ranks: the same lists, counts through one all-reduce
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
    from coderag_amd.shards import STRIDE, ShardSet
    from tests import range_cases as rc
    raw, _, block = rc.corpus(1300, 64)                                                # the same on every rank
    sh = ShardSet(world, lambda s: rc.RangeFakeIndex(dim=64, capacity_rows=2048, n_code_cols=1), backend="dist", block=50, merge_fn=orc.merge_topk)
    shard = sh.route(len(raw))
    sh.append({rank: raw[shard == rank]}, np.zeros((len(raw), 1), np.int32), shard=shard)
    gid = np.empty(len(raw), np.int64)
    for s in range(world):
        sel = np.flatnonzero(shard == s)
        gid[sel] = s * STRIDE + np.arange(sel.size)
    order = np.argsort(gid)                                                            # the collection in global-row order: ties go to the lower global row
    q, thr, _, _, _ = rc.batch(raw, block, 16, 10, False)
    scores = orc.scores(orc.preprocess(raw)[order], orc.preprocess(q))
    ws, wr, wc = rc.select(scores, thr, 10)
    for counts in (True, False):
        s_, shd, loc, c_ = sh.search_range(q, 10, thr, None, counts)
        got = np.where(loc >= 0, shd.astype(np.int64) * STRIDE + loc, -1)
        assert np.array_equal(got, np.where(wr >= 0, gid[order][np.maximum(wr, 0)], -1)) and np.array_equal(_bits(s_), _bits(ws)), f"rank {rank}"
        assert (c_ is None) if not counts else np.array_equal(c_, wc), f"rank {rank}: counts"
    assert wc.max() > rc.MAX_K and wc.min() == 0
    np.save(os.path.join(out_dir, f"rows{rank}.npy"), got)
    np.save(os.path.join(out_dir, f"counts{rank}.npy"), np.asarray(wc))
    dist.destroy_process_group()


def test_two_gloo_ranks_agree_on_lists_and_counts(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_gloo_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    assert sorted(os.listdir(tmp_path)) == ["counts0.npy", "counts1.npy", "rows0.npy", "rows1.npy"]
    for name in ("rows", "counts"):
        assert np.load(os.path.join(tmp_path, f"{name}0.npy")).tobytes() == np.load(os.path.join(tmp_path, f"{name}1.npy")).tobytes()


# ------------------------------------------------------------------ searchers and the MCP tool
class _Recorder:
    def __init__(self, hits=()):
        self.calls, self.hits = [], list(hits)

    async def search(self, **kw):
        self.calls.append(("search", kw))
        return self.hits

    async def search_batch(self, **kw):
        self.calls.append(("search_batch", kw))
        return [self.hits for _ in range(len(kw["query_vectors"]))]


class _Embedder:
    async def embed(self, text):
        return [0.0] * 4

    async def embed_batch(self, texts):
        return [[0.0] * 4 for _ in texts]


def test_searchers_and_tool_forward_min_score_only_when_given():
    from coderag_amd import indexer, mcp_tools, vector_search

    async def run():
        rec = _Recorder()
        vs = vector_search.VectorSearcher(rec, _Embedder())
        await vs.search_code("q", limit=3, language="python")
        await vs.search_summaries("q", limit=3)
        await vs.find_similar_code("def f(): pass", limit=3)
        await vs.search_code_batch(["a", "b"], limit=3)
        assert [set(kw) for _, kw in rec.calls] == [{"collection", "query_vector", "limit", "filters"}] * 2 + \
            [{"collection", "query_vector", "limit"}, {"collection", "query_vectors", "limit", "filters"}]      # today's call shapes
        rec.calls.clear()
        await vs.search_code("q", limit=3, min_score=0.4)
        await vs.search_summaries("q", limit=3, min_score=0.5)
        await vs.find_similar_code("def f(): pass", limit=3, exclude_file="a.py", min_score=0.6)
        await vs.search_code_batch(["a", "b"], limit=3, min_score=[0.1, 0.2])
        assert [kw["score_threshold"] for _, kw in rec.calls] == [0.4, 0.5, 0.6, [0.1, 0.2]]
        assert rec.calls[2][1]["limit"] == 3 + vector_search.EXCLUDE_FILE_BUFFER
        with pytest.raises(ValueError, match="extra_queries"):
            await vs.search_code("q", extra_queries=["q2"], min_score=0.3)
        rec.calls.clear()
        dc = indexer.VectorSearcher(rec, _Embedder())
        await dc.search_code("q", limit=3)
        await dc.search_summaries("q", limit=3)
        await dc.search_code("q", limit=3, min_score=0.7)
        await dc.search_summaries("q", limit=3, min_score=0.0)
        assert ["score_threshold" in kw for _, kw in rec.calls] == [False, False, True, True]
        assert rec.calls[2][1]["score_threshold"] == 0.7 and rec.calls[3][1]["score_threshold"] == 0.0          # (0.0 is a threshold, not "unset")

        class Searcher:
            def __init__(self, n):
                self.kw, self.n = [], n

            async def search_code(self, **kw):
                self.kw.append(kw)
                return [{"entity_name": f"e{i}", "entity_type": "function", "file_path": "f.py", "score": 0.9} for i in range(self.n)]
        sr = Searcher(2)
        tool = mcp_tools.create_semantic_search_tool(lambda: sr)
        plain = await tool["function"]("find it")
        short = await tool["function"]("find it", min_score=0.5)
        assert sr.kw == [{"query": "find it", "limit": 5, "entity_type": None}, {"query": "find it", "limit": 5, "entity_type": None, "min_score": 0.5}]
        assert plain.message == "Found 2 matches for 'find it'." and short.success and len(short.data) == 2
        assert "only 2 rows score at least 0.5" in short.message                           # fewer than `limit`: the list is every row in range
        full = await tool["function"]("find it", limit=2, min_score=0.5)
        assert full.message == "Found 2 matches for 'find it'." and "min_score" in tool["parameters"]
    asyncio.run(run())
