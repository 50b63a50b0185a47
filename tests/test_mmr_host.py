"""Diversity-aware top-k (MMR) above the device: the CPU restatement (tests/mmr_cases.py) against an fp64 greedy and its two
properties; the new C entries' exports and argument checks; the store's plumbing on 1 and 2 local shards over a fake index
with ``ffi.mmr_select`` replaced by the restatement; the zero-fill-and-sum completion of the candidate vectors over two gloo
ranks; the searchers' and the MCP tool's forwarding of the keywords."""
import asyncio
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest

from oracle import search as orc
from tests import mmr_cases
from tests.fake_index import fake_device
from tests.test_filter_sets_host import SetFakeIndex, _corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class MmrFakeIndex(SetFakeIndex):
    """SetFakeIndex that counts the ``gather_vectors`` calls (the gather itself is ``FakeIndex``'s)."""
    gathers = 0

    def gather_vectors(self, *args, **kw):
        MmrFakeIndex.gathers += 1
        return super().gather_vectors(*args, **kw)


# ------------------------------------------------------------------ the restatement itself
def test_restatement_matches_fp64_greedy_on_separated_objectives():
    x = mmr_cases.random_rows(400, 384, seed=1, bf16=False)
    q = mmr_cases.random_rows(3, 384, seed=2, bf16=False)
    scores, rows, vecs = mmr_cases.candidate_lists(x, q, 48)
    for d in (0.0, 0.3, 0.7, 1.0):
        pos, r, s, obj = mmr_cases.mmr_select(scores, rows, vecs, 12, d)
        for qi in range(3):
            assert pos[qi].tolist() == mmr_cases.mmr_fp64(scores[qi], rows[qi], vecs[qi], 12, d), (d, qi)
            assert np.array_equal(r[qi], rows[qi][pos[qi]]) and np.array_equal(s[qi], scores[qi][pos[qi]])
            assert obj[qi, 0] == np.float32(np.float32(1.0) - np.float32(d)) * scores[qi, 0]
    assert np.array_equal(mmr_cases.canonical_sims(vecs[0], vecs[0, 5]),
                          np.asarray([orc.dot(v, vecs[0, 5]) for v in vecs[0]], np.float32))       # the oracle's chain, either way


def test_restatement_properties_diversity_zero_prefix_stability_padding():
    raw, which, q = mmr_cases.clustered(dim=384)
    x = orc.preprocess(raw, to_bf16=True)
    scores, rows, vecs = mmr_cases.candidate_lists(x, orc.preprocess(q[None], to_bf16=True), 64)
    pos, r, s, obj = mmr_cases.mmr_select(scores, rows, vecs, 10, 0.0)
    assert pos[0].tolist() == list(range(10)) and np.array_equal(r[0], rows[0, :10])
    assert np.array_equal(s.view(np.uint32), scores[:, :10].view(np.uint32)) and np.array_equal(obj.view(np.uint32), s.view(np.uint32))
    full = mmr_cases.mmr_select(scores, rows, vecs, 24, 0.5)
    for j in (1, 5, 24):
        part = mmr_cases.mmr_select(scores, rows, vecs, j, 0.5)
        for a, b in zip(part, full):
            assert np.array_equal(a, b[:, :j])
    plain, picked = set(which[rows[0, :10]]), set(which[full[1][0, :10]])
    assert len(picked) > len(plain)                                            # the clustered set: MMR names more centres
    # fewer real candidates than k; an all-padding list
    scores, rows, vecs = mmr_cases.candidate_lists(x, orc.preprocess(q[None], to_bf16=True), 16, real=5)
    pos, r, s, obj = mmr_cases.mmr_select(scores, rows, vecs, 8, 0.5)
    assert sorted(pos[0, :5].tolist()) == [0, 1, 2, 3, 4] and pos[0, 5:].tolist() == [-1] * 3 and r[0, 5:].tolist() == [-1] * 3
    assert np.isneginf(s[0, 5:]).all() and np.isneginf(obj[0, 5:]).all()
    pos, r, s, obj = mmr_cases.mmr_select(np.full((1, 4), -np.inf, np.float32), np.full((1, 4), -1), np.zeros((1, 4, 384), np.float32), 4, 0.5)
    assert pos.tolist() == [[-1] * 4] and r.tolist() == [[-1] * 4] and np.isneginf(s).all() and np.isneginf(obj).all()


# ------------------------------------------------------------------ ABI
def test_new_entries_are_exported_and_check_their_arguments():
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    L = ffi.lib()
    for name in ("crh_index_gather_vectors", "crh_mmr_select"):
        assert name in ffi.EXPORTS and hasattr(L, name)
    assert L.crh_abi_version() == 4
    assert L.crh_index_gather_vectors(None, 1, None, 0, None, None) == ffi.E_INVALID and b"NULL" in L.crh_last_error()
    one = 16   # (a non-NULL, never dereferenced pointer: every case below is refused before a launch)
    for nq, c, k, dim, d, word in ((1, 8, 0, 768, 0.5, b"k="), (1, 8, 9, 768, 0.5, b"k="), (1, 2048, 8, 768, 0.5, b"c="), (-1, 8, 8, 768, 0.5, b"nq="),
                                   (1, 8, 8, 100, 0.5, b"dim"), (1, 8, 8, 768, -0.1, b"diversity"), (1, 8, 8, 768, 1.5, b"diversity"),
                                   (1, 8, 8, 768, float("nan"), b"diversity")):
        assert L.crh_mmr_select(nq, c, k, dim, one, one, one, d, one, one, one, one, None) == ffi.E_INVALID, (nq, c, k, dim, d)
        assert word in L.crh_last_error()
    assert L.crh_mmr_select(1, 8, 8, 768, None, None, None, 0.5, None, None, None, None, None) == ffi.E_INVALID and b"NULL" in L.crh_last_error()
    assert L.crh_mmr_select(0, 8, 8, 768, None, None, None, 0.5, None, None, None, None, None) == ffi.OK       # nothing to do
    with pytest.raises(ffi.NativeError, match="device tensor"):
        ffi.mmr_select(np.zeros((1, 4), np.float32), np.zeros((1, 4), np.int64), np.zeros((1, 4, 768), np.float32), 2, 0.5)


# ------------------------------------------------------------------ store plumbing over the fake index
def _fake_device(monkeypatch):
    ffi = fake_device(monkeypatch, MmrFakeIndex)
    monkeypatch.setattr(ffi, "mmr_select", mmr_cases.mmr_select)
    return ffi


def _expected(everything, vec_of, pred, limit, candidates, diversity):
    """The restatement on the host: the ``candidates`` best hits passing ``pred`` (from a plain search of the whole
    collection), their stored rows, greedy picks -> [(id, score)]."""
    cand = [h for h in everything if pred(h["payload"])][:candidates]
    if not cand:
        return []
    c = max(candidates, 1)
    scores, rows = np.full((1, c), -np.inf, np.float32), np.full((1, c), -1, np.int64)
    vecs = np.zeros((1, c, 768), np.float32)
    for i, h in enumerate(cand):
        scores[0, i], rows[0, i], vecs[0, i] = h["score"], i, vec_of[h["id"]]
    pos, _, s, _ = mmr_cases.mmr_select(scores, rows, vecs, limit, diversity)
    return [(cand[p]["id"], float(sc)) for p, sc in zip(pos[0], s[0]) if p >= 0]


@pytest.mark.parametrize("shards", [1, 2])
def test_store_search_with_diversity(monkeypatch, shards):
    from coderag_amd.errors import VectorStoreError
    from coderag_amd.store import HipVectorStore
    ffi = _fake_device(monkeypatch)
    rng, vecs, payloads, ids = _corpus()
    vecs[200:240] = vecs[0:40] + 1e-4 * rng.standard_normal((40, 768)).astype(np.float32)     # near-duplicates of the first rows
    vecs[40:60] = vecs[0:20]                                                                   # and exact ones
    q = (vecs[3] + vecs[7] + 0.5 * vecs[90]).astype(np.float32)
    vec_of = dict(zip(ids, orc.preprocess(vecs)))

    def pairs(hits):
        return [(h["id"], h["score"]) for h in hits]

    async def run():
        kw = {"shards": shards, "_merge_fn": orc.merge_topk} if shards > 1 else {}
        async with HipVectorStore(dim=768, dtype="f32", initial_capacity=512, device=0, compact_dead_fraction=0.0, **kw) as s:
            await s.create_collections()
            for a in range(0, 240, 60):                                   # four appends: the blocks go round the shards
                await s.upsert("code_chunks", ids[a:a + 60], vecs[a:a + 60], payloads[a:a + 60])
            col = s._col("code_chunks")
            assert all(r > 0 for r in col.shards.rows)
            everything = await s.search("code_chunks", q.tolist(), limit=240)
            assert len(everything) == 240
            plain10 = await s.search("code_chunks", q.tolist(), limit=10)
            # diversity=None: the plain path, no gather
            MmrFakeIndex.gathers = 0
            assert pairs(await s.search("code_chunks", q.tolist(), limit=10, diversity=None)) == pairs(plain10) and MmrFakeIndex.gathers == 0
            # diversity = 0: the prefix; default candidates = 4 * limit
            assert pairs(await s.search("code_chunks", q.tolist(), limit=10, diversity=0.0)) == pairs(plain10)
            got = await s.search("code_chunks", q.tolist(), limit=10, diversity=0.5)
            assert MmrFakeIndex.gathers == 2 * shards
            assert pairs(got) == _expected(everything, vec_of, lambda p: True, 10, 40, 0.5) and pairs(got) != pairs(plain10)
            assert all(set(h) == {"id", "score", "payload"} for h in got)
            by_id = {h["id"]: h for h in everything}
            assert all(h["score"] == by_id[h["id"]]["score"] and h["payload"] == by_id[h["id"]]["payload"] for h in got)   # score = cosine
            # filters and must_not combined with diversity; explicit candidates
            got = await s.search("code_chunks", q.tolist(), limit=8, filters={"language": ["python", "go"]}, must_not={"file_path": "/proj/f3.py"},
                                 diversity=0.7, candidates=30)
            assert pairs(got) == _expected(everything, vec_of, lambda p: p["language"] in ("python", "go") and p["file_path"] != "/proj/f3.py", 8, 30, 0.7)
            # fewer matching rows than candidates, and than limit
            few = lambda p: p["file_path"] == "/proj/f5.py" and p["project_name"] == "p3"      # noqa: E731
            n_few = sum(1 for h in everything if few(h["payload"]))
            assert 0 < n_few < 8
            got = await s.search("code_chunks", q.tolist(), limit=8, filters={"file_path": "/proj/f5.py", "project_name": "p3"}, diversity=0.5)
            assert len(got) == n_few and pairs(got) == _expected(everything, vec_of, few, 8, 32, 0.5)
            assert await s.search("code_chunks", q.tolist(), limit=5, filters={"language": "cobol"}, diversity=0.5) == []
            # the batched form, per query
            qs = np.stack([q, vecs[100], vecs[150]])
            batch = await s.search_batch("code_chunks", qs, limit=6, diversity=0.4, candidates=24)
            for qi in range(3):
                every_q = await s.search("code_chunks", qs[qi].tolist(), limit=240)
                assert pairs(batch[qi]) == _expected(every_q, vec_of, lambda p: True, 6, 24, 0.4)
            assert pairs((await s.search_batch("code_chunks", q[None], limit=10))[0]) == pairs(plain10)
            # a bad value fails its own caller only
            good = s.search("code_chunks", q.tolist(), limit=10, diversity=0.5)
            bad = [s.search("code_chunks", q.tolist(), limit=10, diversity=1.5), s.search("code_chunks", q.tolist(), limit=10, diversity=float("nan")),
                   s.search("code_chunks", q.tolist(), limit=10, diversity=0.5, candidates=5),
                   s.search("code_chunks", q.tolist(), limit=10, diversity=0.5, candidates=ffi.MAX_K + 1),
                   s.search("code_chunks", q.tolist(), limit=10, candidates=50)]
            res = await asyncio.gather(good, *bad, return_exceptions=True)
            assert pairs(res[0]) == _expected(everything, vec_of, lambda p: True, 10, 40, 0.5)
            assert all(isinstance(r, VectorStoreError) for r in res[1:])
            with pytest.raises(VectorStoreError):
                await s.search_batch("code_chunks", q[None], limit=10, diversity=-0.5)
            # coalescing: equal (diversity, candidates) share ONE pass at the largest limit, each caller keeps its prefix; a plain
            # call beside them is a pass of its own, and so is another diversity
            before = s.search_passes
            a, b, c, d = await asyncio.gather(s.search("code_chunks", q.tolist(), limit=4, diversity=0.5, candidates=40),
                                              s.search("code_chunks", vecs[100].tolist(), limit=10, diversity=0.5, candidates=40),
                                              s.search("code_chunks", q.tolist(), limit=10),
                                              s.search("code_chunks", q.tolist(), limit=4, diversity=0.25, candidates=40))
            assert s.search_passes - before == 3
            want = _expected(everything, vec_of, lambda p: True, 10, 40, 0.5)
            assert pairs(a) == want[:4] and pairs(c) == pairs(plain10)
            assert pairs(b) == _expected(await s.search("code_chunks", vecs[100].tolist(), limit=240), vec_of, lambda p: True, 10, 40, 0.5)
            assert pairs(d) == _expected(everything, vec_of, lambda p: True, 4, 40, 0.25)

    asyncio.run(run())


# ------------------------------------------------------------------ two ranks: zero fill + one all-reduce(sum)
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
    from tests import mmr_cases
    from tests.test_mmr_host import MmrFakeIndex
    ffi.mmr_select = mmr_cases.mmr_select
    raw, which, q = mmr_cases.clustered(dim=384)                       # the same on every rank
    sh = ShardSet(world, lambda s: MmrFakeIndex(dim=384, capacity_rows=1024), backend="dist", block=50, merge_fn=orc.merge_topk)
    shard = sh.route(len(raw))
    sh.append({rank: raw[shard == rank]}, None, shard=shard)
    assert all(r > 0 for r in sh.rows) and sh.index[rank].count()[0] == sh.rows[rank]
    x = orc.preprocess(raw)
    gid = np.empty(len(raw), np.int64)                                  # global row of every input row
    for s in range(world):
        sel = np.flatnonzero(shard == s)
        gid[sel] = s * STRIDE + np.arange(sel.size)
    scores, sshard, local = sh.search_mmr(q[None], 10, 64, 0.5, None)
    # the flat restatement: candidates by the oracle over the whole corpus, ties by lower GLOBAL row as the merge orders them
    order = np.argsort(gid)
    cs, cr, cv = mmr_cases.candidate_lists(x[order], orc.preprocess(q[None]), 64)
    pos, er, es, _ = mmr_cases.mmr_select(cs, cr, cv, 10, 0.5)
    exp_gid = gid[order][er[0]]
    assert np.array_equal(scores.view(np.uint32), es.view(np.uint32)), f"rank {rank}: scores differ"
    assert np.array_equal(sshard[0].astype(np.int64) * STRIDE + local[0], exp_gid), f"rank {rank}: picks differ"
    assert len(set(which[order][er[0]])) > len(set(which[order][cr[0, :10]]))
    open(os.path.join(out_dir, f"ok{rank}"), "w").write("ok")
    dist.destroy_process_group()


def test_candidate_vectors_complete_over_two_gloo_ranks(tmp_path):
    import torch.multiprocessing as mp
    port = _free_port()
    mp.spawn(_gloo_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert sorted(os.listdir(tmp_path)) == ["ok0", "ok1"]


# ------------------------------------------------------------------ searchers and the MCP tool
class _Recorder:
    def __init__(self):
        self.calls = []

    async def search(self, **kw):
        self.calls.append(("search", kw))
        return []

    async def search_batch(self, **kw):
        self.calls.append(("search_batch", kw))
        return [[] for _ in kw["query_vectors"]]


class _Embedder:
    async def embed(self, text):
        return [0.0] * 4

    async def embed_batch(self, texts):
        return [[0.0] * 4 for _ in texts]


def test_searchers_forward_the_keywords_only_when_given():
    from coderag_amd import indexer, mcp_tools, vector_search

    async def run():
        for cls in (vector_search.VectorSearcher, indexer.VectorSearcher):
            rec = _Recorder()
            vs = cls(rec, _Embedder())
            await vs.search_code("q", limit=3, language="python")
            await vs.search_summaries("q", limit=3)
            assert [set(kw) for _, kw in rec.calls] == [{"collection", "query_vector", "limit", "filters"}] * 2       # today's call shape
            rec.calls.clear()
            await vs.search_code("q", limit=3, diversity=0.5)
            await vs.search_summaries("q", limit=3, diversity=0.25, candidates=50)
            assert rec.calls[0][1]["diversity"] == 0.5 and "candidates" not in rec.calls[0][1]
            assert (rec.calls[1][1]["diversity"], rec.calls[1][1]["candidates"]) == (0.25, 50)
        rec = _Recorder()
        vs = vector_search.VectorSearcher(rec, _Embedder())
        await vs.find_similar_code("x = 1", limit=3)
        await vs.search_code_batch(["a", "b"], limit=3)
        assert set(rec.calls[0][1]) == {"collection", "query_vector", "limit"} and set(rec.calls[1][1]) == {"collection", "query_vectors", "limit", "filters"}
        rec.calls.clear()
        await vs.find_similar_code("x = 1", limit=3, exclude_file="a.py", exact_exclude=True, diversity=0.5, candidates=12)
        await vs.search_code_batch(["a", "b"], limit=3, diversity=0.5)
        assert rec.calls[0][1]["must_not"] == {"file_path": "a.py"} and (rec.calls[0][1]["diversity"], rec.calls[0][1]["candidates"]) == (0.5, 12)
        assert rec.calls[1][1]["diversity"] == 0.5 and "candidates" not in rec.calls[1][1]

        class Searcher:
            def __init__(self):
                self.kw = []

            async def search_code(self, **kw):
                self.kw.append(kw)
                return []
        sr = Searcher()
        tool = mcp_tools.create_semantic_search_tool(lambda: sr)
        assert (await tool["function"]("find it")).success and (await tool["function"]("find it", limit=3, diversity=0.5)).success
        assert sr.kw == [{"query": "find it", "limit": 5, "entity_type": None}, {"query": "find it", "limit": 3, "entity_type": None, "diversity": 0.5}]
        assert {"diversity", "candidates"} <= set(tool["parameters"])

    asyncio.run(run())
