"""Facets above the device: the new C entries' export and argument checks; the restatement's own properties;
``ShardSet.facet`` and the store's ``facet`` / ``facet_batch`` on 1 and 3 local shards over a fake index -- through delete,
upsert-replace, ``compact()`` and ``save()`` / ``load()``, against a model that never reads the store --; two gloo ranks agreeing
on one all-reduced histogram; the raw client, the searcher and the MCP tool."""
import asyncio
import os
import socket
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest

from oracle import search as orc
from tests import facet_cases as fc
from tests.fake_index import fake_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("crh_index_facet", "crh_search_range_facet", "crh_facet_select")


# ------------------------------------------------------------------ the C surface
def test_new_entries_are_exported_and_check_their_arguments():
    import subprocess
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    L = ffi.lib()
    header = open(os.path.join(ROOT, "include", "coderag_hip.h")).read()
    for path in (ffi.LIB_PATH, ffi.DEBUG_LIB_PATH):
        names = subprocess.check_output(["nm", "-D", "--defined-only", str(path)]).decode()
        for name in NEW:
            assert name in ffi.EXPORTS and hasattr(L, name) and f" T {name}\n" in names and f"int {name}(" in header, (path, name)
    assert L.crh_abi_version() == 4 == ffi.ABI_VERSION and f"#define CRH_FACET_LDS_BINS {ffi.FACET_LDS_BINS}" in header
    # refused before any device is touched
    buf = np.zeros((16,), np.int64)
    p = buf.ctypes.data
    assert L.crh_index_facet(None, 0, None, 0, 4, p, p, None) == ffi.E_INVALID and b"NULL" in L.crh_last_error()
    q, t = np.zeros((1, 384), np.float32), np.zeros((1,), np.float32)
    assert L.crh_search_range_facet(None, 1, q.ctypes.data, 0, t.ctypes.data, None, 0, 0, 4, p, p, None) == ffi.E_INVALID
    for nq, n_bins, k in ((-1, 4, 2), (1, 0, 2), (1, 4, 0), (1, 4, ffi.MAX_K + 1)):
        assert L.crh_facet_select(nq, n_bins, k, p, p, p, p, None) == ffi.E_INVALID and b"facet_select" in L.crh_last_error()
    assert L.crh_facet_select(1, 4, 2, None, p, p, p, None) == ffi.E_INVALID and b"NULL" in L.crh_last_error()
    assert L.crh_facet_select(0, 4, 2, None, None, None, None, None) == ffi.OK                       # no list: nothing to do
    with pytest.raises(ffi.NativeError, match="device tensor"):
        ffi.facet_select(np.zeros((1, 4), np.int64), 2)


def test_the_restatement_orders_ties_by_code_and_keeps_the_prefix():
    bins = np.asarray([[0, 5, 2, 5, 0, 2, 9, 2], [0, 0, 0, 0, 0, 0, 0, 0]], np.int64)
    codes, counts, info = fc.facet_list(bins, 4)
    assert codes.tolist() == [[6, 1, 3, 2], [-1] * 4] and counts.tolist() == [[9, 5, 5, 2], [0] * 4] and info.tolist() == [[6, 25], [0, 0]]
    for j in (1, 2, 3):
        assert np.array_equal(fc.facet_list(bins, j)[0], codes[:, :j])
    assert fc.facet_list(bins, 10)[0][0].tolist() == [6, 1, 3, 2, 5, 7, -1, -1, -1, -1]             # fewer non-zero bins than k
    b, i = fc.histogram(np.asarray([3, -1, 0, 7, 3, 9, 3]), np.asarray([1, 1, 1, 1, 0, 1, 1], bool), 8)
    assert b.tolist() == [1, 0, 0, 2, 0, 0, 0, 1] and i.tolist() == [6, 1, 1] and b.sum() + i[1] + i[2] == i[0]
    for name in fc.GENERATORS:                                                                      # every generator, -1 sprinkled in
        c = fc.codes_for(name, 700)
        assert c.shape == (700,) and c.dtype == np.int32 and (c == -1).sum() > 32 and c.max() >= 0
    edges = np.flatnonzero(np.diff(fc.codes_for("runs", 3000, sprinkle=False))) + 1
    assert {31, 0, 1} == set((edges % 32).tolist()) and {63, 0, 1} <= set(edges % 64) and {255, 0, 1} <= set(edges % 256)


# ------------------------------------------------------------------ the shard set over fake indexes
def _fake(monkeypatch):
    return fake_device(monkeypatch, fc.FacetFakeIndex, Text=fc.FakeText, facet_select=fc.np_facet_select)


@pytest.mark.parametrize("ns", [1, 3])
def test_shard_set_sums_the_shards_and_selects_once(monkeypatch, ns):
    ffi = _fake(monkeypatch)
    from coderag_amd.shards import ShardSet
    n, dim = 900, 64
    rng = np.random.default_rng(ns)
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    codes = np.stack([fc.codes_for("files", n), np.arange(n) % 7], 1).astype(np.int32)
    sh = ShardSet(ns, lambda s: fc.FacetFakeIndex(dim=dim, capacity_rows=1024, n_code_cols=2), block=40, merge_fn=orc.merge_topk)
    shard, local = sh.append(raw, codes)
    dead = np.arange(3, n, 17)
    sh.tombstone(shard[dead], local[dead])
    alive = np.ones((n,), bool)
    alive[dead] = False
    n_bins = int(codes[:, 0].max()) + 1
    for filt, passing in ((None, alive), ([(1, [2, 5])], alive & np.isin(codes[:, 1], [2, 5]))):
        got = sh.facet(filt, 0, n_bins, 12)
        bins, info = fc.histogram(codes[:, 0], passing, n_bins)
        want = fc.facet_list(bins, 12)
        assert all(np.array_equal(g, w) for g, w in zip(got[:3], want)) and got[3].tolist() == [info.tolist()]
        assert got[2][0, 1] + info[1] + info[2] == sh.count_matching(filt)                         # the sum invariant
    q = rng.standard_normal((5, dim)).astype(np.float32)
    scores = orc.scores(orc.preprocess(raw), orc.preprocess(q))
    thr = np.asarray([-2.0, 0.1, np.sort(scores[2])[-30], 2.0, 0.0], np.float32)
    got = sh.facet(None, 0, n_bins, 6, q, thr)
    bins, info = fc.histograms(codes[:, 0], scores, thr, alive, n_bins)
    assert all(np.array_equal(g, w) for g, w in zip(got[:3], fc.facet_list(bins, 6))) and np.array_equal(got[3], info)
    assert np.array_equal(info[:, 0], sh.search_range(q, 1, thr, None)[3]) and info[0, 0] == alive.sum() and info[3, 0] == 0
    with pytest.raises(ValueError, match=rf"{ffi.FACET_MAX_ENTRIES // 1024 + 1} queries x 1024"):
        sh.facet(None, 0, 1024, 5, np.zeros((ffi.FACET_MAX_ENTRIES // 1024 + 1, dim), np.float32), 0.0)


# ------------------------------------------------------------------ the store: every step of the life-cycle against the model
@pytest.mark.parametrize("shards", [1, 3])
def test_store_facets_through_the_life_cycle(monkeypatch, tmp_path, shards):
    from coderag_amd.errors import VectorStoreError
    from coderag_amd.store import HipVectorStore
    _fake(monkeypatch)

    def make_store():
        kw = {"shards": shards, "_merge_fn": orc.merge_topk} if shards > 1 else {}
        return HipVectorStore(dim=fc.SCRIPT_DIM, dtype="f32", initial_capacity=256, device=0, compact_dead_fraction=0.0, **kw)
    fc.FacetFakeIndex.facet_calls.clear()
    out = asyncio.run(fc.store_script(make_store, fc.FacetModel(), str(tmp_path)))
    assert len(out) == 4 * 14
    kinds = {c[0] for c in fc.FacetFakeIndex.facet_calls}
    assert kinds == {"facet", "range"}
    # what the script's data promises: ties at the cut, rows without the key, a value only replacements carry
    filled = out["filled: language"]
    assert filled["hits"][0]["value"] == "python" and None in [h["value"] for h in filled["hits"]] and filled["total"] == 600 and filled["missing"] == 0
    assert len({h["count"] for h in out["filled: files top 10"]["hits"]}) == 1 and out["filled: files all"]["values"] == 75
    assert [h["value"] for h in out["filled: files top 3"]["hits"]] == ["/proj/f0.py", "/proj/f1.py", "/proj/f2.py"]     # equal counts: stored first
    assert "zig" in [h["value"] for h in out["compacted: language"]["hits"]] and "go" not in [h["value"] for h in out["compacted: language"]["hits"]]
    assert out["filled: never stored"] == {"hits": [], "values": 0, "total": 0, "missing": 0}
    assert out["filled: files near the block"]["total"] >= 40 and out["compacted: files near the block"]["total"] < out["filled: files near the block"]["total"]
    assert out["loaded: batch"] == out["compacted: batch"] and out["loaded: files holding TODO("] == out["compacted: files holding TODO("]

    async def refusals():
        async with make_store() as s:
            await s.create_collections()
            ids, pays = zip(*(fc.point(i) for i in range(40)))
            await s.upsert("code_chunks", list(ids), fc.script_vectors()[0][:40], list(pays))
            q = [0.0] * fc.SCRIPT_DIM
            for call, word in ((lambda: s.facet("code_chunks", "start_line"), "filterable: file_path"),
                               (lambda: s.facet("code_chunks", "graph_node_id"), "filterable: file_path"),
                               (lambda: s.facet("code_chunks", "language", limit=0), "limit"),
                               (lambda: s.facet("code_chunks", "language", limit=1025), "limit"),
                               (lambda: s.facet("code_chunks", "language", query_vector=q), "come together"),
                               (lambda: s.facet("code_chunks", "language", score_threshold=0.5), "come together"),
                               (lambda: s.facet("code_chunks", "language", query_vector=q, score_threshold=float("nan")), "finite"),
                               (lambda: s.facet("code_chunks", "language", query_vector=q[:7], score_threshold=0.1), "dim"),
                               (lambda: s.facet("code_chunks", "language", filters=[None]), "per-query"),
                               (lambda: s.facet("code_chunks", "language", filters={"entity_name": {"contains": "x"}}), "text"),
                               (lambda: s.facet_batch("code_chunks", "language", [q, q], [0.1, 0.2, 0.3]), "thresholds"),
                               (lambda: s.facet_batch("code_chunks", "language", None, 0.1), "facet_batch needs")):
                with pytest.raises(VectorStoreError) as e:
                    await call()
                cause = e.value.__cause__ or e.value.cause
                assert isinstance(cause, ValueError) and word in str(cause), (word, cause)
            # the raw client: Qdrant's FacetResponse shape, the filter through the client's own translation
            flt = NS(must=[NS(key="language", match=NS(value=None, text=None, any=["python", "rust"], except_=None), range=None)],
                     must_not=[NS(key="start_line", match=None, range=NS(gte=20, gt=None, lte=None, lt=None))])
            res = await s.client.facet("code_chunks", "entity_type", facet_filter=flt, limit=2)
            want = (await s.facet("code_chunks", "entity_type", 2, {"language": ["python", "rust"]}, {"start_line": {"gte": 20}}))["hits"]
            assert [(h.value, h.count) for h in res.hits] == [(h["value"], h["count"]) for h in want] and len(want) == 2
            assert [h.count for h in (await s.client.facet("code_chunks", "file_path")).hits] == [8] * 5
            with pytest.raises(ValueError, match="filterable"):
                await s.client.facet("code_chunks", "end_line")
            with pytest.raises(ValueError, match="cannot evaluate"):
                await s.client.facet("code_chunks", "language", facet_filter=NS(must=[NS(key="graph_node_id", match=NS(value="mod.ent1", text=None, any=None, except_=None), range=None)], must_not=None))
    asyncio.run(refusals())


# ------------------------------------------------------------------ two ranks: one histogram through one all-reduce
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
    from coderag_amd.shards import ShardSet
    from tests import facet_cases as cases, range_cases as rc
    ffi.facet_select = cases.np_facet_select
    raw, _, block = rc.corpus(1300, 64)                                                # the same on every rank
    codes = np.stack([cases.codes_for("files", len(raw)), np.arange(len(raw)) % 5], 1).astype(np.int32)
    sh = ShardSet(world, lambda s: cases.FacetFakeIndex(dim=64, capacity_rows=2048, n_code_cols=2), backend="dist", block=50, merge_fn=orc.merge_topk)
    shard = sh.route(len(raw))
    sh.append({rank: raw[shard == rank]}, codes, shard=shard)
    n_bins = int(codes[:, 0].max()) + 1
    q, thr, scores, _, _ = rc.batch(raw, block, 16, 10, False)
    got = sh.facet([(1, [1, 2, 4])], 0, n_bins, 9)
    bins, info = cases.histogram(codes[:, 0], np.isin(codes[:, 1], [1, 2, 4]), n_bins)
    assert all(np.array_equal(g, w) for g, w in zip(got[:3], cases.facet_list(bins, 9))) and got[3][0].tolist() == info.tolist(), f"rank {rank}"
    sem = sh.facet(None, 0, n_bins, 9, q, thr)
    bins, info = cases.histograms(codes[:, 0], scores, thr, None, n_bins)
    assert all(np.array_equal(g, w) for g, w in zip(sem[:3], cases.facet_list(bins, 9))) and np.array_equal(sem[3], info), f"rank {rank}"
    assert info[:, 0].max() > rc.MAX_K and info[:, 0].min() == 0
    np.save(os.path.join(out_dir, f"plain{rank}.npy"), got[1])
    np.save(os.path.join(out_dir, f"semantic{rank}.npy"), sem[1])
    dist.destroy_process_group()


def test_two_gloo_ranks_agree_on_the_facets(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_gloo_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    assert sorted(os.listdir(tmp_path)) == ["plain0.npy", "plain1.npy", "semantic0.npy", "semantic1.npy"]
    for name in ("plain", "semantic"):
        assert np.load(os.path.join(tmp_path, f"{name}0.npy")).tobytes() == np.load(os.path.join(tmp_path, f"{name}1.npy")).tobytes()


# ------------------------------------------------------------------ searcher and MCP tool
class _Recorder:
    def __init__(self):
        self.calls = []

    async def facet(self, **kw):
        self.calls.append(kw)
        return {"hits": [{"value": "a.py", "count": 3}, {"value": "b.py", "count": 1}], "values": 5, "total": 9, "missing": 0}


class _Embedder:
    async def embed(self, text):
        return [0.5] * 4


def test_searcher_and_tool_forward_only_what_is_given():
    from coderag_amd import mcp_tools, vector_search
    from coderag_amd.errors import QueryError, VectorStoreError

    async def run():
        rec = _Recorder()
        vs = vector_search.VectorSearcher(rec, _Embedder())
        res = await vs.facet_code()
        assert res["total"] == 9 and rec.calls == [{"collection": "code_chunks", "key": "file_path", "limit": 10, "filters": None}]
        await vs.facet_code("language", "retry with backoff", 0.6, limit=3, language=["python", "go"], contains="TODO(", contains_case=False, matches=r"x\d")
        assert rec.calls[1] == {"collection": "code_chunks", "key": "language", "limit": 3, "query_vector": [0.5] * 4, "score_threshold": 0.6,
                                "filters": {"language": ["python", "go"], "content": {"contains": "TODO(", "matches": r"x\d", "case": False}}}
        for bad in ({"query": "q"}, {"min_score": 0.5}, {"query": "  ", "min_score": 0.5}):
            with pytest.raises(QueryError):
                await vs.facet_code(**bad)

        class Failing(_Recorder):
            async def facet(self, **kw):
                raise VectorStoreError("Failed to facet code_chunks", cause=ValueError("no"))
        with pytest.raises(QueryError, match="count code by value"):
            await vector_search.VectorSearcher(Failing(), _Embedder()).facet_code()

        class Searcher:
            def __init__(self):
                self.kw = []

            async def facet_code(self, **kw):
                self.kw.append(kw)
                return await rec.facet()
        sr = Searcher()
        tool = mcp_tools.create_code_facets_tool(lambda: sr)
        assert tool["name"] == "code_facets" and {"key", "query", "min_score", "limit", "contains", "matches"} <= set(tool["parameters"])
        plain = await tool["function"]()
        asked = await tool["function"]("language", query="where do we retry", min_score=0.5, limit=2, contains="TODO(")
        assert sr.kw == [{"key": "file_path", "limit": 10},
                         {"key": "language", "limit": 2, "query": "where do we retry", "min_score": 0.5, "contains": "TODO("}]
        assert plain.success and plain.data["hits"][0] == {"value": "a.py", "count": 3} and "5 distinct file_path" in plain.message and "2 most frequent" in plain.message
        assert asked.success

        class Broken:
            async def facet_code(self, **kw):
                raise QueryError("Failed to count code by value")
        failed = await mcp_tools.create_code_facets_tool(lambda: Broken())["function"]()
        assert not failed.success and "count code by value" in failed.error
        # the semantic search tool is as it was
        assert set(mcp_tools.create_semantic_search_tool(lambda: sr)["parameters"]) >= {"query", "limit", "matches"}
    asyncio.run(run())
