"""Set conditions ("in" / "not in") above the device: the C ABI's new entries and their argument checks, the store's translation
of dict values / ``must_not`` / raw-client ``Filter`` objects into conditions, and the one-process-per-shard path carrying them
(world-size-2 gloo).  The index is a fake that evaluates conditions in numpy (a subclass of tests/fake_index.py)."""
import asyncio
import ctypes as C
import os
import socket
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest

from oracle import search as orc
from tests.fake_index import FakeIndex, fake_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class SetFakeIndex(FakeIndex):
    """FakeIndex + set conditions, with the semantics of ``crh_condition``; records every filter it is handed."""
    SET_CONDITIONS = True
    seen: list = []
    tombstone_calls = 0

    def _mask(self, filters=None):
        SetFakeIndex.seen.append(filters)
        ok = self.alive.astype(bool).copy()
        for c in (filters or []):
            if len(c) == 2 and isinstance(c[1], (int, np.integer)):
                ok &= self.codes[:, c[0]] == c[1]
            else:
                member = np.isin(self.codes[:, c[0]], np.asarray([v for v in c[1] if v >= 0], np.int32))
                ok &= ~member if (len(c) == 3 and c[2]) else member
        return ok

    def search(self, queries, k, filters=None, row_base=0, **kw):
        q = orc.preprocess(np.asarray(queries, np.float32), to_bf16=(self.dtype == 1))
        if len(self.x) == 0:
            return np.full((len(q), k), -np.inf, np.float32), np.full((len(q), k), -1, np.int64)
        s, r = orc.search(self.x, q, k, alive=self._mask(filters).astype(np.uint8))
        return s, np.where(r >= 0, r + row_base, r)

    def match_rows(self, filters=None, limit=1):
        return np.flatnonzero(self._mask(filters))[:limit].astype(np.int64)

    def tombstone_filter(self, filters):
        SetFakeIndex.tombstone_calls += 1
        return super().tombstone_filter(filters)


def test_new_entries_are_exported_and_check_their_arguments():
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    L = ffi.lib()
    new = ("crh_search_cond", "crh_index_match_rows_cond", "crh_index_tombstone_cond", "crh_index_set_sparse_route")
    for name in new:
        assert name in ffi.EXPORTS and hasattr(L, name)
    assert L.crh_abi_version() == 4 and C.sizeof(ffi.Condition) == 24
    n = C.c_int64(0)
    q = np.zeros((1, 768), np.float32)
    os_, or_ = np.zeros((1, 5), np.float32), np.zeros((1, 5), np.int64)
    cond = (ffi.Condition * 1)()
    assert L.crh_search_cond(None, 1, q.ctypes.data, 0, 5, cond, 1, 0, os_.ctypes.data, or_.ctypes.data, 0, None) == ffi.E_INVALID
    assert b"NULL" in L.crh_last_error()
    assert L.crh_index_match_rows_cond(None, cond, 1, 10, None, C.byref(n)) == ffi.E_INVALID
    assert L.crh_index_tombstone_cond(None, cond, 1, C.byref(n)) == ffi.E_INVALID
    assert L.crh_index_set_sparse_route(None, 1, 0) == ffi.E_INVALID


def test_binding_packs_both_item_forms():
    from coderag_amd import ffi
    assert not ffi.is_set_condition((0, 3)) and not ffi.is_set_condition((0, np.int32(3)))
    assert ffi.is_set_condition((0, [3])) and ffi.is_set_condition((0, [], True)) and ffi.is_set_condition((1, {1, 2}))
    arr, n, keep = ffi._conditions([(0, 3), (1, {9, 4, 4}), (2, [], True)])
    assert n == 3 and (arr[0].col, arr[0].negate, arr[0].n) == (0, 0, 1) and keep[0].tolist() == [3]
    assert (arr[1].col, arr[1].negate, arr[1].n) == (1, 0, 2) and keep[1].tolist() == [4, 9] and arr[1].codes == keep[1].ctypes.data
    assert (arr[2].negate, arr[2].n, arr[2].codes) == (1, 0, None)
    with pytest.raises(ffi.NativeError):
        ffi._conditions([(0, [1])] * 9)


def _payload(i, file, lang, proj):
    return {"file_path": file, "entity_type": "function", "entity_name": f"ent{i}", "language": lang, "start_line": i, "end_line": i + 3,
            "content": f"def ent{i}(): pass", "graph_node_id": f"mod.ent{i}", "content_hash": "h", "project_name": proj}


def _corpus(n=240, dim=768):
    rng = np.random.default_rng(9)
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    files = [f"/proj/f{i % 12}.py" for i in range(n)]
    langs = [("python", "go", "typescript")[i % 3] for i in range(n)]
    projs = ["p1" if i < 100 else ("p2" if i < 180 else "p3") for i in range(n)]
    payloads = [_payload(i, files[i], langs[i], projs[i]) for i in range(n)]
    ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(n)]
    return rng, vecs, payloads, ids


@pytest.mark.parametrize("shards", [1, 3])
def test_store_translates_values_must_not_and_raw_filters(monkeypatch, shards):
    from coderag_amd.store import HipVectorStore
    fake_device(monkeypatch, SetFakeIndex)
    rng, vecs, payloads, ids = _corpus()
    q = rng.standard_normal(768).astype(np.float32)

    async def run():
        kw = {"shards": shards, "_merge_fn": orc.merge_topk} if shards > 1 else {}
        async with HipVectorStore(dim=768, dtype="f32", initial_capacity=512, device=0, compact_dead_fraction=0.0, **kw) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, vecs, payloads)
            everything = await s.search("code_chunks", q.tolist(), limit=240)
            assert len(everything) == 240

            def host(pred, limit):
                return [(h["id"], h["score"]) for h in everything if pred(h["payload"])][:limit]

            def pairs(hits):
                return [(h["id"], h["score"]) for h in hits]
            # a list / tuple / set value = any of; unknown values contribute nothing; must_not takes one value or a collection
            SetFakeIndex.seen.clear()
            got = await s.search("code_chunks", q.tolist(), limit=20, filters={"language": ["python", "go", "cobol"], "project_name": "p2"},
                                 must_not={"file_path": "/proj/f3.py"})
            assert pairs(got) == host(lambda p: p["language"] in ("python", "go") and p["project_name"] == "p2" and p["file_path"] != "/proj/f3.py", 20)
            dfilt = SetFakeIndex.seen[-1]
            assert [len(c) for c in dfilt] == [3, 2, 3] and len(dfilt[0][1]) == 2 and dfilt[0][2] is False and dfilt[2][2] is True
            got = await s.search_batch("code_chunks", q[None], limit=300, filters={"project_name": {"p1", "p3"}},
                                       must_not={"language": ("go", "rust"), "file_path": ["/proj/f1.py", "/never.py"]})
            assert pairs(got[0]) == host(lambda p: p["project_name"] in ("p1", "p3") and p["language"] != "go" and p["file_path"] != "/proj/f1.py", 300)
            assert await s.search("code_chunks", q.tolist(), limit=5, filters={"language": ["cobol"]}) == []
            assert await s.search("code_chunks", q.tolist(), limit=5, filters={"language": []}) == []
            assert pairs(await s.search("code_chunks", q.tolist(), limit=7, must_not={"language": "cobol"})) == pairs(everything[:7])
            # the filter-only fetch takes them too
            got = await s.search("code_chunks", None, limit=500, filters={"language": ["go"]}, must_not={"project_name": ["p1", "p2"]})
            assert sorted(h["id"] for h in got) == sorted(ids[i] for i in range(240) if i % 3 == 1 and i >= 180)
            # coalesced single queries with different must_not do not share a pass
            a, b = await asyncio.gather(s.search("code_chunks", q.tolist(), limit=3, must_not={"language": "go"}),
                                        s.search("code_chunks", q.tolist(), limit=3, must_not={"language": "python"}))
            assert pairs(a) == host(lambda p: p["language"] != "go", 3) and pairs(b) == host(lambda p: p["language"] != "python", 3)

            # raw client: Filter(must=..., must_not=...), MatchAny, MatchExcept, MatchText -- one device call per shard each
            def fc(key, **m):
                return NS(key=key, match=NS(**m))
            raw = s.client
            flt = NS(must=[fc("language", any=["python", "go"])], must_not=[fc("project_name", value="p1")])
            assert (await raw.count("code_chunks", count_filter=flt)).count == sum(1 for p in payloads if p["language"] != "typescript" and p["project_name"] != "p1")
            flt = NS(must=[fc("project_name", except_=["p1", "p2"])], must_not=None)
            assert (await raw.count("code_chunks", count_filter=flt)).count == 60
            SetFakeIndex.tombstone_calls = 0
            await raw.delete("code_chunks", points_selector=NS(filter=NS(must=[fc("file_path", text="/proj/f1")])))   # f1, f10, f11
            assert SetFakeIndex.tombstone_calls == shards
            gone = {"/proj/f1.py", "/proj/f10.py", "/proj/f11.py"}
            assert (await s.get_collection_info("code_chunks")).points_count == sum(1 for p in payloads if p["file_path"] not in gone)
            SetFakeIndex.tombstone_calls = 0
            await s.delete_files("code_chunks", [f"/proj/f{i}.py" for i in range(2, 8)] + ["/never.py"])
            assert SetFakeIndex.tombstone_calls == shards
            gone |= {f"/proj/f{i}.py" for i in range(2, 8)}
            assert (await s.get_collection_info("code_chunks")).points_count == sum(1 for p in payloads if p["file_path"] not in gone)
            await s.delete("code_chunks", {"language": ["python", "typescript"]}, must_not={"project_name": "p3"})
            left = [p for p in payloads if p["file_path"] not in gone and not (p["language"] != "go" and p["project_name"] != "p3")]
            assert (await s.get_collection_info("code_chunks")).points_count == len(left)
    asyncio.run(run())


def test_searchers_pass_lists_and_exact_exclude():
    import coderag_amd  # noqa: F401
    from coderag_amd import indexer, vector_search

    class Store:
        def __init__(self):
            self.calls = []

        async def search(self, **kw):
            self.calls.append(kw)
            hits = [{"id": str(i), "score": 1.0 - i / 100, "payload": {"file_path": "/hot.py" if i < 10 else f"/f{i}.py"}} for i in range(40)]
            banned = (kw.get("must_not") or {}).get("file_path")
            return [h for h in hits if h["payload"]["file_path"] != banned][:kw["limit"]]

    class Emb:
        async def embed(self, text):
            return [0.0] * 4

    async def run():
        st = Store()
        vs = vector_search.VectorSearcher(st, Emb())
        await vs.search_code("q", limit=3, language=["python", "go"], project_name=["a", "b"])
        assert st.calls[-1]["filters"] == {"language": ["python", "go"], "project_name": ["a", "b"]} and "must_not" not in st.calls[-1]
        default = await vs.find_similar_code("s", limit=10, exclude_file="/hot.py")
        assert st.calls[-1] == {"collection": "code_chunks", "query_vector": [0.0] * 4, "limit": 15} and len(default) == 5
        exact = await vs.find_similar_code("s", limit=10, exclude_file="/hot.py", exact_exclude=True)
        assert st.calls[-1]["limit"] == 10 and st.calls[-1]["must_not"] == {"file_path": "/hot.py"} and "filters" not in st.calls[-1]
        assert len(exact) == 10 and all(h["file_path"] != "/hot.py" for h in exact)
        await vs.find_similar_code("s", limit=10, exact_exclude=True)
        assert st.calls[-1] == {"collection": "code_chunks", "query_vector": [0.0] * 4, "limit": 10}
        iv = indexer.VectorSearcher(st, Emb())
        await iv.search_code("q", limit=2, language=["python", "go"])
        assert st.calls[-1]["filters"] == {"language": ["python", "go"]}
    asyncio.run(run())


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank: int, world: int, port: int, out_dir: str) -> None:
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from coderag_amd.sharded import ShardedIndex
    from coderag_amd.store import HipVectorStore
    from tests.test_filter_sets_host import SetFakeIndex, _corpus

    # ShardedIndex: conditions travel to every rank's shard as they are
    rng = np.random.default_rng(77)
    x = rng.standard_normal((600, 768)).astype(np.float32)
    codes = np.stack([rng.integers(0, 5, 600), rng.integers(-1, 3, 600)], axis=1).astype(np.int32)
    q = rng.standard_normal((4, 768)).astype(np.float32)
    cap = 2048
    sh = ShardedIndex(768, 0, shard_capacity=cap, index_factory=lambda **kw: SetFakeIndex(n_code_cols=2, **kw), merge_fn=orc.merge_topk)
    gid = np.empty(600, np.int64)
    nxt = [0] * world
    for b0 in range(0, 600, 64):
        r, n = (b0 // 64) % world, min(64, 600 - b0)
        gid[b0:b0 + n] = r * cap + nxt[r] + np.arange(n)
        nxt[r] += n
        if r == rank:
            sh.append_local(x[b0:b0 + n], codes[b0:b0 + n])
    conds = [(0, [1, 3], False), (1, [0], True)]
    s, rows = sh.search(q, 30, filters=conds)
    m = np.isin(codes[:, 0], [1, 3]) & (codes[:, 1] != 0)
    es, er = orc.search(orc.preprocess(x, to_bf16=False), orc.preprocess(q, to_bf16=False), 30, alive=m.astype(np.uint8))
    assert np.array_equal(s.numpy(), es), f"rank {rank}: scores differ"
    assert [sorted(a) for a in rows.numpy().tolist()] == [sorted(b) for b in np.where(er >= 0, gid[np.clip(er, 0, None)], -1).tolist()]

    # the store, one process per shard: set values and must_not through search and delete
    import asyncio as aio
    ffi.Index = SetFakeIndex
    ffi.lib = lambda: object()
    ffi.device_count = lambda: 1
    ffi.device_info = lambda d=0: {"name": "fake", "arch": "gfx950", "hbm_bytes": 0, "cu_count": 256}
    ffi.use_device = lambda d: None
    rng, vecs, payloads, ids = _corpus()
    qv = rng.standard_normal(768).astype(np.float32)

    async def run():
        async with HipVectorStore(dim=768, dtype="f32", initial_capacity=512, device=0, shards=world, shard_backend="dist",
                                  compact_dead_fraction=0.0, _merge_fn=orc.merge_topk) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, vecs, payloads)
            everything = await s.search("code_chunks", qv.tolist(), limit=240)
            got = await s.search("code_chunks", qv.tolist(), limit=25, filters={"language": ["python", "go"]}, must_not={"project_name": ["p2"]})
            want = [(h["id"], h["score"]) for h in everything if h["payload"]["language"] in ("python", "go") and h["payload"]["project_name"] != "p2"][:25]
            assert [(h["id"], h["score"]) for h in got] == want, f"rank {rank}"
            await s.delete_files("code_chunks", ["/proj/f0.py", "/proj/f5.py", "/never.py"])
            await s.delete("code_chunks", {"project_name": ("p1", "p3")}, must_not={"language": "go"})
            left = [p for p in payloads if p["file_path"] not in ("/proj/f0.py", "/proj/f5.py") and not (p["project_name"] in ("p1", "p3") and p["language"] != "go")]
            assert (await s.get_collection_info("code_chunks")).points_count == len(left), f"rank {rank}"
    aio.run(run())
    open(os.path.join(out_dir, f"ok{rank}"), "w").write("ok")
    dist.destroy_process_group()


def test_world_size_2_gloo_carries_set_conditions(tmp_path):
    import torch.multiprocessing as mp
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert sorted(os.listdir(tmp_path)) == ["ok0", "ok1"]
