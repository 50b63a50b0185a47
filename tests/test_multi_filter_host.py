"""Mixed-filter batches above the device: the C ABI's new entry and its binding, how ``ffi.Index.search_multi`` turns any number
of per-query filters into ``crh_search_multi`` calls, the store's per-query ``filters`` / ``must_not`` and the filter-agnostic
coalescer (``coalesce_filters``).  The index is a fake that evaluates conditions in numpy (a subclass of tests/fake_index.py)
and answers every query under the mask of its own class with the CPU oracle."""
import asyncio
import ctypes as C

import numpy as np
import pytest

from oracle import search as orc
from tests.fake_index import FakeIndex, fake_device


class MultiFakeIndex(FakeIndex):
    """FakeIndex + set conditions + ``search_multi`` (one oracle search per class in use); counts what it is asked."""
    SET_CONDITIONS = True
    multi_calls: list = []
    plain_calls = 0

    def _mask(self, filters=None):
        ok = self.alive.astype(bool).copy()
        for c in (filters or []):
            if len(c) == 2 and isinstance(c[1], (int, np.integer)):
                ok &= self.codes[:, c[0]] == c[1]
            else:
                member = np.isin(self.codes[:, c[0]], np.asarray([v for v in c[1] if v >= 0], np.int32))
                ok &= ~member if (len(c) == 3 and c[2]) else member
        return ok

    def search(self, queries, k, filters=None, row_base=0, **kw):
        MultiFakeIndex.plain_calls += 1
        q = orc.preprocess(np.asarray(queries, np.float32), to_bf16=(self.dtype == 1))
        if len(self.x) == 0 or len(q) == 0:
            return np.full((len(q), k), -np.inf, np.float32), np.full((len(q), k), -1, np.int64)
        s, r = orc.search(self.x, q, k, alive=self._mask(filters).astype(np.uint8))
        return s, np.where(r >= 0, r + row_base, r)

    def search_multi(self, queries, k, class_filters, query_class, row_base=0, **kw):
        from coderag_amd import ffi
        queries = np.asarray(queries, np.float32)
        classes, qclass, calls = ffi.multi_plan(class_filters, query_class)
        MultiFakeIndex.multi_calls.append((len(queries), len(classes), len(calls)))
        out_s, out_r = np.full((len(queries), k), -np.inf, np.float32), np.full((len(queries), k), -1, np.int64)
        before = MultiFakeIndex.plain_calls
        for c in range(len(classes)):
            sel = np.flatnonzero(qclass == c)
            out_s[sel], out_r[sel] = self.search(queries[sel], k, filters=classes[c], row_base=row_base)
        MultiFakeIndex.plain_calls = before
        return out_s, out_r


def test_the_entry_is_exported_bound_and_checks_its_arguments():
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    L = ffi.lib()
    assert "crh_search_multi" in ffi.EXPORTS and hasattr(L, "crh_search_multi") and ffi.MAX_CLASSES == 8
    assert L.crh_abi_version() == 4
    q = np.zeros((1, 768), np.float32)
    os_, or_ = np.zeros((1, 5), np.float32), np.zeros((1, 5), np.int64)
    cond = (ffi.Condition * 1)()
    off, qc = np.asarray([0, 1], np.int32), np.zeros((1,), np.int32)
    assert L.crh_search_multi(None, 1, q.ctypes.data, 0, 5, cond, off.ctypes.data, 1, qc.ctypes.data, 0, os_.ctypes.data, or_.ctypes.data, 0,
                              None) == ffi.E_INVALID
    assert b"NULL" in L.crh_last_error()
    header = open(ffi.PKG_DIR.parent / "include" / "coderag_hip.h").read()
    assert "#define CRH_MAX_CLASSES 8" in header and "#define CRH_ABI_VERSION 4" in header


class RecordingIndex:
    """``ffi.Index`` without a handle: records the native calls ``search_multi`` makes and answers each row with its query's
    first element (so caller order is visible) and its class's first code."""

    def __init__(self):
        from coderag_amd import ffi
        self.dim, self.native, self.plain = 4, [], []
        self.search_multi = ffi.Index.search_multi.__get__(self)

    def _search_multi_native(self, queries, k, classes, qclass, row_base, out_scores, out_rows, stream):
        self.native.append(([list(c) for c in classes], np.asarray(qclass).tolist(), np.asarray(queries)[:, 0].tolist()))
        for i, c in enumerate(np.asarray(qclass).tolist()):
            out_scores[i, :] = queries[i, 0]
            code = classes[c][0][1]
            out_rows[i, :] = (code if isinstance(code, int) else max(code)) + row_base

    def search(self, queries, k, filters=None, row_base=0, out_scores=None, out_rows=None, stream=0):
        self.plain.append((filters, len(queries)))
        return np.zeros((len(queries), k), np.float32), np.full((len(queries), k), -7, np.int64)

    def search_finish(self, stream=0):
        pass


def test_search_multi_deduplicates_splits_and_restores_caller_order():
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    # equal filters are one class, whatever their form and however often they are listed
    ix = RecordingIndex()
    q = np.arange(6, dtype=np.float32)[:, None] * np.ones((1, 4), np.float32)
    s, r = ix.search_multi(q, 3, [[(0, 5)], [(0, [5], False)], [(1, [9, 8], False)], [(1, {8, 9})], [(2, 1)]], [0, 1, 2, 3, 1, 3])
    assert len(ix.native) == 1 and not ix.plain
    classes, qclass, first = ix.native[0]
    assert len(classes) == 2 and qclass == [0, 0, 1, 1, 0, 1] and first == [0, 1, 2, 3, 4, 5]      # (class 4 is used by no query)
    assert r[:, 0].tolist() == [5, 5, 9, 9, 5, 9] and s[:, 0].tolist() == [0, 1, 2, 3, 4, 5]
    # more than 8 classes: the queries ordered by class, at most 8 classes per call, results in caller order
    ix = RecordingIndex()
    n = 50
    rng = np.random.default_rng(0)
    qc = rng.integers(0, 19, n)
    qc[:19] = np.arange(19)
    rng.shuffle(qc)
    q = np.arange(n, dtype=np.float32)[:, None] * np.ones((1, 4), np.float32)
    filters = [[(0, 100 + c)] for c in range(19)]
    s, r = ix.search_multi(q, 2, filters, qc, row_base=1000)
    assert len(ix.native) == 3 and [len(c[0]) for c in ix.native] == [8, 8, 3] and not ix.plain
    assert sorted(v for c in ix.native for v in c[2]) == list(range(n))           # every query in exactly one call
    assert all(max(c[1]) < len(c[0]) for c in ix.native)
    assert s[:, 0].tolist() == list(range(n)) and r[:, 0].tolist() == [1100 + c for c in qc.tolist()]
    assert ffi.multi_passes(filters, qc) == 3 and ffi.multi_passes(filters[:8], np.arange(200) % 8) == 4
    # one distinct class: the existing search path, the code a uniform batch runs today
    ix = RecordingIndex()
    s, r = ix.search_multi(q[:5], 2, [[(0, 5)], [(0, [5])]], [0, 1, 0, 1, 1])
    assert ix.plain == [([(0, 5)], 5)] and not ix.native and (r == -7).all()
    with pytest.raises(ffi.NativeError):
        ix.search_multi(q[:5], 2, [[(0, 5)]], [0, 1, 0, 0, 0])                       # a class id outside the list
    with pytest.raises(ffi.NativeError):
        ix.search_multi(q[:5], 2, [[(0, 5)]], [0, 0])                                # one class id per query


def _payload(i, file, lang, proj):
    return {"file_path": file, "entity_type": "function", "entity_name": f"ent{i}", "language": lang, "start_line": i, "end_line": i + 3,
            "content": f"def ent{i}(): pass", "graph_node_id": f"mod.ent{i}", "content_hash": "h", "project_name": proj}


def _corpus(n=400, dim=768):
    rng = np.random.default_rng(21)
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    langs = [("python", "go", "typescript")[i % 3] for i in range(n)]
    projs = [f"p{i * 5 // n}" for i in range(n)]
    payloads = [_payload(i, f"/proj/f{i % 12}.py", langs[i], projs[i]) for i in range(n)]
    ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(n)]
    return rng, vecs, payloads, ids


def _fake_store(monkeypatch):
    fake_device(monkeypatch, MultiFakeIndex)
    MultiFakeIndex.multi_calls = []
    MultiFakeIndex.plain_calls = 0


FILTERS = [{"project_name": "p0"}, {"project_name": "p1", "language": "go"}, None, {"language": ["python", "typescript"]}, {"project_name": "p4"}]
MUST_NOT = [None, {"file_path": "/proj/f7.py"}, {"language": "go"}, None, {"language": ["go", "python"]}]


def _pairs(hits):
    return [(h["id"], h["score"]) for h in hits]


@pytest.mark.parametrize("shards", [1, 2])
def test_search_batch_with_per_query_filters_equals_lone_searches(monkeypatch, shards):
    from coderag_amd.store import HipVectorStore
    from coderag_amd.vector_search import VectorSearcher
    from coderag_amd.errors import QueryError, VectorStoreError
    _fake_store(monkeypatch)
    rng, vecs, payloads, ids = _corpus()
    nq = 23
    qs = rng.standard_normal((nq, 768)).astype(np.float32)
    flt = [FILTERS[i % 5] for i in range(nq)]
    mnot = [MUST_NOT[i % 5] for i in range(nq)]
    flt[7], mnot[7] = {"project_name": "never-stored"}, None             # an unknown value: nothing, for its own query only
    flt[8], mnot[8] = {"language": ("typescript", "python")}, None       # the same class as FILTERS[3], written differently

    async def run():
        kw = {"shards": shards, "_merge_fn": orc.merge_topk} if shards > 1 else {}
        async with HipVectorStore(dim=768, dtype="f32", initial_capacity=512, device=0, compact_dead_fraction=0.0, search_window_ms=-1, **kw) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, vecs, payloads)
            lone = [await s.search("code_chunks", qs[i].tolist(), limit=9, filters=flt[i], must_not=mnot[i]) for i in range(nq)]
            assert lone[7] == [] and all(len(lone[i]) == 9 for i in range(nq) if i != 7)
            MultiFakeIndex.multi_calls = []
            got = await s.search_batch("code_chunks", qs, limit=9, filters=flt, must_not=mnot)
            assert [_pairs(h) for h in got] == [_pairs(h) for h in lone]
            # every shard saw ONE mixed call: 22 live queries, 5 classes (queries 3 and 8 share theirs)
            assert MultiFakeIndex.multi_calls == [(nq - 1, 5, 1)] * shards
            # one of the two may stay a single dict (or None) for the whole batch
            got = await s.search_batch("code_chunks", qs, limit=9, filters={"language": "go"}, must_not=[{"project_name": f"p{i % 3}"} for i in range(nq)])
            for i in range(nq):
                assert _pairs(got[i]) == _pairs(await s.search("code_chunks", qs[i].tolist(), limit=9, filters={"language": "go"},
                                                               must_not={"project_name": f"p{i % 3}"}))
            # a uniform per-query list runs the plain search: no mixed call
            MultiFakeIndex.multi_calls = []
            got = await s.search_batch("code_chunks", qs, limit=4, filters=[{"project_name": "p2"}] * nq)
            assert not MultiFakeIndex.multi_calls and _pairs(got[3]) == _pairs(await s.search("code_chunks", qs[3].tolist(), limit=4, filters={"project_name": "p2"}))
            assert await s.search_batch("code_chunks", qs[:2], limit=4, filters=[{"project_name": "nope"}, {"language": "cobol"}]) == [[], []]
            # the cases that raise
            for bad in ({"filters": flt[:5]}, {"filters": flt, "diversity": 0.5}, {"must_not": mnot, "group_by": "file_path"},
                        {"filters": ["python"] * nq}):
                with pytest.raises(VectorStoreError) as e:
                    await s.search_batch("code_chunks", qs, limit=4, **bad)
                assert isinstance(e.value.__cause__ or e.value.cause, ValueError)
            # the searcher's keyword
            vs = VectorSearcher(s, None)
            per = [{"language": "go", "project_name": "p1"}, None, {"language": "python"}]
            res = await vs.search_code_batch(qs[:3], limit=5, filters_per_query=per)
            for i in range(3):
                want = await s.search("code_chunks", qs[i].tolist(), limit=5, filters=per[i])
                assert [(h["score"], h["entity_name"]) for h in res[i]] == [(h["score"], h["payload"]["entity_name"]) for h in want]
            with pytest.raises(QueryError):
                await vs.search_code_batch(qs[:3], limit=5, filters_per_query=per, language="go")
            with pytest.raises(QueryError):
                await vs.search_code_batch(qs[:3], limit=5, filters_per_query=per[:2])
    asyncio.run(run())


def test_filter_coalescer_shares_passes_across_filters(monkeypatch):
    from coderag_amd.store import HipVectorStore
    _fake_store(monkeypatch)
    rng, vecs, payloads, ids = _corpus()
    nq = 90
    qs = rng.standard_normal((nq, 768)).astype(np.float32)

    async def run(coalesce_filters):
        kw = {} if coalesce_filters is None else {"coalesce_filters": coalesce_filters}
        async with HipVectorStore(dim=768, dtype="f32", initial_capacity=512, device=0, compact_dead_fraction=0.0, **kw) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, vecs, payloads)
            lone = [await s.search("code_chunks", qs[i].tolist(), limit=3 + i % 6, filters=FILTERS[i % 5], must_not=MUST_NOT[i % 5]) for i in range(nq)]
            before = s.search_passes
            MultiFakeIndex.multi_calls = []
            got = await asyncio.gather(*[s.search("code_chunks", qs[i].tolist(), limit=3 + i % 6, filters=FILTERS[i % 5], must_not=MUST_NOT[i % 5])
                                         for i in range(nq)])
            assert [_pairs(h) for h in got] == [_pairs(h) for h in lone]          # every caller its own filter and its own limit prefix
            return s.search_passes - before, list(MultiFakeIndex.multi_calls)
    passes_on, multi_on = asyncio.run(run(True))
    assert passes_on <= -(-nq // 64) + 1 and multi_on and sum(m[0] for m in multi_on) == nq
    passes_default, multi_default = asyncio.run(run(None))
    passes_off, multi_off = asyncio.run(run(False))
    assert passes_default == passes_off == 5 and not multi_default and not multi_off      # one pass per distinct filter, as before
    monkeypatch.setenv("CODERAG_HIP_COALESCE_FILTERS", "1")
    passes_env, multi_env = asyncio.run(run(None))
    assert passes_env == passes_on and multi_env
