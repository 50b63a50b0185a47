"""The call graph without a device: the restatement of tests/graph_cases.py against the brute-force
definition, the host CSR builder, name resolution, and the store's plumbing over ``FakeGraph`` + a fake index (filters, the
cache, upserts, deletes and compaction, replaced relations, snapshots, refusals, derived degrees, neighbours and chains)."""
import asyncio

import numpy as np
import pytest

from oracle import search as orc
from tests import graph_cases as gc
from tests.facet_cases import FacetFakeIndex
from tests.fake_index import fake_device


# ---------------------------------------------------------------------------------------------------- the restatement
def _matrix_depths(n, edges, direction, sources, max_hops):
    """Minimum depth by definition: the least d for which a walk of d steps from a source exists (Boolean matrix powers)."""
    a = np.zeros((n, n), bool)
    for x, y in edges:
        if x != y:
            if direction in ("callees", "both"):
                a[x, y] = True
            if direction in ("callers", "both"):
                a[y, x] = True
    depth = {}
    reach = np.zeros((n,), bool)
    reach[[s for s in sources if s >= 0]] = True
    for d in range(max_hops + 1):
        for v in np.flatnonzero(reach):
            depth.setdefault(int(v), d)
        reach = (reach.astype(np.int64) @ a.astype(np.int64)) > 0
    return depth


@pytest.mark.parametrize("direction", gc.DIRECTIONS)
def test_restatement_equals_matrix_powers(direction):
    graphs = [gc.chain(9), gc.cycle(7), gc.diamond(), gc.asymmetric(), gc.star(12), gc.random_graph(40, 1, hubs=2, hub_degree=10),
              gc.random_graph(33, 2, mean_degree=1, hubs=1, hub_degree=5), (1, []), (5, [(2, 2)])]
    for gi, (n, edges) in enumerate(graphs):
        for hops in (1, 2, 5, 16):
            for sources in ([0], [n - 1, 0], [], [n // 2, -1, n // 2]):
                assert gc.bfs_depths(n, edges, direction, sources, hops) == _matrix_depths(n, edges, direction, sources, hops), (gi, hops, sources)


def test_restatement_words_lists_and_paths():
    n, edges = gc.diamond()
    levels, seen, active, maps = gc.bfs_words(n, edges, "callees", [[0], [5], []], 3)
    assert maps[0] == {0: 0, 1: 1, 2: 1, 5: 2, 3: 2, 4: 3, 6: 3} and maps[1] == {5: 0, 6: 1} and maps[2] == {}
    assert levels[2, 5] == 1 and levels[0, 5] == 2 and levels[3, 6] == 1 and levels[1, 6] == 2
    assert seen[0] == 0 and seen[5] == 1 and seen[6] == 3 and active.tolist() == [3, 3, 1, 1]
    assert gc.bfs_words(n, edges, "callees", [[0]], 3, include_self=True)[1][0] == 1
    nodes, depth, count = gc.listing(maps, 1, 4)
    assert nodes.tolist() == [[1, 2, 3, 5], [6, -1, -1, -1], [-1] * 4] and depth[0].tolist() == [1, 1, 2, 2] and count.tolist() == [6, 1, 0]
    assert gc.shortest_path(n, edges, "callees", [0], 5, 4) == [0, 1, 5] and gc.shortest_path(n, edges, "callees", [0], 6, 2) == []
    assert gc.shortest_path(n, edges, "callers", [6], 0, 8) == [6, 5, 1, 0] and gc.shortest_path(n, edges, "callees", [3], 3, 1) == [3]
    words = gc.row_words([5, -1, 6, 0, 5] + [6] * 30, {5, 6})
    assert words.tolist() == [0xfffffff5, 0x7] and gc.mask_from_words(words, 35).sum() == 33


# ---------------------------------------------------------------------------------------------------- the host builder
def test_csr_builder():
    import coderag_amd  # noqa: F401
    from coderag_amd import graph
    code, names = {}, []
    pairs = graph.number_edges([("b", "a"), ("a", "c"), ("b", "a"), ("c", "c"), ("d", "a"), ("b", "c")], code, names)
    assert names == ["b", "a", "c", "d"] and code == {"b": 0, "a": 1, "c": 2, "d": 3}                  # order of first appearance
    assert pairs.tolist() == [[0, 1], [1, 2], [0, 1], [2, 2], [3, 1], [0, 2]]
    more = graph.number_edges([("a", "e")], code, names)
    assert names[-1] == "e" and more.tolist() == [[1, 4]] and code["b"] == 0                            # ids only grow
    assert graph.unique_edges(pairs, 4).tolist() == [[0, 1], [0, 2], [1, 2], [3, 1]]                  # no repeat, no self-loop
    off_f, adj_f, off_r, adj_r = graph.build_csr(pairs, 4)
    assert off_f.tolist() == [0, 2, 3, 3, 4] and adj_f.tolist() == [1, 2, 2, 1]
    assert off_r.tolist() == [0, 0, 2, 4, 4] and adj_r.tolist() == [0, 3, 0, 1]                        # every list ascends
    assert (off_f.dtype, adj_f.dtype) == (np.int64, np.int32)
    assert graph.total_degrees(pairs, 4).tolist() == [2, 3, 2, 1]
    for n, edges in (gc.random_graph(200, 3), gc.star(70), (3, []), (1, [(0, 0)])):
        got = graph.build_csr(np.asarray(edges, np.int64).reshape(-1, 2), n)
        for g, w in zip(got, gc.csr_pair(n, edges)):
            assert np.array_equal(g, w)
    with pytest.raises(ValueError, match="pair of strings"):
        graph.number_edges([("a", 3)], {}, [])
    with pytest.raises(ValueError, match="outside"):
        graph.unique_edges(np.asarray([[0, 4]]), 4)


def test_name_resolution():
    from coderag_amd import graph
    names = ["pkg.mod.parse", "parse", "pkg.other.parse", "pkg.mod.reparse", "pkg.mod.run", "x.parse.y"]
    code = {v: i for i, v in enumerate(names)}
    assert graph.resolve("parse", code, names) == ([1], [])
    assert graph.resolve(["parse", "nope", "pkg.mod.run"], code, names) == ([1, 4], ["nope"])
    assert graph.resolve("parse", code, names, "suffix") == ([0, 1, 2], [])                             # never "reparse", never "x.parse.y"
    assert graph.resolve(["mod.parse", "run", "y"], code, names, "suffix") == ([0, 4, 5], [])
    assert graph.resolve(["arse"], code, names, "suffix") == ([], ["arse"])
    with pytest.raises(ValueError, match="suffix"):
        graph.resolve("parse", code, names, "prefix")


# ---------------------------------------------------------------------------------------------------- the store over the fakes
DIM, N = 64, 120
EDGES = [(f"pkg.fn{i}", f"pkg.fn{i + 1}") for i in range(9)] + [("pkg.fn3", "fn8"), ("pkg.fn20", "pkg.fn3"), ("pkg.fn21", "pkg.fn20"),
                                                                   ("pkg.fn5", "pkg.fn5"), ("pkg.fn0", "pkg.fn1"), ("ghost", "pkg.fn0")]


def _point(i):
    """Chunk i belongs to entity fn(i % 30): four chunks per entity; every fourth chunk has no graph_node_id (its key is the
    entity name); start_line = i."""
    pay = {"file_path": f"src/m{i % 5}.py", "entity_type": "function", "entity_name": f"fn{i % 30}", "language": "python" if i % 2 else "go",
           "content": "x", "start_line": i, "end_line": i + 2, "project_name": "demo"}
    if i % 4:
        pay["graph_node_id"] = f"pkg.fn{i % 30}"
    return f"00000000-0000-4000-8000-{i:012d}", pay


def _key(pay):
    return pay.get("graph_node_id") or pay["entity_name"]


def _reached(edges, direction, sources, hops, include_self=True):
    names = []
    for e in edges:
        for v in e:
            if v not in names:
                names.append(v)
    pairs = [(names.index(a), names.index(b)) for a, b in edges]
    depth = gc.bfs_depths(len(names), pairs, direction, [names.index(s) for s in sources if s in names], hops)
    return {names[v]: d for v, d in depth.items() if include_self or d > 0}


def _store(monkeypatch):
    gc.FakeGraph.bfs_calls = 0
    fake_device(monkeypatch, FacetFakeIndex, Graph=gc.FakeGraph)
    from coderag_amd import store
    return store


def _open(store, shards):
    kw = {"shards": shards, "_merge_fn": orc.merge_topk} if shards > 1 else {}
    return store.HipVectorStore(dim=DIM, dtype="f32", initial_capacity=512, device=0, **kw)


def _corpus():
    rng = np.random.default_rng(11)
    ids, pay = zip(*[_point(i) for i in range(N)])
    return list(ids), list(pay), rng.standard_normal((N, DIM)).astype(np.float32), rng.standard_normal((3, DIM)).astype(np.float32)


def _expect(vecs, q, k, mask):
    s, r = orc.search(orc.preprocess(vecs), orc.preprocess(q), k, alive=np.asarray(mask, np.uint8))
    return s, r


async def _ids_of(s, ids, q, k, **kw):
    hits = await s.search_batch("code_chunks", q, limit=k, **kw)
    return [[ids.index(h["id"]) for h in row] for row in hits], [[np.float32(h["score"]) for h in row] for row in hits]


@pytest.mark.parametrize("shards", [1, 2])
def test_graph_filter_composes_and_is_cached(monkeypatch, shards):
    store = _store(monkeypatch)
    ids, pay, vecs, q = _corpus()

    async def run():
        async with _open(store, shards) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, vecs, pay)
            info = await s.set_graph_edges("code_chunks", EDGES)
            assert info == {"nodes": 14, "relations": {"calls": 13}} == await s.graph_info("code_chunks")        # 15 edges - a repeat - a self-loop
            col = s._col("code_chunks")

            async def check(filters, must_not, mask):
                want_s, want_r = _expect(vecs, q, 10, mask)
                got_r, got_s = await _ids_of(s, ids, q, 10, filters=filters, must_not=must_not)
                for qi in range(len(q)):
                    keep = want_r[qi] >= 0
                    assert got_r[qi] == want_r[qi][keep].tolist(), (filters, must_not)
                    assert np.array_equal(np.asarray(got_s[qi], np.float32).view(np.uint32), want_s[qi][keep].view(np.uint32))
                assert (await s.client.count("code_chunks", count_filter=None)).count == N
                fetched = await s.search("code_chunks", None, limit=N, filters=filters, must_not=must_not)
                assert [ids.index(h["id"]) for h in fetched] == np.flatnonzero(mask).tolist()

            callers = _reached(EDGES, "callers", ["pkg.fn3"], 2)
            assert set(callers) == {"pkg.fn3", "pkg.fn2", "pkg.fn1", "pkg.fn20", "pkg.fn21"}
            in_callers = np.asarray([_key(p) in callers for p in pay])
            assert 0 < in_callers.sum() < N
            spec = {"graph": {"callers_of": "pkg.fn3", "hops": 2}}
            await check(spec, None, in_callers)
            assert gc.FakeGraph.bfs_calls == 1 == col.graph_bfs_calls
            await check(spec, None, in_callers)                                                             # the same filter again: no second BFS
            assert gc.FakeGraph.bfs_calls == 1 == col.graph_bfs_calls
            # beside a set, a range and an exclusion; under must_not; without the sources' own rows
            lang = np.asarray([p["language"] == "go" for p in pay])
            lines = np.asarray([20 <= p["start_line"] <= 90 for p in pay])
            await check({**spec, "language": "go", "start_line": {"gte": 20, "lte": 90}}, {"file_path": ["src/m1.py"]},
                        in_callers & lang & lines & np.asarray([p["file_path"] != "src/m1.py" for p in pay]))
            await check({"language": ["go", "python"]}, spec, ~in_callers)
            callees = _reached(EDGES, "callees", ["pkg.fn3", "nobody"], 3, include_self=False)
            assert "fn8" in callees and "pkg.fn3" not in callees
            in_callees = np.asarray([_key(p) in callees for p in pay])
            assert in_callees[8] and in_callees[68] and not in_callees[38]                                 # the rows whose key is the plain entity name
            await check({"graph": {"callees_of": ["pkg.fn3", "nobody"], "hops": 3, "include_self": False}}, None, in_callees)
            both = _reached(EDGES, "both", ["pkg.fn9"], 16)
            await check({"graph": {"connected_to": "pkg.fn9", "hops": 16}}, spec, np.asarray([_key(p) in both for p in pay]) & ~in_callers)
            await check({"graph": {"callers_of": "fn3", "hops": 2, "match": "suffix"}}, None, in_callers)
            # no name is a node: must matches nothing, must_not excludes nothing
            assert await s.search("code_chunks", q[0].tolist(), limit=5, filters={"graph": {"callers_of": "nobody"}}) == []
            await check(None, {"graph": {"callers_of": "nobody"}}, np.ones(N, bool))

            # an upsert of a new chunk of a reached node lets that chunk pass; an unrelated one does not
            before = gc.FakeGraph.bfs_calls
            new_ids = ["00000000-0000-4000-8000-999999999901", "00000000-0000-4000-8000-999999999902"]
            new_pay = [dict(_point(2)[1], graph_node_id="pkg.fn2", entity_name="late"), dict(_point(2)[1], graph_node_id="pkg.late", entity_name="late")]
            await s.upsert("code_chunks", new_ids, np.stack([q[0], q[0]]), new_pay)
            top = await s.search("code_chunks", q[0].tolist(), limit=1, filters=spec)
            assert top[0]["id"] == new_ids[0] and gc.FakeGraph.bfs_calls == before + 1
            assert new_ids[1] not in [h["id"] for h in await s.search("code_chunks", None, limit=2 * N, filters=spec)]

            # a delete, then compact: rows are renumbered, the answer is not
            await s.delete("code_chunks", {"file_path": "src/m1.py"})
            await s.compact("code_chunks")
            left = [h["id"] for h in await s.search("code_chunks", None, limit=2 * N, filters=spec)]
            assert left == [ids[i] for i in np.flatnonzero(in_callers) if pay[i]["file_path"] != "src/m1.py"] + [new_ids[0]]

            # a replaced relation: a new answer under a new tag; another relation is left alone
            tag = col.device_filters(spec)[0].tag
            assert col.device_filters(spec)[0].tag == tag
            await s.set_graph_edges("code_chunks", [("pkg.fn7", "pkg.fn3")])
            await s.set_graph_edges("code_chunks", [("pkg.fn12", "pkg.fn3")], relation="extends")
            assert (await s.graph_info("code_chunks")) == {"nodes": 15, "relations": {"calls": 1, "extends": 1}}       # (pkg.fn12 is new; the old names keep their ids)
            assert col.device_filters(spec)[0].tag != tag
            for rel, who in (("calls", "pkg.fn7"), ("extends", "pkg.fn12")):
                got = {h["payload"].get("graph_node_id") or h["payload"]["entity_name"]
                       for h in await s.search("code_chunks", None, limit=2 * N, filters={"graph": {"callers_of": "pkg.fn3", "relation": rel, "include_self": False}})}
                assert got == {who}
            with pytest.raises(store.VectorStoreError) as e:
                await s.search("code_chunks", None, filters={"graph": {"callers_of": "pkg.fn3", "relation": "imports"}})
            assert "imports" in str(e.value.cause)
    asyncio.run(run())


def test_graph_filter_refusals_name_the_key(monkeypatch):
    store = _store(monkeypatch)
    ids, pay, vecs, q = _corpus()

    async def run():
        async with _open(store, 1) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, vecs, pay)
            await s.set_graph_edges("code_chunks", EDGES)
            spec = {"graph": {"callers_of": "pkg.fn3"}}
            with pytest.raises(store.VectorStoreError) as e:
                await s.search_batch("code_chunks", q, limit=5, filters=[spec, None, None])
            assert "'graph'" in str(e.value.cause) and "per-query" in str(e.value.cause)
            with pytest.raises(store.VectorStoreError) as e:
                await s.delete("code_chunks", spec)
            assert "'graph'" in str(e.value.cause) and "delete" in str(e.value.cause)
            for bad in ({"callers_of": "a", "callees_of": "b"}, {"hops": 2}, {"callers_of": "a", "hops": 17}, {"callers_of": "a", "depth": 2}, {"callers_of": []},
                        {"callers_of": 3}, "pkg.fn3", {"callers_of": "a", "match": "prefix"}):
                with pytest.raises(store.VectorStoreError) as e:
                    await s.search("code_chunks", q[0].tolist(), filters={"graph": bad})
                assert "'graph'" in str(e.value.cause), bad
            col = s._col("code_chunks")
            monkeypatch.setattr(col.shards, "backend", "dist")
            with pytest.raises(store.VectorStoreError) as e:
                await s.search("code_chunks", q[0].tolist(), filters=spec)
            assert "'graph'" in str(e.value.cause) and "dist" in str(e.value.cause)
    asyncio.run(run())


def test_neighbors_chains_and_degrees(monkeypatch):
    store = _store(monkeypatch)
    ids, pay, vecs, q = _corpus()

    async def run():
        async with _open(store, 1) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, vecs, pay)
            await s.set_graph_edges("code_chunks", EDGES, derive_degrees=True)
            col = s._col("code_chunks")
            # pkg.fn3: called by fn2 and fn20, calls fn4 and fn8; the self-loop of fn5 and the repeated edge do not count
            assert col._degrees["pkg.fn3"] == 4 and col._degrees["pkg.fn5"] == 2 and col._degrees["pkg.fn0"] == 2 and col._degrees["ghost"] == 1
            await s.set_graph_degrees("code_chunks", {"pkg.fn3": 9})
            assert col._degrees == {"pkg.fn3": 9}
            await s.set_graph_edges("code_chunks", EDGES)                                                   # without derive_degrees: the table stays
            assert col._degrees == {"pkg.fn3": 9}

            got = await s.graph_neighbors("code_chunks", "pkg.fn3", max_hops=2)
            assert got == {"hits": [{"name": "pkg.fn2", "depth": 1}, {"name": "pkg.fn20", "depth": 1}, {"name": "pkg.fn1", "depth": 2}, {"name": "pkg.fn21", "depth": 2}],
                           "count": 4, "unresolved": []}
            got = await s.graph_neighbors("code_chunks", ["pkg.fn3", "nobody"], direction="callees", max_hops=16, limit=3, include_self=True)
            assert [h["name"] for h in got["hits"]] == ["pkg.fn3", "pkg.fn4", "fn8"] and got["count"] == 8 and got["unresolved"] == ["nobody"]
            many = await s.graph_neighbors_batch("code_chunks", [f"pkg.fn{i % 10}" for i in range(65)], direction="callees", max_hops=1)
            assert len(many) == 65 and gc.FakeGraph.bfs_calls >= 2
            assert [h["name"] for h in many[64]["hits"]] == ["pkg.fn5"] and [h["name"] for h in many[3]["hits"]] == ["pkg.fn4", "fn8"]
            assert (await s.graph_neighbors("code_chunks", "fn3", match="suffix", max_hops=1))["count"] == 2

            assert await s.call_chain("code_chunks", "pkg.fn21", "pkg.fn5") == ["pkg.fn21", "pkg.fn20", "pkg.fn3", "pkg.fn4", "pkg.fn5"]
            assert await s.call_chain("code_chunks", "pkg.fn21", "pkg.fn5", max_hops=3) is None
            assert await s.call_chain("code_chunks", "pkg.fn5", "pkg.fn21") is None and await s.call_chain("code_chunks", "pkg.fn5", "nobody") is None
            assert await s.call_chain("code_chunks", "pkg.fn4", "pkg.fn4") == ["pkg.fn4"]
            with pytest.raises(store.VectorStoreError):
                await s.graph_neighbors("code_chunks", "pkg.fn3", max_hops=17)
            with pytest.raises(store.VectorStoreError):
                await s.graph_neighbors("code_chunks", "pkg.fn3", direction="up")
            for r in range(7):
                await s.set_graph_edges("code_chunks", [("a", "b")], relation=f"r{r}")
            with pytest.raises(store.VectorStoreError) as e:
                await s.set_graph_edges("code_chunks", [("a", "b")], relation="ninth")
            assert "at most 8" in str(e.value.cause)
            with pytest.raises(store.VectorStoreError):
                await s.set_graph_edges("code_chunks", [("a", "zz"), ("a",)], relation="calls")
            assert "zz" not in col._graph_code and (await s.graph_info("code_chunks"))["relations"]["calls"] == 13   # a refused list leaves nothing
    asyncio.run(run())


@pytest.mark.parametrize("with_graph", [True, False])
def test_snapshot_round_trip(monkeypatch, tmp_path, with_graph):
    import json
    store = _store(monkeypatch)
    ids, pay, vecs, q = _corpus()
    spec = {"graph": {"callees_of": "pkg.fn3", "hops": 4}}

    async def run():
        async with _open(store, 1) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, vecs, pay)
            if with_graph:
                await s.set_graph_edges("code_chunks", EDGES)
                await s.set_graph_edges("code_chunks", [("pkg.fn1", "pkg.fn0")], relation="extends")
                want = [h["id"] for h in await s.search("code_chunks", None, limit=N, filters=spec)]
                assert want
            await s.save(str(tmp_path / "snap"))
        meta = json.load(open(tmp_path / "snap" / "code_chunks" / "collection.json"))
        assert meta["format"] == 5 and ("graph" in meta) == with_graph
        async with _open(store, 1) as s:
            await s.create_collections()
            await s.load(str(tmp_path / "snap"))
            if with_graph:
                assert await s.graph_info("code_chunks") == {"nodes": 14, "relations": {"calls": 13, "extends": 1}}
                assert [h["id"] for h in await s.search("code_chunks", None, limit=N, filters=spec)] == want
                assert await s.call_chain("code_chunks", "pkg.fn1", "pkg.fn0", relation="extends") == ["pkg.fn1", "pkg.fn0"]
                await s.set_graph_edges("code_chunks", [("pkg.fn0", "fresh")], relation="extends")        # ids go on growing behind the loaded names
                assert (await s.graph_info("code_chunks"))["nodes"] == 15
            else:
                assert await s.graph_info("code_chunks") == {"nodes": 0, "relations": {}}
                with pytest.raises(store.VectorStoreError):
                    await s.search("code_chunks", None, filters=spec)
    asyncio.run(run())


# ---------------------------------------------------------------------------------------------------- the surfaces
class _Recorder:
    """A store that records what the searcher sends and answers with canned graph results."""
    def __init__(self):
        self.calls = []

    async def search(self, **kw):
        self.calls.append(("search", kw))
        return []

    async def search_batch(self, **kw):
        self.calls.append(("search_batch", kw))
        return [[] for _ in kw["query_vectors"]]

    async def graph_neighbors(self, **kw):
        self.calls.append(("graph_neighbors", kw))
        return {"hits": [{"name": "pkg.mod.f", "depth": 1}, {"name": "main", "depth": 2}], "count": 2, "unresolved": []}

    async def call_chain(self, **kw):
        self.calls.append(("call_chain", kw))
        return ["a.f", "b.g", "c.h"] if kw["target"] == "c.h" else None


class _Embedder:
    async def embed(self, text):
        return [0.0] * 4

    async def embed_batch(self, texts):
        return [[0.0] * 4 for _ in texts]


def test_searcher_and_mcp_surfaces():
    import coderag_amd  # noqa: F401
    from coderag_amd import mcp_tools
    from coderag_amd.errors import QueryError
    from coderag_amd.vector_search import VectorSearcher

    async def run():
        rec = _Recorder()
        vs = VectorSearcher(rec, _Embedder())
        await vs.search_code("timeout handling")
        assert rec.calls[-1][1]["filters"] is None                                                       # nothing asked: the call of before
        await vs.search_code("timeout handling", language="python", within_callees_of="main", graph_hops=5)
        assert rec.calls[-1][1]["filters"] == {"language": "python", "graph": {"callees_of": "main", "hops": 5}}
        await vs.search_summaries("retries", within_callers_of=["a.f", "b.g"])
        assert rec.calls[-1][1]["filters"] == {"graph": {"callers_of": ["a.f", "b.g"]}}
        await vs.find_similar_code("def f(): pass", within_callers_of="a.f")
        assert rec.calls[-1][1]["filters"] == {"graph": {"callers_of": "a.f"}}
        await vs.find_similar_code("def f(): pass")
        assert "filters" not in rec.calls[-1][1]
        await vs.search_code_batch(["x", "y"], within_callees_of="main")
        assert rec.calls[-1][0] == "search_batch" and rec.calls[-1][1]["filters"] == {"graph": {"callees_of": "main"}}
        for bad in (lambda: vs.search_code("x", within_callers_of="a", within_callees_of="b"), lambda: vs.search_code("x", graph_hops=2),
                    lambda: vs.search_code_batch(["x"], within_callers_of="a", filters_per_query=[None])):
            with pytest.raises(QueryError):
                await bad()
        got = await vs.find_callers("c.h", max_hops=2, limit=7)
        assert rec.calls[-1] == ("graph_neighbors", {"collection": "code_chunks", "names": "c.h", "direction": "callers", "max_hops": 2, "limit": 7})
        assert got == [{"name": "f", "qualified_name": "pkg.mod.f", "metadata": {"depth": 1}}, {"name": "main", "qualified_name": "main", "metadata": {"depth": 2}}]
        await vs.find_callees("c.h")
        assert rec.calls[-1][1]["direction"] == "callees" and rec.calls[-1][1]["max_hops"] == 3
        assert await vs.find_call_chain("a.f", "c.h") == [{"nodes": ["a.f", "b.g", "c.h"], "relationships": ["CALLS", "CALLS"], "total_length": 2, "path_type": "call_chain"}]
        assert await vs.find_call_chain("a.f", "nowhere") == []

        search = mcp_tools.create_semantic_search_tool(lambda: vs)
        assert {"within_callers_of", "within_callees_of", "graph_hops"} <= set(search["parameters"])
        assert (await search["function"]("timeouts", within_callees_of="main", graph_hops=4)).success
        assert rec.calls[-1][1]["filters"] == {"graph": {"callees_of": "main", "hops": 4}}
        assert (await search["function"]("timeouts")).success and rec.calls[-1][1]["filters"] is None
        tool = mcp_tools.create_code_graph_tool(lambda: vs)
        assert tool["name"] == "code_graph" and tool["parameters"]["name"]["required"]
        res = await tool["function"]("c.h")
        assert res.success and [n["qualified_name"] for n in res.data] == ["pkg.mod.f", "main"] and rec.calls[-1][1]["direction"] == "callers"
        res = await tool["function"]("a.f", relation="chain", target="c.h", max_hops=4)
        assert res.success and res.data[0]["total_length"] == 2 and rec.calls[-1][1]["max_hops"] == 4
        assert (await tool["function"]("a.f", relation="chain", target="nowhere")).data == []
        assert not (await tool["function"]("a.f", relation="chain")).success and not (await tool["function"]("a.f", relation="sideways")).success
    asyncio.run(run())
