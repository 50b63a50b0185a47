"""Components and layers without a device: the restatement of tests/scc_cases.py against the Boolean closure
(and scipy where it is installed), and the store's plumbing over ``FakeSccGraph`` + a fake index: listings, the four filter
kinds, the cache, upserts, deletes and compaction, snapshots with and without self-loops, refusals, and the surfaces."""
import asyncio
import json

import numpy as np
import pytest

from oracle import search as orc
from tests import facet_cases as fc
from tests import graph_cases as gc
from tests import scc_cases as sc
from tests.fake_index import fake_device

GRAPHS = [gc.chain(9), gc.cycle(7), gc.diamond(), gc.asymmetric(), gc.star(12), sc.two_cycles_joined(), sc.figure_of_eight(), sc.complete(5),
          sc.cycle_entered_above_its_minimum(), sc.cycle_under_a_tail(12), sc.three_cyclic_layers(), sc.wide_lists(9, True), sc.wide_lists(9, False),
          sc.planted(64, 1, sizes=(2, 3, 7)), sc.planted(50, 2, sizes=(2, 2, 11), extra=1), gc.random_graph(40, 1, hubs=2, hub_degree=10), (1, []),
          (5, [(2, 2)]), (3, [])]


# ---------------------------------------------------------------------------------------------------- the restatement
def _closure(n, edges):
    reach = np.eye(n, dtype=bool)
    for a, b in edges:
        reach[a, b] = True
    for k in range(n):
        reach |= reach[:, k:k + 1] & reach[k:k + 1, :]
    return reach


def test_components_equal_the_boolean_closure():
    for gi, (n, edges) in enumerate(GRAPHS):
        assert n <= 64
        reach = _closure(n, edges)
        mutual = reach & reach.T
        want = np.asarray([np.flatnonzero(mutual[v])[0] for v in range(n)], np.int32)
        assert np.array_equal(sc.components(n, edges), want), gi


@pytest.mark.parametrize("direction", ["callees", "callers"])
def test_layers_equal_the_longest_path_by_matrix_powers(direction):
    for gi, (n, edges) in enumerate(GRAPHS):
        comp = sc.components(n, edges)
        arcs = np.zeros((n, n), bool)                                    # the condensation over the labels (a label is a node id)
        for a, b in edges:
            if comp[a] != comp[b]:
                a, b = (comp[a], comp[b]) if direction == "callees" else (comp[b], comp[a])
                arcs[a, b] = True
        longest = np.zeros((n,), np.int32)
        power = np.eye(n, dtype=bool)
        for d in range(1, n + 1):
            power = (power.astype(np.int64) @ arcs.astype(np.int64)) > 0     # walks of exactly d arcs
            longest[power.any(axis=0)] = d
        assert not power.any(), gi                                      # a DAG: no walk of n arcs
        assert np.array_equal(sc.layers(n, edges, comp, direction), longest[comp]), (gi, direction)


def test_components_against_scipy():
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    from scipy.sparse import csr_matrix
    for gi, (n, edges) in enumerate(GRAPHS + [sc.planted(2000, 3), gc.random_graph(1500, 4)]):
        dense = [(a, b) for a, b in edges]
        m = csr_matrix((np.ones(len(dense)), ([a for a, _ in dense], [b for _, b in dense])), shape=(n, n)) if dense else csr_matrix((n, n))
        count, label = csgraph.connected_components(m, directed=True, connection="strong")
        comp = sc.components(n, edges)
        assert len(set(comp.tolist())) == count, gi
        least = {}
        for v in range(n):
            least.setdefault(int(label[v]), v)
        assert comp.tolist() == [least[int(label[v])] for v in range(n)], gi


def test_bins_words_and_self_loops_of_the_restatement():
    n, edges = 6, [(0, 1), (1, 0), (1, 1), (2, 3), (4, 4), (3, 5)]
    comp = sc.components(n, edges)
    assert comp.tolist() == [0, 0, 2, 3, 4, 5] and sc.self_nodes(edges).tolist() == [1, 4]
    bins = sc.cyclic_bins(n, comp, sc.self_nodes(edges))
    assert bins.tolist() == [2, 0, 0, 0, 1, 0] and sc.cyclic_bins(n, comp).tolist() == [2, 0, 0, 0, 0, 0]
    assert sc.top_components(bins, 5) == [(0, 2), (4, 1)] and sc.scc_info(n, comp) == [5, 1, 2]
    assert sc.node_words("in_cycle", comp, bins, q=3).tolist() == [8, 8, 0, 0, 8, 0]
    assert sc.node_words("same_component", comp, lo=0).tolist() == [1, 1, 0, 0, 0, 0]
    assert sc.node_words("range", sc.layers(n, edges, comp, "callees"), lo=1, hi=2, q=63).tolist() == [0, 0, 0, 1 << 63, 0, 1 << 63]


def test_self_loops_of_the_host_builder():
    import coderag_amd  # noqa: F401
    from coderag_amd import graph
    pairs = np.asarray([[3, 3], [0, 1], [1, 1], [3, 3], [1, 0], [2, 3]])
    assert graph.self_loops(pairs, 4).tolist() == [1, 3] and graph.self_loops(pairs, 4).dtype == np.int32
    assert graph.self_loops(np.zeros((0, 2), np.int64), 4).tolist() == [] and graph.unique_edges(pairs, 4).tolist() == [[0, 1], [1, 0], [2, 3]]
    with pytest.raises(ValueError, match="outside"):
        graph.self_loops(np.asarray([[4, 4]]), 4)


# ---------------------------------------------------------------------------------------------------- the store over the fakes
DIM, N = 64, 120
# pkg.fn1 -> pkg.fn2 -> pkg.fn3 -> pkg.fn1 is a cycle (pkg.fn1 also calls itself); pkg.fn5 only calls itself; pkg.fn6 <-> pkg.fn7; "fn8"
# is keyed by its plain entity name; ghost has no chunk
EDGES = [("pkg.fn0", "pkg.fn1"), ("pkg.fn1", "pkg.fn2"), ("pkg.fn2", "pkg.fn3"), ("pkg.fn3", "pkg.fn1"), ("pkg.fn3", "pkg.fn4"), ("pkg.fn1", "pkg.fn1"),
         ("pkg.fn4", "pkg.fn5"), ("pkg.fn5", "pkg.fn5"), ("pkg.fn5", "pkg.fn6"), ("pkg.fn6", "pkg.fn7"), ("pkg.fn7", "pkg.fn6"), ("pkg.fn7", "fn8"),
         ("ghost", "pkg.fn0"), ("pkg.fn0", "pkg.fn1"), ("pkg.fn20", "pkg.fn21")]


def _point(i):
    pay = {"file_path": f"src/m{i % 5}.py", "entity_type": "function", "entity_name": f"fn{i % 30}", "language": "python" if i % 2 else "go",
           "content": "x", "start_line": i, "end_line": i + 2, "project_name": "demo"}
    if i % 4:
        pay["graph_node_id"] = f"pkg.fn{i % 30}"
    return f"00000000-0000-4000-8000-{i:012d}", pay


def _key(pay):
    return pay.get("graph_node_id") or pay["entity_name"]


class Truth:
    """What the restatement says about an edge list given by names."""
    def __init__(self, edges):
        self.names = []
        for e in edges:
            for v in e:
                if v not in self.names:
                    self.names.append(v)
        self.pairs = [(self.names.index(a), self.names.index(b)) for a, b in edges]
        n = len(self.names)
        self.comp = sc.components(n, self.pairs)
        self.loops = sc.self_nodes(self.pairs)
        self.bins = sc.cyclic_bins(n, self.comp, self.loops)
        self.depth, self.height = (sc.layers(n, self.pairs, self.comp, d) for d in ("callees", "callers"))

    def where(self, cond):
        return {self.names[v] for v in range(len(self.names)) if cond(v)}


def _store(monkeypatch):
    sc.FakeSccGraph.scc_calls = 0
    fake_device(monkeypatch, fc.FacetFakeIndex, Graph=sc.FakeSccGraph, facet_select=fc.np_facet_select)
    from coderag_amd import store
    return store


def _open(store, shards):
    kw = {"shards": shards, "_merge_fn": orc.merge_topk} if shards > 1 else {}
    return store.HipVectorStore(dim=DIM, dtype="f32", initial_capacity=512, device=0, **kw)


def _corpus():
    rng = np.random.default_rng(11)
    ids, pay = zip(*[_point(i) for i in range(N)])
    return list(ids), list(pay), rng.standard_normal((N, DIM)).astype(np.float32), rng.standard_normal((3, DIM)).astype(np.float32)


def test_listings(monkeypatch):
    store = _store(monkeypatch)
    ids, pay, vecs, q = _corpus()
    t = Truth(EDGES)

    async def run():
        async with _open(store, 1) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, vecs, pay)
            info = await s.set_graph_edges("code_chunks", EDGES)
            assert info == {"nodes": 12, "relations": {"calls": 12}}                    # 15 edges - a repeat - two self-loops: as before
            col = s._col("code_chunks")
            got = await s.graph_cycles("code_chunks")
            assert got == {"components": [{"id": "pkg.fn1", "size": 3, "nodes": ["pkg.fn1", "pkg.fn2", "pkg.fn3"], "self_recursive": ["pkg.fn1"]},
                                          {"id": "pkg.fn6", "size": 2, "nodes": ["pkg.fn6", "pkg.fn7"], "self_recursive": []},
                                          {"id": "pkg.fn5", "size": 1, "nodes": ["pkg.fn5"], "self_recursive": ["pkg.fn5"]}],
                           "count": 3, "nodes": 6, "self_recursive": ["pkg.fn5"]}
            assert [c["id"] for c in got["components"]] == [t.names[c] for c, _ in sc.top_components(t.bins, 10)]
            one = await s.graph_cycles("code_chunks", limit=1, members=2)
            assert one["components"] == [{"id": "pkg.fn1", "size": 3, "nodes": ["pkg.fn1", "pkg.fn2"], "self_recursive": ["pkg.fn1"]}]
            assert (one["count"], one["nodes"]) == (3, 6)                               # never clipped
            assert (await s.graph_cycles("code_chunks", members=0))["self_recursive"] == 1
            lay = await s.graph_layers("code_chunks", names=["pkg.fn0", "pkg.fn2", "fn8", "nobody", "pkg.fn21"])
            layers = int(t.depth.max()) + 1
            assert lay["layers"] == layers == 7 and lay["unresolved"] == ["nobody"]
            assert lay["histogram"] == {"depth": np.bincount(t.depth, minlength=layers).tolist(), "height": np.bincount(t.height, minlength=layers).tolist()}
            assert lay["nodes"] == [{"name": "pkg.fn0", "depth": 1, "height": 5, "component": "pkg.fn0", "cyclic": False},
                                    {"name": "pkg.fn2", "depth": 2, "height": 4, "component": "pkg.fn1", "cyclic": True},
                                    {"name": "fn8", "depth": 6, "height": 0, "component": "fn8", "cyclic": False},
                                    {"name": "pkg.fn21", "depth": 1, "height": 0, "component": "pkg.fn21", "cyclic": False}]
            assert (await s.graph_layers("code_chunks"))["nodes"] == []
            assert (await s.graph_layers("code_chunks", names="fn2", match="suffix"))["nodes"][0]["name"] == "pkg.fn2"
            assert sc.FakeSccGraph.scc_calls == 1 == col.graph_scc_calls                 # every listing after the first computed nothing
            await s.set_graph_edges("code_chunks", [("pkg.fn1", "pkg.fn0")], relation="extends")
            assert (await s.graph_cycles("code_chunks", relation="extends"))["count"] == 0 and col.graph_scc_calls == 2
            assert (await s.graph_cycles("code_chunks"))["count"] == 3 and col.graph_scc_calls == 3      # a new graph version: derived again
            for call in (s.graph_cycles("code_chunks", relation="imports"), s.graph_cycles("code_chunks", limit=0), s.graph_cycles("code_chunks", members=-1),
                         s.graph_layers("code_chunks", relation="imports"), s.graph_layers("code_chunks", names="a", match="prefix")):
                with pytest.raises(store.VectorStoreError):
                    await call
    asyncio.run(run())


def test_a_self_loop_alone_and_beside_a_pair(monkeypatch):
    store = _store(monkeypatch)

    async def run():
        async with _open(store, 1) as s:
            await s.create_collections()
            await s.set_graph_edges("code_chunks", [("a", "a"), ("a", "b"), ("b", "c"), ("c", "b")])
            got = await s.graph_cycles("code_chunks")
            assert got["components"] == [{"id": "b", "size": 2, "nodes": ["b", "c"], "self_recursive": []},
                                         {"id": "a", "size": 1, "nodes": ["a"], "self_recursive": ["a"]}]
            assert got["self_recursive"] == ["a"] and (got["count"], got["nodes"]) == (2, 3)
            assert await s.graph_info("code_chunks") == {"nodes": 3, "relations": {"calls": 3}}
            await s.set_graph_edges("code_chunks", [("a", "b"), ("b", "c"), ("c", "b")])
            assert (await s.graph_cycles("code_chunks"))["self_recursive"] == []          # the relation was replaced: so were its self-loops
    asyncio.run(run())


@pytest.mark.parametrize("shards", [1, 2])
def test_filters_compose_are_cached_and_follow_the_rows(monkeypatch, shards):
    store = _store(monkeypatch)
    ids, pay, vecs, q = _corpus()
    t = Truth(EDGES)

    async def run():
        async with _open(store, shards) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, vecs, pay)
            await s.set_graph_edges("code_chunks", EDGES)
            col = s._col("code_chunks")

            async def check(filters, must_not, mask):
                want_s, want_r = orc.search(orc.preprocess(vecs), orc.preprocess(q), 10, alive=np.asarray(mask, np.uint8))
                hits = await s.search_batch("code_chunks", q, limit=10, filters=filters, must_not=must_not)
                for qi in range(len(q)):
                    keep = want_r[qi] >= 0
                    assert [ids.index(h["id"]) for h in hits[qi]] == want_r[qi][keep].tolist(), (filters, must_not)
                    assert np.array_equal(np.asarray([h["score"] for h in hits[qi]], np.float32).view(np.uint32), want_s[qi][keep].view(np.uint32))
                fetched = await s.search("code_chunks", None, limit=N, filters=filters, must_not=must_not)
                assert [ids.index(h["id"]) for h in fetched] == np.flatnonzero(mask).tolist()

            def rows(nodes):
                return np.asarray([_key(p) in nodes for p in pay])

            cyclic = t.where(lambda v: t.bins[t.comp[v]] > 0)
            assert cyclic == {"pkg.fn1", "pkg.fn2", "pkg.fn3", "pkg.fn5", "pkg.fn6", "pkg.fn7"}
            in_cycle = rows(cyclic)
            assert 0 < in_cycle.sum() < N
            spec = {"graph": {"in_cycle": True}}
            await check(spec, None, in_cycle)
            tags = [c.tag for c in col.device_filters(spec)]
            await check(spec, None, in_cycle)
            assert [c.tag for c in col.device_filters(spec)] == tags and col.graph_scc_calls == 1 == sc.FakeSccGraph.scc_calls and col.graph_bfs_calls == 0
            await check(None, spec, ~in_cycle)                                           # rows without a node pass a must_not
            lang = np.asarray([p["language"] == "go" for p in pay])
            await check({**spec, "language": "go", "start_line": {"gte": 20, "lte": 90}}, {"file_path": ["src/m1.py"]},
                        in_cycle & lang & np.asarray([20 <= p["start_line"] <= 90 and p["file_path"] != "src/m1.py" for p in pay]))
            same = rows(t.where(lambda v: t.comp[v] == t.comp[t.names.index("pkg.fn2")]))
            await check({"graph": {"same_cycle_as": "pkg.fn2"}}, None, same)
            await check({"graph": {"same_cycle_as": "fn2", "match": "suffix"}}, None, same)
            await check({"language": ["go", "python"]}, {"graph": {"same_cycle_as": "pkg.fn2"}}, ~same)
            await check({"graph": {"same_cycle_as": "pkg.fn4"}}, None, rows({"pkg.fn4"}))   # no cycle: the node's own rows
            assert await s.search("code_chunks", q[0].tolist(), limit=5, filters={"graph": {"same_cycle_as": "nobody"}}) == []
            await check(None, {"graph": {"same_cycle_as": "nobody"}}, np.ones(N, bool))
            for key, layer in (("depth", t.depth), ("height", t.height)):
                await check({"graph": {key: 0}}, None, rows(t.where(lambda v: layer[v] == 0)))
                await check({"graph": {key: {"gte": 2, "lt": 5}}}, None, rows(t.where(lambda v: 2 <= layer[v] < 5)))
                await check({"graph": {key: {"gt": 3}}}, spec, rows(t.where(lambda v: layer[v] > 3)) & ~in_cycle)
                await check({"graph": {key: {"gte": 5, "lte": 4}}}, None, np.zeros(N, bool))
            assert "fn8" in t.where(lambda v: t.height[v] == 0) and rows({"fn8"})[8] and not rows({"fn8"})[38]      # keyed by the entity name
            # the walk conditions beside them: unchanged, and one of each in one filter set
            callers = {t.names[v] for v in gc.bfs_depths(len(t.names), t.pairs, "callers", [t.names.index("pkg.fn3")], 2)}
            await check({"graph": {"callers_of": "pkg.fn3", "hops": 2}}, spec, rows(callers) & ~in_cycle)
            assert col.graph_scc_calls == 1 and col.graph_bfs_calls == 1

            # an upsert of a new chunk of a cyclic node passes; the components are not computed again
            new_ids = ["00000000-0000-4000-8000-999999999901", "00000000-0000-4000-8000-999999999902"]
            new_pay = [dict(_point(2)[1], graph_node_id="pkg.fn2", entity_name="late"), dict(_point(2)[1], graph_node_id="pkg.late", entity_name="late")]
            await s.upsert("code_chunks", new_ids, np.stack([q[0], q[0]]), new_pay)
            top = await s.search("code_chunks", q[0].tolist(), limit=1, filters=spec)
            assert top[0]["id"] == new_ids[0] and col.graph_scc_calls == 1
            # a delete, then compact: rows are renumbered, the answer is not
            await s.delete("code_chunks", {"file_path": "src/m1.py"})
            await s.compact("code_chunks")
            left = [h["id"] for h in await s.search("code_chunks", None, limit=2 * N, filters=spec)]
            assert left == [ids[i] for i in np.flatnonzero(in_cycle) if pay[i]["file_path"] != "src/m1.py"] + [new_ids[0]] and col.graph_scc_calls == 1
            # a replaced relation: the derived state goes, the answer changes
            await s.set_graph_edges("code_chunks", [("pkg.fn8", "pkg.fn9"), ("pkg.fn9", "pkg.fn8")])
            assert col._graph_struct == {}
            got = {_key(h["payload"]) for h in await s.search("code_chunks", None, limit=2 * N, filters=spec)}
            assert got == {"pkg.fn8", "pkg.fn9"} and col.graph_scc_calls == 2
    asyncio.run(run())


def test_refusals_name_the_key(monkeypatch):
    store = _store(monkeypatch)
    ids, pay, vecs, q = _corpus()

    async def run():
        async with _open(store, 1) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, vecs, pay)
            await s.set_graph_edges("code_chunks", EDGES + [("other.fn2", "pkg.fn0")])
            spec = {"graph": {"in_cycle": True}}
            with pytest.raises(store.VectorStoreError) as e:
                await s.search_batch("code_chunks", q, limit=5, filters=[spec, None, None])
            assert "'graph'" in str(e.value.cause) and "per-query" in str(e.value.cause)
            with pytest.raises(store.VectorStoreError) as e:
                await s.delete("code_chunks", spec)
            assert "'graph'" in str(e.value.cause) and "delete" in str(e.value.cause)
            for bad in ({"in_cycle": False}, {"in_cycle": 1}, {"in_cycle": True, "depth": 0}, {"in_cycle": True, "callers_of": "a"}, {"in_cycle": True, "hops": 2},
                        {"depth": -1}, {"depth": 1.5}, {"depth": {"gte": 0.5}}, {"depth": {"from": 1}}, {"depth": True}, {"height": "0"}, {"height": [0, 1]},
                        {"same_cycle_as": ["a", "b"]}, {"same_cycle_as": ""}, {"depth": 1, "match": "suffix"}, {"in_cycle": True, "relation": 3},
                        {"same_cycle_as": "fn2", "match": "suffix"}):
                with pytest.raises(store.VectorStoreError) as e:
                    await s.search("code_chunks", q[0].tolist(), filters={"graph": bad})
                assert "'graph'" in str(e.value.cause), bad
            with pytest.raises(store.VectorStoreError) as e:
                await s.search("code_chunks", None, filters={"graph": {"in_cycle": True, "relation": "imports"}})
            assert "imports" in str(e.value.cause)
            col = s._col("code_chunks")
            monkeypatch.setattr(col.shards, "backend", "dist")
            for call in (s.search("code_chunks", q[0].tolist(), filters=spec), s.graph_cycles("code_chunks"), s.graph_layers("code_chunks")):
                with pytest.raises(store.VectorStoreError) as e:
                    await call
                assert "dist" in str(e.value.cause)
    asyncio.run(run())


@pytest.mark.parametrize("with_self", [True, False])
def test_snapshot_round_trip(monkeypatch, tmp_path, with_self):
    store = _store(monkeypatch)
    ids, pay, vecs, q = _corpus()
    edges = [e for e in EDGES if with_self or e[0] != e[1]]

    async def run():
        async with _open(store, 1) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, vecs, pay)
            await s.set_graph_edges("code_chunks", edges)
            await s.set_graph_edges("code_chunks", [("pkg.fn1", "pkg.fn0"), ("pkg.fn0", "pkg.fn0")], relation="extends")
            want = await s.graph_cycles("code_chunks")
            assert want["count"] == (3 if with_self else 2)
            rows = [h["id"] for h in await s.search("code_chunks", None, limit=N, filters={"graph": {"in_cycle": True}})]
            await s.save(str(tmp_path / "snap"))
        path = tmp_path / "snap" / "code_chunks" / "collection.json"
        meta = json.load(open(path))
        assert meta["format"] == 5
        calls, extends = meta["graph"]["relations"]
        assert ("self" in calls) == with_self and "self" in extends and set(calls) - {"self"} == {"name", "file", "edges"}
        async with _open(store, 1) as s:
            await s.create_collections()
            await s.load(str(tmp_path / "snap"))
            assert await s.graph_cycles("code_chunks") == want
            assert (await s.graph_cycles("code_chunks", relation="extends"))["self_recursive"] == ["pkg.fn0"]
            assert [h["id"] for h in await s.search("code_chunks", None, limit=N, filters={"graph": {"in_cycle": True}})] == rows
        # a snapshot written before there was a "self" entry: no self-loops
        for r in meta["graph"]["relations"]:
            r.pop("self", None)
        json.dump(meta, open(path, "w"))
        async with _open(store, 1) as s:
            await s.create_collections()
            await s.load(str(tmp_path / "snap"))
            got = await s.graph_cycles("code_chunks")
            assert got["count"] == 2 and got["self_recursive"] == [] and [c["self_recursive"] for c in got["components"]] == [[], []]
            assert (await s.graph_cycles("code_chunks", relation="extends"))["count"] == 0
    asyncio.run(run())


# ---------------------------------------------------------------------------------------------------- the surfaces
class _Recorder:
    """A store that records what the searcher sends and answers with canned results."""
    def __init__(self):
        self.calls = []

    async def search(self, **kw):
        self.calls.append(("search", kw))
        return []

    async def search_batch(self, **kw):
        self.calls.append(("search_batch", kw))
        return [[] for _ in kw["query_vectors"]]

    async def graph_cycles(self, **kw):
        self.calls.append(("graph_cycles", kw))
        return {"components": [{"id": "pkg.a.walk", "size": 2, "nodes": ["pkg.a.walk", "pkg.a.visit"], "self_recursive": []}], "count": 4, "nodes": 9,
                "self_recursive": ["pkg.fact"]}

    async def graph_layers(self, **kw):
        self.calls.append(("graph_layers", kw))
        return {"layers": 3, "histogram": {"depth": [4, 3, 2], "height": [5, 2, 2]}, "unresolved": [],
                "nodes": [{"name": "pkg.a.walk", "depth": 1, "height": 2, "component": "pkg.a.walk", "cyclic": True}] if kw["names"] else []}


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
        await vs.search_code("retry handling")
        assert set(rec.calls[-1][1]) == {"collection", "query_vector", "limit", "filters"} and rec.calls[-1][1]["filters"] is None    # the call of before
        await vs.search_code("retry handling", in_cycle=True, language="python")
        assert rec.calls[-1][1]["filters"] == {"language": "python", "graph": {"in_cycle": True}}
        await vs.search_code("retry handling", graph_height=0)
        assert rec.calls[-1][1]["filters"] == {"graph": {"height": 0}}
        await vs.search_code("retry handling", graph_depth={"lte": 1})
        assert rec.calls[-1][1]["filters"] == {"graph": {"depth": {"lte": 1}}}
        await vs.find_similar_code("def f(): pass", in_cycle=True)
        assert rec.calls[-1][1]["filters"] == {"graph": {"in_cycle": True}}
        await vs.search_code("retry handling", within_callers_of="main", graph_hops=2)
        assert rec.calls[-1][1]["filters"] == {"graph": {"callers_of": "main", "hops": 2}}                                              # as before
        for kw in ({"in_cycle": True, "graph_depth": 0}, {"in_cycle": True, "within_callers_of": "main"}, {"graph_height": 0, "graph_hops": 2},
                   {"graph_depth": 0, "graph_height": 0}):
            with pytest.raises(QueryError, match="one graph condition"):
                await vs.search_code("retry handling", **kw)
        with pytest.raises(QueryError, match="filters_per_query"):
            await vs.search_code_batch(["a", "b"], in_cycle=True, filters_per_query=[None, None])
        with pytest.raises(ValueError, match="in_cycle"):
            await vs.search_code("retry handling", propagate=True, in_cycle=True)
        cycles = await vs.find_cycles(limit=3)
        assert rec.calls[-1] == ("graph_cycles", {"collection": "code_chunks", "relation": "calls", "limit": 3, "members": 50})
        assert cycles == {"cycles": [{"name": "walk", "qualified_name": "pkg.a.walk", "size": 2, "members": ["pkg.a.walk", "pkg.a.visit"], "self_recursive": []}],
                          "count": 4, "nodes": 9, "self_recursive": ["pkg.fact"]}
        layers = await vs.find_layers(["walk"], match="suffix")
        assert rec.calls[-1] == ("graph_layers", {"collection": "code_chunks", "relation": "calls", "names": ["walk"], "match": "suffix"})
        assert layers["layers"] == 3 and layers["nodes"] == [{"name": "walk", "qualified_name": "pkg.a.walk", "depth": 1, "height": 2, "component": "pkg.a.walk",
                                                              "cyclic": True}]

        search = mcp_tools.create_semantic_search_tool(lambda: vs)
        assert "in_cycle" in search["parameters"]
        assert (await search["function"]("retry handling", in_cycle=True)).success and rec.calls[-1][1]["filters"] == {"graph": {"in_cycle": True}}
        assert (await search["function"]("retry handling")).success and rec.calls[-1][1]["filters"] is None
        tool = mcp_tools.create_code_graph_tool(lambda: vs)
        res = await tool["function"](op="cycles", limit=5)
        assert res.success and res.data == cycles["cycles"] and rec.calls[-1][1]["limit"] == 5 and "4 call cycle(s) over 9" in res.message
        res = await tool["function"]("walk", op="layers")
        assert res.success and res.data == layers["nodes"] and rec.calls[-1][1]["names"] == "walk" and "3 layer(s)" in res.message
        res = await tool["function"](op="layers")
        assert res.success and res.data == [] and rec.calls[-1][1]["names"] is None
        assert not (await tool["function"]("walk", op="cycles")).success
        assert not (await tool["function"](op="cycles", target="x")).success
        assert not (await tool["function"](op="layers", max_hops=3)).success
        assert not (await tool["function"]("walk", op="levels")).success
    asyncio.run(run())
