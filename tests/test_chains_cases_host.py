"""Chains in full without a device: the restatement of tests/chains_cases.py against a brute force that
enumerates every simple path, and the store's plumbing over ``FakeChainsGraph`` + a fake index: ``call_chains``, batches, the
``between`` filter with its cache, refusals, unresolved and ambiguous names, and the surfaces."""
import asyncio

import numpy as np
import pytest

from oracle import search as orc
from tests import chains_cases as cc
from tests import facet_cases as fc
from tests import graph_cases as gc
from tests.fake_index import fake_device

SHAPES = [gc.chain(6), gc.cycle(5), gc.diamond(), gc.asymmetric(), gc.star(4, extra=1), cc.ladder(3), cc.two_diamonds(), cc.long_detour(4)[:2],
          cc.fan(5)[:2], cc.fan(4, at_target=False)[:2], cc.layered(2, layers=3)[:2], (1, []), (3, [(0, 0)])]


def _random_small(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 11))
    return n, [(int(a), int(b)) for a, b in rng.integers(0, n, size=(int(rng.integers(1, 5 * n)), 2))]


GRAPHS = SHAPES + [_random_small(seed) for seed in range(40)]


def _cases(n, seed):
    """(sources, target, max_hops) triples over a graph of n nodes: single sources, sets, the target a source, short bounds."""
    rng = np.random.default_rng(seed)
    out = [([0], n - 1, 16), ([0], n - 1, 2), ([n - 1], 0, 5)]
    for _ in range(6):
        out.append((rng.integers(0, n, size=int(rng.integers(1, 4))).tolist(), int(rng.integers(0, n)), int(rng.integers(1, 9))))
    out.append(([0, 0, n - 1], n - 1, 3))
    out.append(([], 0, 3))
    return out


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("direction", ["callees", "callers"])
def test_the_restatement_equals_the_brute_force(direction):
    checked = many = 0
    for gi, (n, edges) in enumerate(GRAPHS):
        for sources, target, hops in _cases(n, gi):
            paths = cc.simple_paths(n, edges, direction, sources, target, hops)
            count, length, chains = cc.chains(n, edges, direction, sources, target, hops, cc.MAX_CHAINS)
            where = (gi, sources, target, hops)
            if not paths:
                assert (count, length, chains) == (0, 0, []) and cc.must_pass(n, edges, direction, sources, target, hops) == [], where
                assert cc.between(n, edges, direction, sources, [target], hops) == (set(), -1), where
                continue
            least = min(len(p) for p in paths)
            shortest = sorted((p for p in paths if len(p) == least), key=lambda p: p[::-1])
            assert count == len(shortest) and length == least, where
            assert chains == shortest[:cc.MAX_CHAINS], where
            assert chains[0] == gc.shortest_path(n, edges, direction, sources, target, hops), where
            ends = {int(s) for s in sources} | {target}
            common = set.intersection(*[set(p) - ends for p in paths])
            got = cc.must_pass(n, edges, direction, sources, target, hops)
            assert set(got) == common and got == [v for v in chains[0] if v in common], where
            anyway, dist = cc.between(n, edges, direction, sources, [target], hops)
            assert dist == least - 1 and set().union(*map(set, paths)) <= anyway, where
            assert cc.between(n, edges, direction, sources, [target], hops, shortest=True)[0] == set().union(*map(set, shortest)), where
            checked += 1
            many += count > 1
    assert checked > 150 and many >= 15                              # (the cases are not all trivial: many pairs have several chains)


def test_counts_saturate_and_ranks_still_unrank():
    n, edges, s, t = cc.layered(19)
    assert cc.chains(n, edges, "callees", [s], t, 16, 1)[0] == 19 ** 15 < cc.SATURATED
    n, edges, s, t = cc.layered(20)
    count, length, some = cc.chains(n, edges, "callees", [s], t, 16, 3)
    assert count == cc.SATURATED < 20 ** 15 and length == 17
    last = [1 + k * 20 for k in range(15)]                              # backwards order: the smallest node of every layer first ...
    assert some == [[0] + last + [t], [0, 2] + last[1:] + [t], [0, 3] + last[1:] + [t]]   # ... and the FIRST layer varies fastest
    assert cc.chains(n, edges, "callees", [s], t, 15, 3) == (0, 0, [])     # one hop short
    assert cc.chains(n, edges, "callers", [t], s, 16, 1)[0] == cc.SATURATED


def test_shapes_say_what_their_docstrings_say():
    n, edges = cc.ladder(3)
    assert cc.chains(n, edges, "callees", [0], 9, 16, 64)[:2] == (8, 7) and cc.must_pass(n, edges, "callees", [0], 9, 16) == [3, 6]
    assert cc.must_pass(*gc.diamond(), "callees", [0], 5, 16) == [] and cc.must_pass(*gc.chain(6), "callees", [0], 5, 16) == [1, 2, 3, 4]
    assert cc.must_pass(*cc.two_diamonds(), "callees", [0], 6, 16) == [3]
    n, edges, s, t = cc.long_detour(5)
    assert cc.must_pass(n, edges, "callees", [s], t, 5) == [1] and cc.must_pass(n, edges, "callees", [s], t, 6) == []
    for width in (63, 64, 65, 300):
        for at_target in (True, False):
            n, edges, s, t = cc.fan(width, at_target)
            count, length, some = cc.chains(n, edges, "callees", [s], t, 16, 64)
            assert (count, length) == (width, 3 if at_target else 4) and [c[1] for c in some] == list(range(1, 2 * min(width, 64), 2))
    words = cc.sigma_words(*gc.diamond(), "callees", [[0], [2], [6]], 4)
    assert words.shape == (7, 4) and words[:, 3].tolist() == [0] * 7 and words[5].tolist() == [1, 1, 0, 0] and words[6].tolist() == [1, 1, 1, 0]


# ---------------------------------------------------------------------------------------------------- the store over the fakes
DIM, N = 64, 120
# pkg.fn0 reaches pkg.fn6 by a ladder of two diamonds (fn0 -> {fn1, fn2} -> fn3 -> {fn4, fn5} -> fn6) and by a long way round
# (fn0 -> fn7 -> fn8 -> fn9 -> fn10 -> fn6); other.fn6 makes "fn6" ambiguous under match="suffix"; ghost has no chunk
EDGES = [("pkg.fn0", "pkg.fn1"), ("pkg.fn0", "pkg.fn2"), ("pkg.fn1", "pkg.fn3"), ("pkg.fn2", "pkg.fn3"), ("pkg.fn3", "pkg.fn4"), ("pkg.fn3", "pkg.fn5"),
         ("pkg.fn4", "pkg.fn6"), ("pkg.fn5", "pkg.fn6"), ("pkg.fn0", "pkg.fn7"), ("pkg.fn7", "pkg.fn8"), ("pkg.fn8", "pkg.fn9"), ("pkg.fn9", "pkg.fn10"),
         ("pkg.fn10", "pkg.fn6"), ("pkg.fn6", "pkg.fn11"), ("ghost", "pkg.fn0"), ("pkg.fn12", "pkg.fn3"), ("other.fn6", "pkg.fn13"), ("pkg.fn6", "pkg.fn6"),
         ("pkg.fn20", "pkg.fn21")]


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
        self.n = len(self.names)

    def ids(self, names):
        return [self.names.index(v) for v in ([names] if isinstance(names, str) else names) if v in self.names]

    def answer(self, source, target, hops=8, limit=10, must_pass=True):
        s, t = self.ids(source), self.ids(target)
        missing = [v for v in ([source] if isinstance(source, str) else list(source)) + [target] if v not in self.names]
        count, length, chains = cc.chains(self.n, self.pairs, "callees", s, t[0], hops, max(limit, 1)) if t else (0, 0, [])
        must = cc.must_pass(self.n, self.pairs, "callees", s, t[0], hops) if t and must_pass else []
        return {"count": count, "saturated": count == cc.SATURATED, "length": length - 1 if length else None,
                "chains": [[self.names[v] for v in c] for c in chains[:limit]], "must_pass": [self.names[v] for v in must], "unresolved": missing}

    def between(self, sources, targets, hops=8, shortest=False):
        return {self.names[v] for v in cc.between(self.n, self.pairs, "callees", self.ids(sources), self.ids(targets), hops, shortest)[0]}


def _store(monkeypatch):
    gc.FakeGraph.bfs_calls = 0
    fake_device(monkeypatch, fc.FacetFakeIndex, Graph=cc.FakeChainsGraph, facet_select=fc.np_facet_select)
    from coderag_amd import store
    return store


def _open(store, shards):
    kw = {"shards": shards, "_merge_fn": orc.merge_topk} if shards > 1 else {}
    return store.HipVectorStore(dim=DIM, dtype="f32", initial_capacity=512, device=0, **kw)


def _corpus():
    rng = np.random.default_rng(11)
    ids, pay = zip(*[_point(i) for i in range(N)])
    return list(ids), list(pay), rng.standard_normal((N, DIM)).astype(np.float32), rng.standard_normal((3, DIM)).astype(np.float32)


def test_call_chains_and_batches(monkeypatch):
    store = _store(monkeypatch)
    t = Truth(EDGES)

    async def run():
        async with _open(store, 1) as s:
            await s.create_collections()
            await s.set_graph_edges("code_chunks", EDGES)
            got = await s.call_chains("code_chunks", "pkg.fn0", "pkg.fn6")
            assert got == t.answer("pkg.fn0", "pkg.fn6") and got["count"] == 4 and got["length"] == 4 and got["must_pass"] == []
            assert got["chains"][0] == await s.call_chain("code_chunks", "pkg.fn0", "pkg.fn6")
            assert got["chains"][0] == ["pkg.fn0", "pkg.fn1", "pkg.fn3", "pkg.fn4", "pkg.fn6"] and not got["saturated"]
            # within 4 edges the way round (5 edges) does not count: pkg.fn3 cannot be avoided; within 5 it can
            assert (await s.call_chains("code_chunks", "pkg.fn0", "pkg.fn6", max_hops=4))["must_pass"] == ["pkg.fn3"]
            assert (await s.call_chains("code_chunks", "pkg.fn0", "pkg.fn6", max_hops=5)) == t.answer("pkg.fn0", "pkg.fn6", hops=5)
            assert t.answer("pkg.fn0", "pkg.fn6", hops=5)["must_pass"] == []
            assert await s.call_chains("code_chunks", "pkg.fn0", "pkg.fn6", limit=2) == t.answer("pkg.fn0", "pkg.fn6", limit=2)
            none = await s.call_chains("code_chunks", "pkg.fn0", "pkg.fn6", limit=0, must_pass=False)
            assert none == {"count": 4, "saturated": False, "length": 4, "chains": [], "must_pass": [], "unresolved": []}
            assert await s.call_chains("code_chunks", "pkg.fn6", "pkg.fn0") == {"count": 0, "saturated": False, "length": None, "chains": [], "must_pass": [],
                                                                                "unresolved": []}
            assert await s.call_chains("code_chunks", "pkg.fn0", "pkg.fn0") == t.answer("pkg.fn0", "pkg.fn0") and t.answer("pkg.fn0", "pkg.fn0")["length"] == 0
            sets = await s.call_chains("code_chunks", ["pkg.fn12", "ghost", "nobody"], "pkg.fn11")
            assert sets == t.answer(["pkg.fn12", "ghost", "nobody"], "pkg.fn11") and sets["unresolved"] == ["nobody"] and sets["chains"][0][0] == "pkg.fn12"
            assert sets["must_pass"] == ["pkg.fn6"]                                      # (from ghost, 7 edges lead round pkg.fn3)
            assert await s.call_chains("code_chunks", "pkg.fn0", "nobody") == {"count": 0, "saturated": False, "length": None, "chains": [], "must_pass": [],
                                                                               "unresolved": ["nobody"]}
            assert (await s.call_chains("code_chunks", "fn0", "pkg.fn6", match="suffix"))["count"] == 4
            with pytest.raises(store.VectorStoreError) as e:
                await s.call_chains("code_chunks", "pkg.fn0", "fn6", match="suffix")
            assert "pkg.fn6" in str(e.value.cause) and "other.fn6" in str(e.value.cause) and "name one" in str(e.value.cause)
            for kw in ({"max_hops": 0}, {"max_hops": 17}, {"limit": 65}, {"limit": -1}, {"relation": "imports"}, {"match": "prefix"}):
                with pytest.raises(store.VectorStoreError):
                    await s.call_chains("code_chunks", "pkg.fn0", "pkg.fn6", **kw)
            # 65 pairs: two passes; a repeated pair; every answer the restatement's
            pairs = [(f"pkg.fn{i % 14}", f"pkg.fn{(i * 5 + 6) % 14}") for i in range(63)] + [("pkg.fn0", "pkg.fn6"), ("pkg.fn0", "pkg.fn6")]
            before = gc.FakeGraph.bfs_calls
            batch = await s.call_chains_batch("code_chunks", pairs, must_pass=False)
            assert gc.FakeGraph.bfs_calls == before + 2 and len(batch) == 65
            assert batch == [t.answer(a, b, must_pass=False) for a, b in pairs]
            assert await s.call_chains_batch("code_chunks", pairs) == [t.answer(a, b) for a, b in pairs]
            assert await s.call_chains_batch("code_chunks", []) == []
            col = s._col("code_chunks")
            monkeypatch.setattr(col.shards, "backend", "dist")
            with pytest.raises(store.VectorStoreError) as e:
                await s.call_chains("code_chunks", "pkg.fn0", "pkg.fn6")
            assert "dist" in str(e.value.cause)
    asyncio.run(run())


@pytest.mark.parametrize("shards", [1, 2])
def test_between_filters_compose_and_are_cached(monkeypatch, shards):
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

            wide = t.between(["pkg.fn0"], ["pkg.fn6"])
            assert wide == {f"pkg.fn{i}" for i in range(11)}                              # the ladder and the way round
            spec = {"graph": {"between": ["pkg.fn0", "pkg.fn6"]}}
            assert 0 < rows(wide).sum() < N
            await check(spec, None, rows(wide))
            tags = [c.tag for c in col.device_filters(spec)]
            calls = (gc.FakeGraph.bfs_calls, col.graph_bfs_calls)
            assert calls == (2, 2)                                                       # one search from either end
            await check(spec, None, rows(wide))
            assert [c.tag for c in col.device_filters(spec)] == tags and (gc.FakeGraph.bfs_calls, col.graph_bfs_calls) == calls   # cached: no BFS
            await check(None, spec, ~rows(wide))                                         # rows without a node pass a must_not
            assert (gc.FakeGraph.bfs_calls, col.graph_bfs_calls) == calls
            narrow = t.between(["pkg.fn0"], ["pkg.fn6"], hops=4)
            assert narrow == {f"pkg.fn{i}" for i in range(7)}
            await check({"graph": {"between": ["pkg.fn0", "pkg.fn6"], "hops": 4}}, None, rows(narrow))
            await check({"graph": {"between": [["pkg.fn0"], ["pkg.fn6"]], "shortest": True}}, None, rows(narrow))
            assert col.device_filters({"graph": {"between": ["pkg.fn0", "pkg.fn6"], "shortest": True}})[0].tag != tags[0]
            sets = t.between(["pkg.fn12", "pkg.fn7"], ["pkg.fn4", "pkg.fn10"], hops=3)
            assert sets == {"pkg.fn12", "pkg.fn3", "pkg.fn4", "pkg.fn7", "pkg.fn8", "pkg.fn9", "pkg.fn10"}
            await check({"graph": {"between": [["pkg.fn12", "pkg.fn7"], ["pkg.fn4", "pkg.fn10"]], "hops": 3}}, None, rows(sets))
            await check({"graph": {"between": ["fn0", "fn11"], "match": "suffix", "hops": 5}}, None, rows(t.between(["pkg.fn0"], ["pkg.fn11"], hops=5)))
            lang = np.asarray([p["language"] == "go" for p in pay])
            await check({**spec, "language": "go", "start_line": {"gte": 20, "lte": 90}}, {"file_path": ["src/m1.py"]},
                        rows(wide) & lang & np.asarray([20 <= p["start_line"] <= 90 and p["file_path"] != "src/m1.py" for p in pay]))
            await check({"graph": {"callees_of": "pkg.fn3", "hops": 2}}, spec,
                        rows({t.names[v] for v in gc.bfs_depths(t.n, t.pairs, "callees", t.ids("pkg.fn3"), 2)}) & ~rows(wide))
            # unresolved names match nothing; under must_not they exclude nothing
            for ends in (["nobody", "pkg.fn6"], ["pkg.fn0", "nobody"], ["pkg.fn6", "pkg.fn0"]):
                assert await s.search("code_chunks", q[0].tolist(), limit=5, filters={"graph": {"between": ends}}) == []
                await check(None, {"graph": {"between": ends}}, np.ones(N, bool))
            # a replaced relation: the words are computed again, and differ
            before = gc.FakeGraph.bfs_calls
            await s.set_graph_edges("code_chunks", [("pkg.fn0", "pkg.fn9"), ("pkg.fn9", "pkg.fn6")])
            got = {_key(h["payload"]) for h in await s.search("code_chunks", None, limit=2 * N, filters=spec)}
            assert got == {"pkg.fn0", "pkg.fn9", "pkg.fn6"} and gc.FakeGraph.bfs_calls == before + 2
    asyncio.run(run())


def test_refusals_name_the_key(monkeypatch):
    store = _store(monkeypatch)
    ids, pay, vecs, q = _corpus()

    async def run():
        async with _open(store, 1) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, vecs, pay)
            await s.set_graph_edges("code_chunks", EDGES)
            spec = {"graph": {"between": ["pkg.fn0", "pkg.fn6"]}}
            with pytest.raises(store.VectorStoreError) as e:
                await s.search_batch("code_chunks", q, limit=5, filters=[spec, None, None])
            assert "'graph'" in str(e.value.cause) and "per-query" in str(e.value.cause)
            with pytest.raises(store.VectorStoreError) as e:
                await s.delete("code_chunks", spec)
            assert "'graph'" in str(e.value.cause) and "delete" in str(e.value.cause)
            for bad in ({"between": "pkg.fn0"}, {"between": ["pkg.fn0"]}, {"between": ["a", "b", "c"]}, {"between": ["a", 3]}, {"between": ["a", []]},
                        {"between": ["a", "b"], "hops": 0}, {"between": ["a", "b"], "hops": 17}, {"between": ["a", "b"], "hops": True},
                        {"between": ["a", "b"], "shortest": 1}, {"between": ["a", "b"], "include_self": True}, {"between": ["a", "b"], "callers_of": "a"},
                        {"between": ["a", "b"], "in_cycle": True}, {"between": ["a", "b"], "match": "prefix"}, {"between": ["a", "b"], "relation": 3}):
                with pytest.raises(store.VectorStoreError) as e:
                    await s.search("code_chunks", q[0].tolist(), filters={"graph": bad})
                assert "'graph'" in str(e.value.cause), bad
            with pytest.raises(store.VectorStoreError) as e:
                await s.search("code_chunks", None, filters={"graph": {"between": ["a", "b"], "relation": "imports"}})
            assert "imports" in str(e.value.cause)
            col = s._col("code_chunks")
            monkeypatch.setattr(col.shards, "backend", "dist")
            with pytest.raises(store.VectorStoreError) as e:
                await s.search("code_chunks", q[0].tolist(), filters=spec)
            assert "dist" in str(e.value.cause)
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

    async def call_chains(self, **kw):
        self.calls.append(("call_chains", kw))
        return {"count": 2, "saturated": False, "length": 2, "chains": [["pkg.a.main", "pkg.a.open", "pkg.db.execute"], ["pkg.a.main", "pkg.b.retry", "pkg.db.execute"]],
                "must_pass": [], "unresolved": []}


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
        assert rec.calls[-1][1]["filters"] is None                                       # the call of before
        await vs.search_code("retry handling", between=("main", "execute"), language="python")
        assert rec.calls[-1][1]["filters"] == {"language": "python", "graph": {"between": ["main", "execute"]}}
        await vs.search_code("retry handling", between=(["main", "cli"], "execute"), graph_hops=5)
        assert rec.calls[-1][1]["filters"] == {"graph": {"between": [["main", "cli"], "execute"], "hops": 5}}
        await vs.find_similar_code("def f(): pass", between=("main", "execute"))
        assert rec.calls[-1][1]["filters"] == {"graph": {"between": ["main", "execute"]}}
        await vs.search_summaries("retry handling", between=("main", "execute"), graph_hops=2)
        assert rec.calls[-1][1]["filters"] == {"graph": {"between": ["main", "execute"], "hops": 2}}
        await vs.search_code_batch(["a", "b"], between=("main", "execute"))
        assert rec.calls[-1][1]["filters"] == {"graph": {"between": ["main", "execute"]}}
        for kw in ({"between": ("a", "b"), "in_cycle": True}, {"between": ("a", "b"), "within_callers_of": "main"}, {"between": ("a", "b"), "graph_depth": 0},
                   {"between": ("a",)}, {"between": "ab"}):
            with pytest.raises(QueryError):
                await vs.search_code("retry handling", **kw)
        with pytest.raises(QueryError, match="filters_per_query"):
            await vs.search_code_batch(["a", "b"], between=("a", "b"), filters_per_query=[None, None])
        got = await vs.find_call_chains("main", "execute", max_hops=6, limit=5)
        assert rec.calls[-1] == ("call_chains", {"collection": "code_chunks", "source": "main", "target": "execute", "relation": "calls", "max_hops": 6,
                                                 "limit": 5, "must_pass": True, "match": "exact"})
        assert got["count"] == 2 and got["chains"][1] == ["pkg.a.main", "pkg.b.retry", "pkg.db.execute"] and got["must_pass"] == []

        search = mcp_tools.create_semantic_search_tool(lambda: vs)
        assert "between" in search["parameters"]
        assert (await search["function"]("retry handling", between=["main", "execute"])).success
        assert rec.calls[-1][1]["filters"] == {"graph": {"between": ["main", "execute"]}}
        tool = mcp_tools.create_code_graph_tool(lambda: vs)
        res = await tool["function"]("main", op="chains", target="execute", max_hops=4)
        assert res.success and res.data == got["chains"] and rec.calls[-1][1]["max_hops"] == 4 and "2 shortest chain(s)" in res.message
        assert not (await tool["function"]("main", op="chains")).success               # no target
    asyncio.run(run())
