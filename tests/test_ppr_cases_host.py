"""Personalised PageRank without a device: the restatement of tests/ppr_cases.py against a float64 dense
iteration under a DERIVED bound, the chain whose every entry is known in closed form, the mass dropped at sinks, and the
store's plumbing and the surfaces over ``ppr_cases.FakeGraph`` + a fake index."""
import asyncio

import numpy as np
import pytest

from oracle import search as orc
from tests import fuse_cases
from tests import graph_cases as gc
from tests import ppr_cases as pc
from tests.facet_cases import FacetFakeIndex
from tests.fake_index import fake_device

F32 = np.float32
U32 = np.uint32


# ---------------------------------------------------------------------------------------------------- the restatement
def _dense(fwd, rev, direction, seeds, weights, restart, steps):
    """x <- r * x0 + a * P x in float64, P[u, v] = (times v stands in u's pull list) / out(v)."""
    n = len(fwd)
    pull, out = pc.pull_lists(fwd, rev, direction)
    P = np.zeros((n, n))
    for u in range(n):
        for v in pull[u]:
            P[u, v] += 1.0 / out[v]
    x0 = np.zeros((n, len(seeds)))
    for q, (nodes, ws) in enumerate(zip(seeds, weights)):
        total = sum(float(F32(w)) for v, w in zip(nodes, ws) if v >= 0)
        for v, w in zip(nodes, ws):
            if v >= 0 and total > 0:
                x0[v, q] += float(F32(w)) / total
    r = float(F32(restart))
    a = float(F32(F32(1.0) - F32(restart)))
    x = x0.copy()
    for _ in range(steps):
        x = r * x0 + a * (P @ x)
    return x


def _hub_graph(n, degree, seed):
    """A random graph with one node that ``degree`` others call and that calls ``degree`` others: pull lists of ~degree entries."""
    _, edges = gc.random_graph(n, seed, mean_degree=2, hubs=1, hub_degree=degree)
    return n, edges


@pytest.mark.parametrize("direction", gc.DIRECTIONS)
@pytest.mark.parametrize("n,degree,steps", [(300, 200, 16), (90, 40, 64), (40, 5, 1)])
def test_restatement_within_the_derived_bound(direction, n, degree, steps):
    """All terms are non-negative, so every f32 operation adds at most one relative rounding error of 2^-24 to what it holds:
    c + 2 roundings make an entry of p0 (c - 1 additions per sum, twice, and the division, bounded together), and a step adds
    D + 4 (the product with inv, inv's own rounding, D additions, the two products and the final addition share the rest).
    No cancellation can amplify them.  1.01 covers the second-order terms."""
    n, edges = _hub_graph(n, degree, n + steps)
    fwd, rev = pc.graph_lists(n, edges)
    rng = np.random.default_rng(n)
    c = 9
    seeds = [rng.integers(0, n, c).tolist() for _ in range(5)]
    seeds[1][3] = seeds[1][0]                                                       # a repeated node
    seeds[2][4] = -1                                                                # padding
    weights = [rng.random(c).astype(F32).tolist() for _ in range(5)]
    weights[3][2] = 0.0
    got = pc.ppr(fwd, rev, direction, seeds, weights, 0.15, steps)
    want = _dense(fwd, rev, direction, seeds, [[0.0 if v < 0 else w for v, w in zip(s, ws)] for s, ws in zip(seeds, weights)], 0.15, steps)
    D = max(len(p) for p in pc.pull_lists(fwd, rev, direction)[0])
    assert D >= min(degree, n - 1) - 1                                              # (the hub may have drawn itself: self-loops are dropped)
    bound = 1.01 * (steps * (D + 4) + c + 2) * 2.0 ** -24
    err = np.abs(got.astype(np.float64) - want) / np.maximum(want, 2.0 ** -120)
    print(f"n={n} D={D} steps={steps} {direction}: worst error {err.max() / 2.0 ** -24:.1f} units of 2^-24, bound {bound / 2.0 ** -24:.0f}")
    assert got.dtype == F32 and (got >= 0).all() and err.max() <= bound
    assert (got.sum(0) <= 1.0 + bound).all() and got.sum() > 0


def test_chain_puts_every_entry_where_it_belongs():
    """0 -> 1 -> ... -> 7 walked along the edges from node 0: after T steps node k < T holds restart * a^k, node T holds a^T and
    nothing lies behind it -- each the product of its factors rounded one at a time."""
    n, edges = gc.chain(8)
    fwd, rev = pc.graph_lists(n, edges)
    r = F32(0.15)
    a = F32(F32(1.0) - r)

    def times_a(x, k):
        for _ in range(k):
            x = F32(a * x)
        return x

    for T in (1, 2, 5, 7):
        got = pc.ppr(fwd, rev, "callees", [[0]], None, 0.15, T)[:, 0]
        want = np.asarray([times_a(r, k) for k in range(T)] + [times_a(F32(1.0), T)] + [F32(0.0)] * (n - T - 1), F32)
        assert np.array_equal(got.view(U32), want.view(U32)), T
    # against the edges from the far end: the mirror image
    back = pc.ppr(fwd, rev, "callers", [[7]], None, 0.15, 5)[:, 0]
    fwd5 = pc.ppr(fwd, rev, "callees", [[0]], None, 0.15, 5)[:, 0]
    assert np.array_equal(back[::-1].view(U32), fwd5.view(U32))


def test_mass_is_dropped_at_sinks():
    n, edges = gc.chain(3)
    fwd, rev = pc.graph_lists(n, edges)
    r = F32(0.15)
    a = F32(F32(1.0) - r)
    got = pc.ppr(fwd, rev, "callees", [[0]], None, 0.15, 40)[:, 0]
    want = np.asarray([r, F32(a * r), F32(a * F32(a * r))], F32)                     # node 2 calls nothing: what reaches it goes nowhere
    assert np.array_equal(got.view(U32), want.view(U32)) and float(got.sum()) < 0.5
    # "both": nothing is a sink, the mass stays (up to rounding)
    both = pc.ppr(fwd, rev, "both", [[0]], None, 0.15, 40)[:, 0]
    assert abs(float(both.sum()) - 1.0) < 1e-5
    # a query without a real seed scores nothing, beside a live one
    two = pc.ppr(fwd, rev, "both", [[-1, 1], [0]], [[1.0, 0.0], [2.0]], 0.15, 3)
    assert not two[:, 0].any() and np.array_equal(two[:, 1].view(U32), pc.ppr(fwd, rev, "both", [[0]], None, 0.15, 3)[:, 0].view(U32))


def test_seeds_tops_and_orders():
    p0 = pc.seed_vectors(5, [[3, 1, 3, -1], [2, 2]], [[1.0, 2.0, 3.0, 9.0], [0.0, 0.0]])
    assert p0[:, 0].tolist() == [0.0, F32(2.0) / F32(6.0), 0.0, F32(4.0) / F32(6.0), 0.0] and not p0[:, 1].any()
    clamped = pc.seed_vectors(5, [[0, 1, 2, 7]], [[-1.0, float("nan"), 2.0, 1.0]], device_list=True)
    assert clamped[:, 0].tolist() == [0.0, 0.0, 1.0, 0.0, 0.0]
    scores = np.asarray([[0.25], [0.5], [0.0], [0.25], [0.5]], F32)
    nodes, vals = pc.top_list(scores, 4)
    assert nodes.tolist() == [[1, 4, 0, 3]] and vals.tolist() == [[0.5, 0.5, 0.25, 0.25]]
    nodes, vals = pc.top_list(scores, 6, exclude=[[4, -1]])
    assert nodes.tolist() == [[1, 0, 3, -1, -1, -1]] and vals[0, 3:].tolist() == [0.0] * 3
    assert np.array_equal(pc.bins_of(scores, [[4]])[0], np.asarray([0x3e800000, 0x3f000000, 0, 0x3e800000, 0]))
    fs, fr, gs = pc.order_lists(scores, [[10, 11, 12, 13, -1]], [[0.9, 0.8, 0.7, 0.6, -np.inf]], [[0, 4, -1, 1, 1]])
    assert fr[0, 1].tolist() == [11, 13, 10, -1, -1] and gs.tolist() == [[0.25, 0.5, 0.0, 0.5, 0.0]]
    assert fs[0, 1, :3].tolist() == [0.5, 0.5, 0.25] and np.isneginf(fs[0, 1, 3:]).all() and fr[0, 0].tolist() == [10, 11, 12, 13, -1]
    ranked = pc.rrf_two(fr[0], 3, 60)
    assert [row for row, _, _ in ranked] == [11, 10, 13]                            # 1/62 + 1/61, 1/61 + 1/63, 1/64 + 1/62
    assert ranked[0][1] == F32(F32(1.0) / F32(62) + F32(1.0) / F32(61)) and [f for _, _, f in ranked] == [1, 0, 3]


# ---------------------------------------------------------------------------------------------------- the store over the fakes
DIM, N = 64, 120
EDGES = [(f"pkg.fn{i}", f"pkg.fn{i + 1}") for i in range(9)] + [("pkg.fn3", "fn8"), ("pkg.fn20", "pkg.fn3"), ("pkg.fn21", "pkg.fn20"),
                                                                   ("pkg.fn5", "pkg.fn5"), ("pkg.fn0", "pkg.fn1"), ("ghost", "pkg.fn0"),
                                                                   ("pkg.fn8", "pkg.fn2"), ("pkg.fn21", "pkg.fn6")]


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


def _names(edges):
    names = []
    for e in edges:
        for v in e:
            if v not in names:
                names.append(v)
    return names


def _store(monkeypatch):
    pc.FakeGraph.ppr_calls = 0
    fake_device(monkeypatch, FacetFakeIndex, Graph=pc.FakeGraph, fuse_select=fuse_cases.fuse_select)
    from coderag_amd import store
    return store


def _open(store, shards):
    kw = {"shards": shards, "_merge_fn": orc.merge_topk} if shards > 1 else {}
    return store.HipVectorStore(dim=DIM, dtype="f32", initial_capacity=512, device=0, **kw)


def _global_rows(store, col, n):
    from coderag_amd.shards import STRIDE
    shard, local = col.rows_of(np.arange(n))
    return shard.astype(np.int64) * STRIDE + local


def _want(store, col, ids, pay, vecs, q, alive, names, edges, limit, candidates, related_limit, mask=None, **prop):
    """The restated answer: the oracle's exact top-``candidates`` under ``alive & mask``, their nodes, and ppr_cases.propagated;
    hits as (id, fused bits, cosine bits, graph-score bits), related as (name, score bits, id of the representative chunk)."""
    keep = alive if mask is None else alive & mask
    cs, cr = orc.search(orc.preprocess(vecs), orc.preprocess(q), candidates, alive=keep.astype(np.uint8))
    grow = _global_rows(store, col, len(ids))
    node_of = np.asarray([names.index(_key(p)) if _key(p) in names else -1 for p in pay])
    cand_nodes = np.where(cr >= 0, node_of[np.maximum(cr, 0)], -1)
    cand_rows = np.where(cr >= 0, grow[np.maximum(cr, 0)], -1)
    slot_of_row = {int(g): i for i, g in enumerate(grow)}
    numbered = [(names.index(a), names.index(b)) for a, b in edges]
    fwd, rev = pc.graph_lists(len(names), numbered)
    out = []
    for hits, related in pc.propagated(fwd, rev, cs, cand_rows, cand_nodes, limit, related_limit, **prop):
        rel = []
        for v, s in related:
            owners = sorted(int(grow[i]) for i in range(len(ids)) if alive[i] and node_of[i] == v)
            rel.append((names[v], int(F32(s).view(U32)), ids[slot_of_row[owners[0]]] if owners else None))
        out.append(([(ids[slot_of_row[row]], int(F32(f).view(U32)), int(F32(c).view(U32)), int(F32(g).view(U32))) for row, f, c, g in hits], rel))
    return out


def _got(res, ids_of_payload):
    bits = lambda x: int(F32(x).view(U32))                                           # noqa: E731
    return [([(h["id"], bits(h["score"]), bits(h["cosine"]), bits(h["graph_score"])) for h in one["hits"]],
             [(r["node"], bits(r["graph_score"]), ids_of_payload(r["payload"])) for r in one["related"]]) for one in res]


@pytest.mark.parametrize("shards", [1, 2])
def test_store_over_the_fakes(monkeypatch, shards):
    store = _store(monkeypatch)
    ids, pay = (list(x) for x in zip(*[_point(i) for i in range(N)]))
    rng = np.random.default_rng(11)
    vecs, q = rng.standard_normal((N, DIM)).astype(F32), rng.standard_normal((3, DIM)).astype(F32)
    by_line = {p["start_line"]: i for i, p in zip(ids, pay)}
    id_of = lambda p: None if p is None else by_line[p["start_line"]]               # noqa: E731

    async def run():
        async with _open(store, shards) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, vecs, pay)
            await s.set_graph_edges("code_chunks", EDGES)
            col = s._col("code_chunks")
            names, alive = _names(EDGES), np.ones(N, bool)
            edges = [e for e in EDGES if e[0] != e[1]]

            # the defaults: candidates = 4 * limit, both directions, restart 0.15, 16 steps, cosine weights, rrf_k 60
            got = await s.search_propagated_batch("code_chunks", q, limit=5, related_limit=4)
            assert _got(got, id_of) == _want(store, col, ids, pay, vecs, q, alive, names, edges, 5, 20, 4)
            assert pc.FakeGraph.ppr_calls == 1 == col.graph_ppr_calls and all(len(o["hits"]) == 5 and o["related"] for o in got)
            assert any(h["graph_score"] > 0 for o in got for h in o["hits"])
            one = await s.search_propagated("code_chunks", q[1].tolist(), limit=5, related_limit=4)
            assert _got([one], id_of) == _got(got[1:2], id_of)
            # every setting, a filter, no related list
            prop = {"direction": "callees", "restart": 0.3, "steps": 3, "seed_weight": "uniform", "rrf_k": 7}
            got = await s.search_propagated_batch("code_chunks", q, limit=4, candidates=9, propagate=prop, related_limit=0, filters={"language": "go"})
            lang = np.asarray([p["language"] == "go" for p in pay])
            assert _got(got, id_of) == _want(store, col, ids, pay, vecs, q, alive, names, edges, 4, 9, 0, mask=lang, **prop)
            assert await s.search_propagated("code_chunks", q[0].tolist(), filters={"language": "cobol"}) == {"hits": [], "related": []}

            # refusals, by name
            for kw, word in (({"diversity": 0.5}, "diversity"), ({"group_by": "file_path"}, "group_by"), ({"max_overlap": 0.2}, "max_overlap"),
                             ({"score_threshold": 0.1}, "score_threshold"), ({"filters": [None, None, None]}, "per-query filter lists"),
                             ({"propagate": {"hops": 2}}, "hops"), ({"propagate": {"steps": 65}}, "steps"), ({"propagate": {"restart": 1.0}}, "restart"),
                             ({"propagate": {"direction": "sideways"}}, "direction"), ({"propagate": {"seed_weight": "bm25"}}, "seed_weight"),
                             ({"propagate": {"relation": "imports"}}, "imports"), ({"candidates": 3, "limit": 5}, "candidates"),
                             ({"candidates": 513}, "candidates"), ({"related_limit": -1}, "related_limit")):
                with pytest.raises(store.VectorStoreError) as e:
                    await s.search_propagated_batch("code_chunks", q, **kw)
                assert word in str(e.value.cause), kw
            with pytest.raises(store.VectorStoreError) as e:
                monkeypatch.setattr(s, "_shard_backend", "dist")
                try:
                    await s.search_propagated_batch("code_chunks", q)
                finally:
                    monkeypatch.setattr(s, "_shard_backend", "local")
            assert "dist" in str(e.value.cause)

            # graph_rank: names, weights, a name that is no node, 65 sets in two passes
            numbered = [(names.index(a), names.index(b)) for a, b in edges]
            fwd, rev = pc.graph_lists(len(names), numbered)

            def ranked(seeds, weights, limit, direction="both", exclude=None, **kw):
                scores = pc.ppr(fwd, rev, direction, seeds, weights, kw.get("restart", 0.15), kw.get("steps", 16))
                nodes, vals = pc.top_list(scores, limit, exclude)
                return [[(names[v], int(F32(x).view(U32))) for v, x in zip(nodes[i], vals[i]) if v >= 0] for i in range(len(seeds))]

            def shown(res):
                return [(h["node"], int(F32(h["graph_score"]).view(U32))) for h in res["hits"]]

            before = pc.FakeGraph.ppr_calls
            res = await s.graph_rank("code_chunks", ["pkg.fn3", "nobody"], limit=6)
            at3 = names.index("pkg.fn3")
            assert shown(res) == ranked([[at3]], [[1.0]], 6)[0] and res["unresolved"] == ["nobody"] and res["hits"][0]["node"] == "pkg.fn3"
            assert pc.FakeGraph.ppr_calls == before + 1
            for h in res["hits"]:                                                   # the payload of the node's first alive chunk, or None
                owners = [i for i in range(N) if _key(pay[i]) == h["node"]]
                assert (h["payload"] is None) == (not owners) and (not owners or h["payload"]["start_line"] == pay[owners[0]]["start_line"])
            assert any(h["payload"] is None for h in res["hits"]) or "ghost" not in [h["node"] for h in res["hits"]]
            res = await s.graph_rank("code_chunks", ["pkg.fn3", "pkg.fn8"], weights=[1.0, 3.0], direction="callers", restart=0.4, steps=5, limit=4,
                                     include_seeds=False)
            want = ranked([[at3, names.index("pkg.fn8")]], [[1.0, 3.0]], 4, "callers", exclude=[[at3, names.index("pkg.fn8")]], restart=0.4, steps=5)[0]
            assert shown(res) == want and want and not {"pkg.fn3", "pkg.fn8"} & {n for n, _ in want}
            res = await s.graph_rank("code_chunks", "fn8", match="suffix", limit=3)    # "fn8" and "pkg.fn8"
            two = sorted([names.index("fn8"), names.index("pkg.fn8")])
            assert shown(res) == ranked([[names.index("fn8"), names.index("pkg.fn8")]], [[1.0, 1.0]], 3)[0] == ranked([two], [[1.0, 1.0]], 3)[0]
            assert (await s.graph_rank("code_chunks", "nobody")) == {"hits": [], "unresolved": ["nobody"]}
            sets = [[names[i % len(names)]] for i in range(65)]
            before = pc.FakeGraph.ppr_calls
            many = await s.graph_rank_batch("code_chunks", sets, limit=3)
            assert pc.FakeGraph.ppr_calls == before + 2
            assert [shown(r) for r in many] == ranked([[i % len(names)] for i in range(65)], None, 3)
            for kw, word in (({"weights": [-1.0]}, "weights"), ({"weights": [1.0, 2.0]}, "weights"), ({"steps": 0}, "steps"), ({"limit": 0}, "limit"),
                             ({"direction": "up"}, "direction"), ({"relation": "imports"}, "imports"), ({"match": "fuzzy"}, "match")):
                with pytest.raises(store.VectorStoreError) as e:
                    await s.graph_rank("code_chunks", ["pkg.fn3"], **kw)
                assert word in str(e.value.cause), kw

            # a delete, then compact: rows are renumbered, the answer follows the alive rows only
            await s.delete("code_chunks", {"file_path": "src/m1.py"})
            for i, p in enumerate(pay):
                alive[i] = p["file_path"] != "src/m1.py"
            got = await s.search_propagated_batch("code_chunks", q, limit=5, related_limit=6)
            assert _got(got, id_of) == _want(store, col, ids, pay, vecs, q, alive, names, edges, 5, 20, 6)
            await s.compact("code_chunks")
            kept = [i for i in range(N) if alive[i]]
            ids2, pay2, vecs2 = [ids[i] for i in kept], [pay[i] for i in kept], vecs[kept]
            got = await s.search_propagated_batch("code_chunks", q, limit=5, related_limit=6)
            assert _got(got, id_of) == _want(store, col, ids2, pay2, vecs2, q, np.ones(len(kept), bool), names, edges, 5, 20, 6)

            # a replaced relation: the walk follows the new edges; another relation is left alone
            await s.set_graph_edges("code_chunks", [("pkg.fn7", "pkg.fn3"), ("pkg.fn3", "pkg.fn9")])
            await s.set_graph_edges("code_chunks", [("pkg.fn12", "pkg.fn3")], relation="extends")
            names2 = names + ["pkg.fn12"]
            got = await s.search_propagated_batch("code_chunks", q, limit=5, related_limit=6)
            assert _got(got, id_of) == _want(store, col, ids2, pay2, vecs2, q, np.ones(len(kept), bool), names2,
                                             [("pkg.fn7", "pkg.fn3"), ("pkg.fn3", "pkg.fn9")], 5, 20, 6)
            res = await s.graph_rank("code_chunks", "pkg.fn3", relation="extends", include_seeds=False)
            assert [h["node"] for h in res["hits"]] == ["pkg.fn12"]
    asyncio.run(run())


# ---------------------------------------------------------------------------------------------------- the surfaces
class _Recorder:
    """A store that records what the searcher sends and answers with canned results."""
    def __init__(self):
        self.calls = []

    async def search(self, **kw):
        self.calls.append(("search", kw))
        return []

    async def search_propagated(self, **kw):
        self.calls.append(("search_propagated", kw))
        pay = {"file_path": "a.py", "entity_type": "function", "entity_name": "f", "language": "python", "content": "x", "start_line": 3,
               "end_line": 5, "graph_node_id": "pkg.f"}
        return {"hits": [{"id": "1", "score": 0.03, "cosine": 0.8, "graph_score": 0.25, "payload": pay}],
                "related": [{"node": "pkg.core.send", "graph_score": 0.125, "payload": dict(pay, file_path="core.py", start_line=40)},
                            {"node": "ghost", "graph_score": 0.0625, "payload": None}][: kw["related_limit"]]}

    async def graph_rank(self, **kw):
        self.calls.append(("graph_rank", kw))
        return {"hits": [{"node": "pkg.core.send", "graph_score": 0.5, "payload": {"file_path": "core.py", "entity_type": "function", "start_line": 40}}],
                "unresolved": []}


class _Embedder:
    async def embed(self, text):
        return [0.0] * 4


def test_searcher_and_mcp_surfaces():
    import coderag_amd  # noqa: F401
    from coderag_amd import mcp_tools
    from coderag_amd.errors import QueryError
    from coderag_amd.vector_search import VectorSearcher

    async def run():
        rec = _Recorder()
        vs = VectorSearcher(rec, _Embedder())
        await vs.search_code("retry handling")
        assert rec.calls[-1][0] == "search" and set(rec.calls[-1][1]) == {"collection", "query_vector", "limit", "filters"}   # the call of before
        rows = await vs.search_code("retry handling", limit=3, language="python", propagate=True)
        assert rec.calls[-1] == ("search_propagated", {"collection": "code_chunks", "query_vector": [0.0] * 4, "limit": 3, "candidates": None,
                                                       "propagate": None, "related_limit": 0, "filters": {"language": "python"}})
        assert rows == [{"score": 0.03, "file_path": "a.py", "entity_type": "function", "entity_name": "f", "language": "python", "content": "x",
                         "start_line": 3, "end_line": 5, "graph_node_id": "pkg.f", "cosine": 0.8, "graph_score": 0.25}]
        await vs.search_code("retry handling", propagate={"steps": 4}, candidates=30, within_callees_of="main")
        assert rec.calls[-1][1]["propagate"] == {"steps": 4} and rec.calls[-1][1]["candidates"] == 30
        assert rec.calls[-1][1]["filters"] == {"graph": {"callees_of": "main"}}
        both = await vs.search_code_propagated("retry handling", related_limit=2)
        assert both["results"] == rows and both["related"] == [
            {"name": "send", "qualified_name": "pkg.core.send", "graph_score": 0.125, "file_path": "core.py", "entity_type": "function", "start_line": 40},
            {"name": "ghost", "qualified_name": "ghost", "graph_score": 0.0625, "file_path": None, "entity_type": None, "start_line": None}]
        for kw, word in (({"diversity": 0.5}, "diversity"), ({"max_per_file": 2}, "max_per_file"), ({"extra_queries": ["x"]}, "extra_queries"),
                         ({"min_score": 0.2}, "min_score"), ({"max_overlap": 0.5}, "max_overlap"), ({"mode": "hybrid"}, "hybrid")):
            with pytest.raises(ValueError) as e:
                await vs.search_code("retry handling", propagate=True, **kw)
            assert word in str(e.value)
        with pytest.raises(QueryError):
            await vs.search_code("  ", propagate=True)
        near = await vs.find_important_near("handle_request", limit=4)
        assert rec.calls[-1] == ("graph_rank", {"collection": "code_chunks", "names": ["handle_request"], "weights": None, "direction": "both",
                                                "restart": 0.15, "steps": 16, "limit": 4, "match": "exact", "include_seeds": False})
        assert near == [{"name": "send", "qualified_name": "pkg.core.send", "graph_score": 0.5, "file_path": "core.py", "entity_type": "function",
                         "start_line": 40}]
        with pytest.raises(QueryError):
            await vs.find_important_near([])

        search = mcp_tools.create_semantic_search_tool(lambda: vs)
        res = await search["function"]("retry handling", limit=2, rank="propagated", contains="retry")
        assert res.success and rec.calls[-1][0] == "search_propagated" and rec.calls[-1][1]["filters"] == {"content": {"contains": "retry"}}
        assert [r["qualified_name"] for r in res.data] == ["pkg.f"] and res.data[0]["score"] == 0.03 and "pkg.core.send, ghost" in res.message
        assert not (await search["function"]("retry handling", rank="propagated", diversity=0.3)).success
        assert not (await search["function"]("retry handling", rank="propagated", entities=["f"])).success
        assert not (await search["function"]("retry handling", rank="walked")).success
        assert (await search["function"]("retry handling")).success and rec.calls[-1][0] == "search"
        tool = mcp_tools.create_code_graph_tool(lambda: vs)
        assert "op" in tool["parameters"]
        res = await tool["function"]("handle_request", op="important_near", limit=3)
        assert res.success and res.data == [dict(near[0])] and rec.calls[-1][1]["limit"] == 3 and rec.calls[-1][1]["names"] == ["handle_request"]
        assert not (await tool["function"]("handle_request", op="important_far")).success
        assert not (await tool["function"]("handle_request", op="important_near", target="x")).success
    asyncio.run(run())
