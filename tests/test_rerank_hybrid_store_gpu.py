"""The hybrid re-rank through the store (search_rerank_hybrid_batch / search_and_rank_hybrid_batch_device): search,
BFS, list, candidates, gathers and re-rank on the device against HybridRanker.rank_results on a GraphContext built here from the
deque BFS of tests/graph_cases.py and the representative rows' payloads.  Exact: order, f64 score bits, sources, signals."""
import asyncio
from types import SimpleNamespace as NS

import numpy as np
import pytest

from tests import graph_cases as gc

pytestmark = pytest.mark.gpu

N_NODES, N_ROWS, DIM, LIMIT = 300, 2000, 384, 20
SIGNALS = ("graph_match", "query_entity_match", "relationship_relevance", "centrality", "context_richness", "vector_similarity", "code_quality")


def _payloads():
    out = []
    for i in range(N_ROWS):
        v = i % N_NODES if i < 1800 else None                       # six rows per node, 200 rows that are no node
        name = f"n{v}" if v is not None else f"free{i}"
        p = {"file_path": f"src/m{(i * 7) % 23}.py", "entity_name": name, "entity_type": "class" if v is not None and v % 5 == 0 else "function",
             "language": "python", "content": "x" * (40 + (i * 37) % 300), "start_line": i, "end_line": i + 9, "project_name": "p"}
        if v is not None and i % 3:
            p["graph_node_id"] = name
        if i % 2:
            p["summary"] = f"sum {i}"
        if i % 3 == 0:
            p["docstring"] = "Doc."
        if i % 4 == 0:
            p["signature"] = f"def {name}()"
        out.append(p)
    return out


def _numbered(edge_lists):
    """Node names in order of first appearance over the relations, as set_graph_edges numbers them."""
    number = {}
    for edges in edge_lists:
        for a, b in edges:
            for v in (a, b):
                number.setdefault(f"n{v}", len(number))
    return number


@pytest.mark.parametrize("shards", [1, 2])
def test_store_hybrid_rerank_end_to_end(gpu, shards):
    import coderag_amd  # noqa: F401
    from coderag_amd.engine_helpers import centrality_candidates, search_and_rank_batch_device, search_and_rank_hybrid_batch_device
    from coderag_amd.query_types import GraphContext, GraphNode
    from coderag_amd.ranking import HybridRanker
    from coderag_amd.ranking.device import DeviceReranker, HybridDeviceReranker
    from coderag_amd.shards import STRIDE
    from coderag_amd.store import HipVectorStore
    from coderag_amd.vector_search import _CODE_KEYS, _project

    pay = _payloads()
    rng = np.random.default_rng(17)
    raw = rng.standard_normal((N_ROWS, DIM)).astype(np.float32)
    ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(N_ROWS)]
    _, calls = gc.random_graph(N_NODES, 5, mean_degree=2, hubs=2, hub_degree=70)
    calls = [(a, b) for a, b in calls if a != b]
    extends = [(v, v - 5) for v in range(5, N_NODES, 5)] + [(v, 0) for v in range(50, N_NODES, 50)]      # classes only (v % 5 == 0)
    number = _numbered([calls, extends])
    names = list(number)
    rel = {"calls": [(number[f"n{a}"], number[f"n{b}"]) for a, b in calls], "extends": [(number[f"n{a}"], number[f"n{b}"]) for a, b in extends]}
    qv = raw[[3, 40, 77, 512, 900, 1300, 1801, 1999]] + 0.4 * rng.standard_normal((8, DIM)).astype(np.float32)

    def plan(intent, ents, multi=False, hops=1):
        return NS(primary_intent=intent, entities=[NS(name=e, is_primary=True) for e in ents], requires_multi_hop=multi, max_hops=hops)
    plans = [plan("find_callers", ["n7"], True, 3), plan("find_callees", ["n7", "n12"], True, 2), plan("find_hierarchy", ["n50", "n7"]),
             plan("search_functionality", ["n1", "n2", "n3", "n4"]), plan("find_usages", ["nowhere"]), plan("explain_implementation", ["n10"]),
             plan("find_callers", [names[0]], True, 5), plan("locate_entity", [])]

    def walks(p):
        """Hand-written per intent: (attribute, relation, direction, hops, limit, the primaries it applies to)."""
        prim = [number[e.name] for e in p.entities if e.name in number]
        is_class = lambda v: int(names[v][1:]) % 5 == 0
        it, h = p.primary_intent, (min(p.max_hops, 5) if p.requires_multi_hop else 1)
        if it in ("find_callers", "find_usages"):
            return prim, [("callers", "calls", "callers", h, 50, prim)]
        if it == "find_callees":
            return prim, [("callees", "calls", "callees", h, 50, prim)]
        if it == "find_hierarchy":
            return prim, [("callers", "calls", "callers", h, 50, [v for v in prim if not is_class(v)]),
                          ("parent_classes", "extends", "callees", 5, 50, [v for v in prim if is_class(v)]),
                          ("child_classes", "extends", "callers", 5, 50, [v for v in prim if is_class(v)])]
        if it == "explain_implementation":
            return prim, [("callers", "calls", "callers", 1, 10, prim), ("callees", "calls", "callees", 1, 10, prim)]
        return prim, [("callers", "calls", "callers", 2, 10, prim[:3]), ("callees", "calls", "callees", 2, 10, prim[:3])]

    async def expected(s, col, alive):
        """HybridRanker on the restated GraphContext and the store's own hit lists."""
        key = [p.get("graph_node_id") or p["entity_name"] for p in pay]
        slot_of_id = {col.ids.get(t): t for t in range(col.ids.n)}
        # representative row: the lowest alive GLOBAL row (shard * STRIDE + local; with one shard the slot itself) of the node
        rep = {}
        for i in np.flatnonzero(alive):
            t = slot_of_id[ids[i]]
            g = int(t) if shards == 1 else int(col.row_shard[t]) * STRIDE + int(col.row_local[t])
            if key[i] in number and (key[i] not in rep or g < rep[key[i]][0]):
                rep[key[i]] = (g, i)

        def node(v, depth=None):
            p = pay[rep[names[v]][1]]
            return GraphNode(node_type=p["entity_type"], name=p["entity_name"], qualified_name=names[v], file_path=p["file_path"],
                             signature=p.get("signature"), docstring=p.get("docstring"), summary=p.get("summary"), start_line=p["start_line"],
                             end_line=p["end_line"], metadata={} if depth is None else {"depth": depth})
        lists = await s.search_batch("code_chunks", qv, LIMIT, {"language": "python"})
        deg = col._degrees or {}
        want = []
        for p, hits in zip(plans, lists):
            prim, ws = walks(p)
            ctx = GraphContext(primary_entities=[node(v) for v in prim if names[v] in rep])
            for attr, r, direction, hops, limit, sources in ws:
                for v in sources:
                    depth = gc.bfs_depths(len(names), rel[r], direction, [v], hops)
                    order = sorted((d, u) for u, d in depth.items() if d > 0)[:limit]
                    getattr(ctx, attr).extend(node(u, d if attr in ("callers", "callees") else None) for d, u in order if names[u] in rep)
            flat = [_project(h, _CODE_KEYS) for h in hits]
            cand = centrality_candidates(ctx, flat)
            want.append(HybridRanker().rank_results(p, ctx, flat, {n: {"total_degree": deg[n]} for n in cand if n in deg}))
        return want

    def same(got, want):
        assert len(got) == len(want) == len(plans)
        seen = set()
        for q, (g, w) in enumerate(zip(got, want)):
            assert [(r.file_path, r.entity_name, r.start_line, r.final_score, r.source, r.relationship_path, r.depth_from_query, r.graph_node_id) for r in g] == \
                   [(r.file_path, r.entity_name, r.start_line, r.final_score, r.source, r.relationship_path, r.depth_from_query, r.graph_node_id) for r in w], q
            assert [r.signal_scores for r in g] == [r.signal_scores for r in w], q
            assert [(r.content, r.summary, r.signature, r.docstring) for r in g] == [(r.content, r.summary, r.signature, r.docstring) for r in w], q
            seen.update((r.source, r.relationship_path) for r in g)
        return seen

    async def run():
        async with HipVectorStore(dim=DIM, dtype="bf16", initial_capacity=1024, device=0, shards=shards, compact_dead_fraction=0.0) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, raw, pay)
            col = s._col("code_chunks")
            await s.set_graph_edges("code_chunks", [(f"n{a}", f"n{b}") for a, b in calls], derive_degrees=True)
            await s.set_graph_edges("code_chunks", [(f"n{a}", f"n{b}") for a, b in extends], relation="extends")
            assert list(col._graph_names) == names
            alive = np.ones(N_ROWS, bool)
            for i in [7, 12, 50, 307, 1, 2] + list(range(100, 160)):            # tombstoned FIRST rows: the representative moves on
                await s.delete("code_chunks", {"start_line": i})
                alive[i] = False
            vec_plans = [NS(primary_intent=p.primary_intent, entities=p.entities) for p in plans]
            before = await search_and_rank_batch_device(s, DeviceReranker(), HybridRanker(), qv, vec_plans, limit=LIMIT, language="python")
            rr = HybridDeviceReranker()
            got = await search_and_rank_hybrid_batch_device(s, rr, HybridRanker(), qv, plans, limit=LIMIT, language="python")
            seen = same(got, await expected(s, col, alive))
            assert {("graph", None), ("graph", "caller"), ("graph", "callee"), ("graph", "parent_class"), ("graph", "child_class"), ("vector", None)} <= seen
            assert any(src == "hybrid" for src, _ in seen)
            assert [len(r) for r in got][4] == [len(r) for r in before][4]          # no primary resolves: the vector ranking alone
            builds = col.graph_node_rows_builds
            await search_and_rank_hybrid_batch_device(s, rr, HybridRanker(), qv, plans, limit=LIMIT, language="python")
            assert col.graph_node_rows_builds == builds                              # kept: nothing changed
            after = await search_and_rank_batch_device(s, DeviceReranker(), HybridRanker(), qv, vec_plans, limit=LIMIT, language="python")
            assert [[(r.file_path, r.start_line, r.final_score, r.source) for r in x] for x in before] == \
                   [[(r.file_path, r.start_line, r.final_score, r.source) for r in x] for x in after]
            # a delete and a compaction: the representative rows are rebuilt, the rows renumbered
            for i in (13, 313, 613, 913, 1213, 1513):                                # every row of n13: the node leaves the results
                await s.delete("code_chunks", {"start_line": i})
                alive[i] = False
            assert await s.compact("code_chunks") > 0
            got = await search_and_rank_hybrid_batch_device(s, rr, HybridRanker(), qv, plans, limit=LIMIT, language="python")
            assert col.graph_node_rows_builds > builds
            same(got, await expected(s, col, alive))
            assert not any(r.graph_node_id == "n13" and r.source == "graph" for x in got for r in x)
    asyncio.run(run())


def test_hybrid_route_refuses_dist(gpu):
    import coderag_amd  # noqa: F401
    from coderag_amd.errors import VectorStoreError
    from coderag_amd.store import _Collection
    col = _Collection.__new__(_Collection)
    col.name, col._graph_rel, col._graph = "code_chunks", {"calls": np.zeros((0, 2), np.int32)}, None
    col.shards = NS(backend="dist")
    with pytest.raises(VectorStoreError, match="dist"):
        col.search_rerank_hybrid(np.zeros((1, DIM), np.float32), [NS(primary_intent="find_callers", entities=[])], None, 5, None, "calls")
