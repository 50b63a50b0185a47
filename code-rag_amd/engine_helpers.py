"""The two behaviours of ``QueryEngine`` that shape what reaches the ranker, restated as free functions
(``src/lattice/query/engine.py:315-377``).  The engine itself (LLM planning, Memgraph, response writing) is
out of scope; these helpers let a batch harness feed the ranker exactly what the reference would."""

from __future__ import annotations

import asyncio
from typing import Any, Awaitable, Callable, NamedTuple

from .ffi import ROLE_CALLEE, ROLE_CALLER, ROLE_CHILD, ROLE_METHOD, ROLE_PARENT, ROLE_PRIMARY
from .query_types import QueryIntent, intent_key
from .settings import get_settings

_SUMMARY_INTENTS = {i.value for i in (QueryIntent.EXPLAIN_IMPLEMENTATION, QueryIntent.EXPLAIN_RELATIONSHIP,
                                      QueryIntent.EXPLAIN_DATA_FLOW, QueryIntent.EXPLAIN_ARCHITECTURE,
                                      QueryIntent.SEARCH_FUNCTIONALITY)}


async def execute_vector_search(vector_searcher, query: str, plan, limit: int, language: str | None,
                                project_name: str | None = None) -> list[dict[str, Any]]:
    """engine.py:315-346: code hits capped at ``max_vector_results``; explanatory/functional intents also get
    ``limit // 2`` summary hits appended."""
    cap = get_settings().max_vector_results
    results = await vector_searcher.search_code(query=query, limit=min(limit, cap), language=language, project_name=project_name)
    if intent_key(plan.primary_intent) in _SUMMARY_INTENTS:
        results.extend(await vector_searcher.search_summaries(query=query, limit=limit // 2, project_name=project_name))
    return results


MAX_QUERY_TEXTS = 16      # CRH_MAX_LISTS: the lists one fusion takes


def plan_query_texts(plan, original: str) -> list[str]:
    """The texts one fused vector search asks (``VectorSearcher.search_code(texts[0], extra_queries=texts[1:])``): the original
    query, then the distinct non-empty ``query_text`` of the plan's sub-queries whose ``search_type`` is "vector" or "hybrid"
    (query/query_planner.py:66-91; lower ``priority`` first, the plan's order among equals), at most 16 in all.  The
    reference's engine plans them and then searches the original text only (query/engine.py:315-346)."""
    texts = [original]
    seen = {original.strip()}
    subs = [sq for sq in (getattr(plan, "sub_queries", None) or []) if str(_field(sq, "search_type", "")).lower() in ("vector", "hybrid")]
    for sq in sorted(subs, key=lambda sq: _field(sq, "priority", 1)):           # (sorted is stable)
        text = _field(sq, "query_text", None)
        if not isinstance(text, str) or not text.strip() or text.strip() in seen:
            continue
        if len(texts) == MAX_QUERY_TEXTS:
            break
        seen.add(text.strip())
        texts.append(text)
    return texts


def _field(obj, name: str, default):
    """A sub-query's field, whether the planner left a dataclass or the parsed JSON object."""
    return obj.get(name, default) if isinstance(obj, dict) else getattr(obj, name, default)


def centrality_candidates(graph_context, vector_results: list[dict[str, Any]]) -> list[str]:
    """engine.py:353-363: names of <= 5 primary graph entities and of the first 5 vector hits (graph node id, else
    entity name), de-duplicated, truncated to ``max_centrality_lookups``.  (The reference iterates a ``set``, so
    which names survive the truncation is hash-order dependent there; insertion order is used here.)"""
    names: dict[str, None] = {}
    for node in graph_context.primary_entities[:5]:
        names[node.qualified_name or node.name] = None
    for hit in vector_results[:5]:
        if hit.get("entity_name"):
            names[hit.get("graph_node_id") or hit.get("entity_name")] = None
    return list(names)[: get_settings().max_centrality_lookups]


async def get_centrality_scores(lookup: Callable[[str], Awaitable[dict[str, int]]], graph_context,
                                vector_results: list[dict[str, Any]]) -> dict[str, dict[str, int]]:
    """engine.py:348-377: one degree lookup per candidate, failures dropped."""
    names = centrality_candidates(graph_context, vector_results)
    if not names:
        return {}
    answers = await asyncio.gather(*(lookup(n) for n in names), return_exceptions=True)
    return {n: a for n, a in zip(names, answers) if isinstance(a, dict)}


async def search_and_rank_batch(vector_searcher, ranker, queries, plans, graph_contexts=None, centrality=None,
                                limit: int = 20, language: str | None = None, project_name: str | None = None):
    """BASELINE config 5 in one call: ONE batched corpus scan for all queries (``search_code_batch``), then the hybrid
    re-rank of each query's merged top-k exactly as ``QueryEngine.search`` would do it one query at a time
    (engine.py:222-260: vector limit capped at ``max_vector_results``, then ``HybridRanker.rank_results``).
    ``queries`` are strings or ready vectors; ``plans[i]`` / ``graph_contexts[i]`` / ``centrality[i]`` belong to query i."""
    from .query_types import GraphContext
    cap = get_settings().max_vector_results
    per_query = await vector_searcher.search_code_batch(queries, limit=min(limit, cap), language=language, project_name=project_name)
    ranked = []
    for i, hits in enumerate(per_query):
        ctx = graph_contexts[i] if graph_contexts is not None and graph_contexts[i] is not None else GraphContext()
        ranked.append(ranker.rank_results(plans[i], ctx, hits, (centrality[i] if centrality is not None else None)))
    return ranked


async def search_and_rank_batch_device(store, reranker, host_ranker, query_vectors, plans, limit: int = 20,
                                       language: str | None = None, project_name: str | None = None):
    """:func:`search_and_rank_batch` for vector-only queries with the re-rank on the device: ONE corpus scan, one
    ``crh_rerank_vector`` launch for the whole batch, and payload dictionaries touched only for the <= 50 survivors of each
    query.  A query the device declines (``count == -1``: more than 8 plan entities, an over-long name) goes through
    ``host_ranker`` on its full hit list, so results equal :func:`search_and_rank_batch` in every case."""
    from .query_types import GraphContext
    from .ranking.device import DeviceReranker
    from .store import CollectionName
    from .vector_search import _CODE_KEYS, _project
    cap = get_settings().max_vector_results
    filters = {k: v for k, v in (("language", language), ("project_name", project_name)) if v}
    col, out, rows, scores = await store.search_rerank_batch(CollectionName.CODE_CHUNKS.value, query_vectors, plans, reranker,
                                                             limit=min(limit, cap), filters=filters or None)

    class _Hits:   # candidate position -> the flattened hit dict of query/vector_search.py:111-131, built on demand
        def __init__(self, q):
            self.q = q

        def __getitem__(self, i):
            return _project(col.hit(int(rows[self.q, i]), float(scores[self.q, i])), _CODE_KEYS)

    ranked = []
    for q in range(len(plans)):
        if out.count[q] >= 0:
            ranked.append(DeviceReranker.materialise(out, q, _Hits(q)))
            continue
        hits = [_project(col.hit(int(r), float(s)), _CODE_KEYS) for r, s in zip(rows[q], scores[q]) if r >= 0]
        names = centrality_candidates(GraphContext(), hits)
        deg = col._degrees or {}
        ranked.append(host_ranker.rank_results(plans[q], GraphContext(), hits, {n: {"total_degree": deg[n]} for n in names if n in deg}))
    return ranked


# ---- the graph branch of QueryEngine.search with the call graph on the device
MAX_TRAVERSAL_DEPTH = 5        # graph_reasoning/models.py:5
MAX_RESULTS_PER_QUERY = 50     # graph_reasoning/models.py:6: the per-source limit of a traversal
_CALLER_INTENTS = {QueryIntent.FIND_CALLERS.value, QueryIntent.FIND_USAGES.value}
_HIERARCHY_INTENTS = {QueryIntent.FIND_HIERARCHY.value, QueryIntent.FIND_IMPLEMENTATIONS.value}
_PRIMARY_ONLY_INTENTS = {QueryIntent.FIND_CALL_CHAIN.value, QueryIntent.FIND_DEPENDENCIES.value, QueryIntent.FIND_DEPENDENTS.value}


class GraphWalk(NamedTuple):
    """One traversal of the reference's graph engine: the nodes within ``hops`` edges of ``source`` along ``relation`` in
    ``direction`` ("callers": against the edges, "callees": along them), the first ``limit`` of them, become results in ``role``."""
    role: int
    relation: str
    direction: str
    source: int
    hops: int
    limit: int


class GraphRolePlan(NamedTuple):
    primaries: list        # node ids, in the order (and with the repeats) the reference collects them
    walks: list            # GraphWalk, in the order the reference extends each role's list


def plan_graph_roles(plan, graph_info) -> GraphRolePlan:
    """``GraphReasoningEngine.execute_query_plan`` (graph_reasoning/engine.py:25-84, 329-452) limited to what the ranker reads:
    which nodes are primary entities and which traversals fill callers / callees / methods / parent / child classes.

    ``graph_info`` answers for the collection's graph: ``resolve(name, match) -> [node ids]`` (``graph.resolve``),
    ``relations`` (the names it holds) and ``is_class(node) -> bool``.  Primaries (engine.py:44-47): every entity that is
    marked primary, or any entity while there is none yet, resolved ``"exact"`` first and ``"suffix"`` when nothing matches
    exactly (the reference matches ``name`` OR ``qualified_name``; a node here has one name).  Its fuzzy CONTAINS fallback
    (engine.py:49-52) is not restated.  Then, by intent:

    * callers / usages (:329-345): per primary, callers within ``plan.max_hops`` when the plan is multi-hop, else 1;
    * callees (:347-363): likewise along the edges;
    * hierarchy / implementations (:372-396): a class gives its ancestors and descendants over ``"extends"`` within 5 (queries.py:
      91-92; nothing when the collection has no such relation), anything else its callers;
    * explain_implementation (:398-413): the direct callers and callees, 10 each (queries.py:192-209), and a class's methods;
    * call chain, dependencies, dependents: primaries only (paths and file context are not ranked);
    * everything else (:423-452): the first 3 primaries, callers and callees within 2 hops, 10 each, and a class's methods.

    Hops are clipped at 5, a traversal yields at most 50 nodes (:92, :111).  Methods need a ``"has_method"`` relation.

    Differences: a multi-hop plan with ``max_hops`` < 1 walks 1 hop here (the reference formats the number into
    ``*1..{max_hops}`` as it is, which matches nothing; ``crh_graph_bfs`` takes 1..16).  Where the reference walks from the
    plan's entity NAMES -- when nothing resolved (:339-345, :357-363), and under the hierarchy intents for every plan entity that is
    not among the resolved names even when others resolved (:387-396) -- nothing is walked here: a name that is no node has no
    callers in this graph."""
    relations = graph_info.relations
    primaries: list[int] = []
    for entity in plan.entities:
        if getattr(entity, "is_primary", False) or not primaries:
            primaries.extend(graph_info.resolve(entity.name, "exact") or graph_info.resolve(entity.name, "suffix"))
    intent = intent_key(plan.primary_intent)
    hops = min(int(plan.max_hops) if getattr(plan, "requires_multi_hop", False) else 1, MAX_TRAVERSAL_DEPTH)
    hops = max(hops, 1)
    walks: list[GraphWalk] = []

    def calls(role, direction, node, h, limit):
        if "calls" in relations:
            walks.append(GraphWalk(role, "calls", direction, node, h, limit))

    def methods(node):
        if "has_method" in relations and graph_info.is_class(node):
            walks.append(GraphWalk(ROLE_METHOD, "has_method", "callees", node, 1, MAX_RESULTS_PER_QUERY))

    if intent in _CALLER_INTENTS:
        for v in primaries:
            calls(ROLE_CALLER, "callers", v, hops, MAX_RESULTS_PER_QUERY)
    elif intent == QueryIntent.FIND_CALLEES.value:
        for v in primaries:
            calls(ROLE_CALLEE, "callees", v, hops, MAX_RESULTS_PER_QUERY)
    elif intent in _PRIMARY_ONLY_INTENTS:
        pass
    elif intent in _HIERARCHY_INTENTS:
        for v in primaries:
            if graph_info.is_class(v):
                if "extends" in relations:
                    walks.append(GraphWalk(ROLE_PARENT, "extends", "callees", v, MAX_TRAVERSAL_DEPTH, MAX_RESULTS_PER_QUERY))
                    walks.append(GraphWalk(ROLE_CHILD, "extends", "callers", v, MAX_TRAVERSAL_DEPTH, MAX_RESULTS_PER_QUERY))
            else:
                calls(ROLE_CALLER, "callers", v, hops, MAX_RESULTS_PER_QUERY)
    elif intent == QueryIntent.EXPLAIN_IMPLEMENTATION.value:
        for v in primaries:
            calls(ROLE_CALLER, "callers", v, 1, 10)
            calls(ROLE_CALLEE, "callees", v, 1, 10)
            methods(v)
    else:
        for v in primaries[:3]:
            calls(ROLE_CALLER, "callers", v, 2, 10)
            calls(ROLE_CALLEE, "callees", v, 2, 10)
            methods(v)
    return GraphRolePlan(primaries, walks)


def _graph_item(hits, names, node: int) -> dict[str, Any]:
    """A graph result's fields: the payload of the node's representative row, ``graph_node_id`` = the node's name."""
    name, slot = names[int(node)]
    payload = hits.hit(slot, 0.0)["payload"] or {}
    item = {k: payload.get(k) for k in ("file_path", "entity_name", "entity_type", "start_line", "end_line", "summary", "signature", "docstring")}
    item["file_path"], item["entity_name"], item["entity_type"] = item["file_path"] or "", item["entity_name"] or "", item["entity_type"] or ""
    item["graph_node_id"] = name
    return item


async def search_and_rank_hybrid_batch_device(store, reranker, host_ranker, query_vectors, plans, limit: int = 20,
                                              language: str | None = None, project_name: str | None = None, relation: str = "calls"):
    """:func:`search_and_rank_batch_device` with the graph branch on the device too: per query the same
    ``list[RankedResult]`` ``HybridRanker.rank_results`` gives for the ``GraphContext`` that :func:`plan_graph_roles` and the
    device call graph yield and the query's vector hits.  ``reranker`` is a ``ranking.device.HybridDeviceReranker``.  A query
    the device declines is ranked by ``host_ranker`` with a ``GraphContext`` built from the same device lists."""
    from .query_types import GraphContext, GraphNode
    from .ranking.device import ROLES, HybridDeviceReranker
    from .store import CollectionName
    from .vector_search import _CODE_KEYS, _project
    cap = get_settings().max_vector_results
    filters = {k: v for k, v in (("language", language), ("project_name", project_name)) if v}
    hits, parts, names = await store.search_rerank_hybrid_batch(CollectionName.CODE_CHUNKS.value, query_vectors, plans, reranker,
                                                                limit=min(limit, cap), filters=filters or None, relation=relation)
    ranked, q0 = [], 0
    for out, slots, scores, g_slots, g_nodes, declined in parts:
        for q in range(len(out.count)):
            class _Hits:      # candidate position -> the flattened hit dict, built on demand
                def __getitem__(self, i, q=q):
                    return _project(hits.hit(int(slots[q, i]), float(scores[q, i])), _CODE_KEYS)

            class _Items:
                def __getitem__(self, i, q=q):
                    return _graph_item(hits, names, int(g_nodes[q, i]))
            if out.count[q] >= 0:
                ranked.append(HybridDeviceReranker.materialise(out, q, _Items(), _Hits()))
                continue
            ctx = GraphContext()
            for role, node, depth in declined[q]:
                attr, _, has_depth = ROLES[role]
                it = _graph_item(hits, names, node)
                getattr(ctx, attr).append(GraphNode(node_type=it["entity_type"], name=it["entity_name"], qualified_name=it["graph_node_id"],
                                                    file_path=it["file_path"], signature=it["signature"], docstring=it["docstring"],
                                                    summary=it["summary"], start_line=it["start_line"], end_line=it["end_line"],
                                                    metadata={"depth": depth} if has_depth else {}))
            flat = [_project(hits.hit(int(t), float(s)), _CODE_KEYS) for t, s in zip(slots[q], scores[q]) if t >= 0]
            deg = hits._degrees or {}
            cand = centrality_candidates(ctx, flat)
            ranked.append(host_ranker.rank_results(plans[q0 + q], ctx, flat, {n: {"total_degree": deg[n]} for n in cand if n in deg}))
        q0 += len(out.count)
    return ranked
