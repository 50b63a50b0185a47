"""MCP ``semantic_search`` tool -- ``src/lattice/mcp/tools.py:368-462`` with its two wiring faults (quirk Q4) repaired:
the searcher comes from a factory that really constructs it, and code hits carry ``summary=None`` instead of raising."""

from __future__ import annotations

import logging
from dataclasses import dataclass
from typing import Any, Callable

logger = logging.getLogger(__name__)


@dataclass
class ToolResult:
    success: bool
    data: Any = None
    message: str | None = None
    error: str | None = None


@dataclass
class SearchResult:
    qualified_name: str
    entity_type: str
    file_path: str
    score: float
    summary: str | None = None


def create_semantic_search_tool(vector_searcher_factory: Callable[[], Any]) -> dict[str, Any]:
    async def semantic_search(query: str, limit: int = 5, entity_type: str | None = None, diversity: float | None = None,
                              candidates: int | None = None, max_per_file: int | None = None, extra_queries: list[str] | None = None,
                              fusion: str | None = None, like_ids: list[str] | None = None, unlike_ids: list[str] | None = None,
                              min_score: float | None = None, max_overlap: float | None = None, mode: str | None = None,
                              contains: str | list[str] | None = None, contains_case: bool | None = None,
                              matches: str | None = None, fuzzy: str | None = None, edits: int | None = None,
                              within_callers_of: str | list[str] | None = None, within_callees_of: str | list[str] | None = None,
                              graph_hops: int | None = None, rank: str | None = None, entities: list[str] | None = None,
                              intent: str | None = None, in_cycle: bool | None = None, between: list | None = None) -> ToolResult:
        logger.info(f"[Tool:SemanticSearch] Query: '{query}'")
        try:
            searcher = vector_searcher_factory()
            if rank not in (None, "vector", "hybrid", "propagated"):
                raise ValueError(f"rank {rank!r} is none of 'vector', 'hybrid', 'propagated'")
            if rank == "propagated":             # the matches re-ranked by a random walk over the call graph
                if like_ids or unlike_ids or entities or intent:
                    raise ValueError("rank='propagated' takes the arguments of a plain search, not like_ids, unlike_ids, entities or intent")
                extra = {k: v for k, v in (("diversity", diversity), ("max_per_file", max_per_file), ("extra_queries", extra_queries or None),
                                           ("min_score", min_score), ("max_overlap", max_overlap), ("candidates", candidates),
                                           ("contains", contains or None), ("matches", matches or None), ("fuzzy", fuzzy or None),
                                           ("edits", edits if fuzzy else None), ("within_callers_of", within_callers_of or None),
                                           ("within_callees_of", within_callees_of or None),
                                           ("graph_hops", graph_hops if within_callers_of or within_callees_of else None)) if v is not None}
                if contains_case is not None and (contains or matches or fuzzy):
                    extra["contains_case"] = contains_case
                got = await searcher.search_code_propagated(query=query, limit=limit, entity_type=entity_type, mode=mode or "semantic", **extra)
                data = [vars(SearchResult(qualified_name=h.get("graph_node_id") or h.get("entity_name"), entity_type=h.get("entity_type"),
                                          file_path=h.get("file_path"), score=h.get("score"), summary=None)) for h in got["results"]]
                related = ", ".join(r["qualified_name"] for r in got["related"])
                return ToolResult(success=True, data=data, message=f"Found {len(data)} matches for '{query}', ordered by similarity and call-graph "
                                  "relevance." + (f" Related code the query text did not find: {related}." if related else ""))
            if rank == "hybrid":                 # graph results and vector hits in one list, ranked on the device
                import numpy as np
                from .engine_helpers import search_and_rank_hybrid_batch_device
                from .query_types import ExtractedEntity, QueryIntent, QueryPlan
                from .ranking import HybridRanker
                from .ranking.device import HybridDeviceReranker
                if entity_type or like_ids or unlike_ids or mode not in (None, "semantic"):
                    raise ValueError("rank='hybrid' takes query, limit, entities and intent only")
                plan = QueryPlan(original_query=query, primary_intent=QueryIntent(intent or QueryIntent.SEARCH_FUNCTIONALITY.value),
                                 entities=[ExtractedEntity(name=e, is_primary=True) for e in (entities or [])])
                vector = np.asarray(await searcher.embedder.embed(query), dtype=np.float32)[None, :]
                ranked = (await search_and_rank_hybrid_batch_device(searcher.qdrant, HybridDeviceReranker(), HybridRanker(), vector, [plan],
                                                                    limit=max(limit, 20)))[0][:limit]
                data = [vars(SearchResult(qualified_name=r.graph_node_id or r.entity_name, entity_type=r.entity_type, file_path=r.file_path,
                                          score=r.final_score, summary=r.summary)) for r in ranked]
                return ToolResult(success=True, data=data, message=f"Found {len(data)} graph and vector matches for '{query}'.")
            if like_ids or unlike_ids:           # recommend by example: the query text is not embedded
                if not like_ids:
                    raise ValueError("unlike_ids needs like_ids")
                hits = await searcher.find_similar_to(positive_ids=list(like_ids), negative_ids=list(unlike_ids or []), limit=limit)
                data = [vars(SearchResult(qualified_name=h.get("entity_name"), entity_type=h.get("entity_type"), file_path=h.get("file_path"),
                                          score=h.get("score"), summary=h.get("summary"))) for h in hits]
                return ToolResult(success=True, data=data, message=f"Found {len(data)} matches like {len(like_ids)} example(s).")
            extra = {k: v for k, v in (("diversity", diversity), ("candidates", candidates), ("max_per_file", max_per_file),
                                       ("extra_queries", extra_queries or None), ("fusion", fusion), ("min_score", min_score), ("max_overlap", max_overlap), ("mode", mode),
                                       ("contains", contains or None), ("contains_case", contains_case if contains or matches or fuzzy else None),
                                       ("matches", matches or None), ("fuzzy", fuzzy or None), ("edits", edits if fuzzy else None),
                                       ("within_callers_of", within_callers_of or None), ("within_callees_of", within_callees_of or None),
                                       ("graph_hops", graph_hops if within_callers_of or within_callees_of or between else None),
                                       ("in_cycle", True if in_cycle else None), ("between", tuple(between) if between else None)) if v is not None}   # (only when asked for)
            hits = await searcher.search_code(query=query, limit=limit, entity_type=entity_type, **extra)
            rows = []
            for h in hits:
                get = h.get if isinstance(h, dict) else (lambda k, _h=h: getattr(_h, k, None))
                rows.append(SearchResult(qualified_name=get("entity_name"), entity_type=get("entity_type"),
                                         file_path=get("file_path"), score=get("score"), summary=get("summary")))
            message = f"Found {len(rows)} matches for '{query}'."
            if min_score is not None and len(rows) < limit:   # (a thresholded list shorter than `limit` holds EVERY row in range)
                message = f"Found {len(rows)} matches for '{query}': only {len(rows)} rows score at least {min_score}."
            return ToolResult(success=True, data=[vars(r) for r in rows], message=message)
        except Exception as e:  # the reference's catch-all (tools.py:431-436)
            logger.error(f"[Tool:SemanticSearch] Error: {e}", exc_info=True)
            return ToolResult(success=False, error=str(e))

    return {
        "name": "semantic_search",
        "description": ("Search for code by functionality or intent using natural language. "
                        "Find code based on what it does, not its name."),
        "function": semantic_search,
        "parameters": {
            "query": {"type": "string", "description": "Natural language description of functionality", "required": True},
            "limit": {"type": "integer", "description": "Maximum number of results (default: 5)", "required": False},
            "entity_type": {"type": "string", "description": "Filter by type: function, class, method", "required": False},
            "diversity": {"type": "number", "description": "0..1: prefer results that differ from each other (maximal marginal relevance); "
                                                           "omit for the plain top matches", "required": False},
            "candidates": {"type": "integer", "description": "With diversity: how many top matches to choose among (default: 4 x limit)",
                           "required": False},
            "max_per_file": {"type": "integer", "description": "At most this many results from one file (the list still holds `limit` results)",
                             "required": False},
            "extra_queries": {"type": "array", "description": "Other wordings of the same question (up to 15); the results of all "
                                                              "wordings are fused into one list", "required": False},
            "fusion": {"type": "string", "description": "With extra_queries: 'rrf' (reciprocal-rank fusion, the default) or 'max' "
                                                        "(best match over the wordings)", "required": False},
            "min_score": {"type": "number", "description": "Only results whose similarity score is at least this; fewer than `limit` "
                                                           "(or none) come back when nothing else is that relevant", "required": False},
            "max_overlap": {"type": "number", "description": "0..1: drop a result that repeats more than this share of a better result's "
                                                             "lines (a method under its class, the next part of a long function); the "
                                                             "list still holds `limit` results", "required": False},
            "mode": {"type": "string", "description": "'semantic' (the default: by meaning), 'lexical' (exact keyword search: finds the "
                                                      "chunks that literally hold an identifier such as parse_retry_after) or 'hybrid' "
                                                      "(both, fused by rank)", "required": False},
            "like_ids": {"type": "array", "description": "Ids of results to find more of (up to 8): the answer is built from these "
                                                         "stored examples instead of the query text", "required": False},
            "unlike_ids": {"type": "array", "description": "With like_ids: ids of results to steer away from (up to 8)", "required": False},
            "contains": {"type": "string", "description": "A literal string (or a list of up to 8) every result's code must contain, "
                                                          "punctuation included: 'retry_after=', '.unwrap()', '#include <hip/'",
                         "required": False},
            "contains_case": {"type": "boolean", "description": "With contains / matches / fuzzy: false ignores the case of ASCII letters (default: true)",
                              "required": False},
            "matches": {"type": "string", "description": "A regular expression (Python re syntax, ^ and $ at every line; no "
                                                         "back-references or look-around) that must be found in every result's code: "
                                                         "'def \\w+_retry\\(', '^\\s*#include\\s*<hip/', '[A-Z][a-z]+Error\\b'",
                        "required": False},
            "fuzzy": {"type": "string", "description": "An identifier or string (up to 64 bytes) every result's code must contain up "
                                                       "to a few typos: 'parse_retry_aftr' finds parse_retry_after, 'HTTPServerEror' "
                                                       "finds HTTPServerError; use it when the exact spelling is not known",
                      "required": False},
            "edits": {"type": "integer", "description": "With fuzzy: how many single-character insertions, deletions or substitutions "
                                                        "are allowed, 0..3 (default: 1 for up to 5 characters, 2 above; a swapped pair "
                                                        "of characters counts as 2)", "required": False},
            "within_callers_of": {"type": "string", "description": "A function or method name (or a list): only code that calls it, "
                                                                   "directly or through other calls, is searched -- the named code itself "
                                                                   "included", "required": False},
            "within_callees_of": {"type": "string", "description": "A function or method name (or a list): only code reachable from it by "
                                                                   "calls is searched ('timeout handling, but only under main')",
                                  "required": False},
            "graph_hops": {"type": "integer", "description": "With within_callers_of / within_callees_of: how many calls away code may "
                                                             "be, 1..16 (default: 3); with between: how long a way may be (default: 8)",
                           "required": False},
            "between": {"type": "array", "description": "Two function names [a, b] (either may be a list of names): only code that lies on "
                                                        "a way of calls from a to b is searched ('retry handling, but only between "
                                                        "handle_request and db.execute')", "required": False},
            "in_cycle": {"type": "boolean", "description": "true: only code that lies in a call cycle is searched -- recursive functions "
                                                           "and groups of functions that call each other", "required": False},
            "rank": {"type": "string", "description": "'vector' (the default: the plain matches), 'hybrid': the named entities' graph "
                                                      "neighbourhood (callers, callees, class hierarchy) and the matches ranked as one "
                                                      "list, or 'propagated': the matches re-ordered by how central they are in the code "
                                                      "the matches call and are called from, with the related functions the text did "
                                                      "not find named in the message", "required": False},
            "entities": {"type": "array", "description": "With rank='hybrid': names of the functions or classes the question is about",
                         "required": False},
            "intent": {"type": "string", "description": "With rank='hybrid': find_callers, find_callees, find_hierarchy, "
                                                        "explain_implementation, ... (default: search_functionality)", "required": False},
        },
    }


def create_code_graph_tool(vector_searcher_factory: Callable[[], Any]) -> dict[str, Any]:
    """MCP ``code_graph`` tool (the reference answers these from Memgraph, query/graph_reasoning/engine.py): what calls a
    function, what it calls, and how one function reaches another -- answered on the device from the call edges beside the
    vectors (``VectorSearcher.find_callers`` / ``find_callees`` / ``find_call_chain``)."""
    async def code_graph(name: str = "", relation: str = "callers", target: str | None = None, max_hops: int | None = None,
                         limit: int = 50, op: str | None = None) -> ToolResult:
        logger.info(f"[Tool:CodeGraph] {op or relation} of '{name}'" + (f" -> '{target}'" if target else ""))
        try:
            searcher = vector_searcher_factory()
            if op in ("cycles", "layers"):       # questions about the graph as a whole
                if target or max_hops is not None:
                    raise ValueError(f"op {op!r} takes name and limit only")
                if op == "cycles":
                    if name:
                        raise ValueError("op 'cycles' lists the cycles of the whole graph: it takes no name (search with in_cycle for code inside them)")
                    got = await searcher.find_cycles(limit=limit)
                    return ToolResult(success=True, data=got["cycles"], message=f"Found {got['count']} call cycle(s) over {got['nodes']} function(s); the "
                                      f"{len(got['cycles'])} largest are listed.")
                got = await searcher.find_layers(names=name or None, match="suffix")
                return ToolResult(success=True, data=got["nodes"], message=f"The call graph has {got['layers']} layer(s); by depth below the entry points "
                                  f"they hold {got['histogram']['depth']} functions, by height above the leaves {got['histogram']['height']}.")
            if op == "chains":                   # every shortest chain, and what none of them avoids
                if not name or not target:
                    raise ValueError("op 'chains' needs a name and a target")
                got = await searcher.find_call_chains(name, target, **({} if max_hops is None else {"max_hops": max_hops}), limit=min(limit, 64))
                if not got["count"]:
                    message = f"No chain of calls from '{name}' to '{target}' within {8 if max_hops is None else max_hops} calls."
                else:
                    message = (f"'{name}' reaches '{target}' by {'at least ' if got['saturated'] else ''}{got['count']} shortest chain(s) of {got['length']} call(s); "
                               f"{len(got['chains'])} listed. " + (f"Every way passes {', '.join(got['must_pass'])}." if got["must_pass"] else "No function lies on every way."))
                return ToolResult(success=True, data=got["chains"], message=message)
            if op is not None:
                if op != "important_near":
                    raise ValueError(f"op {op!r} is not one of 'important_near', 'cycles', 'layers', 'chains'")
                if target or max_hops is not None:
                    raise ValueError("op 'important_near' takes name and limit only")
                nodes = await searcher.find_important_near(name, limit=limit)
                return ToolResult(success=True, data=nodes, message=f"Found {len(nodes)} nodes that matter around '{name}'.")
            if relation == "chain":
                if not target:
                    raise ValueError("relation 'chain' needs a target")
                paths = await searcher.find_call_chain(name, target, **({} if max_hops is None else {"max_hops": max_hops}))
                message = (f"'{name}' reaches '{target}' in {paths[0]['total_length']} call(s)." if paths else
                           f"No chain of calls from '{name}' to '{target}' within {8 if max_hops is None else max_hops} calls.")
                return ToolResult(success=True, data=paths, message=message)
            if relation not in ("callers", "callees"):
                raise ValueError(f"relation {relation!r} is not one of 'callers', 'callees', 'chain'")
            walk = searcher.find_callers if relation == "callers" else searcher.find_callees
            nodes = await walk(name, **({} if max_hops is None else {"max_hops": max_hops}), limit=limit)
            return ToolResult(success=True, data=nodes, message=f"Found {len(nodes)} transitive {relation} of '{name}'.")
        except Exception as e:  # the catch-all of the reference's tools (tools.py:431-436)
            logger.error(f"[Tool:CodeGraph] Error: {e}", exc_info=True)
            return ToolResult(success=False, error=str(e))

    return {
        "name": "code_graph",
        "description": ("Walk the call graph: what calls a function (transitively), what it calls, or how one function reaches "
                        "another. Use it for impact analysis and for 'how does X get to Y'."),
        "function": code_graph,
        "parameters": {
            "name": {"type": "string", "description": "The qualified name of the function, method or class to start from (none for op "
                                                      "'cycles'; optional for op 'layers')", "required": True},
            "relation": {"type": "string", "description": "'callers' (the default: what calls it), 'callees' (what it calls) or 'chain' "
                                                          "(one shortest chain of calls from name to target)", "required": False},
            "target": {"type": "string", "description": "With relation 'chain' or op 'chains': the qualified name to reach", "required": False},
            "max_hops": {"type": "integer", "description": "How many calls away to look, 1..16 (default: 3; 8 for a chain)", "required": False},
            "limit": {"type": "integer", "description": "Maximum number of callers / callees listed, nearest first (default: 50)", "required": False},
            "op": {"type": "string", "description": "'important_near': instead of a walk, rank the code around name by a random walk with "
                                                    "restart over the calls, both ways (personalised PageRank): what matters near it, "
                                                    "best first.  'cycles': the groups of functions that call each other in a circle "
                                                    "(recursion, mutual recursion), largest first; takes limit only.  'layers': how deep "
                                                    "below the entry points and how high above the leaf helpers name lies (without a name: "
                                                    "how many functions each layer holds).  'chains': with target, HOW MANY shortest chains "
                                                    "of calls lead from name to target, the first `limit` of them, and the functions every "
                                                    "way of at most max_hops calls passes", "required": False},
        },
    }


def create_code_facets_tool(vector_searcher_factory: Callable[[], Any]) -> dict[str, Any]:
    """MCP ``code_facets`` tool (not in the reference): WHERE something lives -- the most frequent files, languages or entity
    types among the chunks that pass a filter, hold a string or are similar to a description, with exact counts
    (``VectorSearcher.facet_code``)."""
    async def code_facets(key: str = "file_path", query: str | None = None, min_score: float | None = None, limit: int = 10,
                          language: str | None = None, entity_type: str | None = None, contains: str | list[str] | None = None,
                          contains_case: bool | None = None, matches: str | None = None, fuzzy: str | None = None,
                          edits: int | None = None) -> ToolResult:
        logger.info(f"[Tool:CodeFacets] Key: '{key}' query: {query!r}")
        try:
            searcher = vector_searcher_factory()
            extra = {k: v for k, v in (("query", query or None), ("min_score", min_score), ("language", language), ("entity_type", entity_type),
                                       ("contains", contains or None), ("contains_case", contains_case if contains or matches or fuzzy else None),
                                       ("matches", matches or None), ("fuzzy", fuzzy or None), ("edits", edits if fuzzy else None)) if v is not None}   # (only when asked for)
            res = await searcher.facet_code(key=key, limit=limit, **extra)
            shown, values = len(res["hits"]), res["values"]
            message = f"{res['total']} chunks carry {values} distinct {key} value(s)" + (f"; the {shown} most frequent are listed." if shown < values else ".")
            return ToolResult(success=True, data=res, message=message)
        except Exception as e:  # the catch-all of the reference's tools (tools.py:431-436)
            logger.error(f"[Tool:CodeFacets] Error: {e}", exc_info=True)
            return ToolResult(success=False, error=str(e))

    return {
        "name": "code_facets",
        "description": ("Count code chunks per file, language or entity type: where a string, a pattern or a concept lives in the "
                        "code base, with exact counts -- not which chunks."),
        "function": code_facets,
        "parameters": {
            "key": {"type": "string", "description": "What to count by: 'file_path' (the default), 'language', 'entity_type', "
                                                     "'entity_name' or 'project_name'", "required": False},
            "query": {"type": "string", "description": "With min_score: count only chunks at least that similar to this natural "
                                                       "language description", "required": False},
            "min_score": {"type": "number", "description": "With query: the similarity score a chunk must reach to be counted", "required": False},
            "limit": {"type": "integer", "description": "How many values to list, most frequent first (default: 10, at most 1024)", "required": False},
            "language": {"type": "string", "description": "Count only chunks in this language", "required": False},
            "entity_type": {"type": "string", "description": "Count only chunks of this type: function, class, method", "required": False},
            "contains": {"type": "string", "description": "Count only chunks whose code contains this literal string (or every string "
                                                          "of a list of up to 8): 'TODO(', '.unwrap()'", "required": False},
            "contains_case": {"type": "boolean", "description": "With contains / matches / fuzzy: false ignores the case of ASCII letters (default: true)",
                              "required": False},
            "matches": {"type": "string", "description": "Count only chunks in whose code this regular expression (Python re syntax) is found",
                        "required": False},
            "fuzzy": {"type": "string", "description": "Count only chunks whose code contains this string up to a few typos "
                                                       "('parse_retry_aftr' finds parse_retry_after)", "required": False},
            "edits": {"type": "integer", "description": "With fuzzy: the insertions, deletions or substitutions allowed, 0..3 "
                                                        "(default: 1 for up to 5 characters, 2 above)", "required": False},
        },
    }
