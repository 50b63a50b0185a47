"""Dict-returning semantic searcher -- the query-side surface of ``src/lattice/query/vector_search.py:43-280``.

Single-query methods keep the reference's signatures, result keys, validation and error mapping
(``EmbeddingError`` / ``VectorStoreError`` -> ``QueryError``; blank input -> ``QueryError``).  Added here: batch
entry points (``search_code_batch``) that put up to 64 queries through ONE corpus scan, which is what the
MI355X kernels are built for; the reference issues one RPC per query.
"""

from __future__ import annotations

import logging
from dataclasses import dataclass
from typing import Any

import numpy as np

from .errors import EmbeddingError, QueryError, VectorStoreError
from .store import CollectionName

logger = logging.getLogger(__name__)

DEFAULT_SEARCH_LIMIT = 10
EXCLUDE_FILE_BUFFER = 5

_CODE_KEYS = ("file_path", "entity_type", "entity_name", "language", "content", "start_line", "end_line", "graph_node_id")
_SUMMARY_KEYS = ("file_path", "entity_type", "entity_name", "summary", "graph_node_id")
_SIMILAR_KEYS = ("file_path", "entity_type", "entity_name", "content", "start_line", "end_line")


@dataclass
class CodeSearchResult:
    score: float
    file_path: str
    entity_type: str
    entity_name: str
    content: str
    language: str | None = None
    start_line: int | None = None
    end_line: int | None = None
    graph_node_id: str | None = None


@dataclass
class SummarySearchResult:
    score: float
    file_path: str
    entity_type: str
    entity_name: str
    summary: str
    graph_node_id: str | None = None


_NO_FILTER_KWARG = object()


def _mmr_kwargs(diversity: float | None, candidates: int | None) -> dict:
    """``diversity`` / ``candidates`` as store keywords -- only the ones given, so a call that asks for no diversity has the
    shape the reference's has."""
    kw = {}
    if diversity is not None:
        kw["diversity"] = diversity
    if candidates is not None:
        kw["candidates"] = candidates
    return kw


def _group_kwargs(max_per_file: int | None) -> dict:
    """``max_per_file`` as the store's grouped search (at most that many chunks of one file, decided before the cut: the
    list stays ``limit`` long) -- only when given."""
    return {} if max_per_file is None else {"group_by": "file_path", "group_size": max_per_file}


def _threshold_kwargs(min_score: float | None) -> dict:
    """``min_score`` as the store's ``score_threshold`` -- only when given: without it the call is the one issued before."""
    return {} if min_score is None else {"score_threshold": min_score}


def _overlap_kwargs(max_overlap: float | None) -> dict:
    """``max_overlap`` as the store's keyword of that name (no hit repeats more than that share of a better hit's lines) -- only
    when given: without it the call is the one issued before."""
    return {} if max_overlap is None else {"max_overlap": max_overlap}


def _project(hit: dict, keys: tuple[str, ...]) -> dict:
    payload = hit["payload"]
    row = {"score": hit["score"]}
    for k in keys:
        row[k] = payload.get(k)
    return row


def _fused_keys(hit: dict) -> tuple[str, ...]:
    """The extra result keys of a fused hit (``HipVectorStore.search_fused``: two; ``search_hybrid``: three); none for a plain one."""
    if "lexical_score" in hit:
        return ("cosine", "lexical_score", "matched")
    return ("cosine", "matched") if "matched" in hit else ()


def _mode_kwargs(mode: str) -> dict:
    """``mode`` as a keyword of :meth:`VectorSearcher._lookup` -- only when it is not the default: a semantic call is the
    one issued before."""
    return {} if mode == "semantic" else {"mode": mode}


def _contains_filter(key: str, contains, contains_case: bool, matches: str | None = None, fuzzy: str | None = None,
                     edits: int | None = None) -> dict:
    """``contains`` (a str or a list of str: the literal strings a hit's text must ALL hold) and ``matches`` (a regular
    expression ``re.search`` must find in it) as the store's text condition on ``key`` -- ``{}`` without either: the call is
    then the one issued before, keyword for keyword."""
    if contains is None and matches is None and fuzzy is None and edits is None:
        return {}
    spec = {} if contains is None else {"contains": contains}
    if matches is not None:
        spec["matches"] = matches
    if fuzzy is not None:
        spec["fuzzy"] = fuzzy
    if edits is not None:
        spec["edits"] = edits                                          # (alone: the store refuses it by name)
    if not contains_case:
        spec["case"] = False
    return {key: spec}


def _graph_filter(within_callers_of, within_callees_of, graph_hops: int | None, in_cycle: bool | None = None, graph_depth=None,
                  graph_height=None, between=None) -> dict:
    """``within_callers_of`` / ``within_callees_of`` (a node name or a list of them) as the store's ``"graph"`` condition: only
    code that calls / is called from those nodes, transitively within ``graph_hops`` edges (the store's default: 3), the named
    nodes' own chunks included -- ``{}`` without either: the call is then the one issued before.  ``between``
    = ``(a, b)``, each a name or a list of them: only code on a way of at most ``graph_hops`` (default 8) calls from ``a`` to
    ``b``."""
    whole = {k: v for k, v in (("in_cycle", True if in_cycle else None), ("depth", graph_depth), ("height", graph_height)) if v is not None}
    if between is not None:
        if whole or within_callers_of is not None or within_callees_of is not None:
            raise QueryError("between, in_cycle, graph_depth, graph_height, within_callers_of and within_callees_of cannot be combined (one graph condition per search)")
        if isinstance(between, str) or not isinstance(between, (list, tuple)) or len(between) != 2:
            raise QueryError("between takes a pair (a, b): a node name or a list of names for either end")
        spec = {"between": [list(e) if isinstance(e, (list, tuple, set, frozenset)) else e for e in between]}
        if graph_hops is not None:
            spec["hops"] = graph_hops
        return {"graph": spec}
    if whole:                                                            # the node's place in the whole graph
        if len(whole) > 1 or within_callers_of is not None or within_callees_of is not None or graph_hops is not None:
            raise QueryError("in_cycle, graph_depth, graph_height, within_callers_of and within_callees_of cannot be combined (one graph condition per search)")
        return {"graph": whole}
    if within_callers_of is None and within_callees_of is None:
        if graph_hops is not None:
            raise QueryError("graph_hops stands beside within_callers_of or within_callees_of")
        return {}
    if within_callers_of is not None and within_callees_of is not None:
        raise QueryError("within_callers_of and within_callees_of cannot be combined (one graph condition per search)")
    spec = {"callers_of": within_callers_of} if within_callers_of is not None else {"callees_of": within_callees_of}
    if graph_hops is not None:
        spec["hops"] = graph_hops
    return {"graph": spec}


def _node_row(ranked: dict) -> dict:
    """A ranked graph node of the store (``{"node", "graph_score", "payload"}``) as a result row; a node without a chunk has
    its names and score only."""
    pay = ranked.get("payload") or {}
    return {"name": ranked["node"].rsplit(".", 1)[-1], "qualified_name": ranked["node"], "graph_score": ranked["graph_score"],
            "file_path": pay.get("file_path"), "entity_type": pay.get("entity_type"), "start_line": pay.get("start_line")}


def _transform_similar_code_result(hit: dict) -> dict:
    """A store hit in the result shape of ``find_similar_code`` (vector_search.py:199-216); a recommend hit under strategy
    "best" keeps its two extra keys."""
    row = _project(hit, _SIMILAR_KEYS)
    for k in ("negative_score", "matched_positive"):
        if k in hit:
            row[k] = hit[k]
    return row


class VectorSearcher:
    def __init__(self, qdrant, embedder):
        self.qdrant = qdrant
        self.embedder = embedder

    async def _lookup(self, text: str, collection: str, limit: int, filters: Any, embed_fail: str, store_fail: str,
                      must_not: dict | None = None, diversity: float | None = None, candidates: int | None = None,
                      max_per_file: int | None = None, extra_queries: list[str] | None = None, fusion: str = "rrf",
                      min_score: float | None = None, max_overlap: float | None = None, mode: str = "semantic"):
        """Embed, search, map the two error kinds.  ``mode``: "semantic" (the calls below, unchanged), "lexical" (nothing is
        embedded: ``HipVectorStore.search_lexical`` of the text) or "hybrid" (``HipVectorStore.search_hybrid`` of the text's
        vector and the text); the two keyword modes take ``filters`` / ``must_not`` / ``candidates`` only.  ``filters=_NO_FILTER_KWARG`` omits the keyword altogether, as
        the reference's ``find_similar_code`` does (vector_search.py:193-197); ``must_not`` is passed only when given, and
        so are ``diversity`` / ``candidates`` (the store's diversity-aware top-k).  ``extra_queries`` (reformulations of
        ``text``): all texts are embedded in ONE provider batch and the store fuses their hit lists
        (``HipVectorStore.search_fused``); without them the call is the plain one, keyword for keyword.  ``min_score``: the
        store's ``score_threshold`` -- only hits at least that similar come back; not together with ``extra_queries`` (a fused
        score is no cosine), ``diversity`` or ``max_per_file`` (the store refuses those).  ``max_overlap``: the store's overlap-free
        top-k; not together with ``extra_queries``, and the store refuses it beside ``diversity``, ``max_per_file`` or ``min_score``."""
        extra = [t for t in (extra_queries or []) if t and t.strip()]
        if mode != "semantic":
            return await self._lookup_keyword(text, collection, limit, filters, embed_fail, store_fail, must_not, candidates, mode,
                                              diversity=diversity, max_per_file=max_per_file, extra_queries=extra or None,
                                              min_score=min_score, max_overlap=max_overlap)
        if extra and min_score is not None:
            raise ValueError("min_score cannot be combined with extra_queries")
        if extra and (diversity is not None or max_per_file is not None or max_overlap is not None):
            raise ValueError("extra_queries cannot be combined with diversity, max_per_file or max_overlap")
        try:
            kwargs = {} if filters is _NO_FILTER_KWARG else {"filters": filters}
            if must_not:
                kwargs["must_not"] = must_not
            if extra:
                vectors = np.asarray(await self.embedder.embed_batch([text] + extra), dtype=np.float32)
                if candidates is not None:
                    kwargs["candidates"] = candidates
                hits = await self.qdrant.search_fused(collection=collection, query_vectors=vectors, limit=limit, fusion=fusion, **kwargs)
                for h in hits:                      # (what _project copies: the fused score stays "score")
                    h["payload"] = dict(h["payload"], cosine=h["cosine"], matched=h["matched"])
                return hits
            vector = await self.embedder.embed(text)
            kwargs.update(_mmr_kwargs(diversity, candidates))
            kwargs.update(_group_kwargs(max_per_file))
            kwargs.update(_threshold_kwargs(min_score))
            kwargs.update(_overlap_kwargs(max_overlap))
            return await self.qdrant.search(collection=collection, query_vector=vector, limit=limit, **kwargs)
        except EmbeddingError as e:
            logger.error(f"Embedding error: {e}")
            raise QueryError(embed_fail, cause=e)
        except VectorStoreError as e:
            logger.error(f"Vector store error: {e}")
            raise QueryError(store_fail, cause=e)

    async def _lookup_keyword(self, text: str, collection: str, limit: int, filters: Any, embed_fail: str, store_fail: str, must_not,
                              candidates, mode: str, **others):
        """``mode`` "lexical" / "hybrid" of :meth:`_lookup`: the store's keyword and fused searches.  A hybrid hit's
        ``cosine`` / ``lexical_score`` / ``matched`` travel in its payload copy, like a fused hit's."""
        if mode not in ("lexical", "hybrid"):
            raise ValueError(f"unknown search mode {mode!r} (one of 'semantic', 'lexical', 'hybrid')")
        used = [k for k, v in others.items() if v is not None]
        if used:
            raise ValueError(f"mode={mode!r} cannot be combined with {', '.join(used)}")
        try:
            kwargs = {} if filters is _NO_FILTER_KWARG else {"filters": filters}
            if must_not:
                kwargs["must_not"] = must_not
            if mode == "lexical":
                return await self.qdrant.search_lexical(collection=collection, text=text, limit=limit, **kwargs)
            vector = await self.embedder.embed(text)
            if candidates is not None:
                kwargs["candidates"] = candidates
            hits = await self.qdrant.search_hybrid(collection=collection, query_vector=vector, text=text, limit=limit, **kwargs)
            for h in hits:
                h["payload"] = dict(h["payload"], cosine=h["cosine"], lexical_score=h["lexical_score"], matched=h["matched"])
            return hits
        except EmbeddingError as e:
            logger.error(f"Embedding error: {e}")
            raise QueryError(embed_fail, cause=e)
        except VectorStoreError as e:
            logger.error(f"Vector store error: {e}")
            raise QueryError(store_fail, cause=e)

    async def search_code(self, query: str, limit: int = DEFAULT_SEARCH_LIMIT, language: str | list[str] | None = None,
                          entity_type: str | None = None, project_name: str | list[str] | None = None, *,
                          diversity: float | None = None, candidates: int | None = None, max_per_file: int | None = None,
                          extra_queries: list[str] | None = None, fusion: str = "rrf", min_score: float | None = None,
                          max_overlap: float | None = None, mode: str = "semantic", contains: str | list[str] | None = None,
                          contains_case: bool = True, matches: str | None = None,
                          fuzzy: str | None = None, edits: int | None = None, within_callers_of: str | list[str] | None = None,
                          within_callees_of: str | list[str] | None = None, graph_hops: int | None = None,
                          propagate: bool | dict | None = None, in_cycle: bool | None = None, graph_depth: int | dict | None = None,
                          graph_height: int | dict | None = None, between: tuple | list | None = None) -> list[dict]:
        """vector_search.py:60-116.  ``mode`` (not in the reference): "semantic" -- the default, everything below --,
        "lexical" -- exact keyword search (BM25) of ``query``, nothing embedded: where is ``parse_retry_after`` -- or "hybrid"
        -- both, fused by reciprocal rank (``HipVectorStore.search_hybrid``): every result then also carries ``cosine``,
        ``lexical_score`` and ``matched``.  The keyword modes take the filters and ``candidates`` only.  ``language`` / ``project_name`` may be a list: any of them (one device condition).
        ``diversity`` in [0, 1] (not in the reference): ``limit`` maximal-marginal-relevance picks among the ``candidates``
        best hits instead of the plain top-``limit`` (``HipVectorStore.search``).  ``max_per_file`` (the reference applies it
        after the fetch, query/reranker.py:122-145, and comes back short): at most that many chunks of one file among the
        ``limit`` results, exactly (``group_by="file_path"``); not together with ``diversity``.
        ``extra_queries`` (not in the reference, whose engine searches the original text only, query/engine.py:315-346):
        reformulations of ``query`` -- the planner's sub-queries, a HyDE answer -- embedded with it in one batch; the store
        fuses the hit lists of all of them (``fusion`` = "rrf" or "max", ``HipVectorStore.search_fused``), ``score`` is the fused
        score and every result also carries ``cosine`` and ``matched``.  Not together with ``diversity`` / ``max_per_file``.
        ``min_score`` (Qdrant's ``score_threshold``; the reference never sends it): only results whose score is at least that --
        possibly fewer than ``limit``, possibly none ("nothing here is relevant"); a list shorter than ``limit`` is ALL of them.
        Not together with ``diversity`` / ``max_per_file`` / ``extra_queries``.
        ``max_overlap`` in [0, 1] (not in the reference, which returns a class, its method and the method's ``_part2`` for one
        good query): no result repeats more than that share of a better result's lines (``HipVectorStore.search``, DESIGN.md
        3.19); the list still holds ``limit`` results.  Not together with ``diversity`` / ``max_per_file`` / ``min_score`` /
        ``extra_queries``.
        ``contains`` (not in the reference; Qdrant's ``MatchText``): a literal string, or a list of them, every result's
        ``content`` must hold -- ``retry_after=``, ``.unwrap()`` -- matched exactly on the device (``HipVectorStore.search``,
        DESIGN.md 3.21), in every mode and beside every other argument; ``contains_case=False`` ignores the case of ASCII
        letters.  ``matches`` likewise: a regular expression in the syntax of Python's ``re`` on bytes, with ``re.MULTILINE``,
        that ``re.search`` must find in every result's ``content`` -- ``def \\w+_retry\\(`` -- (DESIGN.md 3.22); beside
        ``contains`` both must hold, and ``contains_case`` governs both.  ``fuzzy`` likewise: a string every result's ``content``
        must hold within ``edits`` BYTE insertions, deletions or substitutions (0..3; default 1 for up to 5 bytes, 2 above) --
        ``parse_retry_aftr`` finds ``parse_retry_after`` -- matched exactly on the device; beside the other two
        all must hold, and ``contains_case`` governs it too.  :meth:`search_summaries`, :meth:`find_similar_code`,
        :meth:`facet_code` and :meth:`search_code_batch` take ``fuzzy`` / ``edits`` the same way.
        ``within_callers_of`` / ``within_callees_of`` (not in the reference, which would need Memgraph and a second query): a
        node name or a list of them -- only code that calls / is called from them, transitively within ``graph_hops`` edges
        (default 3), counts: "timeout handling, but only in code reachable from ``main``".  Resolved by a BFS on the device
        over the edges given to ``HipVectorStore.set_graph_edges``, in every mode and beside every other
        argument; :meth:`search_summaries`, :meth:`find_similar_code` and :meth:`search_code_batch` take them the same way.
        ``in_cycle=True`` / ``graph_depth`` / ``graph_height`` (not in the reference) instead: only code whose node lies in a
        call cycle -- a recursive function, or several that call each other -- / at that depth below the entry points / at
        that height above the leaf helpers (an int, or a range such as ``{"lte": 1}``): "retry handling, but only in leaf
        helpers" is ``graph_height=0``.  Components and layers of the whole graph are found on the device once per graph
        (DESIGN.md 3.31); :meth:`find_similar_code` and :meth:`search_code_batch` take them the same way.
        ``between=(a, b)`` (not in the reference) instead, each end a node name or a list of them: only code that lies on a way
        of at most ``graph_hops`` (default 8) calls from ``a`` to ``b`` -- "retry handling, but only between ``handle_request``
        and ``db.execute``" (DESIGN.md 3.32); :meth:`search_summaries`, :meth:`find_similar_code`, :meth:`search_code_batch`
        and :meth:`facet_code` take it the same way.
        ``propagate`` (not in the reference): ``True``, or the settings of ``HipVectorStore.search_propagated`` -- the best
        ``candidates`` matches seed a random walk with restart over the call graph (personalised PageRank) and
        the results are ordered by reciprocal-rank fusion of similarity and graph score: of the matches, those in the middle of
        the code the others call come first.  Every result then also carries ``cosine`` and ``graph_score``;
        :meth:`search_code_propagated` returns the related nodes as well.  Semantic mode only, beside the filters and
        ``candidates``."""
        if propagate is not None and propagate is not False:
            return (await self.search_code_propagated(
                query, limit, language, entity_type, project_name, candidates=candidates, propagate=propagate, related_limit=0,
                contains=contains, contains_case=contains_case, matches=matches, fuzzy=fuzzy, edits=edits, within_callers_of=within_callers_of,
                within_callees_of=within_callees_of, graph_hops=graph_hops, diversity=diversity, max_per_file=max_per_file,
                extra_queries=extra_queries, min_score=min_score, max_overlap=max_overlap, mode=mode, in_cycle=in_cycle or None,
                graph_depth=graph_depth, graph_height=graph_height, between=between))["results"]
        if not query or not query.strip():
            raise QueryError("Search query cannot be empty")
        filters = {k: v for k, v in (("language", language), ("entity_type", entity_type), ("project_name", project_name)) if v}
        filters.update(_contains_filter("content", contains, contains_case, matches, fuzzy, edits))
        filters.update(_graph_filter(within_callers_of, within_callees_of, graph_hops, in_cycle, graph_depth, graph_height, between))
        hits = await self._lookup(query, CollectionName.CODE_CHUNKS.value, limit, filters or None,
                                  "Failed to embed search query", "Failed to search code", diversity=diversity, candidates=candidates,
                                  max_per_file=max_per_file, extra_queries=extra_queries, fusion=fusion, min_score=min_score,
                                  max_overlap=max_overlap, **_mode_kwargs(mode))
        return [_project(h, _CODE_KEYS + _fused_keys(h)) for h in hits]

    async def search_code_propagated(self, query: str, limit: int = DEFAULT_SEARCH_LIMIT, language: str | list[str] | None = None,
                                     entity_type: str | None = None, project_name: str | list[str] | None = None, *,
                                     candidates: int | None = None, propagate: bool | dict | None = None, related_limit: int = 10,
                                     contains: str | list[str] | None = None, contains_case: bool = True, matches: str | None = None,
                                     fuzzy: str | None = None, edits: int | None = None, within_callers_of: str | list[str] | None = None,
                                     within_callees_of: str | list[str] | None = None, graph_hops: int | None = None, mode: str = "semantic",
                                     **others) -> dict:
        """:meth:`search_code` with graph-propagated relevance (``HipVectorStore.search_propagated``; not in the reference):
        ``{"results": [...], "related": [...]}``.  ``results`` have :meth:`search_code`'s shape plus ``cosine`` and
        ``graph_score``, ``score`` being the fused one; ``related`` -- ``[{"name", "qualified_name", "graph_score", "file_path",
        "entity_type", "start_line"}]`` -- are the nodes the walk from the matches ends up at that are no match themselves: the
        function all three retry wrappers call, whose body never says "retry".  The filters apply to the matches (the seeds),
        not to ``related``."""
        if not query or not query.strip():
            raise QueryError("Search query cannot be empty")
        used = [k for k, v in others.items() if v is not None] + ([] if mode == "semantic" else [f"mode={mode!r}"])
        if used:
            raise ValueError(f"propagate cannot be combined with {', '.join(used)}")
        filters = {k: v for k, v in (("language", language), ("entity_type", entity_type), ("project_name", project_name)) if v}
        filters.update(_contains_filter("content", contains, contains_case, matches, fuzzy, edits))
        filters.update(_graph_filter(within_callers_of, within_callees_of, graph_hops))
        try:
            vector = await self.embedder.embed(query)
            got = await self.qdrant.search_propagated(collection=CollectionName.CODE_CHUNKS.value, query_vector=vector, limit=limit,
                                                      candidates=candidates, propagate=None if propagate is True else propagate,
                                                      related_limit=related_limit, filters=filters or None)
        except EmbeddingError as e:
            logger.error(f"Embedding error: {e}")
            raise QueryError("Failed to embed search query", cause=e)
        except VectorStoreError as e:
            logger.error(f"Vector store error: {e}")
            raise QueryError("Failed to search code", cause=e)
        results = [dict(_project(h, _CODE_KEYS), cosine=h["cosine"], graph_score=h["graph_score"]) for h in got["hits"]]
        return {"results": results, "related": [_node_row(r) for r in got["related"]]}

    async def find_important_near(self, names, limit: int = 10, direction: str = "both", weights=None, restart: float = 0.15,
                                  steps: int = 16, include_seeds: bool = False, match: str = "exact") -> list[dict]:
        """What matters around ``names`` (one name or several): personalised PageRank over the store's ``"calls"`` edges seeded
        by them (``HipVectorStore.graph_rank``; not in the reference, whose only graded graph signal is a global degree count)
        -- ``[{"name", "qualified_name", "graph_score", "file_path", "entity_type", "start_line"}]``, best first, the named
        nodes themselves left out unless ``include_seeds``."""
        wanted = [names] if isinstance(names, str) else list(names or [])
        if not wanted or not all(isinstance(n, str) and n.strip() for n in wanted):
            raise QueryError("Entity name cannot be empty")
        try:
            got = await self.qdrant.graph_rank(collection=CollectionName.CODE_CHUNKS.value, names=wanted, weights=weights, direction=direction,
                                               restart=restart, steps=steps, limit=limit, match=match, include_seeds=include_seeds)
        except VectorStoreError as e:
            logger.error(f"Vector store error: {e}")
            raise QueryError("Failed to rank the call graph", cause=e)
        return [_node_row(r) for r in got["hits"]]

    async def search_summaries(self, query: str, limit: int = DEFAULT_SEARCH_LIMIT, project_name: str | None = None, *,
                               diversity: float | None = None, candidates: int | None = None, max_per_file: int | None = None,
                               extra_queries: list[str] | None = None, fusion: str = "rrf", min_score: float | None = None,
                               mode: str = "semantic", contains: str | list[str] | None = None, contains_case: bool = True,
                               matches: str | None = None, fuzzy: str | None = None, edits: int | None = None, within_callers_of: str | list[str] | None = None,
                               within_callees_of: str | list[str] | None = None, graph_hops: int | None = None,
                               between: tuple | list | None = None) -> list[dict]:
        """vector_search.py:118-166 (filters on ``project_name``, which summary payloads never carry: quirk Q6).
        ``extra_queries`` / ``fusion`` / ``min_score`` / ``mode`` as in :meth:`search_code`; ``contains`` / ``contains_case`` /
        ``matches`` likewise, over the ``summary`` text."""
        if not query or not query.strip():
            raise QueryError("Search query cannot be empty")
        filters = {"project_name": project_name} if project_name else None
        if contains is not None or matches is not None or fuzzy is not None or edits is not None:
            filters = dict(filters or {}, **_contains_filter("summary", contains, contains_case, matches, fuzzy, edits))
        if within_callers_of is not None or within_callees_of is not None or graph_hops is not None or between is not None:
            filters = dict(filters or {}, **_graph_filter(within_callers_of, within_callees_of, graph_hops, between=between))
        hits = await self._lookup(query, CollectionName.SUMMARIES.value, limit, filters,
                                  "Failed to embed search query", "Failed to search summaries", diversity=diversity, candidates=candidates,
                                  max_per_file=max_per_file, extra_queries=extra_queries, fusion=fusion, min_score=min_score,
                                  **_mode_kwargs(mode))
        return [_project(h, _SUMMARY_KEYS + _fused_keys(h)) for h in hits]

    async def find_similar_code(self, code_snippet: str, limit: int = DEFAULT_SEARCH_LIMIT, exclude_file: str | None = None,
                                exact_exclude: bool = False, *, diversity: float | None = None, candidates: int | None = None,
                                max_per_file: int | None = None, min_score: float | None = None,
                                max_overlap: float | None = None, contains: str | list[str] | None = None,
                                contains_case: bool = True, matches: str | None = None,
                                fuzzy: str | None = None, edits: int | None = None, within_callers_of: str | list[str] | None = None,
                                within_callees_of: str | list[str] | None = None, graph_hops: int | None = None,
                                in_cycle: bool | None = None, graph_depth: int | dict | None = None,
                                graph_height: int | dict | None = None, between: tuple | list | None = None) -> list[dict]:
        """vector_search.py:168-219: over-fetch by 5 when a file is excluded, drop its chunks, keep ``limit`` -- which comes
        back short when the excluded file owns more than 5 of the best hits.  ``exact_exclude=True`` (not in the reference)
        excludes the file on the device instead (``must_not={"file_path": exclude_file}``) and fetches exactly ``limit``.
        ``min_score`` as in :meth:`search_code`: only chunks at least that similar to the snippet.  ``max_overlap`` as in
        :meth:`search_code`: no chunk repeats more than that share of a better chunk's lines.  ``contains`` / ``contains_case``
        as in :meth:`search_code`: only chunks that hold the literal string(s); ``matches`` likewise: only chunks the regular
        expression matches.  ``in_cycle`` / ``graph_depth`` / ``graph_height`` / ``between`` as in :meth:`search_code`."""
        if not code_snippet or not code_snippet.strip():
            raise QueryError("Code snippet cannot be empty")
        on_device = bool(exact_exclude and exclude_file)
        fetch = limit + EXCLUDE_FILE_BUFFER if exclude_file and not on_device else limit
        hits = await self._lookup(code_snippet, CollectionName.CODE_CHUNKS.value, fetch,
                                  {**_contains_filter("content", contains, contains_case, matches, fuzzy, edits),
                                   **_graph_filter(within_callers_of, within_callees_of, graph_hops, in_cycle, graph_depth, graph_height, between)} or _NO_FILTER_KWARG,
                                  "Failed to embed code snippet", "Failed to find similar code",
                                  must_not={"file_path": exclude_file} if on_device else None, diversity=diversity, candidates=candidates,
                                  max_per_file=max_per_file, min_score=min_score, max_overlap=max_overlap)
        kept = []
        for h in hits:
            if exclude_file and h["payload"].get("file_path") == exclude_file:
                continue
            kept.append(_project(h, _SIMILAR_KEYS))
            if len(kept) >= limit:
                break
        return kept

    async def find_similar_to(self, positive_ids, negative_ids=None, limit: int = DEFAULT_SEARCH_LIMIT, strategy: str = "average",
                              language: str | list[str] | None = None, exclude_files: list[str] | None = None) -> list[dict]:
        """"Other functions like X" from hits the caller already holds (not in the reference, whose ``find_similar`` intent can
        only embed a snippet): ``positive_ids`` / ``negative_ids`` are point ids of code chunks -- nothing is embedded --
        answered by ``HipVectorStore.recommend`` (``strategy`` "average" or "best"), in the result shape of
        :meth:`find_similar_code`.  ``language`` filters, ``exclude_files`` drops whole files, both on the device; the example
        chunks themselves never come back."""
        positive = [positive_ids] if isinstance(positive_ids, str) else list(positive_ids or [])
        negative = [negative_ids] if isinstance(negative_ids, str) else list(negative_ids or [])
        if not positive:
            raise QueryError("find_similar_to needs at least one positive id")
        kwargs = {}
        if language:
            kwargs["filters"] = {"language": language}
        if exclude_files:
            kwargs["must_not"] = {"file_path": list(exclude_files)}
        try:
            hits = await self.qdrant.recommend(collection=CollectionName.CODE_CHUNKS.value, positive=positive, negative=negative, limit=limit,
                                               strategy=strategy, **kwargs)
        except VectorStoreError as e:
            logger.error(f"Vector store error: {e}")
            raise QueryError("Failed to find similar code", cause=e)
        return [_transform_similar_code_result(h) for h in hits]

    async def chunks_at(self, file_path: str, line: int, last_line: int | None = None) -> list[dict]:
        """The code chunks of ``file_path`` that cover line ``line`` -- or any line of ``line .. last_line`` -- in the result shape
        of :meth:`search_code` with ``score`` 0.0, in indexing order: what a stack frame, a diff hunk or the selection of an
        editor points at (not in the reference, whose ``ContextBuilder`` fetches a file's chunks and compares in Python).
        Nothing is embedded: one filter-only device call (``HipVectorStore.chunks_at``)."""
        if not file_path:
            raise QueryError("chunks_at needs a file path")
        try:
            payloads = await self.qdrant.chunks_at(collection=CollectionName.CODE_CHUNKS.value, file_path=file_path, line=line, last_line=last_line)
        except VectorStoreError as e:
            logger.error(f"Vector store error: {e}")
            raise QueryError("Failed to fetch the chunks at a line", cause=e)
        return [_project({"score": 0.0, "payload": p}, _CODE_KEYS) for p in payloads]

    async def facet_code(self, key: str = "file_path", query: str | None = None, min_score: float | None = None,
                         limit: int = DEFAULT_SEARCH_LIMIT, language: str | list[str] | None = None, entity_type: str | None = None,
                         project_name: str | list[str] | None = None, contains: str | list[str] | None = None,
                         contains_case: bool = True, matches: str | None = None, fuzzy: str | None = None,
                         edits: int | None = None, between: tuple | list | None = None, graph_hops: int | None = None) -> dict:
        """WHERE something lives, not which chunks (not in the reference, whose callers fetch hits and count them in Python):
        the ``limit`` most frequent values of ``key`` -- a file path, a language, an entity type -- among the code chunks that
        pass the filters, with their counts (``HipVectorStore.facet``): ``{"hits": [{"value", "count"}], "values", "total",
        "missing"}``.  ``contains`` / ``contains_case`` / ``matches`` / ``fuzzy`` / ``edits`` as in :meth:`search_code`: how many
        chunks per file hold ``TODO(``.  With ``query`` and ``min_score`` -- both or neither -- ``query`` is embedded and only chunks at least that
        similar to it count: in which files does this concept live.  Counts are exact; ties go to the value indexed first.
        ``between`` / ``graph_hops`` as in :meth:`search_code`: which files hold the code between two functions."""
        if (query is None) != (min_score is None):
            raise QueryError("facet_code: query and min_score come together or not at all")
        if query is not None and not query.strip():
            raise QueryError("Search query cannot be empty")
        filters = {k: v for k, v in (("language", language), ("entity_type", entity_type), ("project_name", project_name)) if v}
        filters.update(_contains_filter("content", contains, contains_case, matches, fuzzy, edits))
        if between is not None or graph_hops is not None:
            filters.update(_graph_filter(None, None, graph_hops, between=between))
        try:
            kwargs = {}
            if query is not None:
                kwargs = {"query_vector": await self.embedder.embed(query), "score_threshold": min_score}
            return await self.qdrant.facet(collection=CollectionName.CODE_CHUNKS.value, key=key, limit=limit, filters=filters or None, **kwargs)
        except EmbeddingError as e:
            logger.error(f"Embedding error: {e}")
            raise QueryError("Failed to embed search query", cause=e)
        except VectorStoreError as e:
            logger.error(f"Vector store error: {e}")
            raise QueryError("Failed to count code by value", cause=e)

    # ------------------------------------------------------------------ the call graph (query/graph_reasoning/engine.py's shapes)
    async def _graph_walk(self, name: str, direction: str, max_hops: int, limit: int) -> list[dict]:
        if not name or not name.strip():
            raise QueryError("Entity name cannot be empty")
        try:
            got = await self.qdrant.graph_neighbors(collection=CollectionName.CODE_CHUNKS.value, names=name, direction=direction,
                                                    max_hops=max_hops, limit=limit)
        except VectorStoreError as e:
            logger.error(f"Vector store error: {e}")
            raise QueryError(f"Failed to find transitive {direction}", cause=e)
        return [{"name": h["name"].rsplit(".", 1)[-1], "qualified_name": h["name"], "metadata": {"depth": h["depth"]}} for h in got["hits"]]

    async def find_callers(self, name: str, max_hops: int = 3, limit: int = 50) -> list[dict]:
        """What calls ``name``, transitively (``GraphReasoningEngine.find_transitive_callers``): the fields of its ``GraphNode``
        this store knows -- ``[{"name", "qualified_name", "metadata": {"depth"}}]`` -- by (depth, order of indexing), every
        caller once, at its least depth -- answered by the device
        BFS over the store's ``"calls"`` edges (``HipVectorStore.graph_neighbors``), no graph database asked."""
        return await self._graph_walk(name, "callers", max_hops, limit)

    async def find_callees(self, name: str, max_hops: int = 3, limit: int = 50) -> list[dict]:
        """What ``name`` calls, transitively (``find_transitive_callees``); the shape of :meth:`find_callers`."""
        return await self._graph_walk(name, "callees", max_hops, limit)

    async def find_call_chain(self, source: str, target: str, max_hops: int = 8) -> list[dict]:
        """How ``source`` reaches ``target`` (``find_call_chain``, whose ``GraphPath`` fields these are): ``[{"nodes": [names],
        "relationships": ["CALLS", ...], "total_length", "path_type": "call_chain"}]`` with ONE shortest chain of calls, both
        ends included -- or ``[]`` when there is none within ``max_hops`` calls (``HipVectorStore.call_chain``)."""
        if not source or not target:
            raise QueryError("find_call_chain needs a source and a target")
        try:
            chain = await self.qdrant.call_chain(collection=CollectionName.CODE_CHUNKS.value, source=source, target=target, max_hops=max_hops)
        except VectorStoreError as e:
            logger.error(f"Vector store error: {e}")
            raise QueryError("Failed to find a call chain", cause=e)
        if not chain:
            return []
        return [{"nodes": chain, "relationships": ["CALLS"] * (len(chain) - 1), "total_length": len(chain) - 1, "path_type": "call_chain"}]

    async def find_call_chains(self, source, target: str, max_hops: int = 8, limit: int = 10, must_pass: bool = True, relation: str = "calls",
                               match: str = "exact") -> dict:
        """How ``source`` (a name or several) reaches ``target``, in full (``HipVectorStore.call_chains``; the reference's
        FIND_ALL_PATHS lists every path up to its bound, this the SHORTEST ones): ``{"count", "saturated", "length", "chains":
        [[names]], "must_pass": [names], "unresolved"}`` -- how many shortest chains of at most ``max_hops`` calls there are,
        the first ``limit`` of them, and the functions no way of at most ``max_hops`` calls avoids."""
        if not source or not target:
            raise QueryError("find_call_chains needs a source and a target")
        try:
            return await self.qdrant.call_chains(collection=CollectionName.CODE_CHUNKS.value, source=source, target=target, relation=relation,
                                                 max_hops=max_hops, limit=limit, must_pass=must_pass, match=match)
        except VectorStoreError as e:
            logger.error(f"Vector store error: {e}")
            raise QueryError("Failed to find the call chains", cause=e)

    async def find_cycles(self, limit: int = 10, relation: str = "calls", members: int = 50) -> dict:
        """Which functions are (mutually) recursive -- with ``relation="imports"``: which modules depend on each other in a
        circle (``HipVectorStore.graph_cycles``; not in the reference, whose Cypher has no query for it): ``{"cycles": [{"name",
        "qualified_name", "size", "members": [qualified names], "self_recursive": [...]}], "count", "nodes", "self_recursive"}``,
        the largest cycle first; ``name`` is that of the member indexed first."""
        try:
            got = await self.qdrant.graph_cycles(collection=CollectionName.CODE_CHUNKS.value, relation=relation, limit=limit, members=members)
        except VectorStoreError as e:
            logger.error(f"Vector store error: {e}")
            raise QueryError("Failed to find the call cycles", cause=e)
        cycles = [{"name": c["id"].rsplit(".", 1)[-1], "qualified_name": c["id"], "size": c["size"], "members": c["nodes"],
                   "self_recursive": c["self_recursive"]} for c in got["components"]]
        return {"cycles": cycles, "count": got["count"], "nodes": got["nodes"], "self_recursive": got["self_recursive"]}

    async def find_layers(self, names=None, relation: str = "calls", match: str = "exact") -> dict:
        """Entry points, leaf utilities, a reading order (``HipVectorStore.graph_layers``; not in the reference): ``{"layers",
        "histogram": {"depth", "height"}, "nodes": [{"name", "qualified_name", "depth", "height", "component", "cyclic"}]}`` --
        ``depth`` 0: nobody outside its own cycle calls it; ``height`` 0: it calls nothing outside its own cycle."""
        try:
            got = await self.qdrant.graph_layers(collection=CollectionName.CODE_CHUNKS.value, relation=relation, names=names, match=match)
        except VectorStoreError as e:
            logger.error(f"Vector store error: {e}")
            raise QueryError("Failed to layer the call graph", cause=e)
        nodes = [dict(n, name=n["name"].rsplit(".", 1)[-1], qualified_name=n["name"]) for n in got["nodes"]]
        return {**got, "nodes": nodes}

    # ------------------------------------------------------------------ batch entry (not in the reference)
    async def search_code_batch(self, queries, limit: int = DEFAULT_SEARCH_LIMIT, language: str | list[str] | None = None,
                                entity_type: str | None = None, project_name: str | list[str] | None = None, *,
                                diversity: float | None = None, candidates: int | None = None,
                                max_per_file: int | None = None,
                                filters_per_query: list[dict | None] | None = None, min_score=None,
                                max_overlap: float | None = None, mode: str = "semantic", contains: str | list[str] | None = None,
                                contains_case: bool = True, matches: str | None = None,
                                fuzzy: str | None = None, edits: int | None = None, within_callers_of: str | list[str] | None = None,
                                within_callees_of: str | list[str] | None = None, graph_hops: int | None = None,
                                in_cycle: bool | None = None, graph_depth: int | dict | None = None,
                                graph_height: int | dict | None = None, between: tuple | list | None = None) -> list[list[dict]]:
        """``queries``: list of strings (embedded in one provider batch) or an array [B, dim] of ready vectors.
        ``mode`` "lexical" / "hybrid" as in :meth:`search_code` (``queries`` must be strings then; the filters and
        ``candidates`` only).
        ``filters_per_query``: one filter dict (keys ``language`` / ``entity_type`` / ``project_name``; None = no filter) per
        query -- every query is answered under its own, and the batch still shares corpus passes (up to 8 distinct filters per
        64 queries).  Mutually exclusive with the scalar ``language`` / ``entity_type`` / ``project_name``, where a list already
        means "any of"; not combinable with ``diversity`` / ``max_per_file`` yet.  ``min_score``: one number or one per query, as in
        :meth:`search_code`; not together with ``filters_per_query`` either.  ``max_overlap`` as in :meth:`search_code`; not
        together with ``filters_per_query``, ``diversity``, ``max_per_file`` or ``min_score``.  ``contains`` / ``contains_case`` as in
        :meth:`search_code`, one text condition for the whole batch; not together with ``filters_per_query``.  ``matches`` likewise;
        ``between`` likewise: one graph condition for the whole batch."""
        filters = {k: v for k, v in (("language", language), ("entity_type", entity_type), ("project_name", project_name)) if v}
        if (contains is not None or matches is not None or fuzzy is not None or edits is not None) and filters_per_query is not None:
            raise QueryError("contains / matches / fuzzy cannot be combined with filters_per_query (a text condition is one grep for the whole batch)")
        filters.update(_contains_filter("content", contains, contains_case, matches, fuzzy, edits))
        if (within_callers_of is not None or within_callees_of is not None) and filters_per_query is not None:
            raise QueryError("within_callers_of / within_callees_of cannot be combined with filters_per_query (a graph condition is one BFS for the whole batch)")
        if (in_cycle or graph_depth is not None or graph_height is not None) and filters_per_query is not None:
            raise QueryError("in_cycle / graph_depth / graph_height cannot be combined with filters_per_query (a graph condition is one bitmap for the whole batch)")
        if between is not None and filters_per_query is not None:
            raise QueryError("between cannot be combined with filters_per_query (a graph condition is one bitmap for the whole batch)")
        filters.update(_graph_filter(within_callers_of, within_callees_of, graph_hops, in_cycle, graph_depth, graph_height, between))
        if filters_per_query is not None:
            if filters:
                raise QueryError("filters_per_query cannot be combined with language / entity_type / project_name")
            if len(filters_per_query) != len(queries):
                raise QueryError(f"filters_per_query has {len(filters_per_query)} entries for {len(queries)} queries")
            filters = [({k: v for k, v in f.items() if v} or None) if f else None for f in filters_per_query]
        if mode != "semantic":
            return await self._batch_keyword(queries, limit, filters or None, candidates, mode, diversity=diversity, max_per_file=max_per_file,
                                             filters_per_query=filters_per_query, min_score=min_score, max_overlap=max_overlap)
        try:
            if isinstance(queries, np.ndarray) or (hasattr(queries, "shape") and not isinstance(queries, (list, tuple))):
                vectors = queries
            else:
                texts = list(queries)
                if any((not t or not t.strip()) for t in texts):
                    raise QueryError("Search query cannot be empty")
                vectors = np.asarray(await self.embedder.embed_batch(texts), dtype=np.float32)
            per_query = await self.qdrant.search_batch(collection=CollectionName.CODE_CHUNKS.value, query_vectors=vectors,
                                                       limit=limit, filters=filters or None, **_mmr_kwargs(diversity, candidates),
                                                       **_group_kwargs(max_per_file), **_threshold_kwargs(min_score),
                                                       **_overlap_kwargs(max_overlap))
        except EmbeddingError as e:
            raise QueryError("Failed to embed search query", cause=e)
        except VectorStoreError as e:
            raise QueryError("Failed to search code", cause=e)
        return [[_project(h, _CODE_KEYS) for h in hits] for hits in per_query]

    async def _batch_keyword(self, queries, limit: int, filters, candidates, mode: str, **others) -> list[list[dict]]:
        if mode not in ("lexical", "hybrid"):
            raise QueryError(f"unknown search mode {mode!r} (one of 'semantic', 'lexical', 'hybrid')")
        used = [k for k, v in others.items() if v is not None]
        if used:
            raise QueryError(f"mode={mode!r} cannot be combined with {', '.join(used)}")
        texts = list(queries) if isinstance(queries, (list, tuple)) else None
        if texts is None or any((not isinstance(t, str) or not t.strip()) for t in texts):
            raise QueryError(f"mode={mode!r} needs the query texts")
        try:
            col = CollectionName.CODE_CHUNKS.value
            if mode == "lexical":
                per_query = await self.qdrant.search_lexical_batch(collection=col, texts=texts, limit=limit, filters=filters)
            else:
                vectors = np.asarray(await self.embedder.embed_batch(texts), dtype=np.float32)
                kw = {} if candidates is None else {"candidates": candidates}
                per_query = await self.qdrant.search_hybrid_batch(collection=col, query_vectors=vectors, texts=texts, limit=limit, filters=filters, **kw)
                for hits in per_query:
                    for h in hits:
                        h["payload"] = dict(h["payload"], cosine=h["cosine"], lexical_score=h["lexical_score"], matched=h["matched"])
        except EmbeddingError as e:
            raise QueryError("Failed to embed search query", cause=e)
        except VectorStoreError as e:
            raise QueryError("Failed to search code", cause=e)
        return [[_project(h, _CODE_KEYS + _fused_keys(h)) for h in hits] for hits in per_query]
