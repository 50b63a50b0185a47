"""The graph + vector scenarios of tests/hybrid_cases.py on the host: the restated HybridRanker equals the rows the REFERENCE's
ranker produced for them (tests/golden/ranking_hybrid_reference.json), and the set holds every situation the device kernel has to
get right -- so the goldens and the restatement agree before the device is involved."""
import json
import os

import pytest

import coderag_amd  # noqa: F401
from coderag_amd.query_types import ExtractedEntity, GraphContext, GraphNode, QueryIntent, QueryPlan
from coderag_amd.ranking import HybridRanker
from tests import hybrid_cases

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ranking_hybrid_reference.json")))
SIGNALS = ("graph_match", "query_entity_match", "relationship_relevance", "centrality", "context_richness", "vector_similarity",
           "code_quality")


def build_inputs(s):
    plan = QueryPlan(original_query=s["name"], primary_intent=QueryIntent(s["intent"]), entities=[ExtractedEntity(name=e) for e in s["entities"]])
    ctx = GraphContext(**{role: [GraphNode(**n) for n in s["graph"].get(role, [])] for role in hybrid_cases.ROLES})
    return plan, ctx, [dict(v) for v in s["vector"]], s["centrality"]


def rows_of(ranked):
    return [[r.entity_name, r.file_path, r.start_line, getattr(r.source, "value", r.source), r.final_score] + [r.signal_scores.get(s) for s in SIGNALS]
            for r in ranked]


@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: c["name"])
def test_host_ranker_matches_reference_on_hybrid_scenarios(case):
    sc = hybrid_cases.scenario(int(case["name"].split("_")[1]))
    assert rows_of(HybridRanker().rank_results(*build_inputs(sc))) == case["rows"]


def test_golden_file_is_the_generators():
    assert len(GOLD["cases"]) == hybrid_cases.N_HYBRID and GOLD["seed"] == hybrid_cases.HSEED and GOLD["columns"][5:] == list(SIGNALS)
    gold_dir = os.path.join(os.path.dirname(__file__), "golden")
    assert os.path.getsize(os.path.join(gold_dir, "ranking_hybrid_reference.json")) <= os.path.getsize(
        os.path.join(gold_dir, "ranking_vector_only_reference.json"))


def test_no_scenario_is_one_the_device_declines():
    for sc in hybrid_cases.scenarios():
        ents = {e.lower().encode() for e in sc["entities"]}
        assert len(ents) <= 8 and all(len(e) <= 48 for e in ents), sc["name"]
        for _, d in hybrid_cases.candidates(sc):
            assert len((d["name"] if "name" in d else d["entity_name"]).lower().encode()) <= 64, sc["name"]
        assert len(hybrid_cases.candidates(sc)) <= hybrid_cases.MAX_CANDIDATES
        assert all(h["score"] * 4096 == int(h["score"] * 4096) for h in sc["vector"])           # exact in f32
        assert all(1 <= hybrid_cases.depth_of(n) <= 7 for r in ("callers", "callees") for n in sc["graph"][r])
        # the table holds what the engine can have looked up: keys of primaries and of named hits (engine.py:353-363)
        allowed = {hybrid_cases.node_key(n) for n in sc["graph"]["primary_entities"]} | {hybrid_cases.node_key(h) for h in sc["vector"] if h["entity_name"]}
        assert set(sc["centrality"] or {}) <= allowed


def test_hybrid_scenarios_cover_the_branches():
    """Counted on the inputs (who shares a merge key with whom) and on the host ranker's output."""
    graph_vector = graph_graph = three_way = ties = per_file_cap = total_cap = 0
    for sc in hybrid_cases.scenarios():
        groups = {}
        for role, d in hybrid_cases.candidates(sc):
            groups.setdefault(hybrid_cases.merge_key(d), []).append(role)
        for roles in groups.values():
            n_graph = sum(r is not None for r in roles)
            graph_vector += n_graph >= 1 and n_graph < len(roles)
            graph_graph += n_graph >= 2
            three_way += len(roles) >= 3
        ranker = HybridRanker()
        ranked = ranker.rank_results(*build_inputs(sc))
        assert all((r.source == "hybrid") == (len(groups[r.get_key()]) > 1) for r in ranked)
        # an exact tie between an unmerged graph entry and an unmerged vector entry that both survive
        for a, b in zip(ranked, ranked[1:]):
            ties += a.final_score == b.final_score and {a.source, b.source} == {"graph", "vector"}
        files = {}
        for r in ranked:
            files[r.file_path] = files.get(r.file_path, 0) + 1
        per_file_cap += len(groups) > len(ranked) and max(files.values(), default=0) == ranker.config.max_per_file
        total_cap += len(ranked) == ranker.config.max_total
    assert graph_vector >= 10 and graph_graph >= 10 and three_way >= 10, (graph_vector, graph_graph, three_way)
    assert ties >= 8 and per_file_cap >= 10 and total_cap >= 2, (ties, per_file_cap, total_cap)
    assert {row[3] for c in GOLD["cases"] for row in c["rows"]} == {"graph", "vector", "hybrid"}
    # signals absent from a result are null in the goldens, present ones numbers -- both occur for every signal
    for t in range(len(SIGNALS)):
        col = [row[5 + t] for c in GOLD["cases"] for row in c["rows"]]
        assert any(v is None for v in col) == (SIGNALS[t] not in ("query_entity_match", "centrality")) and any(v is not None for v in col)


def test_segment_table_order():
    """The reference's order: all primaries, caller lists in primary order, callee lists, methods, parents, children."""
    from coderag_amd.ranking.device import segment_table
    per_query = [[(2, -1, 4, 10), (0, 11, -1, 0), (1, -1, 0, 10), (5, -1, 9, 2), (0, 12, -1, 0), (1, -1, 1, 10), (3, -1, 7, 4), (2, -1, 5, 10), (4, -1, 8, 1)], []]
    segs, G = segment_table(per_query)
    assert segs == [(0, 0, 11, -1, 0), (0, 0, 12, -1, 0), (0, 1, -1, 0, 10), (0, 1, -1, 1, 10), (0, 2, -1, 4, 10), (0, 2, -1, 5, 10), (0, 3, -1, 7, 4),
                    (0, 4, -1, 8, 1), (0, 5, -1, 9, 2)] and G == 49
    assert segment_table([[], []]) == ([], 0)


# ---- plan_graph_roles: execute_query_plan's decisions against hand-written expectations (graph_reasoning/engine.py:25-84, 329-452)
class _Info:
    """A graph of eight named nodes; node 1 and 6 are classes."""
    names = ["pkg.a.f", "pkg.a.Repo", "pkg.b.g", "pkg.b.h", "pkg.c.f", "main", "pkg.c.Base", "pkg.d.k"]

    def __init__(self, relations=("calls", "extends", "has_method")):
        self.relations = set(relations)

    def resolve(self, name, match):
        from coderag_amd import graph
        return graph.resolve(name, {n: i for i, n in enumerate(self.names)}, self.names, match)[0]

    def is_class(self, node):
        return node in (1, 6)


def _plan(intent, names, primary=(), multi_hop=False, max_hops=1):
    return QueryPlan(original_query="q", primary_intent=QueryIntent(intent), requires_multi_hop=multi_hop, max_hops=max_hops,
                     entities=[ExtractedEntity(name=n, is_primary=n in primary) for n in names])


def test_plan_graph_roles_per_intent_family():
    from coderag_amd.engine_helpers import GraphWalk as W, plan_graph_roles
    info = _Info()
    # callers / usages: one walk per primary, 1 hop unless the plan is multi-hop; hops clipped at 5; 50 per source
    assert plan_graph_roles(_plan("find_callers", ["main"]), info) == ([5], [W(1, "calls", "callers", 5, 1, 50)])
    assert plan_graph_roles(_plan("find_usages", ["main"], multi_hop=True, max_hops=3), info).walks == [W(1, "calls", "callers", 5, 3, 50)]
    assert plan_graph_roles(_plan("find_callers", ["main"], multi_hop=True, max_hops=9), info).walks == [W(1, "calls", "callers", 5, 5, 50)]
    assert plan_graph_roles(_plan("find_callers", ["main"], multi_hop=False, max_hops=4), info).walks == [W(1, "calls", "callers", 5, 1, 50)]
    # "exact" first, "suffix" when nothing matches exactly: f is pkg.a.f and pkg.c.f; a suffix of nothing resolves to nothing
    got = plan_graph_roles(_plan("find_callees", ["f"], multi_hop=True, max_hops=2), info)
    assert got == ([0, 4], [W(2, "calls", "callees", 0, 2, 50), W(2, "calls", "callees", 4, 2, 50)])
    assert plan_graph_roles(_plan("find_callees", ["pkg.a.f"]), info).primaries == [0]
    # no primaries: nothing is walked, whatever the intent
    for intent in ("find_callers", "find_callees", "find_hierarchy", "explain_implementation", "search_functionality", "find_call_chain"):
        assert plan_graph_roles(_plan(intent, ["nowhere", "zzz"]), info) == ([], [])
        assert plan_graph_roles(_plan(intent, []), info) == ([], [])
    # only the first entity resolves while there is no primary yet -- unless others are marked primary (engine.py:44-47)
    assert plan_graph_roles(_plan("find_callers", ["main", "g"]), info).primaries == [5]
    assert plan_graph_roles(_plan("find_callers", ["main", "g", "h"], primary=("h",)), info).primaries == [5, 3]
    assert plan_graph_roles(_plan("find_callers", ["zzz", "g", "h"]), info).primaries == [2]
    assert plan_graph_roles(_plan("find_callers", ["main", "main"], primary=("main",)), info).primaries == [5, 5]        # repeats stay
    # hierarchy: a class walks "extends" both ways within 5, anything else its callers
    got = plan_graph_roles(_plan("find_hierarchy", ["Repo", "g"], primary=("Repo", "g")), info)
    assert got == ([1, 2], [W(4, "extends", "callees", 1, 5, 50), W(5, "extends", "callers", 1, 5, 50), W(1, "calls", "callers", 2, 1, 50)])
    assert plan_graph_roles(_plan("find_implementations", ["Repo"]), _Info(("calls",))).walks == []                     # no "extends" relation
    # explain_implementation: direct callers and callees, 10 each, and a class's methods
    got = plan_graph_roles(_plan("explain_implementation", ["Base"], multi_hop=True, max_hops=4), info)
    assert got.walks == [W(1, "calls", "callers", 6, 1, 10), W(2, "calls", "callees", 6, 1, 10), W(3, "has_method", "callees", 6, 1, 50)]
    assert plan_graph_roles(_plan("explain_implementation", ["Base"]), _Info(("calls",))).walks == [W(1, "calls", "callers", 6, 1, 10), W(2, "calls", "callees", 6, 1, 10)]
    # call chain / dependencies / dependents: primaries only
    for intent in ("find_call_chain", "find_dependencies", "find_dependents"):
        assert plan_graph_roles(_plan(intent, ["main", "g"], primary=("main", "g")), info) == ([5, 2], [])
    # the comprehensive default: the first 3 of more than 3 primaries, 2 hops, 10 per source
    names = ["main", "g", "Repo", "h", "k"]
    got = plan_graph_roles(_plan("search_functionality", names, primary=names, multi_hop=True, max_hops=5), info)
    assert got.primaries == [5, 2, 1, 3, 7]
    assert got.walks == [W(1, "calls", "callers", 5, 2, 10), W(2, "calls", "callees", 5, 2, 10), W(1, "calls", "callers", 2, 2, 10), W(2, "calls", "callees", 2, 2, 10),
                         W(1, "calls", "callers", 1, 2, 10), W(2, "calls", "callees", 1, 2, 10), W(3, "has_method", "callees", 1, 1, 50)]
    assert plan_graph_roles(_plan("locate_entity", ["main"]), info).walks == [W(1, "calls", "callers", 5, 2, 10), W(2, "calls", "callees", 5, 2, 10)]
