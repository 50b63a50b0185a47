"""The hybrid re-rank with both branches on the device (crh_graph_node_rows, crh_graph_candidates, crh_rerank_hybrid; DESIGN.md
3.28).  Every comparison is exact -- order, source label, f64 score bits, the signal values and WHICH signals a result carries:
hit scores are exact in f32 and the kernel's arithmetic is f64 in the reference's operand order, so no tolerance is needed."""
import json
import os
import random
from types import SimpleNamespace as NS

import numpy as np
import pytest

from tests import hybrid_cases

pytestmark = pytest.mark.gpu

ROLE_INDEX = {r: i for i, r in enumerate(hybrid_cases.ROLES)}     # == CRH_ROLE_*


def node_payload(n):
    """A graph node as a row of its own: the payload whose side columns and richness bits the kernel reads for it."""
    return {"file_path": n["file_path"], "entity_name": n["name"], "entity_type": n["node_type"], "start_line": n["start_line"],
            "end_line": n["end_line"], "graph_node_id": n["qualified_name"], "summary": n["summary"], "docstring": n["docstring"],
            "signature": n["signature"]}


class Batch:
    """Scenarios (hybrid_cases shape) -> SideColumns / RichnessColumn / candidate tables -> ONE crh_rerank_hybrid launch."""

    def __init__(self, scenarios, G=None, k=None, degree_of=None, **reranker):
        import torch
        from coderag_amd.ranking.device import GraphTable, HybridDeviceReranker, RichnessColumn, SideColumns, node_key
        self.scenarios = scenarios
        nq = len(scenarios)
        self.G = G = max(sum(len(v) for v in s["graph"].values()) for s in scenarios) if G is None else G
        self.k = k = max(len(s["vector"]) for s in scenarios) if k is None else k
        payloads, degree = [], []
        g_row = np.full((nq, G), -1, np.int64)
        g_role, g_depth = np.full((nq, G), -1, np.int32), np.full((nq, G), -1, np.int32)
        rows, scores = np.full((nq, k), -1, np.int64), np.full((nq, k), -np.inf, np.float32)
        self.items, self.plans = [], []
        for q, s in enumerate(scenarios):
            cent = s["centrality"] or {}
            deg = degree_of or (lambda p: int(cent[node_key(p)]["total_degree"]) if node_key(p) in cent else -1)
            items = []
            for role, n in hybrid_cases.candidates(s)[: len(hybrid_cases.candidates(s)) - len(s["vector"])]:
                p = node_payload(n)
                g_row[q, len(items)], g_role[q, len(items)] = len(payloads), ROLE_INDEX[role]
                g_depth[q, len(items)] = hybrid_cases.depth_of(n) if role in ("callers", "callees") else 0
                items.append(p)
                payloads.append(p)
                degree.append(deg(p))
            for j, h in enumerate(s["vector"]):
                rows[q, j], scores[q, j] = len(payloads), h["score"]
                payloads.append(h)
                degree.append(deg(h))
            self.items.append(items)
            self.plans.append(NS(primary_intent=s["intent"], entities=[NS(name=e) for e in s["entities"]]))
        side, rich = SideColumns(0), RichnessColumn(0)
        side.append(payloads)
        rich.append(payloads)
        if payloads:
            side.set_int_column("degree", degree)
        dev = torch.device("cuda:0")
        up = lambda a: torch.from_numpy(a).to(dev)
        self.table = GraphTable(up(np.where(g_row >= 0, 7, -1).astype(np.int32)), up(g_row), up(g_role), up(g_depth)) if G else None
        self.rows_d, self.scores_d = (up(rows), up(scores)) if k else (None, None)
        self.rr = HybridDeviceReranker(**reranker)
        self.out = self.rr.rank(self.table, side.gather(self.table.row) if G else None, rich.gather(self.table.row) if G else None, self.scores_d,
                                self.rows_d, side.gather(self.rows_d) if k else None, self.plans)
        self.side = side

    def results(self, q):
        from coderag_amd.ranking.device import HybridDeviceReranker
        return HybridDeviceReranker.materialise(self.out, q, self.items[q], self.scenarios[q]["vector"])


SIGNALS = ("graph_match", "query_entity_match", "relationship_relevance", "centrality", "context_richness", "vector_similarity",
           "code_quality")


# ---- 1. the kernel against the REFERENCE's own outputs: every scenario of tests/hybrid_cases.py in one launch
def test_hybrid_kernel_matches_reference_goldens(gpu):
    import coderag_amd  # noqa: F401
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ranking_hybrid_reference.json")))
    scs = hybrid_cases.scenarios()
    assert [c["name"] for c in gold["cases"]] == [s["name"] for s in scs]
    # the goldens hand the ranker a ready centrality table: every primary and every named hit may be in it
    G = max(sum(len(v) for v in s["graph"].values()) for s in scs)
    k = max(len(s["vector"]) for s in scs)
    b = Batch(scs, primary_top=G, centrality_top=k, centrality_limit=G + k)
    assert G + k <= 512 and int((b.out.count < 0).sum()) == 0                      # declined scenarios: 0
    for q, c in enumerate(gold["cases"]):
        got = [[r.entity_name, r.file_path, r.start_line, r.source, r.final_score] + [r.signal_scores.get(s) for s in SIGNALS] for r in b.results(q)]
        assert got == c["rows"], c["name"]


# ---- 2. the kernel against the host ranker on edges
def host_rank(s, primary_top=5, centrality_top=5, limit=10, degrees=None, config=None):
    """HybridRanker on the scenario, with the centrality table the ENGINE would have looked up (engine.py:348-377 as
    engine_helpers.centrality_candidates states it, with its three numbers as parameters) from per-key degrees."""
    from coderag_amd.query_types import GraphContext, GraphNode
    from coderag_amd.ranking import HybridRanker
    ctx = GraphContext(**{role: [GraphNode(**n) for n in s["graph"].get(role, [])] for role in hybrid_cases.ROLES})
    names = {}
    for n in ctx.primary_entities[:primary_top]:
        names[n.qualified_name or n.name] = None
    for h in s["vector"][:centrality_top]:
        if h.get("entity_name"):
            names[h.get("graph_node_id") or h.get("entity_name")] = None
    names = list(names)[:limit]
    degrees = degrees if degrees is not None else {key: v["total_degree"] for key, v in (s["centrality"] or {}).items()}
    plan = NS(primary_intent=s["intent"], entities=[NS(name=e) for e in s["entities"]])
    return HybridRanker(config).rank_results(plan, ctx, [dict(h) for h in s["vector"]], {n: {"total_degree": degrees[n]} for n in names if n in degrees})


def assert_same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        for f in ("file_path", "entity_name", "entity_type", "start_line", "end_line", "source", "final_score", "signal_scores", "qualified_name",
                  "graph_node_id", "relationship_path", "depth_from_query", "content", "summary", "signature", "docstring"):
            assert getattr(g, f) == getattr(w, f), (what, i, f, getattr(g, f), getattr(w, f))


def _sized(seed, n_graph, n_hits, **over):
    """A scenario with exactly n_graph graph nodes (spread over the roles) and n_hits hits, drawn like hybrid_cases.scenario."""
    rng = random.Random(seed)
    files = hybrid_cases.FILES + [f"pkg/m{j}.py" for j in range(40)]
    hot = [(rng.choice(hybrid_cases.NAMES), rng.choice(files), 1) for _ in range(4)]
    graph = {r: [] for r in hybrid_cases.ROLES}
    for _ in range(n_graph):
        role = rng.choice(hybrid_cases.ROLES)
        graph[role].append(hybrid_cases._node(rng, role in ("callers", "callees"), files, hot))
    scores = sorted((rng.randrange(-800, 4097) / 4096.0 for _ in range(n_hits)), reverse=True)
    vector = [hybrid_cases._hit(rng, s, files, hot) for s in scores]
    keys = sorted({hybrid_cases.node_key(d) for _, d in hybrid_cases.candidates(dict(graph=graph, vector=vector))})
    cent = {key: {"total_degree": rng.choice([0, 3, 25, 49, 50, 51, 120])} for key in keys if rng.random() < 0.7}
    s = dict(name=f"sized_{n_graph}_{n_hits}", intent=rng.choice(hybrid_cases.INTENTS), entities=rng.sample(hybrid_cases.ENTITIES, rng.randrange(0, 4)),
             graph=graph, vector=vector, centrality=cent)
    s.update(over)
    return s


def _all_degrees(s):
    """Per-key degrees for EVERY row (the store's degree column knows every node, whether the engine looks it up or not)."""
    cent = s["centrality"] or {}
    from coderag_amd.ranking.device import node_key
    return lambda p: int(cent[node_key(p)]["total_degree"]) if node_key(p) in cent else -1


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 512])
def test_hybrid_kernel_matches_host_at_every_size(gpu, n):
    import coderag_amd  # noqa: F401
    splits = sorted({(0, n), (n, 0), (n // 2, n - n // 2), (min(n, 3), n - min(n, 3))})
    scs = [_sized(100 * n + j, g, v) for j, (g, v) in enumerate(splits)]
    for s in scs:                           # one launch each: G and k are exact, no padding
        b = Batch([s], degree_of=_all_degrees(s))
        assert b.G + b.k == n and b.out.count[0] >= 0
        assert_same(b.results(0), host_rank(s), s["name"])


def test_padded_batch_and_all_padding_lists(gpu):
    """Scenarios of different sizes share one launch (padding in both tables); a query without any candidate gives an empty list."""
    import coderag_amd  # noqa: F401
    scs = [_sized(7, 5, 9), _sized(8, 0, 0), _sized(9, 30, 2), _sized(10, 0, 17), _sized(11, 12, 0)]
    cent = {}
    for s in scs:
        cent.update(s["centrality"])
    for s in scs:
        s["centrality"] = {key: v for key, v in cent.items()}                  # one degree per key across the batch
    b = Batch(scs, G=32, k=20, degree_of=lambda p: _all_degrees(dict(centrality=cent))(p))
    assert b.out.count[1] == 0 and (b.out.index[1] == -1).all()
    for q, s in enumerate(scs):
        assert_same(b.results(q), host_rank(s), s["name"])
        cnt = int(b.out.count[q])
        assert (b.out.index[q, cnt:] == -1).all() and (b.out.score[q, cnt:] == 0).all() and (b.out.mask[q, cnt:] == 0).all()


def test_no_graph_entries_equals_the_vector_kernel(gpu):
    """G = 0: index, score bits, the four vector signals, the hybrid flag and the count equal crh_rerank_vector's on the same lists."""
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd.ranking.device import DeviceReranker
    scs = [_sized(40 + j, 0, v) for j, v in enumerate([1, 5, 37, 100, 128])]
    for s in scs:
        s["centrality"] = {key: v for key, v in list(s["centrality"].items())[:12]}       # the vector kernel's table holds 16 keys
    b = Batch(scs, centrality_top=128, centrality_limit=512)
    ref = DeviceReranker(centrality_top=128).rank(b.scores_d, b.rows_d, b.side.gather(b.rows_d), b.plans)
    assert np.array_equal(ref.count, b.out.count) and (ref.count > 0).all()
    assert np.array_equal(ref.index, b.out.index) and np.array_equal(ref.score.view(np.int64), b.out.score.view(np.int64))
    assert np.array_equal(ref.hybrid, b.out.hybrid)
    assert np.array_equal(ref.signals.view(np.int64), b.out.signals[:, :, [5, 1, 3, 6]].view(np.int64))
    live = b.out.index >= 0
    assert (b.out.mask[live] == 0x6a).all() and (b.out.mask[~live] == 0).all()
    del torch


def _node(name, file, line, role_depth=None, **kw):
    return dict(node_type="function", name=name, qualified_name=kw.pop("qn", name), file_path=file, start_line=line, end_line=line + 3,
                signature=kw.get("signature"), docstring=kw.get("docstring"), summary=kw.get("summary"),
                metadata={} if role_depth is None else {"depth": role_depth})


def _hit(score, name, file, line, n=150, gid=None, summary=None):
    return dict(score=score, file_path=file, entity_type="function", entity_name=name, language="python", content=("x" * n) if n else None,
                start_line=line, end_line=line + 5, graph_node_id=gid, summary=summary)


def _graph(**roles):
    return {r: roles.get(r, []) for r in hybrid_cases.ROLES}


def test_scripted_edges(gpu):
    import coderag_amd  # noqa: F401
    scs = []
    # a key shared by 5 entries across both sources: primary + caller + method absorb two hits, signals are the union
    scs.append(dict(name="five_way", intent="find_callers", entities=["shared"], centrality={"shared": {"total_degree": 30}},
                    graph=_graph(primary_entities=[_node("shared", "a.py", 1, summary="S")], callers=[_node("shared", "a.py", 1, 3, docstring="D")],
                                 methods=[_node("shared", "a.py", 1, signature="def shared()")]),
                    vector=[_hit(0.75, "shared", "a.py", 1, n=0, summary="from hit"), _hit(0.5, "shared", "a.py", 1, n=150), _hit(0.25, "other", "a.py", 2)]))
    # an empty-string entity is a substring of every name (quirk Q8), also of a graph node's
    scs.append(dict(name="empty_entity", intent="find_callees", entities=[""], centrality=None,
                    graph=_graph(primary_entities=[_node("alpha", "a.py", 1)], callees=[_node("", "b.py", 2, 1)]), vector=[_hit(0.5, "beta", "c.py", 3)]))
    # depth 0 / 1 / 5 / 9 and a node without metadata, on both sides of the 0.3 floor, callers and callees
    scs.append(dict(name="depths", intent="find_usages", entities=[], centrality=None,
                    graph=_graph(callers=[_node(f"c{d}", f"c{d}.py", 1, d) for d in (0, 1, 2, 4, 5, 9)] + [_node("c_none", "cn.py", 1)],
                                 callees=[_node(f"e{d}", f"e{d}.py", 1, d) for d in (0, 1, 2, 4, 5, 9)]), vector=[]))
    # graph + graph merge without any hit: source "hybrid"
    scs.append(dict(name="graph_graph", intent="find_hierarchy", entities=["base"], centrality=None,
                    graph=_graph(parent_classes=[_node("Base", "b.py", 3, summary="S")], child_classes=[_node("Base", "b.py", 3, docstring="D")]), vector=[]))
    # a hit first in a group is impossible (graph entries come first) -- but a hit absorbing a later HIT next to a graph entry of another key
    scs.append(dict(name="hit_hit", intent="search_functionality", entities=["x"], centrality={"x": {"total_degree": 75}},
                    graph=_graph(methods=[_node("m", "m.py", 1)]), vector=[_hit(0.75, "x", "x.py", 1), _hit(0.5, "x", "x.py", 1, n=0, summary="late")]))
    degs = {}
    for s in scs:
        degs.update({key: v["total_degree"] for key, v in (s["centrality"] or {}).items()})
    b = Batch(scs, degree_of=lambda p: degs.get(p.get("graph_node_id") or p.get("entity_name") or "", -1))
    for q, s in enumerate(scs):
        assert_same(b.results(q), host_rank(s, degrees=degs), s["name"])
    five = b.results(0)[0]
    assert five.source == "hybrid" and set(five.signal_scores) == set(SIGNALS) and five.summary == "S" and five.content == "x" * 150
    assert (five.docstring, five.signature) == ("D", "def shared()")
    depths = {r.entity_name: r.signal_scores["graph_match"] for r in b.results(2)}
    assert depths["c0"] == depths["c1"] == depths["c_none"] == 1.0 and depths["c5"] == depths["c9"] == 0.3 and depths["e4"] == 1.0 - 3 * 0.2
    assert b.results(3)[0].source == "hybrid" and "vector_similarity" not in b.results(3)[0].signal_scores


def test_centrality_table_is_cut_at_the_limit(gpu):
    """More distinct keys among the primaries and the first hits than centrality_limit: the later ones answer no lookup."""
    import coderag_amd  # noqa: F401
    prim = [_node(f"p{i}", f"p{i}.py", 1) for i in range(6)] + [_node("p0", "p0b.py", 1)]
    hits = [_hit(0.75 - i / 64, f"h{i}", f"h{i}.py", 1) for i in range(6)]
    s = dict(name="cut", intent="locate_entity", entities=[], graph=_graph(primary_entities=prim, callers=[_node("h4", "z.py", 9, 2), _node("p1", "y.py", 9, 1)]),
             vector=hits, centrality=None)
    degs = {f"p{i}": 10 + i for i in range(6)} | {f"h{i}": 20 + i for i in range(6)}
    for ptop, ctop, limit in [(5, 5, 10), (5, 5, 7), (7, 6, 4), (7, 6, 0), (0, 6, 3), (7, 0, 12)]:
        b = Batch([s], degree_of=lambda p: degs.get(p.get("graph_node_id") or p["entity_name"], -1), primary_top=ptop, centrality_top=ctop,
                  centrality_limit=limit)
        want = host_rank(s, ptop, ctop, limit, degrees=degs)
        assert_same(b.results(0), want, (ptop, ctop, limit))
    cut = [r.signal_scores["centrality"] > 0 for r in host_rank(s, 5, 5, 7, degrees=degs)]
    assert 0 < sum(cut) < len(cut) and not any(r.signal_scores["centrality"] > 0 for r in host_rank(s, 7, 6, 0, degrees=degs))


def test_what_the_device_refuses_or_declines(gpu):
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from coderag_amd.ranking.device import GraphTable
    # 513 candidates: CRH_E_INVALID, whichever way they are split
    s = _sized(1, 3, 3)
    b = Batch([s])
    dev = torch.device("cuda:0")
    for G, k in [(513, 0), (0, 513), (500, 13), (1, 512)]:
        gt = GraphTable(*(torch.full((1, G), -1, dtype=d, device=dev) for d in (torch.int32, torch.int64, torch.int32, torch.int32))) if G else None
        rows = torch.full((1, k), -1, dtype=torch.int64, device=dev) if k else None
        scores = torch.zeros((1, k), dtype=torch.float32, device=dev) if k else None
        with pytest.raises(ffi.NativeError) as e:
            b.rr.rank(gt, b.side.gather(gt.row) if G else None, torch.zeros((G,), dtype=torch.int32, device=dev) if G else None, scores, rows,
                      b.side.gather(rows) if k else None, b.plans)
        assert e.value.code == ffi.E_INVALID
    with pytest.raises(ffi.NativeError):
        b.rr.rank(None, None, None, None, None, None, b.plans)                      # no candidate table at all
    # an over-long name on either side and nine entities: count -1; the neighbours in the batch are ranked
    long_g = dict(name="long_graph", intent="find_callers", entities=[], centrality=None, graph=_graph(callers=[_node("n" * 80, "a.py", 1, 1)]),
                  vector=[_hit(0.5, "ok", "b.py", 1)])
    long_v = dict(name="long_hit", intent="find_callers", entities=[], centrality=None, graph=_graph(callers=[_node("ok", "a.py", 1, 1)]),
                  vector=[_hit(0.5, "n" * 65, "b.py", 1)])
    nine = dict(name="nine", intent="find_callers", entities=[f"e{i}" for i in range(9)], centrality=None, graph=_graph(callers=[_node("ok", "a.py", 1, 1)]),
                vector=[_hit(0.5, "ok2", "b.py", 1)])
    fine = dict(name="fine", intent="find_callers", entities=["n" * 48], centrality=None, graph=_graph(callers=[_node("n" * 64, "a.py", 1, 1)]),
                vector=[_hit(0.5, "n" * 48, "b.py", 1)])
    b = Batch([long_g, fine, long_v, nine])
    assert list(b.out.count) == [-1, 2, -1, -1]
    assert_same(b.results(1), host_rank(fine), "fine")


# ---- 3. crh_graph_node_rows / crh_graph_candidates against numpy, word for word
def np_node_rows(shards, n_nodes):
    out = np.full((n_nodes,), -1, np.int64)
    for base, row_node, alive in shards:
        for r, v in enumerate(row_node):
            if alive[r] and 0 <= v < n_nodes and (out[v] < 0 or base + r < out[v]):
                out[v] = base + r
    return out


def alive_words(alive):
    bits = np.zeros(((len(alive) + 31) // 32 * 32,), np.uint8)
    bits[: len(alive)] = alive
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1).view(np.int32)


@pytest.mark.parametrize("n_rows", [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000])
def test_node_rows_match_numpy(gpu, n_rows):
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd.ranking.device import graph_node_rows
    rng = np.random.default_rng(n_rows)
    n_nodes = 40
    dev = torch.device("cuda:0")
    shards, base = [], 0
    for sh in range(2):
        # nodes 0..9 never occur, 10..19 at most once per shard, the rest many times; -1 and out-of-range entries are no nodes
        pool = np.concatenate([rng.permutation(np.arange(10, 20))[: max(1, n_rows // 8)], rng.integers(20, n_nodes, n_rows), [-1, -1, n_nodes, n_nodes + 5]])
        row_node = rng.permutation(pool)[:n_rows].astype(np.int32)
        alive = rng.random(n_rows) < 0.7
        for v in range(20, 30):                                  # tombstoned FIRST rows: the representative is a later one
            first = np.flatnonzero(row_node == v)
            if first.size:
                alive[first[0]] = False
        shards.append((base, row_node, alive))
        base += n_rows
    out = None
    for b, row_node, alive in shards:
        out = graph_node_rows(torch.from_numpy(row_node).to(dev), n_nodes, torch.from_numpy(alive_words(alive)).to(dev), row_base=b, out=out)
    assert np.array_equal(out.cpu().numpy(), np_node_rows(shards, n_nodes))
    one = graph_node_rows(torch.from_numpy(shards[0][1]).to(dev), n_nodes)          # no alive words: every row counts
    assert np.array_equal(one.cpu().numpy(), np_node_rows([(0, shards[0][1], np.ones(n_rows, bool))], n_nodes))
    assert (one.cpu().numpy()[:10] == -1).all()


def np_candidates(segs, nq, G, list_nodes, list_depth, node_rows):
    out = [np.full((nq, G), -1, np.int64) for _ in range(4)]
    fill = [0] * nq
    for q, role, node, list_row, take in segs:
        entries = [(node, 0)] if node >= 0 else list(zip(list_nodes[list_row][:take], list_depth[list_row][:take]))
        for v, d in entries:
            if v < 0 or v >= len(node_rows) or node_rows[v] < 0:
                continue
            if fill[q] < G:
                for arr, val in zip(out, (v, node_rows[v], role, d)):
                    arr[q, fill[q]] = val
            fill[q] += 1
    return out


def test_candidates_match_numpy(gpu):
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from coderag_amd.ranking.device import graph_candidates, segment_table
    rng = np.random.default_rng(5)
    dev = torch.device("cuda:0")
    n_nodes, n_lists, limit, nq = 300, 12, 150, 7
    node_rows = rng.integers(0, 5000, n_nodes).astype(np.int64)
    node_rows[rng.random(n_nodes) < 0.25] = -1                                        # nodes without a representative row
    list_nodes = rng.integers(0, n_nodes, (n_lists, limit)).astype(np.int32)
    list_depth = rng.integers(1, 6, (n_lists, limit)).astype(np.int32)
    list_nodes[rng.random((n_lists, limit)) < 0.2] = -1                               # holes
    list_nodes[3, 40:] = -1                                                            # a short list
    list_nodes[4, :] = -1                                                              # an empty one
    per_query = [
        [(0, 5, -1, 0), (0, 6, -1, 0), (1, -1, 0, 50), (1, -1, 1, 50), (2, -1, 2, 50)],
        [],                                                                             # a query without graph results
        [(2, -1, 3, 150), (1, -1, 4, 10), (0, 7, -1, 0), (3, -1, 5, 0), (4, -1, 6, 1), (5, -1, 7, 64)],   # roles out of order, take 0
        [(1, -1, 8, 1000)],                                                             # take beyond the list: the list's limit
        [(0, int(v), -1, 0) for v in np.flatnonzero(node_rows < 0)[:3]],                 # primaries without a row: nothing left
        [(1, -1, 9, 65), (1, -1, 10, 63), (2, -1, 11, 129)],
        [(0, 299, -1, 0), (5, -1, 0, 3)],
    ]
    segs, G = segment_table(per_query)
    assert G == 1000 and [s[:2] for s in segs if s[0] == 2] == [(2, 0), (2, 1), (2, 2), (2, 3), (2, 4), (2, 5)]
    up = lambda a: torch.from_numpy(a).to(dev)
    for G in (300, 64, 1):                                                             # roomy, cutting, a single slot
        t = graph_candidates(segs, nq, G, up(node_rows), up(list_nodes), up(list_depth))
        want = np_candidates(segs, nq, G, list_nodes, list_depth, node_rows)
        for got, w in zip((t.node, t.row, t.role, t.depth), want):
            assert np.array_equal(got.cpu().numpy().astype(np.int64), w)
    assert (want[0][1] == -1).all() and (want[0][4] == -1).all()
    # offsets are checked on the host: nothing is launched with an index outside its arrays
    for bad in ([(0, 0, n_nodes, -1, 0)], [(0, 1, -1, n_lists, 5)], [(0, 1, -1, -1, 5)], [(0, 6, -1, 0, 5)], [(0, 1, -1, 0, -1)], [(nq, 0, 1, -1, 0)],
                [(1, 0, 1, -1, 0), (0, 0, 1, -1, 0)]):
        with pytest.raises(ffi.NativeError) as e:
            graph_candidates(bad, nq, 8, up(node_rows), up(list_nodes), up(list_depth))
        assert e.value.code == ffi.E_INVALID


def test_more_centrality_keys_than_the_table_holds(gpu):
    """More than CRH_RR_HYBRID_TABLE (128) distinct keys under a limit that admits them: count -1; a limit of 128 is served."""
    import coderag_amd  # noqa: F401
    prim = [_node(f"p{i}", f"p{i}.py", 1) for i in range(130)]
    s = dict(name="overflow", intent="locate_entity", entities=["p129"], graph=_graph(primary_entities=prim), vector=[_hit(0.5, "h0", "h.py", 1)],
             centrality=None)
    degs = {f"p{i}": i for i in range(130)}
    deg = lambda p: degs.get(p.get("graph_node_id") or p["entity_name"], -1)
    assert Batch([s], degree_of=deg, primary_top=200, centrality_top=5, centrality_limit=200).out.count[0] == -1
    b = Batch([s], degree_of=deg, primary_top=200, centrality_top=5, centrality_limit=128)
    assert b.out.count[0] >= 0
    assert_same(b.results(0), host_rank(s, 200, 5, 128, degrees=degs), "limit 128")
