"""Personalised PageRank on the device: ``crh_graph_ppr`` / ``_ppr_bins`` / ``_ppr_order`` against the restatement of
tests/ppr_cases.py -- scores, bins, top lists and orderings must be equal BIT FOR BIT -- and the store's ``search_propagated`` and
``graph_rank`` against the f32 oracle plus the restatement.  Workspaces and outputs are pre-filled with garbage.  No tolerance
appears anywhere."""
import asyncio
import functools

import numpy as np
import pytest

from tests import graph_cases as gc
from tests import ppr_cases as pc

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32


def _env():
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi, graph
    return ffi, graph


def _graph(n, edges):
    ffi, graph = _env()
    g = ffi.Graph(n, device=0)
    g.set_relation(0, *graph.build_csr(np.asarray(edges, np.int64).reshape(-1, 2), n))
    return g


def _garbage(g, nq):
    import torch
    qs = 1
    while qs < nq:
        qs *= 2
    g._ppr_workspace(qs).view(torch.int32).fill_(-77)                              # (a NaN pattern in every word)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def _ppr(g, fwd, rev, direction, seeds, weights=None, restart=0.15, steps=16, device_list=False):
    """One crh_graph_ppr into a garbage-filled workspace, compared bit for bit with the restatement; returns the scores."""
    import torch
    nq = len(seeds)
    _garbage(g, nq)
    if device_list:
        s = torch.from_numpy(np.asarray(seeds, np.int32)).to("cuda:0")
        w = None if weights is None else torch.from_numpy(np.asarray(weights, F32)).to("cuda:0")
        got = g.ppr(0, direction, s, w, restart, steps)
    else:
        got = g.ppr(0, direction, seeds, weights, restart, steps)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want = pc.ppr(fwd, rev, direction, seeds, weights, restart, steps, device_list)
    assert got.shape == want.shape == (len(fwd), nq)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, (direction, nq, steps, bad[:6].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    full = g._ppr_state("test")[1].cpu().numpy().reshape(len(fwd), -1)
    assert not full[:, nq:].any()                                                  # the columns behind nq are +0
    return want


def _top(g, scores, k, exclude=None):
    import torch
    ex = None if exclude is None else torch.from_numpy(np.asarray(exclude, np.int32)).to("cuda:0")
    nodes, vals = g.ppr_top(k, exclude=ex)
    torch.cuda.synchronize()
    want_n, want_v = pc.top_list(scores, k, exclude)
    assert np.array_equal(nodes.cpu().numpy(), want_n) and np.array_equal(_bits(vals.cpu().numpy()), _bits(want_v))
    return want_n


def _seeds(n, nq, seed, c=4):
    """nq lists of c entries: random nodes and weights, a repeated node, -1 padding, a zero weight, and (with several
    queries) an all-zero query beside the live ones."""
    rng = np.random.default_rng(seed)
    nodes = rng.integers(0, n, size=(nq, c)).tolist()
    weights = (rng.random((nq, c)).astype(F32) + F32(0.125)).tolist()
    for q in range(nq):
        if c > 1 and q % 3 == 0:
            nodes[q][c - 1] = nodes[q][0]
        if c > 2 and q % 4 == 1:
            nodes[q][1] = -1
        if c > 2 and q % 4 == 2:
            weights[q][2] = 0.0
    if nq > 1:
        weights[nq // 2] = [0.0] * c
    return nodes, weights


# ---------------------------------------------------------------------------------------------------- node and query counts
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 1000])
def test_node_counts_with_isolated_nodes(gpu, n):
    _, edges = gc.random_graph(n, n, mean_degree=1, hubs=1 if n > 8 else 0, hub_degree=9)
    fwd, rev = pc.graph_lists(n, edges)
    assert n < 63 or len({v for e in edges for v in e}) < n                        # (isolated nodes are there)
    g = _graph(n, edges)
    try:
        for i, direction in enumerate(gc.DIRECTIONS):
            for nq in (1, 5, 64):
                nodes, weights = _seeds(n, nq, n + i)
                scores = _ppr(g, fwd, rev, direction, nodes, weights, steps=6)
                assert n < 63 or scores.any()
                _top(g, scores, 7)
    finally:
        g.close()


@pytest.mark.parametrize("nq", [1, 2, 3, 5, 16, 17, 33, 64])
def test_query_counts_on_every_state_width(gpu, nq):
    n, edges = gc.random_graph(129, 3, mean_degree=2, hubs=2, hub_degree=70)
    fwd, rev = pc.graph_lists(n, edges)
    g = _graph(n, edges)
    try:
        nodes, weights = _seeds(n, nq, nq)
        scores = _ppr(g, fwd, rev, "both", nodes, weights, steps=5)
        _top(g, scores, 9, exclude=[row[:2] for row in nodes])
        scores = _ppr(g, fwd, rev, "callees", nodes, None, steps=3)                # weights NULL: all 1
        assert scores[:, 0].any()
        again = _ppr(g, fwd, rev, "callees", np.asarray(nodes, np.int32).tolist(), None, steps=3, device_list=True)
        assert np.array_equal(_bits(scores), _bits(again))                         # the same list from the device
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------- degrees and shapes
@pytest.mark.parametrize("degree", [0, 1, 63, 64, 65, 300])
def test_star_degrees_in_every_direction(gpu, degree):
    n, edges = gc.star(degree)
    fwd, rev = pc.graph_lists(n, edges)
    g = _graph(n, edges)
    try:
        for direction in gc.DIRECTIONS:
            for nq in (1, 64):                                                      # one lane per node; one wave per node
                seeds = [[(q * 7) % n, 0, degree + 1] for q in range(nq)]
                weights = [[1.0, 0.5 + q, 2.0] for q in range(nq)]
                scores = _ppr(g, fwd, rev, direction, seeds, weights, steps=4)
                assert scores.any()
    finally:
        g.close()


def test_cycle_diamond_and_an_asymmetric_pair(gpu):
    for n, edges in (gc.cycle(7), gc.diamond(), gc.asymmetric(), (2, [(0, 1)]), (3, [(0, 1), (1, 0), (1, 2)])):
        fwd, rev = pc.graph_lists(n, edges)
        g = _graph(n, edges)
        try:
            for direction in gc.DIRECTIONS:
                scores = _ppr(g, fwd, rev, direction, [[0], [n - 1], [0, n - 1]], [[1.0], [1.0], [1.0, 3.0]], steps=9)
                assert scores[0, 0] > 0
            if n == 2:                                                             # BOTH on one edge: each end pulls the other ONCE
                r = F32(0.15)
                a = F32(F32(1.0) - r)
                one = pc.ppr(fwd, rev, "both", [[0]], None, 0.15, 1)
                assert one[:, 0].tolist() == [r, a]
        finally:
            g.close()


# ---------------------------------------------------------------------------------------------------- seeds and steps
def test_seed_lists(gpu):
    n, edges = gc.random_graph(200, 8, mean_degree=2, hubs=1, hub_degree=80)
    fwd, rev = pc.graph_lists(n, edges)
    g = _graph(n, edges)
    rng = np.random.default_rng(5)
    try:
        # c = 1; duplicates of one node at positions 0 and c - 1; c = 1024 with many repeats, -1 and zero weights
        _ppr(g, fwd, rev, "both", [[17], [3]], [[0.25], [4.0]], steps=2)
        _ppr(g, fwd, rev, "both", [[5, 9, 11, 5]], [[0.1, 0.2, 0.3, 0.7]], steps=2)
        big = rng.integers(-1, n, size=(3, 1024)).tolist()
        wts = rng.random((3, 1024)).astype(F32)
        wts[rng.random((3, 1024)) < 0.2] = 0.0
        big[1][0] = big[1][1023] = 77
        scores = _ppr(g, fwd, rev, "callers", big, wts.tolist(), steps=2)
        assert scores.any(axis=0).all()
        _ppr(g, fwd, rev, "callers", big, wts.tolist(), steps=2, device_list=True)
        # an all-zero query and an all-padding query beside live ones
        scores = _ppr(g, fwd, rev, "both", [[1, 2], [3, 4], [-1, -1], [5, 6]], [[1.0, 1.0], [0.0, 0.0], [1.0, 1.0], [2.0, 1.0]], steps=3)
        assert not scores[:, 1].any() and not scores[:, 2].any() and scores[:, 0].any() and scores[:, 3].any()
        # a device list is clamped: a negative, a NaN and an infinite weight count as +0, an entry that is no node is padding
        dev_nodes = [[1, 2, 3, 4, n, -5], [7, 7, 7, 7, 7, 7]]
        dev_w = [[-1.0, float("nan"), 2.0, float("inf"), 1.0, 1.0], [1.0, -2.0, float("nan"), 0.5, -0.0, 0.25]]
        scores = _ppr(g, fwd, rev, "both", dev_nodes, dev_w, steps=1, device_list=True)
        only3 = pc.ppr(fwd, rev, "both", [[3]], None, 0.15, 1)
        assert np.array_equal(_bits(scores[:, 0]), _bits(only3[:, 0]))
    finally:
        g.close()


@pytest.mark.parametrize("steps", [1, 64])
def test_steps_at_both_ends(gpu, steps):
    n, edges = gc.random_graph(150, 2, mean_degree=2, hubs=1, hub_degree=66)
    fwd, rev = pc.graph_lists(n, edges)
    g = _graph(n, edges)
    try:
        for nq in (3, 64):
            nodes, weights = _seeds(n, nq, steps + nq)
            _ppr(g, fwd, rev, "both", nodes, weights, restart=0.5 if nq == 3 else 0.15, steps=steps)
    finally:
        g.close()


def test_subnormal_ladder(gpu):
    """16 rungs of out-degree 301: the last rung's score is about (0.85 / 301)^15 * 0.15 -- a subnormal f32 -- bit for bit."""
    n, edges = pc.ladder(16, 300)
    fwd, rev = pc.graph_lists(n, edges)
    g = _graph(n, edges)
    try:
        for nq in (1, 64):
            seeds = [[0]] * nq
            scores = _ppr(g, fwd, rev, "callees", seeds, None, steps=16)
            tiny = scores[15, 0]
            assert 0 < tiny < np.finfo(F32).tiny and scores[14, 0] > tiny           # subnormal, and kept
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------- bins, top lists, orders
def test_top_lists_ties_exclusions_and_prefixes(gpu):
    import torch
    n, edges = gc.cycle(12)                                                        # symmetric: nodes at equal distance from the seed tie
    fwd, rev = pc.graph_lists(n, edges)
    g = _graph(n, edges)
    try:
        scores = _ppr(g, fwd, rev, "both", [[0], [6], [-1]], None, steps=5)
        assert scores[1, 0] == scores[11, 0] > 0 and scores[6, 0] == 0             # 5 steps do not reach the far side
        top = _top(g, scores, 12)
        assert list(top[0]).index(1) + 1 == list(top[0]).index(11)                 # the tie goes to the lower id
        assert (top[0] >= 0).sum() == 11 and (top[2] == -1).all()                  # k above the positive nodes; an all-zero query
        for k in (1, 2, 5, 11, 40):                                                # the j-prefix property
            assert np.array_equal(_top(g, scores, k)[:, : min(k, 12)], top[:, :k] if k <= 12 else top)
        _top(g, scores, 6, exclude=[[0, 1, -1], [6, 6, 5], [3, 4, 5]])
        # the bins themselves, into a garbage-filled table
        ffi, _ = _env()
        bins = torch.full((3, n), -77, dtype=torch.int64, device="cuda:0")
        ex = torch.tensor([[1, -1], [n, 7], [0, 0]], dtype=torch.int32, device="cuda:0")
        ffi.check(ffi.lib().crh_graph_ppr_bins(n, 3, g._ppr_state("t")[1].data_ptr(), 2, ex.data_ptr(), bins.data_ptr(), 0))
        torch.cuda.synchronize()
        assert np.array_equal(bins.cpu().numpy(), pc.bins_of(scores, [[1, -1], [n, 7], [0, 0]]))
    finally:
        g.close()


@pytest.mark.parametrize("nq,c", [(1, 1), (3, 7), (17, 40), (64, 512), (2, 1024)])
def test_order_lists(gpu, nq, c):
    import torch
    n, edges = gc.cycle(16)
    fwd, rev = pc.graph_lists(n, edges)
    g = _graph(n, edges)
    rng = np.random.default_rng(nq * c)
    try:
        seeds = [[q % n] for q in range(nq)]
        if nq > 1:
            seeds[1] = [-1]                                                        # all-zero scores: list 1 is padding only
        scores = _ppr(g, fwd, rev, "both", seeds, None, steps=4)
        rows = np.stack([rng.permutation(10 * c)[:c] for _ in range(nq)]).astype(np.int64)
        cos = -np.sort(-rng.random((nq, c)).astype(F32), axis=1)
        nodes = rng.integers(-1, n, size=(nq, c)).astype(np.int32)                  # ties everywhere (16 nodes); candidates with no node
        rows[:, c - c // 4:], cos[:, c - c // 4:] = -1, -np.inf                    # padding at the end, nodes left as they are
        dev = [torch.from_numpy(x).to("cuda:0") for x in (rows, cos, nodes)]
        fs, fr, gs = g.ppr_order(*dev)
        torch.cuda.synchronize()
        want_s, want_r, want_g = pc.order_lists(scores, rows, cos, nodes)
        assert np.array_equal(fr.cpu().numpy(), want_r) and np.array_equal(_bits(fs.cpu().numpy()), _bits(want_s))
        assert np.array_equal(_bits(gs.cpu().numpy()), _bits(want_g))
        if nq > 1:
            assert (want_r[1, 1] == -1).all() and (want_r[0, 1] >= 0).any()
    finally:
        g.close()


def test_two_runs_give_equal_bits_and_random_hub_graphs(gpu):
    import torch
    for seed, n in ((1, 500), (2, 1000)):
        n, edges = gc.random_graph(n, seed)
        fwd, rev = pc.graph_lists(n, edges)
        g = _graph(n, edges)
        try:
            for direction, nq in (("both", 64), ("callees", 7), ("callers", 1)):
                nodes, weights = _seeds(n, nq, seed, c=6)
                want = _ppr(g, fwd, rev, direction, nodes, weights, steps=8)
                _garbage(g, nq)
                again = g.ppr(0, direction, nodes, weights, 0.15, 8)
                torch.cuda.synchronize()
                assert np.array_equal(_bits(again.cpu().numpy()), _bits(want))
                _top(g, want, 25, exclude=[row[:3] for row in nodes])
        finally:
            g.close()


def test_refusals_launch_nothing(gpu):
    import torch
    ffi, _ = _env()
    n, edges = gc.chain(5)
    g = _graph(n, edges)
    try:
        for kw in ({"seeds": [[5]]}, {"seeds": [[-2]]}, {"seeds": [[0]], "weights": [[-1.0]]}, {"seeds": [[0]], "weights": [[float("nan")]]},
                   {"seeds": [[0]], "weights": [[float("inf")]]}, {"seeds": [[0]], "steps": 0}, {"seeds": [[0]], "steps": 65},
                   {"seeds": [[0]], "restart": 0.0}, {"seeds": [[0]], "restart": 1.0}, {"seeds": [[0]], "restart": float("nan")},
                   {"seeds": [[0]] * 65}, {"seeds": [[0] * 1025]}, {"seeds": [[0]], "rel": 1}, {"seeds": [[0]], "direction": 3}):
            _garbage(g, 64)                                                        # (the widest state: no call below takes a new workspace)
            with pytest.raises(ffi.NativeError):
                g.ppr(kw.get("rel", 0), kw.get("direction", "both"), kw["seeds"], kw.get("weights"), kw.get("restart", 0.15), kw.get("steps", 16))
            torch.cuda.synchronize()
            assert bool((g.ppr_work.view(torch.int32) == -77).all()), kw                 # nothing was launched
        # a replaced relation: 1 / out(v) is rebuilt
        fwd, rev = pc.graph_lists(n, edges)
        _ppr(g, fwd, rev, "callees", [[0]], None, steps=3)
        _, graph = _env()
        edges2 = [(0, 1), (0, 2), (0, 3), (3, 4)]
        g.set_relation(0, *graph.build_csr(np.asarray(edges2, np.int64), n))
        fwd, rev = pc.graph_lists(n, edges2)
        _ppr(g, fwd, rev, "callees", [[0]], None, steps=3)
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------- the store, end to end
STORE_N, STORE_DIM, NODES = 700, 384, 120


def _chunks():
    """Chunk i belongs to node i % 150: nodes 120 .. 149 are no nodes of the graph; every fifth chunk carries its key as the
    entity name only."""
    pay = []
    for i in range(STORE_N):
        p = {"file_path": f"src/m{i % 9}.py", "entity_type": "function", "entity_name": f"n{i % 150}", "language": "python" if i % 3 else "go",
             "content": f"def n{i % 150}(): pass", "start_line": i, "end_line": i + 1, "project_name": "p"}
        if i % 5:
            p["graph_node_id"], p["entity_name"] = p["entity_name"], f"other{i}"
        pay.append(p)
    return pay


@functools.lru_cache(maxsize=None)
def _store_graph():
    n, edges = gc.random_graph(NODES, 5, mean_degree=1, hubs=2, hub_degree=12)
    edges = sorted({(a, b) for a, b in edges if a != b}, key=edges.index)
    seen, order = set(), []
    for a, b in edges:                                                           # node ids by first appearance, as the store numbers them
        for v in (a, b):
            if v not in seen:
                seen.add(v)
                order.append(v)
    number = {v: i for i, v in enumerate(order)}
    names = [f"n{v}" for v in order]
    return edges, names, pc.graph_lists(len(names), [(number[a], number[b]) for a, b in edges])


@pytest.mark.parametrize("shards", [1, 2])
def test_store_end_to_end(gpu, shards):
    _env()
    from coderag_amd.shards import STRIDE
    from coderag_amd.store import HipVectorStore
    from oracle import search as orc
    pay = _chunks()
    rng = np.random.default_rng(31)
    raw = rng.standard_normal((STORE_N, STORE_DIM)).astype(F32)
    ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(STORE_N)]
    q = rng.standard_normal((66, STORE_DIM)).astype(F32)
    edges, names, (fwd, rev) = _store_graph()
    key = [p.get("graph_node_id") or p["entity_name"] for p in pay]
    node_of = np.asarray([names.index(k) if k in names else -1 for k in key])
    alive = np.ones(STORE_N, bool)
    x_pre, q_pre = orc.preprocess(raw, to_bf16=True), orc.preprocess(q, to_bf16=True)
    bits = lambda x: int(F32(x).view(U32))                                         # noqa: E731

    async def run():
        async with HipVectorStore(dim=STORE_DIM, dtype="bf16", initial_capacity=1024, device=0, shards=shards, compact_dead_fraction=0.0) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, raw, pay)
            col = s._col("code_chunks")
            await s.set_graph_edges("code_chunks", [(f"n{a}", f"n{b}") for a, b in edges])
            hub = max(range(len(names)), key=lambda v: len(fwd[v]) + len(rev[v]))
            for i in range(STORE_N):                                             # tombstones, never compacted away: every 13th chunk, and
                if i % 13 == 0 or node_of[i] == hub:                             # EVERY chunk of the hub -- a node without an alive row
                    await s.delete("code_chunks", {"start_line": i})
                    alive[i] = False
            shard, local = col.rows_of(np.arange(STORE_N))
            grow = shard.astype(np.int64) * STRIDE + local
            slot_of_row = {int(g): i for i, g in enumerate(grow)}

            def want(limit, candidates, related_limit, mask, **prop):
                cs, cr = orc.search(x_pre, q_pre, candidates, alive=(alive & mask).astype(np.uint8))
                cand_nodes = np.where(cr >= 0, node_of[np.maximum(cr, 0)], -1)     # tombstones leave the row -> node column untouched
                cand_rows = np.where(cr >= 0, grow[np.maximum(cr, 0)], -1)
                out = []
                for hits, related in pc.propagated(fwd, rev, cs, cand_rows, cand_nodes, limit, related_limit, **prop):
                    rel = []
                    for v, sc in related:
                        owners = sorted(int(grow[i]) for i in range(STORE_N) if alive[i] and node_of[i] == v)
                        rel.append((names[v], bits(sc), ids[slot_of_row[owners[0]]] if owners else None))   # no alive row: no payload
                    out.append(([(ids[slot_of_row[row]], bits(f), bits(c), bits(gsc)) for row, f, c, gsc in hits], rel))
                return out

            def shown(res):
                by_line = {p["start_line"]: i for i, p in zip(ids, pay)}
                return [([(h["id"], bits(h["score"]), bits(h["cosine"]), bits(h["graph_score"])) for h in one["hits"]],
                         [(r["node"], bits(r["graph_score"]), None if r["payload"] is None else by_line[r["payload"]["start_line"]]) for r in one["related"]])
                        for one in res]

            python = np.asarray([p["language"] == "python" for p in pay])
            got = await s.search_propagated_batch("code_chunks", q, limit=6, related_limit=8, filters={"language": "python"})
            assert col.graph_ppr_calls == 2                                        # 66 queries: two passes
            exp = want(6, 24, 8, python)
            assert shown(got) == exp
            assert any(h["graph_score"] > 0 for o in got for h in o["hits"]) and any(o["related"] for o in got)
            assert any(r[0] == names[hub] and r[2] is None for _, rel in exp for r in rel)         # ranked, and without a payload
            prop = {"direction": "callees", "restart": 0.25, "steps": 5, "seed_weight": "uniform", "rrf_k": 3}
            got = await s.search_propagated_batch("code_chunks", q[:5], limit=10, candidates=33, propagate=prop, related_limit=3)
            assert shown(got) == want(10, 33, 3, np.ones(STORE_N, bool), **prop)[:5]
            one = await s.search_propagated("code_chunks", q[3].tolist(), limit=6, related_limit=8, filters={"language": "python"})
            assert shown([one]) == exp[3:4]

            # graph_rank through the batch wrapper: 65 sets, two passes
            sets = [[names[i % len(names)], names[(3 * i + 1) % len(names)]] for i in range(65)]
            weights = [[1.0, 0.5 + i % 3] for i in range(65)]
            ranked = await s.graph_rank_batch("code_chunks", sets, weights, direction="both", limit=9)
            scores = pc.ppr(fwd, rev, "both", [[names.index(a), names.index(b)] for a, b in sets], weights, 0.15, 16)
            top_n, top_v = pc.top_list(scores, 9)
            for i, res in enumerate(ranked):
                assert [(h["node"], bits(h["graph_score"])) for h in res["hits"]] == [(names[v], bits(x)) for v, x in zip(top_n[i], top_v[i]) if v >= 0]
                for h in res["hits"]:
                    owners = sorted(int(grow[j]) for j in range(STORE_N) if alive[j] and key[j] == h["node"])
                    assert (h["payload"] is None) == (not owners) and (not owners or h["payload"]["start_line"] == slot_of_row[owners[0]])
    asyncio.run(run())
