"""The call graph on the device: ``crh_graph_*`` against the deque BFS of tests/graph_cases.py -- level words, seen words, active
words, lists, counts, row bitmaps and paths must be equal exactly -- and the graph filter of the store against the f32 oracle
under the restatement's mask (ids and score BITS).  The workspace and the output buffers are pre-filled with garbage.  No
tolerance appears anywhere."""
import asyncio

import numpy as np
import pytest

from tests import graph_cases as gc

pytestmark = pytest.mark.gpu

U64, U32 = np.uint64, np.uint32


def _env():
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi, graph
    return ffi, graph


def _graph(n, edges):
    ffi, graph = _env()
    g = ffi.Graph(n, device=0)
    g.set_relation(0, *graph.build_csr(np.asarray(edges, np.int64).reshape(-1, 2), n))
    assert g.count(0) == (n, len({(a, b) for a, b in edges if a != b})) and g.count(1) == (n, -1)
    return g


def _bfs(g, n, edges, direction, sets, hops, include_self=False, device_sources=None):
    """One crh_graph_bfs into a garbage-filled workspace, compared word for word with the restatement; returns its depth maps."""
    import torch
    g._workspace(hops)
    for t in (g.levels, g.seen, g.active):
        t.fill_(-77)
    sources = sets if device_sources is None else torch.from_numpy(np.asarray(device_sources, np.int32)).to("cuda:0")
    levels, seen, active = g.bfs(0, direction, sources, hops, include_self=include_self)
    torch.cuda.synchronize()
    want_l, want_s, want_a, maps = gc.bfs_words(n, edges, direction, sets, hops, include_self)
    got_l = levels.cpu().numpy().view(U64)
    assert got_l.shape == want_l.shape and np.array_equal(got_l, want_l), (direction, hops, np.argwhere(got_l != want_l)[:8])
    assert np.array_equal(seen.cpu().numpy().view(U64), want_s)
    assert np.array_equal(active.cpu().numpy().view(U64), want_a)
    return maps


def _list(g, maps, first_level, limit):
    import torch
    nodes, depth, count = g.list(limit, first_level=first_level)
    torch.cuda.synchronize()
    wn, wd, wc = gc.listing(maps, first_level, limit)
    assert np.array_equal(nodes.cpu().numpy(), wn) and np.array_equal(depth.cpu().numpy(), wd) and np.array_equal(count.cpu().numpy(), wc)
    return wc


def _whole(n, edges, direction, sets, hops, include_self=False, limits=(5,)):
    g = _graph(n, edges)
    try:
        maps = _bfs(g, n, edges, direction, sets, hops, include_self)
        for limit in limits:
            _list(g, maps, 1, limit)
        _list(g, maps, 0, max(limits))
        return maps
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------- node counts and degrees
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 1000])
def test_node_counts_with_isolated_nodes(gpu, n):
    _, edges = gc.random_graph(n, n, mean_degree=1, hubs=1 if n > 8 else 0, hub_degree=9)
    for i, direction in enumerate(gc.DIRECTIONS):
        sets = gc.random_sets(n, 5, n + i) + [[n - 1], [0]]
        maps = _whole(n, edges, direction, sets, 3, include_self=bool(i % 2), limits=(1, 7))
        if n >= 63:
            assert any(len(m) > 1 for m in maps)
    touched = {v for e in edges for v in e}
    assert n < 63 or len(touched) < n                                          # (isolated nodes are there)


@pytest.mark.parametrize("degree", [0, 1, 63, 64, 65, 300])
def test_degrees_on_both_sides_of_the_wave_boundary(gpu, degree):
    """star(): travelling along the edges the sink PULLS through a reverse list of ``degree`` entries, against them the hub
    through a forward list of as many -- a lane's walk below CRH_GRAPH_WAVE_DEGREE, the wave's from it on."""
    ffi, _ = _env()
    assert ffi.GRAPH_WAVE_DEGREE == gc.WAVE_DEGREE == 64
    n, edges = gc.star(degree)
    sink = degree + 1
    for direction, sources in (("callees", [0]), ("callers", [sink]), ("both", [n - 1]), ("callees", [1 if degree else 0])):
        maps = _whole(n, edges, direction, [sources, [0, sink], list(range(1, 1 + min(degree, 3)))], 4, limits=(2, n))
        if degree and sources in ([0], [sink]):
            assert maps[0][sink if direction == "callees" else 0] == 2            # through every one of the middle nodes at once


@pytest.mark.parametrize("hops", [1, 2, 16])
def test_chain_ends_at_max_hops(gpu, hops):
    n, edges = gc.chain(hops + 2)
    maps = _whole(n, edges, "callees", [[0]], hops, limits=(1, hops, hops + 3))
    assert maps[0][hops] == hops and hops + 1 not in maps[0]                    # depth H is in, depth H + 1 is out
    maps = _whole(n, edges, "callers", [[n - 1], [0]], hops)
    assert maps[0][1] == hops and 0 not in maps[0] and maps[1] == {0: 0}


def test_cycle_diamond_and_directions(gpu):
    n, edges = gc.cycle(6)
    for include_self in (False, True):
        maps = _whole(n, edges, "callees", [[2]], 16, include_self=include_self, limits=(6,))
        assert maps[0] == {2: 0, 3: 1, 4: 2, 5: 3, 0: 4, 1: 5}                  # the source is not met again at depth 6
    n, edges = gc.diamond()
    maps = _whole(n, edges, "callees", [[0]], 8, limits=(3, 6, 9))
    assert maps[0][5] == 2 and maps[0][4] == 3 and maps[0][6] == 3              # minimum depths, not the long way round
    n, edges = gc.asymmetric()
    answers = [_whole(n, edges, d, [[2]], 2, limits=(8,))[0] for d in gc.DIRECTIONS]
    assert answers[0] == {2: 0, 3: 1, 6: 1, 4: 2, 7: 2} and answers[1] == {2: 0, 1: 1, 5: 1, 0: 2}
    assert answers[2] == {2: 0, 1: 1, 3: 1, 5: 1, 6: 1, 0: 2, 4: 2, 7: 2}


# ---------------------------------------------------------------------------------------------------- batches and hops
@pytest.mark.parametrize("nq", [1, 2, 63, 64])
def test_batch_sizes(gpu, nq):
    n, edges = gc.random_graph(200, 7)
    for direction in gc.DIRECTIONS:
        _whole(n, edges, direction, gc.random_sets(n, nq, nq), 3, limits=(4,))


def test_source_set_shapes(gpu):
    n, edges = gc.random_graph(150, 9, mean_degree=2)
    lit = [[] for _ in range(64)]
    for q, v in ((0, 3), (31, 77), (32, 78), (63, 149)):                         # bits 0, 31, 32 and 63 alone
        lit[q] = [v]
    maps = _whole(n, edges, "both", lit, 2)
    assert [q for q, m in enumerate(maps) if m] == [0, 31, 32, 63]
    sets = [[], [5], list(range(n)), [5, 6, 7], [6, 7, 8], [9, 9, 9]]          # empty, one node, every node, overlapping, repeated
    maps = _whole(n, edges, "callees", sets, 4, limits=(3, n))
    assert maps[0] == {} and len(maps[2]) == n and set(maps[2].values()) == {0}
    # the device-source form: a [nq, k] table with -1 padding (and a row of nothing else)
    table = np.full((5, 4), -1, np.int32)
    table[0, :3], table[1, 1], table[3], table[4, ::2] = [5, 6, 7], 5, [9, 9, 9, 9], [0, n - 1]
    host_sets = [[5, 6, 7], [5], [], [9], [0, n - 1]]
    g = _graph(n, edges)
    try:
        for direction in gc.DIRECTIONS:
            maps = _bfs(g, n, edges, direction, host_sets, 3, device_sources=table)
            _list(g, maps, 1, 6)
    finally:
        g.close()


def test_a_dead_frontier_leaves_the_later_levels_zero(gpu):
    import torch
    n, edges = 40, [(0, 1), (1, 2), (0, 3), (10, 11)]
    g = _graph(n, edges)
    try:
        _bfs(g, n, edges, "callees", [[0], [10], [5]], 16)
        levels, active = g.levels.cpu().numpy().view(U64), g.active.cpu().numpy().view(U64)
        assert levels[2, 2] == 1 and not levels[3:].any() and active[:3].tolist() == [7, 3, 1] and not active[3:].any()
        for hops in (1, 2):
            _bfs(g, n, edges, "callees", [[0], [10], [5]], hops)
        torch.cuda.synchronize()
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------- lists
def test_list_cuts_and_counts(gpu):
    n = 1030                                                                     # more than one step of the list kernel's 1024 nodes
    edges = [(0, v) for v in range(1, n, 3)] + [(v, v + 1) for v in range(1, n - 1, 3)] + [(5, n - 1), (n - 1, 0)]
    g = _graph(n, edges)
    try:
        maps = _bfs(g, n, edges, "callees", [[0], [n - 1], [4], []], 3)
        assert 0 in maps[1] and n - 1 in maps[1] and maps[1][0] == 1             # node 0 and node N - 1 both reached
        level1 = sum(1 for d in maps[0].values() if d == 1)
        total = len(maps[0]) - 1
        assert level1 > 300 and total > level1
        for limit in (1, level1 - 5, level1, level1 + 5, total, total + 9, 0):   # a cut inside a level, at its end, at the count, beyond it
            counts = _list(g, maps, 1, limit)
            assert counts.tolist() == [total, len(maps[1]) - 1, len(maps[2]) - 1, 0]     # never clipped at the limit
        _list(g, maps, 0, 7)
        _list(g, maps, 3, 2000)
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------- row bitmaps
@pytest.mark.parametrize("rows", [1, 31, 32, 33, 700])
def test_row_words(gpu, rows):
    import torch
    n, edges = gc.random_graph(90, 4, mean_degree=2, hubs=1, hub_degree=20)
    rng = np.random.default_rng(rows)
    row_node = rng.integers(0, 60, size=rows).astype(np.int32)                   # several rows per node; nodes 60.. have no row
    row_node[rng.random(rows) < 0.2] = -1                                        # rows whose key is no node
    row_node[-1] = 59
    g = _graph(n, edges)
    try:
        sets = [[int(v)] for v in rng.integers(0, n, size=40)] + [list(range(n)), []]
        maps = _bfs(g, n, edges, "both", sets, 2, include_self=True)
        col = torch.from_numpy(row_node).to("cuda:0")
        for q in (0, 7, 39, 40, 41):
            for extra in (0, 3):
                words = (rows + 31) // 32 + extra
                out = torch.full((words + 2,), -77, dtype=torch.int32, device="cuda:0")
                got = g.row_words(col, q, n_words=words, out=out).cpu().numpy().view(U32)
                want = gc.row_words(row_node, set(maps[q]), words)
                assert np.array_equal(got[:words], want) and (got[words:] == U32(-77 & 0xffffffff)).all()     # tail bits and spare words are 0, nothing beyond is touched
        assert gc.mask_from_words(gc.row_words(row_node, set(maps[40]), None), rows).sum() == int((row_node >= 0).sum())
        maps = _bfs(g, n, edges, "both", sets, 2, include_self=False)             # the sources' own rows leave with their bits
        got = g.row_words(col, 0).cpu().numpy().view(U32)
        assert np.array_equal(got, gc.row_words(row_node, {v for v, d in maps[0].items() if d > 0}))
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------- paths
def test_paths(gpu):
    # two shortest paths 0 -> {2, 1} -> 3 -> 4 (the smaller predecessor wins), a longer one 0 -> 5 -> 6 -> 7 -> 4, 8 unreachable
    n, edges = 9, [(0, 2), (0, 1), (2, 3), (1, 3), (3, 4), (0, 5), (5, 6), (6, 7), (7, 4)]
    g = _graph(n, edges)
    try:
        for hops in (3, 8):
            _bfs(g, n, edges, "callees", [[8], [0]], hops, include_self=True)
            assert g.path(0, "callees", 1, 4).tolist() == [0, 1, 3, 4] == gc.shortest_path(n, edges, "callees", [0], 4, hops)
            assert g.path(0, "callees", 1, 8).tolist() == [] and g.path(0, "callees", 0, 4).tolist() == []      # unreachable
            assert g.path(0, "callees", 1, 0).tolist() == [0] and g.path(0, "callees", 0, 8).tolist() == [8]    # source == target
            assert g.path(0, "callees", 1, 7).tolist() == [0, 5, 6, 7]                                           # exactly 3 edges
        _bfs(g, n, edges, "callees", [[0]], 2, include_self=True)
        assert g.path(0, "callees", 0, 7).tolist() == [] and g.path(0, "callees", 0, 3).tolist() == [0, 1, 3]  # max_hops + 1 edges: none
        _bfs(g, n, edges, "callers", [[4]], 3, include_self=True)
        assert g.path(0, "callers", 0, 0).tolist() == [4, 3, 1, 0] == gc.shortest_path(n, edges, "callers", [4], 0, 3)
        _bfs(g, n, edges, "both", [[6, 2]], 4, include_self=True)
        for target in range(n):
            assert g.path(0, "both", 0, target).tolist() == gc.shortest_path(n, edges, "both", [6, 2], target, 4)
    finally:
        g.close()
    n, edges = gc.random_graph(300, 12)
    g = _graph(n, edges)
    try:
        for direction in gc.DIRECTIONS:
            _bfs(g, n, edges, direction, [[], [17, 250]], 5, include_self=True)
            for target in range(0, n, 7):
                assert g.path(0, direction, 1, target).tolist() == gc.shortest_path(n, edges, direction, [17, 250], target, 5), (direction, target)
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------- random graphs
@pytest.mark.parametrize("n", [300, 2000])
def test_random_graphs_with_hubs(gpu, n):
    _, edges = gc.random_graph(n, 100 + n)
    for i, direction in enumerate(gc.DIRECTIONS):
        for hops in ((2, 16) if n == 300 else (3,)):
            maps = _whole(n, edges, direction, gc.random_sets(n, 64, n + i), hops, include_self=bool(i % 2), limits=(10, n))
            assert max(len(m) for m in maps) > n // 2


def test_refusals(gpu):
    ffi, _ = _env()
    n, edges = gc.chain(5)
    g = _graph(n, edges)
    try:
        for call in (lambda: g.bfs(0, "callees", [[0]], 0), lambda: g.bfs(0, "callees", [[0]], 17), lambda: g.bfs(1, "callees", [[0]], 2),
                     lambda: g.bfs(0, "callees", [[5]], 2), lambda: g.bfs(0, "callees", [[0]] * 65, 2), lambda: g.bfs(0, "sideways", [[0]], 2),
                     lambda: g.set_relation(8, *_csr(n, edges)), lambda: g.set_relation(1, *_csr(n, [(0, 5)], check=False)),
                     lambda: g.list(4), lambda: g.path(0, "callees", 0, 1)):
            with pytest.raises(ffi.NativeError):
                call()
        g.bfs(0, "callees", [[0]], 2)
        for call in (lambda: g.list(4, first_level=3), lambda: g.list(-1), lambda: g.path(0, "callees", 0, 5), lambda: g.path(0, "callees", 64, 1)):
            with pytest.raises(ffi.NativeError):
                call()
        assert g.count(1) == (n, -1)                                              # the refused relation was not set
    finally:
        g.close()


def _csr(n, edges, check=True):
    off = np.zeros(n + 1, np.int64)
    off[1:] = len(edges)
    adj = np.asarray([b for _, b in edges], np.int32)
    return off, adj, off, adj


# ---------------------------------------------------------------------------------------------------- the store, end to end
STORE_N, STORE_DIM, NODES = 700, 384, 120


def _chunks():
    """Chunk i belongs to node i % 150: nodes 120 .. 149 are no nodes of the graph; every fifth chunk carries its key as the
    entity name only; a few hold the needle."""
    pay = []
    for i in range(STORE_N):
        p = {"file_path": f"src/m{i % 9}.py", "entity_type": "function", "entity_name": f"n{i % 150}", "language": "python" if i % 3 else "go",
             "content": f"def n{i % 150}(): pass" + ("  # retry_after\n" if i % 4 == 0 else ""), "start_line": i, "end_line": i + 1, "project_name": "p"}
        if i % 5:
            p["graph_node_id"], p["entity_name"] = p["entity_name"], f"other{i}"
        pay.append(p)
    return pay


def _store_graph():
    n, edges = gc.random_graph(NODES, 5, mean_degree=1, hubs=2, hub_degree=12)
    edges = [(a, b) for a, b in edges if a != b]
    seen, order = set(), []
    for a, b in edges:                                                           # node ids by first appearance, as the store numbers them
        for v in (a, b):
            if v not in seen:
                seen.add(v)
                order.append(v)
    return edges, [f"n{v}" for v in order], {v: i for i, v in enumerate(order)}


@pytest.mark.parametrize("shards", [1, 2])
def test_store_graph_filter_end_to_end(gpu, shards):
    ffi, _ = _env()
    from coderag_amd.store import HipVectorStore
    from oracle import search as orc
    pay = _chunks()
    rng = np.random.default_rng(31)
    raw = rng.standard_normal((STORE_N, STORE_DIM)).astype(np.float32)
    ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(STORE_N)]
    q = rng.standard_normal((3, STORE_DIM)).astype(np.float32)
    edges, names, number = _store_graph()
    numbered = [(number[a], number[b]) for a, b in edges]
    key = [p.get("graph_node_id") or p["entity_name"] for p in pay]
    alive = np.ones(STORE_N, bool)
    x_pre, q_pre = orc.preprocess(raw, to_bf16=True), orc.preprocess(q, to_bf16=True)

    def reached(direction, sources, hops, include_self=True):
        depth = gc.bfs_depths(len(names), numbered, direction, [names.index(s) for s in sources if s in names], hops)
        return {names[v] for v, d in depth.items() if include_self or d > 0}

    async def same(s, filters, must_not, mask, k=10):
        mask = mask & alive
        es, er = orc.search(x_pre, q_pre, k, alive=mask.astype(np.uint8))
        got = await s.search_batch("code_chunks", q, k, filters, must_not)
        for i in range(len(q)):
            keep = er[i] >= 0
            assert [h["id"] for h in got[i]] == [ids[r] for r in er[i][keep]], (filters, must_not)
            assert np.array_equal(np.asarray([h["score"] for h in got[i]], np.float32).view(U32), es[i][keep].view(U32))
        one = await s.search("code_chunks", q[1].tolist(), k, filters, must_not)
        assert [h["id"] for h in one] == [h["id"] for h in got[1]]
        assert await s.count_similar("code_chunks", q[2].tolist(), -2.0, filters, must_not) == int(mask.sum())
        fetched = await s.search("code_chunks", None, STORE_N, filters, must_not)
        assert [h["id"] for h in fetched] == [ids[r] for r in np.flatnonzero(mask)]
        return int(mask.sum())

    async def run():
        async with HipVectorStore(dim=STORE_DIM, dtype="bf16", initial_capacity=1024, device=0, shards=shards, compact_dead_fraction=0.0) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, raw, pay)
            col = s._col("code_chunks")
            await s.search("code_chunks", q[0].tolist(), 5, {"language": "python"})
            assert col._graph is None and col._graph_rows == {}                    # a collection never asked about its graph pays nothing
            info = await s.set_graph_edges("code_chunks", [(f"n{a}", f"n{b}") for a, b in edges])
            assert info == {"nodes": len(names), "relations": {"calls": len(set(edges))}}
            dead = list(range(0, STORE_N, 13))
            for i in dead:                                                       # tombstones, never compacted away
                await s.delete("code_chunks", {"start_line": i})
                alive[i] = False

            hub = names[0]
            for direction, word in (("callers", "callers_of"), ("callees", "callees_of"), ("both", "connected_to")):
                inside = reached(direction, [hub, "n7"], 2)
                mask = np.asarray([k in inside for k in key])
                spec = {"graph": {word: [hub, "n7"], "hops": 2}}
                n_in = await same(s, spec, None, mask)
                assert 0 < n_in < int(alive.sum())
                await same(s, None, spec, ~mask)
                await same(s, {**spec, "content": {"contains": "retry_after"}, "language": "python"}, {"file_path": "src/m2.py"},
                           mask & np.asarray([i % 4 == 0 and i % 3 != 0 and i % 9 != 2 for i in range(STORE_N)]))
                outside = reached(direction, [hub, "n7"], 2, include_self=False)
                await same(s, {"graph": {word: [hub, "n7"], "hops": 2, "include_self": False}}, None, np.asarray([k in outside for k in key]))
            calls = ffi.Graph.bfs_calls
            await same(s, {"graph": {"callers_of": [hub, "n7"], "hops": 2}}, None, np.asarray([k in reached("callers", [hub, "n7"], 2) for k in key]))
            assert ffi.Graph.bfs_calls == calls                                    # kept: no second BFS

            # neighbours (65 sets: two launches) and chains against the restatement
            sets = [[names[i % len(names)]] for i in range(65)]
            got = await s.graph_neighbors_batch("code_chunks", sets, direction="callees", max_hops=3, limit=20)
            for i, res in enumerate(got):
                depth = gc.bfs_depths(len(names), numbered, "callees", [i % len(names)], 3)
                order = sorted((d, v) for v, d in depth.items() if d > 0)
                assert res["count"] == len(order) and [(h["depth"], h["name"]) for h in res["hits"]] == [(d, names[v]) for d, v in order[:20]]
            for target in range(0, len(names), 9):
                want = gc.shortest_path(len(names), numbered, "callees", [0], target, 6)
                assert await s.call_chain("code_chunks", names[0], names[target], max_hops=6) == ([names[v] for v in want] or None)

            # search with graph expansion: related == the restatement run on the returned hits' own nodes
            many = rng.standard_normal((66, STORE_DIM)).astype(np.float32)
            out = await s.search_expanded_batch("code_chunks", many, 6, {"direction": "both", "hops": 2, "limit": 15}, {"language": "python"})
            plain = await s.search_batch("code_chunks", many, 6, {"language": "python"})
            saw = 0
            for res, hits in zip(out, plain):
                assert [(h["id"], h["score"]) for h in res["hits"]] == [(h["id"], h["score"]) for h in hits]
                src = [names.index(k) for k in (h["payload"].get("graph_node_id") or h["payload"]["entity_name"] for h in hits) if k in names]
                depth = gc.bfs_depths(len(names), numbered, "both", src, 2)
                order = sorted((d, v) for v, d in depth.items() if d > 0)
                assert res["related_count"] == len(order) and [(h["depth"], h["name"]) for h in res["related"]] == [(d, names[v]) for d, v in order[:15]]
                saw += len(order)
            assert saw > 0
            one = await s.search_expanded("code_chunks", many[3].tolist(), 6, {"direction": "both", "hops": 2, "limit": 15}, {"language": "python"})
            assert one["related"] == out[3]["related"] and [h["id"] for h in one["hits"]] == [h["id"] for h in out[3]["hits"]]
    asyncio.run(run())
