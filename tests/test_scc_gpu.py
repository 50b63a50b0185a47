"""Components and layers on the device: ``crh_graph_scc`` / ``_scc_bins`` / ``_layers`` / ``_node_words`` against the iterative
Tarjan and the topological-order layers of tests/scc_cases.py, and the ``in_cycle`` filter of the store against the f32 oracle
under the restatement's mask.  Every comparison is an exact integer match; the output buffers start out full of garbage where
the binding lets a caller hand them over."""
import asyncio

import numpy as np
import pytest

from tests import graph_cases as gc
from tests import scc_cases as sc

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
    return g


def _whole(n, edges, loops=None):
    """Components, bins and both layer arrays of one graph against the restatement; returns (comp, bins, depth, height, info)."""
    import torch
    ffi, _ = _env()
    g = _graph(n, edges)
    try:
        comp, info = g.scc(0)
        want = sc.components(n, [(a, b) for a, b in edges if a != b])
        got = comp.cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, want), np.flatnonzero(got != want)[:8]
        # launched sweeps: 16 per read-back, of which one at least ran, and at most (n + 2)^2 run (CRH_GRAPH_SCC_MAX_SWEEPS)
        assert info[:3].tolist() == sc.scc_info(n, want) and 1 <= info[3] <= 16 * (n + 2) ** 2
        loops = sc.self_nodes(edges) if loops is None else np.asarray(loops, np.int32)
        bins = g.scc_bins(comp, loops)
        want_bins = sc.cyclic_bins(n, want, loops.tolist())
        assert np.array_equal(bins.cpu().numpy(), want_bins)
        out = [want, want_bins]
        for direction in ("callees", "callers"):
            layer, linfo = g.layers(0, direction, comp)
            want_l = sc.layers(n, edges, want, direction)
            assert np.array_equal(layer.cpu().numpy(), want_l), (direction, np.flatnonzero(layer.cpu().numpy() != want_l)[:8])
            assert linfo[0] == int(want_l.max()) + 1 and 1 <= linfo[1]
            out.append(want_l)
        torch.cuda.synchronize()
        return (*out, info)
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------- sizes and degrees
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_node_counts(gpu, n):
    """The lane, wave, workgroup and grid-stride boundaries: a sparse random graph with a planted cycle through the last node."""
    _, edges = gc.random_graph(n, n, mean_degree=1, hubs=1 if n > 8 else 0, hub_degree=9)
    if n >= 3:
        edges += [(n - 1, 0), (0, n // 2), (n // 2, n - 1)]
    comp, bins, depth, height, info = _whole(n, edges)
    if n >= 3:
        assert comp[n - 1] == 0 and bins[0] >= 3 and info[1] >= 1
    else:
        assert comp.tolist() == [0] and info[:3].tolist() == [1, 0, 0] and depth.tolist() == [0] == height.tolist()


@pytest.mark.parametrize("inside", [True, False])
@pytest.mark.parametrize("degree", [63, 64, 65, 300])
def test_lists_on_both_sides_of_the_wave_boundary(gpu, degree, inside):
    """A hub whose in-list and out-list have ``degree`` entries: the lane's walk below CRH_GRAPH_WAVE_DEGREE, the wave's from it
    on -- in the trim, the colouring (in-list), the back-mark (out-list) and both layer sweeps."""
    ffi, _ = _env()
    assert ffi.GRAPH_WAVE_DEGREE == 64
    n, edges = sc.wide_lists(degree, inside)
    comp, bins, depth, height, info = _whole(n, edges)
    if inside:
        assert bins[0] == 2 * degree + 1 and (comp[: 2 * degree + 1] == 0).all() and info[:3].tolist() == [3, 1, 2 * degree + 1]
        assert depth[0] == 1 and height[0] == 1
    else:
        assert not bins.any() and np.array_equal(comp, np.arange(n)) and depth[0] == 2 and height[0] == 2


def test_empty_relation_and_no_nodes(gpu):
    comp, bins, depth, height, info = _whole(70, [])
    assert np.array_equal(comp, np.arange(70)) and not bins.any() and not depth.any() and not height.any() and info[:3].tolist() == [70, 0, 0]
    ffi, _ = _env()
    g = _graph(0, [])
    try:
        comp, info = g.scc(0)
        assert comp.numel() == 0 and info.tolist() == [0, 0, 0, 0]
        layer, linfo = g.layers(0, "callees", comp)
        assert layer.numel() == 0 and linfo.tolist() == [0, 0]
        assert g.scc_bins(comp).numel() == 0 and g.node_words("range", layer, lo=0, hi=3).numel() == 0
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------- shapes of graphs
def test_chain_is_trimmed_away(gpu):
    """300 nodes, no cycle: the trim alone assigns every node -- many sweeps, and neither a colouring nor a back-mark after them
    (both would need a node left), so the sweeps that ran are at most one per node and the one that found nothing."""
    n, edges = gc.chain(300)
    comp, bins, depth, height, info = _whole(n, edges)
    assert np.array_equal(comp, np.arange(n)) and not bins.any() and info[:3].tolist() == [300, 0, 0]
    assert depth.tolist() == list(range(300)) and height.tolist() == list(range(299, -1, -1))
    assert info[3] <= 300 + 1 + 15                                               # (launched: the last batch of 16 may overshoot by 15)


def test_small_shapes(gpu):
    n, edges = gc.cycle(7)
    comp, bins, depth, height, info = _whole(n, edges)
    assert comp.tolist() == [0] * 7 and bins.tolist() == [7] + [0] * 6 and info[:3].tolist() == [1, 1, 7] and not depth.any() and not height.any()

    comp, bins, depth, height, info = _whole(*sc.two_cycles_joined())
    assert comp.tolist() == [0, 0, 0, 3, 3] and bins.tolist() == [3, 0, 0, 2, 0] and depth.tolist() == [0, 0, 0, 1, 1] and height.tolist() == [1, 1, 1, 0, 0]

    comp, bins, depth, height, info = _whole(*sc.figure_of_eight())
    assert comp.tolist() == [0] * 5 and bins[0] == 5 and info[:3].tolist() == [1, 1, 5]

    comp, bins, depth, height, info = _whole(*sc.complete(5))
    assert comp.tolist() == [0] * 5 and bins[0] == 5

    comp, bins, depth, height, info = _whole(*gc.diamond())
    assert comp.tolist() == list(range(7)) and depth.tolist() == [0, 1, 1, 2, 3, 4, 5] and height.tolist() == [5, 2, 4, 3, 2, 1, 0]   # LONGEST paths

    comp, bins, depth, height, info = _whole(*sc.cycle_entered_above_its_minimum())
    assert comp.tolist() == [0, 1, 2, 2, 4, 2] and bins.tolist() == [0, 0, 3, 0, 0, 0] and depth.tolist() == [0, 1, 2, 2, 3, 2]

    comp, bins, depth, height, info = _whole(*gc.asymmetric())
    assert comp.tolist() == [0, 0, 0, 0, 0, 5, 6, 6] and bins[0] == 5 and bins[6] == 2


def test_cycles_under_a_tail_need_several_rounds(gpu):
    n, edges = sc.cycle_under_a_tail(40)
    comp, bins, depth, height, info = _whole(n, edges)
    assert comp[:8].tolist() == [0, 0, 0, 3, 3, 5, 5, 5] and np.array_equal(comp[8:], np.arange(8, n))
    assert depth[3] == 41 and depth[5] == 42 and height[0] == 42 and info[:3].tolist() == [n - 5, 3, 8]


def test_self_loops_make_single_nodes_cyclic(gpu):
    """The CSRs hold no self-loop: the nodes that carried one are handed to crh_graph_scc_bins.  One of a component of two changes
    nothing; one of a single node makes it a cyclic component of size 1."""
    n, edges = 6, [(0, 1), (1, 0), (1, 1), (2, 3), (4, 4), (3, 5), (5, 5)]
    comp, bins, depth, height, info = _whole(n, edges)
    assert comp.tolist() == [0, 0, 2, 3, 4, 5] and bins.tolist() == [2, 0, 0, 0, 1, 1] and info[:3].tolist() == [5, 1, 2]
    comp, bins, *_ = _whole(n, edges, loops=[])
    assert bins.tolist() == [2, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("seed", [1, 2])
def test_random_graphs_under_a_relabelling(gpu, seed):
    """2000 nodes, planted components of 2 .. 200 nodes in a random DAG.  Under a random renumbering of the nodes the components
    are the same SETS, labelled by their smallest NEW id, and the layers travel with the nodes."""
    n, edges = sc.planted(2000, seed)
    comp, bins, depth, height, info = _whole(n, edges)
    assert info[1] >= 1 and bins.max() >= 200                                    # (planted cycles may merge, never split)
    _, moved, perm = sc.relabel(n, edges, seed + 10)
    comp2, bins2, depth2, height2, info2 = _whole(n, moved)
    assert info2[:3].tolist() == info[:3].tolist()
    assert np.array_equal(depth2[perm], depth) and np.array_equal(height2[perm], height)
    groups = {}
    for v in range(n):
        groups.setdefault(int(comp[v]), []).append(int(perm[v]))
    for v in range(n):
        assert comp2[perm[v]] == min(groups[int(comp[v])])


def test_layers_across_three_cyclic_components(gpu):
    comp, bins, depth, height, info = _whole(*sc.three_cyclic_layers())
    assert comp.tolist() == [0, 0, 2, 3, 3, 5, 5, 5, 8, 9]
    assert depth.tolist() == [0, 0, 1, 2, 2, 3, 3, 3, 0, 4] and height.tolist() == [4, 4, 3, 2, 2, 1, 1, 1, 3, 0]


# ---------------------------------------------------------------------------------------------------- listings and conditions
def test_bins_and_facet_select_with_a_tie(gpu):
    """Cycles of 4, 3, 3 and 2 nodes and a self-loop: the largest first, the tie in size to the lower label."""
    ffi, _ = _env()
    edges = [(10, 11), (11, 12), (12, 10), (0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 6), (6, 3), (7, 8), (8, 7), (9, 9), (2, 3), (13, 10)]
    n = 14
    g = _graph(n, edges)
    try:
        comp, info = g.scc(0)
        bins = g.scc_bins(comp, sc.self_nodes(edges))
        want = sc.cyclic_bins(n, sc.components(n, edges), [9])
        assert np.array_equal(bins.cpu().numpy(), want) and want.tolist() == [3, 0, 0, 4, 0, 0, 0, 2, 0, 1, 3, 0, 0, 0]
        for k in (1, 3, 5, 8):
            codes, counts, finfo = (t.cpu().numpy() for t in ffi.facet_select(bins, k))
            top = sc.top_components(want, k)
            assert codes[0].tolist() == [c for c, _ in top] + [-1] * (k - len(top)) and counts[0].tolist() == [s for _, s in top] + [0] * (k - len(top))
            assert finfo[0].tolist() == [5, 13]
        assert sc.top_components(want, 3) == [(3, 4), (0, 3), (10, 3)]
    finally:
        g.close()


@pytest.mark.parametrize("q", [0, 31, 32, 63])
def test_node_words_then_row_words(gpu, q):
    import torch
    ffi, _ = _env()
    n, edges = sc.planted(300, 5, sizes=(2, 3, 40))
    g = _graph(n, edges)
    try:
        comp, _ = g.scc(0)
        bins = g.scc_bins(comp, sc.self_nodes(edges))
        depth, _ = g.layers(0, "callees", comp)
        want_comp = sc.components(n, edges)
        want_bins = sc.cyclic_bins(n, want_comp, sc.self_nodes(edges).tolist())
        want_depth = sc.layers(n, edges, want_comp, "callees")
        label = int(np.argmax(want_bins))                                         # the largest cycle (planted ones may have merged)
        assert want_bins[label] >= 40
        rng = np.random.default_rng(q)
        row_node = rng.integers(-1, n, size=1000).astype(np.int32)
        rows = torch.from_numpy(row_node).to("cuda:0")
        out = torch.full((n,), -77, dtype=torch.int64, device="cuda:0")
        for mode, values, wv, kw in (("in_cycle", comp, want_comp, {"bins": bins}), ("same_component", comp, want_comp, {"lo": label}),
                                     ("range", depth, want_depth, {"lo": 2, "hi": 4}), ("range", depth, want_depth, {"lo": 0, "hi": 0}),
                                     ("range", depth, want_depth, {"lo": 5, "hi": 4})):
            words = g.node_words(mode, values, q=q, out=out, **kw)
            want = sc.node_words(mode, wv, want_bins if mode == "in_cycle" else None, kw.get("lo", 0), kw.get("hi", 0), q)
            assert np.array_equal(words.cpu().numpy().view(U64), want), mode
            hit = set(np.flatnonzero(want).tolist())
            got = g.row_words(rows, q, seen=words).cpu().numpy().view(U32)
            assert np.array_equal(got, gc.row_words(row_node, hit)), mode
        assert len(hit) == 0                                                      # (the empty range)
    finally:
        g.close()


def test_bad_arguments(gpu):
    import ctypes as C
    import torch
    ffi, _ = _env()
    n, edges = gc.cycle(5)
    g = _graph(n, edges)
    try:
        comp, _ = g.scc(0)
        marker = comp.clone()
        short = torch.zeros((n - 1,), dtype=torch.int32, device="cuda:0")
        for call in (lambda: g.scc(1), lambda: g.scc(8), lambda: g.layers(1, "callees", comp), lambda: g.layers(0, "both", comp),
                     lambda: g.layers(0, "sideways", comp), lambda: g.layers(0, "callees", short), lambda: g.layers(0, "callees", comp.long()),
                     lambda: g.scc_bins(short), lambda: g.scc_bins(comp, np.arange(n + 1)),
                     lambda: g.node_words("nowhere", comp), lambda: g.node_words("in_cycle", comp), lambda: g.node_words("range", comp, q=64),
                     lambda: g.node_words("range", comp, q=-1), lambda: g.node_words("range", short)):
            with pytest.raises(ffi.NativeError) as e:
                call()
            assert e.value.code == ffi.E_INVALID
        lib, info = ffi.lib(), np.full((4,), 7, np.int64)
        h = g._handle()
        assert lib.crh_graph_scc(h, 0, None, None, info.ctypes.data, None) == ffi.E_INVALID and info.tolist() == [0, 0, 0, 0]
        assert lib.crh_graph_scc(h, 0, comp.data_ptr(), comp.data_ptr(), None, None) == ffi.E_INVALID
        assert lib.crh_graph_scc(None, 0, comp.data_ptr(), comp.data_ptr(), info.ctypes.data, None) == ffi.E_INVALID
        assert lib.crh_graph_layers(h, 0, 0, comp.data_ptr(), None, None, info.ctypes.data, None) == ffi.E_INVALID
        assert lib.crh_graph_scc_bins(n, comp.data_ptr(), None, 2, comp.data_ptr(), None) == ffi.E_INVALID
        assert lib.crh_graph_scc_bins(-1, comp.data_ptr(), None, 0, comp.data_ptr(), None) == ffi.E_INVALID
        assert lib.crh_graph_node_words(n, 3, comp.data_ptr(), None, 0, 0, 0, comp.data_ptr(), None) == ffi.E_INVALID
        assert lib.crh_graph_node_words(n, 2, None, None, 0, 0, 0, comp.data_ptr(), None) == ffi.E_INVALID
        torch.cuda.synchronize()
        assert torch.equal(comp, marker)                                          # nothing was launched on the refused calls
        # labels that are no components of this relation (every node its own, on a cycle): refused at the sweep bound, no endless loop
        own = torch.arange(n, dtype=torch.int32, device="cuda:0")
        with pytest.raises(ffi.NativeError) as e:
            g.layers(0, "callees", own)
        assert e.value.code == ffi.E_INTERNAL and "sweeps" in str(e.value)
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


@pytest.mark.parametrize("shards", [1, 2])
def test_store_in_cycle_filter_end_to_end(gpu, shards):
    ffi, _ = _env()
    from coderag_amd.store import HipVectorStore
    from oracle import search as orc
    pay = _chunks()
    rng = np.random.default_rng(37)
    raw = rng.standard_normal((STORE_N, STORE_DIM)).astype(np.float32)
    ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(STORE_N)]
    q = rng.standard_normal((3, STORE_DIM)).astype(np.float32)
    _, edges = sc.planted(NODES, 9, sizes=(2, 3, 9), extra=1)
    names = []
    for e in edges:                                                              # node ids by first appearance, as the store numbers them
        for v in e:
            if f"n{v}" not in names:
                names.append(f"n{v}")
    pairs = [(names.index(f"n{a}"), names.index(f"n{b}")) for a, b in edges]
    comp = sc.components(len(names), pairs)
    loops = sc.self_nodes(pairs)
    bins = sc.cyclic_bins(len(names), comp, loops)
    height = sc.layers(len(names), pairs, comp, "callers")
    key = [p.get("graph_node_id") or p["entity_name"] for p in pay]
    alive = np.ones(STORE_N, bool)
    x_pre, q_pre = orc.preprocess(raw, to_bf16=True), orc.preprocess(q, to_bf16=True)

    def rows(cond):
        inside = {names[v] for v in range(len(names)) if cond(v)}
        return np.asarray([k in inside for k in key])

    async def same(s, filters, must_not, mask, k=10):
        mask = mask & alive
        es, er = orc.search(x_pre, q_pre, k, alive=mask.astype(np.uint8))
        got = await s.search_batch("code_chunks", q, k, filters, must_not)
        for i in range(len(q)):
            keep = er[i] >= 0
            assert [h["id"] for h in got[i]] == [ids[r] for r in er[i][keep]], (filters, must_not)
            assert np.array_equal(np.asarray([h["score"] for h in got[i]], np.float32).view(U32), es[i][keep].view(U32))
        assert await s.count_similar("code_chunks", q[2].tolist(), -2.0, filters, must_not) == int(mask.sum())
        fetched = await s.search("code_chunks", None, STORE_N, filters, must_not)
        assert [h["id"] for h in fetched] == [ids[r] for r in np.flatnonzero(mask)]
        return int(mask.sum())

    async def run():
        async with HipVectorStore(dim=STORE_DIM, dtype="bf16", initial_capacity=1024, device=0, shards=shards, compact_dead_fraction=0.0) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, raw, pay)
            col = s._col("code_chunks")
            await s.set_graph_edges("code_chunks", [(f"n{a}", f"n{b}") for a, b in edges])
            for i in range(0, STORE_N, 13):                                      # tombstones, never compacted away
                await s.delete("code_chunks", {"start_line": i})
                alive[i] = False
            calls = ffi.Graph.scc_calls
            in_cycle = rows(lambda v: bins[comp[v]] > 0)
            spec = {"graph": {"in_cycle": True}}
            assert 0 < await same(s, spec, None, in_cycle) < int(alive.sum())
            await same(s, None, spec, ~in_cycle)
            await same(s, {**spec, "language": "python"}, {"file_path": "src/m2.py"}, in_cycle & np.asarray([i % 3 != 0 and i % 9 != 2 for i in range(STORE_N)]))
            big = int(np.argmax(bins))
            await same(s, {"graph": {"same_cycle_as": names[big]}}, None, rows(lambda v: comp[v] == big))
            await same(s, {"graph": {"height": 0}}, spec, rows(lambda v: height[v] == 0) & ~in_cycle)
            await same(s, {"graph": {"height": {"gte": 1, "lte": 2}}}, None, rows(lambda v: 1 <= height[v] <= 2))
            assert ffi.Graph.scc_calls == calls + 1 == calls + col.graph_scc_calls  # one component pass served every filter

            got = await s.graph_cycles("code_chunks", limit=4, members=5)
            top = sc.top_components(bins, 4)
            assert [(c["id"], c["size"]) for c in got["components"]] == [(names[c], size) for c, size in top]
            assert got["components"][0]["nodes"] == [names[v] for v in np.flatnonzero(comp == top[0][0])[:5]]
            assert (got["count"], got["nodes"]) == (int((bins > 0).sum()), int(bins.sum()))
            assert got["self_recursive"] == [names[v] for v in loops.tolist() if bins[comp[v]] == 1]
            lay = await s.graph_layers("code_chunks", names=[names[0], names[big]])
            depth = sc.layers(len(names), pairs, comp, "callees")
            assert lay["layers"] == int(depth.max()) + 1 == int(height.max()) + 1
            assert lay["histogram"] == {"depth": np.bincount(depth).tolist(), "height": np.bincount(height).tolist()}
            assert [(n["name"], n["depth"], n["height"], n["component"], n["cyclic"]) for n in lay["nodes"]] == sorted(
                {(names[v], int(depth[v]), int(height[v]), names[comp[v]], bool(bins[comp[v]] > 0)) for v in (0, big)}, key=lambda t: names.index(t[0]))
            assert ffi.Graph.scc_calls == calls + 1
    asyncio.run(run())
