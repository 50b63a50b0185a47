"""Chains in full on the device: ``crh_graph_sigma`` / ``_chains`` / ``_between`` / ``_bfs_avoiding`` against the
restatement of tests/chains_cases.py, and ``call_chains`` / the ``between`` filter of the store against it and the f32 oracle.
Every comparison is an exact integer match; the output buffers start out full of garbage where the binding lets a caller hand
them over."""
import asyncio

import numpy as np
import pytest

from tests import chains_cases as cc
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
    return g


def _garbage(shape, dtype):
    import torch
    return torch.full(shape, -0x5a5a5a5b, dtype=dtype, device="cuda:0")


def _qs(nq):
    qs = 1
    while qs < nq:
        qs *= 2
    return qs


def _chains(g, n, edges, direction, sets, targets, hops, k, device_targets=False):
    """One BFS, sigma and chains of ``g`` against the restatement, every word; chain 0 against ``Graph.path``.  Returns the
    restatement's (nodes, length, count)."""
    import torch
    nq = len(sets)
    levels, _, _ = g.bfs(0, direction, sets, hops, include_self=True)
    want_levels = gc.bfs_words(n, edges, direction, sets, hops, include_self=True)[0]
    assert np.array_equal(levels.cpu().numpy().view(U64), want_levels)
    sig = g.sigma(0, direction, out=_garbage((n, _qs(nq)), torch.int64))
    want_sig = cc.sigma_words(n, edges, direction, sets, hops)
    got_sig = sig.cpu().numpy().view(U64)
    assert got_sig.shape == want_sig.shape and np.array_equal(got_sig, want_sig), np.argwhere(got_sig != want_sig)[:8]
    out = (_garbage((nq, k, hops + 1), torch.int32), _garbage((nq,), torch.int32), _garbage((nq,), torch.int64))
    given = torch.tensor(targets, dtype=torch.int32, device="cuda:0") if device_targets else targets
    nodes, length, count = (t.cpu().numpy() for t in g.chains(0, direction, given, k, out=out))
    want = cc.chains_arrays(n, edges, direction, sets, targets, hops, k)
    assert np.array_equal(count.view(U64), want[2]), (count.view(U64), want[2])
    assert np.array_equal(length, want[1]) and np.array_equal(nodes, want[0]), np.argwhere(nodes != want[0])[:8]
    for q, t in enumerate(targets):
        if 0 <= t < n:
            assert g.path(0, direction, q, t).tolist() == nodes[q, 0, :length[q]].tolist(), q
    return want


def _pairs(n, nq, seed, top, direction):
    """Source sets and targets for ``nq`` queries: ``graph_cases.random_sets`` (set 0 empty when there are several, a repeated
    source, overlapping sets), the planted ladder end to end, a target that is a source, a repeated pair, a target that is -1."""
    rng = np.random.default_rng(seed)
    sets = gc.random_sets(n, nq, seed)
    targets = rng.integers(0, n, size=nq).tolist()
    ends = (0, top) if direction == "callees" else (top, 0)
    at = 0 if nq == 1 else 1
    sets[at], targets[at] = [ends[0]], ends[1]
    if nq > 2:
        targets[2] = sets[2][0]                                          # a source: one chain of one node
    if nq > 5:
        sets[4], targets[4] = list(sets[at]), targets[at]               # the ladder's pair again
        targets[5] = -1
    return sets, targets


# ---------------------------------------------------------------------------------------------------- sizes and batch widths
@pytest.mark.parametrize("nq", [1, 2, 3, 33, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_node_counts_and_batch_widths(gpu, n, nq):
    """The lane, wave, workgroup and grid-stride boundaries, QS = 1, 2, 4, 64, 64 (a count that is no power of two, spare columns
    that stay 0, the wide form), both directions, max_hops 1 and 16."""
    n, edges, top = cc.with_ladder(n, seed=n + nq)
    plans = [("callees", 16), ("callers", 1)] if (n + nq) % 2 else [("callees", 1), ("callers", 16)]
    g = _graph(n, edges)
    try:
        for direction, hops in plans:
            sets, targets = _pairs(n, nq, n * 100 + nq, top, direction)
            _, length, count = _chains(g, n, edges, direction, sets, targets, hops, 10, device_targets=bool(nq % 2))
            at = 0 if nq == 1 else 1
            if hops == 16 and top:
                assert count[at] >= 1 and length[at] >= 2
            if nq > 2:
                assert (int(count[2]), int(length[2])) == (1, 1)
            if nq > 5:
                assert count[5] == 0 and count[4] == count[at] and count[0] == 0
    finally:
        g.close()


@pytest.mark.parametrize("nq", [1, 64])
@pytest.mark.parametrize("width,dead_first", [(63, 0), (64, 0), (65, 0), (300, 0), (20, 100), (20, 390), (300, 100)])
def test_lists_on_both_sides_of_the_wave_boundary(gpu, width, dead_first, nq):
    """Pull lists of 63, 64, 65 and 300 qualifying entries at the target and at an interior node: the lane's and the wave's walk
    of sigma (and the wide form's), the wave scan of the chains.  Entries that do not qualify stand between and before them:
    the sought rank then falls into the first, a middle or the last 64-entry step of the list.  K = 1, 10 and 64 with the
    count below, at and above K; unused chains and tails are -1."""
    for at_target in (True, False):
        n, edges, s, t = cc.fan(width, at_target, dead_first)
        mids = list(range(1 + dead_first, 1 + dead_first + 2 * width, 2))
        sets = [[[s], [mids[q % width]], []][q % 3] for q in range(nq)]
        g = _graph(n, edges)
        try:
            for k in ((1, 10, 64) if nq == 1 else (10,)):
                nodes, length, count = _chains(g, n, edges, "callees", sets, [t] * nq, 16, k)
                assert int(count[0]) == width and length[0] == (3 if at_target else 4)
                listed = min(k, width)
                assert nodes[0, :listed, 1].tolist() == mids[:listed] and (nodes[0, listed:] == -1).all() and (nodes[0, :, length[0]:] == -1).all()
            if nq > 1:
                assert (int(count[1]), int(length[1]), int(count[2])) == (1, 2 if at_target else 3, 0)
            if nq == 1:                                                          # against the edges the source's list is the long one
                _chains(g, n, edges, "callers", [[t]], [s], 16, 10)
        finally:
            g.close()


def test_count_equal_to_k(gpu):
    n, edges, s, t = cc.fan(10)
    g = _graph(n, edges)
    try:
        nodes, length, count = _chains(g, n, edges, "callees", [[s]], [t], 4, 10)
        assert int(count[0]) == 10 and (nodes[0, :, :3] >= 0).all() and (nodes[0, :, 3:] == -1).all()
    finally:
        g.close()


@pytest.mark.parametrize("nq", [1, 64])
@pytest.mark.parametrize("width", [19, 20])
def test_saturation(gpu, width, nq):
    """source, 15 complete layers, target, max_hops 16: 19 ** 15 chains fit a u64, 20 ** 15 do not -- and the first chains are
    still the restatement's."""
    n, edges, s, t = cc.layered(width)
    sets = [[s] if q in (0, 7, 63) else [] for q in range(nq)]
    g = _graph(n, edges)
    try:
        nodes, length, count = _chains(g, n, edges, "callees", sets, [t] * nq, 16, 10)
        assert int(count[0]) == (19 ** 15 if width == 19 else 2 ** 64 - 1) and length[0] == 17
        assert (int(count[0]) == cc.SATURATED) == (width == 20) and 19 ** 15 < 2 ** 64 < 20 ** 15
        assert nodes[0, 1].tolist() == [0, 2] + [1 + k * width for k in range(1, 15)] + [t]
        _chains(g, n, edges, "callees", sets, [t] * nq, 15, 10)                # one hop short: unreached
        _chains(g, n, edges, "callers", [[t]] + sets[1:], [s] * nq, 16, 3)
    finally:
        g.close()


def test_unreached_empty_and_several_sources(gpu):
    n, edges = gc.diamond()
    g = _graph(n, edges)
    try:
        sets = [[0], [], [6], [0, 2], [2, 0, 2], [1, 4], [0]]
        targets = [6, 5, 0, 5, 6, 5, 0]
        nodes, length, count = _chains(g, n, edges, "callees", sets, targets, 3, 4)
        assert count.tolist() == [1, 0, 0, 1, 1, 2, 1] and length.tolist() == [4, 0, 0, 3, 4, 2, 1]
        assert nodes[5, :2, :2].tolist() == [[1, 5], [4, 5]] and nodes[3, 0, :3].tolist() == [0, 1, 5]
        _chains(g, n, edges, "callees", sets, targets, 2, 4)                      # node 6 is three edges from node 0
        _chains(g, n, edges, "callers", [[5], [6]], [0, 2], 5, 64, device_targets=True)
        import torch
        g.bfs(0, "callees", [[0], [0], [0]], 4, include_self=True)
        g.sigma(0, "callees")
        wild = torch.tensor([5, n + 5, -7], dtype=torch.int32, device="cuda:0")   # device targets that are no nodes: count 0
        nodes, length, count = (t.cpu().numpy() for t in g.chains(0, "callees", wild, 2))
        assert count.tolist() == [1, 0, 0] and length.tolist() == [3, 0, 0] and (nodes[1:] == -1).all()
    finally:
        g.close()


def test_refusals_launch_nothing(gpu):
    import torch
    ffi, _ = _env()
    n, edges = gc.diamond()
    g = _graph(n, edges)
    try:
        levels, seen, active = g.bfs(0, "callees", [[0], [2]], 4, include_self=True)
        sig = g.sigma(0, "callees")
        torch.cuda.synchronize()
        keep = sig.clone()
        nodes, length, count = _garbage((2, 3, 5), torch.int32), _garbage((2,), torch.int32), _garbage((2,), torch.int64)
        marks = [t.clone() for t in (nodes, length, count)]
        for call in (lambda: g.sigma(0, "both"), lambda: g.sigma(1, "callees"), lambda: g.sigma(0, "callees", nq=65, max_hops=4, levels=levels, active=active),
                     lambda: g.sigma(0, "callees", nq=2, max_hops=17, levels=levels, active=active),
                     lambda: g.chains(0, "both", [5, 5], 3, out=(nodes, length, count)), lambda: g.chains(0, "callees", [5, n], 3, out=(nodes, length, count)),
                     lambda: g.chains(0, "callees", [5, -2], 3, out=(nodes, length, count)), lambda: g.chains(0, "callees", [5, 5], 0),
                     lambda: g.chains(0, "callees", [5, 5], 65), lambda: g.chains(0, "callees", [5], 3), lambda: g.chains(0, "callees", [5, 5], 3, out=(nodes, length, length)),
                     lambda: g.between(mode="any"), lambda: g.between(levels_back=levels, nq=2, max_hops=4, levels=levels, mode="nearest"),
                     lambda: g.between(levels_back=levels, nq=0, max_hops=4, levels=levels), lambda: g.between(levels_back=levels, nq=2, max_hops=0, levels=levels),
                     lambda: g.bfs_avoiding(0, "callees", [[0]], 3, seen[:3]), lambda: g.bfs_avoiding(0, "callees", [[0]], 3, [n])):
            with pytest.raises(ffi.NativeError) as e:
                call()
            assert e.value.code == ffi.E_INVALID
        lib, h = ffi.lib(), g._handle()
        assert lib.crh_graph_sigma(h, 0, 0, 2, None, active.data_ptr(), 4, sig.data_ptr(), None) == ffi.E_INVALID
        assert lib.crh_graph_sigma(None, 0, 0, 2, levels.data_ptr(), active.data_ptr(), 4, sig.data_ptr(), None) == ffi.E_INVALID
        assert lib.crh_graph_chains(h, 0, 0, 2, levels.data_ptr(), sig.data_ptr(), 4, None, 0, 3, nodes.data_ptr(), length.data_ptr(), count.data_ptr(), None) == ffi.E_INVALID
        assert lib.crh_graph_between(n, 2, levels.data_ptr(), levels.data_ptr(), 4, 2, active.data_ptr(), seen.data_ptr(), None, None) == ffi.E_INVALID
        assert lib.crh_graph_between(n, 2, levels.data_ptr(), None, 4, 0, active.data_ptr(), seen.data_ptr(), None, None) == ffi.E_INVALID
        off = np.zeros(2, np.int64)
        assert lib.crh_graph_bfs_avoiding(h, 0, 0, 1, off.ctypes.data, None, 0, 3, 1, None, levels.data_ptr(), seen.data_ptr(), active.data_ptr(), None) == ffi.E_INVALID
        torch.cuda.synchronize()
        assert torch.equal(sig, keep) and all(torch.equal(a, b) for a, b in zip((nodes, length, count), marks))
    finally:
        g.close()
    empty = ffi.Graph(0, device=0)                                              # a graph without nodes: CRH_OK, nothing launched
    try:
        empty.set_relation(0, np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.int32))
        empty.bfs(0, "callees", [[]], 3, include_self=True)
        empty.bfs(0, "callers", [[]], 3, include_self=True, back=True)
        assert tuple(empty.sigma(0, "callees").shape) == (0, 1)
        nodes, length, count = empty.chains(0, "callees", [-1], 2)
        assert (nodes.cpu().numpy() == -1).all() and length.tolist() == [0] and count.tolist() == [0]
        words, dist = empty.between()
        assert words.numel() == 0 and dist.tolist() == [-1]
        empty.bfs_avoiding(0, "callees", [[]], 3, [-1], include_self=True)
    finally:
        empty.close()


# ---------------------------------------------------------------------------------------------------- between
def _between(g, n, edges, direction, sets, target_sets, hops):
    import torch
    nq = len(sets)
    levels, _, _ = g.bfs(0, direction, sets, hops, include_self=True)
    back, _, _ = g.bfs(0, cc.OPPOSITE[direction], target_sets, hops, include_self=True, back=True)
    torch.cuda.synchronize()
    before = (levels.clone(), back.clone())
    out = []
    for mode in ("any", "shortest"):
        words, dist = g.between(mode=mode, out=_garbage((n,), torch.int64), dist=_garbage((nq,), torch.int32))
        want_w, want_d = cc.between_words(n, edges, direction, sets, target_sets, hops, mode == "shortest")
        got = words.cpu().numpy().view(U64)
        assert np.array_equal(got, want_w), (mode, np.flatnonzero(got != want_w)[:8])
        assert np.array_equal(dist.cpu().numpy(), want_d), mode
        out.append((want_w, want_d))
    only, none = g.between(mode="shortest", dist=None)
    assert np.array_equal(only.cpu().numpy().view(U64), out[1][0]) and np.array_equal(none.cpu().numpy(), out[1][1])
    assert torch.equal(levels, before[0]) and torch.equal(back, before[1])        # the levels it reads are not its workspace
    return out


@pytest.mark.parametrize("n,nq,hops", [(1, 1, 1), (64, 2, 16), (257, 33, 5), (1025, 64, 16), (255, 3, 1), (65, 64, 2)])
@pytest.mark.parametrize("direction", ["callees", "callers"])
def test_between(gpu, n, nq, hops, direction):
    n, edges, top = cc.with_ladder(n, seed=n + hops)
    sets, target_sets = gc.random_sets(n, nq, n + 1), gc.random_sets(n, nq, n + 2)
    if nq > 1:
        ends = (0, top) if direction == "callees" else (top, 0)
        sets[1], target_sets[1] = [ends[0]], [ends[1]]
        target_sets[0] = [0]                                                    # an empty source set: an all-zero column
    g = _graph(n, edges)
    try:
        (any_w, dist), (short_w, _) = _between(g, n, edges, direction, sets, target_sets, hops)
        if nq > 1:
            assert dist[0] == -1 and not (any_w & U64(1)).any()
            assert (short_w & ~any_w).sum() == 0
        if nq >= 33:
            assert len(set(dist.tolist())) >= (3 if hops >= 5 else 2)            # one batch, several distances: mode 1's masks differ per query
    finally:
        g.close()


def test_between_on_a_chain_mixes_distances(gpu):
    n, edges = gc.chain(20)
    edges = edges + [(3, 20), (20, 5)]                                           # a way round node 4 of the same length
    g = _graph(n + 1, edges)
    try:
        sets = [[0], [2], [19], [0], [3, 7], [0]]
        target_sets = [[19], [6], [0], [0], [9], [17]]
        (any_w, dist), (short_w, _) = _between(g, n + 1, edges, "callees", sets, target_sets, 16)
        assert dist.tolist() == [-1, 4, -1, 0, 2, -1]                            # 19 edges > 16; against the edges; the same node; from 7; 17 > 16
        assert [v for v in range(n + 1) if (int(short_w[v]) >> 1) & 1] == [2, 3, 4, 5, 6, 20]
        assert [v for v in range(n + 1) if (int(any_w[v]) >> 4) & 1] == [3, 4, 5, 6, 7, 8, 9, 20] and [v for v in range(n + 1) if (int(short_w[v]) >> 4) & 1] == [7, 8, 9]
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------- a BFS that avoids nodes
def test_bfs_avoiding_zero_words_equal_bfs(gpu):
    import torch
    n, edges, _ = cc.with_ladder(257, 5)
    sets = gc.random_sets(n, 33, 6)
    g = _graph(n, edges)
    try:
        for direction, hops, own in (("callees", 16, True), ("callers", 3, False), ("both", 4, False)):
            plain = [t.clone() for t in g.bfs(0, direction, sets, hops, include_self=own)]
            got = g.bfs_avoiding(0, direction, sets, hops, torch.zeros((n,), dtype=torch.int64, device="cuda:0"), include_self=own)
            assert all(torch.equal(a, b) for a, b in zip(plain, got)), direction
    finally:
        g.close()


@pytest.mark.parametrize("n,nq", [(65, 3), (257, 64)])
def test_bfs_avoiding_against_the_restatement(gpu, n, nq):
    import torch
    n, edges, _ = cc.with_ladder(n, 9)
    rng = np.random.default_rng(n)
    sets = gc.random_sets(n, nq, 10)
    avoid = np.zeros((n,), U64)
    gone = [rng.integers(0, n, size=int(rng.integers(0, 6))).tolist() for _ in range(nq)]
    gone[nq - 1] = gone[nq - 1] + sets[nq - 1][:1]                                 # an avoided source is dropped
    for q, nodes in enumerate(gone):
        for v in nodes:
            avoid[v] |= U64(1 << q)
    g = _graph(n, edges)
    try:
        for direction, hops in (("callees", 16), ("callers", 2)):
            levels, seen, active = g.bfs_avoiding(0, direction, sets, hops, torch.from_numpy(avoid.view(np.int64)).to("cuda:0"), include_self=True)
            want = np.zeros((hops + 1, n), U64)
            for q in range(nq):
                for v, d in cc.depths_avoiding(n, edges, direction, sets[q], hops, gone[q]).items():
                    want[d, v] |= U64(1 << q)
            got = levels.cpu().numpy().view(U64)
            assert np.array_equal(got, want), np.argwhere(got != want)[:8]
            assert np.array_equal(seen.cpu().numpy().view(U64), np.bitwise_or.reduce(want, axis=0))
            assert np.array_equal(active.cpu().numpy().view(U64), np.bitwise_or.reduce(want, axis=1))
            assert not (want[0, sets[nq - 1][0]] >> U64(nq - 1)) & U64(1)
    finally:
        g.close()


def _must_pass(g, sources, target, hops):
    """Must-pass as the store finds it: the interior of chain 0, one query bit per candidate, one avoided node per bit."""
    g.bfs(0, "callees", [sources], hops, include_self=True)
    g.sigma(0, "callees")
    nodes, length, _ = (t.cpu().numpy() for t in g.chains(0, "callees", [target], 1))
    cand = [int(v) for v in nodes[0, 0, 1:max(int(length[0]) - 1, 1)]]
    if not cand:
        return []
    g.bfs_avoiding(0, "callees", [sources] * len(cand), hops, cand, include_self=True)
    return [v for v, still in zip(cand, g.seen_bits([target] * len(cand))) if not still]


def test_must_pass(gpu):
    detour = cc.long_detour(7)[:2]                                               # the only way round node 1 has 8 edges
    cases = [(*gc.diamond(), [0], 5, 16, []), (*gc.chain(12), [0], 11, 16, list(range(1, 11))), (*cc.two_diamonds(), [0], 6, 16, [3]),
             (*cc.ladder(5), [0], 15, 16, [3, 6, 9, 12]), (*detour, [0], 2, 7, [1]), (*detour, [0], 2, 8, []), (*gc.chain(12), [0], 11, 10, []),
             (*gc.diamond(), [0, 2], 5, 16, [])]
    for n, edges, sources, target, hops, expect in cases:
        g = _graph(n, edges)
        try:
            got = _must_pass(g, sources, target, hops)
            assert got == cc.must_pass(n, edges, "callees", sources, target, hops) == expect, (n, sources, target, hops)
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
def test_store_call_chains_and_between_filter_end_to_end(gpu, shards):
    ffi, _ = _env()
    from coderag_amd.store import HipVectorStore
    from oracle import search as orc
    pay = _chunks()
    rng = np.random.default_rng(41)
    raw = rng.standard_normal((STORE_N, STORE_DIM)).astype(np.float32)
    ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(STORE_N)]
    q = rng.standard_normal((3, STORE_DIM)).astype(np.float32)
    _, edges, top = cc.with_ladder(NODES, 12, rungs=4)
    names = []
    for e in edges:                                                              # node ids by first appearance, as the store numbers them
        for v in e:
            if f"n{v}" not in names:
                names.append(f"n{v}")
    n = len(names)
    pairs = [(names.index(f"n{a}"), names.index(f"n{b}")) for a, b in edges]
    key = [p.get("graph_node_id") or p["entity_name"] for p in pay]
    x_pre, q_pre = orc.preprocess(raw, to_bf16=True), orc.preprocess(q, to_bf16=True)

    def answer(source, target, hops, limit):
        s, t = [names.index(v) for v in source], names.index(target)
        count, length, chains = cc.chains(n, pairs, "callees", s, t, hops, max(limit, 1))
        return {"count": count, "saturated": False, "length": length - 1 if length else None, "chains": [[names[v] for v in c] for c in chains[:limit]],
                "must_pass": [names[v] for v in cc.must_pass(n, pairs, "callees", s, t, hops)], "unresolved": []}

    async def same(s, filters, must_not, mask, k=10):
        es, er = orc.search(x_pre, q_pre, k, alive=mask.astype(np.uint8))
        got = await s.search_batch("code_chunks", q, k, filters, must_not)
        for i in range(len(q)):
            keep = er[i] >= 0
            assert [h["id"] for h in got[i]] == [ids[r] for r in er[i][keep]], (filters, must_not)
            assert np.array_equal(np.asarray([h["score"] for h in got[i]], np.float32).view(U32), es[i][keep].view(U32))
        fetched = await s.search("code_chunks", None, STORE_N, filters, must_not)
        assert [h["id"] for h in fetched] == [ids[r] for r in np.flatnonzero(mask)]
        return int(mask.sum())

    async def run():
        async with HipVectorStore(dim=STORE_DIM, dtype="bf16", initial_capacity=1024, device=0, shards=shards, compact_dead_fraction=0.0) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, raw, pay)
            col = s._col("code_chunks")
            await s.set_graph_edges("code_chunks", [(f"n{a}", f"n{b}") for a, b in edges])
            got = await s.call_chains("code_chunks", "n0", f"n{top}", max_hops=8)
            assert got == answer(["n0"], f"n{top}", 8, 10) and got["count"] >= 1 and got["chains"][0] == await s.call_chain("code_chunks", "n0", f"n{top}", max_hops=8)
            wanted = [([f"n{int(a)}" for a in rng.integers(0, NODES, size=int(rng.integers(1, 3))) if f"n{int(a)}" in names], f"n{int(b)}")
                      for b in rng.integers(0, NODES, size=70) if f"n{int(b)}" in names]
            wanted = [(a, b) for a, b in wanted if a] + [(["n0"], f"n{top}")]
            assert len(wanted) > 64
            batch = await s.call_chains_batch("code_chunks", wanted, max_hops=6, limit=3)
            assert batch == [answer(a, b, 6, 3) for a, b in wanted]
            assert sum(r["count"] > 1 for r in batch) >= 3 and any(r["must_pass"] for r in batch) and any(r["count"] == 0 for r in batch)

            calls = ffi.Graph.bfs_calls
            for hops, shortest in ((8, False), (8, True), (3, False)):
                inside = {names[v] for v in cc.between(n, pairs, "callees", [names.index("n0")], [names.index(f"n{top}")], hops, shortest)[0]}
                mask = np.asarray([k in inside for k in key])
                spec = {"graph": {"between": ["n0", f"n{top}"], "hops": hops, "shortest": shortest}}
                assert 0 < await same(s, spec, None, mask) < STORE_N
                await same(s, {"language": "python"}, spec, ~mask & np.asarray([i % 3 != 0 for i in range(STORE_N)]))
            assert ffi.Graph.bfs_calls == calls + 6 and col.graph_bfs_calls == 6   # two searches per condition; every repeat from the cache
    asyncio.run(run())
