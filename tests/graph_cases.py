"""The call graph's restatement and cases.  Test infrastructure only.

The restatement is a plain deque BFS per source set over adjacency dictionaries: no bit tricks, no CSR, no code shared with the
product.  Everything the device returns -- level words, seen words, lists, counts, row bitmaps, paths -- is rebuilt from its
depth maps and compared word for word."""
from collections import deque

import numpy as np

DIRECTIONS = ("callees", "callers", "both")           # along the edges, against them, either way (ffi.GRAPH_ALONG / _AGAINST / _BOTH)
WAVE_DEGREE = 64                                      # CRH_GRAPH_WAVE_DEGREE: lists of so many entries are walked by a wave


# ---------------------------------------------------------------------------------------------------- the restatement
def neighbours(n, edges, direction):
    """node -> the set of nodes one step away when travelling in ``direction``; self-loops never count."""
    out = {v: set() for v in range(n)}
    for a, b in edges:
        a, b = int(a), int(b)
        if a == b:
            continue
        if direction in ("callees", "both"):
            out[a].add(b)
        if direction in ("callers", "both"):
            out[b].add(a)
    return out


def bfs_depths(n, edges, direction, sources, max_hops):
    """node -> minimum depth (0 for a source) of the nodes within ``max_hops`` steps of the set ``sources`` (-1: padding)."""
    nb = neighbours(n, edges, direction)
    depth = {}
    queue = deque()
    for s in sources:
        s = int(s)
        if s >= 0 and s not in depth:
            depth[s] = 0
            queue.append(s)
    while queue:
        v = queue.popleft()
        if depth[v] == max_hops:
            continue
        for u in sorted(nb[v]):
            if u not in depth:
                depth[u] = depth[v] + 1
                queue.append(u)
    return depth


def bfs_words(n, edges, direction, source_sets, max_hops, include_self=False):
    """``(levels u64 [max_hops + 1, n], seen u64 [n], active u64 [max_hops + 1], depth maps)`` as crh_graph_bfs defines them."""
    levels = np.zeros((max_hops + 1, n), np.uint64)
    maps = []
    for q, sources in enumerate(source_sets):
        depth = bfs_depths(n, edges, direction, sources, max_hops)
        maps.append(depth)
        for v, d in depth.items():
            levels[d, v] |= np.uint64(1 << q)
    seen = np.bitwise_or.reduce(levels[0 if include_self else 1:], axis=0) if n else np.zeros((0,), np.uint64)
    active = np.bitwise_or.reduce(levels, axis=1) if n else np.zeros((max_hops + 1,), np.uint64)
    return levels, seen, active, maps


def listing(maps, first_level, limit):
    """``(nodes int32 [nq, limit], depth int32 [nq, limit], count int64 [nq])``: (depth, node id) order, padding -1."""
    nodes = np.full((len(maps), limit), -1, np.int32)
    depth = np.full((len(maps), limit), -1, np.int32)
    count = np.zeros((len(maps),), np.int64)
    for q, m in enumerate(maps):
        order = sorted((d, v) for v, d in m.items() if d >= first_level)
        count[q] = len(order)
        for i, (d, v) in enumerate(order[:limit]):
            nodes[q, i], depth[q, i] = v, d
    return nodes, depth, count


def row_words(row_node, reached, n_words=None):
    """u32 words: bit r set iff ``row_node[r]`` is a node of the set ``reached``."""
    row_node = np.asarray(row_node, np.int64)
    n_words = (len(row_node) + 31) // 32 if n_words is None else n_words
    bits = np.zeros((n_words * 32,), np.uint8)
    bits[: len(row_node)] = [1 if int(v) in reached else 0 for v in row_node]
    return np.packbits(bits, bitorder="little").view(np.uint32).copy() if n_words else np.zeros((0,), np.uint32)


def mask_from_words(words, n):
    return np.unpackbits(np.asarray(words).view(np.uint8), bitorder="little").astype(bool)[:n]


def shortest_path(n, edges, direction, sources, target, max_hops):
    """The path crh_graph_path defines: from the target's depth back, always to the smallest node one level up that is one
    step before the current one; [] when the target is not within ``max_hops``."""
    depth = bfs_depths(n, edges, direction, sources, max_hops)
    if target not in depth:
        return []
    nb = neighbours(n, edges, direction)
    path, cur = [target], target
    for d in range(depth[target], 0, -1):
        cur = min(p for p in range(n) if depth.get(p) == d - 1 and cur in nb[p])
        path.append(cur)
    return path[::-1]


# ---------------------------------------------------------------------------------------------------- graphs
def chain(length):
    """0 -> 1 -> ... -> length - 1."""
    return length, [(i, i + 1) for i in range(length - 1)]


def cycle(length):
    return length, [(i, (i + 1) % length) for i in range(length)]


def diamond():
    """0 -> 5 by paths of 2 edges (through 1) and of 4 (through 2, 3, 4); 6 hangs off 5: its minimum depth from 0 is 3."""
    return 7, [(0, 1), (1, 5), (0, 2), (2, 3), (3, 4), (4, 5), (5, 6)]


def asymmetric():
    """A graph whose three directions answer differently from node 2."""
    return 8, [(0, 1), (1, 2), (2, 3), (3, 4), (5, 2), (2, 6), (6, 7), (7, 6), (4, 0)]


def star(degree, extra=3):
    """Node 0 calls ``degree`` nodes (1 .. degree), each of which calls node degree + 1; a tail of ``extra`` nodes behind that:
    node 0's forward list and node degree + 1's reverse list both have ``degree`` entries."""
    hub, sink = 0, degree + 1
    edges = [(hub, i) for i in range(1, degree + 1)] + [(i, sink) for i in range(1, degree + 1)]
    edges += [(sink + j, sink + j + 1) for j in range(extra)]
    return sink + extra + 1, edges


def random_graph(n, seed, mean_degree=3, hubs=3, hub_degree=150):
    """``n`` nodes, ``mean_degree * n`` random edges (repeats and self-loops included, as a caller may hand them over), and a
    few hubs with ``hub_degree`` callers and as many callees -- on the wave's side of the degree boundary."""
    rng = np.random.default_rng(seed)
    edges = rng.integers(0, n, size=(mean_degree * n, 2)).tolist()
    for h in rng.choice(n, size=hubs, replace=False).tolist():
        k = min(hub_degree, n - 1)
        edges += [(h, int(v)) for v in rng.choice(n, size=k, replace=False)]
        edges += [(int(v), h) for v in rng.choice(n, size=k, replace=False)]
    return n, [(int(a), int(b)) for a, b in edges]


def random_sets(n, nq, seed, max_size=4):
    """``nq`` source sets: sizes 0 .. max_size, set 0 empty when there are several, overlapping and with a repeated source."""
    rng = np.random.default_rng(seed)
    sets = [rng.integers(0, n, size=int(rng.integers(1, max_size + 1))).tolist() for _ in range(nq)]
    if nq > 1:
        sets[0] = []
        sets[1] = sets[1] + sets[1][:1]                                   # a repeated source
    if nq > 3:
        sets[3] = sets[2] + sets[3]                                      # overlapping sets
    return sets


def csr_pair(n, edges):
    """The two CSRs by sorting Python tuples (the product's builder is numpy: tests compare the two)."""
    clean = sorted({(int(a), int(b)) for a, b in edges if a != b})
    out = []
    for key in (lambda e: e, lambda e: (e[1], e[0])):
        ordered = sorted(key(e) for e in clean)
        off = np.zeros(n + 1, np.int64)
        for a, _ in ordered:
            off[a + 1] += 1
        out += [np.cumsum(off), np.asarray([b for _, b in ordered], np.int32)]
    return tuple(out)


# ---------------------------------------------------------------------------------------------------- the CPU tier's fake
class FakeGraph:
    """``ffi.Graph`` on the host, built on the restatement above: same methods, numpy arrays for device tensors (int64 views of
    the u64 words, as the binding hands them out)."""
    bfs_calls = 0
    instances: list = []

    def __init__(self, n_nodes, device=0):
        self.n_nodes, self.device = int(n_nodes), device
        self.rel = {}
        self.levels = self.seen = self.active = None
        self.last = self.maps = None
        self.closed = False
        FakeGraph.instances.append(self)

    def close(self):
        self.closed = True

    def count(self, rel=0):
        return self.n_nodes, len(self.rel[rel]) if rel in self.rel else -1

    def set_relation(self, rel, off_fwd, adj_fwd, off_rev, adj_rev):
        off_fwd, adj_fwd = np.asarray(off_fwd, np.int64), np.asarray(adj_fwd, np.int32)
        assert len(off_fwd) == self.n_nodes + 1 == len(off_rev) and len(adj_fwd) == len(adj_rev) == off_fwd[-1]
        edges = [(a, int(b)) for a in range(self.n_nodes) for b in adj_fwd[off_fwd[a]:off_fwd[a + 1]]]
        back = [(int(a), b) for b in range(self.n_nodes) for a in np.asarray(adj_rev)[int(off_rev[b]):int(off_rev[b + 1])]]
        assert sorted(edges) == sorted(back), "the two CSRs hold different edges"
        self.rel[rel] = edges

    @staticmethod
    def _direction(direction):
        return direction if isinstance(direction, str) else DIRECTIONS[int(direction)]

    def bfs(self, rel, direction, sources, max_hops, include_self=False, stream=0):
        assert 1 <= max_hops <= 16
        sets = [list(s) for s in (np.asarray(sources).tolist() if isinstance(sources, np.ndarray) else sources)]
        assert 1 <= len(sets) <= 64
        FakeGraph.bfs_calls += 1
        levels, seen, active, self.maps = bfs_words(self.n_nodes, self.rel[rel], self._direction(direction), sets, max_hops, include_self)
        self.levels, self.seen, self.active = levels.view(np.int64), seen.view(np.int64), active.view(np.int64)
        self.last = (len(sets), max_hops)
        return self.levels, self.seen, self.active

    def list(self, limit, first_level=1, nq=None, max_hops=None, levels=None, stream=0):
        return listing(self.maps, first_level, int(limit))

    def row_words(self, row_node, q=0, n_words=None, out=None, seen=None, stream=0):
        seen = (self.seen if seen is None else seen).view(np.uint64)
        reached = {v for v in range(self.n_nodes) if (int(seen[v]) >> q) & 1}
        return row_words(row_node, reached, n_words).view(np.int32)

    def path(self, rel, direction, q, target, max_hops=None, levels=None, stream=0):
        lv = self.levels.view(np.uint64)
        sources = [v for v in range(self.n_nodes) if (int(lv[0, v]) >> q) & 1]
        return np.asarray(shortest_path(self.n_nodes, self.rel[rel], self._direction(direction), sources, int(target), self.last[1]), np.int32)
