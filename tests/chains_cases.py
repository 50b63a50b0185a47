"""Chains in full: the restatement, a brute force to hold it against, and cases.  Test infrastructure only.

The restatement follows the text of include/coderag_hip.h with Python ints, dictionaries and the deque BFS of
tests/graph_cases.py: chain counts (``min(..., 2**64 - 1)``), unranking, between, must-pass by a BFS with a node removed.  The
brute force enumerates every simple path by depth-first search and shares nothing with it."""
from collections import deque

import numpy as np

from tests import graph_cases as gc

SATURATED = 2 ** 64 - 1
MAX_CHAINS = 64                                       # CRH_GRAPH_MAX_CHAINS
OPPOSITE = {"callees": "callers", "callers": "callees"}


# ---------------------------------------------------------------------------------------------------- the restatement
def pull_lists(n, edges, direction):
    """node -> its pull list when travelling in ``direction``: the nodes one step BEFORE it, ascending, without repeats or
    self-loops -- the list the host builder hands to the device."""
    nb = gc.neighbours(n, edges, OPPOSITE[direction])
    return {u: sorted(nb[u]) for u in range(n)}


def depths_avoiding(n, edges, direction, sources, max_hops, avoid=()):
    """``graph_cases.bfs_depths`` that never enters a node of ``avoid`` (an avoided source is no source)."""
    avoid = {int(v) for v in avoid}
    nb = gc.neighbours(n, edges, direction)
    depth, queue = {}, deque()
    for s in sources:
        s = int(s)
        if s >= 0 and s not in depth and s not in avoid:
            depth[s] = 0
            queue.append(s)
    while queue:
        v = queue.popleft()
        if depth[v] == max_hops:
            continue
        for u in sorted(nb[v]):
            if u not in depth and u not in avoid:
                depth[u] = depth[v] + 1
                queue.append(u)
    return depth


def sigma(n, edges, direction, sources, max_hops):
    """``(depth map, node -> number of shortest chains from the set, saturated)``."""
    depth = gc.bfs_depths(n, edges, direction, sources, max_hops)
    pull = pull_lists(n, edges, direction)
    count = {v: 1 for v, d in depth.items() if d == 0}
    for d in range(1, max_hops + 1):
        for u in [u for u, du in depth.items() if du == d]:
            count[u] = min(sum(count[v] for v in pull[u] if depth.get(v) == d - 1), SATURATED)
    return depth, count


def sigma_words(n, edges, direction, source_sets, max_hops):
    """u64 [n, QS] as crh_graph_sigma writes it."""
    qs = 1
    while qs < len(source_sets):
        qs *= 2
    out = np.zeros((n, qs), np.uint64)
    for q, sources in enumerate(source_sets):
        for v, c in sigma(n, edges, direction, sources, max_hops)[1].items():
            out[v, q] = c
    return out


def unrank(depth, count, pull, target, rank):
    """Chain ``rank`` of the order by the node ids read backwards from the target, from a source to the target."""
    rem, u, chain = rank, target, [target]
    for d in range(depth[target], 0, -1):
        for v in pull[u]:
            if depth.get(v) != d - 1:
                continue
            if rem < count[v]:
                u = v
                break
            rem -= count[v]
        else:
            raise AssertionError("the rank is not below the count")
        chain.append(u)
    return chain[::-1]


def chains(n, edges, direction, sources, target, max_hops, k):
    """``(count, nodes per chain or 0, the first min(k, count) chains)`` of one pair."""
    depth, count = sigma(n, edges, direction, sources, max_hops)
    if target not in depth:
        return 0, 0, []
    pull = pull_lists(n, edges, direction)
    return count[target], depth[target] + 1, [unrank(depth, count, pull, target, r) for r in range(min(k, count[target]))]


def chains_arrays(n, edges, direction, source_sets, targets, max_hops, k):
    """``(nodes int32 [nq, k, max_hops + 1], length int32 [nq], count u64 [nq])`` as crh_graph_chains writes them."""
    nq = len(source_sets)
    nodes = np.full((nq, k, max_hops + 1), -1, np.int32)
    length, count = np.zeros((nq,), np.int32), np.zeros((nq,), np.uint64)
    for q, (sources, t) in enumerate(zip(source_sets, targets)):
        if not 0 <= t < n:
            continue
        c, ln, some = chains(n, edges, direction, sources, int(t), max_hops, k)
        count[q], length[q] = c, ln
        for r, chain in enumerate(some):
            nodes[q, r, :ln] = chain
    return nodes, length, count


def between(n, edges, direction, sources, targets, max_hops, shortest=False):
    """``(the set of nodes between, the distance of the two sets or -1)``: two deque BFS, one from either end."""
    df = gc.bfs_depths(n, edges, direction, sources, max_hops)
    db = gc.bfs_depths(n, edges, OPPOSITE[direction], targets, max_hops)
    both = {v: df[v] + db[v] for v in df if v in db and df[v] + db[v] <= max_hops}
    if not both:
        return set(), -1
    least = min(both.values())
    return {v for v, d in both.items() if not shortest or d == least}, least


def between_words(n, edges, direction, source_sets, target_sets, max_hops, shortest=False):
    """``(u64 [n], int32 [nq])`` as crh_graph_between writes them."""
    words, dist = np.zeros((n,), np.uint64), np.full((len(source_sets),), -1, np.int32)
    for q, (s, t) in enumerate(zip(source_sets, target_sets)):
        nodes, dist[q] = between(n, edges, direction, s, t, max_hops, shortest)
        for v in nodes:
            words[v] |= np.uint64(1 << q)
    return words, dist


def must_pass(n, edges, direction, sources, target, max_hops):
    """The nodes, other than the target and the sources, without which the target is not reached within ``max_hops``; in the
    order of chain 0.  By a BFS with the node removed."""
    _, _, first = chains(n, edges, direction, sources, target, max_hops, 1)
    if not first:
        return []
    ends = {int(s) for s in sources} | {target}
    return [v for v in first[0] if v not in ends and target not in depths_avoiding(n, edges, direction, sources, max_hops, [v])]


# ---------------------------------------------------------------------------------------------------- the brute force
def simple_paths(n, edges, direction, sources, target, max_hops):
    """Every simple path of at most ``max_hops`` edges from a node of ``sources`` to ``target``, by depth-first search."""
    nb = gc.neighbours(n, edges, direction)
    found = []

    def walk(path, on):
        if path[-1] == target:
            found.append(list(path))
            return
        if len(path) - 1 == max_hops:
            return
        for u in nb[path[-1]]:
            if u not in on:
                path.append(u)
                on.add(u)
                walk(path, on)
                on.discard(u)
                path.pop()

    for s in sorted({int(s) for s in sources if s >= 0}):
        walk([s], {s})
    return found


# ---------------------------------------------------------------------------------------------------- graphs
def ladder(rungs, base=0):
    """``rungs`` diamonds in a row: base -> {base + 1, base + 2} -> base + 3 -> ... : 2 ** rungs shortest chains of 2 * rungs
    edges from the first node to the last, every joint a must-pass node.  Returns (nodes used, edges)."""
    edges = []
    for r in range(rungs):
        a = base + 3 * r
        edges += [(a, a + 1), (a, a + 2), (a + 1, a + 3), (a + 2, a + 3)]
    return 3 * rungs + 1, edges


def with_ladder(n, seed, rungs=3):
    """``graph_cases.random_graph`` with a ladder planted over its first nodes (where there is room for one): the pair (0, 3 *
    rungs) then has chains, several of them, and joints."""
    n, edges = gc.random_graph(n, seed, hubs=min(3, n), hub_degree=min(150, max(n // 3, 1)))
    rungs = min(rungs, (n - 1) // 3)
    return n, edges + ladder(rungs)[1], 3 * rungs


def fan(width, at_target=True, dead_first=0):
    """A source, ``width`` nodes in the middle and a target -- the target's pull list (``at_target``) or, with one more node behind
    it, an interior node's has ``width`` qualifying entries, and ``width`` chains.  Entries that do NOT qualify (nodes the
    source does not reach) stand between them, and ``dead_first`` more before them all: they push the entry a rank asks for
    into a later 64-entry step of the list.  Returns (n, edges, source, target)."""
    src, first = 0, 1 + dead_first
    mid, join = list(range(first, first + 2 * width, 2)), first + 2 * width
    edges = [(src, m) for m in mid] + [(m, join) for m in mid]
    edges += [(m + 1, join) for m in mid[::7]] + [(v, join) for v in range(1, first)]     # unreached callers of the join
    if at_target:
        return join + 1, edges, src, join
    return join + 2, edges + [(join, join + 1)], src, join + 1


def layered(width, layers=15):
    """source, ``layers`` complete layers of ``width`` nodes, target: ``width ** layers`` chains of ``layers + 1`` edges."""
    edges = [(0, 1 + i) for i in range(width)]
    for k in range(layers - 1):
        a, b = 1 + k * width, 1 + (k + 1) * width
        edges += [(a + i, b + j) for i in range(width) for j in range(width)]
    last, target = 1 + (layers - 1) * width, 1 + layers * width
    edges += [(last + i, target) for i in range(width)]
    return target + 1, edges, 0, target


def two_diamonds():
    """0 -> {1, 2} -> 3 -> {4, 5} -> 6: node 3 is the articulation."""
    return 7, [(0, 1), (0, 2), (1, 3), (2, 3), (3, 4), (3, 5), (4, 6), (5, 6)]


def long_detour(hops):
    """0 -> 1 -> 2 beside a detour 0 -> 3 -> ... -> 2 that avoids node 1 and is exactly ``hops + 1`` edges long: within ``hops``
    node 1 is a must-pass node, within ``hops + 1`` it is not.  Returns (n, edges, source, target)."""
    via = list(range(3, 3 + hops))
    edges = [(0, 1), (1, 2), (0, via[0])] + [(a, b) for a, b in zip(via, via[1:])] + [(via[-1], 2)]
    return 3 + hops, edges, 0, 2


# ---------------------------------------------------------------------------------------------------- the CPU tier's fake
class FakeChainsGraph(gc.FakeGraph):
    """``graph_cases.FakeGraph`` plus the chain methods of ``ffi.Graph``, on the restatement above."""

    def __init__(self, n_nodes, device=0):
        super().__init__(n_nodes, device)
        self.levels_back = self.seen_back = self.active_back = self.last_back = None
        self.sets = self.sets_back = self.asked = self.asked_back = None

    def bfs(self, rel, direction, sources, max_hops, include_self=False, stream=0, back=False, avoid=None):
        assert 1 <= max_hops <= 16
        sets = [list(s) for s in (np.asarray(sources).tolist() if isinstance(sources, np.ndarray) else sources)]
        assert 1 <= len(sets) <= 64
        gc.FakeGraph.bfs_calls += 1
        direction = self._direction(direction)
        levels = np.zeros((max_hops + 1, self.n_nodes), np.uint64)
        for q, s in enumerate(sets):
            gone = [] if avoid is None else [v for v in range(self.n_nodes) if (int(np.asarray(avoid).view(np.uint64)[v]) >> q) & 1]
            for v, d in depths_avoiding(self.n_nodes, self.rel[rel], direction, s, max_hops, gone).items():
                levels[d, v] |= np.uint64(1 << q)
        seen = np.bitwise_or.reduce(levels[0 if include_self else 1:], axis=0) if self.n_nodes else np.zeros((0,), np.uint64)
        active = np.bitwise_or.reduce(levels, axis=1) if self.n_nodes else np.zeros((max_hops + 1,), np.uint64)
        got = (levels.view(np.int64), seen.view(np.int64), active.view(np.int64))
        if back:
            self.levels_back, self.seen_back, self.active_back = got
            self.last_back, self.sets_back, self.asked_back = (len(sets), max_hops), sets, (rel, direction)
        else:
            self.levels, self.seen, self.active = got
            self.last, self.sets, self.asked = (len(sets), max_hops), sets, (rel, direction)
            self.maps = [gc.bfs_depths(self.n_nodes, self.rel[rel], direction, s, max_hops) for s in sets] if avoid is None else None
        return got

    def avoid_words(self, nodes):
        out = np.zeros((self.n_nodes,), np.uint64)
        for q, v in enumerate(nodes):
            if v >= 0:
                out[int(v)] |= np.uint64(1 << q)
        return out.view(np.int64)

    def bfs_avoiding(self, rel, direction, sources, max_hops, avoid, include_self=False, stream=0, back=False):
        if not isinstance(avoid, np.ndarray):
            avoid = self.avoid_words(avoid)
        return self.bfs(rel, direction, sources, max_hops, include_self=include_self, back=back, avoid=avoid)

    def seen_bits(self, nodes, seen=None):
        seen = (self.seen if seen is None else seen).view(np.uint64)
        return np.asarray([v >= 0 and bool((int(seen[int(v)]) >> q) & 1) for q, v in enumerate(nodes)], bool)

    def sigma(self, rel, direction, nq=None, max_hops=None, levels=None, active=None, out=None, stream=0):
        assert levels is None and (rel, self._direction(direction)) == self.asked, "sigma reads the last bfs"
        self.sigma_last = sigma_words(self.n_nodes, self.rel[rel], self.asked[1], self.sets, self.last[1]).view(np.int64)
        return self.sigma_last

    def chains(self, rel, direction, targets, k, nq=None, max_hops=None, levels=None, sigma=None, out=None, stream=0):
        assert levels is None and (rel, self._direction(direction)) == self.asked and 1 <= k <= MAX_CHAINS
        nodes, length, count = chains_arrays(self.n_nodes, self.rel[rel], self.asked[1], self.sets, list(targets), self.last[1], int(k))
        return nodes, length, count.view(np.int64)

    def between(self, levels_back=None, mode="any", nq=None, max_hops=None, levels=None, out=None, dist=None, stream=0):
        assert self.last == self.last_back and self.asked[0] == self.asked_back[0] and self.asked_back[1] == OPPOSITE[self.asked[1]]
        before = (self.levels.copy(), self.levels_back.copy())
        words, dist = between_words(self.n_nodes, self.rel[self.asked[0]], self.asked[1], self.sets, self.sets_back, self.last[1], mode in ("shortest", 1))
        assert np.array_equal(before[0], self.levels) and np.array_equal(before[1], self.levels_back)
        return words.view(np.int64), dist
