"""Components and layers of the call graph: the restatement and the cases.  Test infrastructure only.

The restatement is an iterative Tarjan over adjacency lists and a dynamic programme over a topological order of the
condensation: no sweeps, no colours, no CSR, no code shared with the product.  Every array the device returns is rebuilt here
and compared word for word."""
import numpy as np

from tests import graph_cases as gc


# ---------------------------------------------------------------------------------------------------- the restatement
def _lists(n, edges):
    out = [[] for _ in range(n)]
    for a, b in edges:
        out[int(a)].append(int(b))
    return out


def components(n, edges):
    """int32 [n]: the smallest node id of every node's strongly connected component (iterative Tarjan)."""
    succ = _lists(n, edges)
    index, low, on = [-1] * n, [0] * n, [False] * n
    comp = np.full((n,), -1, np.int32)
    stack, counter = [], 0
    for root in range(n):
        if index[root] >= 0:
            continue
        work = [(root, 0)]
        index[root] = low[root] = counter
        counter += 1
        stack.append(root)
        on[root] = True
        while work:
            v, i = work.pop()
            if i < len(succ[v]):
                work.append((v, i + 1))
                w = succ[v][i]
                if index[w] < 0:
                    index[w] = low[w] = counter
                    counter += 1
                    stack.append(w)
                    on[w] = True
                    work.append((w, 0))
                elif on[w]:
                    low[v] = min(low[v], index[w])
                continue
            if low[v] == index[v]:
                members = []
                while True:
                    w = stack.pop()
                    on[w] = False
                    members.append(w)
                    if w == v:
                        break
                comp[members] = min(members)
            if work:
                parent = work[-1][0]
                low[parent] = min(low[parent], low[v])
    return comp


def layers(n, edges, comp, direction):
    """int32 [n]: the longest-path layer of every node's component in the condensation, travelling ``"callees"`` (depth: 0 for a
    component nothing else points at) or ``"callers"`` (height).  Kahn's order over the components, then one pass."""
    comp = np.asarray(comp, np.int64)
    arcs = {(int(comp[a]), int(comp[b])) for a, b in edges if comp[a] != comp[b]}
    if direction == "callers":
        arcs = {(b, a) for a, b in arcs}
    labels = sorted(set(comp.tolist()))
    succ = {c: [] for c in labels}
    indeg = {c: 0 for c in labels}
    for a, b in sorted(arcs):
        succ[a].append(b)
        indeg[b] += 1
    ready = [c for c in labels if indeg[c] == 0]
    level = {c: 0 for c in labels}
    done = 0
    while ready:
        c = ready.pop()
        done += 1
        for d in succ[c]:
            level[d] = max(level[d], level[c] + 1)
            indeg[d] -= 1
            if indeg[d] == 0:
                ready.append(d)
    assert done == len(labels), "the condensation has a cycle: comp is no component labelling"
    return np.asarray([level[int(c)] for c in comp], np.int32).reshape(n)


def self_nodes(edges):
    return np.asarray(sorted({int(a) for a, b in edges if a == b}), np.int32)


def cyclic_bins(n, comp, loops=()):
    """int64 [n]: bins[c] = the size of component c when it has two nodes or more, or one node that carries a self-loop."""
    sizes = np.bincount(np.asarray(comp, np.int64), minlength=n).astype(np.int64) if n else np.zeros((0,), np.int64)
    loops = {int(v) for v in loops}
    keep = np.asarray([sizes[c] >= 2 or (sizes[c] == 1 and c in loops) for c in range(n)], bool).reshape(n)
    return np.where(keep, sizes, 0).astype(np.int64)


def top_components(bins, k):
    """[(label, size)]: the k largest cyclic components, ties to the lower label."""
    order = sorted((-int(s), c) for c, s in enumerate(bins) if s > 0)
    return [(c, -s) for s, c in order[:k]]


def scc_info(n, comp):
    sizes = np.bincount(np.asarray(comp, np.int64), minlength=n) if n else np.zeros((0,), np.int64)
    return [int((sizes > 0).sum()), int((sizes >= 2).sum()), int(sizes[sizes >= 2].sum())]


def node_words(mode, values, bins=None, lo=0, hi=0, q=0):
    """u64 [n]: 1 << q where the condition of crh_graph_node_words holds."""
    values = np.asarray(values, np.int64)
    n = len(values)
    if mode == "in_cycle":
        hit = np.asarray([0 <= x < n and bins[x] > 0 for x in values], bool).reshape(n)
    elif mode == "same_component":
        hit = values == lo
    else:
        hit = (values >= lo) & (values <= hi)
    return np.where(hit, np.uint64(1 << q), np.uint64(0)).astype(np.uint64)


# ---------------------------------------------------------------------------------------------------- graphs
def two_cycles_joined():
    """0 -> 1 -> 2 -> 0 and 3 -> 4 -> 3, joined one way by 2 -> 3."""
    return 5, [(0, 1), (1, 2), (2, 0), (3, 4), (4, 3), (2, 3)]


def figure_of_eight():
    """Two cycles that share node 2: ONE component."""
    return 5, [(2, 0), (0, 1), (1, 2), (2, 3), (3, 4), (4, 2)]


def complete(k):
    return k, [(a, b) for a in range(k) for b in range(k) if a != b]


def cycle_entered_above_its_minimum():
    """The cycle 2 -> 5 -> 3 -> 2 is entered at 5 (from 0 through 1) and left at 3 (to 4): its smallest id, 2, is no entry."""
    return 6, [(0, 1), (1, 5), (5, 3), (3, 2), (2, 5), (3, 4)]


def cycle_under_a_tail(tail=40):
    """The cycle {0, 1, 2} feeds a tail of ``tail`` nodes, the tail the cycle {3, 4}, and that the cycle {5, 6, 7}: the colour of
    the upstream cycle (the smallest id) floods everything below it, so a colouring finds one cycle per round -- three rounds,
    with the tail trimmed between the first and the second."""
    base = 8
    edges = [(0, 1), (1, 2), (2, 0), (3, 4), (4, 3), (5, 6), (6, 7), (7, 5)]
    edges += [(0, base)] + [(base + i, base + i + 1) for i in range(tail - 1)] + [(base + tail - 1, 3), (4, 5)]
    return base + tail, edges


def three_cyclic_layers():
    """A chain of three cyclic components with plain nodes between and beside them."""
    return 10, [(0, 1), (1, 0), (1, 2), (2, 3), (3, 4), (4, 3), (4, 5), (5, 6), (6, 7), (7, 5), (8, 3), (6, 9)]


def wide_lists(degree, inside):
    """A hub with ``degree`` callers and ``degree`` callees.  ``inside``: every caller is called back by a callee, so hub, callers
    and callees form one cycle; otherwise the hub lies on no cycle."""
    hub = 0
    callers = list(range(1, degree + 1))
    callees = list(range(degree + 1, 2 * degree + 1))
    edges = [(c, hub) for c in callers] + [(hub, c) for c in callees]
    if inside:
        edges += [(callees[i], callers[i]) for i in range(degree)]
    return 2 * degree + 3, edges + [(2 * degree + 1, callers[0]), (callees[-1], 2 * degree + 2)]


def planted(n, seed, sizes=(2, 3, 7, 70, 200), extra=3):
    """A random DAG over ``n`` nodes (edges from a lower to a higher position of a random order) with cycles planted over
    random node sets, and a few self-loops and repeats as a caller may hand them over."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(n)
    pairs = rng.integers(0, n, size=(extra * n, 2))
    edges = [(int(order[min(a, b)]), int(order[max(a, b)])) for a, b in pairs if a != b]
    free = rng.permutation(n).tolist()
    for size in sizes:
        members, free = free[:size], free[size:]
        edges += [(members[i], members[(i + 1) % size]) for i in range(size)]
    edges += [(int(v), int(v)) for v in rng.integers(0, n, size=5)] + edges[:7]
    return n, edges


def relabel(n, edges, seed):
    perm = np.random.default_rng(seed).permutation(n)
    return n, [(int(perm[a]), int(perm[b])) for a, b in edges], perm


# ---------------------------------------------------------------------------------------------------- the CPU tier's fake
class FakeSccGraph(gc.FakeGraph):
    """``graph_cases.FakeGraph`` plus the component and layer methods of ``ffi.Graph``, on the restatement above."""
    scc_calls = 0

    def scc(self, rel, stream=0):
        FakeSccGraph.scc_calls += 1
        comp = components(self.n_nodes, self.rel[rel])
        return comp, np.asarray(scc_info(self.n_nodes, comp) + [0], np.int64)

    def scc_bins(self, comp, self_nodes=None, stream=0):
        return cyclic_bins(self.n_nodes, comp, () if self_nodes is None else np.asarray(self_nodes).tolist())

    def layers(self, rel, direction, comp, stream=0):
        out = layers(self.n_nodes, self.rel[rel], comp, self._direction(direction))
        return out, np.asarray([int(out.max()) + 1 if self.n_nodes else 0, 0], np.int64)

    def node_words(self, mode, values, bins=None, lo=0, hi=0, q=0, out=None, stream=0):
        return node_words(mode, values, bins, lo, hi, q).view(np.int64)
