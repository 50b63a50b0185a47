"""Personalised PageRank's restatement and cases.  Test infrastructure only.

The restatement follows the definition in include/coderag_hip.h with plain Python loops over pull lists and numpy f32 vectors
over the queries, one ``astype(float32)`` per operation: no CSR arithmetic, no code shared with the product.  The device's
scores, bins, top lists and orderings are compared with it bit for bit."""
import numpy as np

from tests import graph_cases as gc

F32 = np.float32
MAX_STEPS = 64                                        # CRH_GRAPH_PPR_MAX_STEPS
NEG_INF = F32(-np.inf)


# ---------------------------------------------------------------------------------------------------- the restatement
def lists_of(n, off, adj):
    """node -> its list, from one CSR, in the CSR's order."""
    off, adj = np.asarray(off, np.int64), np.asarray(adj, np.int64)
    return [[int(v) for v in adj[int(off[u]):int(off[u + 1])]] for u in range(n)]


def pull_lists(fwd, rev, direction):
    """``(pull, out)``: node u's pull list and out(v), from the forward lists (a node's targets) and the reverse lists (its
    sources)."""
    n = len(fwd)
    if direction == "callees":                        # along the edges: a node pulls from its sources
        return [list(rev[u]) for u in range(n)], [len(fwd[v]) for v in range(n)]
    if direction == "callers":
        return [list(fwd[u]) for u in range(n)], [len(rev[v]) for v in range(n)]
    assert direction == "both"
    return [list(rev[u]) + list(fwd[u]) for u in range(n)], [len(fwd[v]) + len(rev[v]) for v in range(n)]


def graph_lists(n, edges):
    """``(fwd, rev)`` of an edge list, as ``gc.csr_pair`` lays the two CSRs out (ascending, repeats and self-loops dropped)."""
    off_f, adj_f, off_r, adj_r = gc.csr_pair(n, edges)
    return lists_of(n, off_f, adj_f), lists_of(n, off_r, adj_r)


def inverse_out(out):
    inv = np.zeros(len(out), F32)
    for v, d in enumerate(out):
        if d > 0:
            inv[v] = F32(1.0) / F32(d)
    return inv


def seed_vectors(n, seeds, weights=None, device_list=False):
    """p0 as f32 [n, nq].  ``seeds[q]`` is a list of nodes, ``weights[q]`` their weights (None: all 1).  ``device_list``: the
    kernel's clamp -- an entry that is no node is padding, a negative, NaN or infinite weight counts as +0."""
    nq = len(seeds)
    p0 = np.zeros((n, nq), F32)
    for q in range(nq):
        ws = [1.0] * len(seeds[q]) if weights is None else list(weights[q])
        assert len(ws) == len(seeds[q])
        total, per_node = F32(0.0), {}
        for v, w in zip(seeds[q], ws):
            v, w = int(v), F32(w)
            if device_list:
                if not 0 <= v < n:
                    v = -1
                if not (w > 0 and w < np.inf):
                    w = F32(0.0)
            else:
                assert -1 <= v < n and np.isfinite(w) and w >= 0
            if v == -1 or w == 0:
                continue
            per_node[v] = F32(per_node.get(v, F32(0.0)) + w)
            total = F32(total + w)
        if total > 0 and np.isfinite(total):
            for v, w in per_node.items():
                p0[v, q] = F32(w / total)
    return p0


def ppr(fwd, rev, direction, seeds, weights=None, restart=0.15, steps=16, device_list=False):
    """The scores, f32 [n, nq]."""
    n = len(fwd)
    pull, out = pull_lists(fwd, rev, direction)
    inv = inverse_out(out)
    p0 = seed_vectors(n, seeds, weights, device_list)
    nq = p0.shape[1]
    r = F32(restart)
    a = F32(F32(1.0) - r)
    base = (r * p0).astype(F32)                       # restart * p0[u]: the same product every step
    p = p0.copy()
    with np.errstate(under="ignore"):
        for _ in range(steps):
            contrib = (p * inv[:, None]).astype(F32)
            nxt = np.empty_like(p)
            for u in range(n):
                acc = np.zeros(nq, F32)
                for v in pull[u]:
                    acc = (acc + contrib[v]).astype(F32)
                nxt[u] = (base[u] + (a * acc).astype(F32)).astype(F32)
            p = nxt
    return p


def bins_of(scores, exclude=None):
    """int64 [nq, n]: the bit patterns, 0 for the nodes a query excludes."""
    scores = np.ascontiguousarray(scores, F32)
    bins = scores.T.copy().view(np.uint32).astype(np.int64)
    if exclude is not None:
        for q, row in enumerate(exclude):
            for v in row:
                if 0 <= int(v) < scores.shape[0]:
                    bins[q, int(v)] = 0
    return bins


def top_list(scores, k, exclude=None):
    """``(nodes int32 [nq, k], scores f32 [nq, k])``: positive scores descending, ties to the lower node, tail (-1, 0)."""
    n, nq = scores.shape
    nodes, vals = np.full((nq, k), -1, np.int32), np.zeros((nq, k), F32)
    for q in range(nq):
        out = {int(v) for v in (exclude[q] if exclude is not None else [])}
        ranked = sorted((-float(scores[v, q]), v) for v in range(n) if scores[v, q] > 0 and v not in out)
        for i, (_, v) in enumerate(ranked[:k]):
            nodes[q, i], vals[q, i] = v, scores[v, q]
    return nodes, vals


def order_lists(scores, rows, cosine, nodes):
    """``(fuse scores f32 [nq, 2, c], fuse rows int64 [nq, 2, c], graph_score f32 [nq, c])`` as crh_graph_ppr_order defines them."""
    rows, cosine, nodes = np.asarray(rows, np.int64), np.asarray(cosine, F32), np.asarray(nodes, np.int64)
    nq, c = rows.shape
    n = scores.shape[0]
    fs, fr, gs = np.full((nq, 2, c), NEG_INF, F32), np.full((nq, 2, c), -1, np.int64), np.zeros((nq, c), F32)
    for q in range(nq):
        fs[q, 0], fr[q, 0] = cosine[q], rows[q]
        for i in range(c):
            if rows[q, i] >= 0 and 0 <= nodes[q, i] < n and scores[nodes[q, i], q] > 0:
                gs[q, i] = scores[nodes[q, i], q]
        ranked = sorted((-float(gs[q, i]), i) for i in range(c) if gs[q, i] > 0)
        for at, (_, i) in enumerate(ranked):
            fs[q, 1, at], fr[q, 1, at] = gs[q, i], rows[q, i]
    return fs, fr, gs


def rrf_two(fuse_rows, k, rrf_k):
    """crh_fuse_select's RRF restated for the two lists of one query (int64 [2, c]): ``[(row, fused f32, first)]``, the first
    ``k`` distinct rows by descending fused score, ties to the lower row."""
    c = fuse_rows.shape[1]
    fused, first = {}, {}
    for j in range(2):
        for p in range(c):
            row = int(fuse_rows[j, p])
            if row < 0:
                continue
            fused[row] = F32(fused.get(row, F32(0.0)) + F32(1.0) / F32(rrf_k + p + 1))
            first.setdefault(row, j * c + p)
    ranked = sorted(fused, key=lambda row: (-float(fused[row]), row))
    return [(row, fused[row], first[row]) for row in ranked[:k]]


def propagated(fwd, rev, cand_scores, cand_rows, cand_nodes, limit, related_limit, direction="both", restart=0.15, steps=16,
               seed_weight="cosine", rrf_k=60):
    """``HipVectorStore.search_propagated`` restated from the candidate table of every query (cosines f32, GLOBAL rows, nodes;
    padding -inf / -1 / -1): per query ``(hits [(row, fused, cosine, graph_score)], related [(node, graph_score)])``."""
    cand_scores, cand_rows, cand_nodes = np.asarray(cand_scores, F32), np.asarray(cand_rows, np.int64), np.asarray(cand_nodes, np.int64)
    weights = np.maximum(cand_scores, F32(0.0)) if seed_weight == "cosine" else None
    scores = ppr(fwd, rev, direction, cand_nodes.tolist(), None if weights is None else weights.tolist(), restart, steps, device_list=True)
    _, fr, gs = order_lists(scores, cand_rows, cand_scores, cand_nodes)
    top_nodes, top_scores = top_list(scores, related_limit, cand_nodes.tolist()) if related_limit else (None, None)
    out = []
    for q in range(len(cand_rows)):
        hits = [(row, fused, cand_scores[q, first], gs[q, first]) for row, fused, first in rrf_two(fr[q], limit, rrf_k)]
        related = [(int(v), s) for v, s in zip(top_nodes[q], top_scores[q]) if v >= 0] if related_limit else []
        out.append((hits, related))
    return out


# ---------------------------------------------------------------------------------------------------- graphs
def ladder(rungs=16, sinks=300):
    """Rung i (node i) calls ``sinks`` shared sinks and rung i + 1: out-degree sinks + 1 each (the last rung: sinks).  Seeded at
    rung 0, the mass on rung i after i steps or more is about (a / (sinks + 1)) ** i: subnormal f32 at rung 15."""
    n = rungs + sinks
    edges = [(i, rungs + s) for i in range(rungs) for s in range(sinks)] + [(i, i + 1) for i in range(rungs - 1)]
    return n, edges


# ---------------------------------------------------------------------------------------------------- the CPU tier's fake
class FakeGraph(gc.FakeGraph):
    """``gc.FakeGraph`` with ``ffi.Graph``'s personalised PageRank on the restatement above; numpy arrays for device tensors."""
    ppr_calls = 0

    def ppr(self, rel, direction, seeds, weights=None, restart=0.15, steps=16, stream=0):
        assert 1 <= steps <= MAX_STEPS and 0 < restart < 1
        device_list = isinstance(seeds, np.ndarray)
        seeds = [list(s) for s in (seeds.tolist() if device_list else seeds)]
        if weights is not None:
            weights = [list(w) for w in (weights.tolist() if isinstance(weights, np.ndarray) else weights)]
        assert 1 <= len(seeds) <= 64
        FakeGraph.ppr_calls += 1
        fwd, rev = graph_lists(self.n_nodes, self.rel[rel])
        self.ppr_scores = ppr(fwd, rev, self._direction(direction), seeds, weights, restart, steps, device_list)
        return self.ppr_scores

    def ppr_top(self, k, exclude=None, stream=0):
        return top_list(self.ppr_scores, int(k), exclude)

    def ppr_order(self, rows, cosine, nodes, stream=0):
        return order_lists(self.ppr_scores, rows, cosine, nodes)
