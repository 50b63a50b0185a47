"""CPU restatement of recommend-by-example (``crh_recommend_query`` / ``crh_recommend_select``), the brute-force
definition of the answers a store must give, and the inputs the tests of both tiers share.  Test infrastructure only -- the
checker of both tiers.  Everything that scores uses the oracle's own sequential preprocess and dot (``oracle.search``).

A logical query is ``P`` positive and ``N`` negative examples, each a STORED row (as ``read_rows`` / ``gather_vectors`` return
it); its slots are ``[P positives | N negatives]`` of which the first ``n_pos`` / ``n_neg`` of each part are live.

* ``average``: ``q[i] = (ap + ap) - an``, ``ap = sp / (float)n_pos``, ``an = sn / (float)n_neg``, ``sp`` / ``sn`` = ``+0.0f`` plus
  the live examples' elements in ascending slot order, every operation rounded to f32; ``n_neg = 0``: ``q[i] = ap``.  The answer
  is the plain exact top-``limit`` for ``q`` with the example rows removed.
* ``best``: ``s(e, x)`` = the score a search gives row ``x`` for the raw query ``e`` (``orc.preprocess`` then ``orc_dot``);
  ``p(x) = max_j s(pos_j, x)`` (``best`` = the lowest ``j`` attaining it), ``n(x) = max_j s(neg_j, x)`` (-inf without negatives);
  a NaN ``s(e, x)`` -- the example holds a NaN or an infinity -- is no score and stands as -inf in both maxima;
  KEPT iff no example row and ``ord(p) > ord(n)``; the answer is the first ``limit`` kept rows by descending ``p``, ties to the
  lower row.
* the selection from lists: list ``j`` is the exact top-``c`` of positive ``j``; the first flat entry of a row stands for it;
  ``T`` = the largest last score over the lists whose ``c`` entries are all real; the kept rows with ``ord(p) > ord(T)`` are
  SETTLED (all of them without a full list).  ``info = (kept, settled, distinct, vetoed = distinct - kept)``; the tail of the
  outputs is ``(-1, -inf, -inf, -1)``.
"""
import numpy as np

from oracle import search as orc
from tests.fuse_cases import ord_f32, unord_f32

F32, U32 = np.float32, np.uint32
STRATEGIES = ("average", "best")
MAX_POS, MAX_NEG, MAX_K = 8, 8, 1024
NEG_INF_ORD = int(ord_f32(F32(-np.inf))[()])


def _counts(n_pos, n_neg, nq, P, N):
    n_pos = np.full((nq,), P, np.int32) if n_pos is None else np.asarray(n_pos, np.int32).reshape(nq)
    n_neg = np.full((nq,), N, np.int32) if n_neg is None else np.asarray(n_neg, np.int32).reshape(nq)
    assert ((n_pos >= 1) & (n_pos <= P) & (n_neg >= 0) & (n_neg <= N)).all()
    return n_pos, n_neg


def recommend_query(examples, P, N, n_pos=None, n_neg=None, **_):
    """The call shape of ``ffi.recommend_query`` on host arrays: ``examples`` [nq, P + N, dim] -> [nq, dim]."""
    ex = np.asarray(examples, F32)
    P, N = int(P), int(N)
    nq, dim = ex.shape[0], ex.shape[2]
    assert ex.shape[1] == P + N and 1 <= P <= MAX_POS and 0 <= N <= MAX_NEG
    n_pos, n_neg = _counts(n_pos, n_neg, nq, P, N)
    out = np.empty((nq, dim), F32)
    for q in range(nq):
        sp, sn = np.zeros((dim,), F32), np.zeros((dim,), F32)
        for j in range(n_pos[q]):
            sp = (sp + ex[q, j]).astype(F32)                             # one rounded f32 addition per element
        for j in range(n_neg[q]):
            sn = (sn + ex[q, P + j]).astype(F32)
        ap = (sp / F32(n_pos[q])).astype(F32)
        out[q] = ap if n_neg[q] == 0 else ((ap + ap).astype(F32) - (sn / F32(n_neg[q])).astype(F32)).astype(F32)
    return out


def example_scores(examples_raw, vecs, bf16=False):
    """``s(e, x)`` of every (example, row) pair: [ne, n] f32."""
    return orc.scores(vecs, orc.preprocess(np.asarray(examples_raw, F32), to_bf16=bool(bf16)))


def recommend_select(scores, rows, cand_vecs, examples, example_rows, P, N, k, strategy="best", bf16=False, n_pos=None, n_neg=None, **_):
    """The call shape of ``ffi.recommend_select`` on host arrays -> (rows i64, score f32, neg f32, best i32) each [nq, k] and
    info i32 [nq, 4]."""
    strategy = strategy.lower()
    assert strategy in STRATEGIES
    P, N, k = int(P), int(N), int(k)
    best = strategy == "best"
    m = P if best else 1
    scores, rows = np.asarray(scores, F32), np.asarray(rows, np.int64)
    example_rows = np.asarray(example_rows, np.int64)
    nq, c = scores.shape[0], scores.shape[2]
    assert scores.shape == rows.shape == (nq, m, c) and example_rows.shape == (nq, P + N)
    assert 1 <= P <= MAX_POS and 0 <= N <= MAX_NEG and c >= 1 and m * c <= MAX_K and 1 <= k <= m * c
    n_pos, n_neg = _counts(n_pos, n_neg, nq, P, N)
    out = (np.full((nq, k), -1, np.int64), np.full((nq, k), -np.inf, F32), np.full((nq, k), -np.inf, F32), np.full((nq, k), -1, np.int32),
           np.zeros((nq, 4), np.int32))
    for q in range(nq):
        flat_r, flat_s = rows[q].reshape(-1), scores[q].reshape(-1)
        real = np.flatnonzero(flat_r >= 0)
        uniq, first = np.unique(flat_r[real], return_index=True)         # (the first occurrence of every row)
        first = real[first]
        d = uniq.size
        if best and d:
            live = list(range(n_pos[q])) + list(range(P, P + n_neg[q]))
            s = example_scores(np.asarray(examples, F32)[q, live], np.asarray(cand_vecs, F32)[q, first], bf16)
            s = np.where(np.isnan(s), F32(-np.inf), s)                  # a NaN score is no score: that example neither wins nor vetoes
            so = ord_f32(s).astype(np.int64)
            p_ord, which = so[:n_pos[q]].max(0), so[:n_pos[q]].argmax(0).astype(np.int32)       # (argmax: the first maximum)
            n_ord = so[n_pos[q]:].max(0) if n_neg[q] else np.full((d,), NEG_INF_ORD, np.int64)
            kept = ~np.isin(uniq, example_rows[q]) & (p_ord > n_ord)
            order = np.lexsort((uniq, -p_ord))
        else:
            p_ord = ord_f32(flat_s[first]).astype(np.int64)
            which, n_ord = np.full((d,), -1, np.int32), np.full((d,), NEG_INF_ORD, np.int64)
            kept = ~np.isin(uniq, example_rows[q])
            order = np.argsort(first, kind="stable")                     # AVERAGE keeps the list's own order
        t_ord = 0
        if best:
            for j in range(m):
                if rows[q, j, c - 1] >= 0:
                    t_ord = max(t_ord, int(ord_f32(scores[q, j, c - 1])[()]))
        order = order[kept[order]]
        nk = int(kept.sum())
        out[4][q] = (nk, int((p_ord[kept] > t_ord).sum()) if best else nk, d, d - nk)
        order = order[:k]
        w = order.size
        out[0][q, :w], out[3][q, :w] = uniq[order], which[order]
        out[1][q, :w] = flat_s[first[order]] if not best else unord_f32(p_ord[order].astype(U32))
        out[2][q, :w] = unord_f32(n_ord[order].astype(U32))
    return out


def brute_force(stored, pos, neg, limit, strategy, bf16=False, passing=None):
    """The definition itself for one logical query over the whole collection: ``stored`` [n, dim] the preprocessed rows in the
    order ties follow, ``pos`` / ``neg`` indexes into it, ``passing`` [n] the rows that are alive and pass the filter.  Every
    score comes from ``oracle.search`` with ``k`` = all rows.  Returns [(row, score bits, neg bits, best)]; under "average" the
    last two are ``(-inf bits, -1)``."""
    stored = np.asarray(stored, F32)
    n = stored.shape[0]
    alive = None if passing is None else np.asarray(passing, np.uint8)
    pos, neg = [int(v) for v in pos], [int(v) for v in neg]
    ninf = int(F32(-np.inf).view(U32))
    if strategy == "average":
        ex = stored[pos + neg][None]
        q = recommend_query(ex, len(pos), len(neg))
        s, r = orc.search(stored, orc.preprocess(q, to_bf16=bool(bf16)), min(n, limit + len(pos) + len(neg)), alive=alive)
        keep = (r[0] >= 0) & ~np.isin(r[0], pos + neg)
        return [(int(row), int(sc.view(U32)), ninf, -1) for row, sc in zip(r[0][keep][:limit], s[0][keep][:limit])]
    s, r = orc.search(stored, orc.preprocess(stored[pos + neg], to_bf16=bool(bf16)), n, alive=alive)
    mat = np.zeros((len(pos) + len(neg), n), np.int64)                   # ord images; 0 = the row does not pass
    for j in range(mat.shape[0]):
        real = r[j] >= 0
        mat[j, r[j][real]] = ord_f32(s[j][real])
    p_ord, which = mat[:len(pos)].max(0), mat[:len(pos)].argmax(0)
    n_ord = mat[len(pos):].max(0) if neg else np.full((n,), NEG_INF_ORD, np.int64)
    n_ord = np.maximum(n_ord, NEG_INF_ORD)
    kept = (p_ord > 0) & (p_ord > n_ord)
    kept[pos + neg] = False
    rows = np.flatnonzero(kept)
    order = rows[np.lexsort((rows, -p_ord[rows]))][:limit]
    return [(int(row), int(unord_f32(U32(p_ord[row])).view(U32)), int(unord_f32(U32(n_ord[row])).view(U32)), int(which[row])) for row in order]


def corpus(n=400, dim=384, seed=3, clusters=8, dups=20, spread=0.5):
    """A seeded clustered corpus of ``n`` raw rows of which the last ``dups`` are exact copies of the first ones (equal scores:
    ties).  Returns (raw rows [n, dim], cluster of every row [n])."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((clusters, dim)).astype(F32)
    which = rng.integers(0, clusters, n)
    raw = (centres[which] + F32(spread) * rng.standard_normal((n, dim)).astype(F32)).astype(F32)
    raw[n - dups:], which[n - dups:] = raw[:dups], which[:dups]
    return raw, which


def case(nq, P, N, c, dim, seed, bf16=False, ragged=True, n_rows=400):
    """Inputs of both kernels for ``nq`` logical queries, made with the oracle's own search over a clustered corpus of ``n_rows``
    stored rows (20 of them exact copies): real top-``c`` lists of every positive (odd queries under a mask that leaves about a
    quarter of the rows: their deeper lists end in padding), lists that share rows (positives of one cluster), every third query
    with negative 0 ON positive 0 (``p == n`` exactly for the rows that positive wins), ragged live counts whose dead lists are
    all padding, unused example slots -1, shard bits above 2^32 on some queries' rows.  Returns a dict of host arrays."""
    rng = np.random.default_rng(seed)
    raw, _ = corpus(n_rows, dim, seed)
    x = orc.preprocess(raw, to_bf16=bool(bf16))
    E = P + N
    ex_idx = rng.integers(0, n_rows, (nq, E))
    if N:
        ex_idx[::3, P] = ex_idx[::3, 0]
    n_pos, n_neg = rng.integers(1, P + 1, nq).astype(np.int32), rng.integers(0, N + 1, nq).astype(np.int32)
    if not ragged:
        n_pos[:], n_neg[:] = P, N
    n_pos[::4], n_neg[::4] = P, N
    examples = np.ascontiguousarray(x[ex_idx])                            # stored rows, as gather_vectors returns them
    few = (rng.random(n_rows) < 0.25).astype(np.uint8)
    scores, rows = np.full((nq, P, c), -np.inf, F32), np.full((nq, P, c), -1, np.int64)
    avg_s, avg_r = np.full((nq, 1, c), -np.inf, F32), np.full((nq, 1, c), -1, np.int64)
    avg_q = recommend_query(examples, P, N, n_pos, n_neg)
    if nq:
        pre = orc.preprocess(examples[:, :P].reshape(nq * P, dim), to_bf16=bool(bf16))
        apre = orc.preprocess(avg_q, to_bf16=bool(bf16))
        for part, alive in ((slice(0, None, 2), None), (slice(1, None, 2), few)):
            sel = np.arange(nq)[part]
            if sel.size:
                flat = (sel[:, None] * P + np.arange(P)[None, :]).reshape(-1)
                s, r = orc.search(x, pre[flat], c, alive=alive)
                scores[sel], rows[sel] = s.reshape(-1, P, c), r.reshape(-1, P, c)
                s, r = orc.search(x, apre[sel], c, alive=alive)
                avg_s[sel, 0], avg_r[sel, 0] = s, r
    dead = np.arange(P)[None, :] >= n_pos[:, None]
    scores[dead], rows[dead] = -np.inf, -1
    cand = x[np.maximum(rows, 0)].reshape(nq, P * c, dim)
    cand[(rows < 0).reshape(nq, P * c)] = 0
    shift = (rng.integers(0, 3, (nq, 1)) << 32).astype(np.int64)
    ex_rows = ex_idx + shift
    ex_rows[:, :P][dead] = -1
    ex_rows[:, P:][np.arange(N)[None, :] >= n_neg[:, None]] = -1
    rows = np.where(rows >= 0, rows + shift[:, :, None], -1)
    avg_r = np.where(avg_r >= 0, avg_r + shift[:, :, None], -1)
    return {"scores": np.ascontiguousarray(scores), "rows": np.ascontiguousarray(rows), "cand_vecs": np.ascontiguousarray(cand),
            "examples": examples, "example_rows": np.ascontiguousarray(ex_rows), "n_pos": n_pos, "n_neg": n_neg, "avg_query": avg_q,
            "avg_scores": np.ascontiguousarray(avg_s), "avg_rows": np.ascontiguousarray(avg_r), "stored": x, "bf16": bool(bf16)}


# ------------------------------------------------------------------ end to end: the inputs and the rounds a store runs
def e2e_inputs(dim=384, n=3000):
    """The collection and the example sets of the end-to-end tests: ``n`` clustered raw rows (12 centres; rows ``i < 60`` have
    exact copies at ``n - 60 + i``) and two batches ``(limit, [(positive rows, negative rows)])``.  Batch A (limit 10): plain
    sets, a row and its copy both positive (ties between positives), eight negatives from the lone positive's own cluster
    (about one near row in nine survives: round 2), and a positive whose copy is the negative (``p == n`` everywhere: nothing
    is ever settled, the answer is short and empty).  Batch B (limit 200): the eight-negatives set again (two rounds cannot
    settle 200 rows: a short, non-empty answer) and a plain set."""
    raw, which = corpus(n, dim, seed=21, clusters=12, dups=60)
    rng = np.random.default_rng(2)
    mid = np.arange(60, n - 60)

    def of(cluster, count):
        return rng.choice(mid[which[mid] == cluster], count, replace=False).tolist()
    own = of(int(which[1000]), 9)
    own = [r for r in own if r != 1000][:8]
    a = (10, [([100, 101, 102], []), ([200], [300, 301]), (of(1, 2) + of(2, 1), of(3, 2)), ([5], [n - 60 + 5]), ([1000], own),
              (rng.choice(mid, 8, replace=False).tolist(), rng.choice(mid, 8, replace=False).tolist()), ([7, n - 60 + 7], [400]), ([500, 501], [])])
    b = (200, [([1000], own), ([600, 601], [])])
    return raw, [a, b]


def rounds(stored, pos, neg, limit, bf16=False, passing=None, candidates=None, batch_p=None):
    """What ``_Collection.recommend`` does for one "best" query, with the oracle's own lists and the restatement: (answer as
    :func:`brute_force` returns it, went to round 2, came back short).  ``batch_p``: the largest positive count of the batch
    the query travels in (the depths of both rounds go by it)."""
    stored = np.asarray(stored, F32)
    P, N = len(pos), len(neg)
    alive = None if passing is None else np.asarray(passing, np.uint8)
    deep = MAX_K // (batch_p or P)
    c1 = max(1, min(deep, 4 * limit)) if candidates is None else candidates
    pre = orc.preprocess(stored[list(pos)], to_bf16=bool(bf16))
    round2 = False
    for c in (c1, deep):
        s, r = orc.search(stored, pre, c, alive=alive)
        k = min(limit, P * c)
        rows, score, nscore, best, info = (v[0] for v in recommend_select(s[None], r[None], stored[np.maximum(r, 0).reshape(-1)][None],
                                                                         stored[list(pos) + list(neg)][None], np.asarray([list(pos) + list(neg)]),
                                                                         P, N, k, "best", bf16))
        full = bool((r[:, -1] >= 0).any())
        done = info[1] >= limit or not full
        if done or c == deep:
            break
        round2 = True
    w = int(min(info[1], k))
    ans = [(int(a), int(b), int(d), int(e)) for a, b, d, e in zip(rows[:w], score[:w].view(U32), nscore[:w].view(U32), best[:w])]
    return ans, round2, not done
