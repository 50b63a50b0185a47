"""CPU restatement of the multi-query fusion (``crh_fuse_select``), the brute-force definition of the best-match
search it serves, and the inputs the tests of both tiers share.  Test infrastructure only -- the checker of both tiers.

The definition, per logical query: ``m`` lists of ``c`` entries ``(score f32, row i64)`` as ``crh_search`` / ``crh_merge_topk*``
return them (scores descending, padding ``(-inf, -1)`` at the end of a list).  Entry ``(j, p)`` has flat index ``u = j * c + p``.
Padding takes no part.

* contribution of ``(j, p)``: RRF ``w_j / (float)(rrf_k + p + 1)`` -- ONE f32 division, correctly rounded, ``w_j`` f32 (default
  1), ``rrf_k`` an int >= 0 (default 60); MAX the entry's score.
* fused score of a row: RRF ``+0.0f`` plus the contributions of all entries with that row in ascending ``u``, every addition
  rounded to f32 (no FMA); MAX the largest contribution under the order below.
* with it: ``cos`` the largest score among its entries (same order), ``lists`` bit ``j`` set when list ``j`` holds it,
  ``first`` its smallest ``u``.
* order: descending fused score compared through the order-preserving integer image of f32 (``ord``; ``-0.0 < +0.0``), ties to
  the lower row.
* output: the first ``k`` distinct rows -- row, fused, cos, lists, first; the tail is ``(-1, -inf, -inf, 0, -1)``;
  ``info = (distinct rows, real entries)``.
"""
import numpy as np

from oracle import search as orc

F32, U32 = np.float32, np.uint32
METHODS = ("rrf", "max")
MAX_LISTS, MAX_K = 16, 1024


def ord_f32(x) -> np.ndarray:
    """The order-preserving map f32 -> u32 of the selection kernels (larger float <=> larger integer; -0.0 < +0.0)."""
    a = np.asarray(x, dtype=F32)
    u = a.reshape(-1).view(U32).reshape(a.shape)
    return np.where(u & U32(0x80000000), ~u, u | U32(0x80000000)).astype(U32)


def unord_f32(o) -> np.ndarray:
    o = np.asarray(o, dtype=U32)
    return np.where(o & U32(0x80000000), o & U32(0x7fffffff), ~o).astype(U32).reshape(-1).view(F32).reshape(o.shape)


def contribution(w, rrf_k: int, p) -> np.ndarray:
    """``w / (float)(rrf_k + p + 1)`` in f32: numpy's f32 division is the correctly rounded one."""
    return (np.asarray(w, F32) / (np.asarray(p, np.int64) + int(rrf_k) + 1).astype(F32)).astype(F32)


def fuse_select_one(scores: np.ndarray, rows: np.ndarray, k: int, method: str = "rrf", rrf_k: int = 60, weights=None):
    """One logical query, ``scores`` / ``rows`` [m, c]: (rows i64 [k], fused f32 [k], cos f32 [k], lists i32 [k], first i32 [k],
    info i32 [2]).  The walk itself, entry by entry in ascending ``u``."""
    m, c = scores.shape
    assert method in METHODS and 1 <= m <= MAX_LISTS and c >= 1 and m * c <= MAX_K and 1 <= k <= m * c and rrf_k >= 0
    w = np.ones((m,), F32) if weights is None else np.asarray(weights, F32)
    assert w.shape == (m,) and np.isfinite(w).all() and (w >= 0).all() and (weights is None or method == "rrf")
    scores, rows = np.asarray(scores, F32), np.asarray(rows, np.int64)
    state: dict[int, list] = {}                      # row -> [fused f32, cos ord, lists, first]
    nreal = 0
    for j in range(m):
        for p in range(c):
            r = int(rows[j, p])
            if r < 0:
                continue
            nreal += 1
            so = int(ord_f32(scores[j, p])[()])
            st = state.setdefault(r, [F32(0.0), 0, 0, j * c + p])
            if method == "rrf":
                st[0] = F32(st[0] + contribution(w[j], rrf_k, p)[()])           # one rounded f32 addition
            st[1] = max(st[1], so)
            st[2] |= 1 << j
    if method == "max":
        for st in state.values():
            st[0] = unord_f32(st[1])[()]
    order = sorted(state, key=lambda r: (-int(ord_f32(state[r][0])[()]), r))[:k]
    out = (np.full((k,), -1, np.int64), np.full((k,), -np.inf, F32), np.full((k,), -np.inf, F32), np.zeros((k,), np.int32),
           np.full((k,), -1, np.int32))
    for i, r in enumerate(order):
        st = state[r]
        out[0][i], out[1][i], out[2][i], out[3][i], out[4][i] = r, st[0], unord_f32(st[1])[()], st[2], st[3]
    return out + (np.asarray([len(state), nreal], np.int32),)


def _fuse_fast(scores: np.ndarray, rows: np.ndarray, k: int, method: str, rrf_k: int, w: np.ndarray):
    """:func:`fuse_select_one` list by list instead of entry by entry -- the same additions in the same order as long as no
    list names a row twice (the caller checks), which is what lets the sweeps of the GPU tier run in seconds."""
    m, c = scores.shape
    real = rows >= 0
    uniq, inv = np.unique(rows[real], return_inverse=True)
    where = np.full(rows.shape, -1, np.int64)
    where[real] = inv
    d = uniq.size
    fused, cos, lists, first = np.zeros((d,), F32), np.zeros((d,), U32), np.zeros((d,), np.int32), np.full((d,), m * c, np.int32)
    for j in range(m):
        p = np.flatnonzero(real[j])
        at = where[j, p]
        if method == "rrf":
            fused[at] = fused[at] + contribution(w[j], rrf_k, p)
        cos[at] = np.maximum(cos[at], ord_f32(scores[j, p]))
        lists[at] |= np.int32(1 << j)
        first[at] = np.minimum(first[at], (j * c + p).astype(np.int32))
    if method == "max":
        fused = unord_f32(cos)
    order = np.lexsort((uniq, U32(0xffffffff) - ord_f32(fused)))[:k]
    out = (np.full((k,), -1, np.int64), np.full((k,), -np.inf, F32), np.full((k,), -np.inf, F32), np.zeros((k,), np.int32),
           np.full((k,), -1, np.int32))
    n = order.size
    out[0][:n], out[1][:n], out[2][:n], out[3][:n], out[4][:n] = uniq[order], fused[order], unord_f32(cos[order]), lists[order], first[order]
    return out + (np.asarray([d, int(real.sum())], np.int32),)


def fuse_select(scores, rows, m, k, method="rrf", rrf_k=60, weights=None, **_):
    """The restatement with the call shape of ``ffi.fuse_select`` on host arrays: ``[nq * m, c]`` or ``[nq, m, c]`` ->
    (rows, fused, cos, lists, first) each [nq, k] and info [nq, 2]."""
    scores, rows = np.asarray(scores, F32), np.asarray(rows, np.int64)
    m, k = int(m), int(k)
    c = scores.shape[-1]
    scores, rows = scores.reshape(-1, m, c), rows.reshape(-1, m, c)
    nq = scores.shape[0]
    method = method.lower()
    assert method in METHODS and 1 <= m <= MAX_LISTS and m * c <= MAX_K and 1 <= k <= m * c and rrf_k >= 0
    assert weights is None or method == "rrf"
    w = np.ones((m,), F32) if weights is None else np.asarray(weights, F32)
    outs = (np.full((nq, k), -1, np.int64), np.full((nq, k), -np.inf, F32), np.full((nq, k), -np.inf, F32), np.zeros((nq, k), np.int32),
            np.full((nq, k), -1, np.int32), np.zeros((nq, 2), np.int32))
    for q in range(nq):
        srt = np.sort(rows[q], axis=1)
        twice = ((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)).any()
        one = fuse_select_one(scores[q], rows[q], k, method, rrf_k, weights) if twice else _fuse_fast(scores[q], rows[q], k, method, rrf_k, w)
        for o, v in zip(outs, one):
            o[q] = v
    return outs


def brute_force_max(corpus_pre: np.ndarray, queries_pre: np.ndarray, limit: int, passing=None):
    """The best-match definition itself for one logical query: the oracle's score of EVERY passing row under each of the ``m``
    sub-queries (``k = n``), the largest of them per row (``ord`` order), the first ``limit`` rows by descending value, ties to
    the lower row.  Returns (fused f32 [<= limit], rows i64 [<= limit])."""
    n = corpus_pre.shape[0]
    alive = None if passing is None else np.asarray(passing, np.uint8)
    s, r = orc.search(corpus_pre, np.atleast_2d(np.asarray(queries_pre, F32)), n, alive=alive)
    best = np.zeros((n,), U32)
    for j in range(s.shape[0]):
        real = r[j] >= 0
        best[r[j][real]] = np.maximum(best[r[j][real]], ord_f32(s[j][real]))
    rows = np.flatnonzero(best > 0)
    order = np.lexsort((rows, U32(0xffffffff) - best[rows]))[:limit]
    return unord_f32(best[rows[order]]), rows[order].astype(np.int64)


def oracle_lists(corpus_pre: np.ndarray, queries_pre: np.ndarray, c: int, passing=None):
    """The ``m`` candidate lists of one logical query as the oracle returns them: (scores [m, c], rows [m, c])."""
    alive = None if passing is None else np.asarray(passing, np.uint8)
    return orc.search(corpus_pre, np.atleast_2d(np.asarray(queries_pre, F32)), c, alive=alive)


def expected(stored: np.ndarray, gid: np.ndarray, queries_pre: np.ndarray, limit: int, candidates: int, method: str, rrf_k: int = 60,
             weights=None, passing=None):
    """What a store must answer for one logical query: the restatement applied to the oracle's own top-``candidates`` lists.
    ``stored`` [n, dim]: the preprocessed rows in slot order, ``gid`` [n] their GLOBAL rows (the order ties follow),
    ``passing`` [n] the rows that are alive and pass the filter.  Returns [(slot, fused bits, cos bits, matched)]."""
    order = np.argsort(gid)
    pas = None if passing is None else np.asarray(passing, bool)[order]
    s, r = oracle_lists(stored[order], queries_pre, candidates, pas)
    rows, fused, cos, bits, _, _ = fuse_select(s[None], r[None], s.shape[0], limit, method, rrf_k, weights)
    return [(int(order[row]), int(f.view(U32)), int(cv.view(U32)), [j for j in range(MAX_LISTS) if b >> j & 1])
            for row, f, cv, b in zip(rows[0], fused[0], cos[0], bits[0].tolist()) if row >= 0]


def lists(nq: int, m: int, c: int, mode: str, seed: int):
    """``nq`` sets of ``m`` candidate lists of ``c`` entries, [nq, m, c]: scores descending with runs of equal values, rows
    distinct inside a list (shard bits above 2^32 on some), padded tails of random length and every fifth query all padding.
    ``mode``: "disjoint" (no row in two lists), "identical" (every list the same), "overlap" (rows drawn from a pool of 1.5 c),
    "mixed" (a pool of 4 c)."""
    rng = np.random.default_rng(seed)
    shape = (nq, m, c)
    scores = unord_f32(-np.sort(-ord_f32(np.round(rng.standard_normal(shape), 1)).astype(np.int64), axis=2))   # (+0.0 ahead of -0.0: both occur)
    if mode == "disjoint":
        rows = rng.permuted(np.tile(np.arange(m * c, dtype=np.int64), (nq, 1)), axis=1).reshape(shape)
    else:
        pool = {"identical": 2 * c, "overlap": c + (c + 1) // 2, "mixed": 4 * c}[mode]
        rows = rng.permuted(np.tile(np.arange(pool, dtype=np.int64), (nq * m, 1)), axis=1)[:, :c].reshape(shape)
    rows = rows + (rng.integers(0, 3, (nq, 1, 1)) << 32)
    for lst_s, lst_r in zip(scores.reshape(-1, c), rows.reshape(-1, c)):     # equal scores: the lower row first, as a search returns them
        lst_r[:] = lst_r[np.lexsort((lst_r, -ord_f32(lst_s).astype(np.int64)))]
    if mode == "identical":
        scores, rows = np.repeat(scores[:, :1], m, axis=1), np.repeat(rows[:, :1], m, axis=1)
    real = rng.integers(0, c + 1, (nq, m))
    real[::3] = c                                                     # (full lists too)
    if mode == "identical":
        real[:] = real[:, :1]
    if nq >= 5:
        real[4::5] = 0
    pad = np.arange(c)[None, None, :] >= real[:, :, None]
    scores[pad], rows[pad] = -np.inf, -1
    return np.ascontiguousarray(scores), np.ascontiguousarray(rows)


def corpus(n: int = 900, dim: int = 384, seed: int = 7, dups: int = 60):
    """A seeded corpus of ``n`` raw rows of which the last ``dups`` are exact copies of earlier ones (equal scores: ties in every
    order), and three sets of raw sub-queries: four random ones, three ON stored rows (two of them a duplicated pair's), one
    alone.  Returns (raw rows [n, dim], [queries [m_i, dim]])."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n - dups, dim)).astype(F32)
    src = rng.choice(n - dups, dups, replace=False)
    x = np.concatenate([x, x[src]])
    sets = [rng.standard_normal((4, dim)).astype(F32), np.stack([x[src[0]], x[src[1]], x[5]]), rng.standard_normal((1, dim)).astype(F32)]
    return x, sets
