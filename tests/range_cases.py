"""Score threshold and in-range counts: the CPU restatement, the case generator and the fake index of the
CPU tier.  Test infrastructure only.

The restatement is the definition read aloud: ``oracle.search.scores`` -> mask -> ``>= thr`` (f32, inclusive) -> sort by
descending score, lower row first -> cut at ``k``; the count is the number of rows the comparison lets through, unclipped."""
import numpy as np

from oracle import search as orc
from tests.test_filter_sets_host import SetFakeIndex

MAX_K = 1024          # CRH_MAX_K
BLOCK = 500           # identical rows in the duplicate block of a corpus (fewer when the corpus is smaller)
KINDS = ("zero", "short", "full", "more", "huge")     # count 0, 0 < count < k, == k, > k, > CRH_MAX_K


def select(all_scores: np.ndarray, thr, k: int, passing=None, row_base: int = 0):
    """``all_scores`` [nq, n] f32 (``oracle.search.scores``), ``thr`` [nq] f32, ``passing`` bool [n] or None: ``(scores [nq, k]
    f32, rows [nq, k] i64, counts [nq] i64)``."""
    all_scores = np.asarray(all_scores, np.float32)
    nq, n = all_scores.shape
    thr = np.broadcast_to(np.asarray(thr, np.float32), (nq,))
    ok = np.ones((n,), bool) if passing is None else np.asarray(passing, bool)
    out_s, out_r = np.full((nq, k), -np.inf, np.float32), np.full((nq, k), -1, np.int64)
    counts = np.zeros((nq,), np.int64)
    for q in range(nq):
        rows = np.flatnonzero(ok & (all_scores[q] >= thr[q]))
        counts[q] = rows.size
        order = rows[np.lexsort((rows, -all_scores[q, rows].astype(np.float64)))][:k]      # (f32 -> f64 is exact: the order is the f32 order)
        out_s[q, :order.size], out_r[q, :order.size] = all_scores[q, order], order + row_base
    return out_s, out_r, counts


def kinds_of(counts, k: int) -> set:
    out = set()
    for c in np.asarray(counts).tolist():
        out.add("zero" if c == 0 else "short" if c < k else "full" if c == k else "more")
        if c > MAX_K:
            out.add("huge")
    return out


def corpus(n: int, dim: int, seed: int = 0):
    """Raw rows [n, dim] with one block of identical rows (``BLOCK`` of them, or a third of a small corpus) starting at an
    odd row in the middle -- it straddles tiles -- and two code columns (row % 7, row % 5): ``(raw, codes, (first, size))``."""
    rng = np.random.default_rng(1000 * seed + n + dim)
    raw = rng.standard_normal((n, dim), dtype=np.float32)
    size = min(BLOCK, n // 3)
    first = (n // 2) | 1
    first = min(first, n - size)
    raw[first:first + size] = raw[first]
    codes = np.stack([np.arange(n) % 7, np.arange(n) % 5], 1).astype(np.int32)
    return raw, codes, (first, size)


def batch(raw, block, nq: int, k: int, bf16: bool, passing=None, seed: int = 0):
    """``nq`` queries against the corpus with the thresholds of the issue mixed across them, query i taking kind i % 8:
      0  the exact canonical score of a stored row -- the k-th best passing one (inclusive: count >= k);
      1  nextafter of that score, up (that row is out: count < k);     2  nextafter of it, down;
      3  above the maximum (count 0);                                   4  -2.0 (every passing row);
      5  the duplicate block's score exactly (the whole block is in);   6  one ulp above it (the whole block is out: the block sits
         one ulp below the threshold);                                  7  the score of rank 3k (count > k).
    Returns ``(queries raw [nq, dim], thr f32 [nq], all_scores [nq, n], x_pre, want)`` with ``want`` = :func:`select` of it, and
    asserts ON THE ORACLE that the batch holds a query of every kind of ``KINDS`` the shape admits: all five from 16 queries and
    more than ``MAX_K`` passing rows on; what one query or a tiny corpus cannot hold is not asked of it."""
    n, dim = raw.shape
    rng = np.random.default_rng(77 + seed + nq)
    x_pre = orc.preprocess(raw, to_bf16=bf16)
    queries = rng.standard_normal((nq, dim), dtype=np.float32)
    queries[::3] += 0.5 * raw[block[0]]                       # (a third of the queries lean towards the block: it ranks high there)
    all_scores = orc.scores(x_pre, orc.preprocess(queries, to_bf16=bf16))
    ok = np.ones((n,), bool) if passing is None else np.asarray(passing, bool)
    live = int(ok.sum())
    thr = np.empty((nq,), np.float32)
    for q in range(nq):
        ranked = np.sort(all_scores[q, ok])[::-1]
        kth = ranked[min(k, live) - 1]
        kind = (q + seed) % 8
        thr[q] = (kth, np.nextafter(kth, np.float32(4)), np.nextafter(kth, np.float32(-4)), np.nextafter(ranked[0], np.float32(4)), np.float32(-2.0),
                  all_scores[q, block[0]], np.nextafter(all_scores[q, block[0]], np.float32(4)), ranked[min(3 * k, live) - 1])[kind]
    want = select(all_scores, thr, k, ok)
    need = set()
    if nq >= 16:
        need = {"zero", "full"} | ({"short"} if k > 1 else set()) | ({"more"} if live > 3 * k else set()) | ({"huge"} if live > MAX_K else set())
    got = kinds_of(want[2], k)
    assert need <= got, f"degenerate batch: kinds {sorted(got)} of {sorted(need)} (n={n} nq={nq} k={k})"
    return queries, thr, all_scores, x_pre, want


class RangeFakeIndex(SetFakeIndex):
    """``FakeIndex`` (+ set conditions) with ``search_range``: the restatement over the rows it holds."""
    range_calls: list = []

    def search_range(self, queries, k, thresholds, filters=None, row_base=0, counts=True, **kw):
        q = orc.preprocess(np.asarray(queries, np.float32).reshape(-1, self.dim), to_bf16=(self.dtype == 1))
        thr = np.broadcast_to(np.asarray(thresholds, np.float32), (len(q),))
        RangeFakeIndex.range_calls.append((len(q), int(k), bool(counts)))
        if len(self.x) == 0:
            return np.full((len(q), k), -np.inf, np.float32), np.full((len(q), k), -1, np.int64), (np.zeros((len(q),), np.int64) if counts else None)
        s, r, c = select(orc.scores(self.x, q), thr, k, self._mask(filters), row_base)
        return s, r, (c if counts else None)
