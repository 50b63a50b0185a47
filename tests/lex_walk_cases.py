"""Constructed inputs for the exact BM25 keyword search (``crh_lex.hip``: ``k_lex_walk<HIST|APPEND|DF>``, ``k_lex_cut``,
``k_lex_select``, ``crh_lex_stats``, ``crh_lex_search``): full term tables, probe chains that wrap, tile walks
with their step and iteration edges, and histogram cuts steered into chosen buckets.  Test infrastructure only, no GPU import.

Every builder returns plain CSR arrays (``row_off``, ``terms``, ``tf``, ``dl``), per call the query and idf lists, the mask as
validity words, ``k`` and ``row_base``.  The expected ``(scores, rows, counts)`` come from two independent sources:

(a) :func:`expected` -- the restatement ``lex_cases.bm25_search``;
(b) :func:`closed_form` -- for calls with ``k1 = 0`` and ``b = 0``: the kernel's ``norm`` is 0 and ``c * 1 / (c + 0)`` is 1
    exactly, so a row's score is the f32 sum of the idf values of the query terms it holds, added in ascending id.  Computed
    here in rational arithmetic with one rounding to f32 per addition (for the cut families no addition rounds at all: the idf
    values are powers of two within 24 significant bits), and selected by the integer image of the score, not by a float sort.

The module also restates ``lex_slot`` and ``LexTable::build`` (:func:`lex_slot`, :func:`pass_keys`, :func:`build_table`,
:func:`probe`) and ``k_lex_cut`` (:func:`cut_model`), which tests/test_lex_walk_cases_host.py uses to prove that every case
is the case it claims to be.  The constants below are compared with the text of ``crh_lex.hip`` there."""
import functools
from fractions import Fraction
from types import SimpleNamespace as NS

import numpy as np

from tests import lex_cases as lc

U32 = np.uint32
f32 = np.float32

PASS_Q = 64            # kLexPassQ
MAX_KEYS = 2048        # kLexMaxKeys = kLexPassQ * CRH_LEX_MAX_QUERY_TERMS
BUCKETS = 65536        # kLexBuckets
STEPS = 4              # kLexSteps
WAVES = 4              # kLexWaves
MULT = 2654435761      # lex_slot's multiplier
MAX_K = 1024           # CRH_MAX_K
K1, B = 1.2, 0.75

MAX_ROWS, MAX_ENTRIES, MAX_NQ = 6000, 400_000, 130      # the sizes every case stays under


# ------------------------------------------------------------------ the host side of a pass, restated

def lex_slot(term: int, log2_slots: int) -> int:
    return ((int(term) * MULT) & 0xFFFFFFFF) >> (32 - log2_slots)


def pass_keys(queries) -> list:
    """The distinct term ids of one pass (at most 64 queries) in order of first appearance."""
    assert len(queries) <= PASS_Q
    seen, keys = set(), []
    for q in queries:
        for t in np.asarray(q, U32).tolist():
            if t not in seen:
                seen.add(t)
                keys.append(t)
    return keys


def build_table(keys):
    """``LexTable::build``: (log2_slots, slots) with slots[s] the key at slot s or None."""
    log2 = 6
    while (1 << log2) < 2 * len(keys):
        log2 += 1
    slots = [None] * (1 << log2)
    for t in keys:
        s = lex_slot(t, log2)
        while slots[s] is not None:
            s = (s + 1) & ((1 << log2) - 1)
        slots[s] = t
    return log2, slots


def probe(log2: int, slots, term: int):
    """The kernel's probe: (found, occupied slots read, the slot the probe ended at)."""
    s, read = lex_slot(term, log2), 0
    while slots[s] is not None:
        read += 1
        if slots[s] == term:
            return True, read, s
        s = (s + 1) & ((1 << log2) - 1)
    return False, read, s


def passes(queries):
    return [list(queries[p:p + PASS_Q]) for p in range(0, len(queries), PASS_Q)]


def ord32(score) -> int:
    """``lex_ord``: the order-preserving u32 image of an f32."""
    u = int(np.asarray(score, f32).view(U32))
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def bucket(score) -> int:
    return ord32(score) >> 16


def cut_model(scores, k: int):
    """``k_lex_cut`` on the scores of one query's qualifying rows: (B, M, count, the thread whose chunk holds the k-th row or
    None, its bucket inside that chunk or None)."""
    hist = np.bincount([bucket(s) for s in scores], minlength=BUCKETS)
    count = int(hist.sum())
    if count < k:
        return 0, count, count, None, None
    run = 0
    for b in range(BUCKETS - 1, -1, -1):
        run += int(hist[b])
        if run >= k:
            return b, run, count, b // 256, b % 256
    raise AssertionError("unreachable")


# ------------------------------------------------------------------ corpora and calls

def csr(rows):
    """rows: per row ``(ids ascending, tf per id or one int, dl or None = the sum of tf)``."""
    off, terms, tfs, dls = [0], [], [], []
    for ids, tf, dl in rows:
        ids = [int(t) for t in ids]
        tf = [int(tf)] * len(ids) if np.isscalar(tf) else [int(v) for v in tf]
        assert len(tf) == len(ids)
        terms.extend(ids)
        tfs.extend(tf)
        dls.append(sum(tf) if dl is None else int(dl))
        off.append(len(terms))
    return NS(row_off=np.asarray(off, np.int64), terms=np.asarray(terms, np.uint64).astype(U32), tf=np.asarray(tfs, np.uint8),
              dl=np.asarray(dls, np.int32), n=len(rows))


def call(name, queries, idf, k=10, k1=K1, b=B, avgdl=None, words=None, row_base=0, corpus=None, facts=None):
    queries = [np.asarray(q, np.uint64).astype(U32) for q in queries]
    idf = [np.asarray(w, f32) for w in idf]
    assert len(queries) == len(idf) and all(len(q) == len(w) for q, w in zip(queries, idf))
    if avgdl is None:
        avgdl = f32(max(1.0, float(corpus.dl.mean()))) if corpus.n else f32(1.0)
    return NS(name=name, queries=queries, idf=idf, k=int(k), k1=k1, b=b, avgdl=f32(avgdl), row_base=int(row_base),
              words=None if words is None else np.asarray(words, np.uint64).astype(U32), facts=facts or {})


def call_mask(corpus, c):
    return None if c.words is None else lc.mask_from_words(c.words, corpus.n)


def expected(corpus, c):
    """Source (a): the restatement."""
    return lc.bm25_search(corpus.row_off, corpus.terms, corpus.tf, corpus.dl, call_mask(corpus, c), c.queries, c.idf, c.k1, c.b,
                          c.avgdl, c.k, c.row_base)


def _round32(x: Fraction):
    """(f32 nearest to x, whether x was representable).  Every x here has far fewer than 53 significant bits, so the step
    through a double does not round."""
    d = float(x)
    assert Fraction(d) == x, "the closed form needs sums a double holds exactly"
    r = f32(d)
    return r, Fraction(float(r)) == x


def row_scores(corpus, c, order="ascending"):
    """Source (b) before the selection: per query ``(rows that hold a query term, ascending; their f32 scores; whether every
    addition was exact)`` -- for ``k1 = 0, b = 0`` only.  ``order``: "ascending" ids (the prescribed order) or "descending"."""
    assert c.k1 == 0.0 and c.b == 0.0
    er = lc.row_ids(corpus.row_off)
    out = []
    for ids, ws in zip(c.queries, c.idf):
        held = {}                                                   # row -> its query terms' idf, in ascending id
        for t, w in zip(ids.tolist(), ws.tolist()):
            for r in er[corpus.terms == U32(t)].tolist():
                held.setdefault(r, []).append(w)
        rows = np.asarray(sorted(held), np.int64)
        memo, scores, exact = {}, [], True
        for r in rows.tolist():
            key = tuple(held[r]) if order == "ascending" else tuple(reversed(held[r]))
            if key not in memo:
                acc, ok = f32(0.0), True
                for w in key:
                    acc, e = _round32(Fraction(float(acc)) + Fraction(float(f32(w))))
                    ok = ok and e
                memo[key] = (acc, ok)
            scores.append(memo[key][0])
            exact = exact and memo[key][1]
        out.append((rows, np.asarray(scores, f32), exact))
    return out


def closed_form(corpus, c, order="ascending"):
    """Source (b): ``(scores, rows, counts)`` selected by the integer image of the score, ties to the lower row."""
    mask = call_mask(corpus, c)
    nq = len(c.queries)
    scores, rows, counts = np.full((nq, c.k), -np.inf, f32), np.full((nq, c.k), -1, np.int64), np.zeros(nq, np.int64)
    for q, (r, s, _) in enumerate(row_scores(corpus, c, order)):
        if mask is not None:
            s, r = s[mask[r]], r[mask[r]]
        counts[q] = r.size
        keys = sorted(((ord32(v) << 32) | (~int(i) & 0xFFFFFFFF), j) for j, (v, i) in enumerate(zip(s, r)))[::-1][:c.k]
        pick = [j for _, j in keys]
        scores[q, :len(pick)] = s[pick]
        rows[q, :len(pick)] = r[pick] + c.row_base
    return scores, rows, counts


def has_closed_form(c) -> bool:
    return c.k1 == 0.0 and c.b == 0.0


def home_ids(log2: int, slot: int, count: int, start: int = 1, lo=None, hi=None) -> list:
    """The first ``count`` ids from ``start`` whose home slot at ``log2`` is ``slot`` (or lies in lo..hi)."""
    out, a = [], start
    while len(out) < count:
        ids = np.arange(a, a + (1 << 18), dtype=np.uint64)
        h = ((ids * np.uint64(MULT)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - log2)
        ok = (h == slot) if lo is None else ((h >= lo) & (h <= hi))
        out.extend(int(v) for v in ids[ok])
        a += 1 << 18
    return out[:count]


def _weights(rng, queries):
    return [rng.uniform(0.25, 8.0, len(q)).astype(f32) for q in queries]


def _random_rows(rng, universe, n, max_len):
    universe = np.asarray(sorted(universe), np.uint64)
    rows = []
    for i in range(n):
        ln = int(rng.integers(0, min(max_len, len(universe)) + 1))
        ids = np.sort(rng.choice(universe, ln, replace=False))
        tf = rng.integers(1, 4, ln)
        if ln and i % 7 == 0:
            tf[int(rng.integers(0, ln))] = 255
        rows.append((ids.tolist(), tf.tolist(), int(tf.sum()) + int(rng.integers(0, 50))))
    return rows


# ------------------------------------------------------------------ table families

@functools.lru_cache(maxsize=None)
def _full_pass_parts():
    rng = np.random.default_rng(20)
    ids = (rng.choice(2 ** 32 - 2, size=2 * MAX_KEYS + 8, replace=False) + 1).astype(np.uint64)      # neither 0 nor 0xFFFFFFFF
    keys, foreign, absent = ids[:MAX_KEYS], ids[MAX_KEYS:2 * MAX_KEYS], ids[2 * MAX_KEYS:]
    universe = np.sort(ids[:2 * MAX_KEYS])
    lens = rng.integers(0, 401, 1900)
    lens[:4] = (0, 400, 1, 399)
    rows = []
    for ln in lens.tolist():
        pick = np.sort(rng.choice(universe, ln, replace=False))
        tf = rng.integers(1, 4, ln)
        if ln and ln % 5 == 0:
            tf[ln // 2] = 255
        rows.append((pick.tolist(), tf.tolist(), int(tf.sum()) + int(rng.integers(0, 50))))
    return csr(rows), keys, foreign, absent


def full_pass():
    """64 queries x 32 pairwise distinct terms = 2048 keys: the 4096-slot table and 2048 idf values, 72 KiB of LDS; then 2047
    keys; then the same 2048 keys as the second pass of a 128-query call whose first pass has a 128-slot table."""
    corpus, keys, _, _ = _full_pass_parts()
    rng = np.random.default_rng(21)
    full = [np.sort(keys[32 * q:32 * q + 32]) for q in range(PASS_Q)]
    short = [q.copy() for q in full]
    short[37] = short[37][:31]
    small = [keys[q:q + 1] for q in range(PASS_Q)]
    calls = [call("2048_keys", full, _weights(rng, full), corpus=corpus, facts=dict(keys=[2048], log2=[12])),
             call("2047_keys", short, _weights(rng, short), corpus=corpus, facts=dict(keys=[2047], log2=[12])),
             call("second_pass", small + full, _weights(rng, small + full), corpus=corpus, facts=dict(keys=[64, 2048], log2=[7, 12]))]
    return NS(name="full_pass", corpus=corpus, calls=calls)


def half_full():
    """32 keys in 64 slots -- a table exactly half full, the fullest ``build`` makes -- and 33 keys in 128 slots."""
    corpus, keys, _, _ = _full_pass_parts()
    rng = np.random.default_rng(22)
    q32 = [np.sort(keys[100:132])]
    q33 = [np.sort(keys[100:132]), keys[200:201]]
    return NS(name="half_full", corpus=corpus,
              calls=[call("32_keys", q32, _weights(rng, q32), corpus=corpus, facts=dict(keys=[32], log2=[6])),
                     call("33_keys", q33, _weights(rng, q33), corpus=corpus, facts=dict(keys=[33], log2=[7]))])


CHAIN = 20


@functools.lru_cache(maxsize=None)
def _chain_parts():
    low = home_ids(6, 63, 2 * CHAIN)                        # 55, 144, 199, 288, 343, ...
    high = home_ids(12, 4095, 2 * CHAIN)                    # 2584, 6765, 13530, ...
    fill = home_ids(12, None, 1100, start=1_000_000, lo=100, hi=4000)      # homes far from the chain's slots
    rng = np.random.default_rng(23)
    others = (rng.choice(2 ** 31, 40, replace=False) + 2 ** 31).tolist()
    universe = set(low) | set(high) | set(fill[:60]) | set(others)
    rows = _random_rows(rng, universe, 150, 60)
    for i, t in enumerate(low[CHAIN:] + high[CHAIN:]):      # every corpus-only id of a chain is in at least one row
        ids, tf, dl = rows[3 + 3 * i]
        if t not in ids:
            rows[3 + 3 * i] = (sorted(ids + [t]), tf + [1], dl + 1)
    return csr(rows), low, high, fill


def wrapped_chain():
    """20 query terms with one home slot -- the LAST slot of the table -- so the chain runs 63, 0, 1, ... 18 (4095, 0, ... 18 in
    the 4096-slot table), and 20 corpus-only ids with the same home slot whose probes read the whole chain and end at the empty
    slot behind it."""
    corpus, low, high, fill = _chain_parts()
    rng = np.random.default_rng(24)
    q6 = [sorted(low[:CHAIN])]
    q12 = [sorted(high[:CHAIN])] + [sorted(fill[i:i + 32]) for i in range(0, len(fill), 32)]
    return NS(name="wrapped_chain", corpus=corpus,
              calls=[call("log2_6", q6, _weights(rng, q6), corpus=corpus,
                          facts=dict(keys=[CHAIN], log2=[6], chain=sorted(low[:CHAIN]), foreign=low[CHAIN:])),
                     call("log2_12", q12, _weights(rng, q12), corpus=corpus,
                          facts=dict(keys=[CHAIN + len(fill)], log2=[12], chain=sorted(high[:CHAIN]), foreign=high[CHAIN:]))])


EDGE_IDS = (0, 0xFFFFFFFF)


@functools.lru_cache(maxsize=None)
def _edge_corpus(with_edges: bool):
    rng = np.random.default_rng(25)
    mid = [7, 1000, 2 ** 31, 0xFFFFFFFE, 12345, 99]
    rows = []
    for i in range(70):
        ids = sorted(set(rng.choice(mid, int(rng.integers(0, 5))).tolist()))
        if with_edges and i % 3 == 0:
            ids = [0] + ids
        if with_edges and i % 4 == 1:
            ids = ids + [0xFFFFFFFF]
        rows.append((ids, 1 + i % 3, None))
    rows[5] = ((EDGE_IDS if with_edges else (7, 99)), 2, 9)
    rows[33] = (((0,) if with_edges else (7,)), 1, 1)
    return csr(rows)


def edge_ids():
    """Term ids 0 (the value padded lanes carry) and 0xFFFFFFFF: in the query and in rows, in rows only, in the query only."""
    rng = np.random.default_rng(26)
    have, lack = _edge_corpus(True), _edge_corpus(False)
    both, plain = [[0, 7, 0xFFFFFFFF], [0], [0xFFFFFFFF], [0, 0xFFFFFFFF]], [[7, 1000], [99]]
    return [NS(name="edge_ids", corpus=have,
               calls=[call("query_and_rows", both, _weights(rng, both), corpus=have), call("rows_only", plain, _weights(rng, plain), corpus=have)]),
            NS(name="edge_ids_query_only", corpus=lack, calls=[call("query_only", both, _weights(rng, both), corpus=lack)])]


SHARED = dict(all=5000, ends=5001, odd=5002, one=5003)


def shared_terms():
    """One term in all 64 queries with 64 distinct idf values (lane 63 reads ``base + 63``), one in queries {0, 63}, one in the odd
    queries, one in a single query -- each query with private terms on both sides of the shared ids, so the shared contribution
    falls in the middle of its ascending-id sum."""
    rng = np.random.default_rng(27)
    queries, idf = [], []
    for q in range(PASS_Q):
        ids = [100 + 2 * q, 101 + 2 * q, SHARED["all"], 9000 + 2 * q, 9001 + 2 * q]
        ids += [SHARED["ends"]] if q in (0, 63) else []
        ids += [SHARED["odd"]] if q % 2 else []
        ids += [SHARED["one"]] if q == 17 else []
        queries.append(sorted(ids))
        idf.append([f32(1.0 + q / 7.0) if t == SHARED["all"] else f32(rng.uniform(0.25, 8.0)) for t in sorted(ids)])
    universe = set(t for q in queries for t in q) | set(range(20000, 20030))
    corpus = csr(_random_rows(rng, universe, 300, 80))
    return NS(name="shared_terms", corpus=corpus, calls=[call("64_queries", queries, idf, corpus=corpus)])


# ------------------------------------------------------------------ walk families (32-row tiles)

def _pad_tile(rows):
    return rows + [((), 1, 0)] * (-len(rows) % 32)


def one_ballot():
    """Tiles of 32 rows of one entry each, every entry a hit: 32 finished rows inside one 64-lane step; two such tiles, so the
    row being summed starts afresh in each."""
    rng = np.random.default_rng(28)
    out = []
    queries = [[11, 12, 13], [11], [12, 13]]
    for n in (32, 64):
        corpus = csr([((11 + i % 3,), 1 + i % 4, 4 + i % 5) for i in range(n)])
        out.append(NS(name="one_ballot_%d" % n, corpus=corpus, calls=[call("rows_%d" % n, queries, _weights(rng, queries), k=40, corpus=corpus)]))
    return out


LONG_AT = (0, 63, 64, 127, 128, 191, 192, 255, 256, 257, 319, 320, 383, 384, 511, 512, 513, 639, 640, 767, 768, 769, 895, 896,
           959, 960, 998, 999, 1, 62, 65, 500)
LONG_BEFORE = ((), (1,), (62,), (193,), (1, 62, 193))        # the rows in front of the long row, per tile


def long_row():
    """A row of 1000 ascending ids whose 32 query terms straddle every 64-entry step edge and every 256-entry outer-iteration
    edge; first in its tile and behind 1, 62, 193 and 256 other entries; the next row's first entry is a hit in the long row's
    last ballot."""
    rng = np.random.default_rng(29)
    long_ids = [1000 + 3 * i for i in range(1000)]
    q_ids = sorted(long_ids[p] for p in LONG_AT)
    rows = []
    for before in LONG_BEFORE:
        tile = [([1001 + 3 * i for i in range(n)], 1, None) for n in before]       # ids between the long row's: no hits
        tile.append((long_ids, rng.integers(1, 256, 1000).tolist(), 300_000 + len(rows)))
        tile.append(([q_ids[0], q_ids[0] + 1, q_ids[5]], [3, 1, 2], 9))
        rows += _pad_tile(tile)
    corpus = csr(rows)
    queries = [q_ids, q_ids[::2], [q_ids[0], q_ids[-1]]]
    return NS(name="long_row", corpus=corpus, calls=[call("five_tiles", queries, _weights(rng, queries), corpus=corpus)])


def empty_rows():
    """Empty rows at the start of a tile, between two hit rows and at its end; a tile of 32 empty rows under a set mask word; a
    tile whose only non-empty row is its row 31."""
    rng = np.random.default_rng(30)
    hit = lambda i: ((21, 22 + i % 2, 30 + i), [1, 2, 1], 5 + i)        # noqa: E731
    none = ((), 1, 0)
    rows = [none] * 5 + [hit(0)] + [none] * 4 + [hit(1)] + [none] * 21
    rows += [none] * 32
    rows += [none] * 31 + [hit(2)]
    rows += [hit(3), none, hit(4)] + [none] * 28 + [hit(5)]
    corpus = csr(rows)
    queries = [[21], [22, 23], [21, 22, 23, 31]]
    w = _weights(rng, queries)
    return NS(name="empty_rows", corpus=corpus,
              calls=[call("no_mask", queries, w, corpus=corpus), call("all_set", queries, w, words=[0xFFFFFFFF] * 4, corpus=corpus)])


def masked_between():
    """Three consecutive one-entry hit rows with the middle one masked out, and a masked row with hits on both sides of a step
    edge (entries 63 and 64 of its tile) between two rows that count."""
    rng = np.random.default_rng(31)
    rows = [((40,), 1, 2), ((40,), 2, 2), ((40,), 3, 3)] + [((), 1, 0)] * 29
    lead = ([39 + 100 * i for i in range(1, 60)], 1, None)                       # entries 0..58 of tile 1, no hits
    before = ([40, 41], [1, 1], 4)                                               # entries 59, 60: hits
    across = ([38, 39, 40, 41, 42], [1, 1, 2, 2, 1], 9)                          # entries 61..65: hits at 63 and 64
    after = ([40, 43], [5, 1], 7)                                                # entries 66, 67
    rows += _pad_tile([lead, before, across, after])
    corpus = csr(rows)
    words = [0xFFFFFFFF & ~(1 << 1), 0xFFFFFFFF & ~(1 << 2)]
    queries = [[40, 41], [40], [41]]
    w = _weights(rng, queries)
    return NS(name="masked_between", corpus=corpus,
              calls=[call("middle_out", queries, w, words=words, corpus=corpus, facts=dict(masked=[1, 34])),
                     call("no_mask", queries, w, corpus=corpus)])


def tails():
    """A last tile of 1 and of 31 rows under a last mask word of 0xFFFFFFFF (the bits past the row count must be ignored), in
    corpora of 1, 3 and 5 tiles: fewer tiles than one workgroup has waves, exactly one short of it, and one more."""
    rng = np.random.default_rng(32)
    out = []
    queries = [[50, 51, 52], [52]]
    for n in (1, 31, 95, 129):
        corpus = csr(_random_rows(rng, set(range(48, 56)), n, 6)[:-1] + [((50, 52), [2, 1], 4)])
        w = _weights(rng, queries)
        words = [0xFFFFFFFF] * ((n + 31) // 32)
        out.append(NS(name="tails_%d" % n, corpus=corpus,
                      calls=[call("all_set", queries, w, k=200, words=words, corpus=corpus), call("no_mask", queries, w, k=200, corpus=corpus)]))
    return out


ORDER_WEIGHTS = ((2.0 ** 25, 1.0, -2.0 ** 25), (2.0 ** 25, -2.0 ** 25, 1.0), (1.0, 2.0 ** 25, -2.0 ** 25), (1.0, -2.0 ** 25, 2.0 ** 25),
                 (-2.0 ** 25, 2.0 ** 25, 1.0), (-2.0 ** 25, 1.0, 2.0 ** 25))
ORDER_SUMS = (0.0, 1.0, 0.0, 0.0, 1.0, 0.0)                # the ascending-id f32 sum of each assignment, worked out by hand:
#   2^25 + 1 and -2^25 + 1 are ties between two f32 and round to the even one, +-2^25; 1 - 2^25 likewise rounds to -2^25.


def order_matters():
    """Three terms weighing (+2^25, +1, -2^25) in all six assignments, six queries of one call: with k1 = 0, b = 0 the
    ascending-id f32 sum is 0 or 1 by the assignment, and any other order gives other bits for some of them.  A second call uses
    k1 = 1.2 on rows of tf 255 and dl 2^24 + 1 (no closed form: against the restatement)."""
    ids = [60, 61, 62]
    rows = [(ids, 255, 2 ** 24 + 1), ((60, 61), 255, 2 ** 24 + 1), ((61, 62), 1, 2), ((60, 62), 2, 2 ** 24 + 1), ((62,), 255, 255),
            (ids, 1, 3), ((59, 63), 1, 2), (ids, [255, 1, 255], 2 ** 24 + 1)]
    corpus = csr(_pad_tile(rows) + [(ids, 3, 2 ** 24 + 1)])
    queries, idf = [ids] * 6, [list(w) for w in ORDER_WEIGHTS]
    return NS(name="order_matters", corpus=corpus,
              calls=[call("closed", queries, idf, k1=0.0, b=0.0, avgdl=1.0, corpus=corpus), call("bm25", queries, idf, avgdl=2.0 ** 20, corpus=corpus)])


# ------------------------------------------------------------------ cut and select families

# 16 "bit" terms and one more in the middle of their ids.  With STD_IDF a row that holds the bits of the 16-bit two's complement
# of n scores n / 128 exactly: 2.0 = 256 / 128 is bucket 0xC000, 255 / 128 = 1.9921875 is bucket 0xBFFF, -2.0 is 0x3FFF and
# -1.9921875 is 0x4000.  The seventeenth term weighs 0: a row that holds it alone scores +0.0, bucket 0x8000.
STD_IDF = tuple(2.0 ** (j - 7) for j in range(15)) + (-2.0 ** 8,)
TOP_IDF = tuple(2.0 ** (112 + j) for j in range(15)) + (2.0 ** 127,)            # bit 15 set: >= 2^127, thread 255's chunk
BOTTOM_IDF = tuple(-2.0 ** (112 + j) for j in range(15)) + (-2.0 ** 127,)       # bit 15 set: <= -2^127, thread 0's chunk
CROWD_IDF = tuple(2.0 ** (j - 22) for j in range(16))                           # + 2.0 from the seventeenth term: one bucket


def _bits(n: int) -> list:
    return [j for j in range(16) if (n >> j) & 1]


def _sub(name, idf, levels, mid=0.0, **facts):
    """levels: per row the list of term positions (0..15 the bits, 16 the middle term)."""
    return NS(name=name, idf=tuple(idf) + (mid,), rows=[sorted(r) for r in levels], facts=facts)


def _twos(ns):
    return [_bits(n & 0xFFFF) for n in ns]


def cut_subcases(k: int) -> list:
    up = [258 + 29 * i for i in range(k)]                  # distinct scores above 2.0 + 2^-6, none in bucket 0xC000
    tail = [254 - 7 * i for i in range(20)] + [-5, -300]
    neg_up = [-250 + 29 * i for i in range(k)]             # distinct, all above -1.9921875, never 0
    neg_tail = [-258 - 7 * i for i in range(20)]
    pos = [1 + 29 * i for i in range(k)]
    subs = [
        _sub("i0", STD_IDF, _twos(up[:k - 1] + [256] + [255] * 3 + tail), kth=0xC000, nxt=0xBFFF, m=k, count=k + 25),
        _sub("i255", STD_IDF, _twos(up[:max(k - 2, 0)] + [256] * min(k - 1, 1) + [255] * 2 + tail), kth=0xBFFF, nxt=0xBFFF, m=k + 1,
             count=k + 23),
        _sub("neg_i0", STD_IDF, _twos(neg_up[:k - 1] + [-255] + [-256] * 3 + neg_tail), kth=0x4000, nxt=0x3FFF, m=k, count=k + 23),
        _sub("neg_i255", STD_IDF, _twos(neg_up[:max(k - 2, 0)] + [-255] * min(k - 1, 1) + [-256] * 2 + neg_tail), kth=0x3FFF, nxt=0x3FFF,
             m=k + 1, count=k + 21),
        _sub("zero", STD_IDF, _twos(pos[:k - 1]) + [[16], [16]] + [b + [16] for b in _twos([-1 - 7 * i for i in range(20)])] + _twos([-3]),
             kth=0x8000, nxt=0x8000, m=k + 1, count=k + 22),
        _sub("chunk0", BOTTOM_IDF, _twos([1 + 29 * i for i in range(max(k - 3, 0))] + [0x8000 + 5 + 700 * i for i in range(10)]),
             kth_chunk=0, count=max(k - 3, 0) + 10),
        _sub("chunk255", TOP_IDF, _twos([0x8000 + 5 + 29 * i for i in range(k + 5)] + [1 + 29 * i for i in range(20)]), kth_chunk=255, count=k + 25),
        _sub("m_eq_k", STD_IDF, _twos(up[:max(k - 3, 0)] + [100] * min(k, 3) + [90 - i for i in range(20)]), kth=bucket(100 / 128.0), m=k,
             count=max(k - 3, 0) + min(k, 3) + 20),
        _sub("count_eq_k", STD_IDF, _twos([(-1) ** i * (3 + i // 2) for i in range(k)]), count=k, m=k),
        _sub("count_eq_km1", STD_IDF, _twos([(-1) ** i * (3 + i // 2) for i in range(k - 1)]), count=k - 1, m=k - 1),
    ]
    return subs


def _term_ids(slot: int) -> list:
    """The 17 term ids of sub-case ``slot``, ascending: bits 0..7, the middle term, bits 8..15; odd ids in between are foreign."""
    base = 100_000 * (slot + 1)
    pos = list(range(8)) + [16] + list(range(8, 16))
    ids = [0] * 17
    for at, p in enumerate(pos):
        ids[p] = base + 2 * at
    return ids


def cut_group(name, subs, k, seed, alone=False):
    """One corpus holding the rows of every sub-case (each over its own 17 term ids, all rows shuffled together) and one call in
    which query q is sub-case q: the per-query cut, M, list base and fill slots side by side.  ``alone``: each sub-case also as
    a call of its own."""
    rng = np.random.default_rng(seed)
    rows, queries, idf = [], [], []
    for s, sub in enumerate(subs):
        ids = _term_ids(s)
        order = np.argsort(ids)
        queries.append([ids[p] for p in order])
        idf.append([sub.idf[p] for p in order])
        for held in sub.rows:
            mine = [ids[p] for p in held]
            mine += [t + 1 for t in mine if rng.random() < 0.3]                  # foreign ids in between
            rows.append((sorted(mine), int(rng.integers(1, 256)), None))
    rows = [rows[i] for i in rng.permutation(len(rows))]
    corpus = csr(rows)
    c = call("k_%d" % k, queries, idf, k=k, k1=0.0, b=0.0, avgdl=1.0, corpus=corpus, facts=dict(subs=[s.name for s in subs], sub_facts=[s.facts for s in subs]))
    singles = [call("alone_" + s.name, [queries[i]], [idf[i]], k=k, k1=0.0, b=0.0, avgdl=1.0, corpus=corpus) for i, s in enumerate(subs)] if alone else []
    return NS(name=name, corpus=corpus, calls=[c] + singles)


def cuts():
    out = []
    for k in (1, 10):
        out.append(cut_group("cut_k%d" % k, cut_subcases(k), k, 40 + k, alone=k == 10))
    subs = cut_subcases(MAX_K)
    out.append(cut_group("cut_k1024_a", subs[:5], MAX_K, 50))
    out.append(cut_group("cut_k1024_b", subs[5:], MAX_K, 51))
    return out


def crowded():
    """5000 rows of 3000 distinct scores in ONE bucket (they differ only below the top 16 bits of ``ord``): the list is 5000 long
    and the radix passes of ``k_lex_select`` decide; and the same 5000 rows under a one-term query: one identical score over 157
    tiles, the answer rows 0..k-1 in order, ``row_base = 3 << 32``."""
    rng = np.random.default_rng(60)
    distinct = rng.choice(65536, 3000, replace=False)
    ms = np.concatenate([distinct, rng.choice(distinct, 2000)])
    ms = ms[rng.permutation(ms.size)]
    ids = _term_ids(0)
    order = np.argsort(ids)
    rows = [(sorted([ids[p] for p in _bits(int(m)) + [16]]), 1 + int(m) % 200, None) for m in ms.tolist()]
    corpus = csr(rows)
    q, w = [[ids[p] for p in order]], [[(CROWD_IDF + (2.0,))[p] for p in order]]
    one, w_one = [[ids[16]]], [[1.5]]
    both, w_both = q + one, w + w_one
    kw = dict(k1=0.0, b=0.0, avgdl=1.0, corpus=corpus)
    calls = [call("crowded_k%d" % k, q, w, k=k, facts=dict(one_bucket=0xC000, distinct=3000), **kw) for k in (1, 10, MAX_K)]
    calls += [call("identical_k%d" % k, one, w_one, k=k, row_base=3 << 32, facts=dict(identical=True), **kw) for k in (1, MAX_K)]
    calls += [call("both_k1024", both, w_both, k=MAX_K, row_base=3 << 32, **kw)]
    return NS(name="crowded", corpus=corpus, calls=calls)


# ------------------------------------------------------------------ all search families, and the statistics

@functools.lru_cache(maxsize=None)
def families() -> dict:
    out = [full_pass(), half_full(), wrapped_chain()] + edge_ids() + [shared_terms()] + one_ballot() + [long_row(), empty_rows(), masked_between()]
    out += tails() + [order_matters()] + cuts() + [crowded()]
    assert len(set(f.name for f in out)) == len(out)
    return {f.name: f for f in out}


def interloper(fam):
    """A call with a table of another size than the family's own (and hits of its own), to run between two runs of the family
    on one handle: 2048 keys for a family of small tables, one key for a family of large ones."""
    own = np.unique(fam.corpus.terms).astype(np.uint64)
    big = max(max(c.facts.get("log2", [6])) for c in fam.calls) >= 10 or max(len(pass_keys(p)) for c in fam.calls for p in passes(c.queries)) > 512
    if big:
        queries = [own[:1]] if own.size else [[1]]
    else:
        extra = np.setdiff1d(np.arange(7_000_000, 7_000_000 + MAX_KEYS, dtype=np.uint64), own)
        keys = np.concatenate([own[:MAX_KEYS // 2], extra])[:MAX_KEYS]
        queries = [np.sort(keys[32 * q:32 * q + 32]) for q in range(PASS_Q)]
    return call("interloper", queries, [np.ones(len(q), f32) for q in queries], k=MAX_K, corpus=fam.corpus)


STATS_MASKS = ("none", "random", "clear")


def stats_mask(corpus, kind):
    """Validity words, or None."""
    if kind == "none":
        return None
    if kind == "clear":
        return np.zeros((corpus.n + 31) // 32, U32)
    return lc.words_from_mask(np.random.default_rng(70).random(corpus.n) < 0.05)


@functools.lru_cache(maxsize=None)
def stats_families() -> dict:
    """name -> (corpus, ids): 2048, 2049 and 4100 distinct ids over the ``full_pass`` corpus (one walk, two, three with a short
    last one), repeats on both sides of a chunk edge, the chain ids, ids 0 and 0xFFFFFFFF."""
    corpus, keys, foreign, absent = _full_pass_parts()
    chain_corpus, low, high, _ = _chain_parts()
    every = np.concatenate([keys, foreign, absent[:4]])
    repeats = np.concatenate([every[:2040], every[5:9], every[2040:2060], every[2044:2052], every[:3], every[2060:2100], every[2047:2049]])
    return {"ids_2048": (corpus, keys.copy()), "ids_2049": (corpus, np.concatenate([keys, foreign[:1]])), "ids_4100": (corpus, every),
            "repeats": (corpus, repeats), "chain": (chain_corpus, np.asarray(low + high, np.uint64)),
            "edge_ids": (_edge_corpus(True), np.asarray([0, 7, 0xFFFFFFFF, 0, 5], np.uint64)),
            "edge_ids_absent": (_edge_corpus(False), np.asarray([0xFFFFFFFF, 7, 0], np.uint64))}


@functools.lru_cache(maxsize=None)
def _df_table(corpus_key, kind):
    """``lex_cases.stats`` once per (corpus, mask) over every id any statistics case asks of that corpus."""
    corpus = next(c for c, _ in stats_families().values() if id(c) == corpus_key)
    ids = np.unique(np.concatenate([i for c, i in stats_families().values() if id(c) == corpus_key])).astype(U32)
    words = stats_mask(corpus, kind)
    mask = None if words is None else lc.mask_from_words(words, corpus.n)
    df, rows, sum_dl = lc.stats(corpus.row_off, corpus.terms, corpus.dl, mask, ids)
    return dict(zip(ids.tolist(), df.tolist())), rows, sum_dl


def stats_expected(name, kind):
    """(df int64 per id, rows, sum_dl) from ``lex_cases.stats``."""
    corpus, ids = stats_families()[name]
    table, rows, sum_dl = _df_table(id(corpus), kind)
    return np.asarray([table[int(t)] for t in ids.astype(U32).tolist()], np.int64), rows, sum_dl
