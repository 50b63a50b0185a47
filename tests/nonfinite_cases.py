"""Non-finite vectors: corpora, query batches and expectations.  Test infrastructure only; no GPU import.

The rule: A NaN SCORE IS NO SCORE.  A stored row or a query that holds a NaN or an infinity preprocesses to a vector with NaN
elements (``orc_cosine_preprocess``: a NaN makes ``len2`` NaN and the whole vector NaN; an infinity makes ``len2`` infinite and
leaves zeros with a NaN where the infinity stood), every canonical score it takes part in is NaN, and such a (query, row) pair is
in no result list and in no score-conditioned count -- exactly as ``score >= t`` is false for it.  Everything that does not score
vectors (filters, counts without a threshold, text, deletes, compaction, snapshots) treats the row as any other.

The corpora have ``N = 4099`` rows (129 tiles of 32, a ragged last tile) with the bad rows at fixed places (``bad_rows``); the
expected lists are ``oracle.search`` on ``oracle.search.preprocess`` of the raw rows.  ``sunk`` corpora are built as ``-(query
direction) + noise``: every finite row scores below 0, so a nomination scheme that gives a bad row the interval ``[-c, +c]`` (the
int8 copy's zero-scale row) both has to nominate it (its upper end is above any valid threshold) and -- with bad rows in at least
``k`` sample tiles -- would take ``-c`` for a lower bound of the k-th score and nominate no finite row at all."""
import functools

import numpy as np

from oracle import search as orc

F32, U32 = np.float32, np.uint32
N = 4099
TILE = 32
WHOLE_TILE = 7                                   # every row of this tile is bad
FILTER = [(1, 9)]                                # code column 1 == 9: FILTER_ROWS, 3 of them bad
KINDS = ("nan_first", "nan_last", "plus_inf", "minus_inf", "all_nan")


def spoil(vec: np.ndarray, kind: str, at: int | None = None) -> np.ndarray:
    """``vec`` with one kind of non-finite content: a NaN at element 0 / at the last element, one +inf / -inf at ``at`` (default:
    the middle), or NaN everywhere."""
    v = np.array(vec, F32)
    mid = v.shape[-1] // 2 if at is None else at
    if kind == "nan_first":
        v[..., 0] = np.nan
    elif kind == "nan_last":
        v[..., -1] = np.nan
    elif kind == "plus_inf":
        v[..., mid] = np.inf
    elif kind == "minus_inf":
        v[..., mid] = -np.inf
    elif kind == "all_nan":
        v[...] = np.nan
    else:
        raise ValueError(kind)
    return v


def bad_rows(n: int = N) -> dict:
    """row -> kind.  Row 0, rows 31 and 32 (both sides of a tile edge), the last row (in the ragged tile); every row of tile
    ``WHOLE_TILE``; one row with a single +inf, one with a single -inf, one with NaN as its last element; four more in tiles of
    their own, so that bad rows sit in 11 tiles: more than the k = 10 of the smallest case."""
    rows = {0: "nan_first", 31: "nan_last", 32: "all_nan", n - 1: "nan_first"}
    for j in range(TILE):
        rows[WHOLE_TILE * TILE + j] = KINDS[j % len(KINDS)]
    rows.update({1000: "plus_inf", 2050: "minus_inf", 3333: "nan_last", 500: "nan_first", 1500: "plus_inf", 2500: "minus_inf", 3700: "all_nan"})
    return {r: k for r, k in rows.items() if 0 <= r < n}


FILTER_TILES = (0, 31, 104, 3, 9, 16, 22, 28, 40, 47, 55, 61, 70, 77, 85, 90, 99, 110, 120, 126)
FILTER_ROWS = np.asarray(sorted([31, 5, 1000, 31 * TILE + 20, 3333, 104 * TILE + 20] + [t * TILE + j for t in FILTER_TILES[3:] for j in (5, 20)]), np.int64)


def direction(dim: int) -> np.ndarray:
    d = np.random.default_rng(7).standard_normal(dim).astype(F32)
    return d / F32(np.linalg.norm(d))


@functools.lru_cache(maxsize=None)
def corpus(kind: str = "gauss", dim: int = 768, n: int = N):
    """``(raw [n, dim] f32, codes [n, 2] i32, bad bool [n])``.  ``gauss``: N(0, 1) rows scaled by 0.2 .. 5 per row; ``sunk``: ``-3 *
    direction + N(0, 1) / 4`` (every finite row scores about -0.4 against a query near ``direction``).  Code columns as in
    tests/test_search_gpu.py (column 0 in 0..2, column 1 in 0..6) with column 1 = 9 on ``FILTER_ROWS``: 40 rows in 20 tiles, rows 31,
    1000 and 3333 of them bad."""
    rng = np.random.default_rng([11, dim, n, kind == "sunk"])
    if kind == "gauss":
        raw = rng.standard_normal((n, dim), dtype=F32) * rng.uniform(0.2, 5.0, size=(n, 1)).astype(F32)
    elif kind == "sunk":
        raw = (F32(-3.0) * direction(dim)[None, :] + F32(0.25) * rng.standard_normal((n, dim), dtype=F32)).astype(F32)
    else:
        raise ValueError(kind)
    codes = np.stack([rng.integers(0, 3, n), rng.integers(0, 7, n)], axis=1).astype(np.int32)
    codes[FILTER_ROWS[FILTER_ROWS < n], 1] = 9
    bad = np.zeros(n, bool)
    for r, k in bad_rows(n).items():
        raw[r] = spoil(raw[r], k, at=(r * 13) % dim)
        bad[r] = True
    raw.setflags(write=False)
    codes.setflags(write=False)
    bad.setflags(write=False)
    return raw, codes, bad


def bad_slots(nq: int) -> dict:
    """slot -> kind: the bad queries of a batch of ``nq`` -- slots 0, 31, 32 and 63 (the edges of the two 32-query MFMA column
    blocks) and 17, then 64 and the last slot of a wider batch -- every kind at least once from 64 queries up."""
    want = {0: "nan_first", 17: "all_nan", 31: "nan_last", 32: "plus_inf", 63: "minus_inf", 64: "all_nan", nq - 1: "nan_last" if nq > 64 else "minus_inf"}
    return {s: k for s, k in want.items() if 0 <= s < nq}


@functools.lru_cache(maxsize=None)
def queries(kind: str = "gauss", dim: int = 768, nq: int = 64, spoiled: bool = True):
    """``(q [nq, dim] f32, bad bool [nq])``: finite queries (``sunk``: near ``direction``) with the bad ones of ``bad_slots``
    between them; ``spoiled=False``: the same batch with zeros in the bad slots."""
    rng = np.random.default_rng([13, dim, nq, kind == "sunk"])
    q = rng.standard_normal((nq, dim), dtype=F32)
    if kind == "sunk":
        q = (direction(dim)[None, :] + F32(0.02) * q).astype(F32)
    bad = np.zeros(nq, bool)
    for s, k in bad_slots(nq).items():
        q[s] = spoil(q[s], k) if spoiled else 0
        bad[s] = True
    q.setflags(write=False)
    bad.setflags(write=False)
    return q, bad


@functools.lru_cache(maxsize=None)
def stored(kind: str, dim: int, bf16: bool, n: int = N) -> np.ndarray:
    """The stored form of the corpus: ``orc_preprocess_rows`` of the raw rows."""
    out = orc.preprocess(corpus(kind, dim, n)[0], to_bf16=bf16)
    out.setflags(write=False)
    return out


def same_stored(got: np.ndarray, want: np.ndarray) -> bool:
    """Stored rows compared by NaN POSITIONS plus the bit patterns of every other element (the payload bits of a NaN may differ
    between the CPU and the device)."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    gn, wn = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(gn, wn) and np.array_equal(got.view(U32)[~gn], want.view(U32)[~wn])


def nan_pattern(raw_row: np.ndarray) -> np.ndarray:
    """Where the stored form of a raw row holds NaN, from the description in the module docstring: everywhere if the row holds a
    NaN, else exactly where it holds an infinity."""
    r = np.asarray(raw_row, F32)
    return np.ones(r.shape, bool) if np.isnan(r).any() else np.isinf(r)


@functools.lru_cache(maxsize=None)
def expected(kind: str, dim: int, bf16: bool, nq: int, k: int, filtered: bool = False, spoiled: bool = True, n: int = N):
    """The restated oracle's ``(scores [nq, k], rows [nq, k])`` for the corpus and the batch; ``filtered``: under ``FILTER``."""
    _, codes, _ = corpus(kind, dim, n)
    q, _ = queries(kind, dim, nq, spoiled)
    s, r = orc.search(stored(kind, dim, bf16, n), orc.preprocess(q, to_bf16=bf16), k, codes=codes if filtered else None, filters=FILTER if filtered else None)
    s.setflags(write=False)
    r.setflags(write=False)
    return s, r


def same_lists(s, r, es, er) -> bool:
    return np.array_equal(np.asarray(r), np.asarray(er)) and np.array_equal(np.asarray(s, F32).view(U32), np.asarray(es, F32).view(U32))


def well_formed(s: np.ndarray, r: np.ndarray) -> bool:
    """Every list: no NaN, descending score with ascending row among equals, then only ``(-inf, -1)`` padding."""
    for sq, rq in zip(np.asarray(s), np.asarray(r)):
        hits = int((rq >= 0).sum())
        if np.isnan(sq).any() or (rq[:hits] < 0).any() or (rq[hits:] != -1).any() or not np.isneginf(sq[hits:]).all():
            return False
        a, b = sq[:hits].astype(np.float64), rq[:hits]
        if hits > 1 and not np.all((a[:-1] > a[1:]) | ((a[:-1] == a[1:]) & (b[:-1] < b[1:]))):
            return False
    return True


# ------------------------------------------------------------------ the store-level case (tests/lifecycle_cases.py's points and checks)

STORE_POINTS = 300
BAD_KINDS = ("nan_first", "plus_inf", "minus_inf", "nan_last", "all_nan")
BAD_PAYLOAD_OF = (3, 12, 28, 44, 61)            # each bad point carries a COPY of this point's payload: no value the dictionaries have not seen
BAD_AT = (0, 96, 97, 203, 304)                  # where the five sit in the upsert (the first row of all, a pair, one inside, the last row)
# the read paths that score vectors (features of lifecycle_cases.checks), the checks of other features that do, and the checks that
# still see the five points
SCORED = ("plain", "filter", "range", "threshold", "mmr", "group", "span", "batch", "multi", "range_batch", "groups", "fused", "recommend", "text_filter", "rerank")
SCORED_NAMES = ("any-of", "must_not", "no file_path")
SEES_THEM = ("filter-only fetch", "filter-only fetch, must_not", "lexical_count", "search_lexical_batch", "count_text {'contains': 'TODO'}",
             "search_text {'contains': 'TODO'}", "client.count MatchText")


def _bad_point(j: int):
    from tests import lifecycle_cases as lc
    import copy
    pid, vec, _ = lc.point(900 + j)
    return pid, spoil(vec, BAD_KINDS[j]), copy.deepcopy(lc.point(BAD_PAYLOAD_OF[j])[2])


BAD_IDS = tuple(f"00000000-0000-4000-8000-{900 + j:012d}" for j in range(5))


def store_points(with_bad: bool):
    """``(ids, vectors [n, DIM], payloads)`` of ONE upsert: lifecycle_cases' points 0 .. 299 and, ``with_bad``, the five non-finite
    points at positions ``BAD_AT`` of the call."""
    from tests import lifecycle_cases as lc
    ids, vecs, pays = lc.points(range(STORE_POINTS))
    ids, vecs, pays = list(ids), list(vecs), list(pays)
    if with_bad:
        for j, at in enumerate(BAD_AT):
            pid, vec, pay = _bad_point(j)
            ids.insert(at, pid)
            vecs.insert(at, vec)
            pays.insert(at, pay)
    return ids, np.stack(vecs), pays


def store_models(bf16: bool, ns: int = 1, block: int = 4096):
    """``(model with the five points, model without)`` after that one upsert."""
    from tests import lifecycle_cases as lc
    out = []
    for with_bad in (True, False):
        m = lc.Model(ns=ns, block=block)
        m.upsert(*store_points(with_bad))
        out.append(m)
    return tuple(out)


def sums_model():
    from tests import lifecycle_cases as lc
    m = lc.Model(text_key="summary")
    m.upsert(*lc.summary_points())
    return m
