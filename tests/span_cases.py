"""CPU restatement of the overlap-free walk (``crh_span_select``), the brute-force definition of the
``max_overlap`` top-k it serves, the numpy form of a filter with range conditions, and the inputs the tests of both tiers share.
Test infrastructure only -- the checker of both tiers.

The definition, per query: all alive rows that pass the filter in the order of the plain search (score descending, ties by
lower global row).  A row HAS A SPAN iff its file code, its first line ``lo`` and its last line ``hi`` satisfy ``file >= 0``,
``lo >= 0`` and ``hi >= lo``; the span's length is ``hi - lo + 1``.  Walking that order, a row without a span is kept; a row
``i`` with a span is REDUNDANT iff some earlier KEPT row ``j`` with a span and the same file has ``ov = min(hi_i, hi_j) -
max(lo_i, lo_j) + 1 > 0`` and ``ov * 1000 > permille * min(len_i, len_j)`` (integers, nothing rounded); otherwise it is kept.
The ``max_overlap`` top-``limit`` = the first ``limit`` kept rows.

``crh_span_select`` is that walk over one candidate list of ``c`` entries (padding ``(-inf, -1)`` at the end is skipped): the
first ``k`` kept candidates in list order -- position, row, the score's bits, file, lo, hi -- the tail ``(-1, -1, -inf, -1, -1,
-1)``, and ``info = (kept in the WHOLE list, real candidates)``.  Whether a candidate is kept depends on the candidates before
it only, so the kept candidates of a list that is a prefix of the corpus-wide order are a prefix of the corpus-wide walk.
"""
import numpy as np

from oracle import search as orc

F32 = np.float32


def walk(files, los, his, permille: int) -> list[int]:
    """Positions kept by the walk over real candidates given in order (Python integers: no overflow, no rounding).  The kept
    spans of a file are held once each: a second kept copy of a span (permille 1000) answers every later test as the first does."""
    kept_spans: dict[int, dict[tuple[int, int], None]] = {}
    kept = []
    for i, (f, lo, hi) in enumerate(zip(files, los, his)):
        f, lo, hi = int(f), int(lo), int(hi)
        if f >= 0 and lo >= 0 and hi >= lo:
            redundant = False
            for (l, h) in kept_spans.get(f, ()):
                ov = min(hi, h) - max(lo, l) + 1
                if ov > 0 and ov * 1000 > permille * min(hi - lo + 1, h - l + 1):
                    redundant = True
                    break
            if redundant:
                continue
            kept_spans.setdefault(f, {})[(lo, hi)] = None
        kept.append(i)
    return kept


def span_select_one(scores, rows, files, los, his, k: int, permille: int):
    """One query: (pos i32 [k], rows i64 [k], scores f32 [k], file i32 [k], lo i32 [k], hi i32 [k], info i32 [2])."""
    c = int(scores.shape[0])
    assert 1 <= k <= c and 0 <= permille <= 1000
    rows = np.asarray(rows, np.int64)
    real = np.flatnonzero(rows >= 0)
    kept = real[np.asarray(walk(files[real], los[real], his[real], permille), np.int64)] if real.size else real
    at = kept[:k]
    out_pos, out_rows, out_s = np.full((k,), -1, np.int32), np.full((k,), -1, np.int64), np.full((k,), -np.inf, F32)
    out_f, out_lo, out_hi = (np.full((k,), -1, np.int32) for _ in range(3))
    n = at.size
    out_pos[:n], out_rows[:n], out_s[:n] = at, rows[at], np.asarray(scores, F32)[at]
    out_f[:n], out_lo[:n], out_hi[:n] = files[at], los[at], his[at]
    return out_pos, out_rows, out_s, out_f, out_lo, out_hi, np.asarray([int(kept.size), int(real.size)], np.int32)


def span_select(scores, rows, files, los, his, k, permille, **_):
    """The restatement with the call shape of ``ffi.span_select`` on host arrays: five [nq, c] arrays -> (pos, rows, scores, file,
    lo, hi) each [nq, k] and info [nq, 2]."""
    scores, rows = np.asarray(scores, F32), np.asarray(rows, np.int64)
    files, los, his = (np.asarray(a, np.int32) for a in (files, los, his))
    nq = scores.shape[0]
    outs = (np.full((nq, k), -1, np.int32), np.full((nq, k), -1, np.int64), np.full((nq, k), -np.inf, F32), np.full((nq, k), -1, np.int32),
            np.full((nq, k), -1, np.int32), np.full((nq, k), -1, np.int32), np.zeros((nq, 2), np.int32))
    for q in range(nq):
        for o, v in zip(outs, span_select_one(scores[q], rows[q], files[q], los[q], his[q], k, permille)):
            o[q] = v
    return outs


def plain_order(corpus_pre, query_pre, passing=None):
    """Every passing row of the corpus in the order of the plain search: (scores f32 [m], rows i64 [m]) from the oracle at k = n."""
    n = corpus_pre.shape[0]
    alive = None if passing is None else np.asarray(passing, np.uint8)
    s, r = orc.search(corpus_pre, np.asarray(query_pre, F32).reshape(1, -1), n, alive=alive)
    return s[0][r[0] >= 0], r[0][r[0] >= 0]


def brute_force(corpus_pre, query_pre, files, los, his, limit: int, permille: int, passing=None, order=None):
    """The definition itself for one query: score the WHOLE corpus with the oracle (k = n: every passing row, in the plain
    order) and walk it.  ``passing``: boolean [n], the rows that are alive and pass the filter; ``order``: :func:`plain_order` of
    the same arguments, computed once by a caller that walks it several times.  Returns (scores f32 [<= limit], rows i64
    [<= limit], kept rows of the whole corpus)."""
    s, r = plain_order(corpus_pre, query_pre, passing) if order is None else order
    kept = np.asarray(walk(files[r], los[r], his[r], permille), np.int64)
    return s[kept[:limit]], r[kept[:limit]], int(kept.size)


def candidate_lists(corpus_pre, queries_pre, files, los, his, c, passing=None):
    """Candidate lists as ``crh_search`` returns them plus the three gathered columns (-1 at padding)."""
    alive = None if passing is None else np.asarray(passing, np.uint8)
    s, r = orc.search(corpus_pre, np.atleast_2d(queries_pre), c, alive=alive)
    cols = [np.where(r >= 0, np.asarray(a, np.int32)[np.clip(r, 0, None)], -1).astype(np.int32) for a in (files, los, his)]
    return (s, r, *cols)


def np_mask(codes, alive, conds):
    """The rows a filter keeps: every condition -- ``(col, code)``, ``(col, codes, negate)`` or ``(col, lo, hi, "between" |
    "not_between")`` -- AND the alive bits.  A row whose value is negative is inside no range."""
    ok = np.asarray(alive, bool).copy()
    for c in conds or []:
        v = codes[:, c[0]].astype(np.int64)
        if len(c) == 4:
            member = (v >= 0) & (v >= int(c[1])) & (v <= int(c[2]))
            ok &= member if c[3] == "between" else ~member
        elif len(c) == 2 and isinstance(c[1], (int, np.integer)):
            ok &= v == c[1]
        else:
            member = np.isin(v, np.asarray([x for x in c[1] if x >= 0], np.int64))
            ok &= ~member if (len(c) == 3 and c[2]) else member
    return ok


def spans_corpus(dim: int = 64, seed: int = 7, files: int = 40, keyless: int = 60, hot_copies: int = 1100):
    """A seeded corpus of ``files`` files.  Each has one class span, method spans nested in it, for some methods ``_partN``-style
    neighbours that share 0-30 % of their lines with the part before, exact duplicate rows (equal vectors and equal spans: score
    ties) and a few rows with ``start_line`` only (``hi`` = -1); ``keyless`` rows carry no file.  The rows of a file lie around
    a centre of their own, so a query near one centre meets many overlapping spans.  The first method of file 0 is stored
    ``hot_copies`` times (more than ``MAX_K``: a query on it fills a 1024-candidate list with ONE span).  Shuffled.
    Returns (raw rows [n, dim], file [n], lo [n], hi [n], a row of the hot method) -- the middle three int32, -1 = absent."""
    rng = np.random.default_rng(seed)
    vec, fil, lo, hi = [], [], [], []
    for f in range(files):
        centre = rng.standard_normal(dim)

        def add(a, b, copies=1):
            v = centre + 0.6 * rng.standard_normal(dim)
            for _ in range(copies):
                vec.append(v)
                fil.append(f)
                lo.append(a)
                hi.append(b)
        top = int(rng.integers(1, 40))
        nmeth = int(rng.integers(2, 9))
        lens = rng.integers(3, 60, nmeth)
        add(top, top + int(lens.sum()) + nmeth)                       # the class
        at = top + 1
        for m in range(nmeth):
            a, b = at, at + int(lens[m]) - 1
            add(a, b, copies=hot_copies if f == 0 and m == 0 else 2 if rng.random() < 0.2 else 1)   # a method (sometimes stored twice: a tie)
            if lens[m] >= 20 and rng.random() < 0.6:                   # split into parts that share trailing lines
                half = int(lens[m]) // 2
                share = int(round(float(rng.choice([0.0, 0.1, 0.2, 0.3])) * half))
                add(a, a + half - 1)
                add(a + half - share, b)
            if rng.random() < 0.15:
                add(a, -1)                                             # start_line only
            at = b + 1
    n_file = len(vec)
    x = np.concatenate([np.asarray(vec), rng.standard_normal((keyless, dim))]).astype(F32)
    fil = np.concatenate([np.asarray(fil), np.full((keyless,), -1)]).astype(np.int32)
    lo = np.concatenate([np.asarray(lo), rng.integers(1, 50, keyless)]).astype(np.int32)       # (lines without a file: no span)
    hi = np.concatenate([np.asarray(hi), rng.integers(50, 90, keyless)]).astype(np.int32)
    perm = rng.permutation(n_file + keyless)
    return x[perm], fil[perm], lo[perm], hi[perm], int(np.flatnonzero(perm == 1)[0])      # (row 1 before the shuffle: file 0's first method)


def rounds_corpus(kind: str, dim: int = 384, seed: int = 13, others: int = 1500):
    """The three corpora of the exactness rounds, for ``limit 10 / max_overlap 0.5 / candidates 40`` (``limit`` 5 for "short").
    File 0 is the hot one: its rows have cosine 0.9 .. 0.99 to the query and all carry the span 10..50, every other row at most
    0.5 and a span of its own file, so the walk keeps ONE hot row and every other row.
      "round1":  hot = 2     -- the first 40 hits hold ten kept rows already
      "round2":  hot = 100   -- more than the 40 candidates of round 1, well inside the 1024 of round 2
      "short":   hot = 2000 exact copies of ONE row, the query is that row -- 1024 candidates keep one row: the answer is short
    Returns (raw rows [n, dim], file [n], lo [n], hi [n] int32, raw query [dim]); the rows are shuffled."""
    from tests.group_cases import _at_cosine
    hot = {"round1": 2, "round2": 100, "short": 2000}[kind]
    rng = np.random.default_rng(seed)
    q = rng.standard_normal(dim)
    q /= np.linalg.norm(q)
    if kind == "short":
        hot_rows = np.repeat(_at_cosine(rng, q, np.asarray([0.95])), hot, axis=0)
    else:
        hot_rows = _at_cosine(rng, q, np.linspace(0.99, 0.9, hot))
    x = np.concatenate([hot_rows, _at_cosine(rng, q, rng.permutation(np.linspace(0.5, -0.2, others)))])
    files = np.concatenate([np.zeros((hot,), np.int32), 1 + np.arange(others, dtype=np.int32) % 50])
    lo = np.concatenate([np.full((hot,), 10, np.int32), (100 * (np.arange(others) // 50)).astype(np.int32)])      # (a file's spans are disjoint)
    hi = np.concatenate([np.full((hot,), 50, np.int32), lo[hot:] + 60])
    perm = rng.permutation(hot + others)
    query = hot_rows[0].copy() if kind == "short" else (3.0 * q).astype(F32)
    return x[perm], files[perm], lo[perm], hi[perm], query


def payloads(files, los, his, lang=None):
    """One payload per row: ``file_path`` absent where the file is -1, ``start_line`` / ``end_line`` absent where they are -1."""
    out = []
    for i, (f, a, b) in enumerate(zip(files, los, his)):
        p = {"entity_type": "function", "entity_name": f"ent{i}", "language": ("python", "go", "rust")[int(lang[i])] if lang is not None else "python",
             "content": f"def ent{i}(): pass", "graph_node_id": f"mod.ent{i}", "content_hash": "h", "project_name": "p"}
        if f >= 0:
            p["file_path"] = f"/proj/f{int(f)}.py"
        if a >= 0:
            p["start_line"] = int(a)
        if b >= 0:
            p["end_line"] = int(b)
        out.append(p)
    return out


def strip_to_format4(directory: str, collection: str = "code_chunks") -> int:
    """Turn a store snapshot written with numeric columns back into what the code before them wrote: ``collection.json`` says
    format 4 and names no numeric keys, and every shard's code image keeps its first ``len(keys)`` columns -- ``codes.i32`` is
    columnar, so the old file is a prefix of the new one (``index.json`` patched to match); a fake index's ``fake_codes.npy``
    loses its last columns.  Returns the number of columns kept."""
    import json
    import os
    root = os.path.join(directory, collection)
    with open(os.path.join(root, "collection.json")) as f:
        meta = json.load(f)
    assert meta["format"] == 5 and meta["numeric_keys"]
    keep = len(meta["keys"])
    del meta["numeric_keys"]
    meta["format"] = 4
    with open(os.path.join(root, "collection.json"), "w") as f:
        json.dump(meta, f)
    shards = [root] if int(meta.get("shards", 1)) == 1 else [os.path.join(root, f"shard{s}") for s in range(int(meta["shards"]))]
    for sub in shards:
        fake = os.path.join(sub, "fake_codes.npy")
        if os.path.exists(fake):
            np.save(fake, np.ascontiguousarray(np.load(fake)[:, :keep]))
            continue
        with open(os.path.join(sub, "index.json")) as f:
            im = json.load(f)
        nbytes = keep * int(im["tiles"]) * 32 * 4
        with open(os.path.join(sub, "codes.i32"), "r+b") as f:
            f.truncate(nbytes)
        im["n_code_cols"] = keep
        im["sizes"]["codes.i32"] = nbytes
        with open(os.path.join(sub, "index.json"), "w") as f:
            json.dump(im, f)
    return keep
