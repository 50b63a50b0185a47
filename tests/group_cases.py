"""CPU restatement of the capped walk (``crh_group_select``; DESIGN.md 3.13, "Per-group cap"), the brute-force definition of
the grouped top-k it serves, and the inputs the tests of both tiers share.  Test infrastructure only -- the checker of both tiers.

The definition, per query: all alive rows that pass the filter in the order of the plain search (score descending, ties by
lower global row).  A row's GROUP is its code in the ``group_by`` column, its RANK IN ITS GROUP the number of earlier rows of
that order with the same code.  The grouped top-``limit`` with cap ``S`` = the first ``limit`` rows whose rank in their group
is < ``S``.  A row with a negative code (-1: the key is absent) belongs to no group and is never capped.

``crh_group_select`` is that walk over one candidate list of ``c`` entries (padding ``(-inf, -1)`` at the end; padding neither
counts nor is kept): the first ``k`` kept candidates in list order -- position, row, the score's bits, code -- the tail
``(-1, -1, -inf, -1)``, and ``info = (kept in the WHOLE list, real candidates)``.
"""
import numpy as np

from oracle import search as orc

F32 = np.float32


def group_select_one(scores: np.ndarray, rows: np.ndarray, codes: np.ndarray, k: int, group_size: int):
    """One query: (pos i32 [k], rows i64 [k], scores f32 [k], codes i32 [k], info i32 [2])."""
    c = int(scores.shape[0])
    assert 1 <= k <= c and group_size >= 1
    rows, codes = np.asarray(rows, np.int64), np.asarray(codes, np.int32)
    real = rows >= 0
    grouped = real & (codes >= 0)
    same = (codes[:, None] == codes[None, :]) & grouped[None, :] & np.tri(c, c, -1, dtype=bool)       # [i, j]: j < i, j real, same code
    rank = same.sum(1)
    keep = real & (~grouped | (rank < group_size))
    at = np.flatnonzero(keep)[:k]
    out_pos, out_rows = np.full((k,), -1, np.int32), np.full((k,), -1, np.int64)
    out_s, out_c = np.full((k,), -np.inf, F32), np.full((k,), -1, np.int32)
    out_pos[:at.size], out_rows[:at.size], out_s[:at.size], out_c[:at.size] = at, rows[at], np.asarray(scores, F32)[at], codes[at]
    return out_pos, out_rows, out_s, out_c, np.asarray([int(keep.sum()), int(real.sum())], np.int32)


def group_select(scores, rows, codes, k, group_size, **_):
    """The restatement with the call shape of ``ffi.group_select`` on host arrays: three [nq, c] arrays ->
    (pos, rows, scores, codes) each [nq, k] and info [nq, 2]."""
    scores, rows, codes = np.asarray(scores, F32), np.asarray(rows, np.int64), np.asarray(codes, np.int32)
    nq = scores.shape[0]
    outs = (np.full((nq, k), -1, np.int32), np.full((nq, k), -1, np.int64), np.full((nq, k), -np.inf, F32), np.full((nq, k), -1, np.int32),
            np.zeros((nq, 2), np.int32))
    for q in range(nq):
        for o, v in zip(outs, group_select_one(scores[q], rows[q], codes[q], k, group_size)):
            o[q] = v
    return outs


def brute_force(corpus_pre: np.ndarray, query_pre: np.ndarray, group_codes: np.ndarray, limit: int, group_size: int, passing=None):
    """The definition itself for one query: score the WHOLE corpus with the oracle (k = n: every passing row, in the plain
    order), walk it with one counter per group.  ``passing``: boolean [n], the rows that are alive and pass the filter.
    Returns (scores f32 [<= limit], rows i64 [<= limit])."""
    n = corpus_pre.shape[0]
    alive = None if passing is None else np.asarray(passing, np.uint8)
    s, r = orc.search(corpus_pre, np.asarray(query_pre, F32).reshape(1, -1), n, alive=alive)
    seen: dict[int, int] = {}
    out_s, out_r = [], []
    for sc, row in zip(s[0], r[0]):
        if row < 0 or len(out_r) == limit:
            break
        g = int(group_codes[row])
        if g >= 0:
            if seen.get(g, 0) >= group_size:
                continue
            seen[g] = seen.get(g, 0) + 1
        out_s.append(sc)
        out_r.append(int(row))
    return np.asarray(out_s, F32), np.asarray(out_r, np.int64)


def candidate_lists(corpus_pre, queries_pre, group_codes, c, passing=None):
    """Candidate lists as ``crh_search`` returns them plus the gathered codes: (scores [nq, c], rows [nq, c], codes [nq, c])."""
    alive = None if passing is None else np.asarray(passing, np.uint8)
    s, r = orc.search(corpus_pre, np.atleast_2d(queries_pre), c, alive=alive)
    codes = np.where(r >= 0, np.asarray(group_codes, np.int32)[np.clip(r, 0, None)], -1).astype(np.int32)
    return s, r, codes


def files_corpus(dim: int = 64, seed: int = 3, files: int = 40, lo: int = 1, hi: int = 300, dup_across: int = 40, dup_within: int = 40,
                 keyless: int = 60):
    """A seeded corpus of ``files`` files with ``lo..hi`` rows each, shuffled; ``dup_across`` rows are exact copies of rows of
    OTHER files and ``dup_within`` of rows of their own file (equal scores: ties in the order); ``keyless`` rows carry no file
    (code -1).  Returns (raw rows [n, dim], file code of every row [n] int32, second column (a "language" 0..2) [n] int32)."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(lo, hi + 1, files)
    which = np.repeat(np.arange(files, dtype=np.int32), sizes)
    x = rng.standard_normal((which.size, dim)).astype(F32)
    src = rng.choice(which.size, dup_across + dup_within, replace=False)
    extra = x[src].copy()
    extra_file = which[src].copy()
    extra_file[:dup_across] = (extra_file[:dup_across] + 1 + rng.integers(0, files - 1, dup_across)) % files
    x = np.concatenate([x, extra, rng.standard_normal((keyless, dim)).astype(F32)])
    which = np.concatenate([which, extra_file.astype(np.int32), np.full((keyless,), -1, np.int32)])
    perm = rng.permutation(which.size)
    x, which = x[perm], which[perm]
    return x, which, rng.integers(0, 3, which.size).astype(np.int32)


def _at_cosine(rng, q_unit: np.ndarray, cos: np.ndarray) -> np.ndarray:
    """Unit rows whose cosine to ``q_unit`` is ``cos`` (up to f32 rounding)."""
    u = rng.standard_normal((cos.size, q_unit.size))
    u -= np.outer(u @ q_unit, q_unit)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (cos[:, None] * q_unit[None, :] + np.sqrt(1.0 - cos[:, None] ** 2) * u).astype(F32)


def rounds_corpus(kind: str, dim: int = 768, seed: int = 11, files: int = 30, others: int = 1500):
    """The three corpora of the exactness rounds, for ``limit 10 / group_size 3 / candidates 40``.  File 0 is the hot one: its
    ``hot`` rows have cosine 0.9 .. 0.99 to the query and every other row at most 0.5, so bf16 rounding cannot reorder the two
    classes (the cosines inside a class are all different: no duplicates).
      "exclusion": hot = 1100 > MAX_K -- both searches return nothing but the hot file: an exclusion round is needed
      "round2":    hot = 100  -- more than the 40 candidates of round 1, well inside the 1024 of round 2
      "round1":    hot = 2    -- the first 40 hits hold ten rows of the cap already
    Returns (raw rows [n, dim], file of every row [n], raw query [dim]); the rows are shuffled."""
    hot = {"exclusion": 1100, "round2": 100, "round1": 2}[kind]
    rng = np.random.default_rng(seed)
    q = rng.standard_normal(dim)
    q /= np.linalg.norm(q)
    cos_hot = np.linspace(0.99, 0.9, hot)
    cos_other = rng.permutation(np.linspace(0.5, -0.2, others))
    x = np.concatenate([_at_cosine(rng, q, cos_hot), _at_cosine(rng, q, cos_other)])
    which = np.concatenate([np.zeros((hot,), np.int32), rng.integers(1, files, others).astype(np.int32)])
    perm = rng.permutation(which.size)
    return x[perm], which[perm], (3.0 * q).astype(F32)
