"""CPU restatement of the diversity-aware top-k (``crh_mmr_select``; DESIGN.md, "Diversity-aware top-k") and the inputs its
tests share.  Test infrastructure only -- the checker of both tiers.

The definition, per query: candidates ``0..C-1`` as a search returns them (scores f32 descending, padding ``(-inf, -1)`` at the
end), their stored vectors, ``diversity`` in [0, 1], ``k <= C``.  ``rel[c]`` = the candidate's score; ``sim(c, s)`` = the
CANONICAL dot of the two rows -- the C oracle's sequential chain (``orc.search`` of the picked row against the candidate rows,
un-sorted by the returned rows), never numpy's.  Pick 1 is position 0; pick ``t > 1`` maximises, over the real candidates not
yet picked, ``obj = lam * rel - diversity * pen`` with ``lam = 1 - diversity`` and ``pen`` = the largest ``sim`` to a picked
row -- every operation a separately rounded ``np.float32`` one; ties go to the lower position.  Padding is never picked (a
list whose position 0 is padding is empty); the tail of a short result is ``(pos -1, row -1, score -inf, obj -inf)``.
"""
import numpy as np

from oracle import search as orc

F32 = np.float32


def canonical_sims(cand_vecs: np.ndarray, picked: np.ndarray) -> np.ndarray:
    """sim(c, picked) for every candidate row, f32 [C]: one oracle search with k = C, put back in candidate order."""
    c = cand_vecs.shape[0]
    s, r = orc.search(np.ascontiguousarray(cand_vecs, dtype=F32), np.ascontiguousarray(picked, dtype=F32).reshape(1, -1), c)
    out = np.empty((c,), F32)
    out[r[0]] = s[0]
    return out


def mmr_one(scores: np.ndarray, rows: np.ndarray, vecs: np.ndarray, k: int, diversity: float):
    """One query: (pos i32 [k], rows i64 [k], scores f32 [k], obj f32 [k])."""
    c = int(scores.shape[0])
    assert 1 <= k <= c
    rel = np.asarray(scores, F32)
    d = F32(diversity)
    lam = F32(1.0) - d
    out_pos, out_rows = np.full((k,), -1, np.int32), np.full((k,), -1, np.int64)
    out_s, out_o = np.full((k,), -np.inf, F32), np.full((k,), -np.inf, F32)
    avail = np.asarray(rows) >= 0
    if not avail[0]:
        return out_pos, out_rows, out_s, out_o
    pen = np.full((c,), -np.inf, F32)
    pick, pobj = 0, lam * rel[0]
    for t in range(k):
        out_pos[t], out_rows[t], out_s[t], out_o[t] = pick, rows[pick], rel[pick], pobj
        avail[pick] = False
        if t + 1 == k or not avail.any():
            break
        sim = canonical_sims(vecs, vecs[pick])
        pen = np.where(sim > pen, sim, pen).astype(F32)
        with np.errstate(invalid="ignore"):
            a = (lam * rel).astype(F32)
            b = (d * pen).astype(F32)
            obj = (a - b).astype(F32)
        best = -1
        for i in np.flatnonzero(avail):                     # the largest objective, ties to the lower position
            if best < 0 or obj[i] > obj[best]:
                best = int(i)
        pick, pobj = best, obj[best]
    return out_pos, out_rows, out_s, out_o


def mmr_select(scores, rows, vecs, k, diversity, **_):
    """The restatement with the call shape of ``ffi.mmr_select`` on host arrays: [nq, C], [nq, C], [nq, C, dim] ->
    (pos, rows, scores, obj), each [nq, k]."""
    scores, rows, vecs = np.asarray(scores, F32), np.asarray(rows, np.int64), np.asarray(vecs, F32)
    nq = scores.shape[0]
    outs = (np.full((nq, k), -1, np.int32), np.full((nq, k), -1, np.int64), np.full((nq, k), -np.inf, F32), np.full((nq, k), -np.inf, F32))
    for q in range(nq):
        for o, v in zip(outs, mmr_one(scores[q], rows[q], vecs[q], k, diversity)):
            o[q] = v
    return outs


def mmr_fp64(scores, rows, vecs, k, diversity):
    """Independent fp64 greedy (numpy dots): the positions picked, for inputs whose objectives are well separated."""
    rel, x = np.asarray(scores, np.float64), np.asarray(vecs, np.float64)
    avail = np.asarray(rows) >= 0
    picks = []
    pen = np.full(rel.shape, -np.inf)
    pick = 0 if avail[0] else -1
    while pick >= 0 and len(picks) < k:
        picks.append(pick)
        avail[pick] = False
        if not avail.any():
            break
        pen = np.maximum(pen, x @ x[pick])
        obj = np.where(avail, (1.0 - diversity) * rel - diversity * pen, -np.inf)
        pick = int(np.argmax(obj))
    return picks


def random_rows(n: int, dim: int, seed: int, bf16: bool) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return orc.preprocess(rng.standard_normal((n, dim)).astype(F32), to_bf16=bf16)


def clustered(dim: int = 768, seed: int = 5, bf16: bool = True, centres: int = 40, copies: int = 8, noise: float = 1e-3, dups: int = 16):
    """40 centres x 8 copies with noise of relative size 1e-3, plus exact duplicates of some rows: raw rows [n, dim] (not yet
    preprocessed), the centre of every row [n], and a raw query mixing four centres.  Near-duplicates put many objectives
    within rounding of each other; identical vectors give identical ``sim`` bits and equal objectives."""
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((centres, dim)).astype(F32)
    cen /= np.linalg.norm(cen, axis=1, keepdims=True)
    x = np.repeat(cen, copies, axis=0) + (noise / np.sqrt(dim)) * rng.standard_normal((centres * copies, dim)).astype(F32)
    which = np.repeat(np.arange(centres), copies)
    src = rng.choice(len(x), dups, replace=False)
    x = np.concatenate([x, x[src]]).astype(F32)
    which = np.concatenate([which, which[src]])
    perm = rng.permutation(len(x))
    x, which = x[perm], which[perm]
    q = (cen[0] * 1.0 + cen[1] * 0.9 + cen[2] * 0.8 + cen[3] * 0.7).astype(F32)
    return x, which, q


def candidate_lists(corpus_pre: np.ndarray, queries_pre: np.ndarray, c: int, real: int | None = None):
    """Candidate lists as ``crh_search`` returns them, made by the oracle: (scores [nq, c], rows [nq, c], vecs [nq, c, dim]);
    ``real`` < c keeps that many and pads the rest with (-inf, -1) and zero vectors."""
    n = corpus_pre.shape[0]
    take = min(c if real is None else real, n)
    s, r = orc.search(corpus_pre, np.atleast_2d(queries_pre), take)
    nq = s.shape[0]
    scores, rows = np.full((nq, c), -np.inf, F32), np.full((nq, c), -1, np.int64)
    scores[:, :take], rows[:, :take] = s, r
    vecs = np.where((rows >= 0)[:, :, None], corpus_pre[np.clip(rows, 0, None)], F32(0)).astype(F32)
    return scores, rows, vecs
