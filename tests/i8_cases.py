"""Corpora, queries and the fp64 / f32 models of the int8 nomination's interval arithmetic (code-rag_amd/csrc/crh_i8.hpp).

Shared by tests/test_i8_intervals_host.py (no GPU: the header's algebra, and the kernels' f32 evaluation restated in numpy) and
tests/test_i8_intervals_gpu.py (the product kernels' own numbers against the oracle).  Plain numpy, seeded.  Every kind of row and
query names the allowance or branch of crh_i8.hpp it aims at.

What the kernels do, in the header's symbols:  x_i = s_r (X_i + d_i), X = rint(x * 127 / max|x|), s_r = max|x| / 127 per stored row;
q_i = s_q (Q_i + g_i), Q = rint(q * 16256 / max|q|), s_q = max|q| / 16256 per canonical query;  dot = X . Q in integers;
    | x.q - s_r s_q dot | <= s_r s_q B,   B = dn (|Q|_2 + |g|_2) + 127 sqrt(D) |g|_2,   dn >= |d|_2 of every row.
"""
from __future__ import annotations

import os
import re
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = 16256.0                     # kI8QueryLevels
NQS = (1, 31, 32, 33, 64)            # 32 is the edge between one and two 32-query blocks; short blocks leave padding slots
KS = (1, 10, 100, 256)


def scan_dims() -> dict:
    """{dim: query blocks per pass} of the k_scan_i8 instantiations, read from the dispatch in crh_index.hip.  The block count picks
    the branch of intervals(): 2 = pairs of query blocks, 1 = pairs of rows.  (It goes with the DIMENSION: a 1536-wide index takes
    32 queries per pass and always runs the row-pair branch, every other width always runs the block-pair branch.)"""
    src = open(os.path.join(ROOT, "code-rag_amd", "csrc", "crh_index.hip")).read()
    got = {int(d): int(qb) for d, qb in re.findall(r"case (\d+): CRH_I8\(\d+, \w+, (\d)\); break;", src)}
    assert got, "the int8 dispatch of crh_index.hip was not found"
    return got


def dot_round(dim: int) -> float:
    """kDotRound of k_scan_i8 for this width."""
    return 128.0 if dim <= 1024 else 512.0


def c_abs(dim: int) -> np.float32:
    """The allowance for the canonical score's own f32 summation order (crh_index.hip, i8_c_abs), in the host's f32 operations."""
    f = np.float32
    return f(f(1.5e-4) * (f(dim) / f(768.0) if dim > 768 else f(1.0))) + f(1e-5)


def bf16_round(a: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


# ------------------------------------------------------------------ adversarial constructions
def _odd_with_square_sum(total: int, count: int, amax: int, rng) -> np.ndarray:
    """`count` odd integers in [1, amax] whose squares sum to `total` (needs total = count mod 8: odd squares are 1 mod 8)."""
    assert total % 8 == count % 8 and count <= total <= count * amax * amax
    mid = int(np.sqrt(total / count)) | 1
    a = np.clip(mid + 2 * rng.integers(-20, 21, count), 1, amax).astype(np.int64)
    rest = total - int((a * a).sum())
    for _ in range(200_000):                             # single steps a -> a +- 2 (the sum moves by 4 a +- 4) while they fit
        if abs(rest) <= 4 * amax:
            break
        i = int(rng.integers(count))
        up, down = 4 * int(a[i]) + 4, 4 * int(a[i]) - 4
        if rest > 0 and a[i] + 2 <= amax and up <= rest:
            a[i] += 2
            rest -= up
        elif rest < 0 and a[i] >= 3 and down <= -rest:
            a[i] -= 2
            rest += down
    for _ in range(64):                                  # pairs: a_i up, a_j down moves the sum by 4 (a_i - a_j) + 8
        if rest == 0:
            break
        want = int(np.clip((rest - 8) // 4, -40, 40))
        where = {int(v): j for j, v in enumerate(a) if v >= 3}
        for i, v in enumerate(a):
            j = where.get(int(v) - want)
            if j is not None and j != i and v + 2 <= amax:
                a[i] += 2
                a[j] -= 2
                rest -= 4 * want + 8
                break
    assert rest == 0 and int((a * a).sum()) == total and a.min() >= 1 and a.max() <= amax and np.all(a % 2 == 1), "no half-step pattern found"
    return rng.permutation(a)


def halfstep_rows(dim: int, n: int, rng) -> np.ndarray:
    """HALF-STEP ROWS (aims at dn, the `dn * 1.0001 + 2e-3` allowance and the dn (|Q| + gn) term): x_i = +-a_i 2^-11 with a_i odd
    <= 253 except for one element 254 (the maximum) and three elements 4 (the sum of D - 4 odd squares is 4 mod 8; the four even
    ones bring it to 0), sum a_i^2 = 2^22.  The f32 sum of squares is exact and equal to 1, so the row is stored as it is, in f32
    and (8-bit significands) in bf16; x_i * 127 / max|x| = a_i / 2 is a half-integer for the odd ones, rint rounds it to even and
    |d_i| = 1/2 EXACTLY: |d|_2 = 0.5 sqrt(D - 4), i.e. sqrt(1 - 4/D) = 0.9948 (D = 384) .. 0.9987 (D = 1536) of the 0.5 sqrt(D) no row
    can pass.  (Four patterns per call; the rows are their permutations under random signs.)"""
    base = [np.concatenate([_odd_with_square_sum((1 << 22) - 254 * 254 - 3 * 16, dim - 4, 253, rng), [254, 4, 4, 4]]) for _ in range(4)]
    out = np.empty((n, dim), np.float32)
    for r in range(n):
        out[r] = (rng.permutation(base[r % 4]) * rng.choice([-1.0, 1.0], dim)) * 2.0 ** -11
    return out


def halfstep_eps_rows(dim: int, n: int, rng) -> np.ndarray:
    """Half-step rows off the tie: x_i * 127 / max|x| = n_i + 0.5 - 2^-9 (any norm: normalised on insert, which moves the images by
    ~1e-5).  An f32 store keeps |d_i| = 0.498; a bf16 store rounds them to something ordinary."""
    y = rng.integers(0, 127, (n, dim)) + 0.5 - 2.0 ** -9
    y[np.arange(n), rng.integers(0, dim, n)] = 127.0
    return (y * rng.choice([-1.0, 1.0], (n, dim))).astype(np.float32)


def halfstep_query(dim: int, rng) -> np.ndarray:
    """HALF-STEP QUERY in the 16256-level grid (aims at gn, `gn * 1.001 + 0.25` and the 127 sqrt(D) gn term): q_i = +-a_i 2^-15 with
    a_i odd <= 255, three elements 2 and the LAST element 32512 (= 16256 half-steps; the even ones for the same reason as in
    halfstep_rows), sum a_i^2 = 2^30.  Summed in index order the small squares stay below 2^-6 and exact, the last addition gives
    1.0: the query is its own canonical form, in f32 and in bf16, and q_i * 16256 / max|q| = a_i / 2: |g_i| = 1/2 exactly on
    D - 4 elements, |g|_2 = 0.5 sqrt(D - 4)."""
    a = np.concatenate([_odd_with_square_sum((1 << 30) - 32512 * 32512 - 3 * 4, dim - 4, 255, rng), [2, 2, 2]])
    q = np.append(rng.permutation(a) * rng.choice([-1.0, 1.0], dim - 1), 32512.0) * 2.0 ** -15
    return q.astype(np.float32)


def residual_signs(stored_row: np.ndarray) -> np.ndarray:
    """The saturated query along a stored row's quantisation residual: sign(d_i).  Its own g is 0 and Q is parallel to d, so
    |d . Q| = |d|_2 |Q|_2 -- the Cauchy-Schwarz step of the bound holds with equality."""
    x = stored_row.astype(np.float64)
    y = x * 127.0 / np.abs(x).max()
    d = y - np.rint(y)
    return np.where(d >= 0, 1.0, -1.0).astype(np.float32)


ROW_KINDS = ("gaussian", "spike", "onehot", "zero", "tiny", "saturated", "halfstep", "halfstep_eps")
_MIX = (0.40, 0.05, 0.03, 0.02, 0.03, 0.25, 0.12, 0.10)


def rows_of_kind(kind: str, dim: int, n: int, rng, signs: np.ndarray) -> np.ndarray:
    if kind == "gaussian":                       # the header's own figures (half-width 0.23 sigma)
        return rng.standard_normal((n, dim), dtype=np.float32)
    if kind == "spike":                          # max|x| ~ the norm: the largest s_r a unit row can have, the widest intervals
        x = rng.standard_normal((n, dim), dtype=np.float32) * np.float32(0.01 / np.sqrt(dim))
        x[np.arange(n), rng.integers(0, dim, n)] = rng.choice([-1.0, 1.0], n)
        return x
    if kind == "onehot":                         # d = 0: the interval is the query's share alone
        x = np.zeros((n, dim), np.float32)
        x[np.arange(n), rng.integers(0, dim, n)] = rng.choice([-2.5, 0.7, 1.0], n)
        return x
    if kind == "zero":                           # scale 0: [-c, c]
        return np.zeros((n, dim), np.float32)
    if kind == "tiny":                           # below the normalisation's epsilon: stored as they are, s_r ~ 3e-22
        return rng.standard_normal((n, dim), dtype=np.float32) * np.float32(1e-20)
    if kind == "saturated":                      # every element +-max, 0..39 sign flips off a query's pattern: |dot| up to 127 * 16256 * D (kDotRound)
        x = signs[rng.integers(0, len(signs), n)].copy()
        for i, f in enumerate(rng.integers(0, 40, n)):
            if f:
                x[i, rng.choice(dim, f, replace=False)] *= -1.0
        x[::7] *= -1.0
        return x * rng.choice([1.0, 3.0, 1e-3], (n, 1)).astype(np.float32)
    if kind == "halfstep":
        return halfstep_rows(dim, n, rng)
    if kind == "halfstep_eps":
        return halfstep_eps_rows(dim, n, rng)
    raise KeyError(kind)


def sign_pool(dim: int, seed: int) -> np.ndarray:
    return np.random.default_rng(1000 + seed).choice([-1.0, 1.0], (8, dim)).astype(np.float32)


def mixed_corpus(dim: int, n: int, seed: int):
    """Every kind of row, shuffled so that each 32-row tile mixes them.  Returns (raw rows [n, dim] f32, kind index [n])."""
    rng = np.random.default_rng(seed)
    counts = [int(n * f) for f in _MIX]
    counts[0] += n - sum(counts)
    signs = sign_pool(dim, seed)
    x = np.concatenate([rows_of_kind(k, dim, c, rng, signs) for k, c in zip(ROW_KINDS, counts)])
    kind = np.concatenate([np.full(c, i, np.int32) for i, c in enumerate(counts)])
    order = rng.permutation(n)
    return np.ascontiguousarray(x[order]), kind[order]


QUERY_KINDS = ("residual", "halfstep", "gaussian", "outlier", "zero", "saturated", "equal_row", "negated_row")


def queries_for(dim: int, nq: int, seed: int, raw: np.ndarray, kind: np.ndarray, stored: np.ndarray):
    """nq queries cycling through QUERY_KINDS.  `stored`: the rows as the index keeps them (for the residual-aligned queries)."""
    rng = np.random.default_rng(7000 + seed)
    signs = sign_pool(dim, seed)
    hs = np.flatnonzero(kind == ROW_KINDS.index("halfstep"))
    q = np.empty((nq, dim), np.float32)
    names = []
    for i in range(nq):
        name = QUERY_KINDS[i % len(QUERY_KINDS)]
        if name == "halfstep":                   # largest gn
            q[i] = halfstep_query(dim, rng)
        elif name == "gaussian":
            q[i] = rng.standard_normal(dim, dtype=np.float32)
        elif name == "outlier":                  # one element 40 x the rest: s_q large, most Q_i small
            q[i] = rng.standard_normal(dim, dtype=np.float32)
            q[i, rng.integers(dim)] = 40.0
        elif name == "zero":                     # scale 0, gn = 0
            q[i] = 0.0
        elif name == "saturated":                # g = 0, |Q|_2 = 16256 sqrt(D): with the saturated rows, the largest integer dots
            q[i] = signs[(i // len(QUERY_KINDS)) % len(signs)] * np.float32(0.37)
        elif name == "residual":                 # parallel to a half-step row's d
            src = hs[(i // len(QUERY_KINDS)) % len(hs)] if len(hs) else int(rng.integers(len(raw)))
            q[i] = residual_signs(stored[src]) * np.float32(0.5)
        elif name == "equal_row":                # score 1 (or the row's squared norm): the top of every list
            q[i] = raw[int(rng.integers(len(raw)))]
        else:                                    # ... and its negative: the bottom
            q[i] = -raw[int(rng.integers(len(raw)))]
        names.append(name)
    return q, names


# ------------------------------------------------------------------ the cases
@dataclass(frozen=True)
class Case:
    name: str
    dim: int
    bf16: bool
    n: int
    nq: int
    seed: int
    corpus: str          # "mixed" | "gaussian" | "mutated"
    aims: str

    @property
    def id(self) -> str:
        return f"{self.name}-d{self.dim}-{'bf16' if self.bf16 else 'f32'}-nq{self.nq}"


def cases() -> list:
    out = []
    dims = sorted(scan_dims())
    for di, dim in enumerate(dims):
        for bf16 in (True, False):
            for ni, nq in enumerate(NQS):
                # 12 013 rows: 376 tiles, the last one 13 rows short; > 256 sample tiles so that k = 256 has a threshold
                out.append(Case("mixed", dim, bf16, 12_013, nq, 100 * di + 10 * int(bf16) + ni, "mixed",
                                "every row and query kind; padding slots of short query blocks; the ragged last tile; tombstones and a filter"))
    for bf16 in (True, False):
        out.append(Case("gaussian", 768, bf16, 59_999, 64, 900 + int(bf16), "gaussian", "the header's stated figures; dn and gn tightness on ordinary data"))
        out.append(Case("mutated", 768, bf16, 20_011, 33, 950 + int(bf16), "mutated",
                        "dn as a running maximum: quantised, then appended rows of larger |d|_2, then compacted (lazy rebuild of the copy)"))
    return out


@lru_cache(maxsize=4)
def build_raw(case: Case):
    """(raw rows in the order the index ends up holding them, row kind index)."""
    if case.corpus == "gaussian":
        rng = np.random.default_rng(case.seed)
        return rng.standard_normal((case.n, case.dim), dtype=np.float32), np.zeros(case.n, np.int32)
    x, kind = mixed_corpus(case.dim, case.n, case.seed)
    if case.corpus == "mutated":
        first, second, dead = mutation_plan(case)
        keep = np.concatenate([np.setdiff1d(first, dead), second])
        return np.ascontiguousarray(x[keep]), kind[keep]
    return x, kind


def mutation_plan(case: Case):
    """The "mutated" case, as indices into mixed_corpus(dim, n, seed): (rows appended first -- everything but the half-step rows,
    whose |d|_2 is the largest --, rows appended after a first search has quantised those, rows of the first lot tombstoned before
    the compaction).  dn has then seen every row of the first lot, the deleted ones included."""
    kind = mixed_corpus(case.dim, case.n, case.seed)[1]
    late = np.isin(kind, [ROW_KINDS.index("halfstep"), ROW_KINDS.index("halfstep_eps")])
    rng = np.random.default_rng(case.seed + 1)
    first, second = np.flatnonzero(~late), np.flatnonzero(late)
    dead = np.sort(rng.choice(first, len(first) // 5, replace=False))
    return first, second, dead


def tombstones_and_codes(case: Case):
    """Rows deleted before the scan, and one payload column: code 1 on ~half the rows, code 2 on 50 rows (fewer than k = 100), 0 else."""
    rng = np.random.default_rng(case.seed + 5)
    n = len(build_raw(case)[0])
    dead = np.sort(rng.choice(n, n // 9, replace=False))
    codes = (rng.random(n) < 0.5).astype(np.int32)
    codes[rng.choice(n, 50, replace=False)] = 2
    return dead, codes[:, None]


# ------------------------------------------------------------------ the header's algebra, exactly (fp64 + exact integers)
def quantise(v: np.ndarray, levels: float):
    """Per vector: (scale f32 as the kernels compute it, integer image, residual) with v = scale * (image + residual) in fp64.
    The scale is the F32 quotient max|v| / levels -- the number the kernels multiply by -- and the image is the kernels'
    rint(v * (levels / max|v|)) in f32; the residual is then whatever makes the identity hold, which is what the bound must cover."""
    f = np.float32
    v32 = np.ascontiguousarray(v, dtype=np.float32)
    m = np.abs(v32).max(axis=1)
    m = np.where(np.isfinite(m), m, f(0)).astype(np.float32)
    scale = (m / f(levels)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(m > 0, f(levels) / m, f(0)).astype(np.float32)
        y32 = (v32 * inv[:, None]).astype(np.float32)
        image = np.clip(np.rint(y32), -levels, levels)
        res32 = (y32 - image).astype(np.float32)                         # the residual as the kernels see it
        exact = np.where(scale[:, None] > 0, v32.astype(np.float64) / scale.astype(np.float64)[:, None] - image, 0.0)
    return scale, image.astype(np.float64), exact, res32


def exact_dots(X: np.ndarray, Q: np.ndarray) -> np.ndarray:
    """X . Q as int64 [nq, n].  Evaluated by the fp64 matrix product: every operand is an integer (|X| <= 127, |Q| <= 16256) and
    every partial sum stays below 127 * 16256 * 1536 < 2^32, far inside the 2^53 fp64 holds exactly; checked on the way out."""
    s = Q @ X.T
    i = s.astype(np.int64)
    assert np.array_equal(i.astype(np.float64), s)
    return i


def split_hl(Q: np.ndarray):
    """Q = 128 H + L, L in [-64, 63] (prep_query_i8)."""
    H = np.floor((Q + 64.0) / 128.0)
    return H, Q - 128.0 * H


# ------------------------------------------------------------------ the kernels' f32 evaluation, restated in numpy
def fma32(a, b, c):
    """fmaf on f32 arrays: the product of two f32 is exact in fp64, the sum is rounded to fp64 and then to f32 (a double rounding
    that differs from fmaf only on exact fp64 half-way cases)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def norm_as_kernel(res32: np.ndarray, chunk: int) -> np.ndarray:
    """sqrtf of the sum of squares in a kernel's order: `lanes` partial fma chains over the elements each lane owns, then a tree."""
    f = np.float32
    n, dim = res32.shape
    if chunk == 16:          # k_requant_i8: lane half hh owns elements [32 p + 16 hh, + 16) of every piece p; two chains, one addition
        parts = res32.reshape(n, dim // 32, 2, 16).transpose(0, 2, 1, 3).reshape(n, 2, dim // 2)
    else:                    # prep_query_i8: lane l owns the 8-element groups l, l + 64, ...; 64 chains, a butterfly
        g = dim // 8
        pad = np.zeros((n, (-g) % 64 * 8), np.float32)
        parts = np.concatenate([res32, pad], axis=1).reshape(n, -1, 64, 8).transpose(0, 2, 1, 3).reshape(n, 64, -1)
    acc = np.zeros(parts.shape[:2], np.float32)
    for j in range(parts.shape[2]):
        acc = fma32(parts[:, :, j], parts[:, :, j], acc)
    while acc.shape[1] > 1:                              # __shfl_xor butterflies from the widest distance down
        half = acc.shape[1] // 2
        acc = (acc[:, :half] + acc[:, half:]).astype(f)
    return np.sqrt(acc[:, 0]).astype(f)


def dn_as_kernel(res32: np.ndarray, scale: np.ndarray) -> np.float32:
    f = np.float32
    per_row = (norm_as_kernel(res32, 16) * f(1.0001)).astype(f) + f(2e-3)
    per_row = np.where(scale > 0, per_row, f(0))
    return f(per_row.max()) if len(per_row) else f(0)


def qpar_as_kernel(Q: np.ndarray, res32: np.ndarray, scale: np.ndarray):
    f = np.float32
    Qn = (norm_as_kernel(Q.astype(np.float32), 8) * f(1.0001)).astype(f)
    gn = np.where(scale > 0, (norm_as_kernel(res32, 8) * f(1.001)).astype(f) + f(0.25), f(0)).astype(f)
    return Qn, gn


def intervals_as_kernel(dotH, dotL, s_r, s_q, Qn, gn, dn, dim):
    """(hi, lo) [nq, n] f32 as intervals() and lower_end() of k_scan_i8 evaluate them."""
    f = np.float32
    c = c_abs(dim)
    Bq = ((((f(dn) * (Qn + gn).astype(f)).astype(f) + ((f(127.0) * f(np.sqrt(f(dim)))).astype(f) * gn).astype(f)).astype(f) * f(1.0001)).astype(f)
          + f(dot_round(dim))).astype(f)
    fdot = fma32(dotH.astype(f), f(128.0), dotL.astype(f))
    w = (s_q[:, None] * s_r[None, :]).astype(f)
    hi = fma32(w, (fdot + Bq[:, None]).astype(f), c)
    w2 = (s_r[None, :] * s_q[:, None]).astype(f)
    lo = ((hi - (f(2.0) * fma32(w2, Bq[:, None], c)).astype(f)).astype(f) - f(2e-6)).astype(f)
    return hi, lo, Bq


def half_width_fp64(srow, qpar, dn, c, dim) -> np.ndarray:
    """The half-width the kernel's constants ask for, [nq, n] fp64: s_r s_q ((dn (Qn + gn) + 127 sqrt(D) gn) 1.0001 + kDotRound) + c
    (+ 1e-6: half of lower_end's 2e-6), from the parameters the kernel returned."""
    s_q, Qn, gn = (qpar[:, j].astype(np.float64) for j in range(3))
    B = (float(dn) * (Qn + gn) + 127.0 * np.sqrt(float(dim)) * gn) * 1.0001 + dot_round(dim)
    return srow.astype(np.float64)[None, :] * (s_q * B)[:, None] + float(c) + 1e-6
