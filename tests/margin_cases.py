"""Worst-case rounding inputs for the nomination margin and for cosine preprocessing (numpy only; no GPU import).

The nomination margin (margin_for)
-------------------------------------------------
An f32 store is scanned through the bf16 image of its rows and of the query, and the rows the scan nominates are re-scored
canonically (f32 operands, f32 sequential sum).  The margin has to cover |scan score - canonical score|.  bf16 keeps 8
significant bits, so rounding to it moves a value by up to 2^-8 of itself (half an ulp at the bottom of a binade) and a product
of two rounded operands by up to 2 * 2^-8 + 2^-16 of itself.  `adversarial_pair` builds unit vectors that reach two thirds of that
per row (the rest is the part of the vectors that carries no rounding error):

  lo = 1 + 2^-8 - 2^-14    bf16 rounds it DOWN to 1          (relative error -2^-8 * 0.98)
  hi = 1 + 2^-8 + 2^-14    bf16 rounds it UP   to 1 + 2^-7   (relative error +2^-8 * 0.98)

q carries a block of lo's and a block of hi's (times the power of two S, which leaves significands alone).  Row A lives on the lo
block, row B on the hi block: every product of A shrinks by about 2^-7 in the scan, every product of B grows by as much, and one
exact product (q[258] * A[258] = 2^-12) puts A ahead canonically.  The scan ranks them the other way round, about 1e-2 apart.
Every vector is topped up to unit length with a few bf16-exact fillers at positions no other vector uses, so that cosine
preprocessing leaves it bit-unchanged and the stored rows are exactly these.

Cosine preprocessing (k_append, k_prep_queries)
-----------------------------------------------
len2 = sum v_i^2 in f32, in index order, each product rounded on its own; the row is kept when len2 < FLT_EPSILON or
|len2 - 1| <= 1e-6f and divided by sqrtf(len2) otherwise.  `boundary_rows` puts rows one ulp either side of each threshold, a row
whose len2 depends on the order of the sum, rows whose len2 overflows or nearly does, a row whose quotients are subnormal, and
rows of bf16 rounding ties (stored verbatim).
"""
from typing import NamedTuple

import numpy as np

F32, U32 = np.float32, np.uint32

H = 130                                         # start of the hi block
BLOCK = 127                                     # elements per block; the row doubles the first DOUBLED of them
DOUBLED = 42
SIGNED = 20                                     # elements per block the "signed" variant turns negative
HEAD = 258                                      # the exact product that puts A ahead
S = F32(2.0 ** -4)
LO = F32(1 + 2.0 ** -8 - 2.0 ** -14)
HI = F32(1 + 2.0 ** -8 + 2.0 ** -14)
U_BF16 = 2.0 ** -8                              # unit roundoff of bf16 (8 significant bits, round to nearest even)
PRODUCT_BOUND = 2 * U_BF16 + U_BF16 ** 2        # |bf16(a) bf16(b) - a b| <= PRODUCT_BOUND * |a b|
MIN_SWING = 1.0e-2                              # how far the scan must move B against A (asserted by the host test)
UNIT_TOL = 5e-7                                 # |len2 - 1| of every vector of a pair: inside preprocessing's 1e-6
VARIANTS = ("plain", "signed")
DIMS = (384, 768, 1024, 1536)


def bf16_round(x: np.ndarray) -> np.ndarray:
    """f32 -> bf16 (round to nearest even) -> f32 on finite values."""
    u = np.ascontiguousarray(x, dtype=F32).view(U32)
    return ((u + U32(0x7fff) + ((u >> U32(16)) & U32(1))) & U32(0xffff0000)).view(F32)


def len2(v: np.ndarray) -> np.float32:
    """Squared length as preprocessing sums it: f32 products, f32 sum, index order."""
    v = np.asarray(v, dtype=F32)
    with np.errstate(over="ignore", under="ignore"):      # (the overflow row's inf and underflowing squares are meant)
        return np.cumsum(v * v, dtype=F32)[-1]


def scan_model(q: np.ndarray, x: np.ndarray) -> float:
    """What a scan over the bf16 images computes, without its accumulation error: the f64 dot of the bf16-rounded operands."""
    return float(np.dot(bf16_round(q).astype(np.float64), bf16_round(x).astype(np.float64)))


def _bf16_floor_sqrt(r: float) -> np.float32:
    """The largest bf16-exact value whose square is <= r."""
    v = bf16_round(np.asarray([np.sqrt(r)], F32))[0]
    while float(v) * float(v) > r:
        v = (np.asarray([v], F32).view(U32) - U32(0x10000)).view(F32)[0]
    return v


def _top_up(v: np.ndarray, at: int) -> None:
    """Fill v[at], v[at + 1], ... with bf16-exact values until the sequential f32 len2 is within UNIT_TOL of 1."""
    for i in range(at, at + 12):
        gap = 1.0 - float(len2(v))
        if abs(gap) <= UNIT_TOL:
            return
        assert gap > 0 and v[i] == 0, (gap, i)
        v[i] = _bf16_floor_sqrt(gap)
    assert abs(1.0 - float(len2(v))) <= UNIT_TOL, len2(v)


def adversarial_pair(dim: int, variant: str = "plain"):
    """(q, A, B, scan_model): unit f32 vectors that preprocessing leaves unchanged; canonically A scores above B for q, the scan
    over the bf16 images moves B 1.01e-2 up against A (5.06e-3 off A, 5.08e-3 onto B)."""
    assert variant in VARIANTS and dim >= 384
    q, a, b = (np.zeros((dim,), F32) for _ in range(3))
    q[0:BLOCK], q[H:H + BLOCK] = LO * S, HI * S
    a[0:BLOCK] = LO * S
    a[0:DOUBLED] = F32(2) * LO * S
    b[H:H + BLOCK] = HI * S
    b[H:H + DOUBLED] = F32(2) * HI * S
    if variant == "signed":
        # negative products: the operands that round UP go under A (its negative terms grow), those that round DOWN under B
        q[0:SIGNED], a[0:SIGNED] = HI * S, -F32(2) * HI * S
        q[H:H + SIGNED], b[H:H + SIGNED] = LO * S, -F32(2) * LO * S
    q[BLOCK - 1] = q[H + BLOCK - 1] = 0
    q[HEAD] = a[HEAD] = F32(2.0 ** -6)
    _top_up(q, dim - 36)
    _top_up(a, dim - 24)
    _top_up(b, dim - 12)
    return q, a, b, scan_model


# ---------------------------------------------------------------------------------------------- preprocessing

FLT_EPSILON = F32(2.0 ** -23)


def _ulps(x, n: int) -> np.float32:
    return (np.asarray([x], F32).view(U32) + U32(n & 0xffffffff)).view(F32)[0]


# name -> (the exact sequential len2, whether preprocessing then divides the row)
LEN2_TARGETS = {
    "eps-1ulp": (_ulps(FLT_EPSILON, -1), False),
    "eps": (FLT_EPSILON, True),
    "eps+1ulp": (_ulps(FLT_EPSILON, 1), True),
    "1-17ulp": (F32(1 - 17 * 2.0 ** -24), True),
    "1-16ulp": (F32(1 - 16 * 2.0 ** -24), False),
    "1+8ulp": (F32(1 + 8 * 2.0 ** -23), False),
    "1+9ulp": (F32(1 + 9 * 2.0 ** -23), True),
}


def row_with_len2(dim: int, target, seed: int) -> np.ndarray:
    """A dense Gaussian row (both signs, every element non-zero) whose sequential f32 len2 is `target` to the bit: scaled to
    the target, then ONE element -- the largest, a third of the way in -- is nudged in ulps until the restated sum hits it.
    len2 is a non-decreasing function of that element's magnitude and one ulp of it moves the sum by far less than an ulp of
    the sum, so nearby values of the sum are reached one by one -- except where a later addition is a tie, which rounds to even
    and can step over an odd target: then the next draw is taken.  The walk over ulps is done by bisection."""
    for draw in range(16):
        v = _nudged(dim, target, np.random.default_rng([seed, draw]))
        if v is not None:
            return v
    raise AssertionError(f"len2 {target!r} not reached at dim {dim}")


def _nudged(dim: int, target, rng):
    v = rng.standard_normal(dim).astype(F32)
    j = dim // 3
    v[j] = F32(4.0)
    v *= F32(np.sqrt(float(target)) / np.sqrt(float(np.dot(v.astype(np.float64), v.astype(np.float64)))))
    base = int(v[j:j + 1].view(U32)[0])
    lo, hi = -(1 << 21), 1 << 21                # in ulps of v[j]: a quarter of its value either way
    while lo <= hi:
        mid = (lo + hi) // 2
        v[j:j + 1].view(U32)[0] = base + mid
        got = len2(v)
        if got == target:
            return v
        if got < target:
            lo = mid + 1
        else:
            hi = mid - 1
    return None


def bf16_tie_row(dim: int) -> np.ndarray:
    """Elements whose low 16 bits are 0x7fff (just below the tie: down), 0x8000 over an even upper half (tie: down), 0x8000
    over an odd upper half (tie: up) and 0x8001 (just above: up), both signs, over upper halves that include a mantissa of all
    ones (the carry goes into the exponent).  256 elements of magnitude 2^-5 .. 2^-4: the row is shorter than a unit vector."""
    low = np.asarray([0x7fff, 0x8000, 0x8000, 0x8001], U32)
    odd = np.asarray([0, 0, 1, 0], U32)
    i = np.arange(256, dtype=U32)
    upper = U32(0x3d00) + (((i >> U32(2)) * U32(2)) & U32(0x7e))            # even upper halves 0x3d00 .. 0x3d7e
    upper = np.where(i >= 192, U32(0x3d7e), upper) | odd[i & U32(3)]          # the last 64: 0x3d7e / 0x3d7f (all ones)
    upper = np.where((i >> U32(2)) & U32(1), upper | U32(0x8000), upper)      # every other group negative
    v = np.zeros((dim,), F32)
    v[:256] = ((upper << U32(16)) | low[i & U32(3)]).view(F32)
    return v


class Boundary(NamedTuple):
    names: list                 # of the raw rows
    raw: np.ndarray             # [n, dim] f32: appended / queried as they are, preprocessing decides
    divided: np.ndarray         # [n] bool: whether preprocessing divides the row (False: kept bit for bit)
    verbatim: np.ndarray        # [m, dim] f32: appended with preprocessed=True (bf16 rounding ties)


def boundary_rows(dim: int) -> Boundary:
    names, rows, divided = [], [], []

    def add(name, v, div):
        names.append(name)
        rows.append(np.asarray(v, F32))
        divided.append(div)

    for i, (name, (target, div)) in enumerate(LEN2_TARGETS.items()):
        add(name, row_with_len2(dim, target, 100 * dim + i), div)
    v = np.zeros((dim,), F32)                   # in index order every + 2^-24 is a tie that rounds back to 1.0 (even)
    v[0], v[1:65] = 1.0, 2.0 ** -12
    add("order", v, False)
    v = np.zeros((dim,), F32)                   # finite elements, len2 = inf: x / inf = a signed zero
    v[3], v[dim // 2], v[dim - 1], v[7] = 1.5e19, -1.5e19, 1.5e19, -2.0
    add("overflow", v, True)
    v = np.full((dim,), np.sqrt(1e38 / dim), F32)       # len2 about 1e38: finite, the divisor is about 1e19
    v[1::2] *= -1
    v[5] = 1e-20                                        # its quotient is subnormal, its square vanishes in the sum
    add("large", v, True)
    v = np.zeros((dim,), F32)                   # len2 = 1.25: subnormal inputs and subnormal quotients of normal inputs
    v[:8] = [1.0, 0.5, 1e-42, 3e-39, -1e-42, -1.1754944e-38, 1.4e-45, -1.2e-38]
    v[dim - 1] = 7e-39
    add("subnormal", v, True)
    add("zero", np.zeros((dim,), F32), False)
    ties = bf16_tie_row(dim)
    return Boundary(names, np.stack(rows), np.asarray(divided), np.stack([ties, -ties[::-1].copy()]))
