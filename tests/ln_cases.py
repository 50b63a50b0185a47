"""Hard rows for every place the encoder normalises a row: families whose variance is far below eps, whose mean dwarfs their spread,
or which carry one outlier at a lane / chunk end of the 3 x 256-column layout; the identity-weight construction that puts such a
row into a GEMM's f32 accumulator without error; float32 emulations of the kernels' arithmetic and of the mistakes the families are
there to catch (tests/test_ln_cases_host.py proves both on the CPU); the bound for epilogue 5's statistics on such rows; and the part
of the child runner of tests/gemm_cases.py that runs them.  numpy / torch on the CPU, except run_child.

Families (rows of 768 values; eps = 1e-5 for all, eps = 1e-12 additionally for the first three):

  unit            bf16(randn)                                control; a variance divided by 767
  small           bf16(1e-3 randn): variance 1e-6 < eps      where eps stands and what it is
  tiny            bf16(2^-20 randn): output ~ v / sqrt(eps)   the same
  zero, one_hot   all 0; a single 1.0 at column 5            eps alone decides the scale
  const           all 1000; all -3                           the output is beta within the bound; a wrong mean
  offset_coarse   bf16(1000 + randn), bf16(64 + randn)       a mean far above the spread, on a bf16 row
  offset_fine     f32(1000 + bf16(0.5 randn)), f32(-256 + bf16(0.125 randn)): f32 sites only       a one-pass variance
  outlier         bf16(randn) with +-4096 at column 0, 255, 256 or 767 (one row each)     lane and chunk ends
  two_level       +-1024 alternating by column               sigma exact, z = +-1
  big             bf16(2^30 randn)                           scale invariance inside the f32 range

Out of scope: NaN or infinite elements, and |v| > 2^40 (squares leave the f32 range well before 2^64; nothing here goes near).

A family is (row, p, q): p and q are bf16 numbers and row = f32(p + q), the np.float32 addition the kernels make.  The sites that
normalise a bf16 row (k_layernorm768, epilogue 5 and what follows it) take the families whose row is itself a bf16 number; the sites
that form the row in f32 take all of them as the pair: p through the GEMM (or the word table), q as the bf16 residual, the f32
residual or the position row.  For a bf16 family p = q = row / 2, the sum exact; for offset_fine p is the constant and q the
fluctuation, and the sum rounds -- in the reference as in the kernel, so the reference's row is the kernel's row.

Identity weights: W = I (768 x 768, bf16) -- for K = 3072 [I | 0 | 0 | 0] with finite junk in the other 2304 columns of A -- and
bias 0: the accumulator of output column n is p_n * 1 plus exact zeros, the row without error.
"""
import functools
from typing import NamedTuple

import numpy as np
import torch

from tests import gemm_cases as gc

D = 768
F32 = np.float32
U = gc.U32
EPS = gc.LN_EPS
EPS_ALT = 1e-12                     # honoured-argument check: unit / small / tiny (the first three families) only
N_ALT = 3
PAD_ID = 1


def bf16(x) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).bfloat16().float().numpy()


def is_bf16(x) -> bool:
    return bool(np.array_equal(bf16(x), np.asarray(x, np.float32)))


class Family(NamedTuple):
    name: str
    row: np.ndarray         # f32 [768] = f32(p + q): the row the LayerNorm sees
    p: np.ndarray           # f32 [768] of bf16 numbers: through the GEMM / the word table
    q: np.ndarray           # f32 [768] of bf16 numbers: the residual / the position row
    f32_only: bool          # the row is no bf16 number: sites that form it in f32 only


@functools.lru_cache(maxsize=1)
def all_families():
    """In an order that puts the three eps = 1e-12 families first and a hard row of every kind into the first five of either site."""
    rng = np.random.default_rng(768)
    out = []

    def plain(name, r):
        r = bf16(r)
        h = r * F32(0.5)
        assert is_bf16(h) and np.array_equal(h + h, r)
        out.append(Family(name, r, h, h, False))

    def fine(name, c, scale):
        p, q = np.full(D, c, F32), bf16(scale * rng.standard_normal(D))
        assert is_bf16(p)
        out.append(Family(name, p + q, p, q, True))

    def outlier(col, val):
        r = rng.standard_normal(D)
        r[col] = val
        plain(f"outlier_{col}", r)

    one_hot = np.zeros(D)
    one_hot[5] = 1.0
    # the control: a row on which the eps mistakes stay hidden, as on the randn rows of the older tests.  How far dropping eps moves an
    # output, |g z| eps / 2, is a hundredth of the bf16 rounding 2^-8 |y| -- except where y = g z + b crosses zero and only the f32 term E
    # is left of the tolerance, which two draws in three do somewhere.  Drawn until none does (test_ln_cases_host.py asserts 0.1).
    gam, bet = ln_params()
    for _ in range(64):
        r = bf16(rng.standard_normal(D)).astype(np.float64)
        ref, tol = tolerance(r[None], EPS)
        if (np.abs(gc.layernorm64(r[None], gam, bet, 0.0)[0] - ref) / tol).max() < 0.08:
            break
    else:
        raise AssertionError("no control row")
    plain("unit", r)
    plain("small", 1e-3 * rng.standard_normal(D))
    plain("tiny", 2.0 ** -20 * rng.standard_normal(D))
    fine("offset_fine_1000", 1000.0, 0.5)
    outlier(767, -4096.0)
    plain("offset_coarse_1000", 1000 + rng.standard_normal(D))
    plain("zero", np.zeros(D))
    plain("one_hot", one_hot)
    plain("const_1000", np.full(D, 1000.0))
    plain("const_m3", np.full(D, -3.0))
    plain("offset_coarse_64", 64 + rng.standard_normal(D))
    fine("offset_fine_m256", -256.0, 0.125)
    outlier(0, 4096.0)
    outlier(255, -4096.0)
    outlier(256, 4096.0)
    plain("two_level", 1024.0 * (1 - 2 * (np.arange(D) % 2)))
    plain("big", 2.0 ** 30 * rng.standard_normal(D))
    assert [f.name for f in out[:N_ALT]] == ["unit", "small", "tiny"] and len({f.name for f in out}) == len(out)
    return tuple(out)


def families(site: str, eps: float = EPS):
    """site "bf16": the families a bf16 row can hold; "f32": all.  eps = 1e-12: the first three."""
    fs = [f for f in all_families() if site == "f32" or not f.f32_only]
    return fs[:N_ALT] if eps != EPS else fs


def family(name: str) -> Family:
    return {f.name: f for f in all_families()}[name]


def hard_T(site: str, eps: float = EPS):
    """The whole list as one batch, then its first 5 and its first 1: a ragged end for one wave per row / four rows per workgroup."""
    n = len(families(site, eps))
    return (n,) if eps != EPS else (n, 5, 1)


@functools.lru_cache(maxsize=1)
def ln_params():
    """gamma, beta as gemm_cases.ln_apply_inputs draws them."""
    g = torch.Generator(device="cpu").manual_seed(1768)
    return (1 + 0.25 * torch.randn((D,), generator=g)).numpy(), (0.25 * torch.randn((D,), generator=g)).numpy()


def rows64(fs) -> np.ndarray:
    return np.stack([f.row for f in fs]).astype(np.float64)


def tolerance(v64: np.ndarray, eps: float, f32_out: bool = False):
    """(ref, tol) of the standalone LayerNorm kernels and k_embed_ln: gemm_cases.layernorm64's E, behind one bf16 rounding unless the
    output is the f32 copy."""
    gam, bet = ln_params()
    ref, E = gc.layernorm64(v64, gam, bet, eps)
    return ref, (E if f32_out else gc.bf16_after(ref, E))


# ---------------------------------------------------------------- float32 emulation of k_layernorm768 (and the mistakes)

MUTANTS = ("no_eps", "eps_outside", "n767", "one_pass", "skip_last_chunk")
SECOND_ORDER_LIMIT = 4.0 / (200.0 * U)      # layernorm64's docstring: Vmax / sigma * max|z| must stay below this


def _wave_sum(s: np.ndarray) -> np.ndarray:
    """wave_sum of the kernels: six xor-shuffle levels; every lane ends with the same bits."""
    idx = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        s = s + s[..., idx ^ d]
    return s[..., :1]


def ln_f32(v, eps: float, mutant=None, divide: bool = False) -> np.ndarray:
    """k_layernorm768's arithmetic in np.float32, operation by operation (lane l holds columns 256 i + 4 l .. + 3, i = 0..2; a serial
    sum per lane, then the shuffles; two passes; * f32(1/768) -- `divide`: / 768, k_embed_ln's form; rsqrt; ((v - mu) rstd) g + b).
    -> f32 [rows, 768] before the bf16 rounding.  `mutant`: one of MUTANTS, the mistakes the families must catch."""
    assert mutant is None or mutant in MUTANTS
    gam, bet = (a.astype(F32).reshape(3, 64, 4) for a in ln_params())
    x = np.asarray(v, F32).reshape(-1, 3, 64, 4)
    keep = np.ones((3, 64), F32)
    if mutant == "skip_last_chunk":         # lane 63 loses its third chunk: columns 764..767
        keep[2, 63] = 0
    inv = F32(1) / F32(D)

    def scale(t, n=None):
        if n is not None:
            return t * (F32(1) / F32(n))
        return t / F32(D) if divide else t * inv

    s = np.zeros(x.shape[:1] + (64,), F32)
    for i in range(3):
        s = s + (((x[:, i, :, 0] + x[:, i, :, 1]) + x[:, i, :, 2]) + x[:, i, :, 3]) * keep[i]
    mu = scale(_wave_sum(s))                # [rows, 1]
    q = np.zeros_like(s)
    for i in range(3):
        for j in range(4):
            d = x[:, i, :, j] * x[:, i, :, j] if mutant == "one_pass" else (x[:, i, :, j] - mu) * (x[:, i, :, j] - mu)
            q = q + d * keep[i]
    var = scale(_wave_sum(q), 767 if mutant == "n767" else None)
    if mutant == "one_pass":
        var = var - mu * mu
    with np.errstate(divide="ignore", invalid="ignore"):
        if mutant == "no_eps":
            rstd = F32(1) / np.sqrt(var)
        elif mutant == "eps_outside":
            rstd = F32(1) / (np.sqrt(var) + F32(eps))
        else:
            rstd = F32(1) / np.sqrt(var + F32(eps))
        y = ((x - mu[:, :, None, None]) * rstd[:, :, None, None]) * gam + bet
    assert y.dtype == F32
    return y.reshape(-1, D)


def worst_ratio(got: np.ndarray, ref: np.ndarray, tol: np.ndarray) -> float:
    """max |got - ref| / tol over every element; an element that is not finite counts as infinitely wrong."""
    assert (tol > 0).all()
    r = np.abs(got.astype(np.float64) - ref) / tol
    return float(np.where(np.isfinite(r), r, np.inf).max())


# ---------------------------------------------------------------- epilogue 5's statistics: emulation and bound

def _fma(a, b, c):
    """fmaf on f32 operands: the product is exact in float64 and the sum rounds there once before the rounding to f32 (a double
    rounding differs from fmaf in one case in 2^29: of no account for a bound, and these bits are never compared)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def lnacc_f32(rows, eps: float) -> np.ndarray:
    """(rstd, nmr) as LnAcc / ln_acc_done8 / ln_join_row / k_ln_finalize build them, in np.float32: a lane holds columns 4 g .. + 3 and
    16 + 4 g .. + 3 of a 32-column slot (g = 0..3), shifted by its first; g joins g ^ 1, then the pairs join; 24 slots in index order."""
    x = np.asarray(rows, F32).reshape(-1, 24, 2, 4, 4)         # row, slot, fragment, g, j
    a, b = x[:, :, 0], x[:, :, 1]
    s = a[..., 0]
    d1, d2, d3 = a[..., 1] - s, a[..., 2] - s, a[..., 3] - s
    sd = (d1 + d2) + d3
    sdd = _fma(d3, d3, _fma(d2, d2, d1 * d1))
    e0, e1, e2, e3 = (b[..., j] - s for j in range(4))
    sd = sd + ((e0 + e1) + (e2 + e3))
    sdd = _fma(e3, e3, _fma(e2, e2, _fma(e1, e1, _fma(e0, e0, sdd))))
    md = sd * F32(0.125)
    mean, m2 = s + md, np.maximum(sdd - sd * md, F32(0))        # [rows, 24, 4]

    def join(ma, qa, mb, qb, half_n):
        d = ma - mb
        return F32(0.5) * (ma + mb), (qa + qb) + (d * d) * F32(half_n)
    mean, m2 = join(mean[..., 0::2], m2[..., 0::2], mean[..., 1::2], m2[..., 1::2], 4.0)
    mean, m2 = join(mean[..., 0], m2[..., 0], mean[..., 1], m2[..., 1], 8.0)       # [rows, 24]
    msum = np.zeros(len(x), F32)
    for p in range(24):
        msum = msum + mean[:, p]
    mu = msum / F32(24)
    q, dev = np.zeros_like(mu), np.zeros_like(mu)
    for p in range(24):
        d = mean[:, p] - mu
        q = q + m2[:, p]
        dev = dev + d * d
    var = (q + F32(32) * dev) / F32(768)
    rstd = F32(1) / np.sqrt(var + F32(eps))
    out = np.stack([rstd, -mu * rstd], 1)
    assert out.dtype == F32
    return out


class StatsBound(NamedTuple):
    rstd: np.ndarray        # float64 [T]: the reference
    nmr: np.ndarray
    rel_rstd: np.ndarray    # |d rstd| <= rel_rstd * rstd
    d_mu: np.ndarray        # |d mu|
    d_nmr: np.ndarray       # |d nmr|


def stats_bound(stored64: np.ndarray, eps: float) -> StatsBound:
    """What stats_out = (rstd, nmr) may lose to f32 on a row x of bf16 numbers (u = 2^-24, first order, one rounding per operation;
    V = max |x|, s^2 = the row's variance, M2 = 768 s^2; every partial mean lies in [-V, V]).

    A lane (ln_acc4, ln_acc_done8): 8 values, d_j = x_j - x_0 (u |d_j| each), D1 = sum |d_j| <= 14 V, Q = sum d_j^2.
      sd   six additions, at most three on the way of one term: 4 u D1 with the d_j's own rounding.
      sdd  d_j^2 carries 2 u from d_j; seven roundings of partial sums <= Q: 9 u Q.
      mean = x_0 + sd / 8: u V for the addition + 4 u D1 / 8 <= 8 u V.
      M2   = sdd - sd (sd / 8): 9 u Q; the error of sd twice, 2 |sd| 4 u D1 / 8 <= u D1^2 <= 7 u Q; the product, u sd^2 / 8 <= u Q
           (sd^2 <= 7 Q); the subtraction, u M2 <= u Q: 18 u Q (clamping at 0 moves it towards the true value).
      Q is a SHIFTED sum: (x_j - x_0)^2 <= 2 (x_j - mu)^2 + 2 (x_0 - mu)^2, so a row's 96 lanes together hold sum Q <= 2 M2 + 14 M2
      (all of the row's deviation in first elements): 288 u M2 from the lanes.
    A join (ln_join) of two partials whose means are off by e each: mean = (a + b) / 2: u V + e (8 u V -> 9 u V -> 10 u V for a slot);
      M2 = (M2a + M2b) + d^2 n / 2, d = a - b: two additions, 2 u of the result; d^2 n / 2 carries 2 u (d) + u (the square) and
      2 |d| 2 e n / 2 from the means.  Over a row the results of a level add up to <= M2 and so do the terms d^2 n / 2, whence
      sum |d| n / 2 <= sqrt(192 M2) = 384 s (Cauchy-Schwarz; 192 = the level's n / 2 summed): 5 u M2 + 1536 e s per level, that is
      (on the variance, / 768) 5 u s^2 + 16 u V s for lanes into pairs, 5 u s^2 + 18 u V s for pairs into slots.
    k_ln_finalize: mu = (24 slot means added one by one) / 24: 23 u V + u V + the slots' own 10 u V: |d mu| <= 34 u V.
      sum of the M2s: 23 u M2.  d_p = mean_p - mu is off by 44 u V (+ u |d_p|): sum d_p^2 carries (2 + 1 + 23) u of 32 sum d_p^2 <= M2 and
      2 * 44 u V sum 32 |d_p| <= 88 u V 768 s.  The last addition and the division: 2 u.
    Together |d var| <= u (349 s^2 + 122 V s) + (50 u V)^2 -- the last term the squares of the mean errors (8^2 + 9^2 + 44^2 < 50^2), which
    first order drops and a constant row, s = 0, has nothing else but.  Then var + f32(eps): u for eps as an f32, u for the addition;
    rsqrtf: 2 ulp = 4 u:   |d rstd| / rstd <= |d var| / (2 (s^2 + eps)) + 5 u;   |d nmr| <= rstd |d mu| + |nmr| (|d rstd| / rstd + u).

    A unit row: 349 + 122 * 3.5 = 780 u on the variance, 2.3e-5 on rstd: where STATS_RTOL is.  Rows with V / s in the hundreds go
    far beyond it; a family is held to the larger of this bound and the constants."""
    V = np.abs(stored64).max(-1)
    mu = stored64.mean(-1)
    var = ((stored64 - mu[:, None]) ** 2).mean(-1)
    s = np.sqrt(var)
    d_var = U * (349.0 * var + 122.0 * V * s) + (50.0 * U * V) ** 2
    rel = d_var / (2.0 * (var + eps)) + 5.0 * U
    d_mu = 34.0 * U * V
    rstd = 1.0 / np.sqrt(var + eps)
    nmr = -mu * rstd
    return StatsBound(rstd, nmr, rel, d_mu, rstd * d_mu + np.abs(nmr) * (rel + U))


def hard_stats_excess(got: np.ndarray, stored64: np.ndarray, eps: float) -> float:
    """max over rows of |error| - tolerance; the tolerance the larger of gemm_cases.STATS_* and stats_bound."""
    b = stats_bound(stored64, eps)
    t0 = np.maximum(gc.STATS_RTOL, b.rel_rstd) * b.rstd
    t1 = np.maximum(gc.STATS_RTOL * np.abs(b.nmr) + gc.STATS_NMR_ATOL, b.d_nmr)
    e0 = np.abs(got[:, 0].astype(np.float64) - b.rstd) - t0
    e1 = np.abs(got[:, 1].astype(np.float64) - b.nmr) - t1
    bad = ~np.isfinite(got.astype(np.float64)).all(1)
    return float(np.inf if bad.any() else max(e0.max(), e1.max()))


def dev_stats_tolerance(stored64: np.ndarray, eps: float, gain: np.ndarray, consumer: bool):
    """(ref, tol) of a LayerNorm finished from the DEVICE's stats_out: k_ln_apply768, y = fma(fma(x, rstd, nmr), g, b), or epilogue 3
    with W' = diag(g), colsum = g, bias = beta: acc = x g exactly, y = fma(acc, rstd, fma(nmr, g, b)).  ref: the float64 LayerNorm of the
    row with that gain.  Two parts, both stated:
      the chain's own roundings, ln_apply64's E = u (|g| |t| + |y|), t = x rstd + nmr (apply); u (|nmr g + b| + |y|) (consumer);
      the statistics: x d rstd + d nmr = (x - mu) d rstd - rstd d mu (+ the rounding of nmr): |g| (|z| rel_rstd + rstd |d mu| + u |nmr|),
      rel_rstd and d mu of stats_bound -- the two errors of (rstd, nmr) are one error of mu and one of rstd, not independent.
    Behind one bf16 rounding (bf16_after)."""
    _, bet = ln_params()
    g, b = gain.astype(np.float64), bet.astype(np.float64)
    sb = stats_bound(stored64, eps)
    mu = stored64.mean(-1, keepdims=True)
    z = (stored64 - mu) * sb.rstd[:, None]
    ref = z * g + b
    own = U * ((np.abs(sb.nmr[:, None] * g + b) if consumer else np.abs(g) * np.abs(z)) + np.abs(ref))
    prop = np.abs(g) * (np.abs(z) * sb.rel_rstd[:, None] + (sb.rstd * sb.d_mu + U * np.abs(sb.nmr))[:, None])
    return ref, gc.bf16_after(ref, own + prop)


# ---------------------------------------------------------------- k_embed_ln: tables that make (word + type0) + pos the family row

class EmbedInputs(NamedTuple):
    word: np.ndarray        # f32 [3 + n, 768] of bf16 numbers: row 1 the pad token's, row 3 + r family r's p
    pos: np.ndarray         # f32 [2 + n, 768]: row 1 (= PAD_ID) the pad position's, row 2 + r family r's q
    type0: np.ndarray       # f32 [768]: zeros -- p + 0 is p, and the family row stays the family row (type0's part in the sum is
    #                         test_embed_ln_and_pool's business)
    seqs: tuple             # token ids per sequence: all families with a pad after the second, the first five (or fewer), the first
    v: tuple                # float64 [len, 768] per sequence: the row of every token, the pad's included
    pad_v: np.ndarray       # float64 [768]


@functools.lru_cache(maxsize=2)
def embed_inputs(eps: float) -> EmbedInputs:
    """Position ids are 1 + PAD_ID + (number of real tokens before), whatever the column: the interior pad of the first sequence
    shifts every later token's column by one.  Lengths n + 1, min(5, n - 1), 1: none a multiple of 16."""
    fs = families("f32", eps)
    n = len(fs)
    rng = np.random.default_rng(4242)
    word = bf16(7.0 * rng.standard_normal((3 + n, D)))
    pos = bf16(7.0 * rng.standard_normal((2 + n, D)))
    for r, f in enumerate(fs):
        word[3 + r], pos[2 + r] = f.p, f.q
    type0 = np.zeros(D, F32)
    pad_v = ((word[PAD_ID] + type0) + pos[PAD_ID]).astype(np.float64)
    ids = [3 + r for r in range(n)]
    seqs = (tuple(ids[:2] + [PAD_ID] + ids[2:]), tuple(ids[:min(5, n - 1)]), tuple(ids[:1]))
    v = tuple(np.stack([pad_v if t == PAD_ID else ((word[t] + type0) + pos[2 + t - 3]).astype(np.float64) for t in s]) for s in seqs)
    assert all(len(s) % 16 for s in seqs)
    return EmbedInputs(word, pos, type0, seqs, v, pad_v)


# ---------------------------------------------------------------- the cases and the child runner

GEMM_VARIANTS = {           # variant -> (site, K values): every tiled kernel runs them
    "hard_res_ln": ("bf16", (768, 3072)),       # k_layernorm768: K = 768 in place (y == residual), K = 3072 out of place; residual 0
    "hard_bias_lnres": ("f32", (768,)),         # k_layernorm768_res: p through the GEMM, q the bf16 residual
    "hard_bias_res32_ln": ("f32", (768,)),      # k_layernorm768_res32: q the f32 residual; both outputs
    "hard_res_raw": ("bf16", (768, 3072)),      # epilogue 5 without res_stats, residual 0: the stored row on bits, stats_out
    "hard_lnin": ("bf16", (768,)),              # epilogue 3 as the LayerNorm itself, from hard_res_raw's stats_out
}
ALT_VARIANTS = ("hard_res_ln", "hard_bias_lnres", "hard_bias_res32_ln", "hard_res_raw")       # the entries that take eps, at K = 768
NO_GEMM_VARIANTS = ("hard_ln_apply", "hard_ln_apply_dev", "hard_embed", "hard_embed_packed", "hard_embed_e12", "hard_embed_packed_e12")
STATS_VARIANTS = ("hard_res_raw", "hard_res_raw_e12")
AGREE = tuple(GEMM_VARIANTS) + tuple(v + "_e12" for v in ALT_VARIANTS)


def variant_eps(variant: str) -> float:
    return EPS_ALT if variant.endswith("_e12") else EPS


def cases(kernel: str):
    out = []
    for v, (site, Ks) in GEMM_VARIANTS.items():
        out += [gc.Case(f"{kernel}-{v}-{T}x768x{K}", kernel, v, T, D, K) for K in Ks for T in hard_T(site)]
    for v in ALT_VARIANTS:
        T = hard_T(GEMM_VARIANTS[v][0], EPS_ALT)[0]
        out.append(gc.Case(f"{kernel}-{v}_e12-{T}x768x768", kernel, v + "_e12", T, D, 768))
    if kernel == gc.KERNELS[0]:     # no tiled kernel in these: once, in the first child
        for v in NO_GEMM_VARIANTS[:2]:
            out += [gc.Case(f"{kernel}-{v}-{T}x768x0", kernel, v, T, D, 0) for T in hard_T("bf16")]
        for v in NO_GEMM_VARIANTS[2:]:
            T = sum(len(s) for s in embed_inputs(variant_eps(v)).seqs)
            out.append(gc.Case(f"{kernel}-{v}-{T}x768x0", kernel, v, T, D, 0))
    return out


def run_child(kernel: str, L, t, records) -> None:
    """The hard-row records of one child of tests/gemm_cases.py.  t: the runner's helpers (dev, guarded, guards_ok, sha, up, call)."""
    dev = t.dev
    gam, bet = ln_params()
    gam_d, bet_d, zero_bias = t.up(gam), t.up(bet), t.up(np.zeros(D, F32))
    gain = bf16(gam)                # epilogue 3: W' = diag(bf16(gamma)), colsum the same numbers
    gain_d = t.up(gain)
    eye = {768: t.up(np.eye(D, dtype=F32), torch.bfloat16),
           3072: t.up(np.concatenate([np.eye(D, dtype=F32), np.zeros((D, 2304), F32)], 1), torch.bfloat16)}
    wdiag = t.up(np.diag(gain), torch.bfloat16)
    junk = bf16(100.0 * np.random.default_rng(3072).standard_normal((len(all_families()), 2304)))
    dev_stats = {}                  # (T, eps) -> stats_out of hard_res_raw at K = 768 (device tensor)

    def rec_of(c, entry, epi, kind):
        return dict(id=c.id, kernel=kernel, variant=c.variant, entry=entry, epilogue=epi, kind=kind, T=c.T, N=D, K=c.K,
                    ragged=gc.is_ragged(kernel, c.T), multi_tile=gc.is_multi_tile(kernel, c.T, D), diff_words=None, excess=None, stats_excess=None,
                    aux_excess=None, sha_stats=None)

    def excess(got, ref, tol):
        e = np.abs(got.double().cpu().numpy() - ref) - tol
        return float(np.where(np.isfinite(e), e, np.inf).max())

    def run_gemm(c):
        base = c.variant[:-4] if c.variant.endswith("_e12") else c.variant
        eps = variant_eps(c.variant)
        site = GEMM_VARIANTS[base][0]
        fs = families(site, eps)[:c.T]
        T, K = c.T, c.K
        assert len(fs) == T and (kernel != "pp" or gc.pp_allowed(T, D, K))
        entry, epi, kind = gc.VARIANTS[c.variant]
        rec = rec_of(c, entry, epi, kind)
        # through the GEMM: the bf16 row itself at a bf16 site, p at an f32 site
        a = np.stack([f.row if site == "bf16" else f.p for f in fs])
        if K == 3072:
            a = np.concatenate([a, junk[:T]], 1)
        a_d = t.up(a, torch.bfloat16)
        yf, y = t.guarded(T, (D,), torch.bfloat16)
        ok = True
        if base == "hard_res_ln":
            if K <= 1024:           # in place: epilogue 2 at this K
                y.zero_()
                res_ptr = y.data_ptr()
            else:
                res = torch.zeros((T, D), dtype=torch.bfloat16, device=dev)
                res_ptr = res.data_ptr()
            t.call(L.crh_gemm_bf16_bias_res_ln, a_d.data_ptr(), eye[K].data_ptr(), zero_bias.data_ptr(), res_ptr, gam_d.data_ptr(), bet_d.data_ptr(), eps,
                   y.data_ptr(), T, D, K, 0)
            rec["excess"] = excess(y, *tolerance(rows64(fs), eps))
        elif base == "hard_bias_lnres":
            res = t.up(np.stack([f.q for f in fs]), torch.bfloat16)
            t.call(L.crh_gemm_bf16_bias_res_ln, a_d.data_ptr(), eye[K].data_ptr(), zero_bias.data_ptr(), res.data_ptr(), gam_d.data_ptr(), bet_d.data_ptr(), eps,
                   y.data_ptr(), T, D, K, 0)
            rec["excess"] = excess(y, *tolerance(rows64(fs), eps))
        elif base == "hard_bias_res32_ln":
            rf, r32 = t.guarded(T, (D,), torch.float32, t.up(np.stack([f.q for f in fs])))
            t.call(L.crh_gemm_bf16_bias_res32_ln, a_d.data_ptr(), eye[K].data_ptr(), zero_bias.data_ptr(), r32.data_ptr(), gam_d.data_ptr(), bet_d.data_ptr(), eps,
                   y.data_ptr(), T, D, K, 0)
            ok = t.guards_ok(rf, T)
            rec["excess"] = excess(y, *tolerance(rows64(fs), eps))
            rec["aux_excess"] = excess(r32, *tolerance(rows64(fs), eps, f32_out=True))
        elif base == "hard_res_raw":
            res = torch.zeros((T, D), dtype=torch.bfloat16, device=dev)
            pf, part = t.guarded(T, (24, 2), torch.float32)
            sf, st = t.guarded(T, (2,), torch.float32)
            t.call(L.crh_gemm_bf16_res_lnstats, a_d.data_ptr(), eye[K].data_ptr(), zero_bias.data_ptr(), res.data_ptr(), None, None, eps, y.data_ptr(),
                   part.data_ptr(), st.data_ptr(), T, D, K, 0)
            ok = t.guards_ok(pf, T) and t.guards_ok(sf, T)
            want = torch.from_numpy(np.stack([f.row for f in fs])).bfloat16()
            rec["diff_words"] = int((y.cpu().view(torch.int16) != want.view(torch.int16)).sum())
            rec["stats_excess"] = hard_stats_excess(st.cpu().numpy(), rows64(fs), eps)
            rec["sha_stats"] = t.sha(st)
            if K == 768:
                dev_stats[(T, eps)] = st.clone()
        elif base == "hard_lnin":
            st = dev_stats[(T, eps)]
            t.call(L.crh_gemm_bf16_lnin, a_d.data_ptr(), st.data_ptr(), wdiag.data_ptr(), gain_d.data_ptr(), bet_d.data_ptr(), y.data_ptr(), T, D, K, 0, 0)
            rec["excess"] = excess(y, *dev_stats_tolerance(rows64(fs), eps, gain, consumer=True))
        else:
            raise KeyError(c.variant)
        rec["guards_ok"] = ok and t.guards_ok(yf, T)
        rec["sha_out"] = t.sha(y)
        records.append(rec)

    def run_apply(c):
        fs = families("bf16")[:c.T]
        T = c.T
        v64 = rows64(fs)
        rec = rec_of(c, "crh_layernorm_apply", None, "tol")
        xf, xd = t.guarded(T, (D,), torch.bfloat16, t.up(np.stack([f.row for f in fs]), torch.bfloat16))
        yf, y = t.guarded(T, (D,), torch.bfloat16)
        if c.variant == "hard_ln_apply":        # the float64 statistics rounded to f32: ln_apply64 from those very numbers
            rstd, nmr = gc.row_stats64(v64)
            i = gc.LnApplyInputs(torch.from_numpy(v64).bfloat16(), np.stack([rstd, nmr], 1).astype(F32), gam, bet)
            st = t.up(i.stats)
            ref, E = gc.ln_apply64(i)
            tol = gc.bf16_after(ref, E)
        else:                                   # the device's own stats_out: the float64 LayerNorm of the row
            st = dev_stats[(T, EPS)]
            ref, tol = dev_stats_tolerance(v64, EPS, gam, consumer=False)
        t.call(L.crh_layernorm_apply, xd.data_ptr(), st.data_ptr(), gam_d.data_ptr(), bet_d.data_ptr(), y.data_ptr(), T, D, 0)
        rec["excess"] = excess(y, ref, tol)
        rec["guards_ok"] = t.guards_ok(xf, T) and t.guards_ok(yf, T)
        rec["sha_out"] = t.sha(y)
        records.append(rec)

    def run_embed(c):
        eps = variant_eps(c.variant)
        packed = "packed" in c.variant
        e = embed_inputs(eps)
        B, Lp = len(e.seqs), 32
        assert max(len(s) for s in e.seqs) <= Lp
        word, pos, typ = t.up(e.word, torch.bfloat16), t.up(e.pos, torch.bfloat16), t.up(e.type0, torch.bfloat16)
        bits = [sum(1 << k for k, tok in enumerate(s) if tok != PAD_ID) for s in e.seqs]
        rec = rec_of(c, "crh_embed_ln_packed" if packed else "crh_embed_ln", None, "tol")
        kf, km = t.guarded(B, (1,), torch.int64)
        if packed:
            flat = [tok for s in e.seqs for tok in s]
            T = len(flat)
            off = np.cumsum([0] + [len(s) for s in e.seqs]).astype(np.int32)
            ids, off_d = t.up(np.array(flat, np.int32), torch.int32), t.up(off, torch.int32)
            of, out = t.guarded(T, (D,), torch.bfloat16)
            t.call(L.crh_embed_ln_packed, ids.data_ptr(), off_d.data_ptr(), word.data_ptr(), pos.data_ptr(), typ.data_ptr(), gam_d.data_ptr(), bet_d.data_ptr(),
                   eps, PAD_ID, out.data_ptr(), km.data_ptr(), B, T, Lp, D, 0)
            t.call(L.crh_encoder_finish, 0)
            v = np.concatenate(e.v)
            rows = T
        else:
            ids_np = np.full((B, Lp), PAD_ID, np.int32)
            for b, s in enumerate(e.seqs):
                ids_np[b, :len(s)] = s
            ids = t.up(ids_np, torch.int32)
            of, out = t.guarded(B * Lp, (D,), torch.bfloat16)
            t.call(L.crh_embed_ln, ids.data_ptr(), word.data_ptr(), pos.data_ptr(), typ.data_ptr(), gam_d.data_ptr(), bet_d.data_ptr(), eps, PAD_ID,
                   out.data_ptr(), km.data_ptr(), B, Lp, D, 0)
            v = np.concatenate([np.concatenate([vs, np.broadcast_to(e.pad_v, (Lp - len(vs), D))]) for vs in e.v])
            rows = B * Lp
        assert c.T == sum(len(s) for s in e.seqs)
        rec["excess"] = excess(out, *tolerance(v, eps))
        rec["diff_words"] = int(sum(int(w) & (2 ** 64 - 1) != b for w, b in zip(km.cpu().numpy().ravel().tolist(), bits)))      # the mask words
        rec["guards_ok"] = t.guards_ok(of, rows) and t.guards_ok(kf, B)
        rec["sha_out"] = t.sha(out)
        records.append(rec)

    for c in cases(kernel):
        if c.variant in ("hard_ln_apply", "hard_ln_apply_dev"):
            run_apply(c)
        elif c.variant in NO_GEMM_VARIANTS:
            run_embed(c)
        else:
            run_gemm(c)
