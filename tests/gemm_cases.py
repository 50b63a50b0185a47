"""Encoder GEMM test matrix: inputs whose result is known exactly, the shapes at each kernel's tile edges, float64 references with
derived bounds, and the child runner that executes one kernel's whole matrix in a process of its own.

The top level is numpy / torch on the CPU only; the GPU is touched under ``if __name__ == "__main__"`` alone
(``python -m tests.gemm_cases --kernel {mid,nt,pp} --out FILE``, started by tests/test_gemm_matrix_gpu.py with the
environment of ENV[kernel]: the library reads its kernel switches once per process).

Exact cases.  A in {-3..3}, W in {-1, 0, 1}, the bias a bf16-exact integer in [-1000, 1000], the residual an integer in [-128, 128]; rows
of A and rows of W (the output's columns) pairwise distinct.  Every input is exact in bf16, every product and every
partial sum an integer below 3 K <= 9216 < 2^24, so the f32 accumulator holds the exact sum whatever the order of the additions,
and so does the epilogue's f32 arithmetic (sums of such integers; with the given statistics of epilogues 3 and 5 -- rstd and gamma
in {0.5, 1, 2}, nmr and colsum integers -- multiples of 1/4 below 2^15).  The one rounding left is pack2's round-to-nearest-even to
bf16: the expected output is bf16_rne(float64 result), compared on BITS.  The bias range puts about three outputs in four above
256, where an integer needs rounding (ROUNDED_SHARE / TIE_SHARE, proved per case by tests/test_gemm_cases_host.py): a rounding
point moved before the bias or the residual changes bits.

Tolerance cases state their bound where it is computed: gelu_bound, layernorm64, ln_apply64, STATS_*; for the hard LayerNorm rows
(tiny variance, large offset, outliers: tests/ln_cases.py, run by the same children through identity weights) stats_bound and
dev_stats_tolerance of that file.  No bound here or there was chosen by looking at what a GPU returned.
"""
import functools
import hashlib
import json
import os
import sys
import time
from typing import NamedTuple, Optional

import numpy as np
import torch

# ---------------------------------------------------------------- kernels, their forcing environment, their shapes

KERNELS = ("mid", "nt", "pp")       # the order the children run in
TILE = {"nt": (256, 128), "mid": (64, 64), "pp": (256, 256)}
# choose_gemm, asked by every entry's one launch_gemm call (csrc/crh_encoder.hip): CODERAG_HIP_MID=2 -> k_gemm_mid whenever
# N % 64 == 0; CODERAG_HIP_GEMM256=2 -> the ping-pong kernel whenever pp_allowed(); both 0 -> k_gemm_nt
ENV = {"nt": {"CODERAG_HIP_GEMM256": "0", "CODERAG_HIP_MID": "0"},
       "mid": {"CODERAG_HIP_MID": "2"},
       "pp": {"CODERAG_HIP_GEMM256": "2", "CODERAG_HIP_MID": "0"}}

# the encoder's four GEMMs at one ragged T (one partial 256-row panel, four full 64-row tiles and a partial one): in every list,
# so that every (epilogue, shape) of the product is compared across the three kernels
PRODUCT_SHAPES = ((300, 768, 768), (300, 2304, 768), (300, 3072, 768), (300, 768, 3072))

# k_gemm_nt: 256x128 tiles, k-step 64, 3-stage ring; 8 XCD labels x (grid / 8 <= 32) workgroups; by_panel from 16 panels
NT_SHAPES = ((1, 128, 64),          # one pipeline step in the whole launch (total == 1), 7 labels without a tile
             (255, 128, 128),       # two steps (total == 2)
             (257, 256, 192),       # total == 3; ragged second panel (one row); 4 tiles on 8 labels
             (513, 768, 768),
             (3841, 768, 256),      # 16 panels: by_panel, 2 panels per label (hm = 2 < HM), nb = 6 < WN, last panel one row
             (4100, 2304, 256),     # 17 panels: label 0 owns 3; nb = 18 = 8 + 8 + 2; 54 tiles on 32 workgroups: a pipeline carried across tiles
             (2049, 3072, 768),
             (5000, 768, 3072),     # the product's FFN2 inside k_gemm_nt's own window of the cost model
             # (added to the starting list) one and two k-steps per tile under a tile list of two -- label 0's 54 tiles on 32 workgroups:
             # the total == 2 start-up stages two different tiles and every step ends in an epilogue; with nk = 2 (total == 4) the
             # prologue's third stage and the one LDS-DMA issued inside the loop already belong to the second tile
             (4100, 2304, 64),
             (4100, 2304, 128),
             ) + PRODUCT_SHAPES
# k_gemm_mid: 64x64 tiles, 4-stage ring with three k-steps in flight
MID_SHAPES = ((1, 128, 64),         # nk = 1
              (63, 128, 128),       # nk = 2
              (65, 128, 192),       # nk = 3: the whole K issued by the prologue; ragged second tile row
              (64, 768, 256),       # nk = 4: the first in-loop issue, into the stage just vacated
              (577, 2304, 768),
              (129, 768, 3072)) + PRODUCT_SHAPES
# the ping-pong kernel: 256x256 tiles; N % 256 == 0, K % 128 == 0, K >= 256
PP_SHAPES = ((1, 256, 256),
             (255, 256, 384),
             (257, 512, 256),
             (3841, 768, 256),      # 16 panels: by_panel
             (4100, 2304, 256),     # nb = 9 = 8 + 1
             (6144, 3072, 256),     # 36 tiles per label: a second tile for four workgroups of each
             (5121, 3072, 768)) + PRODUCT_SHAPES
SHAPES = {"nt": NT_SHAPES, "mid": MID_SHAPES, "pp": PP_SHAPES}
LN_APPLY_T = (1, 5, 300)            # crh_layernorm_apply: one wave per row, four rows per workgroup


def pp_allowed(T: int, N: int, K: int) -> bool:
    """pp_allowed() of csrc/crh_encoder.hip: the shapes the ping-pong kernel takes."""
    if N % 256 or K % 128 or K < 256:
        return False
    return T * K * 2 < 2 ** 32 and N * K * 2 < 2 ** 32 and T * N * 2 < 2 ** 32


# variant -> (public entry, epilogue the tiled kernel runs, "exact" | "tol")
VARIANTS = {
    "bias": ("crh_gemm_bf16_bias", 0, "exact"),
    "bias_gelu": ("crh_gemm_bf16_bias", 1, "tol"),
    "lnin": ("crh_gemm_bf16_lnin", 3, "exact"),
    "lnin_gelu": ("crh_gemm_bf16_lnin", 4, "tol"),
    "res_raw": ("crh_gemm_bf16_res_lnstats", 5, "exact"),        # without res_stats: bias + residual, one rounding
    "res_norm": ("crh_gemm_bf16_res_lnstats", 5, "exact"),       # with res_stats: the residual normalised on the fly
    "res_ln": ("crh_gemm_bf16_bias_res_ln", 2, "tol"),           # K > 1024 out of place; K <= 1024 with y == residual
    "bias_lnres": ("crh_gemm_bf16_bias_res_ln", 0, "tol"),       # K <= 1024, y != residual: k_layernorm768_res adds the residual
    "bias_res32_ln": ("crh_gemm_bf16_bias_res32_ln", 0, "tol"),  # k_layernorm768_res32
    # the hard LayerNorm rows of tests/ln_cases.py behind identity weights (..._e12: eps = 1e-12, the first three families)
    "hard_res_ln": ("crh_gemm_bf16_bias_res_ln", 2, "tol"),
    "hard_bias_lnres": ("crh_gemm_bf16_bias_res_ln", 0, "tol"),
    "hard_bias_res32_ln": ("crh_gemm_bf16_bias_res32_ln", 0, "tol"),
    "hard_res_raw": ("crh_gemm_bf16_res_lnstats", 5, "exact"),   # the stored row on bits; stats_out within ln_cases.stats_bound
    "hard_lnin": ("crh_gemm_bf16_lnin", 3, "tol"),               # W' = diag(gamma): the consumer GEMM is the LayerNorm itself
    "hard_res_ln_e12": ("crh_gemm_bf16_bias_res_ln", 2, "tol"),
    "hard_bias_lnres_e12": ("crh_gemm_bf16_bias_res_ln", 0, "tol"),
    "hard_bias_res32_ln_e12": ("crh_gemm_bf16_bias_res32_ln", 0, "tol"),
    "hard_res_raw_e12": ("crh_gemm_bf16_res_lnstats", 5, "exact"),
}
AGREE_VARIANTS = ("bias", "lnin", "res_raw", "res_norm", "res_ln", "bias_lnres", "bias_res32_ln")     # epilogues 0, 2, 3, 5


def variants_for(T: int, N: int, K: int):
    v = ["bias", "bias_gelu", "lnin", "lnin_gelu"]
    if N == 768:
        v += ["res_raw", "res_norm", "res_ln", "bias_res32_ln"]
        if K <= 1024:
            v.append("bias_lnres")
    return v


class Case(NamedTuple):
    id: str
    kernel: str
    variant: str
    T: int
    N: int
    K: int


def cases(kernel: str):
    out = [Case(f"{kernel}-{v}-{T}x{N}x{K}", kernel, v, T, N, K) for (T, N, K) in SHAPES[kernel] for v in variants_for(T, N, K)]
    if kernel == KERNELS[0]:        # the LayerNorm-only entry involves no tiled kernel: it runs once, in the first child
        out += [Case(f"{kernel}-ln_apply-{T}x768x0", kernel, "ln_apply", T, 768, 0) for T in LN_APPLY_T]
    from tests import ln_cases      # (imports this module: not at the top)
    return out + ln_cases.cases(kernel)


def is_ragged(kernel: str, T: int) -> bool:
    return T % TILE[kernel][0] != 0


def is_multi_tile(kernel: str, T: int, N: int) -> bool:
    bm, bn = TILE[kernel]
    return -(-T // bm) * (N // bn) > 1


# ---------------------------------------------------------------- inputs

def _distinct_rows(x: np.ndarray) -> bool:
    return len(np.unique(np.ascontiguousarray(x).astype(np.int8), axis=0)) == len(x)


class ExactInputs(NamedTuple):
    a: np.ndarray           # f32 [T, K] in {-3..3}, rows distinct
    w: np.ndarray           # f32 [N, K] in {-1, 0, 1}, rows distinct
    bias: np.ndarray        # f32 [N] integers in [-1000, 1000], those bf16 holds (even above 256, multiples of 4 above 512)
    res: Optional[np.ndarray]   # f32 [T, N] integers in [-128, 128] (N == 768 only)
    res32: Optional[np.ndarray]     # f32 [T, N] multiples of 1/4 in (-32, 32): the f32 residual stream of ..._res32_ln
    rstd: np.ndarray        # f32 [T] in {0.5, 1, 2}
    nmr: np.ndarray         # f32 [T] integers in {-3..3}
    colsum: np.ndarray      # f32 [N] integers in [-50, 50]: GIVEN to epilogue 3, not the sum of w's rows
    gamma: np.ndarray       # f32 [N] in {0.5, 1, 2}: the gain of epilogue 5's on-the-fly LayerNorm
    ln_gamma: np.ndarray    # f32 [N], ln_beta f32 [N]: the LayerNorm AFTER the GEMM (tolerance cases): generic values
    ln_beta: np.ndarray


@functools.lru_cache(maxsize=2)
def exact_inputs(T: int, N: int, K: int) -> ExactInputs:
    for attempt in range(8):
        rng = np.random.default_rng([11, T, N, K, attempt])
        a = rng.integers(-3, 4, (T, K)).astype(np.float32)
        w = rng.integers(-1, 2, (N, K)).astype(np.float32)
        if _distinct_rows(a) and _distinct_rows(w):
            break
    else:
        raise AssertionError("no distinct rows")
    half = np.array([0.5, 1.0, 2.0], np.float32)
    bias = torch.from_numpy(rng.integers(-1000, 1001, N).astype(np.float32)).bfloat16().float().numpy()      # integers that bf16 holds
    rstd = half[rng.integers(0, 3, T)]
    nmr = rng.integers(-3, 4, T).astype(np.float32)
    colsum = rng.integers(-50, 51, N).astype(np.float32)
    gamma = half[rng.integers(0, 3, N)]
    ln_gamma = (1 + 0.25 * rng.standard_normal(N)).astype(np.float32)
    ln_beta = (0.25 * rng.standard_normal(N)).astype(np.float32)
    res = res32 = None
    if N == 768:
        res = rng.integers(-128, 129, (T, N)).astype(np.float32)
        res32 = (rng.integers(-127, 128, (T, N)) / 4).astype(np.float32)
    return ExactInputs(a, w, bias, res, res32, rstd, nmr, colsum, gamma, ln_gamma, ln_beta)


GELU_NNZ = 6


class GeluInputs(NamedTuple):
    w: np.ndarray           # f32 [N, K]: GELU_NNZ entries of +-1 per row, anywhere along K: the accumulator stays within a few units
    bias: np.ndarray        # f32 [N] multiples of 1/8 in [-2, 2]
    rstd: np.ndarray        # f32 [T] in {0.5, 1}
    nmr: np.ndarray         # f32 [T] in {-1, 0, 1}
    colsum: np.ndarray      # f32 [N] integers in {-2..2}


@functools.lru_cache(maxsize=2)
def gelu_inputs(T: int, N: int, K: int) -> GeluInputs:
    """With A of exact_inputs (variance 4 per entry) the pre-activation A.w^T + bias is exact in f32 -- a multiple of 1/8, standard
    deviation about 2 sqrt(6) = 4.9 -- so GELU is sampled all over (-4, 4), between the integers, and well into both tails."""
    rng = np.random.default_rng([13, T, N, K])
    pos = np.argpartition(rng.random((N, K)), GELU_NNZ, axis=1)[:, :GELU_NNZ]
    w = np.zeros((N, K), np.float32)
    np.put_along_axis(w, pos, (2 * rng.integers(0, 2, pos.shape) - 1).astype(np.float32), axis=1)
    bias = (rng.integers(-16, 17, N) / 8).astype(np.float32)
    rstd = np.array([0.5, 1.0], np.float32)[rng.integers(0, 2, T)]       # (2 would push two thirds of a row's pre-activations out of (-4, 4))
    nmr = rng.integers(-1, 2, T).astype(np.float32)
    colsum = rng.integers(-2, 3, N).astype(np.float32)
    return GeluInputs(w, bias, rstd, nmr, colsum)


# ---------------------------------------------------------------- float64 references

def acc64(a: np.ndarray, w: np.ndarray) -> np.ndarray:
    """A . W^T in float64 (torch on the CPU: BLAS)."""
    return (torch.from_numpy(a).double() @ torch.from_numpy(w).double().T).numpy()


def exact_value(variant: str, x: ExactInputs, acc: np.ndarray) -> np.ndarray:
    """The epilogue's result before its one rounding, in float64 (an exact number: see the module docstring)."""
    if variant == "bias":
        return acc + x.bias.astype(np.float64)
    if variant == "lnin":           # fma(acc, rstd, fma(nmr, c, b))
        return acc * x.rstd.astype(np.float64)[:, None] + (x.nmr.astype(np.float64)[:, None] * x.colsum.astype(np.float64) + x.bias.astype(np.float64))
    if variant == "res_raw":        # (acc + b) + r
        return acc + x.bias.astype(np.float64) + x.res.astype(np.float64)
    if variant == "res_norm":       # fma(fma(r, rstd, nmr), gamma, acc + b)
        h = x.res.astype(np.float64) * x.rstd.astype(np.float64)[:, None] + x.nmr.astype(np.float64)[:, None]
        return h * x.gamma.astype(np.float64) + (acc + x.bias.astype(np.float64))
    raise KeyError(variant)


def bf16_rne(v64: np.ndarray) -> torch.Tensor:
    """float64 -> bf16, round to nearest even, for values that are exact in f32 (asserted): one rounding, torch's."""
    t = torch.from_numpy(np.ascontiguousarray(v64))
    f = t.float()
    assert bool((f.double() == t).all()), "the value is not exact in f32: two roundings would differ from one"
    return f.bfloat16()


def bf16_bits(v64: np.ndarray) -> np.ndarray:
    return bf16_rne(v64).view(torch.int16).numpy()


def needs_rounding_share(v64: np.ndarray):
    """(share of values that are not bf16 numbers, share that lie exactly half-way between two): the 16 bits of the f32 form that
    bf16 drops are not zero / are 0x8000."""
    t = torch.from_numpy(np.ascontiguousarray(v64))
    f = t.float()
    assert bool((f.double() == t).all())
    low = f.view(torch.int32).numpy() & 0xffff
    return float((low != 0).mean()), float((low == 0x8000).mean())


ROUNDED_SHARE = 0.25        # at least a quarter of an exact case's outputs are not bf16 numbers before the epilogue's rounding ...
TIE_SHARE = 0.05            # ... and at least one in twenty sits exactly between two (round-to-nearest-EVEN decides)

BF16_REL = 2.0 ** -8        # one round-to-nearest to bf16: half an ulp <= 2^-9 * 2^(e+1) <= 2^-8 |v|
U32 = 2.0 ** -24            # one f32 rounding, relative
GELU_ABS = 4e-6             # gelu_erf2's stated bound (csrc/crh_encoder.hip, the comment above it): |x Phi(x) - gelu(x)| <= 4e-6


def gelu_x(variant: str, x: ExactInputs, g: GeluInputs, acc: np.ndarray) -> np.ndarray:
    """The pre-activation in float64; exact in f32 as well (multiples of 1/16 of a few dozen)."""
    if variant == "bias_gelu":
        return acc + g.bias.astype(np.float64)
    if variant == "lnin_gelu":
        return acc * g.rstd.astype(np.float64)[:, None] + (g.nmr.astype(np.float64)[:, None] * g.colsum.astype(np.float64) + g.bias.astype(np.float64))
    raise KeyError(variant)


def gelu64(x: np.ndarray) -> np.ndarray:
    """erf-GELU in float64: x Phi(x) with Phi(x) = erfc(-x / sqrt 2) / 2 (no cancellation in the negative tail)."""
    t = torch.from_numpy(x)
    return (t * 0.5 * torch.special.erfc(-t / 2.0 ** 0.5)).numpy()


def gelu_bound(x: np.ndarray, ref: np.ndarray) -> np.ndarray:
    """One bf16 rounding of the result + the kernel's own stated bound for gelu_erf2, scaled by (1 + |x|): the pre-activation is
    exact, so nothing else enters."""
    return BF16_REL * np.abs(ref) + GELU_ABS * (1.0 + np.abs(x))


LN_EPS = 1e-5


def ln_pre(variant: str, x: ExactInputs, acc: np.ndarray) -> np.ndarray:
    """The rows the LayerNorm after the GEMM normalises, exactly (float64 of f32 values the kernels hold without error)."""
    if variant == "res_ln":         # epilogue 2: one rounding of acc + bias + residual, LayerNorm of the bf16 rows
        return bf16_rne(exact_value("res_raw", x, acc)).double().numpy()
    y0 = bf16_rne(exact_value("bias", x, acc)).double().numpy()      # epilogue 0 rounds acc + bias; the residual joins in f32, exactly
    if variant == "bias_lnres":
        return y0 + x.res.astype(np.float64)
    if variant == "bias_res32_ln":
        return y0 + x.res32.astype(np.float64)
    raise KeyError(variant)


def layernorm64(pre: np.ndarray, gamma: np.ndarray, beta: np.ndarray, eps: float = LN_EPS):
    """(float64 LayerNorm of `pre`, E): E bounds what k_layernorm768 / _res / _res32 lose to f32 arithmetic on inputs v that are
    exact in f32 (u = 2^-24, first order; the file is compiled with -ffp-contract=off, every operation rounds once):
      mu    768 values summed through 12 serial additions per lane and 6 shuffle levels: |dS| <= 18 u sum|v|; times the rounded
            constant 1/768: 2 u more.  |d mu| <= 20 u Vmax, Vmax = the row's largest |v|.
      var   d_i = v_i - mu carries d mu + u |d_i|; the error of mu cancels to first order in sum d_i^2 (sum d_i = 0) and enters as
            (d mu / sigma)^2 <= (20 u * 28)^2, nothing.  Per term 2 u (from d_i) + u (the square), 18 u for the summation, 2 u for
            the 1/768, u for adding eps: 24 u relative on var + eps.
      rstd  half of that, 12 u, + rsqrtf: 2 ulp = 4 u (the larger of the two documented figures: HIP's device-function table
            says 1 ulp, the OpenCL profile its implementation is written to says 2): 16 u.
      y     ((v - mu) rstd) g + b: |g| rstd (d mu + u |d|) from the difference, (16 + 2) u |g z| from rstd and the two products,
            u |y| from the last addition: <= u (|g| (20 Vmax / sigma + 19 |z|) + |y|), z = (v - mu) / sigma.
    E = u (24 |g| (Vmax / sigma + |z|) + |y|): the constants rounded up to one.  The bf16 result is within
    2^-8 |ref| + (1 + 2^-8) E of the reference (the rounding acts on a value within E of it); the f32 copy of ..._res32_ln within E.
    k_embed_ln forms v by two f32 additions (mirrored by its reference, so v is exact here too) and DIVIDES the two sums by 768 where
    the others multiply by the rounded 1/768: one rounding (u) where the derivation counts two, so E covers it unchanged.
    Rows whose mean dwarfs their spread, or whose variance is below eps (tests/ln_cases.py; sigma includes eps), need what "nothing"
    above assumed of Vmax / sigma: the squared error of mu enters var + eps as (20 u Vmax / sigma)^2 and y as half of that times
    |g z|, 200 u^2 (Vmax / sigma)^2 |g z|.  It stays below the 4 u |g| Vmax / sigma that rounding 20 up to 24 left over as long as
    (Vmax / sigma) |z| <= 4 / (200 u) = 3.3e5, which tests/test_ln_cases_host.py checks for every row used (a constant row has z = 0)."""
    g, b = gamma.astype(np.float64), beta.astype(np.float64)
    mu = pre.mean(-1, keepdims=True)
    sigma = np.sqrt(((pre - mu) ** 2).mean(-1, keepdims=True) + eps)
    z = (pre - mu) / sigma
    ref = z * g + b
    vmax = np.abs(pre).max(-1, keepdims=True)
    E = U32 * (24.0 * np.abs(g) * (vmax / sigma + np.abs(z)) + np.abs(ref))
    return ref, E


def bf16_after(ref: np.ndarray, E: np.ndarray) -> np.ndarray:
    return BF16_REL * np.abs(ref) + (1.0 + BF16_REL) * E


def row_stats64(rows: np.ndarray, eps: float = LN_EPS):
    """(rstd, nmr = -mu rstd) of each row in float64."""
    mu = rows.mean(-1)
    rstd = 1.0 / np.sqrt(((rows - mu[:, None]) ** 2).mean(-1) + eps)
    return rstd, -mu * rstd


# epilogue 5's stats_out: the criterion of test_folded_producer_gemm_residual_and_statistics, against float64 statistics of the
# rows AS STORED.  (Rows of order one; what the LnAcc / ln_join / k_ln_finalize arithmetic may lose on ANY row is derived in
# tests/ln_cases.py, stats_bound: |d var| <= u (349 s^2 + 122 V s) + (50 u V)^2, |d mu| <= 34 u V -- on a unit row 2.3e-5 of rstd, these
# constants; the hard rows are held to the larger of the two.)
STATS_RTOL, STATS_NMR_ATOL = 2e-5, 2e-6


def stats_excess(got: np.ndarray, stored_rows: np.ndarray) -> float:
    rstd, nmr = row_stats64(stored_rows)
    e0 = np.abs(got[:, 0].astype(np.float64) - rstd) - STATS_RTOL * np.abs(rstd)
    e1 = np.abs(got[:, 1].astype(np.float64) - nmr) - (STATS_RTOL * np.abs(nmr) + STATS_NMR_ATOL)
    return float(max(e0.max(), e1.max()))


class LnApplyInputs(NamedTuple):
    x: torch.Tensor         # bf16 [T, 768]: un-normalised rows (some scale, some mean)
    stats: np.ndarray       # f32 [T, 2]: (rstd, nmr) of those rows
    gamma: np.ndarray       # f32 [768]
    beta: np.ndarray


def ln_apply_inputs(T: int) -> LnApplyInputs:
    g = torch.Generator(device="cpu").manual_seed(1000 + T)
    x = (3.0 * torch.randn((T, 768), generator=g) + 0.7).bfloat16()
    rstd, nmr = row_stats64(x.double().numpy())
    gamma = (1 + 0.25 * torch.randn((768,), generator=g)).numpy()
    beta = (0.25 * torch.randn((768,), generator=g)).numpy()
    return LnApplyInputs(x, np.stack([rstd, nmr], 1).astype(np.float32), gamma, beta)


def ln_apply64(i: LnApplyInputs):
    """k_ln_apply768: y = bf16(fma(fma(x, rstd, nmr), g, b)) from the f32 statistics it is handed: the float64 value of that
    expression and E = u (|g| |t| + |y|), t = x rstd + nmr: the inner fma rounds once (u |t|, scaled by |g|), the outer once (u |y|)."""
    x = i.x.double().numpy()
    t = x * i.stats[:, :1].astype(np.float64) + i.stats[:, 1:].astype(np.float64)
    ref = t * i.gamma.astype(np.float64) + i.beta.astype(np.float64)
    return ref, U32 * (np.abs(i.gamma.astype(np.float64)) * np.abs(t) + np.abs(ref))


# ---------------------------------------------------------------- coverage (DESIGN.md's table is checked against this)

def coverage(records, hard: bool = False) -> dict:
    """(kernel, epilogue, entry) -> [cases, ragged ones, multi-tile ones] over records / Cases: of the matrix proper, or (hard) of the
    hard LayerNorm rows that tests/ln_cases.py sends through the same kernels -- two tables in DESIGN.md."""
    out = {}
    for r in records:
        r = r._asdict() if isinstance(r, Case) else r
        if r["variant"] not in VARIANTS or r["variant"].startswith("hard_") != hard:      # (not in VARIANTS: no tiled kernel involved)
            continue
        entry, epi, _ = VARIANTS[r["variant"]]
        c = out.setdefault((r["kernel"], epi, entry), [0, 0, 0])
        c[0] += 1
        c[1] += is_ragged(r["kernel"], r["T"])
        c[2] += is_multi_tile(r["kernel"], r["T"], r["N"])
    return out


KERNEL_NAME = {"mid": "k_gemm_mid", "nt": "k_gemm_nt", "pp": "g256::k_gemm_pp"}


def coverage_table(records, hard: bool = False) -> str:
    """The markdown table of DESIGN.md: one line per (kernel, epilogue, entry): cases / ragged T / more than one tile."""
    cov = coverage(records, hard)
    lines = ["| kernel | epilogue | entry point | cases | ragged T | multi-tile |", "|---|---|---|---|---|---|"]
    for k in KERNELS:
        for (kk, epi, entry), (n, rag, multi) in sorted(cov.items(), key=lambda kv: (kv[0][1], kv[0][2])):
            if kk == k:
                lines.append(f"| `{KERNEL_NAME[k]}` | {epi} | `{entry}` | {n} | {rag} | {multi} |")
    return "\n".join(lines)


# ---------------------------------------------------------------- the child runner (the only GPU code of this file)

GUARD = 4                   # rows of sentinel in front of and behind every buffer a kernel writes
SENTINEL = 7.0


def _main(argv) -> int:
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", required=True, choices=KERNELS)
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    kernel = args.kernel
    for k, v in ENV[kernel].items():
        if os.environ.get(k) != v:
            print(f"gemm_cases: {k}={os.environ.get(k)!r}, the {kernel} matrix needs {v}", file=sys.stderr)
            return 2
    t_start = time.time()
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    dev = torch.device("cuda:0")
    L = ffi.lib()
    records, error, gpu_s = [], None, 0.0

    def guarded(rows, cols, dtype, init=None):
        """[GUARD + rows + GUARD, ...] of sentinel; -> (whole buffer, the rows in the middle)."""
        full = torch.full((rows + 2 * GUARD,) + tuple(cols), SENTINEL, dtype=dtype, device=dev)
        mid = full[GUARD: GUARD + rows]
        if init is not None:
            mid.copy_(init)
        return full, mid

    def guards_ok(full, rows):
        return bool((full[:GUARD] == SENTINEL).all()) and bool((full[GUARD + rows:] == SENTINEL).all())

    def sha(t):
        return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()

    def up(x, dtype=torch.float32):
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev, dtype)

    def call(fn, *a):
        nonlocal gpu_s
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = fn(*a)
        torch.cuda.synchronize()
        gpu_s += time.perf_counter() - t0
        ffi.check(rc)

    def run_shape(T, N, K):
        if kernel == "pp":
            assert pp_allowed(T, N, K), (T, N, K)
        x, g = exact_inputs(T, N, K), gelu_inputs(T, N, K)
        acc_e, acc_g = acc64(x.a, x.w), acc64(x.a, g.w)
        a_d, w_d, wg_d = up(x.a, torch.bfloat16), up(x.w, torch.bfloat16), up(g.w, torch.bfloat16)
        bias_d, gbias_d, gam_d, bet_d = up(x.bias), up(g.bias), up(x.ln_gamma), up(x.ln_beta)       # (all named: a temporary's block could be reused)
        for v in variants_for(T, N, K):
            entry, epi, kind = VARIANTS[v]
            rec = dict(id=f"{kernel}-{v}-{T}x{N}x{K}", kernel=kernel, variant=v, entry=entry, epilogue=epi, kind=kind, T=T, N=N, K=K,
                       ragged=is_ragged(kernel, T), multi_tile=is_multi_tile(kernel, T, N), diff_words=None, excess=None, stats_excess=None,
                       aux_excess=None, sha_stats=None)
            yf, y = guarded(T, (N,), torch.bfloat16)
            ok = True
            if v in ("bias", "bias_gelu"):
                call(L.crh_gemm_bf16_bias, a_d.data_ptr(), (w_d if v == "bias" else wg_d).data_ptr(), (bias_d if v == "bias" else gbias_d).data_ptr(),
                     y.data_ptr(), T, N, K, int(v == "bias_gelu"), 0)
            elif v in ("lnin", "lnin_gelu"):
                s = x if v == "lnin" else g
                rst = up(np.stack([s.rstd, s.nmr], 1))
                col, bf = up(s.colsum), up(s.bias)
                call(L.crh_gemm_bf16_lnin, a_d.data_ptr(), rst.data_ptr(), (w_d if v == "lnin" else wg_d).data_ptr(), col.data_ptr(), bf.data_ptr(),
                     y.data_ptr(), T, N, K, int(v == "lnin_gelu"), 0)
            elif v in ("res_raw", "res_norm"):
                res = up(x.res, torch.bfloat16)
                rst, gm = up(np.stack([x.rstd, x.nmr], 1)), up(x.gamma)
                pf, part = guarded(T, (24, 2), torch.float32)
                sf, st = guarded(T, (2,), torch.float32)
                call(L.crh_gemm_bf16_res_lnstats, a_d.data_ptr(), w_d.data_ptr(), bias_d.data_ptr(), res.data_ptr(), rst.data_ptr() if v == "res_norm" else None,
                     gm.data_ptr() if v == "res_norm" else None, LN_EPS, y.data_ptr(), part.data_ptr(), st.data_ptr(), T, N, K, 0)
                ok = guards_ok(pf, T) and guards_ok(sf, T)
                rec["stats_excess"] = stats_excess(st.cpu().numpy(), y.double().cpu().numpy())
                rec["sha_stats"] = sha(st)
            elif v in ("res_ln", "bias_lnres"):
                if v == "res_ln" and K <= 1024:         # in place: the only way to epilogue 2 at this K
                    y.copy_(up(x.res, torch.bfloat16))
                    res_ptr = y.data_ptr()
                else:
                    res = up(x.res, torch.bfloat16)
                    res_ptr = res.data_ptr()
                call(L.crh_gemm_bf16_bias_res_ln, a_d.data_ptr(), w_d.data_ptr(), bias_d.data_ptr(), res_ptr, gam_d.data_ptr(), bet_d.data_ptr(), LN_EPS,
                     y.data_ptr(), T, N, K, 0)
            elif v == "bias_res32_ln":
                rf, r32 = guarded(T, (N,), torch.float32, up(x.res32))
                call(L.crh_gemm_bf16_bias_res32_ln, a_d.data_ptr(), w_d.data_ptr(), bias_d.data_ptr(), r32.data_ptr(), gam_d.data_ptr(), bet_d.data_ptr(), LN_EPS,
                     y.data_ptr(), T, N, K, 0)
                ok = guards_ok(rf, T)
            got = y.cpu()
            if kind == "exact":
                rec["diff_words"] = int((got.view(torch.int16).numpy() != bf16_bits(exact_value(v, x, acc_e))).sum())
            elif v in ("bias_gelu", "lnin_gelu"):
                xin = gelu_x(v, x, g, acc_g)
                ref = gelu64(xin)
                rec["excess"] = float((np.abs(got.double().numpy() - ref) - gelu_bound(xin, ref)).max())
            else:
                ref, E = layernorm64(ln_pre(v, x, acc_e), x.ln_gamma, x.ln_beta)
                rec["excess"] = float((np.abs(got.double().numpy() - ref) - bf16_after(ref, E)).max())
                if v == "bias_res32_ln":
                    rec["aux_excess"] = float((np.abs(r32.double().cpu().numpy() - ref) - E).max())
            rec["guards_ok"] = ok and guards_ok(yf, T)
            rec["sha_out"] = sha(y)
            records.append(rec)

    def run_ln_apply(T):
        i = ln_apply_inputs(T)
        st, gm, bt = up(i.stats), up(i.gamma), up(i.beta)
        xf, xd = guarded(T, (768,), torch.bfloat16, i.x.to(dev))
        yf, y = guarded(T, (768,), torch.bfloat16)
        call(L.crh_layernorm_apply, xd.data_ptr(), st.data_ptr(), gm.data_ptr(), bt.data_ptr(), y.data_ptr(), T, 768, 0)
        untouched = bool(torch.equal(xd.cpu().view(torch.int16), i.x.view(torch.int16)))
        call(L.crh_layernorm_apply, xd.data_ptr(), st.data_ptr(), gm.data_ptr(), bt.data_ptr(), xd.data_ptr(), T, 768, 0)      # in place
        ref, E = ln_apply64(i)
        records.append(dict(id=f"{kernel}-ln_apply-{T}x768x0", kernel=kernel, variant="ln_apply", entry="crh_layernorm_apply", epilogue=None, kind="tol",
                            T=T, N=768, K=0, excess=float((np.abs(y.double().cpu().numpy() - ref) - bf16_after(ref, E)).max()),
                            diff_words=int((y.cpu().view(torch.int16) != xd.cpu().view(torch.int16)).sum()),     # in place against out of place
                            guards_ok=untouched and guards_ok(xf, T) and guards_ok(yf, T), sha_out=sha(y), stats_excess=None, aux_excess=None, sha_stats=None))

    rc = 0
    try:
        for (T, N, K) in SHAPES[kernel]:
            run_shape(T, N, K)
        if kernel == KERNELS[0]:
            for T in LN_APPLY_T:
                run_ln_apply(T)
        from tests import ln_cases
        from types import SimpleNamespace
        ln_cases.run_child(kernel, L, SimpleNamespace(dev=dev, guarded=guarded, guards_ok=guards_ok, sha=sha, up=up, call=call), records)
    except ffi.NativeError as e:        # an error return from the library: the one way to a non-zero exit that is not a crash
        error, rc = str(e), 3
    with open(args.out, "w") as f:
        json.dump(dict(kernel=kernel, error=error, wall_s=time.time() - t_start, gpu_call_s=gpu_s, records=records), f)
    return rc


if __name__ == "__main__":
    sys.exit(_main(sys.argv[1:]))
