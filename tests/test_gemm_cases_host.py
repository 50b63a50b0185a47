"""The premises of tests/test_gemm_matrix_gpu.py, proved without a GPU: the inputs of tests/gemm_cases.py are what their docstrings
say, f32 arithmetic on them is exact in any order (why the GPU file may compare BITS), the expected outputs do exercise the
rounding point, the shape lists reach the paths their comments name, and DESIGN.md's coverage table is the one the case lists give."""
import os

import numpy as np
import pytest
import torch

from tests import gemm_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_SHAPES = sorted({s for k in gc.KERNELS for s in gc.SHAPES[k]})
ALL_CASES = [c for k in gc.KERNELS for c in gc.cases(k)]
EXACT = [v for v, (_, _, kind) in gc.VARIANTS.items() if kind == "exact"]


def _sid(s):
    return "x".join(map(str, s))


def _bf16_exact(x) -> bool:
    t = torch.from_numpy(np.ascontiguousarray(x))
    return bool((t.bfloat16().float() == t).all())


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_sid)
def test_every_input_is_a_bf16_number_and_rows_are_distinct(shape):
    T, N, K = shape
    x, g = gc.exact_inputs(T, N, K), gc.gelu_inputs(T, N, K)
    # (ln_gamma / ln_beta are left out: arbitrary f32 parameters of the LayerNorm that FOLLOWS a GEMM, tolerance cases only; the
    # reference takes the same f32 numbers)
    for name in ("a", "w", "bias", "res", "res32", "rstd", "nmr", "colsum", "gamma"):
        v = getattr(x, name)
        assert (v is None) == (name in ("res", "res32") and N != 768), name
        if v is not None:
            assert v.dtype == np.float32 and _bf16_exact(v), name
    for name in ("w", "bias", "rstd", "nmr", "colsum"):
        assert _bf16_exact(getattr(g, name)), name
    assert x.a.shape == (T, K) and x.w.shape == (N, K) and g.w.shape == (N, K)
    assert set(np.unique(x.a)) <= set(range(-3, 4)) and set(np.unique(x.w)) <= {-1.0, 0.0, 1.0}
    assert len(np.unique(x.a, axis=0)) == T and len(np.unique(x.w, axis=0)) == N       # a wrong row / column cannot go unseen
    assert np.abs(x.bias).max() <= 1000 and (x.bias == np.round(x.bias)).all()
    assert set(np.unique(x.rstd)) <= {0.5, 1.0, 2.0} and set(np.unique(x.gamma)) <= {0.5, 1.0, 2.0}
    assert (np.abs(g.w).sum(1) == gc.GELU_NNZ).all() and (g.bias * 8 == np.round(g.bias * 8)).all()
    assert not np.array_equal(x.colsum, x.w.sum(1))                                      # epilogue 3's column sums are GIVEN


def _f32_orders(a: np.ndarray, w: np.ndarray, seed: int):
    """A . W^T summed in float32 in several orders: K shuffled (two permutations, BLAS chunks them its own way), then K cut into
    chunks of 32 added front to back and chunks of 64 added back to front -- the tiled kernels' k-steps, in both directions."""
    ta, tw = torch.from_numpy(a), torch.from_numpy(w)
    K = a.shape[1]
    rng = np.random.default_rng(seed)
    for _ in range(2):
        p = torch.from_numpy(rng.permutation(K))
        yield ta[:, p] @ tw[:, p].T
    for step, rev in ((32, False), (64, True)):
        ks = list(range(0, K, step))
        acc = torch.zeros((a.shape[0], w.shape[0]), dtype=torch.float32)
        for k0 in (ks[::-1] if rev else ks):
            acc = acc + ta[:, k0:k0 + step] @ tw[:, k0:k0 + step].T
        yield acc


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_sid)
def test_f32_sums_are_exact_in_any_order_and_so_is_every_exact_epilogue(shape):
    T, N, K = shape
    x, g = gc.exact_inputs(T, N, K), gc.gelu_inputs(T, N, K)
    f32 = np.float32
    for w in (x.w, g.w):
        assert (np.abs(x.a) @ np.abs(w).T).max() < 2 ** 24          # no partial sum of any order can leave the exact integers
        acc = gc.acc64(x.a, w)
        assert (acc == np.round(acc)).all()
        for got in _f32_orders(x.a, w, K):
            assert bool((got.double() == torch.from_numpy(acc)).all())
    acc = gc.acc64(x.a, x.w)
    a32 = acc.astype(f32)
    # the epilogues in float32, one rounding per operation where the kernels fuse two: on these inputs neither rounds at all
    got = {"bias": a32 + x.bias,
           "lnin": a32 * x.rstd[:, None] + (x.nmr[:, None] * x.colsum + x.bias)}
    if N == 768:
        got["res_raw"] = (a32 + x.bias) + x.res
        got["res_norm"] = (x.res * x.rstd[:, None] + x.nmr[:, None]) * x.gamma + (a32 + x.bias)
    assert sorted(got) == sorted(v for v in gc.variants_for(T, N, K) if v in EXACT)
    for v, y32 in got.items():
        assert y32.dtype == f32 and np.array_equal(y32.astype(np.float64), gc.exact_value(v, x, acc)), v
    accg = gc.acc64(x.a, g.w)
    g32 = accg.astype(f32)
    assert np.array_equal((g32 + g.bias).astype(np.float64), gc.gelu_x("bias_gelu", x, g, accg))
    assert np.array_equal((g32 * g.rstd[:, None] + (g.nmr[:, None] * g.colsum + g.bias)).astype(np.float64), gc.gelu_x("lnin_gelu", x, g, accg))
    if N == 768:        # the residual joins the rounded GEMM output in f32 without a rounding (k_layernorm768_res / _res32)
        y0 = gc.bf16_rne(gc.exact_value("bias", x, acc)).float().numpy()
        assert np.array_equal((y0 + x.res).astype(np.float64), y0.astype(np.float64) + x.res)
        assert np.array_equal((y0 + x.res32).astype(np.float64), gc.ln_pre("bias_res32_ln", x, acc))


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_sid)
def test_the_expected_outputs_exercise_the_rounding_point(shape):
    """ROUNDED_SHARE of an exact case's outputs are not bf16 numbers before pack2 rounds them, TIE_SHARE sit exactly half-way;
    and the GELU cases sample the curve where it bends: 40 % of the pre-activations inside (-4, 4), half of all off the
    integers, both tails present."""
    T, N, K = shape
    x, g = gc.exact_inputs(T, N, K), gc.gelu_inputs(T, N, K)
    acc = gc.acc64(x.a, x.w)
    for v in gc.variants_for(T, N, K):
        if v in EXACT:
            rounded, ties = gc.needs_rounding_share(gc.exact_value(v, x, acc))
            assert rounded >= gc.ROUNDED_SHARE and ties >= gc.TIE_SHARE, (v, rounded, ties)
    accg = gc.acc64(x.a, g.w)
    for v in ("bias_gelu", "lnin_gelu"):
        xin = gc.gelu_x(v, x, g, accg)
        assert (np.abs(xin) < 4).mean() >= 0.4 and (xin != np.round(xin)).mean() >= 0.5 and xin.min() < -4 and xin.max() > 4, v
        ref = gc.gelu64(xin)
        assert np.abs(ref - xin * 0.5 * (1 + torch.erf(torch.from_numpy(xin) / 2 ** 0.5).numpy())).max() < 1e-14


def test_the_layernorm_bound_holds_for_a_plain_float32_layernorm():
    """Not a tuning: a float32 LayerNorm written with numpy (its own summation order) stays inside the derived f32 term E, and E is
    a hundredth of the bf16 rounding it is added to at the median (it matters where the output crosses zero)."""
    x = gc.exact_inputs(300, 768, 3072)
    acc = gc.acc64(x.a, x.w)
    for v in ("res_ln", "bias_res32_ln"):
        pre = gc.ln_pre(v, x, acc)
        ref, E = gc.layernorm64(pre, x.ln_gamma, x.ln_beta)
        p = pre.astype(np.float32)
        assert np.array_equal(p.astype(np.float64), pre)
        mu = p.sum(-1, keepdims=True, dtype=np.float32) * np.float32(1 / 768)
        d = p - mu
        rstd = np.float32(1) / np.sqrt((d * d).sum(-1, keepdims=True, dtype=np.float32) * np.float32(1 / 768) + np.float32(gc.LN_EPS))
        y = d * rstd * x.ln_gamma + x.ln_beta
        assert y.dtype == np.float32 and (np.abs(y - ref) <= E).all()
        assert np.median(E / (gc.BF16_REL * np.abs(ref))) < 1e-2


def _nt_steps(T, N, K, cus=256):
    """Pipeline steps (tiles x k-steps) of every k_gemm_nt workgroup that has a tile: the tile-list arithmetic of the kernel and of
    xcd_grid (csrc/crh_encoder.hip), 32 workgroups per XCD label at most."""
    panels, nb, nk = -(-T // 256), N // 128, K // 64
    by_panel = panels >= 16
    busiest = -(-panels // 8) * nb if by_panel else -(-(panels * nb) // 8)
    bpx = max(1, min(busiest, cus // 8))
    units = panels if by_panel else panels * nb
    out = []
    for xcd in range(8):
        cnt = units // 8 + (1 if xcd < units % 8 else 0)
        mine = cnt * nb if by_panel else cnt
        out += [-(-(mine - jx) // bpx) * nk for jx in range(bpx) if jx < mine]
    return out


def test_the_shape_lists_reach_the_paths_their_comments_name():
    for k in gc.KERNELS:
        assert len(set(gc.SHAPES[k])) == len(gc.SHAPES[k])
        for (T, N, K) in gc.SHAPES[k]:
            assert T > 0 and N % 128 == 0 and K % 64 == 0, (k, T, N, K)         # what the public entries accept
        assert set(gc.PRODUCT_SHAPES) <= set(gc.SHAPES[k])
    assert all(gc.pp_allowed(*s) for s in gc.PP_SHAPES)
    assert not gc.pp_allowed(300, 128, 256) and not gc.pp_allowed(300, 256, 192) and not gc.pp_allowed(300, 256, 128)
    # k_gemm_nt's start-up branches: total == 1, == 2, == 3 steps for the workgroup, and the short K under a list of two tiles
    assert set(_nt_steps(1, 128, 64)) == {1} and len(_nt_steps(1, 128, 64)) == 1
    assert set(_nt_steps(255, 128, 128)) == {2}
    assert set(_nt_steps(257, 256, 192)) == {3} and len(_nt_steps(257, 256, 192)) == 4
    assert set(_nt_steps(4100, 2304, 64)) == {1, 2} and set(_nt_steps(4100, 2304, 128)) == {2, 4}
    assert max(_nt_steps(4100, 2304, 256)) == 8 and -(-3841 // 256) == 16 and -(-4100 // 256) == 17
    for s in gc.NT_SHAPES[:3]:
        assert s in gc.SHAPES["nt"]
    # k_gemm_mid's ring: K of one to four k-steps
    assert [K // 64 for (_, _, K) in gc.MID_SHAPES[:4]] == [1, 2, 3, 4]
    # shapes shared between the lists (what test_the_three_kernels_agree_to_the_bit compares)
    assert {(4100, 2304, 256), (3841, 768, 256)} <= set(gc.NT_SHAPES) & set(gc.PP_SHAPES) and (1, 128, 64) in set(gc.NT_SHAPES) & set(gc.MID_SHAPES)


def test_every_kernel_epilogue_pair_has_a_ragged_and_a_multi_tile_case_and_design_md_says_so():
    cov = gc.coverage(ALL_CASES)
    for k in gc.KERNELS:
        for epi in range(6):
            hit = [c for (kk, e, _), c in cov.items() if kk == k and e == epi]
            assert hit and sum(c[1] for c in hit) >= 1 and sum(c[2] for c in hit) >= 1, (k, epi)
    assert len({c.id for c in ALL_CASES}) == len(ALL_CASES)
    assert gc.coverage_table(ALL_CASES) in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_subtly_wrong_epilogues_change_bits_of_the_exact_cases():
    """What the bit comparison is there to catch, emulated on the CPU at the product's O-projection shape: each of these stays
    inside the random-input tolerance of the older tests (rel 2^-7 + abs 2e-3 at these magnitudes, or nearly) and each changes
    thousands of the expected words.  (One limit of the input set: the accumulator alone -- A in -3..3, W in -1..1 -- rarely leaves the
    integers bf16 holds, +-256, so a rounding of the accumulator BEFORE the bias would move a few words per case only; it is the
    bias that carries the sums to where rounding happens, and everything from the bias on is covered.)"""
    T, N, K = 300, 768, 768
    x = gc.exact_inputs(T, N, K)
    acc = gc.acc64(x.a, x.w)
    want = gc.bf16_bits(gc.exact_value("res_raw", x, acc))
    n = want.size

    def bits(v64):
        return gc.bf16_bits(np.asarray(v64, np.float64))

    def rne(v64):
        return gc.bf16_rne(np.asarray(v64, np.float64)).double().numpy()
    wrong = {
        "residual added after the rounding": bits(rne(acc + x.bias) + x.res),
        "truncation instead of round-to-nearest-even": (torch.from_numpy(gc.exact_value("res_raw", x, acc)).float().view(torch.int32).numpy() >> 16).astype(np.int16),
        "bias of the neighbouring 4-column group": bits(acc + np.roll(x.bias, 4) + x.res),
        "residual of the row above": bits(acc + x.bias + np.roll(x.res, 1, axis=0)),
        "the last k-step dropped": bits(gc.acc64(x.a[:, :-64], x.w[:, :-64]) + x.bias + x.res),
        # (integers: a quarter away from zero moves exactly the ties)
        "ties away from zero instead of to even": bits(gc.exact_value("res_raw", x, acc) + 0.25 * np.sign(gc.exact_value("res_raw", x, acc))),
    }
    for what, got in wrong.items():
        assert (got != want).sum() > n // 50, (what, int((got != want).sum()), n)
    # epilogues 3 and 5 with the statistics swapped or misplaced
    want3 = gc.bf16_bits(gc.exact_value("lnin", x, acc))
    swapped = acc * x.nmr[:, None] + (x.rstd[:, None].astype(np.float64) * x.colsum + x.bias)
    assert (bits(swapped) != want3).sum() > n // 50
    want5 = gc.bf16_bits(gc.exact_value("res_norm", x, acc))
    late = rne(acc + x.bias) + (x.res.astype(np.float64) * x.rstd[:, None] + x.nmr[:, None]) * x.gamma
    assert (bits(late) != want5).sum() > n // 50
