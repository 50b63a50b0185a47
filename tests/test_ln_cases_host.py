"""The premises of the hard LayerNorm rows (tests/ln_cases.py), proved without a GPU: the families are what their table says; the
kernels' documented arithmetic, emulated in np.float32, stays inside the derived tolerance on every element of every family; each
mistake the families are there for leaves it by a factor of two at least, while on the `unit` row alone -- all the older tests had --
the eps and one-pass mistakes stay far inside; epilogue 5's statistics, emulated, stay inside stats_bound."""
import os

import numpy as np
import pytest

from tests import gemm_cases as gc
from tests import ln_cases as lc

EPSES = (lc.EPS, lc.EPS_ALT)
OTHER = {lc.EPS: lc.EPS_ALT, lc.EPS_ALT: lc.EPS}


def _ratio(f, eps, mutant=None, run_eps=None, divide=False):
    """Worst |bf16(emulation) - float64 reference| / tolerance over the row's 768 elements; run_eps: the eps the emulation uses
    when it is not the one the call passed."""
    ref, tol = lc.tolerance(f.row.astype(np.float64)[None], eps)
    y = lc.ln_f32(f.row[None], eps if run_eps is None else run_eps, mutant, divide)
    return lc.worst_ratio(lc.bf16(y), ref, tol)


def test_the_families_are_what_the_table_says():
    fs = {f.name: f for f in lc.all_families()}
    assert len(fs) == 17 and len(lc.families("bf16")) == 15 and len(lc.families("f32")) == 17
    assert [f.name for f in lc.families("f32", lc.EPS_ALT)] == ["unit", "small", "tiny"] == [f.name for f in lc.families("bf16", lc.EPS_ALT)]
    for f in fs.values():
        assert f.row.dtype == np.float32 and f.row.shape == (768,) and lc.is_bf16(f.p) and lc.is_bf16(f.q)
        assert np.array_equal(f.p + f.q, f.row) and (f.p + f.q).dtype == np.float32       # the kernels' f32 addition IS the row
        assert lc.is_bf16(f.row) != f.f32_only
        assert np.isfinite(f.row).all() and np.abs(f.row).max() <= 2.0 ** 40
    var = {n: float(f.row.astype(np.float64).var()) for n, f in fs.items()}
    mean = {n: float(f.row.astype(np.float64).mean()) for n, f in fs.items()}
    assert 0.8 < var["unit"] < 1.2 and 0.5e-6 < var["small"] < 2e-6 < lc.EPS and 0.5 * 2.0 ** -40 < var["tiny"] < 2.0 ** -39
    assert var["zero"] == 0 and var["const_1000"] == 0 and var["const_m3"] == 0 and mean["const_1000"] == 1000 and mean["const_m3"] == -3
    assert fs["one_hot"].row[5] == 1 and fs["one_hot"].row.sum() == 1
    for n, c in (("offset_coarse_1000", 1000), ("offset_coarse_64", 64), ("offset_fine_1000", 1000), ("offset_fine_m256", -256)):
        assert abs(mean[n] - c) < 0.2 and abs(c) / np.sqrt(var[n]) > 40, n
    assert 0.2 < var["offset_fine_1000"] < 0.3 and 0.012 < var["offset_fine_m256"] < 0.02
    for col in (0, 255, 256, 767):      # lane 0's first and lane 63's last column of the first chunk, the second chunk's first, the row's last
        r = fs[f"outlier_{col}"].row
        assert abs(r[col]) == 4096 and np.abs(np.delete(r, col)).max() < 8
    assert set(fs["two_level"].row) == {-1024.0, 1024.0} and var["two_level"] == 1024.0 ** 2 and mean["two_level"] == 0
    assert 0.8 * 2.0 ** 60 < var["big"] < 1.2 * 2.0 ** 60
    # first five of either site: the three eps families and a hard row of two more kinds
    assert {f.name for f in lc.families("bf16")[:5]} == {"unit", "small", "tiny", "outlier_767", "offset_coarse_1000"}
    assert {f.name for f in lc.families("f32")[:5]} == {"unit", "small", "tiny", "outlier_767", "offset_fine_1000"}
    assert lc.hard_T("bf16") == (15, 5, 1) and lc.hard_T("f32") == (17, 5, 1) and lc.hard_T("f32", lc.EPS_ALT) == (3,)


def test_the_second_order_premise_of_layernorm64_holds_for_every_row_used():
    """layernorm64's docstring: (Vmax / sigma) |z| <= 4 / (200 u), sigma with eps; the embedding test's pad row included."""
    rows = [f.row.astype(np.float64) for f in lc.all_families()] + [lc.embed_inputs(lc.EPS).pad_v]
    for eps in EPSES:
        for v in rows:
            sigma = np.sqrt(v.var() + eps)
            assert np.abs(v).max() / sigma * np.abs((v - v.mean()) / sigma).max() <= lc.SECOND_ORDER_LIMIT


@pytest.mark.parametrize("divide", [False, True], ids=["times_1_768", "divide_768"])
def test_the_float32_emulation_stays_within_the_tolerance_on_every_element(divide):
    """Every (family, eps) the GPU tier runs, both ways of scaling the sums (k_layernorm768* / k_embed_ln), no element left out; and
    what is left of the tolerance is the bf16 rounding: the worst ratio is above one half somewhere."""
    worst = 0.0
    for eps in EPSES:
        for f in lc.families("f32", eps):
            r = _ratio(f, eps, divide=divide)
            assert r <= 1.0, (f.name, eps, r)
            worst = max(worst, r)
    assert worst > 0.5
    v = lc.embed_inputs(lc.EPS).pad_v
    ref, tol = lc.tolerance(v[None], lc.EPS)
    assert lc.worst_ratio(lc.bf16(lc.ln_f32(v[None].astype(np.float32), lc.EPS, divide=divide)), ref, tol) <= 1.0


# mutant -> the families that must catch it (each of them, at every eps it runs at): by a factor of 2 over the tolerance at least
MUST_CATCH = {"no_eps": ("small", "tiny"),
              "eps_outside": ("small", "tiny"),
              "n767": ("unit", "big"),
              "one_pass": ("offset_fine_1000", "offset_fine_m256"),
              "skip_last_chunk": ("outlier_767", "offset_fine_1000", "offset_fine_m256")}


@pytest.mark.parametrize("mutant", sorted(MUST_CATCH))
def test_each_mistake_leaves_the_tolerance_on_the_families_named_for_it(mutant):
    for name in MUST_CATCH[mutant]:
        r = _ratio(lc.family(name), lc.EPS, mutant)        # (at 1e-12 an eps left out or misplaced is no mistake worth the name)
        assert r >= 2.0, (mutant, name, r)


def test_an_eps_that_ignores_the_argument_leaves_the_tolerance():
    """eps fixed at 1e-5 when the call passes 1e-12, and the reverse: small and tiny."""
    for name in ("small", "tiny"):
        for eps in EPSES:
            r = _ratio(lc.family(name), eps, run_eps=OTHER[eps])
            assert r >= 2.0, (name, eps, r)


def test_on_the_unit_row_alone_the_eps_and_one_pass_mistakes_stay_hidden():
    """Why the families were needed: at variance 1 the three eps mistakes reach a tenth of the tolerance at most and a one-pass
    variance a hundredth."""
    f = lc.family("unit")
    _, tol = lc.tolerance(f.row.astype(np.float64)[None], lc.EPS)
    y0 = lc.ln_f32(f.row[None], lc.EPS).astype(np.float64)

    def moved(mutant=None, run_eps=lc.EPS):
        """How far the mistake moves the f32 result, in units of the tolerance (worst element)."""
        return float((np.abs(lc.ln_f32(f.row[None], run_eps, mutant).astype(np.float64) - y0) / tol).max())
    assert 0 < moved("no_eps") < 0.1 and 0 < moved("eps_outside") < 0.1 and 0 < moved(run_eps=lc.EPS_ALT) < 0.1
    assert moved("one_pass") < 0.01
    for m in ("no_eps", "eps_outside", "one_pass"):         # and the bf16 result stays inside the tolerance: nothing fails
        assert _ratio(f, lc.EPS, m) <= 1.0
    assert _ratio(f, lc.EPS, run_eps=lc.EPS_ALT) <= 1.0


def test_the_statistics_emulation_stays_within_stats_bound():
    """LnAcc / ln_join / k_ln_finalize in np.float32 on every bf16 family, both eps: inside the derived bound, and on the rows of order
    one inside the older constants too (the derived bound is not what lets them pass)."""
    for eps in EPSES:
        fs = lc.families("bf16", eps)
        rows = lc.rows64(fs)
        got = lc.lnacc_f32(rows, eps)
        b = lc.stats_bound(rows, eps)
        assert (np.abs(got[:, 0] - b.rstd) <= b.rel_rstd * b.rstd).all(), [f.name for f in fs]
        assert (np.abs(got[:, 1] - b.nmr) <= b.d_nmr).all()
        assert lc.hard_stats_excess(got, rows, eps) <= 0
    unit = lc.rows64([lc.family("unit")])
    assert gc.stats_excess(lc.lnacc_f32(unit, lc.EPS), unit) <= 0
    b = lc.stats_bound(unit, lc.EPS)
    assert 0.5 * gc.STATS_RTOL < b.rel_rstd[0] < 2 * gc.STATS_RTOL       # a unit row: the derivation lands where the constant is
    # statistics that lose a lane's last fragment, or a slot, leave the bound on the rows built for it
    hard = lc.rows64([lc.family("outlier_767"), lc.family("offset_coarse_1000")])
    cut = hard.copy()
    cut[:, 764:] = cut[:, 760:764]
    assert lc.hard_stats_excess(lc.lnacc_f32(cut, lc.EPS), hard, lc.EPS) > 0


def test_the_device_statistics_tolerance_is_the_chain_plus_the_propagated_bound():
    """dev_stats_tolerance: the emulated statistics fed through the apply chain / the consumer chain in np.float32 stay inside."""
    gam, bet = lc.ln_params()
    fs = lc.families("bf16")
    rows = lc.rows64(fs)
    st = lc.lnacc_f32(rows, lc.EPS)
    x = rows.astype(np.float32)
    y = lc._fma(lc._fma(x, st[:, :1], st[:, 1:]), gam[None], bet[None])
    ref, tol = lc.dev_stats_tolerance(rows, lc.EPS, gam, consumer=False)
    assert lc.worst_ratio(lc.bf16(y), ref, tol) <= 1.0
    g = lc.bf16(gam)
    y = lc._fma(x * g[None], st[:, :1], lc._fma(st[:, 1:], g[None], bet[None]))
    ref, tol = lc.dev_stats_tolerance(rows, lc.EPS, g, consumer=True)
    assert lc.worst_ratio(lc.bf16(y), ref, tol) <= 1.0
    # and it has teeth where the statistics matter: rstd without eps on the small row leaves it
    small = lc.rows64([lc.family("small")])
    bad = lc.lnacc_f32(small, 0.0)
    y = lc._fma(lc._fma(small.astype(np.float32), bad[:, :1], bad[:, 1:]), gam[None], bet[None])
    ref, tol = lc.dev_stats_tolerance(small, lc.EPS, gam, consumer=False)
    assert lc.worst_ratio(lc.bf16(y), ref, tol) >= 2.0


def test_the_embedding_tables_give_the_family_rows_and_the_cases_are_listed_once():
    for eps in EPSES:
        e = lc.embed_inputs(eps)
        fs = lc.families("f32", eps)
        assert lc.is_bf16(e.word) and lc.is_bf16(e.pos) and not e.type0.any()
        assert e.seqs[0].count(lc.PAD_ID) == 1 and e.seqs[0][2] == lc.PAD_ID and all(len(s) % 16 for s in e.seqs)
        real = [t for t in e.seqs[0] if t != lc.PAD_ID]
        assert real == [3 + r for r in range(len(fs))]
        got = e.v[0][[k for k, t in enumerate(e.seqs[0]) if t != lc.PAD_ID]]
        assert np.array_equal(got, lc.rows64(fs))
        assert np.array_equal(e.v[1], lc.rows64(fs)[:len(e.seqs[1])]) and np.array_equal(e.v[2], lc.rows64(fs)[:1])
    ids = [c.id for k in gc.KERNELS for c in gc.cases(k)]
    assert len(set(ids)) == len(ids)
    for k in gc.KERNELS:
        mine = lc.cases(k)
        assert {c.variant for c in mine} >= set(lc.AGREE) and all(gc.pp_allowed(c.T, 768, c.K) for c in mine if c.K)
        assert ({c.variant for c in mine} & set(lc.NO_GEMM_VARIANTS) == set(lc.NO_GEMM_VARIANTS)) == (k == gc.KERNELS[0])


def test_design_md_tabulates_the_hard_row_cases_beside_the_matrix():
    """Two tables: the matrix proper (unchanged by the hard rows; tests/test_gemm_cases_host.py) and what the hard rows add."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cases = [c for k in gc.KERNELS for c in gc.cases(k)]
    design = open(os.path.join(root, "DESIGN.md")).read()
    assert gc.coverage_table(cases, hard=True) in design and gc.coverage_table(cases) in design
    assert gc.coverage_table(cases) == gc.coverage_table([c for c in cases if not c.variant.startswith("hard_")])
    hard = gc.coverage(cases, hard=True)
    assert sum(n for n, _, _ in hard.values()) == sum(c.variant in lc.AGREE for c in cases)
    for k in gc.KERNELS:
        assert {e for (kk, e, _) in hard if kk == k} == {0, 2, 3, 5}
