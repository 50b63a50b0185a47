"""The preconditions of tests/test_margin_gpu.py, proved without a GPU on exactly the inputs that file runs
(tests/margin_cases.py) and against oracle/search only: the adversarial pair is stored as built, the oracle ranks A first, a scan
over the bf16 images moves B at least 1e-2 up against A, and no row's scan error exceeds the bound margin_for must use; every
boundary row has the len2 bits it claims, and the oracle keeps or divides it as the builder says."""
import numpy as np
import pytest

from oracle import search as orc
from tests import margin_cases as mc

U32, F32 = np.uint32, np.float32


def _bits_equal(a, b) -> bool:
    return np.array_equal(np.ascontiguousarray(a, F32).view(U32), np.ascontiguousarray(b, F32).view(U32))


@pytest.mark.parametrize("variant", mc.VARIANTS)
@pytest.mark.parametrize("dim", mc.DIMS)
def test_adversarial_pair_preconditions(dim, variant):
    q, a, b, scan = mc.adversarial_pair(dim, variant)
    both = np.stack([a, b])
    for v in (q, a, b):
        assert v.shape == (dim,) and abs(float(mc.len2(v)) - 1.0) <= mc.UNIT_TOL
        assert _bits_equal(orc.preprocess(v)[0], v)                        # stored / used verbatim
    # no two vectors share a filler position: the fillers add nothing to any score
    fill = [np.flatnonzero(v[dim - 36:]) for v in (q, a, b)]
    assert all(f.size for f in fill) and not (set(fill[0]) & set(fill[1])) and not (set(fill[0]) & set(fill[2]))
    assert all(_bits_equal(mc.bf16_round(v[dim - 36:]), v[dim - 36:]) for v in (q, a, b))
    s, r = orc.cosine_search(both, q, 2)
    assert r.tolist() == [[0, 1]] and s[0, 0] > s[0, 1]                    # the oracle ranks A above B, strictly
    canon = orc.scores(both, q)[0].astype(np.float64)
    model = np.asarray([scan(q, a), scan(q, b)])
    assert model[1] - model[0] - (canon[1] - canon[0]) >= mc.MIN_SWING
    assert model[1] > model[0]                                             # the scan alone ranks them the other way round
    for x, c, m in zip(both, canon, model):
        weight = float(np.abs(q.astype(np.float64) * x.astype(np.float64)).sum())
        assert weight <= 1.0 + 1e-6                                        # (Cauchy-Schwarz on unit vectors)
        exact = float(np.dot(q.astype(np.float64), x.astype(np.float64)))
        assert abs(m - exact) <= mc.PRODUCT_BOUND * weight
        assert abs(exact - c) <= dim * 2.0 ** -24                          # the canonical sum's own f32 error
        # ... and the term the code used before, 2 * 2^-9 + 2^-18 = 3.92e-3, does not hold for unit vectors
        assert abs(m - exact) > (2 * 2.0 ** -9 + 2.0 ** -18) * 1.0
    # a bf16 store scans what it ranks by: the model IS the canonical score of the rounded operands, up to the f32 sum
    rounded = orc.scores(mc.bf16_round(both), mc.bf16_round(q))[0]
    assert np.abs(rounded - model).max() <= dim * 2.0 ** -24


def test_the_pair_is_the_same_at_every_dim():
    """Zeros add nothing to a sequential sum: scores and lengths do not depend on dim, only the fillers' positions do."""
    for variant in mc.VARIANTS:
        ref = None
        for dim in mc.DIMS:
            q, a, b, _ = mc.adversarial_pair(dim, variant)
            got = (orc.dot(q, a), orc.dot(q, b), float(mc.len2(q)), float(mc.len2(a)), float(mc.len2(b)))
            ref = ref or got
            assert got == ref
    q, a, b, scan = mc.adversarial_pair(768, "plain")
    assert round(orc.dot(q, a), 6) == 0.661551 and round(orc.dot(q, b), 6) == 0.661467
    assert round(scan(q, a), 6) == 0.656494 and round(scan(q, b), 6) == 0.666544


def test_signed_variant_has_negative_products_under_both_rows():
    q, a, b, scan = mc.adversarial_pair(384, "signed")
    assert (q >= 0).all() and (a[:mc.SIGNED] < 0).all() and (b[mc.H:mc.H + mc.SIGNED] < 0).all()
    neg_a, neg_b = (q * a)[:mc.SIGNED].astype(np.float64), (q * b)[mc.H:mc.H + mc.SIGNED].astype(np.float64)
    ra = (mc.bf16_round(q) * mc.bf16_round(a))[:mc.SIGNED].astype(np.float64)
    rb = (mc.bf16_round(q) * mc.bf16_round(b))[mc.H:mc.H + mc.SIGNED].astype(np.float64)
    assert (ra < neg_a).all() and (rb > neg_b).all()                       # A's negative terms grow, B's shrink


def test_bf16_round_is_the_oracles():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(2000).astype(F32), mc.bf16_tie_row(384), [0.0, -0.0, 1e-40, -3e-39, 3.3e38]]).astype(F32)
    L = orc._load()
    assert _bits_equal(mc.bf16_round(x), np.asarray([L.orc_bf16_round(float(v)) for v in x], F32))


@pytest.mark.parametrize("dim", mc.DIMS)
def test_boundary_rows_have_their_len2_and_their_fate(dim):
    b = mc.boundary_rows(dim)
    pre = orc.preprocess(b.raw)
    by = dict(zip(b.names, range(len(b.names))))
    for name, (target, div) in mc.LEN2_TARGETS.items():
        v = b.raw[by[name]]
        assert np.cumsum(v * v, dtype=F32)[-1:].view(U32)[0] == np.asarray([target], F32).view(U32)[0], name
        assert np.count_nonzero(v) == dim and (v < 0).any() and (v > 0).any()
        assert b.divided[by[name]] == div
    t = {n: mc.LEN2_TARGETS[n][0] for n in mc.LEN2_TARGETS}
    assert t["eps-1ulp"] < mc.FLT_EPSILON == t["eps"] < t["eps+1ulp"] and mc.FLT_EPSILON == np.finfo(F32).eps
    assert np.abs(t["1-16ulp"] - F32(1)) <= F32(1e-6) < np.abs(t["1-17ulp"] - F32(1))
    assert np.abs(t["1+8ulp"] - F32(1)) <= F32(1e-6) < np.abs(t["1+9ulp"] - F32(1))
    assert np.nextafter(t["1-17ulp"], F32(2)) == t["1-16ulp"] and np.nextafter(t["1+8ulp"], F32(2)) == t["1+9ulp"]
    # the oracle keeps exactly the rows the builder says it keeps, and changes every other one
    for i, name in enumerate(b.names):
        assert _bits_equal(pre[i], b.raw[i]) == (not b.divided[i]), name
    # order: sequentially every addend is a tie that rounds back to 1.0; any pairwise or fused sum sees 64 * 2^-24
    v = b.raw[by["order"]]
    sq = v * v
    assert mc.len2(v) == F32(1.0) and sq[0] == 1 and (sq[1:65] == F32(2.0 ** -24)).all() and not sq[65:].any()
    assert F32(sq[0] + np.sum(sq[1:], dtype=F32)) == F32(1 + 64 * 2.0 ** -24)           # the small terms first: exact
    assert np.abs(np.sum(sq, dtype=F32) - F32(1)) > F32(1e-6)                           # numpy's own pairwise sum would divide too
    assert abs(float(np.dot(v.astype(np.float64), v.astype(np.float64))) - 1.0) > 1e-6
    # overflow: finite elements, infinite len2, signed zeros out
    v, p = b.raw[by["overflow"]], pre[by["overflow"]]
    assert np.isfinite(v).all() and np.isinf(mc.len2(v)) and not p.any()
    assert np.array_equal(np.signbit(p), np.signbit(v)) and np.signbit(p).any()
    # large: a finite len2 near the top of the range, a unit row out, one subnormal quotient
    v, p = b.raw[by["large"]], pre[by["large"]]
    assert 5e37 < mc.len2(v) < 2e38
    assert abs(float(np.dot(p.astype(np.float64), p.astype(np.float64))) - 1.0) < 2 * dim * 2.0 ** -24      # (len2's own sequential f32 error)
    assert 0 < p[5] < np.finfo(F32).tiny
    # subnormal: the small inputs stay non-zero and subnormal through the division, to the oracle's bits
    v, p = b.raw[by["subnormal"]], pre[by["subnormal"]]
    small = np.flatnonzero((v != 0) & (np.abs(v) < 1e-30))
    assert small.size == 7 and (p[small] != 0).all() and (np.abs(p[small]) < np.finfo(F32).tiny).all()
    assert np.array_equal(np.signbit(p[small]), np.signbit(v[small]))
    want = (v.astype(np.float64) / np.float64(np.sqrt(F32(1.25)))).astype(F32)      # one correctly rounded division per element
    assert _bits_equal(p, want)
    assert not b.raw[by["zero"]].any() and not pre[by["zero"]].any()


@pytest.mark.parametrize("dim", mc.DIMS)
def test_verbatim_rows_hold_every_kind_of_bf16_tie(dim):
    v = mc.boundary_rows(dim).verbatim
    assert v.shape == (2, dim) and np.isfinite(v).all() and all(float(mc.len2(r)) < 1.0 for r in v)
    u = v[0, :256].view(U32)
    low, odd = u & U32(0xffff), (u >> U32(16)) & U32(1)
    kinds = {(int(l), int(o)) for l, o in zip(low, odd)}
    assert kinds == {(0x7fff, 0), (0x8000, 0), (0x8000, 1), (0x8001, 0)}
    rb =mc.bf16_round(v[0, :256]).view(U32) >> U32(16)
    up = rb == (u >> U32(16)) + U32(1)
    assert np.array_equal(up, (low == 0x8001) | ((low == 0x8000) & (odd == 1)))
    assert ((u >> U32(16)) & U32(0x7f) == 0x7f).any() and (v[0] < 0).any() and (v[0] > 0).any()      # a carry into the exponent; both signs
    carried = up & ((u >> U32(16)) & U32(0x7f) == 0x7f)
    assert carried.any() and (np.abs(mc.bf16_round(v[0, :256])[carried]) == F32(2.0 ** -4)).all()
