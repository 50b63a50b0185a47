"""What the int8 scan computes BEFORE it nominates, against the oracle (code-rag_amd/csrc/crh_i8.hpp, k_scan_i8).

Every other int8 test compares final ids and score bits, which an interval a few per cent too narrow passes for thousands of
queries and an interval too wide passes for ever.  Here crh_debug_i8_intervals (debug library only) returns the product kernels'
own numbers -- both ends of every (query, row) interval, srow, qpar, dn, c_abs, tau_q -- and each case of tests/i8_cases.py checks

  soundness   lo <= score <= hi for the oracle's canonical f32 score and for the fp64 dot, every row, every query, no exception;
              the recorded (bf16, rounded up) upper end is no lower than the f32 one;
  threshold   tau_q <= the oracle's k-th score over alive, unfiltered rows (k = 1, 10, 100, 256), -inf with fewer than k such rows;
  parameters  srow, s_q to the bit; dn, Qn, gn no smaller than the fp64 norms they bound; zero rows and queries: scale 0, [-c, c];
  tightness   dn, gn, Qn no larger than the kernel's constants allow plus what its f32 evaluation can add, and (hi - lo) / 2 equal
              to the half-width those constants give, from both sides, to within that evaluation's roundings;
  branches    the same query gives the same bits alone and as query 0 and query 40 of a 64-query call.  (Which branch of
              intervals() runs goes with the DIMENSION, not with nq: 1536 takes 32 queries per pass and pairs rows, the other
              widths pair query blocks; each is covered by the cases of its widths, and query 40 of a 1536-wide call is slot 8
              of the second pass.)

Recorded, not asserted: the median half-width of the Gaussian D = 768 case (python -m pytest -s prints it) -- see
test_intervals_against_the_oracle's docstring.
"""
import numpy as np
import pytest

from oracle import search as orc
from tests import i8_cases as ic

pytestmark = pytest.mark.gpu

CASES = ic.cases()
F32_EPS = 2.0 ** -24          # half an ulp, relative: one f32 rounding


def _ffi():
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    return ffi


@pytest.fixture(autouse=True)
def debug_library(gpu, monkeypatch):
    """Every index of this file lives in the debug build (the two libraries do not share handles): same sources, same kernels."""
    ffi = _ffi()
    monkeypatch.setattr(ffi, "_lib", ffi.debug_lib())
    return ffi


def _build(ffi, case):
    """The index of a case, the rows it holds (the oracle's preprocessing; checked against read_rows), who is alive, the codes, and
    the largest |d|_2 of any row the copy ever quantised."""
    raw, kind = ic.build_raw(case)
    n = len(raw)
    dead, codes = ic.tombstones_and_codes(case)
    dtype = ffi.DTYPE_BF16 if case.bf16 else ffi.DTYPE_F32
    idx = ffi.Index(case.dim, dtype, capacity_rows=case.n, n_code_cols=1)
    ever = raw
    if case.corpus == "mutated":
        full = ic.mixed_corpus(case.dim, case.n, case.seed)[0]
        first, second, gone = ic.mutation_plan(case)
        keep = np.concatenate([np.setdiff1d(first, gone), second])
        codes_full = np.zeros((case.n, 1), np.int32)
        codes_full[keep] = codes
        idx.append(full[first], codes_full[first])
        idx.search(full[:4], 10)                                     # quantises the first lot: dn is now their maximum
        idx.append(full[second], codes_full[second])
        idx.tombstone(np.searchsorted(first, gone))
        o2n = idx.compact()
        assert int((o2n >= 0).sum()) == n
        ever = full
    else:
        idx.append(raw, codes)
    idx.tombstone(dead)
    assert idx.nomination() == ffi.NOMINATE_INT8
    stored = orc.preprocess(raw, case.bf16)
    assert np.array_equal(idx.read_rows(0, n).view(np.uint32), stored.view(np.uint32)), "the index holds other rows than the oracle's preprocessing gives"
    alive = np.ones(n, bool)
    alive[dead] = False
    d_ever = np.linalg.norm(ic.quantise(orc.preprocess(ever, case.bf16), 127.0)[2], axis=1).max()
    return idx, raw, kind, stored, alive, codes[:, 0], d_ever


def _worst(viol, lo, s, hi):
    q, r = np.unravel_index(int(np.argmax(viol)), viol.shape)
    return f"{int((viol > 0).sum())} violations; worst: query {q} row {r} lo {lo[q, r]!r} score {s[q, r]!r} hi {hi[q, r]!r}"


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_intervals_against_the_oracle(debug_library, case):
    """Measured on an MI355X, Gaussian rows and queries, D = 768, 59 999 rows: median half-width 8.64e-3 with dn = 8.78 (bf16
    store) and 8.44e-3 with dn = 8.55 (f32 store); over all eight kinds of query 8.75e-3 / 8.52e-3.  The header of crh_i8.hpp
    stated 8.3e-3 and max |d| 8.6: that was dn (|Q| + |g|) + 127 sqrt(D) |g| without the + 0.25 on gn, the 2e-3 on dn, kDotRound
    and c, at a smaller maximum |d|_2; the header now carries the measured figures."""
    ffi = debug_library
    idx, raw, kind, stored, alive, codes, d_ever = _build(ffi, case)
    try:
        n, dim = stored.shape
        q, qkinds = ic.queries_for(dim, case.nq, case.seed, raw, kind, stored)
        qc = orc.preprocess(q, case.bf16)
        o = ffi.debug_i8_intervals(idx._handle(), n, dim, q, ic.KS[0])
        hi, lo, rec = o["hi"], o["lo"], o["hi_rec"]
        c = float(o["c_abs"])
        assert o["c_abs"] == ic.c_abs(dim)

        # ---- soundness
        canon = orc.scores(stored, qc).astype(np.float64)
        fp64 = qc.astype(np.float64) @ stored.astype(np.float64).T
        assert np.isfinite(hi).all() and np.isfinite(lo).all()
        for name, s in (("canonical f32", canon), ("fp64", fp64)):
            viol = np.maximum(lo - s, s - hi)
            assert viol.max() <= 0, f"{case.id} {name}: " + _worst(viol, lo, s, hi)
        assert np.all(rec >= hi), "a recorded upper end below the f32 upper end"

        # ---- quantisation parameters
        s_r, X, d, _ = ic.quantise(stored, 127.0)
        s_q, Q, g, _ = ic.quantise(qc, ic.LEVELS)
        assert np.array_equal(o["srow"].view(np.uint32), s_r.view(np.uint32))
        qpar = o["qpar"]
        assert np.array_equal(qpar[:case.nq, 0].view(np.uint32), s_q.view(np.uint32)) and not qpar[case.nq:].any() and not qpar[:, 3].any()
        dn, Qn, gn = float(o["dn"]), qpar[:case.nq, 1].astype(np.float64), qpar[:case.nq, 2].astype(np.float64)
        d_norm, Q_norm, g_norm = np.linalg.norm(d, axis=1), np.linalg.norm(Q, axis=1), np.linalg.norm(g, axis=1)
        assert dn >= d_norm.max() and dn >= d_ever, (dn, d_norm.max(), d_ever)
        assert np.all(Qn >= Q_norm) and np.all(gn >= g_norm)
        zero_q, zero_r = s_q == 0, s_r == 0
        assert zero_q.sum() >= sum(k == "zero" for k in qkinds) and not gn[zero_q].any() and not Qn[zero_q].any()
        for sel in ((slice(None), zero_r), (zero_q, slice(None))):       # scale 0: the interval is [-c, c] (- lower_end's 2e-6)
            assert np.all(hi[sel] == o["c_abs"]) and np.all(lo[sel] <= -c) and np.all(lo[sel] >= -c - 2e-6 - 4 * F32_EPS)
        if case.corpus != "gaussian":
            assert zero_r.sum() >= 100

        # ---- tightness.  What the f32 evaluation may ADD to the constants' own half-width:
        #   hi = fma(w, f + B, c): w, f + B and the fma round once each, <= 2^-24 relative on terms no larger than |hi| + the width;
        #   lo = hi - 2 fma(w', B, c) - 2e-6: w', the fma, the two subtractions, on terms no larger than |hi| + |lo| + the width.
        #   Eight roundings of at most 2^-24 (|hi| + |lo| + 2 hw) each bound it; the record adds its round-up, <= 2^-7 |hi| on the
        #   upper end alone, i.e. 2^-8 |hi| on the half-width.  Nothing here comes from the kernel's output but the operands' sizes.
        ref = ic.half_width_fp64(o["srow"], qpar[:case.nq], o["dn"], o["c_abs"], dim)
        hw = (hi.astype(np.float64) - lo) / 2
        room = 8 * F32_EPS * (np.abs(hi) + np.abs(lo) + 2 * ref)
        assert np.all(hw <= ref + room), f"half-widths beyond the constants: worst excess {(hw - ref - room).max():.3e}"
        #   ... nor may it fall short by more: a dropped term or allowance narrows EVERY interval at once, long before a score of
        #   these inputs falls outside one (where dn (|Q| + gn) is large it hides a missing 127 sqrt(D) gn or kDotRound from the
        #   soundness check; the same eight roundings bound the shortfall).
        assert np.all(hw >= ref - room), f"half-widths short of the constants: worst shortfall {(ref - room - hw).max():.3e}"
        assert np.all((rec.astype(np.float64) - lo) / 2 <= ref + room + 2.0 ** -8 * np.abs(rec))
        #   dn: sqrtf(dsq) * 1.0001 + 2e-3 where sqrtf(dsq) is off the true norm by what the 2e-3 was derived for (the f32 images
        #   move every d_i by <= 127 (2^-23 + 2^-22): < 2e-3 over 1536 elements) -- over-estimating is as possible as under-estimating --
        #   plus three roundings; gn and Qn the same way with their own constants.
        assert dn <= 1.0001 * d_ever + 2e-3 + (1.0001 * 2e-3 + 3 * F32_EPS * dn), (dn, d_ever)
        live_q = ~zero_q
        assert np.all(gn[live_q] <= 1.001 * g_norm[live_q] + 0.25 + (1.001 * 0.25 + 3 * F32_EPS * gn[live_q]))
        assert np.all(Qn <= 1.0001 * Q_norm * (1 + (dim / 64 + 8) * F32_EPS))      # integer squares: only the summation and the product round

        # ---- thresholds, for every k and under the payload filter: a masked or deleted row must never raise tau_q
        for filters, ok in ((None, alive), ([(0, 1)], alive & (codes == 1)), ([(0, 2)], alive & (codes == 2))):
            admissible = np.sort(canon[:, ok], axis=1)[:, ::-1]
            for k in ic.KS:
                t = ffi.debug_i8_intervals(idx._handle(), n, dim, q, k, filters)
                assert np.array_equal(t["hi"], hi) and np.array_equal(t["lo"], lo)       # (intervals do not depend on k or the mask)
                tau = t["tau"].astype(np.float64)
                if admissible.shape[1] < k:
                    assert np.all(np.isneginf(tau)), f"k={k} filter {filters}: fewer than k admissible rows, yet tau = {tau}"
                else:
                    kth = admissible[:, k - 1]
                    assert np.all(tau <= kth), f"k={k} filter {filters}: tau above the k-th score for queries {np.flatnonzero(tau > kth)}: {tau[tau > kth]} > {kth[tau > kth]}"

        gq = [i for i, name in enumerate(qkinds) if name == "gaussian"]
        rows = kind == 0
        print(f"\n{case.id}: dn {dn:.4f} (largest |d|_2 {d_ever:.4f}); half-width median {np.median(hw):.3e}, Gaussian rows x Gaussian queries "
              f"{np.median(hw[gq][:, rows]) if gq else float('nan'):.3e}; tightest slack lo {np.min(canon - lo):.3e} hi {np.min(hi - canon):.3e}")
    finally:
        idx.close()


@pytest.mark.parametrize("dim", sorted(ic.scan_dims()))
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
def test_a_query_gets_the_same_interval_alone_and_in_a_full_batch(debug_library, dim, bf16):
    ffi = debug_library
    case = next(c for c in CASES if c.dim == dim and c.bf16 == bf16 and c.nq == 64 and c.corpus == "mixed")
    idx, raw, kind, stored, alive, codes, _ = _build(ffi, case)
    try:
        n = len(stored)
        q, qkinds = ic.queries_for(dim, 64, case.seed, raw, kind, stored)
        for j in range(len(ic.QUERY_KINDS)):                             # one query of every kind
            batch = q.copy()
            batch[0], batch[40] = q[j], q[j]
            alone = ffi.debug_i8_intervals(idx._handle(), n, dim, q[j:j + 1], 10)
            full = ffi.debug_i8_intervals(idx._handle(), n, dim, batch, 10)
            for slot in (0, 40):
                for name in ("hi", "lo", "hi_rec"):
                    assert np.array_equal(alone[name][0].view(np.uint32), full[name][slot].view(np.uint32)), (qkinds[j], slot, name)
                assert np.array_equal(alone["qpar"][0].view(np.uint32), full["qpar"][slot].view(np.uint32))
                assert alone["tau"][0].view(np.uint32) == full["tau"][slot].view(np.uint32)
    finally:
        idx.close()


def test_the_entry_refuses_what_it_cannot_hold(debug_library):
    ffi = debug_library
    idx = ffi.Index(384, ffi.DTYPE_BF16, capacity_rows=8193 * 32)
    try:
        with pytest.raises(ffi.NativeError) as e:                         # no rows
            ffi.debug_i8_intervals(idx._handle(), 1, 384, np.zeros((1, 384), np.float32), 10)
        assert e.value.code == ffi.E_INVALID
        idx.append(np.random.default_rng(0).standard_normal((8192 * 32 + 1, 384), dtype=np.float32))
        with pytest.raises(ffi.NativeError) as e:                         # 8193 tiles: one more than the record of upper ends holds
            ffi.debug_i8_intervals(idx._handle(), 8192 * 32 + 1, 384, np.zeros((1, 384), np.float32), 10)
        assert e.value.code == ffi.E_INVALID
        with pytest.raises(ffi.NativeError):                              # 65 queries
            ffi.debug_i8_intervals(idx._handle(), 8192 * 32 + 1, 384, np.zeros((65, 384), np.float32), 10)
    finally:
        idx.close()
