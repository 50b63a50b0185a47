"""Line spans on the device: ``crh_span_select`` against the CPU restatement (tests/span_cases.py), bit for bit -- positions,
rows, score bits, spans and ``out_info``; range conditions (``CRH_COND_BETWEEN`` / ``_NOT_BETWEEN``) through every entry point
that takes a ``crh_condition`` against the f32 oracle under the numpy mask; and the store end to end (``max_overlap``,
``chunks_at``, range deletes, format-5 and stripped format-4 snapshots) against the brute-force definition run with
``oracle.search`` on ``read_rows`` of the whole collection.  No tolerance appears anywhere.

The restatement's ``k``-output result is the prefix of its ``c``-output result (tests/test_spans_host.py pins that): the sweeps
run it once per list at ``k = c`` and compare every ``k`` of the device against that prefix."""
import asyncio
import json
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U32 = np.uint32
NAMES = ("pos", "rows", "scores", "file", "lo", "hi", "info")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(U32)


def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[0]), _bits(b[0]))


def _lists(nq, c, mode, seed):
    """nq candidate lists of c entries: scores descending with runs of equal values, distinct rows, padded tails of random
    length (every fifth list all padding when there are enough of them), (file, lo, hi) by ``mode``."""
    rng = np.random.default_rng(seed)
    scores = -np.sort(-np.round(rng.standard_normal((nq, c)), 1).astype(np.float32), axis=1)
    rows = (rng.permuted(np.tile(np.arange(4 * c, dtype=np.int64), (nq, 1)), axis=1)[:, :c] + (rng.integers(0, 3, (nq, 1)) << 32)) if nq else np.zeros((0, c), np.int64)
    real = rng.integers(0, c + 1, nq)
    real[::3] = c                                                     # (full lists too)
    if nq >= 5:
        real[4::5] = 0
    pad = np.arange(c)[None, :] >= real[:, None]
    if mode == "padding":
        pad[:] = True
    if mode == "one":                                                 # all one file with one span: the first real candidate alone survives
        files, lo, hi = np.full((nq, c), 3, np.int32), np.full((nq, c), 10, np.int32), np.full((nq, c), 30, np.int32)
    elif mode == "disjoint":                                          # c pairwise disjoint spans of one file: the longest kept list
        files = np.full((nq, c), 0, np.int32)
        lo = (rng.permuted(np.tile(np.arange(c, dtype=np.int32), (nq, 1)), axis=1) * 10) if nq else np.zeros((0, c), np.int32)
        hi = lo + rng.integers(0, 10, (nq, c)).astype(np.int32)
    else:                                                             # nested, overlapping, touching and broken spans of a few files
        files = rng.integers(-1, 24, (nq, c)).astype(np.int32)
        lo = rng.integers(0, 400, (nq, c)).astype(np.int32)
        hi = lo + (rng.geometric(0.04, (nq, c)) - 1).astype(np.int32)
        lo[rng.random((nq, c)) < 0.03] = -1                           # no start line
        broken = rng.random((nq, c)) < 0.03
        hi[broken] = lo[broken] - 1 - rng.integers(0, 3, int(broken.sum()))   # hi < lo (also -1: end line absent)
        big = rng.random((nq, c)) < 0.02
        lo[big], hi[big] = 0, 2 ** 31 - 1                             # the longest span an int32 column can hold
    scores[pad], rows[pad] = -np.inf, -1
    files[pad], lo[pad], hi[pad] = (rng.integers(-1, 5, int(pad.sum())).astype(np.int32) for _ in range(3))   # (whatever a gather left there)
    return scores, rows, files, lo, hi


def _device_select(torch, ffi, ins, nq, c, k, permille):
    """``crh_span_select`` into outputs pre-filled with garbage (every slot must be written)."""
    L = ffi.lib()
    dev = "cuda:0"
    tens = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in ins]
    outs = [torch.full((nq, k), -77, dtype=t, device=dev) for t in (torch.int32, torch.int64, torch.float32, torch.int32, torch.int32, torch.int32)]
    info = torch.full((nq, 2), -77, dtype=torch.int32, device=dev)
    rc = L.crh_span_select(nq, c, k, permille, *(int(t.data_ptr()) if nq else None for t in tens), *(int(o.data_ptr()) if nq else None for o in outs),
                           int(info.data_ptr()) if nq else None, None)
    assert rc == ffi.OK, L.crh_last_error()
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs] + [info.cpu().numpy()]


def _assert_equal(got, want, k, what):
    for g, w, name in zip(got, want, NAMES):
        w = w if name == "info" else w[:, :k]
        if name == "scores":
            assert np.array_equal(_bits(g), _bits(w)), f"{what}: score bits differ"
        else:
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f"{what}: {name} differ\n{g}\n{w}"


# ------------------------------------------------------------------ crh_span_select against the restatement
@pytest.mark.parametrize("c", [1, 40, 64, 65, 1024])
def test_span_select_equals_the_restatement(gpu, c):
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from tests import span_cases
    for nq in (0, 1, 64):
        for mode in ("mixed", "one", "disjoint", "padding"):
            if mode != "mixed" and nq == 64:
                continue
            ins = _lists(nq, c, mode, seed=c * 1000 + nq)
            for permille in (0, 500, 1000):
                want = span_cases.span_select(*ins, c, permille)
                for k in sorted({1, c}):
                    got = _device_select(torch, ffi, ins, nq, c, k, permille)
                    _assert_equal(got, want, k, f"c={c} nq={nq} {mode} permille={permille} k={k}")
                real = ins[1] >= 0
                if nq and permille == 1000:                              # the candidates unchanged
                    assert np.array_equal(got[1], np.where(real, ins[1], -1)) and np.array_equal(got[6][:, 0], real.sum(1))
                if nq and mode == "one":
                    assert np.array_equal(got[6][:, 0], np.minimum(real.sum(1), 1) if permille < 1000 else real.sum(1))
                if nq and mode == "disjoint":
                    assert np.array_equal(got[6][:, 0], real.sum(1))     # nothing overlaps: every real candidate is kept
                if mode == "padding":
                    assert (got[0] == -1).all() and (got[6] == 0).all()


def test_span_select_through_the_binding_and_its_argument_checks(gpu):
    """``ffi.span_select`` returns what the raw call writes; nq = 3 inside buffers sized for 5 leaves the neighbours alone;
    refused arguments launch nothing."""
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from tests import span_cases
    L = ffi.lib()
    c, k = 100, 12
    ins = _lists(3, c, "mixed", seed=5)
    want = span_cases.span_select(*ins, k, 300)
    dev = "cuda:0"
    tens = [torch.from_numpy(a).to(dev) for a in ins]
    got = ffi.span_select(*tens, k, 300)
    torch.cuda.synchronize()
    _assert_equal([g.cpu().numpy() for g in got], want, k, "binding")
    outs = [torch.full((5, k), -77, dtype=t, device=dev) for t in (torch.int32, torch.int64, torch.float32, torch.int32, torch.int32, torch.int32)]
    info = torch.full((5, 2), -77, dtype=torch.int32, device=dev)
    ptr = [int(o[1:4].data_ptr()) for o in outs] + [int(info[1:4].data_ptr())]
    assert L.crh_span_select(3, c, k, 300, *(int(t.data_ptr()) for t in tens), *ptr, None) == ffi.OK
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in outs] + [info.cpu().numpy()]
    _assert_equal([h[1:4] for h in host], want, k, "inside larger buffers")
    assert all((h[0] == -77).all() and (h[4] == -77).all() for h in host)
    for bad in ((3, c, 0, 300), (3, c, c + 1, 300), (3, c, k, -1), (3, c, k, 1001), (-1, c, k, 300)):
        assert L.crh_span_select(*bad, *(int(t.data_ptr()) for t in tens), *ptr, None) == ffi.E_INVALID
    with pytest.raises(ffi.NativeError, match="int32"):
        ffi.span_select(tens[0], tens[1], tens[2].long(), tens[3], tens[4], k, 300)
    with pytest.raises(ffi.NativeError, match="shape"):
        ffi.span_select(tens[0], tens[1], tens[2], tens[3][:, :7].contiguous(), tens[4], 4, 300)
    torch.cuda.synchronize()
    assert all((o[0].cpu().numpy() == -77).all() for o in outs)


# ------------------------------------------------------------------ range conditions
ROWS = 2085                       # crosses the 32-row tile, the 64-lane wave and the 256-thread block edges
VMAX = 2 ** 31 - 1


def _range_corpus(dim, seed=1):
    """2085 rows; columns: two dictionary columns (0..3 and -1..2), the row number, and a value in 0..499 that a tenth of the
    rows lack (-1)."""
    rng = np.random.default_rng(seed + dim)
    x = rng.standard_normal((ROWS, dim)).astype(np.float32)
    val = rng.integers(0, 500, ROWS)
    val[rng.random(ROWS) < 0.1] = -1
    codes = np.stack([rng.integers(0, 4, ROWS), rng.integers(-1, 3, ROWS), np.arange(ROWS), val], axis=1).astype(np.int32)
    return rng, x, codes


RANGE_CASES = [
    [(2, 100, 1500, "between")], [(2, 100, 1500, "not_between")],
    [(3, 50, 120, "between")], [(3, 50, 120, "not_between")],                   # rows without the value: out of / inside
    [(3, 0, VMAX, "between")], [(3, 0, VMAX, "not_between")],                   # open at both ends: every row that has the value / none of them
    [(3, 300, VMAX, "between")], [(3, 0, 17, "between")], [(3, -5, 17, "between")],    # open above / below
    [(2, 700, 699, "between")], [(2, 700, 699, "not_between")],                 # lo > hi: empty
    [(3, 77, 77, "between")], [(2, 31, 32, "between")], [(2, 2084, 2084, "between")], [(2, 2085, 4000, "between")],
    [(2, 64, 1999, "between"), (0, [1, 3], False)], [(3, 100, 400, "not_between"), (1, [0], True), (0, 2)],
    [(2, 0, 1000, "between"), (3, 200, 300, "between"), (2, 500, 600, "not_between")],
]


@pytest.mark.parametrize("dtype_name", ["bf16", "f32"])
def test_range_conditions_equal_the_oracle_under_the_numpy_mask(gpu, dtype_name):
    """search_cond, match_rows_cond / count and -- after tombstone and compact -- the same ranges again."""
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from oracle import search as orc
    from tests import span_cases
    bf16 = dtype_name == "bf16"
    dim, nq, k = 384, 70, 40                                      # 70 queries: more than one 64-query batch
    rng, x, codes = _range_corpus(dim)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    idx = ffi.Index(dim, ffi.DTYPE_BF16 if bf16 else ffi.DTYPE_F32, capacity_rows=ROWS + 64, n_code_cols=4)
    idx.append(x[:1000], codes[:1000])
    idx.append(x[1000:], codes[1000:])
    xpre, qpre = orc.preprocess(x, to_bf16=bf16), orc.preprocess(q, to_bf16=bf16)
    alive = np.ones(ROWS, bool)

    def check(xp, cd, al, tag):
        unfiltered = idx.search(q, k)
        for conds in RANGE_CASES:
            got = idx.search(q, k, filters=conds)
            m = span_cases.np_mask(cd, al, conds)
            assert _same(got, orc.search(xp, qpre, k, alive=m.astype(np.uint8))), (tag, conds)
            want_rows = np.flatnonzero(m)
            assert idx.count_matching(conds) == len(want_rows), (tag, conds)
            assert np.array_equal(idx.match_rows(conds, limit=len(al)), want_rows) and np.array_equal(idx.match_rows(conds, limit=17), want_rows[:17])
            if conds in ([(2, 700, 699, "between")], [(2, 2085, 4000, "between")]):
                assert (got[1] == -1).all() and np.isneginf(got[0]).all()
            if conds == [(2, 700, 699, "not_between")]:
                assert _same(got, unfiltered)
        return {json.dumps(c): idx.search(q[:8], k, filters=c) for c in RANGE_CASES}

    check(xpre, codes, alive, "fresh")
    dead = np.sort(rng.choice(ROWS, ROWS // 3, replace=False))
    idx.tombstone(dead)
    alive[dead] = False
    before = check(xpre, codes, alive, "tombstoned")
    o2n = idx.compact()
    keep = np.flatnonzero(alive)
    assert np.array_equal(o2n[keep], np.arange(len(keep)))
    after = check(xpre[keep], codes[keep], np.ones(len(keep), bool), "compacted")
    for key, (s, r) in before.items():                            # the same range answers the same points (column 2 names them)
        s2, r2 = after[key]
        assert np.array_equal(_bits(s), _bits(s2)) and np.array_equal(np.where(r >= 0, codes[np.clip(r, 0, None), 2], -1),
                                                                         np.where(r2 >= 0, codes[keep][np.clip(r2, 0, None), 2], -1)), key
    idx.close()


def test_range_argument_checks_sparse_route_multi_counts_and_delete(gpu):
    import ctypes as C
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from oracle import search as orc
    from tests import range_cases, span_cases
    dim, k = 384, 40
    rng, x, codes = _range_corpus(dim, seed=2)
    q = rng.standard_normal((64, dim)).astype(np.float32)
    idx = ffi.Index(dim, ffi.DTYPE_BF16, capacity_rows=ROWS + 64, n_code_cols=4)
    idx.append(x, codes)
    xpre, qpre = orc.preprocess(x, to_bf16=True), orc.preprocess(q, to_bf16=True)
    alive = np.ones(ROWS, bool)
    L = ffi.lib()
    # mode 2 / 3 take exactly two bounds; every other non-zero mode is "not in"
    bounds = np.asarray([5, 9, 11], np.int32)
    n = C.c_int64(0)
    for mode in (ffi.COND_BETWEEN, ffi.COND_NOT_BETWEEN):
        for cnt in (0, 1, 3):
            cond = (ffi.Condition * 1)()
            cond[0].col, cond[0].negate, cond[0].n, cond[0].codes = 2, mode, cnt, bounds.ctypes.data
            assert L.crh_index_match_rows_cond(idx._handle(), cond, 1, 1 << 40, None, C.byref(n)) == ffi.E_INVALID
            assert b"n = 2" in L.crh_last_error()
            assert L.crh_index_tombstone_cond(idx._handle(), cond, 1, C.byref(n)) == ffi.E_INVALID
    assert idx.count() == (ROWS, ROWS)
    cond = (ffi.Condition * 1)()
    cond[0].col, cond[0].negate, cond[0].n, cond[0].codes = 2, 7, 2, bounds.ctypes.data
    assert L.crh_index_match_rows_cond(idx._handle(), cond, 1, 1 << 40, None, C.byref(n)) == ffi.OK and n.value == ROWS - 2    # not in {5, 9}

    # a range leaving 4 of the 66 tiles takes the sparse route; the dense route gives the same bits
    conds = [(2, 1000, 1100, "between")]
    m = span_cases.np_mask(codes, alive, conds)
    idx.set_sparse_route(True)
    got = idx.search(q, k, filters=conds)
    st = idx.stats()
    print("sparse route under a range:", st)
    assert st["batches"] == 1 and 0 < st["tiles"] <= 4 and st["rows"] <= 4 * 32
    idx.set_sparse_route(False)
    dense = idx.search(q, k, filters=conds)
    assert idx.stats()["tiles"] >= 66
    idx.set_sparse_route(True)
    assert _same(got, dense) and _same(got, orc.search(xpre, qpre, k, alive=m.astype(np.uint8)))

    # three classes of different ranges in one pass == every query searched alone
    classes = [[(2, 100, 900, "between")], [(3, 100, 300, "not_between"), (0, [0, 1], False)], [(2, 1500, 2084, "between"), (3, 0, 250, "between")]]
    qclass = np.arange(64) % 3
    ms, mr = idx.search_multi(q, k, classes, qclass)
    for i in range(64):
        s1, r1 = idx.search(q[i:i + 1], k, filters=classes[qclass[i]])
        assert np.array_equal(mr[i], r1[0]) and np.array_equal(_bits(ms[i]), _bits(s1[0])), i
    for cl in range(3):
        mm = span_cases.np_mask(codes, alive, classes[cl])
        es, er = orc.search(xpre, qpre[qclass == cl], k, alive=mm.astype(np.uint8))
        assert _same((ms[qclass == cl], mr[qclass == cl]), (es, er)), cl

    # in-range counts under a range condition
    conds = [(3, 100, 400, "between"), (1, [2], True)]
    m = span_cases.np_mask(codes, alive, conds)
    all_scores = orc.scores(xpre, qpre)
    thr = np.where(np.arange(64) % 2 == 0, np.float32(0.0), np.sort(all_scores[:, m], axis=1)[:, -5]).astype(np.float32)
    want = range_cases.select(all_scores, thr, k, m)
    rs, rr, rc = idx.search_range(q, k, thr, filters=conds)
    assert np.array_equal(rc, want[2]) and _same((rs, rr), want[:2]) and rc.max() > k and rc.min() == 5

    # delete by range: the returned count and the survivors equal numpy; deleting again finds nothing
    idx.tombstone(np.arange(0, ROWS, 9))
    alive[::9] = False
    conds = [(2, 300, 1200, "between"), (3, 0, 99, "not_between")]
    want = span_cases.np_mask(codes, alive, conds)
    calls = ffi.Index.device_calls
    assert idx.tombstone_filter(conds) == int(want.sum()) and ffi.Index.device_calls == calls + 1
    alive &= ~want
    assert idx.count()[1] == int(alive.sum()) and np.array_equal(idx.match_rows(None, limit=ROWS), np.flatnonzero(alive))
    assert idx.tombstone_filter(conds) == 0
    idx.close()


def test_range_under_the_int8_nomination_equals_the_three_launch_form_at_1m_rows(gpu):
    """1.1M rows x 768 (the size from which the library nominates from its int8 copy by itself), one range on the row-number
    column ANDed with a set: ids and score bits of the int8 nomination equal those of the three-launch bf16 form."""
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    n, dim, k, block = 1_100_000, 768, 100, 100_000
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(31)
    idx = ffi.Index(dim, ffi.DTYPE_BF16, capacity_rows=n, n_code_cols=2)
    for r0 in range(0, n, block):
        xb = torch.randn((block, dim), generator=gen, device=dev, dtype=torch.float32)
        rown = torch.arange(r0, r0 + block, device=dev, dtype=torch.int64)
        idx.append(xb, torch.stack([(rown % 7).to(torch.int32), rown.to(torch.int32)], dim=1).contiguous())
        torch.cuda.synchronize()
        del xb
    q = np.random.default_rng(32).standard_normal((64, dim)).astype(np.float32)
    conds = [(1, 123_457, 987_654, "between"), (0, [1, 2, 5], False)]
    assert idx.nomination() == ffi.NOMINATE_INT8
    s8, r8 = idx.search(q, k, filters=conds)
    assert idx.stats()["fallback_used"] & 6 == 0
    idx.set_nomination(ffi.NOMINATE_BF16_3)
    assert idx.nomination() == ffi.NOMINATE_BF16_3
    s3, r3 = idx.search(q, k, filters=conds)
    assert np.array_equal(r8, r3) and np.array_equal(_bits(s8), _bits(s3))
    assert (r8 >= 123_457).all() and (r8 <= 987_654).all() and np.isin(r8 % 7, [1, 2, 5]).all()
    assert np.all((s8[:, :-1] > s8[:, 1:]) | ((s8[:, :-1] == s8[:, 1:]) & (r8[:, :-1] < r8[:, 1:])))
    assert idx.count_matching(conds) == int(np.isin(np.arange(123_457, 987_655) % 7, [1, 2, 5]).sum())
    idx.close()


# ------------------------------------------------------------------ end to end through the store
def _pairs(hits):
    return [(h["id"], np.float32(h["score"]).view(U32).item()) for h in hits]


async def _filled(s, ids, raw, payloads, shards):
    """The collection in four appends (the blocks go round the shards); returns the stored rows in slot order."""
    n = len(raw)
    await s.create_collections()
    step = (n + 3) // 4
    for a in range(0, n, step):
        await s.upsert("code_chunks", ids[a:a + step], raw[a:a + step], payloads[a:a + step])
    col = s._col("code_chunks")
    assert all(r > 0 for r in col.shards.rows)
    sh, lo = col.rows_of(np.arange(n))
    stored = {t: col.shards.index[t].read_rows(0, col.shards.rows[t]) for t in range(shards)}
    return col, np.stack([stored[int(sh[i])][int(lo[i])] for i in range(n)])


@pytest.mark.parametrize("shards", [1, 2])
@pytest.mark.parametrize("dtype_name", ["bf16", "f32"])
def test_store_max_overlap_equals_the_brute_force(gpu, dtype_name, shards):
    """``search(max_overlap=...)`` on the corpus of nested, split and duplicated spans, and the rounds corpora: ids and score bits
    of the brute force over ``oracle.search`` on ``read_rows`` (ties to the lower global row), and the rounds each was built to need."""
    import coderag_amd  # noqa: F401
    from coderag_amd.store import HipVectorStore
    from oracle import search as orc
    from tests import span_cases
    from tests.test_spans_host import _brute_pairs, _ids
    bf16 = dtype_name == "bf16"

    async def run():
        raw, files, lo, hi, hot = span_cases.spans_corpus(dim=384)
        n = len(raw)
        ids = _ids(n)
        rng = np.random.default_rng(8)
        lang = rng.integers(0, 3, n)
        async with HipVectorStore(dim=384, dtype=dtype_name, initial_capacity=4096, device=0, shards=shards, compact_dead_fraction=0.0) as s:
            col, stored = await _filled(s, ids, raw, span_cases.payloads(files, lo, hi, lang), shards)
            qs = np.concatenate([rng.standard_normal((2, 384)).astype(np.float32), raw[[hot]], raw[[int(np.flatnonzero(files == 7)[0])]]])
            qpre = orc.preprocess(qs, to_bf16=bf16)
            for limit, share in ((10, 0.0), (10, 0.5), (100, 0.2)):
                batch = await s.search_batch("code_chunks", qs, limit=limit, max_overlap=share)
                for qi in range(len(qs)):
                    assert _pairs(batch[qi]) == _brute_pairs(col, stored, qpre[qi], files, lo, hi, ids, limit, round(share * 1000)), (limit, share, qi)
            got = await s.search("code_chunks", qs[0].tolist(), limit=12, max_overlap=0.25, filters={"start_line": {"gte": 5, "lte": 200}, "language": ["python", "rust"]},
                                 must_not={"end_line": {"gt": 400}})
            passing = (lo >= 5) & (lo <= 200) & (lang != 1) & ~((hi >= 0) & (hi > 400))
            assert _pairs(got) == _brute_pairs(col, stored, qpre[0], files, lo, hi, ids, 12, 250, passing) and len(got) == 12
            plain = await s.search("code_chunks", qs[1].tolist(), limit=10)
            assert _pairs(await s.search("code_chunks", qs[1].tolist(), limit=10, max_overlap=1.0)) == _pairs(plain)
            print(f"spans corpus {dtype_name} shards={shards}: rounds {col.span_rounds}")
        for kind, limit, want in (("round2", 10, {"queries": 1, "round2": 1, "short": 0}), ("short", 5, {"queries": 1, "round2": 1, "short": 1})):
            raw, files, lo, hi, q = span_cases.rounds_corpus(kind)
            ids = _ids(len(raw))
            async with HipVectorStore(dim=384, dtype=dtype_name, initial_capacity=4096, device=0, shards=shards, compact_dead_fraction=0.0) as s:
                col, stored = await _filled(s, ids, raw, span_cases.payloads(files, lo, hi), shards)
                qp = orc.preprocess(q[None], to_bf16=bf16)[0]
                got = await s.search("code_chunks", q.tolist(), limit=limit, max_overlap=0.5)
                assert col.span_rounds == want, (kind, col.span_rounds)
                assert _pairs(got) == _brute_pairs(col, stored, qp, files, lo, hi, ids, limit, 500), kind
                assert len(got) == (1 if kind == "short" else limit)
                assert _pairs(got) == _brute_pairs(col, stored, qp, files, lo, hi, ids, limit, 500, depth=None)[:len(got)]

    asyncio.run(run())


@pytest.mark.parametrize("shards", [1, 2])
def test_store_ranges_chunks_at_delete_and_both_snapshot_formats(gpu, tmp_path, shards):
    """Range filters and ``chunks_at`` against the payloads, a range delete, then save -> load and the same directory stripped
    back to format 4 (``codes.i32`` cut to its first ``len(keys)`` columns): both answer a range search, ``chunks_at`` and a
    ``max_overlap`` search with identical ids and score bits, and a save after the format-4 load writes format 5."""
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from coderag_amd.store import HipVectorStore
    from tests import span_cases
    from tests.test_spans_host import _ids
    raw, files, lo, hi, hot = span_cases.spans_corpus(dim=384, hot_copies=40)
    n = len(raw)
    ids = _ids(n)
    rng = np.random.default_rng(9)
    lang = rng.integers(0, 3, n)
    pay = span_cases.payloads(files, lo, hi, lang)
    pay[5]["start_line"], pay[6]["end_line"], pay[7]["start_line"] = "12", None, 2 ** 31      # values the device cannot hold: -1 there
    lo, hi = lo.copy(), hi.copy()
    lo[[5, 7]], hi[6] = -1, -1
    q = rng.standard_normal(384).astype(np.float32)
    snap, snap2 = str(tmp_path / "snap"), str(tmp_path / "snap2")
    kw = dict(dim=384, dtype="bf16", initial_capacity=4096, device=0, shards=shards, compact_dead_fraction=0.0)
    line = int(np.median(lo[(files == 3) & (lo >= 0)]))

    async def answers(s):
        return (_pairs(await s.search("code_chunks", q.tolist(), limit=20, filters={"start_line": {"gte": 30, "lte": 90}})),
                _pairs(await s.search("code_chunks", q.tolist(), limit=20, max_overlap=0.3)),
                await s.chunks_at("code_chunks", "/proj/f3.py", line, last_line=line + 10),
                _pairs(await s.search("code_chunks", q.tolist(), limit=20, must_not={"end_line": {"gte": 0}})),
                (await s.get_collection_info("code_chunks")).points_count)

    async def run():
        async with HipVectorStore(**kw) as s:
            col, _ = await _filled(s, ids, raw, pay, shards)
            everything = await s.search("code_chunks", q.tolist(), limit=1024)
            assert len(everything) == n

            def host(pred, limit):
                return [(h["id"], np.float32(h["score"]).view(U32).item()) for h in everything if pred(h["payload"])][:limit]
            num = lambda p, k: p.get(k) if type(p.get(k)) is int and p.get(k) < 2 ** 31 else None   # noqa: E731
            got = await s.search("code_chunks", q.tolist(), limit=25, filters={"start_line": {"gt": 99.5, "lt": 160.5}, "language": ["python", "go"]})
            assert _pairs(got) == host(lambda p: num(p, "start_line") is not None and 100 <= p["start_line"] <= 160 and p["language"] != "rust", 25) and got
            got = await s.search("code_chunks", q.tolist(), limit=25, must_not={"end_line": {"gte": 50}})
            assert _pairs(got) == host(lambda p: num(p, "end_line") is None or p["end_line"] < 50, 25)
            calls = ffi.Index.device_calls
            at = await s.chunks_at("code_chunks", "/proj/f3.py", line)
            assert ffi.Index.device_calls == calls + shards                      # ONE filter-only device call per shard
            assert at == [pay[i] for i in range(n) if files[i] == 3 and lo[i] >= 0 and hi[i] >= 0 and lo[i] <= line <= hi[i]] and len(at) >= 2
            calls = ffi.Index.device_calls
            await s.delete("code_chunks", {"file_path": "/proj/f9.py", "start_line": {"gte": int(lo[(files == 9) & (lo >= 0)].min()) + 1}})
            assert ffi.Index.device_calls == calls + shards
            gone = (files == 9) & (lo > lo[(files == 9) & (lo >= 0)].min())
            assert gone.sum() > 0 and (await s.get_collection_info("code_chunks")).points_count == n - int(gone.sum())
            want = await answers(s)
            assert all(w for w in want)
            await s.save(snap)
        meta = json.load(open(os.path.join(snap, "code_chunks", "collection.json")))
        assert meta["format"] == 5 and meta["numeric_keys"] == ["start_line", "end_line"]
        async with HipVectorStore(**kw) as s:
            await s.create_collections()
            await s.load(snap)
            assert await answers(s) == want
        shutil.copytree(snap, snap2)
        kept = span_cases.strip_to_format4(snap2)
        sub = os.path.join(snap2, "code_chunks", "shard0" if shards > 1 else "")
        im = json.load(open(os.path.join(sub, "index.json")))
        assert im["n_code_cols"] == kept == len(meta["keys"]) and os.path.getsize(os.path.join(sub, "codes.i32")) == kept * im["tiles"] * 128
        async with HipVectorStore(**kw) as s:
            await s.create_collections()
            await s.load(snap2)
            assert await answers(s) == want
            await s.save(snap2)
        assert json.load(open(os.path.join(snap2, "code_chunks", "collection.json")))["format"] == 5
        assert json.load(open(os.path.join(sub, "index.json")))["n_code_cols"] == kept + 2
        async with HipVectorStore(**kw) as s:
            await s.create_collections()
            await s.load(snap2)
            assert await answers(s) == want

    asyncio.run(run())


def test_smoke_passes_with_its_spans_line(gpu):
    import __graft_entry__ as entry
    line = entry._smoke_spans()
    assert line.startswith("spans:") and "bit-exact" in line
