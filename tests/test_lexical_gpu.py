"""Keyword search on the device: ``crh_lex_search`` / ``crh_lex_stats`` / ``crh_lex_append`` / ``crh_index_row_mask`` against the
CPU restatement (tests/lex_cases.py) -- rows, score BITS, counts and padding, into outputs pre-filled with garbage.  No
tolerance appears anywhere.  The corpora and their postings are built once per row count and shared."""
import functools

import numpy as np
import pytest

from tests import lex_cases as lc

pytestmark = pytest.mark.gpu

U32 = np.uint32
K1, B = 1.2, 0.75


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(U32)


@functools.lru_cache(maxsize=None)
def _corpus(n):
    off, terms, tf, dl = lc.corpus(n)
    return off, terms, tf, dl, lc._postings(terms)


_handles = {}


def _lex(ffi, n):
    """One device index per row count, appended in one call and kept for the module."""
    if n not in _handles:
        off, terms, tf, dl, _ = _corpus(n)
        lex = ffi.Lex(capacity_rows=n, device=0)
        lex.append(off, terms, tf, dl)
        assert lex.count() == (n, int(off[-1]))
        _handles[n] = lex
    return _handles[n]


def _queries(nq, seed, n):
    """nq queries of 0, 1, 7 and 32 terms in turn over the vocabulary, the everywhere-term and the nowhere-term; query 3 (when
    there is one) is the first 32 terms of row 100 -- the 40 identical rows 100..139 tie at its top."""
    words, every, nowhere = lc.vocabulary()
    rng = np.random.default_rng(seed)
    out = []
    for q in range(nq):
        nt = (0, 1, 7, 32)[q % 4]
        pick = set(int(w) for w in rng.choice(words, size=nt, replace=False)) if nt else set()
        if nt and q % 3 == 0:
            pick = set(list(pick)[: nt - 1]) | {int(every)}
        if nt > 1 and q % 5 == 0:
            pick = set(list(pick)[: nt - 1]) | {int(nowhere)}
        if nt == 1 and q % 8 == 5:
            pick = {int(nowhere)}
        out.append(np.asarray(sorted(pick), U32))
    if nq > 3 and n > 140:
        off, terms = _corpus(n)[:2]
        out[3] = terms[off[100]:off[101]][:32].copy()
    return out


def _weights(n, queries, mask=None):
    """Per query the idf of its terms, and avgdl, from the restatement's statistics over ``mask`` (None: every row)."""
    off, terms, tf, dl, _ = _corpus(n)
    ids = np.unique(np.concatenate([np.zeros(0, U32)] + list(queries)))
    df, rows, sum_dl = lc.stats(off, terms, dl, mask, ids)
    w, avgdl = lc.idf(df, rows, sum_dl)
    table = dict(zip(ids.tolist(), w))
    return [np.asarray([table[int(t)] for t in q], np.float32) for q in queries], avgdl


def _masks(n, kind):
    """(bool per row or None, device words or None)."""
    import torch
    if kind == "null":
        return None, None
    words = (n + 31) // 32
    rng = np.random.default_rng(11)
    if kind == "all":
        w = np.full(words, 0xFFFFFFFF, U32)
    elif kind == "clear":
        w = np.zeros(words, U32)
    elif kind == "alternating":
        w = np.where(np.arange(words) % 2 == 0, 0xFFFFFFFF, 0).astype(U32)
    else:                                                    # 5 % of the rows: most words hold a bit or two, some none
        w = lc.words_from_mask(rng.random(n) < 0.05)
    return lc.mask_from_words(w, n), torch.from_numpy(w.view(np.int32).copy()).to("cuda:0")


def _check(ffi, n, nq, k, mask_kind="null", row_base=0, seed=1):
    import torch
    off, terms, tf, dl, post = _corpus(n)
    queries = _queries(nq, seed, n)
    idf, avgdl = _weights(n, queries)
    mask, mask_dev = _masks(n, mask_kind)
    want = lc.bm25_search(off, terms, tf, dl, mask, queries, idf, K1, B, avgdl, k, row_base, postings=post)
    outs = (torch.full((nq, k), -77.0, dtype=torch.float32, device="cuda:0"), torch.full((nq, k), -77, dtype=torch.int64, device="cuda:0"),
            torch.full((nq,), -77, dtype=torch.int64, device="cuda:0"))
    got = _lex(ffi, n).search(queries, idf, k, K1, B, float(avgdl), mask=mask_dev, row_base=row_base,
                              out_scores=outs[0], out_rows=outs[1], out_count=outs[2])
    torch.cuda.synchronize()
    s, r, c = (g.cpu().numpy() for g in got)
    assert np.array_equal(c, want[2]), "counts differ"
    assert np.array_equal(r, want[1]), "rows differ"
    assert np.array_equal(_bits(s), _bits(want[0])), "score bits differ"
    assert np.isneginf(s[r < 0]).all() and (r[r >= 0] >= row_base).all()
    return want


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 2053, 20000])
def test_search_equals_the_restatement_at_every_row_count(gpu, n):
    from coderag_amd import ffi
    want = _check(ffi, n, nq=65, k=10)
    if n >= 2053:
        assert want[2].max() > 1024 and (want[2] == 0).any() and ((want[2] > 0) & (want[2] < 1024)).any()


@pytest.mark.parametrize("nq", [0, 1, 64, 65, 130])
def test_any_number_of_queries_in_passes_of_64(gpu, nq):
    from coderag_amd import ffi
    _check(ffi, 2053, nq=nq, k=10, mask_kind="alternating", seed=2)


@pytest.mark.parametrize("k", [1, 10, 1024])
def test_k_below_inside_and_above_the_qualifying_rows(gpu, k):
    from coderag_amd import ffi
    want = _check(ffi, 2053, nq=12, k=k, seed=3)
    if k == 10:                                            # query 3's cut at k lies inside the run of 40 equal scores
        assert want[0][3, 0] == want[0][3, 9] and list(want[1][3]) == list(range(100, 110))
    if k == 1024:
        assert ((want[2] > 0) & (want[2] < 1024)).any() and (want[2] > 1024).any() and (want[1][:, -1] == -1).any()


@pytest.mark.parametrize("n", [2053, 20000])
@pytest.mark.parametrize("mask_kind", ["null", "all", "clear", "alternating", "random"])
@pytest.mark.parametrize("row_base", [0, 3 << 32])
def test_masks_and_row_base(gpu, n, mask_kind, row_base):
    from coderag_amd import ffi
    want = _check(ffi, n, nq=9, k=10, mask_kind=mask_kind, row_base=row_base, seed=4)
    if mask_kind == "clear":
        assert (want[2] == 0).all() and (want[1] == -1).all()


@pytest.mark.parametrize("n", [33, 2053, 20000])
@pytest.mark.parametrize("mask_kind", ["null", "all", "clear", "alternating", "random"])
def test_stats_equal_the_restatement(gpu, n, mask_kind):
    import torch
    from coderag_amd import ffi
    off, terms, tf, dl, _ = _corpus(n)
    words, every, nowhere = lc.vocabulary()
    ids = np.concatenate([words[:40], [every, nowhere, words[3], every]]).astype(U32)     # (repeats are allowed)
    mask, mask_dev = _masks(n, mask_kind)
    df, rows, sum_dl = _lex(ffi, n).stats(ids, mask_dev)
    torch.cuda.synchronize()
    wdf, wrows, wsum = lc.stats(off, terms, dl, mask, ids)
    assert np.array_equal(df, wdf) and (rows, sum_dl) == (wrows, wsum)
    if mask_kind == "null":
        assert df[40] == np.count_nonzero(np.diff(off)) - 1 and df[41] == 0      # (row 10 holds one word 300 times and nothing else)


def _result(lex, queries, idf, avgdl, k=50):
    import torch
    got = lex.search(queries, idf, k, K1, B, float(avgdl))
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in got]


@pytest.mark.parametrize("piece", [1, 31, 1000])
def test_append_in_pieces_equals_one_append(gpu, piece):
    from coderag_amd import ffi
    n = 2053
    off, terms, tf, dl, _ = _corpus(n)
    queries = _queries(9, 5, n)
    idf, avgdl = _weights(n, queries)
    whole = _result(_lex(ffi, n), queries, idf, avgdl)
    lex = ffi.Lex(capacity_rows=0, device=0)               # (grows by doubling from nothing)
    for a in range(0, n, piece):
        b = min(n, a + piece)
        lex.append(off[a:b + 1] - off[a], terms[off[a]:off[b]], tf[off[a]:off[b]], dl[a:b])
    assert lex.count() == (n, int(off[-1]))
    parts = _result(lex, queries, idf, avgdl)
    lex.clear()
    assert lex.count() == (0, 0)
    lex.close()
    assert np.array_equal(parts[1], whole[1]) and np.array_equal(_bits(parts[0]), _bits(whole[0])) and np.array_equal(parts[2], whole[2])


def test_append_refusals_leave_the_index_unchanged(gpu):
    from coderag_amd import ffi
    n = 33
    off, terms, tf, dl, _ = _corpus(n)
    queries = _queries(5, 6, n)
    idf, avgdl = _weights(n, queries)
    lex = ffi.Lex(capacity_rows=64, device=0)
    lex.append(off, terms, tf, dl)
    before = _result(lex, queries, idf, avgdl, k=33)
    good = (np.asarray([0, 2, 2, 3], np.int64), np.asarray([5, 9, 7], U32), np.asarray([1, 2, 255], np.uint8), np.asarray([3, 0, 300], np.int32))
    bad = {
        "offsets start above 0": (np.asarray([1, 2, 2, 3], np.int64),) + good[1:],
        "offsets decrease": (np.asarray([0, 2, 1, 3], np.int64),) + good[1:],
        "ids equal": (good[0], np.asarray([5, 5, 7], U32)) + good[2:],
        "ids descend": (good[0], np.asarray([9, 5, 7], U32)) + good[2:],
        "tf 0": good[:2] + (np.asarray([1, 0, 255], np.uint8), good[3]),
        "dl below the sum of tf": good[:3] + (np.asarray([2, 0, 300], np.int32),),
    }
    L = ffi.lib()
    for name, (o, t, f, d) in bad.items():
        rc = L.crh_lex_append(lex._handle(), 3, o.ctypes.data, t.ctypes.data, f.ctypes.data, d.ctypes.data)
        assert rc == ffi.E_INVALID, name
        assert lex.count() == (n, int(off[-1])), name
    after = _result(lex, queries, idf, avgdl, k=33)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(before, after))
    lex.append(*good)                                      # the accepted form of the same rows: an empty row in the middle
    assert lex.count() == (n + 3, int(off[-1]) + 3)
    s, r, c = _result(lex, [np.asarray([7], U32)], [np.asarray([1.0], np.float32)], 1.0, k=3)
    assert c[0] == 1 and r[0, 0] == n + 2 and r[0, 1] == -1
    lex.close()


def test_library_refuses_bad_queries_with_nothing_launched(gpu):
    import torch
    from coderag_amd import ffi
    lex = _lex(ffi, 33)
    outs = (torch.full((1, 4), -77.0, dtype=torch.float32, device="cuda:0"), torch.full((1, 4), -77, dtype=torch.int64, device="cuda:0"),
            torch.full((1,), -77, dtype=torch.int64, device="cuda:0"))
    L = ffi.lib()

    def call(terms, k):
        t, w = np.asarray(terms, U32), np.ones(len(terms), np.float32)
        o = np.asarray([0, len(terms)], np.int64)
        return L.crh_lex_search(lex._handle(), 1, o.ctypes.data, t.ctypes.data, w.ctypes.data, K1, B, 10.0, k, None, 0,
                                outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), 0)
    assert call(list(range(33)), 4) == ffi.E_INVALID       # more than 32 terms
    assert call([3, 2], 4) == ffi.E_INVALID and call([3, 3], 4) == ffi.E_INVALID
    assert call([1, 2], 0) == ffi.E_INVALID and call([1, 2], ffi.MAX_K + 1) == ffi.E_INVALID
    torch.cuda.synchronize()
    assert (outs[1].cpu().numpy() == -77).all() and (outs[2].cpu().numpy() == -77).all()
    assert call(list(range(32)), 4) == ffi.OK


def test_row_mask_equals_the_numpy_mask(gpu):
    import torch
    from coderag_amd import ffi
    from tests import span_cases
    n = 2053
    rng = np.random.default_rng(8)
    codes = np.stack([rng.integers(0, 6, n), rng.integers(-1, 200, n), rng.integers(0, 3, n)], axis=1).astype(np.int32)
    idx = ffi.Index(384, ffi.DTYPE_BF16, capacity_rows=n, n_code_cols=3, device=0)
    idx.append(rng.standard_normal((n, 384), dtype=np.float32), codes)
    dead = rng.choice(n, 300, replace=False)
    idx.tombstone(dead)
    alive = np.ones(n, bool)
    alive[dead] = False
    for conds in ([], [(0, [1, 2, 4])], [(0, [3], True)], [(1, 20, 120, "between")], [(1, 50, 60, "not_between"), (2, 1)],
                  [(0, [1, 2, 4]), (0, [2], True), (1, 0, 150, "between")], [(0, [9])]):
        out = torch.full(((n + 31) // 32 + 3,), -77, dtype=torch.int32, device="cuda:0")
        idx.row_mask(conds, out=out)
        torch.cuda.synchronize()
        words = out.cpu().numpy().view(U32)
        assert (words[(n + 31) // 32:].view(np.int32) == -77).all()
        assert np.array_equal(lc.mask_from_words(words[: (n + 31) // 32], n), span_cases.np_mask(codes, alive, conds)), conds
    with pytest.raises(ffi.NativeError):
        idx.row_mask([], out=torch.zeros((3,), dtype=torch.int32, device="cuda:0"))
    idx.close()


# ------------------------------------------------------------------ the store end to end
STORE_N, STORE_DIM = 3000, 384
STORE_TEXTS = ["retry_after", "parse request header", "HTTPServerError MAX_BACKOFF_MS", lc.RARE, "no_such_identifier_anywhere", "",
               "flushPayloadHTTPServer encode_token"]


def _pairs(hits):
    return [(h["id"], int(np.float32(h["score"]).view(U32))) for h in hits]


def _hybrid_expected(col, qv, texts, limit, c, passes, ids_of):
    """``lex_cases.hybrid_expected`` on what the store holds: ``read_rows`` of every shard in global-row order, the texts of the
    stored payloads, the alive and filter masks; per query the expected hit fields."""
    from oracle import search as orc
    row_texts, alive, ok, grow, slots = lc.store_lists(col, passes)
    x = np.concatenate([col.shards.index[sh].read_rows(0, len(sl)) for sh, (sl, _) in sorted(lc.store_rows(col).items())])
    slot_of = dict(zip(grow, slots))
    want = lc.hybrid_expected(x, orc.preprocess(qv, to_bf16=True), row_texts, alive, ok, texts, limit, c, grow=grow)
    return [[(ids_of(slot_of[h[0]]),) + h[1:] for h in hits] for hits in want]


@pytest.mark.parametrize("shards", [1, 2])
def test_store_lexical_and_hybrid_end_to_end(gpu, tmp_path, shards):
    """~3000 synthetic code chunks through ``upsert``: ``search_lexical``, ``lexical_count`` and ``search_hybrid`` against the
    restatements run on the stored payloads and ``read_rows`` -- before and after deleting a file, after ``compact()`` and after
    ``save`` / ``load``; the chunk that alone holds a rare identifier is rank 1 lexically and inside the hybrid top-``limit``."""
    import asyncio
    import coderag_amd  # noqa: F401
    from coderag_amd.store import HipVectorStore
    pay = lc.chunks(STORE_N)
    rng = np.random.default_rng(9)
    raw = rng.standard_normal((STORE_N, STORE_DIM)).astype(np.float32)
    ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(STORE_N)]
    qv = (raw[[lc.RARE_AT, 3, 50]] + 0.7 * rng.standard_normal((3, STORE_DIM))).astype(np.float32)
    htexts = [lc.RARE, "retry_after MAX_BACKOFF_MS", "fetch shard cursor"]
    snap = str(tmp_path / "snap")
    kw = dict(dim=STORE_DIM, dtype="bf16", initial_capacity=4096, device=0, shards=shards, compact_dead_fraction=0.0)

    async def check(s, col, passes=None, filters=None, must_not=None):
        want, counts, _, _ = lc.store_expected(col, STORE_TEXTS, 25, passes)
        got = await s.search_lexical_batch("code_chunks", STORE_TEXTS, limit=25, filters=filters, must_not=must_not)
        assert [_pairs(g) for g in got] == want
        assert [await s.lexical_count("code_chunks", t, filters=filters, must_not=must_not) for t in STORE_TEXTS[:4]] == counts[:4]
        exp = _hybrid_expected(col, qv, htexts, 10, 40, passes, col.ids.get)
        hyb = await s.search_hybrid_batch("code_chunks", qv, htexts, limit=10, filters=filters, must_not=must_not)
        assert [[(h["id"], int(np.float32(h["score"]).view(U32)), h["cosine"], h["lexical_score"], h["matched"]) for h in one] for one in hyb] == exp
        return want, counts, hyb

    async def run():
        async with HipVectorStore(**kw) as s:
            await s.create_collections()
            for a in range(0, STORE_N, 750):                                 # (several appends: the blocks go round the shards)
                await s.upsert("code_chunks", ids[a:a + 750], raw[a:a + 750], pay[a:a + 750])
            col = s._col("code_chunks")
            assert col._lex == {} and all(r > 0 for r in col.shards.rows)
            want, counts, hyb = await check(s, col)
            assert want[3][0][0] == ids[lc.RARE_AT] and counts[3] == 1       # the rare identifier: one chunk, rank 1 lexically ...
            assert ids[lc.RARE_AT] in [h["id"] for h in hyb[0]]              # ... and inside the hybrid top-10
            assert counts[0] > 25 and want[0][0][1] == want[0][1][1] and counts[4] == 0 and counts[5] == 0
            await check(s, col, lambda p: p.get("language") == "go" and p.get("file_path") != "/proj/f5.py",
                        filters={"language": "go"}, must_not={"file_path": "/proj/f5.py"})
            await check(s, col, lambda p: 100 <= p.get("start_line", -1) <= 300, filters={"start_line": {"gte": 100, "lte": 300}})
            await s.delete("code_chunks", {"file_path": "/proj/f3.py"})
            w2, c2, _ = await check(s, col)
            assert c2[0] < counts[0]
            assert await s.compact("code_chunks") > 0 and col._lex == {}
            w3, c3, _ = await check(s, col)
            assert c3 == c2 and [[b for _, b in w] for w in w3] == [[b for _, b in w] for w in w2]
            await s.upsert("code_chunks", ids[:40], raw[:40], [dict(p, content=p["content"] + " zzfreshlyaddedzz") for p in pay[:40]])   # replaces 40 points
            w4, _, _ = await check(s, col)
            assert len(await s.search_lexical("code_chunks", "zzfreshlyaddedzz", limit=100)) == 40
            await s.save(snap)
        async with HipVectorStore(**kw) as s:
            await s.create_collections()
            await s.load(snap)
            col = s._col("code_chunks")
            w5, _, _ = await check(s, col)
            assert [[b for _, b in w] for w in w5] == [[b for _, b in w] for w in w4]

    asyncio.run(run())
