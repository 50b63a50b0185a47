"""Non-finite vectors on the real index and store (a NaN score is no score), on every nomination route.

Stored rows or queries that hold a NaN or an infinity (tests/nonfinite_cases.py: row 0, both sides of a tile edge, the last row, a
whole tile, single +-inf elements; bad queries at the edges of the MFMA column blocks) against the restated oracle -- ids, f32
score bits and padding, exactly.  tests/test_nonfinite_cases_host.py proves the cases themselves on the CPU."""
import asyncio
import tempfile

import numpy as np
import pytest

from oracle import search as orc
from tests import nonfinite_cases as nf

pytestmark = pytest.mark.gpu

ROUTES = ("int8", "fused", "three")
LISTS = [(10, False), (100, True), (1024, False)]            # (k, under the 40-row filter)


def _ffi():
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    return ffi


def _route(monkeypatch, route):
    """The switches of one nomination route, set BEFORE the index exists (crh_index_create reads them once): the int8 copy from 0
    rows (tests/conftest.py's default), the product's one-launch bf16 scan, the three-launch bf16 form."""
    if route == "int8":
        monkeypatch.setenv("CODERAG_HIP_I8_MIN_ROWS", "0")
    else:
        monkeypatch.delenv("CODERAG_HIP_I8_MIN_ROWS", raising=False)
    if route == "three":
        monkeypatch.setenv("CODERAG_HIP_FUSED_SCAN", "0")
    else:
        monkeypatch.delenv("CODERAG_HIP_FUSED_SCAN", raising=False)


def _index(ffi, kind, dim, bf16, route=None):
    raw, codes, _ = nf.corpus(kind, dim)
    idx = ffi.Index(dim, ffi.DTYPE_BF16 if bf16 else ffi.DTYPE_F32, capacity_rows=nf.N, n_code_cols=2)
    idx.append(raw[:1000], codes[:1000])
    idx.append(raw[1000:], codes[1000:])                   # the second append starts mid-tile
    if route is not None:
        want = {"int8": ffi.NOMINATE_INT8, "fused": ffi.NOMINATE_BF16, "three": ffi.NOMINATE_BF16_3}[route]
        assert idx.nomination() == want, (route, idx.nomination())
    return idx


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), (what, "ids", np.argwhere(np.asarray(got[1]) != np.asarray(want[1]))[:5].tolist())
    assert np.array_equal(np.asarray(got[0]).view(np.uint32), np.asarray(want[0]).view(np.uint32)), (what, "score bits")


@pytest.mark.parametrize("dim", [768, 384, 1536])
@pytest.mark.parametrize("bf16", [False, True])
def test_stored_rows_equal_the_oracles_preprocess(gpu, bf16, dim):
    """k_append on rows with a NaN or an infinity: NaN exactly where orc_preprocess_rows leaves one, every other element to the bit."""
    ffi = _ffi()
    idx = _index(ffi, "gauss", dim, bf16)
    got = idx.read_rows(0, nf.N)
    idx.close()
    want = nf.stored("gauss", dim, bf16)
    assert np.isnan(want).any(1).sum() == 43 and nf.same_stored(got, want)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("bf16", [False, True])
def test_every_nomination_route_equals_the_oracle(gpu, monkeypatch, route, bf16):
    """64 queries, five of them bad, against the Gaussian and the sunk corpus: k = 10, k = 100 under the 40-row filter (the sparse
    tile list and, with that route switched off, the dense scans under a mask), k = 1024 (beyond the int8 pass's k: the index takes
    its bf16 scan for that call).  The bad queries' lists are all padding; the finite ones' equal, bit for bit, those of the batch
    with zeros in the bad slots."""
    ffi = _ffi()
    _route(monkeypatch, route)
    for kind in ("gauss", "sunk"):
        idx = _index(ffi, kind, 768, bf16, route)
        q, qbad = nf.queries(kind)
        qz, _ = nf.queries(kind, 768, 64, False)
        for k, filtered in LISTS:
            want = nf.expected(kind, 768, bf16, 64, k, filtered)
            for sparse in ((True, False) if filtered else (True,)):
                idx.set_sparse_route(sparse)
                got = idx.search(q, k, filters=nf.FILTER if filtered else None)
                st = idx.stats()
                what = (route, kind, k, filtered, sparse, st)
                _same(got, want, what)
                assert nf.well_formed(*got) and st["fallback_used"] == 0, what
                if filtered:
                    assert (st["tiles"] <= 20) == sparse, what               # the 40 rows sit in 20 of the 129 tiles
            assert (got[1][qbad] == -1).all() and np.isneginf(got[0][qbad]).all()
            zs, zr = idx.search(qz, k, filters=nf.FILTER if filtered else None)
            _same((zs[~qbad], zr[~qbad]), (got[0][~qbad], got[1][~qbad]), (route, kind, k, "zeros in the bad slots"))
        assert idx.nomination() == {"int8": ffi.NOMINATE_INT8, "fused": ffi.NOMINATE_BF16, "three": ffi.NOMINATE_BF16_3}[route]
        idx.close()


@pytest.mark.parametrize("bf16", [False, True])
def test_all_routes_agree_bit_for_bit(gpu, monkeypatch, bf16):
    """One corpus, one batch: the int8 copy, the one-launch and the three-launch bf16 scans, the wide scan (the same 64 queries
    and one more) and the classed scans (every query under the same filter, named twice) return the same bytes."""
    ffi = _ffi()
    for kind in ("gauss", "sunk"):
        q, _ = nf.queries(kind)
        q65 = np.concatenate([q, q[5:6]])
        got = {}
        for route in ROUTES:
            _route(monkeypatch, route)
            idx = _index(ffi, kind, 768, bf16, route)
            got[route] = idx.search(q, 100)
            if route == "fused":
                idx.set_nomination(ffi.NOMINATE_BF16)
                ws, wr = idx.search(q65, 100)
                assert idx.stats()["batches"] == 1                                # ONE wide pass
                got["wide"] = (ws[:64], wr[:64])
                _same((ws[64:], wr[64:]), (ws[5:6], wr[5:6]), "the 65th query is the 6th")
                got["classed"] = idx.search_multi(q, 100, [None, [(0, [0, 1, 2], False)]], np.arange(64) % 2)      # (two filters that keep every row)
            idx.close()
        for name, g in got.items():
            _same(g, got["three"], (kind, name))
        _same(got["three"], nf.expected(kind, 768, bf16, 64, 100), kind)


@pytest.mark.parametrize("nq", [65, 200])
@pytest.mark.parametrize("bf16", [False, True])
def test_the_wide_scan_equals_the_oracle(gpu, bf16, nq):
    ffi = _ffi()
    idx = _index(ffi, "gauss", 768, bf16)
    idx.set_nomination(ffi.NOMINATE_BF16)                  # (with the int8 copy in play 65..128 queries are two passes over it)
    q, qbad = nf.queries("gauss", 768, nq)
    got = idx.search(q, 10)
    assert idx.stats()["batches"] == 1 and idx.stats()["fallback_used"] == 0
    idx.close()
    _same(got, nf.expected("gauss", 768, bf16, nq, 10), nq)
    assert qbad[[0, 31, 32, 63, 64, nq - 1]].all() and (got[1][qbad] == -1).all()


@pytest.mark.parametrize("bf16", [False, True])
def test_the_classed_scans_equal_the_oracle(gpu, bf16):
    """Per-query filters in one batch: every tile (one class keeps every row) and the union's tile list (both classes inside the
    40 rows of the selective filter)."""
    ffi = _ffi()
    for kind in ("gauss", "sunk"):
        idx = _index(ffi, kind, 768, bf16)
        raw, codes, _ = nf.corpus(kind)
        q, qbad = nf.queries(kind)
        qpre = orc.preprocess(q, to_bf16=bf16)
        for classes, sparse in (([None, nf.FILTER, [(0, 1)]], False), ([nf.FILTER, nf.FILTER + [(0, 1)]], True)):
            qclass = np.arange(64) % len(classes)
            got = idx.search_multi(q, 100, classes, qclass)
            st = idx.stats()
            assert (st["tiles"] <= 20) == sparse and st["fallback_used"] == 0, (kind, sparse, st)
            for c, filt in enumerate(classes):
                es, er = orc.search(nf.stored(kind, 768, bf16), qpre[qclass == c], 100, codes=codes, filters=filt)
                _same((got[0][qclass == c], got[1][qclass == c]), (es, er), (kind, sparse, c))
            assert (got[1][qbad] == -1).all() and nf.well_formed(*got)
        idx.close()


@pytest.mark.parametrize("route", ["int8", "fused"])
@pytest.mark.parametrize("dim,bf16", [(1536, True), (1536, False), (384, True), (384, False)])
def test_other_dimensions(gpu, monkeypatch, route, dim, bf16):
    """dim 1536 (one 32-query column block per pass: the bad queries at slots 31 and 32 end one pass and begin the next) and 384."""
    ffi = _ffi()
    _route(monkeypatch, route)
    idx = _index(ffi, "sunk", dim, bf16, route)
    q, qbad = nf.queries("sunk", dim)
    for k, filtered in LISTS[:2]:
        got = idx.search(q, k, filters=nf.FILTER if filtered else None)
        assert idx.stats()["fallback_used"] == 0
        _same(got, nf.expected("sunk", dim, bf16, 64, k, filtered), (route, dim, k))
    idx.close()


@pytest.mark.parametrize("bf16", [False, True])
def test_score_conditioned_counts_leave_the_bad_rows_out(gpu, bf16):
    """Threshold -1.0 keeps every finite score: the range count and the threshold facet equal live rows minus bad rows, a bad
    query counts 0; the count and the facet WITHOUT a query still see the bad rows."""
    ffi = _ffi()
    raw, codes, bad = nf.corpus("gauss")
    q, qbad = nf.queries("gauss")
    idx = _index(ffi, "gauss", 768, bf16)
    dead = np.concatenate([[0, 500, 7 * 32 + 3], np.arange(40, nf.N, 9)])
    idx.tombstone(dead)
    live = np.ones(nf.N, bool)
    live[dead] = False
    assert (live & bad).sum() > 30 and idx.count() == (nf.N, int(live.sum()))
    for filt, passing in ((None, np.ones(nf.N, bool)), (nf.FILTER, codes[:, 1] == 9)):
        ok = live & passing
        s, r, c = idx.search_range(q, 10, -1.0, filters=filt)
        assert np.array_equal(c, np.where(qbad, 0, int((ok & ~bad).sum()))), (filt, c)
        es, er = orc.search(nf.stored("gauss", 768, bf16), orc.preprocess(q, to_bf16=bf16), 10, alive=ok.astype(np.uint8))
        _same((s, r), (es, er), ("range list", filt))
        bins, info = (t.cpu().numpy() for t in idx.search_range_facet(q, -1.0, 0, 3, filters=filt))
        want = np.bincount(codes[ok & ~bad, 0], minlength=3)
        assert np.array_equal(bins, np.where(qbad[:, None], 0, want[None, :])), filt
        assert np.array_equal(info, np.stack([c, np.zeros_like(c), np.zeros_like(c)], 1)), filt
        bins, info = (t.cpu().numpy() for t in idx.facet(0, 3, filters=filt))
        assert np.array_equal(bins, np.bincount(codes[ok, 0], minlength=3)) and info.tolist() == [int(ok.sum()), 0, 0]
        assert idx.count_matching(filt) == int(ok.sum())
    idx.close()


@pytest.mark.parametrize("bf16", [False, True])
def test_tombstone_compact_save_and_load(gpu, monkeypatch, bf16):
    """The bad rows move (compaction) and restore (snapshot) with the same NaN positions; the lists before and after are equal
    through old_to_new; the requantised int8 copy still returns none of them."""
    ffi = _ffi()
    _route(monkeypatch, "int8")
    raw, codes, bad = nf.corpus("gauss")
    q, qbad = nf.queries("gauss")
    stored = nf.stored("gauss", 768, bf16)
    idx = _index(ffi, "gauss", 768, bf16, "int8")
    dead = np.unique(np.concatenate([[0, 31, 500, 7 * 32 + 3, 7 * 32 + 30], np.arange(17, nf.N, 11)]))
    idx.tombstone(dead)
    live = np.ones(nf.N, bool)
    live[dead] = False
    assert (live & bad).sum() > 30 and (~live & bad).sum() >= 5

    def lists(ix):
        return [ix.search(q, k, filters=nf.FILTER if filtered else None) for k, filtered in LISTS[:2]]
    before = lists(idx)
    for (k, filtered), got in zip(LISTS[:2], before):
        es, er = orc.search(stored, orc.preprocess(q, to_bf16=bf16), k, alive=live.astype(np.uint8), codes=codes, filters=nf.FILTER if filtered else None)
        _same(got, (es, er), ("tombstoned", k))
    with tempfile.TemporaryDirectory() as tmp:
        idx.save(tmp)
        fresh = ffi.Index(768, ffi.DTYPE_BF16 if bf16 else ffi.DTYPE_F32, capacity_rows=64, n_code_cols=2)
        fresh.load(tmp)
    assert fresh.count() == idx.count() and nf.same_stored(fresh.read_rows(0, nf.N), stored)
    assert fresh.nomination() == ffi.NOMINATE_INT8
    for a, b in zip(lists(fresh), before):
        _same(a, b, "restored")
    for ix in (idx, fresh):
        o2n = ix.compact()
        assert np.array_equal(o2n >= 0, live) and np.array_equal(o2n[live], np.arange(int(live.sum())))
        assert nf.same_stored(ix.read_rows(0, int(live.sum())), stored[live])
        assert ix.nomination() == ffi.NOMINATE_INT8
        for a, b in zip(lists(ix), before):
            _same(a, (b[0], np.where(b[1] >= 0, o2n[np.maximum(b[1], 0)], -1)), "compacted")
            assert ix.stats()["fallback_used"] == 0
        ix.close()


# ------------------------------------------------------------------ the store

@pytest.mark.parametrize("dtype,shards", [("bf16", 1), ("f32", 1), ("bf16", 2), ("f32", 2)])
def test_the_store_keeps_the_points_and_never_returns_them_as_vector_hits(gpu, monkeypatch, dtype, shards):
    """300 points and five non-finite ones (payloads copied from stored points: the dictionaries see no new value), one upsert.
    Every vector-scored read path returns exactly what the same store WITHOUT the five returns -- ids, score bits, counts --, and
    what the life-cycle model (tests/lifecycle_cases.py) answers; count, the filter-only fetch, text and keyword search still see
    them.  search_hybrid_batch is held to the model alone: its keyword leg sees the five points and BM25's N and average length
    count them, so its scores cannot be those of the store without them.  recommend with a bad positive: `average` has a NaN
    query and returns nothing; under `best` that positive scores nothing and the answer is that of the other positives alone."""
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi, shards as shards_mod
    from coderag_amd.ranking.device import DeviceReranker
    from coderag_amd.store import HipVectorStore
    from tests import lifecycle_cases as lc
    bf16 = dtype == "bf16"
    block = 32
    orig = shards_mod.ShardSet.__init__

    def small_blocks(self, *a, **kw):
        kw["block"] = block
        orig(self, *a, **kw)
    monkeypatch.setattr(shards_mod.ShardSet, "__init__", small_blocks)
    reranker = DeviceReranker(device=0)

    async def run():
        stores, models = [], []
        try:
            for with_bad in (True, False):
                s = HipVectorStore(dim=lc.DIM, dtype=dtype, initial_capacity=64, device=0, shards=shards)
                stores.append(s)
                await s.connect()
                await s.create_collections()
                m, sums = lc.Model(ns=shards, block=block), lc.Model(text_key="summary", ns=shards, block=block)
                pts, spts = nf.store_points(with_bad), lc.summary_points()
                await s.upsert(lc.CODE, *pts)
                await s.upsert(lc.SUMS, *spts)
                m.upsert(*pts)
                sums.upsert(*spts)
                models.append((m, sums))
            with_, without = stores
            assert all(ix.nomination() == ffi.NOMINATE_INT8 for ix in with_._col(lc.CODE).shards.index.values())
            # every read path of the store with the five points against the model that holds them too
            tally = []
            await lc.check_all(with_, models[0][0], models[0][1], lc.FULL, bf16, reranker, "five non-finite points", tally)
            assert len(tally) == lc.checks_in(lc.FULL) > 40
            # ... and against the store without them
            v = models[0][0].view(bf16)
            compared, seen = [], []
            for name, feature, _, got in lc.checks(v, models[0][1].view(bf16), reranker):
                if feature in nf.SCORED or name in nf.SCORED_NAMES:
                    a, b = await lc._value(got(with_)), await lc._value(got(without))
                    assert a == b, f"{name}\n  with:    {lc._short(a)}\n  without: {lc._short(b)}"
                    compared.append(name)
                elif name in nf.SEES_THEM:
                    a, b = await lc._value(got(with_)), await lc._value(got(without))
                    assert a != b, name
                    seen.append(name)
            assert len(compared) >= 25 and set(seen) == set(nf.SEES_THEM), (compared, seen)
            q0 = lc.Q[0].tolist()
            for kw in (dict(query_vector=q0, score_threshold=lc.THRESHOLD), dict(query_vector=q0, score_threshold=-1.0, filters=lc.F_EQ)):
                a, b = await with_.facet(lc.CODE, "file_path", 10, **kw), await without.facet(lc.CODE, "file_path", 10, **kw)
                assert a == b and a["total"] + a["missing"] > 0, (kw, a, b)
            assert await with_.count_similar(lc.CODE, q0, -1.0) == await without.count_similar(lc.CODE, q0, -1.0) == nf.STORE_POINTS
            plain = await with_.facet(lc.CODE, "file_path", 10)
            assert plain["total"] + plain["missing"] == nf.STORE_POINTS + 5 == (await with_.client.count(lc.CODE)).count
            ids = {h["id"] for h in await with_.search(lc.CODE, None, 1000)}
            assert set(nf.BAD_IDS) <= ids and len(ids) == nf.STORE_POINTS + 5
            text = await with_.search_text(lc.CODE, "def ", 1000)
            assert set(nf.BAD_IDS) <= {h["id"] for h in text["hits"]}
            name = lc.point(nf.BAD_PAYLOAD_OF[0])[2]["entity_name"]
            assert nf.BAD_IDS[0] in {h["id"] for h in await with_.search_lexical(lc.CODE, name, 1000)}
            # a bad query is similar to nothing
            nanq = nf.spoil(lc.Q[0], "nan_last").tolist()
            assert await with_.search(lc.CODE, nanq, 10) == [] and await with_.count_similar(lc.CODE, nanq, -1.0) == 0
            assert [len(h) for h in await with_.search_batch(lc.CODE, np.stack([lc.Q[0], nf.spoil(lc.Q[1], "plus_inf"), lc.Q[2]]), 5)] == [5, 0, 5]
            # recommend with one of the five among the positives
            pos, neg = [nf.BAD_IDS[0], lc.EXAMPLES[0][1]], lc.EXAMPLES[1]
            assert await with_.recommend(lc.CODE, pos, neg, 6, "average", None, lc.F_NOT) == []
            best = lc.got_hits(await with_.recommend(lc.CODE, pos, neg, 6, "best", None, lc.F_NOT), "negative_score", "matched_positive")
            alone = lc.got_hits(await without.recommend(lc.CODE, pos[1:], neg, 6, "best", None, lc.F_NOT), "negative_score", "matched_positive")
            assert len(best) == 6 and best == alone == lc._recommend(v, pos, neg, 6, "best", v.mask(None, lc.F_NOT, "recommend"))
        finally:
            for s in stores:
                await s.close()
    asyncio.run(run())
