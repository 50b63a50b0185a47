"""crh_search_range on the device against the CPU restatement (tests/range_cases.py): ids, f32 score bits and counts, all exact.
Every case mixes the issue's thresholds across the queries of its batch -- a stored row's exact score, one ulp above and below
it, above the maximum, -2.0, and the two duplicate-block thresholds that are the band's worst case -- and range_cases.batch
asserts on the oracle that counts of 0, below k, k, above k and above CRH_MAX_K all occur."""
import asyncio

import numpy as np
import pytest

from oracle import search as orc
from tests import range_cases

pytestmark = pytest.mark.gpu
U32, F32 = np.uint32, np.float32
K = 10


def _same(got, want, what=""):
    gs, gr, gc = got
    ws, wr, wc = want
    assert np.array_equal(np.asarray(gr), wr), f"{what}: rows differ"
    assert np.array_equal(np.ascontiguousarray(gs, dtype=F32).view(U32), ws.view(U32)), f"{what}: score bits differ"
    if wc is not None:
        assert np.array_equal(np.asarray(gc), wc), f"{what}: counts differ: {np.asarray(gc).tolist()} vs {wc.tolist()}"


def _index(ffi, raw, codes, dtype, dead=None):
    idx = ffi.Index(raw.shape[1], dtype, capacity_rows=len(raw), n_code_cols=codes.shape[1], device=0)
    idx.append(raw, codes)
    if dead is not None:
        idx.tombstone(dead)
    return idx


def _dead(n, block):
    """Tombstones: every 11th row, and three rows of the duplicate block."""
    return np.unique(np.concatenate([np.arange(5, n, 11), block[0] + np.asarray([0, 7, block[1] - 1])])).astype(np.int64)


# every dim x store at every row count; the three batch sizes rotate so that each meets each row count and each dim
SHAPES = [(dim, bf16, n, (1, 64, 65)[(i + j + int(bf16)) % 3])
          for i, dim in enumerate((384, 768, 1536)) for bf16 in (True, False) for j, n in enumerate((33, 3000, 40000))]


@pytest.mark.parametrize("dim,bf16,n,nq", SHAPES)
def test_lists_and_counts_equal_the_restatement(gpu, dim, bf16, n, nq):
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    raw, codes, block = range_cases.corpus(n, dim)
    dead = _dead(n, block)
    alive = np.ones((n,), bool)
    alive[dead] = False
    q, thr, scores, _, want = range_cases.batch(raw, block, nq, K, bf16, alive, seed=dim + n)
    idx = _index(ffi, raw, codes, ffi.DTYPE_BF16 if bf16 else ffi.DTYPE_F32, dead)
    try:
        got = idx.search_range(q, K, thr)
        st = idx.stats()
        print(f"dim {dim} bf16 {bf16} n {n} nq {nq}: counts {sorted(set(want[2].tolist()))[:6]}.. max {want[2].max()} cands {st['candidates']} "
              f"max/query {st['max_query_cands']} fallback {st['fallback_used']} seed {st['seed_tiles']}")
        _same(got, want, "count mode")
        assert st["seed_tiles"] == 0 and st["batches"] == (nq + idx_batch(dim) - 1) // idx_batch(dim)      # no sample: tau is the band's lower edge
        # list-only mode on the same inputs: the same lists, no counts, thresholds seeded as for a plain search
        ls, lr, lc = idx.search_range(q, K, thr, counts=False)
        assert lc is None
        _same((ls, lr, None), (want[0], want[1], None), "list only")
        assert idx.stats()["seed_tiles"] > 0
        # a scalar threshold stands for every query
        _same(idx.search_range(q, K, float(thr[0])), range_cases.select(scores, thr[0], K, alive), "scalar")
    finally:
        idx.close()


def idx_batch(dim):
    return 32 if dim > 1024 else 64


@pytest.fixture(scope="module")
def mid():
    """One 3 000-row corpus at dim 768 and its oracle scores for 65 queries, shared by the path tests below (read only)."""
    n, dim, nq = 3000, 768, 65
    raw, codes, block = range_cases.corpus(n, dim, seed=3)
    codes = codes.copy()
    codes[700:740, 0] = 99                                   # a value only 40 consecutive rows carry: 2-3 of the 94 tiles
    dead = _dead(n, block)
    alive = np.ones((n,), bool)
    alive[dead] = False
    out = {"raw": raw, "codes": codes, "block": block, "dead": dead, "alive": alive, "n": n, "nq": nq}
    for bf16 in (True, False):
        q, thr, scores, _, want = range_cases.batch(raw, block, nq, K, bf16, alive, seed=5)
        out[bf16] = {"q": q, "thr": thr, "scores": scores, "want": want}
    return out


@pytest.mark.parametrize("bf16", [True, False])
def test_filters_sparse_route_and_regrowth(gpu, mid, bf16):
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    c, codes, alive = mid[bf16], mid["codes"], mid["alive"]
    idx = _index(ffi, mid["raw"], codes, ffi.DTYPE_BF16 if bf16 else ffi.DTYPE_F32, mid["dead"])
    try:
        # any-of + exclusion: thresholds made for the unfiltered corpus still mix empty, short and long answers
        conds = [(0, [1, 3, 4]), (1, [2], True)]
        m = alive & np.isin(codes[:, 0], [1, 3, 4]) & ~np.isin(codes[:, 1], [2])
        want = range_cases.select(c["scores"], c["thr"], K, m)
        assert {"zero", "short", "more"} <= range_cases.kinds_of(want[2], K)
        _same(idx.search_range(c["q"], K, c["thr"], filters=conds), want, "set conditions")
        _same(idx.search_range(c["q"], K, c["thr"], filters=conds, counts=False)[:2] + (None,), want[:2] + (None,), "set conditions, list only")
        # a filter sparse enough for the tile-list route (k_scan_list), both modes; stats() says the list was walked
        m = alive & (codes[:, 0] == 99)
        ntiles, listed = (mid["n"] + 31) // 32, len(np.unique(np.flatnonzero(m) // 32))
        thr = np.where(np.arange(mid["nq"]) % 2 == 0, np.float32(-2.0), c["thr"]).astype(F32)
        want = range_cases.select(c["scores"], thr, K, m)
        assert want[2].max() == m.sum() > K and want[2].min() == 0 and listed * 4 <= ntiles
        idx.set_sparse_route(True)
        for counts in (True, False):
            got = idx.search_range(c["q"], K, thr, filters=[(0, 99)], counts=counts)
            st = idx.stats()
            assert st["tiles"] == listed * st["batches"] and st["rows"] <= 32 * listed * st["batches"], st
            _same(got[:2] + (got[2] if counts else None,), want[:2] + (want[2] if counts else None,), f"list route counts={counts}")
        idx.set_sparse_route(False)
        got = idx.search_range(c["q"], K, thr, filters=[(0, 99)])
        assert idx.stats()["tiles"] == ntiles * idx.stats()["batches"]
        _same(got, want, "dense route under the sparse filter")
        idx.set_sparse_route(True)
        assert idx.search_range(c["q"], K, thr, filters=[(0, 12345)])[2].tolist() == [0] * mid["nq"]          # an empty tile list: padding, count 0
        # the regrow path: absurdly small candidate buffers, the batch runs again and rewrites lists AND counts
        idx.set_tuning(force_fallback=1)
        got = idx.search_range(c["q"], K, c["thr"])
        assert idx.stats()["fallback_used"] & 1
        got_l = idx.search_range(c["q"], K, c["thr"], counts=False)
        idx.set_tuning(force_fallback=0)
        _same(got, c["want"], "regrown")
        _same(got_l[:2] + (None,), c["want"][:2] + (None,), "regrown, list only")
    finally:
        idx.close()


def test_device_outputs_row_base_and_argument_checks(gpu, mid):
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    c = mid[True]
    idx = _index(ffi, mid["raw"], mid["codes"], ffi.DTYPE_BF16, mid["dead"])
    empty = ffi.Index(768, ffi.DTYPE_BF16, capacity_rows=64, n_code_cols=2, device=0)
    try:
        base, nq = 3 << 32, mid["nq"]
        qd = torch.from_numpy(c["q"]).cuda()
        os_ = torch.empty((nq, K), dtype=torch.float32, device="cuda")
        or_ = torch.empty((nq, K), dtype=torch.int64, device="cuda")
        oc = torch.full((nq,), -7, dtype=torch.int64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        idx.set_tuning(force_fallback=1)                       # (the re-run happens inside search_finish, thresholds kept with the batch)
        idx.search_range(qd, K, c["thr"], row_base=base, out_scores=os_, out_rows=or_, out_counts=oc, stream=stream)
        idx.search_finish(stream)
        idx.set_tuning(force_fallback=0)
        ws, wr, wc = c["want"]
        _same((os_.cpu().numpy(), or_.cpu().numpy(), oc.cpu().numpy()), (ws, np.where(wr >= 0, wr + base, wr), wc), "device outputs")
        # refused with nothing launched
        L = ffi.lib()
        for bad in (np.nan, np.inf, -np.inf):
            t = c["thr"].copy()
            t[7] = bad
            with pytest.raises(ffi.NativeError, match="finite"):
                idx.search_range(c["q"], K, t)
            rc = L.crh_search_range(idx._handle(), nq, c["q"].ctypes.data, 0, K, t.ctypes.data, None, 0, 0, os_.data_ptr(), or_.data_ptr(), None, 1, None)
            assert rc == ffi.E_INVALID and b"thresholds_host[7]" in L.crh_last_error()
        for k in (0, ffi.MAX_K + 1):
            rc = L.crh_search_range(idx._handle(), nq, c["q"].ctypes.data, 0, k, c["thr"].ctypes.data, None, 0, 0, os_.data_ptr(), or_.data_ptr(), None, 1, None)
            assert rc == ffi.E_INVALID and b"k=" in L.crh_last_error()
        with pytest.raises(ffi.NativeError, match="column"):
            idx.search_range(c["q"], K, c["thr"], filters=[(5, [1, 2])])
        # the largest k, and an empty index
        s, r, n = idx.search_range(c["q"][:3], ffi.MAX_K, np.asarray([-2.0, 2.0, c["thr"][5]], F32))
        _same((s, r, n), range_cases.select(c["scores"][:3], np.asarray([-2.0, 2.0, c["thr"][5]], F32), ffi.MAX_K, mid["alive"]), "k = MAX_K")
        s, r, n = empty.search_range(c["q"], K, c["thr"])
        assert (r == -1).all() and np.isneginf(s).all() and n.tolist() == [0] * nq
    finally:
        idx.close()
        empty.close()


def test_store_end_to_end_on_two_shards(gpu, mid):
    import coderag_amd  # noqa: F401
    from coderag_amd.store import HipVectorStore
    from tests.test_filter_sets_host import _payload
    n = 600
    raw = mid["raw"][:n].copy()
    raw[290:330] = raw[290]                                   # 40 identical rows across two upserts: they land on both shards
    ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(n)]
    payloads = [_payload(i, f"/proj/f{i % 12}.py", ("python", "go", "typescript")[i % 3], "p1") for i in range(n)]
    q = (raw[290] + 0.3 * mid[False]["q"][0]).astype(F32)
    scores = orc.scores(orc.preprocess(raw), orc.preprocess(q[None]))[0]
    thr = float(scores[290])                                  # the block's own score: inclusive, all 40 are in
    in_range = np.flatnonzero(scores >= np.float32(thr))
    py = np.asarray([i % 3 == 0 for i in range(n)])

    async def run():
        async with HipVectorStore(dim=768, dtype="f32", initial_capacity=512, device=0, shards=2, compact_dead_fraction=0.0) as s:
            await s.create_collections()
            for a in range(0, n, 100):                        # (blocks of rows go to the shards in turn)
                await s.upsert("code_chunks", ids[a:a + 100], raw[a:a + 100], payloads[a:a + 100])
            plain = await s.search("code_chunks", q.tolist(), limit=100)
            want = [(h["id"], h["score"]) for h in plain if np.float32(h["score"]) >= np.float32(thr)]
            assert len(want) == len(in_range) >= 40 and len(want) < 100
            got = await s.search("code_chunks", q.tolist(), limit=100, score_threshold=thr)
            assert [(h["id"], h["score"]) for h in got] == want
            assert [(h["id"], h["score"]) for h in await s.search("code_chunks", q.tolist(), limit=7, score_threshold=thr)] == want[:7]
            res = await s.search_range("code_chunks", q.tolist(), thr, limit=5)
            assert res["count"] == len(in_range) and [(h["id"], h["score"]) for h in res["hits"]] == want[:5]
            up = float(np.nextafter(np.float32(thr), np.float32(4)))
            assert await s.count_similar("code_chunks", q.tolist(), up) == int((scores >= np.float32(up)).sum()) <= len(in_range) - 40
            assert await s.count_similar("code_chunks", q.tolist(), -2.0) == n
            assert await s.count_similar("code_chunks", q.tolist(), thr, filters={"language": "python"}) == int((py & (scores >= np.float32(thr))).sum())
            assert await s.count_similar("code_chunks", q.tolist(), 2.0) == 0 and await s.search("code_chunks", q.tolist(), score_threshold=2.0) == []
            both = await s.search_range_batch("code_chunks", np.stack([q, q]), [thr, -2.0], limit=3)
            assert [b["count"] for b in both] == [len(in_range), n] and [h["id"] for h in both[0]["hits"]] == [w[0] for w in want[:3]]
    asyncio.run(run())
