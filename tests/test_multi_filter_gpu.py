"""Mixed-filter batches (``crh_search_multi``: every query under its own filter, one corpus pass per 64 queries) on the real index.

The checker is the f32 oracle under the row mask of EACH QUERY'S class -- computed here in numpy from the code columns and the
alive bits, as in test_filter_sets_gpu.py -- and ids and f32 score BITS must be equal.  (Reference behaviour this stands in for:
every query of query/vector_search.py:83-93 carries its own payload filter -- project_name always, language / entity_type
often -- and the reference sends one query per RPC.)"""
import asyncio
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _env():
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    return ffi


def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(np.asarray(a[0]).view(np.uint32), np.asarray(b[0]).view(np.uint32))


def np_mask(codes, alive, conds):
    ok = np.asarray(alive, bool).copy()
    for c in conds or []:
        if len(c) == 2 and isinstance(c[1], (int, np.integer)):
            ok &= codes[:, c[0]] == c[1]
        else:
            member = np.isin(codes[:, c[0]], np.asarray([v for v in c[1] if v >= 0], np.int32))
            ok &= ~member if (len(c) == 3 and c[2]) else member
    return ok


def expected(orc, xpre, qpre, k, codes, alive, classes, qclass):
    """Row i = the oracle's answer for query i under the mask of its class (one oracle call per class in use)."""
    qclass = np.asarray(qclass)
    es = np.empty((len(qpre), k), np.float32)
    er = np.empty((len(qpre), k), np.int64)
    for c in sorted(set(qclass.tolist())):
        sel = np.flatnonzero(qclass == c)
        s, r = orc.search(xpre, qpre[sel], k, alive=np_mask(codes, alive, classes[c]).astype(np.uint8))
        es[sel], er[sel] = s, r
    return es, er


ONE_ROW = 77777            # the row class 5 selects
# the class pool: the empty filter, equality, any-of, not-in, a class matching no row, a class matching exactly one row, two ANDs
POOL = [[], [(0, 3)], [(0, [1, 2, 5], False)], [(1, [0], True)], [(0, 99)], [(2, ONE_ROW)],
        [(0, 4), (1, [1, 2], False)], [(0, [6, 7], False), (1, [3], True)]]


def _corpus(rng, rows, dim):
    x = rng.standard_normal((rows, dim)).astype(np.float32)
    codes = np.stack([rng.integers(0, 8, rows), rng.integers(-1, 4, rows), np.arange(rows)], axis=1).astype(np.int32)   # column 0 interleaved: every tile has every project
    return x, codes


def _cycle(n_classes, nq, rng):
    qc = np.arange(nq) % n_classes
    rng.shuffle(qc)
    return qc.astype(np.int32)


@pytest.mark.parametrize("dtype_name,dim", [("bf16", 768), ("f32", 768), ("bf16", 1536), ("f32", 1536)])
def test_mixed_batches_equal_the_oracle_under_each_querys_mask(gpu, dtype_name, dim):
    import torch
    ffi = _env()
    from oracle import search as orc
    bf16 = dtype_name == "bf16"
    rows, extra = 150001, 77                                      # the second append starts inside a partly filled tile
    rng = np.random.default_rng(dim * 2 + bf16)
    x, codes = _corpus(rng, rows + extra, dim)
    q = rng.standard_normal((200, dim)).astype(np.float32)
    q[6] = q[5]                                                   # the same vector under two different classes (see qclass below)
    q[9] = x[ONE_ROW]
    idx = ffi.Index(dim, ffi.DTYPE_BF16 if bf16 else ffi.DTYPE_F32, capacity_rows=rows + extra + 64, n_code_cols=3)
    idx.append(x[:rows], codes[:rows])
    alive = np.ones(rows + extra, bool)
    dead = np.unique(rng.choice(rows, rows // 5, replace=False))
    dead = dead[dead != ONE_ROW]
    idx.tombstone(dead)
    alive[dead] = False
    idx.append(x[rows:], codes[rows:])
    xpre, qpre = orc.preprocess(x, to_bf16=bf16), orc.preprocess(q, to_bf16=bf16)
    per_pass = 32 if dim == 1536 else 64

    def check(nq, k, classes, qclass, tag):
        got = idx.search_multi(q[:nq], k, classes, qclass)
        st = idx.stats()
        want = expected(orc, xpre, qpre[:nq], k, codes, alive, classes, qclass)
        assert _same(got, want), (tag, nq, k, len(classes))
        return got, st

    # 1 .. 8 classes in one batch, k in {1, 10, 100}; queries 5 and 6 are one vector under two classes
    for n_classes in range(1, 9):
        k = (1, 10, 100)[n_classes % 3]
        qc = _cycle(n_classes, per_pass, rng)
        if n_classes > 1:
            qc[5], qc[6] = 0, 1
        if n_classes == 1:                                        # (ffi.search_multi sends one class to crh_search: the C entry directly)
            os_, or_ = np.empty((per_pass, k), np.float32), np.empty((per_pass, k), np.int64)
            idx._search_multi_native(np.ascontiguousarray(q[:per_pass]), k, [POOL[1]], qc, 0, os_, or_, 0)
            assert _same((os_, or_), expected(orc, xpre, qpre[:per_pass], k, codes, alive, [POOL[1]], qc))
            continue
        got, st = check(per_pass, k, POOL[:n_classes], qc, "classes")
        assert st["batches"] == 1 and st["tiles"] == (rows + extra + 31) // 32
        if n_classes >= 5:                                        # the class that matches no row: all padding
            none = np.flatnonzero(qc == 4)
            assert (got[1][none] == -1).all() and np.isneginf(got[0][none]).all()
        if n_classes >= 6:                                        # the class of exactly one row
            one = np.flatnonzero(qc == 5)
            assert (got[1][one, 0] == ONE_ROW).all() and (got[1][one, 1:] == -1).all()
    # short and long batches
    for nq in ((1, 33, 64, 65, 200) if (bf16 and dim == 768) else (1, 65)):
        qc = _cycle(8, nq, rng)
        _, st = check(nq, 10, POOL, qc, "nq")
        assert st["batches"] == (nq + per_pass - 1) // per_pass
    # row i equals crh_search_cond for query i alone, on the same index
    qc = _cycle(8, per_pass, rng)
    qc[5], qc[6], qc[9] = 2, 3, 5
    got, _ = check(per_pass, 100, POOL, qc, "lone")
    for i in (0, 5, 6, 9, 17, per_pass - 1):
        lone = idx.search(q[i:i + 1], 100, filters=[(c[0], [c[1]], False) if len(c) == 2 else c for c in POOL[qc[i]]])
        assert _same((got[0][i:i + 1], got[1][i:i + 1]), lone), i
    assert not np.array_equal(got[1][5], got[1][6])                # one vector, two classes, two answers
    # the nomination mode is irrelevant to a mixed batch
    for mode in (ffi.NOMINATE_BF16_3, ffi.NOMINATE_BF16, ffi.NOMINATE_INT8):
        idx.set_nomination(mode)
        assert _same(idx.search_multi(q[:per_pass], 100, POOL, qc), got), mode
    # the regrow-and-rerun path runs the classed pipeline again
    idx.set_tuning(force_fallback=1)
    again = idx.search_multi(q[:per_pass], 100, POOL, qc)
    st = idx.stats()
    idx.set_tuning(force_fallback=0)
    assert st["fallback_used"] & 1 and _same(again, got)
    # row_base, device outputs and crh_search_finish
    base, k = 1 << 33, 10
    qd = torch.from_numpy(q[:per_pass + 3]).cuda()
    qc2 = _cycle(8, per_pass + 3, rng)
    os_ = torch.empty((per_pass + 3, k), dtype=torch.float32, device="cuda")
    or_ = torch.empty((per_pass + 3, k), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    idx.search_multi(qd, k, POOL, qc2, row_base=base, out_scores=os_, out_rows=or_, stream=stream)
    idx.search_finish(stream)
    es, er = expected(orc, xpre, qpre[:per_pass + 3], k, codes, alive, POOL, qc2)
    assert _same((os_.cpu().numpy(), or_.cpu().numpy()), (es, np.where(er >= 0, er + base, er)))
    # the class masks are kept between calls, beside the single mask, and follow mutations
    single = idx.search(q[:8], 10, filters=POOL[2])
    assert _same(idx.search_multi(q[:per_pass], 100, POOL, qc), got)
    assert _same(idx.search(q[:8], 10, filters=POOL[2]), single)
    more = np.unique(got[1][got[1] >= 0])[:50]
    more = more[more != ONE_ROW]
    idx.tombstone(more)
    alive[more] = False
    check(per_pass, 100, POOL, qc, "after tombstone")
    # more than 8 distinct filters: several calls, caller order
    many = POOL + [[(0, p)] for p in (0, 1, 2)]
    qc = _cycle(len(many), per_pass + 7, rng)
    check(per_pass + 7, 10, many, qc, "11 classes")
    # argument checks of the C entry
    L, h = ffi.lib(), idx._handle()
    o_s, o_r = np.empty((2, 5), np.float32), np.empty((2, 5), np.int64)
    q2 = np.ascontiguousarray(q[:2])
    cond = (ffi.Condition * 1)()
    code = np.asarray([3], np.int32)
    cond[0].col, cond[0].negate, cond[0].n, cond[0].codes = 0, 0, 1, code.ctypes.data
    off = np.asarray([0, 1, 1, 1, 1, 1, 1, 1, 1, 1], np.int32)

    def call(n_classes, qcl, col=0):
        cond[0].col = col
        qcl = np.asarray(qcl, np.int32)
        return L.crh_search_multi(h, 2, q2.ctypes.data, 0, 5, cond, off.ctypes.data, n_classes, qcl.ctypes.data, 0, o_s.ctypes.data, o_r.ctypes.data, 0, None)
    assert call(2, [0, 1]) == ffi.OK
    assert call(2, [0, 2]) == ffi.E_INVALID and call(2, [-1, 0]) == ffi.E_INVALID      # class ids
    assert call(0, [0, 0]) == ffi.E_INVALID and call(9, [0, 0]) == ffi.E_INVALID       # n_classes
    assert call(2, [0, 1], col=3) == ffi.E_INVALID and call(2, [0, 1], col=-1) == ffi.E_INVALID
    idx.close()


@pytest.mark.parametrize("dtype_name,dim", [("bf16", 768), ("f32", 1536)])
def test_union_sparse_route_reads_only_the_unions_tiles(gpu, dtype_name, dim):
    """Eight contiguous projects that together populate 1/8 of the tiles: the batch walks the list of the union's tiles
    (crh_search_stats.tiles is bounded by the non-zero words of the union mask -- derived, not tuned) and answers with the bits
    of the oracle and of the dense classed route."""
    ffi = _env()
    from oracle import search as orc
    bf16 = dtype_name == "bf16"
    rows = 150011
    rng = np.random.default_rng(rows + dim)
    x = rng.standard_normal((rows, dim)).astype(np.float32)
    proj = (np.arange(rows) * 64 // rows).astype(np.int32)        # 64 contiguous projects whose ends fall inside tiles
    codes = np.stack([proj, rng.integers(0, 3, rows).astype(np.int32)], axis=1)
    idx = ffi.Index(dim, ffi.DTYPE_BF16 if bf16 else ffi.DTYPE_F32, capacity_rows=rows, n_code_cols=2)
    idx.append(x, codes)
    alive = np.ones(rows, bool)
    dead = np.unique(rng.choice(rows, 5000, replace=False))
    idx.tombstone(dead)
    alive[dead] = False
    xpre = orc.preprocess(x, to_bf16=bf16)
    per_pass = 32 if dim == 1536 else 64
    nq = per_pass + 6
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    qpre = orc.preprocess(q, to_bf16=bf16)
    classes = [[(0, p)] for p in (3, 4, 17, 30, 31, 44, 58)] + [[(0, 63), (1, [1], True)]]
    qc = _cycle(8, nq, rng)
    union = np.zeros(rows, bool)
    for c in classes:
        union |= np_mask(codes, alive, c)
    n_pad = -rows % 32
    nz = int(np.pad(union, (0, n_pad)).reshape(-1, 32).any(axis=1).sum())
    ntiles = (rows + 31) // 32
    assert 0 < nz * 4 <= ntiles
    batches = (nq + per_pass - 1) // per_pass
    for k in (10, 100):
        idx.set_sparse_route(True)
        got = idx.search_multi(q, k, classes, qc)
        st = idx.stats()
        print(f"k={k}: tiles {st['tiles']} seed {st['seed_tiles']} union words {nz} all tiles {ntiles} fallback {st['fallback_used']}")
        assert st["batches"] == batches and 0 < st["tiles"] <= nz * batches and st["seed_tiles"] <= nz * batches
        assert st["rows"] <= 32 * nz * batches
        assert _same(got, expected(orc, xpre, qpre, k, codes, alive, classes, qc)), k
        idx.set_sparse_route(False)
        dense = idx.search_multi(q, k, classes, qc)
        assert idx.stats()["tiles"] == ntiles * batches
        assert _same(got, dense), k
    # a union that matches nothing: padding, nothing read
    idx.set_sparse_route(True)
    got = idx.search_multi(q[:4], 5, [[(0, 100)], [(0, 101)]], [0, 1, 0, 1])
    assert (got[1] == -1).all() and np.isneginf(got[0]).all() and idx.stats()["tiles"] == 0
    # the regrow path keeps the route
    idx.set_tuning(force_fallback=1)
    got = idx.search_multi(q, 100, classes, qc)
    st = idx.stats()
    idx.set_tuning(force_fallback=0)
    assert st["fallback_used"] & 1 and _same(got, expected(orc, xpre, qpre, 100, codes, alive, classes, qc))
    idx.close()


@pytest.mark.parametrize("dtype_name", ["bf16", "f32"])
def test_mixed_and_single_filter_calls_each_keep_a_correct_mask(gpu, dtype_name):
    """A mixed-filter call and the single-filter calls around it keep their masks side by side: each must find its own as it
    left it, and rebuild it after a mutation, on another stream and when the sparse route is switched.  129 tiles, the last one
    partial: the tile-list kernels run one block of more than one wave.  The single filter populates 26 tiles (sparse route),
    the union of the two classes every tile (dense classed scan).  After every call: ids and score bits of the oracle under
    each query's mask; after a sparse call crh_search_stats.tiles is bounded by the non-zero words of the numpy mask."""
    import torch
    ffi = _env()
    from oracle import search as orc
    bf16 = dtype_name == "bf16"
    rows, dim, nq, k = 4113, 384, 40, 10
    ntiles = (rows + 31) // 32
    rng = np.random.default_rng(4113 + bf16)
    x = rng.standard_normal((rows, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    tile = np.arange(rows) // 32
    col0 = rng.choice(np.asarray([0, 2, 3, 4], np.int32), rows)
    in_a = (tile % 5 == 3) & (rng.random(rows) < 0.5)             # tiles 3, 8, .. 128 -- the partial one among them
    in_a[np.arange(3, ntiles, 5) * 32 + 1] = True                 # (each of them for certain)
    col0[in_a] = 1
    col0[::32] = 2                                                # every tile has a row of class 0
    codes = np.stack([col0, rng.integers(-1, 4, rows).astype(np.int32)], axis=1)
    A = [(0, 1)]
    classes = [[(0, [1, 2], False)], [(0, [1, 2], True), (1, 3)]]
    qc = _cycle(2, nq, rng)
    idx = ffi.Index(dim, ffi.DTYPE_BF16 if bf16 else ffi.DTYPE_F32, capacity_rows=rows, n_code_cols=2)
    idx.append(x, codes)
    alive = np.ones(rows, bool)
    xpre, qpre = orc.preprocess(x, to_bf16=bf16), orc.preprocess(q, to_bf16=bf16)

    def words(mask):
        return int(np.pad(mask, (0, -rows % 32)).reshape(-1, 32).any(axis=1).sum())

    want = {}

    def refresh():                                                # the oracle's answers and the masks' words, once per state of the index
        want["A"] = expected(orc, xpre, qpre, k, codes, alive, [A], np.zeros(nq, np.int32))
        want["M"] = expected(orc, xpre, qpre, k, codes, alive, classes, qc)
        want["nzA"] = words(np_mask(codes, alive, A))
        want["nzM"] = words(np_mask(codes, alive, classes[0]) | np_mask(codes, alive, classes[1]))
        assert 0 < want["nzA"] * 4 <= ntiles and want["nzM"] == ntiles

    def single(step, sparse=True, rerun=False):
        got = idx.search(q, k, filters=A)
        st = idx.stats()
        print(f"step {step}: search(A) tiles {st['tiles']} (mask words {want['nzA']}, all tiles {ntiles}) fallback {st['fallback_used']}")
        assert _same(got, want["A"]), step
        assert rerun or (st["batches"] == 1 and (0 < st["tiles"] <= want["nzA"] if sparse else st["tiles"] == ntiles)), step
        return st

    def multi(step, rerun=False):
        got = idx.search_multi(q, k, classes, qc)
        st = idx.stats()
        print(f"step {step}: search_multi tiles {st['tiles']} (union words {want['nzM']}) fallback {st['fallback_used']}")
        assert _same(got, want["M"]), step
        assert rerun or (st["batches"] == 1 and st["tiles"] == ntiles), step   # (the union leaves no tile out: the dense classed scan)
        return st

    refresh()
    single(1)
    multi(2)
    single(3)
    dead = np.flatnonzero(np_mask(codes, alive, A))[::3]
    idx.tombstone(dead)
    alive[dead] = False
    refresh()
    multi(5)
    single(6)
    idx.set_sparse_route(False)
    single(8, sparse=False)
    multi(9)
    idx.set_sparse_route(True)
    # a second stream, device buffers: the kept mask was built on the default stream and nothing orders the two
    qd = torch.from_numpy(q).cuda()
    os_ = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    or_ = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    idx.search(qd, k, filters=A, out_scores=os_, out_rows=or_, stream=side.cuda_stream)
    idx.search_finish(side.cuda_stream)
    side.synchronize()
    st = idx.stats()
    assert _same((os_.cpu().numpy(), or_.cpu().numpy()), want["A"]), 11
    assert st["batches"] == 1 and 0 < st["tiles"] <= want["nzA"], 11
    multi(12)
    # the regrow-and-rerun path builds the masks and enqueues again, for both kinds (a batch run twice counts its tiles twice)
    idx.set_tuning(force_fallback=1)
    st_m = multi(13, rerun=True)
    st_a = single(14, rerun=True)
    idx.set_tuning(force_fallback=0)
    assert st_m["fallback_used"] & 1 and st_a["fallback_used"] & 1
    idx.close()


def _payload(i, file, lang, proj):
    return {"file_path": file, "entity_type": "function", "entity_name": f"ent{i}", "language": lang, "start_line": i, "end_line": i + 3,
            "content": f"def ent{i}(): pass", "graph_node_id": f"mod.ent{i}", "content_hash": "h", "project_name": proj}


def test_store_per_query_filters_and_the_filter_coalescer(gpu):
    import coderag_amd  # noqa: F401
    from coderag_amd.store import HipVectorStore

    async def run(shards):
        rng = np.random.default_rng(17 + shards)
        n, dim = 4000, 768
        vecs = rng.standard_normal((n, dim)).astype(np.float32)
        langs = [("python", "go", "typescript", "rust")[i % 4] for i in range(n)]
        projs = [f"p{i * 6 // n}" for i in range(n)]
        payloads = [_payload(i, f"/proj/f{i % 300}.py", langs[i], projs[i]) for i in range(n)]
        ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(n)]
        flt = [{"project_name": "p0"}, {"project_name": "p1", "language": "go"}, None, {"language": ["python", "rust"]},
               {"project_name": "never-stored"}, {"project_name": "p5"}]
        mnot = [None, {"file_path": "/proj/f7.py"}, {"language": "go"}, None, None, {"language": ["go", "rust"]}]
        nq = 90
        qs = rng.standard_normal((nq, dim)).astype(np.float32)
        async with HipVectorStore(dim=dim, dtype="f32", initial_capacity=4096, device=0, shards=shards, compact_dead_fraction=0.0,
                                  coalesce_filters=True) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, vecs, payloads)
            lone = [await s.search("code_chunks", qs[i].tolist(), limit=5 + i % 7, filters=flt[i % 6], must_not=mnot[i % 6]) for i in range(nq)]
            assert all(lone[i] == [] for i in range(4, nq, 6)) and all(len(lone[i]) == 5 + i % 7 for i in range(0, nq, 6))
            got = await s.search_batch("code_chunks", qs, limit=11, filters=[flt[i % 6] for i in range(nq)], must_not=[mnot[i % 6] for i in range(nq)])
            for i in range(nq):
                assert [(h["id"], h["score"]) for h in got[i][:5 + i % 7]] == [(h["id"], h["score"]) for h in lone[i]], i
            before = s.search_passes
            co = await asyncio.gather(*[s.search("code_chunks", qs[i].tolist(), limit=5 + i % 7, filters=flt[i % 6], must_not=mnot[i % 6])
                                        for i in range(nq)])
            assert list(co) == lone
            assert s.search_passes - before <= (nq + 63) // 64 + 1
    asyncio.run(run(1))
    asyncio.run(run(2))
