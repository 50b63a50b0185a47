"""Set conditions ("in" / "not in" a set of codes) and the sparse route of filtered searches on the real HIP index.

The checker is the f32 oracle under an arbitrary row mask: the expected mask is computed here in numpy from the code columns,
AND-ed with the alive bits, and ids and f32 score BITS must match (as in test_search_gpu.py).  Semantics (include/coderag_hip.h,
crh_condition): an empty "in" set matches nothing, an empty "not in" set everything; a row whose code is -1 is in no set.
(Reference behaviour this stands in for: Qdrant's MatchAny / must_not / MatchExcept conditions and its payload indexes,
embeddings/client.py:93-113 -- the reference itself filters exclusions on the host, query/vector_search.py:199-215.)"""
import asyncio

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
    """The rows a filter keeps: every condition -- (col, code) or (col, codes, negate) -- AND the alive bits."""
    ok = np.asarray(alive, bool).copy()
    for c in conds or []:
        if len(c) == 2 and isinstance(c[1], (int, np.integer)):
            ok &= codes[:, c[0]] == c[1]
        else:
            member = np.isin(codes[:, c[0]], np.asarray([v for v in c[1] if v >= 0], np.int32))
            ok &= ~member if (len(c) == 3 and c[2]) else member
    return ok


def _oracle(orc, xpre, qpre, k, mask):
    return orc.search(xpre, qpre, k, alive=mask.astype(np.uint8))


@pytest.mark.parametrize("dtype_name,dim", [("bf16", 768), ("f32", 768), ("bf16", 384), ("f32", 1024)])
def test_set_conditions_equal_the_oracle_under_the_numpy_mask(gpu, dtype_name, dim):
    ffi = _env()
    from oracle import search as orc
    bf16 = dtype_name == "bf16"
    rows, nq, k = 6001, 70, 40                                    # 70 queries: more than one 64-query batch
    rng = np.random.default_rng(dim + bf16)
    x = rng.standard_normal((rows, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    codes = np.stack([rng.integers(0, 4, rows), rng.integers(0, 3000, rows), rng.integers(-1, 3, rows)], axis=1).astype(np.int32)
    many = sorted(set(rng.integers(0, 4000, 1500).tolist()))      # ~1100 distinct codes, a quarter of them in no row
    cases = [
        [(0, [1], False)], [(0, [1, 2], False)], [(1, many, False)], [(0, [2], True)], [(1, many, True)],
        [(2, [0, 1], False)],                                     # a -1 row is in no set ...
        [(2, [0], True)], [(2, [-1, 0], True)],                   # ... and outside every set; a -1 in the set itself is ignored
        [(0, [], False)], [(0, [], True)],
        [(0, 1), (1, many, False)], [(0, 2), (2, [1], True)], [(0, [1, 3], False), (1, many, True), (2, 0)],
        [(0, [3, 3, 1, 1], False)],                               # repeats and any order
    ]
    idx = ffi.Index(dim, ffi.DTYPE_BF16 if bf16 else ffi.DTYPE_F32, capacity_rows=rows + 64, n_code_cols=3)
    idx.append(x, codes)
    xpre, qpre = orc.preprocess(x, to_bf16=bf16), orc.preprocess(q, to_bf16=bf16)
    alive = np.ones(rows, bool)

    def check(xp, cd, al, tag):
        unfiltered = idx.search(q, k)
        for conds in cases:
            got = idx.search(q, k, filters=conds)
            m = np_mask(cd, al, conds)
            assert _same(got, _oracle(orc, xp, qpre, k, m)), (tag, conds[0][0], len(conds))
            if conds == [(0, [], False)]:
                assert (got[1] == -1).all() and np.isneginf(got[0]).all()
            if conds == [(0, [], True)]:
                assert _same(got, unfiltered)
            assert idx.count_matching(conds) == int(m.sum())

    check(xpre, codes, alive, "fresh")
    dead = np.sort(rng.choice(rows, rows // 3, replace=False))
    idx.tombstone(dead)
    alive[dead] = False
    check(xpre, codes, alive, "tombstoned")
    o2n = idx.compact()
    keep = np.flatnonzero(alive)
    assert np.array_equal(o2n[keep], np.arange(len(keep)))
    check(xpre[keep], codes[keep], np.ones(len(keep), bool), "compacted")
    idx.close()


def test_match_and_delete_with_sets_equal_numpy(gpu):
    ffi = _env()
    rows = 50000
    rng = np.random.default_rng(5)
    x = rng.standard_normal((rows, 384)).astype(np.float32)
    codes = np.stack([rng.integers(0, 40000, rows), rng.integers(-1, 5, rows)], axis=1).astype(np.int32)
    idx = ffi.Index(384, ffi.DTYPE_BF16, capacity_rows=rows, n_code_cols=2)
    idx.append(x, codes)
    alive = np.ones(rows, bool)
    idx.tombstone(np.arange(0, rows, 7))
    alive[::7] = False
    big = rng.choice(40000, 20000, replace=False).tolist()        # 20 000 codes: one call
    for conds in ([(0, big, False)], [(0, big, True), (1, [0, 4], False)], [(1, [2], True)], [(1, [], False)], [(0, big[:1], False), (1, 3)]):
        want = np.flatnonzero(np_mask(codes, alive, conds))
        assert idx.count_matching(conds) == len(want)
        assert np.array_equal(idx.match_rows(conds, limit=rows), want)
        assert np.array_equal(idx.match_rows(conds, limit=17), want[:17])
    calls = ffi.Index.device_calls
    conds = [(0, big, False), (1, [1, 2], True)]
    want = np_mask(codes, alive, conds)
    assert idx.tombstone_filter(conds) == int(want.sum()) and ffi.Index.device_calls == calls + 1
    alive &= ~want
    assert idx.count()[1] == int(alive.sum())
    assert np.array_equal(idx.match_rows(None, limit=rows), np.flatnonzero(alive))
    assert idx.tombstone_filter([(0, [], True), (1, [0], False)]) == int((alive & (codes[:, 1] == 0)).sum())
    idx.close()


def _project_corpus(rng, rows, dim):
    """Contiguous "projects" (column 0) as rows arrive project by project; project 7 holds ~1/64 of the rows and starts and
    ends inside a tile; project 9 holds 50 rows.  Column 1 is scattered (every tile has every value)."""
    x = rng.standard_normal((rows, dim)).astype(np.float32)
    proj = np.empty(rows, np.int32)
    start7, len7 = 100003, rows // 64 + 5
    start9 = 150011
    bounds = sorted(set(rng.choice(rows, 40, replace=False).tolist()) | {0})
    for i, b in enumerate(bounds):
        proj[b:bounds[i + 1] if i + 1 < len(bounds) else rows] = 20 + i
    proj[start7:start7 + len7] = 7
    proj[start9:start9 + 50] = 9
    codes = np.stack([proj, rng.integers(0, 3, rows).astype(np.int32)], axis=1).astype(np.int32)
    return x, codes, (start7, len7)


@pytest.mark.parametrize("dtype_name,dim,rows", [("bf16", 768, 204813), ("f32", 384, 200003)])
def test_sparse_route_is_exact_and_reads_only_populated_tiles(gpu, dtype_name, dim, rows):
    """A search filtered to one contiguous project reads the tiles that project populates and no others, and answers with the
    bits of the oracle and of the dense route.  The bounds on `tiles` / `seed_tiles` are derived, not tuned: the list holds
    exactly the non-zero words of the mask.  (Without the sparse route `tiles` is every tile of the index.)"""
    import torch
    ffi = _env()
    from oracle import search as orc
    bf16 = dtype_name == "bf16"
    rng = np.random.default_rng(rows)
    x, codes, (s7, l7) = _project_corpus(rng, rows, dim)
    idx = ffi.Index(dim, ffi.DTYPE_BF16 if bf16 else ffi.DTYPE_F32, capacity_rows=rows, n_code_cols=2)
    idx.append(x, codes)
    alive = np.ones(rows, bool)
    dead = np.concatenate([s7 + rng.choice(l7, l7 // 10, replace=False), rng.choice(rows, 3000, replace=False)])
    idx.tombstone(np.unique(dead))
    alive[dead] = False
    xpre = orc.preprocess(x, to_bf16=bf16)
    q = rng.standard_normal((70, dim)).astype(np.float32)
    q[3] = x[s7 + 11]
    qpre = orc.preprocess(q, to_bf16=bf16)

    def words(mask, n):
        return int(np.add.reduceat(np.pad(mask, (0, -n % 32)).astype(np.int64), np.arange(0, n + (-n % 32), 32)).astype(bool).sum())

    def check(xp, cd, al, tag):
        n = len(al)
        ntiles = (n + 31) // 32
        for conds, k, nq in (([(0, 7)], 100, 64), ([(0, [7], False)], 100, 70), ([(0, 9)], 100, 5),       # k > the 50 rows of project 9: padding
                             ([(0, 7), (1, [0, 2], False)], 100, 64), ([(0, [7, 9], False), (1, [1], True)], 1024, 33)):
            m = np_mask(cd, al, conds)
            nz = words(m, n)
            assert 0 < nz * 8 <= ntiles                                # sparse by any crossover this library would use
            idx.set_sparse_route(True)
            got = idx.search(q[:nq], k, filters=conds)
            st = idx.stats()
            batches = (nq + 63) // 64
            print(f"{tag} {conds[0]} nq={nq} k={k}: tiles {st['tiles']} seed {st['seed_tiles']} nonzero words {nz} all tiles {ntiles} fallback {st['fallback_used']}")
            assert st["batches"] == batches and st["tiles"] <= nz * batches and st["seed_tiles"] <= nz * batches
            assert 0 < st["tiles"] and st["rows"] <= 32 * nz * batches
            assert _same(got, _oracle(orc, xp, qpre[:nq], k, m)), (tag, conds)
            idx.set_sparse_route(False)
            dense = idx.search(q[:nq], k, filters=conds)
            assert idx.stats()["tiles"] >= ntiles                      # the A/B switch: the dense route streams every tile
            assert _same(got, dense), (tag, conds)
            if conds == [(0, 9)]:
                assert (got[1][:, int(m.sum()):] == -1).all() and np.isneginf(got[0][:, int(m.sum()):]).all()
        # row_base, device outputs and crh_search_finish
        idx.set_sparse_route(True)
        conds, k, base = [(0, 7), (1, [0, 1], False)], 50, 1 << 32
        qd = torch.from_numpy(q[:64]).cuda()
        os_, or_ = torch.empty((64, k), dtype=torch.float32, device="cuda"), torch.empty((64, k), dtype=torch.int64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        idx.search(qd, k, filters=conds, row_base=base, out_scores=os_, out_rows=or_, stream=stream)
        idx.search_finish(stream)
        m = np_mask(cd, al, conds)
        assert idx.stats()["tiles"] <= words(m, n)
        es, er = _oracle(orc, xp, qpre[:64], k, m)
        assert _same((os_.cpu().numpy(), or_.cpu().numpy()), (es, np.where(er >= 0, er + base, er))), tag
        # the regrow-and-rerun path keeps the route and the answer
        idx.set_tuning(force_fallback=1)
        got = idx.search(q[:64], 100, filters=[(0, 7)])
        st = idx.stats()
        idx.set_tuning(force_fallback=0)
        m = np_mask(cd, al, [(0, 7)])
        assert st["fallback_used"] & 1 and _same(got, _oracle(orc, xp, qpre[:64], 100, m)), tag

    check(xpre, codes, alive, "tombstoned")
    o2n = idx.compact()
    keep = np.flatnonzero(alive)
    assert np.array_equal(o2n[keep], np.arange(len(keep)))
    check(xpre[keep], codes[keep], np.ones(len(keep), bool), "compacted")
    idx.close()


def test_dense_route_is_untouched_by_a_filter_that_populates_every_tile(gpu):
    ffi = _env()
    from oracle import search as orc
    rows, dim = 60000, 768
    rng = np.random.default_rng(11)
    x = rng.standard_normal((rows, dim)).astype(np.float32)
    codes = rng.integers(0, 3, (rows, 1)).astype(np.int32)
    q = rng.standard_normal((64, dim)).astype(np.float32)
    idx = ffi.Index(dim, ffi.DTYPE_BF16, capacity_rows=rows, n_code_cols=1)
    idx.append(x, codes)
    ntiles = (rows + 31) // 32
    out = {}
    for on in (True, False):
        idx.set_sparse_route(on)
        mode = idx.nomination()
        got = idx.search(q, 100, filters=[(0, 1)])
        st = idx.stats()
        out[on] = (mode, st["tiles"], st["seed_tiles"], st["batches"], got)
    assert out[True][:4] == out[False][:4] and out[True][1] == ntiles and _same(out[True][4], out[False][4])
    m = np_mask(codes, np.ones(rows, bool), [(0, 1)])
    assert _same(out[True][4], _oracle(orc, orc.preprocess(x, to_bf16=True), orc.preprocess(q, to_bf16=True), 100, m))
    idx.close()


def _payload(i, file, lang, proj):
    return {"file_path": file, "entity_type": "function", "entity_name": f"ent{i}", "language": lang, "start_line": i, "end_line": i + 3,
            "content": f"def ent{i}(): pass", "graph_node_id": f"mod.ent{i}", "content_hash": "h", "project_name": proj}


class _Embedder:
    def __init__(self, vec):
        self.vec = vec

    async def embed(self, text):
        return self.vec.tolist()


def test_store_sets_must_not_exact_exclude_and_one_call_deletes(gpu):
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from coderag_amd.store import HipVectorStore
    from coderag_amd.vector_search import VectorSearcher

    async def run(shards):
        rng = np.random.default_rng(3)
        n, dim = 3000, 768
        vecs = rng.standard_normal((n, dim)).astype(np.float32)
        q = rng.standard_normal(dim).astype(np.float32)
        hot = "/proj/hot.py"
        vecs[:10] = q + 0.01 * rng.standard_normal((10, dim)).astype(np.float32)       # one file owns the top 10
        files = [hot if i < 10 else f"/proj/f{i % 1500}.py" for i in range(n)]
        langs = [("python", "go", "typescript", "rust")[i % 4] for i in range(n)]
        payloads = [_payload(i, files[i], langs[i], "p1" if i < 2000 else "p2") for i in range(n)]
        ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(n)]
        async with HipVectorStore(dim=dim, dtype="f32", initial_capacity=4096, device=0, shards=shards, compact_dead_fraction=0.0) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, vecs, payloads)
            everything = await s.search("code_chunks", q.tolist(), limit=1024)
            p = files[20]
            want = [h for h in everything if h["payload"]["language"] in ("python", "go") and h["payload"]["file_path"] != p][:30]
            got = await s.search("code_chunks", q.tolist(), limit=30, filters={"language": ["python", "go"]}, must_not={"file_path": p})
            assert [(h["id"], h["score"]) for h in got] == [(h["id"], h["score"]) for h in want]
            got = await s.search_batch("code_chunks", q[None], limit=30, filters={"language": {"python", "go", "cobol"}, "project_name": ("p1", "p2")},
                                       must_not={"file_path": [p, "/never/stored.py"]})
            assert [(h["id"], h["score"]) for h in got[0]] == [(h["id"], h["score"]) for h in want]
            assert await s.search("code_chunks", q.tolist(), limit=5, filters={"language": ["cobol", "fortran"]}) == []
            assert await s.search("code_chunks", q.tolist(), limit=5, must_not={"language": "cobol"}) == everything[:5]

            vs = VectorSearcher(s, _Embedder(q))
            default = await vs.find_similar_code("snippet", limit=10, exclude_file=hot)
            exact = await vs.find_similar_code("snippet", limit=10, exclude_file=hot, exact_exclude=True)
            assert len(default) == 5                                    # the reference's shape: 15 fetched, 10 of them the file's
            assert len(exact) == 10 and all(h["file_path"] != hot for h in exact)
            assert [h["score"] for h in exact] == [h["score"] for h in everything if h["payload"]["file_path"] != hot][:10]

            calls = ffi.Index.device_calls
            gone = [f"/proj/f{i}.py" for i in range(1000)] + ["/never/stored.py"]
            await s.delete_files("code_chunks", gone)
            assert ffi.Index.device_calls == calls + shards             # ONE device call per shard for 1 000 paths
            left = await s.get_collection_info("code_chunks")
            assert left.points_count == sum(1 for f in files if f not in set(gone))
    asyncio.run(run(1))
    asyncio.run(run(2))
