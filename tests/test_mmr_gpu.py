"""Diversity-aware top-k (MMR) on the device: ``crh_index_gather_vectors`` against ``read_rows`` and ``crh_mmr_select`` /
``HipVectorStore.search(diversity=...)`` against the CPU restatement (tests/mmr_cases.py).  Every comparison is BIT-EXACT on
positions, rows and the bits of score and objective -- no tolerance appears anywhere: both sides run the same separately
rounded f32 operations.

The restatement is a deterministic greedy loop, so its ``k``-pick result is the prefix of its ``C``-pick result
(tests/test_mmr_host.py pins that): the sweeps run it once per candidate list at ``k = C`` and compare every ``k`` of the
device against that prefix."""
import asyncio

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIMS = (384, 768, 1024, 1536)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _device_select(torch, ffi, scores, rows, vecs, k, diversity):
    out = ffi.mmr_select(torch.from_numpy(scores).cuda(), torch.from_numpy(rows).cuda(), torch.from_numpy(vecs).cuda(), k, diversity)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _assert_equal(got, want, k, what):
    """``got``: the device's [nq, k] outputs; ``want``: the restatement's [nq, >= k] outputs, compared on their first k columns --
    behind a query's picks both hold the padding record."""
    for g, w, name in zip(got, want, ("pos", "rows", "scores", "obj")):
        w = w[:, :k]
        if name in ("scores", "obj"):
            assert np.array_equal(_bits(g), _bits(w)), f"{what}: {name} bits differ\n{g}\n{w}"
        else:
            assert g.dtype == w.dtype and np.array_equal(g, w), f"{what}: {name} differ\n{g}\n{w}"


# ------------------------------------------------------------------ crh_index_gather_vectors
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dtype_name", ["f32", "bf16"])
@pytest.mark.parametrize("i8_live", [True, False])
def test_gather_vectors_equals_read_rows(gpu, monkeypatch, dtype_name, dim, i8_live):
    """Owned rows give the stored row, rows of other shards (``row_base`` offsets) and -1 give zeros -- from the f32 master, from
    the row-major bf16 side copy while the int8 nomination copy is live (tests/conftest.py lets every index use it; a search
    brings it up to date), from the tiled image for tiles appended since (no search in between) and with the copy switched off
    (CODERAG_HIP_I8=0: the library's own switch, so no 1M-row index is needed)."""
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    if not i8_live:
        monkeypatch.setenv("CODERAG_HIP_I8", "0")
    rng = np.random.default_rng(dim + i8_live)
    n0, n1 = 1500, 700
    x = rng.standard_normal((n0 + n1, dim)).astype(np.float32)
    idx = ffi.Index(dim, ffi.DTYPE_BF16 if dtype_name == "bf16" else ffi.DTYPE_F32, capacity_rows=4096, device=0)
    try:
        idx.append(x[:n0])
        idx.search(rng.standard_normal((4, dim)).astype(np.float32), 10)
        assert (idx.nomination() == ffi.NOMINATE_INT8) == i8_live
        base = 5 << 32
        for count in (n0, n0 + n1):
            if count > n0:
                idx.append(x[n0:])                                           # new tiles: the side copy does not cover them yet
            stored = idx.read_rows(0, count)
            local = np.concatenate([rng.integers(0, count, 300), [0, count - 1, 31, 32, n0 - 1, min(n0, count - 1)]])
            rows = local + base
            rows[5::7] = -1                                                  # padding
            rows[3::11] = local[3::11] + (4 << 32)                           # a lower shard's row
            rows[2::13] = local[2::13] + base + count                        # past this shard's end
            rows[4::17] = local[4::17]                                       # row_base 0's rows: below this shard's base
            rows = rows.reshape(2, -1)
            own = (rows >= base) & (rows < base + count)
            want = np.where(own[:, :, None], stored[np.clip(rows - base, 0, count - 1)], np.float32(0))
            out = torch.full(rows.shape + (dim,), 7.0, dtype=torch.float32, device="cuda:0")
            got = idx.gather_vectors(torch.from_numpy(rows).cuda(), row_base=base, out=out)
            torch.cuda.synchronize()
            assert got is out and np.array_equal(_bits(got.cpu().numpy()), _bits(want)) and own.sum() > 100
        with pytest.raises(ffi.NativeError, match="device tensor"):
            idx.gather_vectors(np.zeros((3,), np.int64))
        with pytest.raises(ffi.NativeError, match="int64"):
            idx.gather_vectors(torch.zeros((3,), dtype=torch.int32, device="cuda:0"))
    finally:
        idx.close()


# ------------------------------------------------------------------ crh_mmr_select against the restatement
def _sets(dim):
    """(name, preprocessed corpus, preprocessed queries): random unit rows (f32), and the clustered set (bf16-rounded: 40 centres
    x 8 noisy copies + 16 exact duplicates -- equal ``sim`` bits and equal objectives, so the tie rule decides, and many
    objectives within rounding of each other, so the canonical arithmetic decides)."""
    from oracle import search as orc
    from tests import mmr_cases
    raw, which, q = mmr_cases.clustered(dim=dim)
    rng = np.random.default_rng(11)
    cq = np.stack([q, raw[5] + raw[77], rng.standard_normal(dim).astype(np.float32)])
    return (("random", mmr_cases.random_rows(2000, dim, seed=3, bf16=False), mmr_cases.random_rows(2, dim, seed=4, bf16=False)),
            ("clustered", orc.preprocess(raw, to_bf16=True), orc.preprocess(cq[:2], to_bf16=True)))


@pytest.mark.parametrize("c", [1, 7, 64, 100, 256, 1024])
def test_mmr_select_equals_the_restatement(gpu, c):
    """C x k x diversity on both sets at dim 768 (C = 1024 of the 336-row clustered set: lists with trailing padding, and k
    larger than the real candidates)."""
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from tests import mmr_cases
    for name, corpus, queries in _sets(768):
        scores, rows, vecs = mmr_cases.candidate_lists(corpus, queries, c)
        for d in (0.0, 0.25, 0.5, 1.0):
            want = mmr_cases.mmr_select(scores, rows, vecs, c, d)
            for k in sorted({k for k in (1, 10, 100, c) if k <= c}):
                _assert_equal(_device_select(torch, ffi, scores, rows, vecs, k, d), want, k, f"{name} C={c} k={k} diversity={d}")
            if d == 0.0:
                real = int((rows[0] >= 0).sum())
                assert want[0][0, :real].tolist() == list(range(real))           # diversity 0: the candidates unchanged


@pytest.mark.parametrize("dim", [384, 1024, 1536])
def test_mmr_select_other_dims(gpu, dim):
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from tests import mmr_cases
    for name, corpus, queries in _sets(dim):
        scores, rows, vecs = mmr_cases.candidate_lists(corpus, queries, 64)
        want = mmr_cases.mmr_select(scores, rows, vecs, 64, 0.5)
        for k in (10, 64):
            _assert_equal(_device_select(torch, ffi, scores, rows, vecs, k, 0.5), want, k, f"{name} dim={dim} k={k}")


@pytest.mark.parametrize("nq", [1, 3, 64, 65])
def test_mmr_select_batch_sizes_and_the_feature_does_something(gpu, nq):
    """The clustered set at diversity 0.5, k = 10, C = 64, for 1 / 3 / 64 / 65 queries; query 0 mixes four centres: its picks
    differ from the plain top-10 and name more distinct centres than it does."""
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from oracle import search as orc
    from tests import mmr_cases
    raw, which, q = mmr_cases.clustered(dim=768)
    rng = np.random.default_rng(nq)
    qs = np.concatenate([q[None], raw[rng.integers(0, len(raw), nq - 1)] + 0.5 * raw[rng.integers(0, len(raw), nq - 1)]]) if nq > 1 else q[None]
    corpus = orc.preprocess(raw, to_bf16=True)
    scores, rows, vecs = mmr_cases.candidate_lists(corpus, orc.preprocess(qs, to_bf16=True), 64)
    want = mmr_cases.mmr_select(scores, rows, vecs, 10, 0.5)
    got = _device_select(torch, ffi, scores, rows, vecs, 10, 0.5)
    _assert_equal(got, want, 10, f"clustered nq={nq}")
    plain, picked = rows[0, :10], got[1][0]
    assert picked.tolist() != plain.tolist()
    assert len(set(which[picked])) > len(set(which[plain])), (sorted(set(which[picked])), sorted(set(which[plain])))


def test_mmr_select_padding_and_neighbouring_buffers(gpu):
    """Lists with trailing padding, an all-padding list, k larger than the real candidates: the slots behind a query's picks hold
    (-1, -1, -inf, -inf); nq = 3 inside buffers sized for 5: the neighbours' slots keep their sentinels."""
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from oracle import search as orc
    from tests import mmr_cases
    raw, which, q = mmr_cases.clustered(dim=768)
    corpus = orc.preprocess(raw, to_bf16=True)
    qs = orc.preprocess(np.stack([q, raw[1], raw[2]]), to_bf16=True)
    c, k = 32, 12
    scores, rows, vecs = mmr_cases.candidate_lists(corpus, qs, c)
    scores[0, 5:], rows[0, 5:], vecs[0, 5:] = -np.inf, -1, 0           # 5 real candidates < k
    scores[1, :], rows[1, :], vecs[1, :] = -np.inf, -1, 0              # all padding
    want = mmr_cases.mmr_select(scores, rows, vecs, k, 0.5)
    assert want[0][0, 5:].tolist() == [-1] * 7 and want[0][1].tolist() == [-1] * k and (want[0][2] >= 0).all()
    dev = "cuda:0"
    big_s = torch.full((5, c), 3.0, dtype=torch.float32, device=dev)
    big_r = torch.full((5, c), 12345, dtype=torch.int64, device=dev)
    big_v = torch.full((5, c, 768), 0.25, dtype=torch.float32, device=dev)
    big_s[1:4], big_r[1:4], big_v[1:4] = torch.from_numpy(scores).to(dev), torch.from_numpy(rows).to(dev), torch.from_numpy(vecs).to(dev)
    outs = [torch.full((5, k), -77, dtype=t, device=dev) for t in (torch.int32, torch.int64, torch.float32, torch.float32)]
    ffi.mmr_select(big_s[1:4], big_r[1:4], big_v[1:4], k, 0.5, out_pos=outs[0][1:4], out_rows=outs[1][1:4], out_scores=outs[2][1:4],
                   out_obj=outs[3][1:4])
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in outs]
    _assert_equal([h[1:4] for h in host], want, k, "padding")
    for h in host:
        assert (h[0] == -77).all() and (h[4] == -77).all()
    assert np.isneginf(host[2][1, 5:]).all() and np.isneginf(host[3][2]).all()


def test_invalid_arguments_are_refused_and_launch_nothing(gpu):
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    dev = "cuda:0"
    s = torch.zeros((2, 8), dtype=torch.float32, device=dev)
    r = torch.zeros((2, 8), dtype=torch.int64, device=dev)
    v = torch.zeros((2, 8, 768), dtype=torch.float32, device=dev)
    outs = dict(out_pos=torch.full((2, 4), -77, dtype=torch.int32, device=dev), out_rows=torch.full((2, 4), -77, dtype=torch.int64, device=dev),
                out_scores=torch.full((2, 4), -77.0, dtype=torch.float32, device=dev), out_obj=torch.full((2, 4), -77.0, dtype=torch.float32, device=dev))
    for d in (-0.01, 1.01, float("nan"), float("inf")):
        with pytest.raises(ffi.NativeError, match="diversity") as e:
            ffi.mmr_select(s, r, v, 4, d, **outs)
        assert e.value.code == ffi.E_INVALID
    for k in (0, 9):
        with pytest.raises(ffi.NativeError) as e:
            ffi.mmr_select(s, r, v, k, 0.5)
        assert e.value.code == ffi.E_INVALID and "k=" in str(e.value)
    with pytest.raises(ffi.NativeError, match="dim") as e:
        ffi.mmr_select(s, r, torch.zeros((2, 8, 100), dtype=torch.float32, device=dev), 4, 0.5, **outs)
    assert e.value.code == ffi.E_INVALID
    with pytest.raises(ffi.NativeError, match="float32"):
        ffi.mmr_select(s.double(), r, v, 4, 0.5)
    with pytest.raises(ffi.NativeError, match="shape"):
        ffi.mmr_select(s, r[:, :7].contiguous(), v, 4, 0.5)
    torch.cuda.synchronize()
    assert all(bool((o == -77).all()) for o in outs.values())


# ------------------------------------------------------------------ end to end through the store
def test_store_search_with_diversity_on_one_and_two_shards(gpu):
    """``search`` / ``search_batch`` with ``diversity`` return, on 1 and 2 local shards, the same hits -- those of the restatement
    run on ``read_rows`` of the candidates; ``diversity=None`` returns what a plain search of the same limit returns."""
    import coderag_amd  # noqa: F401
    from coderag_amd.store import HipVectorStore
    from tests import mmr_cases
    raw, which, q = mmr_cases.clustered(dim=768)
    n = len(raw)
    ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(n)]
    payloads = [{"file_path": f"/proj/f{i % 9}.py", "entity_type": "function", "entity_name": f"ent{i}", "language": ("python", "go")[i % 2],
                 "start_line": i, "end_line": i + 3, "content": f"def ent{i}(): pass", "graph_node_id": f"mod.ent{i}", "content_hash": "h",
                 "project_name": "p1"} for i in range(n)]
    qs = np.stack([q, raw[5] + raw[77], raw[200]])

    def pairs(hits):
        return [(h["id"], h["score"]) for h in hits]

    async def run(shards):
        async with HipVectorStore(dim=768, dtype="bf16", initial_capacity=4096, device=0, shards=shards, compact_dead_fraction=0.0) as s:
            await s.create_collections()
            for a in range(0, n, 84):                                       # four appends: the blocks go round the shards
                await s.upsert("code_chunks", ids[a:a + 84], raw[a:a + 84], payloads[a:a + 84])
            col = s._col("code_chunks")
            assert all(r > 0 for r in col.shards.rows)
            sh, lo = col.rows_of(np.arange(n))
            stored = {t: col.shards.index[t].read_rows(0, col.shards.rows[t]) for t in range(shards)}
            vec_of = {ids[i]: stored[int(sh[i])][int(lo[i])] for i in range(n)}

            def expected(cand, limit, c, d):
                scores, rows = np.full((1, c), -np.inf, np.float32), np.full((1, c), -1, np.int64)
                vecs = np.zeros((1, c, 768), np.float32)
                for i, h in enumerate(cand[:c]):
                    scores[0, i], rows[0, i], vecs[0, i] = h["score"], i, vec_of[h["id"]]
                pos, _, sc, _ = mmr_cases.mmr_select(scores, rows, vecs, limit, d)
                return [(cand[p]["id"], float(v)) for p, v in zip(pos[0], sc[0]) if p >= 0]

            out = {}
            plain = await s.search("code_chunks", q.tolist(), limit=64)
            out["none"] = pairs(await s.search("code_chunks", q.tolist(), limit=10, diversity=None))
            assert out["none"] == pairs(plain[:10]) == pairs(await s.search("code_chunks", q.tolist(), limit=10))
            assert pairs(await s.search("code_chunks", q.tolist(), limit=10, diversity=0.0, candidates=64)) == pairs(plain[:10])
            got = await s.search("code_chunks", q.tolist(), limit=10, diversity=0.5, candidates=64)
            assert pairs(got) == expected(plain, 10, 64, 0.5) and pairs(got) != pairs(plain[:10])
            centre = {ids[i]: which[i] for i in range(n)}
            assert len({centre[h["id"]] for h in got}) > len({centre[h["id"]] for h in plain[:10]})
            assert all(set(h) == {"id", "score", "payload"} and h["payload"]["entity_name"] == f"ent{int(h['id'][-12:])}" for h in got)
            out["mmr"] = pairs(got)
            # default candidates (4 x limit), a filter and an exclusion with it
            want = [h for h in await s.search("code_chunks", q.tolist(), limit=336, filters={"language": "go"}, must_not={"file_path": "/proj/f3.py"})]
            assert all(h["payload"]["language"] == "go" and h["payload"]["file_path"] != "/proj/f3.py" for h in want)
            got = await s.search("code_chunks", q.tolist(), limit=6, filters={"language": "go"}, must_not={"file_path": "/proj/f3.py"}, diversity=0.3)
            assert pairs(got) == expected(want, 6, 24, 0.3)
            out["filtered"] = pairs(got)
            batch = await s.search_batch("code_chunks", qs, limit=10, diversity=0.5, candidates=40)
            for qi in range(3):
                assert pairs(batch[qi]) == expected(await s.search("code_chunks", qs[qi].tolist(), limit=40), 10, 40, 0.5), qi
            out["batch"] = [pairs(b) for b in batch]
            # coalesced callers with equal (diversity, candidates) share a pass and keep their own prefix
            before = s.search_passes
            a, b, c = await asyncio.gather(s.search("code_chunks", q.tolist(), limit=4, diversity=0.5, candidates=64),
                                           s.search("code_chunks", q.tolist(), limit=10, diversity=0.5, candidates=64),
                                           s.search("code_chunks", q.tolist(), limit=10))
            assert s.search_passes - before == 2 and pairs(a) == out["mmr"][:4] and pairs(b) == out["mmr"] and pairs(c) == out["none"]
            return out

    one, two = asyncio.run(run(1)), asyncio.run(run(2))
    # Points with IDENTICAL stored vectors tie in score and in objective; among them the lower row wins, and a row's number
    # depends on the sharding (shard * 2^32 + local row).  So the two runs agree on every score and on WHICH VECTOR each hit
    # is, not on which of several identical points carries it: ids are compared through the first point with the same stored row.
    from oracle import search as orc
    stored = orc.preprocess(raw, to_bf16=True)
    first = {}
    canon = {ids[i]: first.setdefault(stored[i].tobytes(), i) for i in range(n)}

    def norm(v):
        return [norm(x) for x in v] if isinstance(v, list) else (canon[v[0]], v[1])
    assert {k: norm(v) for k, v in one.items()} == {k: norm(v) for k, v in two.items()}
