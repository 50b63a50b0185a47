"""Exact per-group cap on the device: ``crh_group_select`` against the CPU restatement (tests/group_cases.py), bit for bit --
positions, rows, score bits, codes and ``out_info``; ``crh_index_gather_codes`` against the codes that were appended; and
``HipVectorStore.search(group_by=...)`` / ``search_groups`` / ``find_similar_code(max_per_file=...)`` end to end against the
brute-force definition run with ``oracle.search`` on ``read_rows`` of the whole collection.  No tolerance appears anywhere.

The restatement's ``k``-output result is the prefix of its ``c``-output result (tests/test_grouped_host.py pins that): the
sweeps run it once per list at ``k = c`` and compare every ``k`` of the device against that prefix."""
import asyncio

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U32 = np.uint32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(U32)


def _lists(nq, c, mode, seed):
    """nq candidate lists of c entries: scores descending with runs of equal values, distinct rows, padded tails of random
    length (every fifth list all padding when there are enough of them), codes by ``mode``."""
    rng = np.random.default_rng(seed)
    scores = -np.sort(-np.round(rng.standard_normal((nq, c)), 1).astype(np.float32), axis=1)
    rows = (rng.permuted(np.tile(np.arange(4 * c, dtype=np.int64), (nq, 1)), axis=1)[:, :c] + (rng.integers(0, 3, (nq, 1)) << 32)) if nq else np.zeros((0, c), np.int64)
    real = rng.integers(0, c + 1, nq)
    real[::3] = c                                                     # (full lists too)
    if nq >= 5:
        real[4::5] = 0
    pad = np.arange(c)[None, :] >= real[:, None]
    if mode == "equal":
        codes = np.full((nq, c), 7, np.int32)
    elif mode == "distinct":
        codes = np.tile(np.arange(c, dtype=np.int32), (nq, 1))
    elif mode == "none":
        codes = np.full((nq, c), -1, np.int32)
    else:                                                             # a few groups of very different sizes, some rows in none
        codes = np.minimum(rng.geometric(0.15, (nq, c)), 40).astype(np.int32) - 2
    scores[pad], rows[pad] = -np.inf, -1
    codes[pad] = rng.integers(-1, 5, int(pad.sum())).astype(np.int32)  # (whatever a gather left there: never looked at)
    return scores, rows, codes


def _device_select(torch, ffi, scores, rows, codes, k, group_size):
    out = ffi.group_select(torch.from_numpy(scores).cuda(), torch.from_numpy(rows).cuda(), torch.from_numpy(codes).cuda(), k, group_size)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _assert_equal(got, want, k, what):
    for g, w, name in zip(got, want, ("pos", "rows", "scores", "codes", "info")):
        w = w if name == "info" else w[:, :k]
        if name == "scores":
            assert np.array_equal(_bits(g), _bits(w)), f"{what}: score bits differ"
        else:
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f"{what}: {name} differ\n{g}\n{w}"


# ------------------------------------------------------------------ crh_group_select against the restatement
@pytest.mark.parametrize("c", [1, 7, 64, 100, 1000, 1024])
def test_group_select_equals_the_restatement(gpu, c):
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from tests import group_cases
    for nq in (0, 1, 64, 200):
        for mode in ("mixed", "equal", "distinct", "none"):
            if nq == 200 and mode != "mixed":
                continue
            scores, rows, codes = _lists(nq, c, mode, seed=c * 1000 + nq)
            for group_size in sorted({1, 3, c}):
                want = group_cases.group_select(scores, rows, codes, c, group_size)
                for k in sorted({1, c}):
                    got = _device_select(torch, ffi, scores, rows, codes, k, group_size)
                    _assert_equal(got, want, k, f"c={c} nq={nq} {mode} S={group_size} k={k}")
                if group_size == c and nq:                              # S >= c: the candidates unchanged
                    real = rows >= 0
                    assert np.array_equal(got[1], np.where(real, rows, -1)) and np.array_equal(got[4][:, 0], real.sum(1))


def test_group_select_neighbouring_buffers_and_arguments(gpu):
    """nq = 3 inside buffers sized for 5: the neighbours' slots keep their sentinels; refused arguments launch nothing."""
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from tests import group_cases
    L = ffi.lib()
    c, k = 100, 12
    scores, rows, codes = _lists(3, c, "mixed", seed=5)
    want = group_cases.group_select(scores, rows, codes, k, 2)
    dev = "cuda:0"
    ins = [torch.from_numpy(a).to(dev) for a in (scores, rows, codes)]
    outs = [torch.full((5, k), -77, dtype=t, device=dev) for t in (torch.int32, torch.int64, torch.float32, torch.int32)]
    info = torch.full((5, 2), -77, dtype=torch.int32, device=dev)
    ptr = [int(o[1:4].data_ptr()) for o in outs] + [int(info[1:4].data_ptr())]
    assert L.crh_group_select(3, c, k, 2, *(int(t.data_ptr()) for t in ins), *ptr, None) == ffi.OK
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in outs] + [info.cpu().numpy()]
    _assert_equal([h[1:4] for h in host], want, k, "inside larger buffers")
    assert all((h[0] == -77).all() and (h[4] == -77).all() for h in host)
    for bad in ((3, c, 0, 2), (3, c, c + 1, 2), (3, c, k, 0), (-1, c, k, 2)):
        assert L.crh_group_select(*bad, *(int(t.data_ptr()) for t in ins), *ptr, None) == ffi.E_INVALID
    with pytest.raises(ffi.NativeError, match="int32"):
        ffi.group_select(ins[0], ins[1], ins[2].long(), k, 2)
    with pytest.raises(ffi.NativeError, match="shape"):
        ffi.group_select(ins[0], ins[1][:, :7].contiguous(), ins[2], 4, 2)
    torch.cuda.synchronize()
    assert all((o[0].cpu().numpy() == -77).all() for o in outs)


# ------------------------------------------------------------------ crh_index_gather_codes
@pytest.mark.parametrize("dtype_name", ["f32", "bf16"])
def test_gather_codes_equals_the_appended_codes(gpu, dtype_name):
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    rng = np.random.default_rng(3)
    n, ncols = 2200, 3
    x = rng.standard_normal((n, 384)).astype(np.float32)
    codes = rng.integers(-1, 50, (n, ncols)).astype(np.int32)
    idx = ffi.Index(384, ffi.DTYPE_BF16 if dtype_name == "bf16" else ffi.DTYPE_F32, capacity_rows=4096, n_code_cols=ncols, device=0)
    try:
        idx.append(x[:1500], codes[:1500])
        idx.append(x[1500:], codes[1500:])
        idx.tombstone(np.arange(0, n, 7, dtype=np.int64))                 # tombstoned rows still gather
        base = 5 << 32
        local = np.concatenate([rng.integers(0, n, 500), [0, n - 1, 31, 32, 1499, 1500]])
        rows = local + base
        rows[5::7] = -1                                                  # padding
        rows[3::11] = local[3::11] + (4 << 32)                           # a lower shard's row
        rows[2::13] = local[2::13] + base + n                            # past this shard's end
        rows[4::17] = local[4::17]                                       # row_base 0's rows: below this shard's base
        rows = rows.reshape(2, -1)
        own = (rows >= base) & (rows < base + n)
        assert own.sum() > 200 and (~own).sum() > 100 and (local[own.reshape(-1)] % 7 == 0).any()
        rows_d = torch.from_numpy(rows).cuda()
        for col in range(ncols):
            for fill in (-1, 123):                                       # positions this index does not own are left untouched
                out = torch.full(rows.shape, fill, dtype=torch.int32, device="cuda:0")
                got = idx.gather_codes(rows_d, col, row_base=base, out=out)
                torch.cuda.synchronize()
                assert got is out and np.array_equal(got.cpu().numpy(), np.where(own, codes[np.clip(rows - base, 0, n - 1), col], fill))
        fresh = idx.gather_codes(rows_d, 1, row_base=base)               # allocated full of -1
        assert np.array_equal(fresh.cpu().numpy(), np.where(own, codes[np.clip(rows - base, 0, n - 1), 1], -1))
        for col in (-1, ncols):
            with pytest.raises(ffi.NativeError, match="column") as e:
                idx.gather_codes(rows_d, col, row_base=base)
            assert e.value.code == ffi.E_INVALID
        with pytest.raises(ffi.NativeError, match="device tensor"):
            idx.gather_codes(np.zeros((3,), np.int64), 0)
        with pytest.raises(ffi.NativeError, match="int64"):
            idx.gather_codes(torch.zeros((3,), dtype=torch.int32, device="cuda:0"), 0)
    finally:
        idx.close()


# ------------------------------------------------------------------ end to end through the store
def _payloads(which):
    return [{"file_path": f"/proj/f{int(w)}.py", "entity_type": "function", "entity_name": f"ent{i}", "language": ("python", "go")[i % 2],
             "start_line": i, "end_line": i + 3, "content": f"def ent{i}(): pass", "graph_node_id": f"mod.ent{i}", "content_hash": "h",
             "project_name": "p1"} for i, w in enumerate(which)]


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
def test_store_exactness_rounds_equal_the_brute_force(gpu, dtype_name, shards):
    """The three rounds corpora (limit 10 / group_size 3 / default candidates 40): ids and score bits of the brute force over
    ``oracle.search`` on ``read_rows``, and the rounds each corpus was built to need."""
    import coderag_amd  # noqa: F401
    from coderag_amd.store import HipVectorStore
    from oracle import search as orc
    from tests import group_cases

    async def run():
        for kind, want_round2, want_exclusion in (("exclusion", 1, 1), ("round2", 1, 0), ("round1", 0, 0)):
            raw, which, q = group_cases.rounds_corpus(kind, dim=768)
            ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(len(raw))]
            async with HipVectorStore(dim=768, dtype=dtype_name, initial_capacity=4096, device=0, shards=shards, compact_dead_fraction=0.0) as s:
                col, stored = await _filled(s, ids, raw, _payloads(which), shards)
                qp = orc.preprocess(q[None], to_bf16=(dtype_name == "bf16"))[0]
                got = await s.search("code_chunks", q.tolist(), limit=10, group_by="file_path", group_size=3)
                es, er = group_cases.brute_force(stored, qp, which, 10, 3)
                print(f"{kind} {dtype_name} shards={shards}: rounds {col.group_rounds}")
                assert _pairs(got) == [(ids[r], v.view(U32).item()) for v, r in zip(es, er)], kind
                assert col.group_rounds == {"queries": 1, "round2": want_round2, "exclusion": want_exclusion}, (kind, col.group_rounds)
                # with a filter and an exclusion of the caller's own on the grouped column, batched
                qs = np.stack([q, raw[7]])
                batch = await s.search_batch("code_chunks", qs, limit=10, filters={"language": "go"}, must_not={"file_path": "/proj/f5.py"},
                                             group_by="file_path", group_size=3)
                passing = (np.arange(len(raw)) % 2 == 1) & (which != 5)
                for qi in range(2):
                    es, er = group_cases.brute_force(stored, orc.preprocess(qs[qi][None], to_bf16=(dtype_name == "bf16"))[0], which, 10, 3, passing)
                    assert _pairs(batch[qi]) == [(ids[r], v.view(U32).item()) for v, r in zip(es, er)], (kind, qi)

    asyncio.run(run())


@pytest.mark.parametrize("shards", [1, 2])
def test_store_large_cap_groups_and_max_per_file(gpu, shards):
    """A cap larger than any file is the plain search bit for bit; ``search_groups`` is the brute-force grouping;
    ``find_similar_code(max_per_file=2)`` never returns three chunks of one file and still returns ``limit`` results."""
    import coderag_amd  # noqa: F401
    from coderag_amd.store import HipVectorStore
    from coderag_amd.vector_search import VectorSearcher
    from tests import group_cases
    raw, which, q = group_cases.rounds_corpus("round2", dim=768)
    n = len(raw)
    ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(n)]

    class Emb:
        async def embed(self, text):
            return q.tolist()

    async def run():
        async with HipVectorStore(dim=768, dtype="bf16", initial_capacity=4096, device=0, shards=shards, compact_dead_fraction=0.0) as s:
            await _filled(s, ids, raw, _payloads(which), shards)
            plain = await s.search("code_chunks", q.tolist(), limit=100)
            assert len({h["payload"]["file_path"] for h in plain}) == 1                      # the hot file owns the plain list
            assert _pairs(await s.search("code_chunks", q.tolist(), limit=100, group_by="file_path", group_size=5000, candidates=100)) == _pairs(plain)
            assert _pairs((await s.search_batch("code_chunks", q[None], limit=100, group_by="file_path", group_size=1200))[0]) == _pairs(plain)
            everything = await s.search("code_chunks", q.tolist(), limit=1024)
            assert len(everything) == 1024
            want = {}
            for h in everything:                                                             # 5 groups x 4 hits all lie inside the 1024 best
                f = h["payload"]["file_path"]
                if f in want or len(want) < 5:
                    want.setdefault(f, [])
                    if len(want[f]) < 4:
                        want[f].append((h["id"], np.float32(h["score"]).view(U32).item()))
            got = await s.search_groups("code_chunks", q.tolist(), "file_path", limit=5, group_size=4)
            assert [(g["id"], _pairs(g["hits"])) for g in got] == list(want.items()) and all(len(v) == 4 for v in want.values())
            vs = VectorSearcher(s, Emb())
            capped = await vs.find_similar_code("x = 1", limit=10, max_per_file=2)
            assert len(capped) == 10 and max(np.unique([h["file_path"] for h in capped], return_counts=True)[1]) == 2
            uncapped = await vs.find_similar_code("x = 1", limit=10)
            assert len({h["file_path"] for h in uncapped}) == 1

    asyncio.run(run())


def test_smoke_passes_with_its_grouped_line(gpu):
    import __graft_entry__ as entry
    line = entry._smoke_grouped()
    assert line.startswith("grouped:") and "bit-exact" in line
