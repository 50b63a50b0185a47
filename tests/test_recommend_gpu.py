"""Recommend by example on the device: ``crh_recommend_query`` / ``crh_recommend_select`` against the CPU restatement
(tests/recommend_cases.py), every output bit for bit; the recomputed score of every list entry against the score a real search
returned; and ``HipVectorStore.recommend_batch`` end to end against the brute force over every row's oracle score (``oracle.search``
with ``k`` = all rows on ``read_rows`` of the whole collection).  No tolerance appears anywhere."""
import asyncio

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U32, F32 = np.uint32, np.float32
NAMES = ("rows", "score", "neg", "best", "info")


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(U32)


def _assert_equal(got, want, k, what):
    for g, w, name in zip(got, want, NAMES):
        w = w if name == "info" else w[:, :k]
        if name in ("score", "neg"):
            bad = np.flatnonzero((_bits(g) != _bits(w)).any(1)) if g.size else []
            assert len(bad) == 0, f"{what}: {name} bits differ at query {bad[:4]}\n{g[bad[:1]]}\n{w[bad[:1]]}"
        else:
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f"{what}: {name} differ\n{g}\n{w}"


# ------------------------------------------------------------------ the two kernels against the restatement
@pytest.mark.parametrize("c", [1, 7, 64, 128])
@pytest.mark.parametrize("P,N", [(1, 0), (1, 1), (2, 8), (8, 0), (8, 8)])
@pytest.mark.parametrize("dim", [384, 768, 1536])
def test_kernels_equal_the_restatement(gpu, dim, P, N, c):
    """Real lists of a clustered corpus (tests/recommend_cases.case): padding, lists sharing rows, a negative ON a positive
    (``p == n`` exactly), ragged live counts, shard bits; the bf16 rounding of the examples on every other shape."""
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from tests import recommend_cases as rc
    assert P * c <= ffi.MAX_K
    bf16 = bool((P + N + c) & 1)
    launches = 0
    for nq in (0, 1, 3, 65):
        cs = rc.case(nq, P, N, c, dim, seed=dim + 100 * P + 10 * N + c + nq, bf16=bf16, ragged=nq != 1)
        dev = {k: torch.from_numpy(v).cuda() for k, v in cs.items() if k in ("scores", "rows", "cand_vecs", "examples", "example_rows", "avg_scores", "avg_rows")}
        counts = {"n_pos": cs["n_pos"], "n_neg": cs["n_neg"]} if nq != 1 else {}
        what = f"dim={dim} P={P} N={N} c={c} nq={nq} bf16={bf16}"
        q = ffi.recommend_query(dev["examples"], P, N, **counts)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(q.cpu().numpy()), _bits(cs["avg_query"])), f"{what}: the average query differs"
        want = rc.recommend_select(cs["scores"], cs["rows"], cs["cand_vecs"], cs["examples"], cs["example_rows"], P, N, P * c, "best", bf16, **counts)
        for k in sorted({1, min(10, P * c), P * c}):
            out = ffi.recommend_select(dev["scores"], dev["rows"], dev["cand_vecs"], dev["examples"], dev["example_rows"], P, N, k, "best", bf16, **counts)
            torch.cuda.synchronize()
            launches += 1
            _assert_equal([o.cpu().numpy() for o in out], want, k, f"{what} k={k}")
        want = rc.recommend_select(cs["avg_scores"], cs["avg_rows"], None, None, cs["example_rows"], P, N, c, "average", **counts)
        for k in sorted({1, c}):
            out = ffi.recommend_select(dev["avg_scores"], dev["avg_rows"], None, None, dev["example_rows"], P, N, k, "average", **counts)
            torch.cuda.synchronize()
            _assert_equal([o.cpu().numpy() for o in out], want, k, f"{what} average k={k}")
    assert launches == 4 * len({1, min(10, P * c), P * c})


def test_select_inside_larger_buffers_and_refused_arguments(gpu):
    """nq = 3 inside buffers sized for 5: the neighbours' slots keep their sentinels; refused arguments launch nothing."""
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from tests import recommend_cases as rc
    L = ffi.lib()
    P, N, c, k, dim = 3, 2, 20, 12, 384
    cs = rc.case(3, P, N, c, dim, seed=5)
    want = rc.recommend_select(cs["scores"], cs["rows"], cs["cand_vecs"], cs["examples"], cs["example_rows"], P, N, k, "best", False, cs["n_pos"], cs["n_neg"])
    ins = [torch.from_numpy(cs[name]).cuda() for name in ("scores", "rows", "cand_vecs", "examples", "example_rows")]
    outs = [torch.full((5, k), -77, dtype=t, device="cuda:0") for t in (torch.int64, torch.float32, torch.float32, torch.int32)]
    info = torch.full((5, 4), -77, dtype=torch.int32, device="cuda:0")
    qout = torch.full((5, dim), -77, dtype=torch.float32, device="cuda:0")
    ptr = [int(o[1:4].data_ptr()) for o in outs] + [int(info[1:4].data_ptr())]
    inp = [int(t.data_ptr()) for t in ins]
    cnt = [cs["n_pos"].ctypes.data, cs["n_neg"].ctypes.data]
    assert L.crh_recommend_select(3, P, N, c, k, dim, ffi.RECOMMEND_BEST, 0, *inp, *cnt, *ptr, None) == ffi.OK
    assert L.crh_recommend_query(3, P, N, dim, inp[3], *cnt, int(qout[1:4].data_ptr()), None) == ffi.OK
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in outs] + [info.cpu().numpy()]
    _assert_equal([h[1:4] for h in host], want, k, "inside larger buffers")
    assert all((h[0] == -77).all() and (h[4] == -77).all() for h in host)
    qh = qout.cpu().numpy()
    assert np.array_equal(_bits(qh[1:4]), _bits(cs["avg_query"])) and (qh[0] == -77).all() and (qh[4] == -77).all()
    for o in outs + [info, qout]:
        o.fill_(-77)
    bad_pos, bad_neg = np.asarray([1, 4, 1], np.int32), np.asarray([0, 0, 3], np.int32)
    for nq_, P_, N_, c_, k_, dim_, method, bf, cp, cn in ((3, 0, N, c, k, dim, 1, 0, None, None), (3, 9, N, c, k, dim, 1, 0, None, None),
                                                          (3, P, 9, c, k, dim, 1, 0, None, None), (3, P, -1, c, k, dim, 1, 0, None, None),
                                                          (3, P, N, 342, k, dim, 1, 0, None, None), (3, P, N, 0, k, dim, 1, 0, None, None),
                                                          (3, P, N, c, 0, dim, 1, 0, None, None), (3, P, N, c, P * c + 1, dim, 1, 0, None, None),
                                                          (3, P, N, c, c + 1, dim, 0, 0, None, None), (3, P, N, c, k, 512, 1, 0, None, None),
                                                          (3, P, N, c, k, dim, 2, 0, None, None), (3, P, N, c, k, dim, 1, 2, None, None),
                                                          (-1, P, N, c, k, dim, 1, 0, None, None), (3, P, N, c, k, dim, 1, 0, bad_pos, None),
                                                          (3, P, N, c, k, dim, 1, 0, None, bad_neg)):
        rc_ = L.crh_recommend_select(nq_, P_, N_, c_, k_, dim_, method, bf, *inp, None if cp is None else cp.ctypes.data,
                                     None if cn is None else cn.ctypes.data, *ptr, None)
        assert rc_ == ffi.E_INVALID, (nq_, P_, N_, c_, k_, dim_, method, bf)
    for nq_, P_, N_, dim_, cp, cn in ((3, 0, N, dim, None, None), (3, P, 9, dim, None, None), (3, P, N, 100, None, None), (-1, P, N, dim, None, None),
                                      (3, P, N, dim, bad_pos, None), (3, P, N, dim, None, bad_neg)):
        rc_ = L.crh_recommend_query(nq_, P_, N_, dim_, inp[3], None if cp is None else cp.ctypes.data, None if cn is None else cn.ctypes.data,
                                    int(qout[1:4].data_ptr()), None)
        assert rc_ == ffi.E_INVALID, (nq_, P_, N_, dim_)
    with pytest.raises(ffi.NativeError, match="int64"):
        ffi.recommend_select(ins[0], ins[1].int(), ins[2], ins[3], ins[4], P, N, k)
    with pytest.raises(ffi.NativeError, match="shape"):
        ffi.recommend_select(ins[0], ins[1], ins[2][:, :7].contiguous(), ins[3], ins[4], P, N, k)
    with pytest.raises(ValueError):
        ffi.recommend_select(ins[0], ins[1], ins[2], ins[3], ins[4], P, N, k, "worst")
    torch.cuda.synchronize()
    assert all((o.cpu().numpy() == -77).all() for o in outs + [info, qout])


# ------------------------------------------------------------------ end to end through the store
def _payloads(n):
    return [{"file_path": f"/proj/f{i % 9}.py", "entity_type": "function", "entity_name": f"ent{i}", "language": ("python", "go", "rust")[i % 3],
             "start_line": i, "end_line": i + 3, "content": f"def ent{i}(): pass", "graph_node_id": f"mod.ent{i}", "content_hash": "h",
             "project_name": "p1"} for i in range(n)]


def _quads(hits):
    return [(h["id"], _bits(h["score"]).item(), _bits(h.get("negative_score", -np.inf)).item(), h.get("matched_positive")) for h in hits]


@pytest.mark.parametrize("dtype_name,shards,filtered", [("bf16", 1, False), ("f32", 1, True), ("bf16", 2, False), ("f32", 2, False)])
def test_store_recommend_equals_the_brute_force(gpu, dtype_name, shards, filtered):
    """3 000 clustered rows (60 exact copies), the two batches of tests/recommend_cases.e2e_inputs under both strategies: ids,
    score bits, ``negative_score`` bits and ``matched_positive`` of the brute force; a short list is the brute force's prefix
    of its own length -- the length the rounds on the oracle's own lists give; and for every entry of a real search's list
    the recomputed ``s(pos_j, x)`` is the list's score, bit for bit."""
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from coderag_amd.shards import STRIDE
    from coderag_amd.store import HipVectorStore
    from oracle import search as orc
    from tests import recommend_cases as rc
    raw, batches = rc.e2e_inputs()
    n = len(raw)
    ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(n)]
    bf16 = dtype_name == "bf16"

    async def run():
        async with HipVectorStore(dim=raw.shape[1], dtype=dtype_name, initial_capacity=4096, device=0, shards=shards, compact_dead_fraction=0.0) as s:
            await s.create_collections()
            step = (n + 3) // 4
            pay = _payloads(n)
            for a in range(0, n, step):
                await s.upsert("code_chunks", ids[a:a + step], raw[a:a + step], pay[a:a + step])
            col = s._col("code_chunks")
            sh, lo = col.rows_of(np.arange(n))
            per = {t: col.shards.index[t].read_rows(0, col.shards.rows[t]) for t in range(shards)}
            stored = np.stack([per[int(sh[i])][int(lo[i])] for i in range(n)])
            gid = np.asarray(sh, np.int64) * STRIDE + np.asarray(lo, np.int64)
            order = np.argsort(gid)                                       # the order ties follow
            inv = np.empty(n, np.int64)
            inv[order] = np.arange(n)
            kw = {"filters": {"language": ["python", "rust"]}} if filtered else {}
            passing = (np.arange(n) % 3 != 1)[order] if filtered else None
            asked = full = 0
            for limit, sets in batches:
                named = [([ids[i] for i in p], [ids[i] for i in ng]) for p, ng in sets]
                batch_p = max(len(p) for p, _ in sets)
                for strategy in ("average", "best"):
                    got = await s.recommend_batch("code_chunks", named, limit=limit, strategy=strategy, **kw)
                    assert len(got) == len(sets)
                    for (p, ng), hits in zip(sets, got):
                        what = f"{dtype_name} shards={shards} filtered={filtered} {strategy} limit={limit} pos={p} neg={ng}"
                        bf = rc.brute_force(stored[order], inv[p], inv[ng], limit, strategy, bf16, passing)
                        want = [(ids[order[r]], sb, nb, ids[p[b]] if strategy == "best" else None) for r, sb, nb, b in bf]
                        if strategy == "best":
                            expect_len = len(rc.rounds(stored[order], inv[p], inv[ng], limit, bf16, passing, batch_p=batch_p)[0])
                            asked += 1
                            full += int(len(hits) == limit)
                        else:
                            expect_len = len(want)
                        assert len(hits) == expect_len and _quads(hits) == want[:expect_len], what
                        assert not {h["id"] for h in hits} & {ids[i] for i in p + ng}
            assert col.recommend_rounds["round2"] >= 1 and col.recommend_rounds["short"] >= 1 and 2 * full >= asked, (col.recommend_rounds, full, asked)
            # the list-score check: a real search's lists, the recomputed s(pos_j, x) of every entry
            pos = [100, 101, 1000, 5]
            ex_rows = gid[pos][None]
            dev = torch.device("cuda", 0)
            examples = col.shards._gather_everywhere(torch.from_numpy(ex_rows).to(dev), 0)
            cs, cr = col.shards.search_device(examples[0], 64, col.device_filters(kw.get("filters"), None))
            torch.cuda.synchronize()
            cs, cr = cs.cpu().numpy(), cr.cpu().numpy()
            assert (cr >= 0).all()
            slot_of_gid = {int(g): i for i, g in enumerate(gid)}
            for j in range(len(pos)):
                x = stored[[slot_of_gid[int(g)] for g in cr[j]]]
                assert np.array_equal(_bits(rc.example_scores(stored[pos[j]][None], x, bf16)[0]), _bits(cs[j])), f"list {j}"
            # and the device's own recomputation: one list per query, no negatives -- out_score is the list's score
            vecs = col.shards._gather_everywhere(torch.from_numpy(cr).to(dev), 0)
            out = ffi.recommend_select(torch.from_numpy(cs[:, None]).to(dev), torch.from_numpy(cr[:, None]).to(dev), vecs,
                                       examples[0][:, None].contiguous(), torch.from_numpy(np.ascontiguousarray(ex_rows.T)).to(dev), 1, 0, 64, "best", bf16)
            torch.cuda.synchronize()
            rows, score = out[0].cpu().numpy(), out[1].cpu().numpy()
            for j in range(len(pos)):
                keep = cr[j] != ex_rows[0, j]
                assert np.array_equal(rows[j, :keep.sum()], cr[j][keep]) and np.array_equal(_bits(score[j, :keep.sum()]), _bits(cs[j][keep]))

    asyncio.run(run())
