"""Recommend by example above the device: the CPU restatement of ``crh_recommend_query`` / ``crh_recommend_select``
(tests/recommend_cases.py) and the properties DESIGN.md 3.17 states; the new C entries' export and argument checks; the store's
``recommend`` / ``recommend_batch`` on 1 and 2 local shards over a fake index with the two ``ffi`` calls replaced by the
restatement, against the brute force over every row's oracle score; the searcher's and the MCP tool's forwarding."""
import asyncio
import os
import re

import numpy as np
import pytest

from oracle import search as orc
from tests import fuse_cases, recommend_cases as rc
from tests.fake_index import fake_device
from tests.test_filter_sets_host import SetFakeIndex, _corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, F32 = np.uint32, np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(U32)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) if x.dtype == F32 else np.array_equal(x, y) for x, y in zip(a, b))


def _select(cs, k, strategy="best", **kw):
    return rc.recommend_select(cs["scores"], cs["rows"], cs["cand_vecs"], cs["examples"], cs["example_rows"], kw.pop("P"), kw.pop("N"), k,
                               strategy, cs["bf16"], cs["n_pos"], cs["n_neg"])


# ------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("P,N,c", [(1, 0, 7), (2, 3, 20), (4, 2, 64), (8, 8, 16)])
def test_restatement_prefixes_examples_ties_and_counts(P, N, c):
    cs = rc.case(9, P, N, c, 384, seed=P * 100 + N * 10 + c, bf16=bool(N & 1))
    full = _select(cs, P * c, P=P, N=N)
    for j in (1, 5, P * c):                                           # the first j outputs of a k-output call are the j-output call
        part = _select(cs, min(j, P * c), P=P, N=N)
        assert _same(part[:4], [a[:, :min(j, P * c)] for a in full[:4]]) and np.array_equal(part[4], full[4])
    rows, score, neg, best, info = full
    for q in range(9):
        kept, settled, distinct, vetoed = info[q].tolist()
        real = cs["rows"][q][cs["rows"][q] >= 0]
        assert distinct == np.unique(real).size and kept + vetoed == distinct and 0 <= settled <= kept
        got = rows[q, :kept]
        assert (got >= 0).all() and (rows[q, kept:] == -1).all() and np.isneginf(score[q, kept:]).all() and (best[q, kept:] == -1).all()
        assert not np.isin(got, cs["example_rows"][q]).any()           # the example rows are never returned
        key = fuse_cases.ord_f32(score[q, :kept]).astype(np.int64)     # descending in the ord order, ties to the lower row
        assert ((np.diff(key) < 0) | ((np.diff(key) == 0) & (np.diff(got) > 0))).all()
        assert (fuse_cases.ord_f32(score[q, :kept]) > fuse_cases.ord_f32(neg[q, :kept])).all()      # the veto is strict
        assert ((best[q, :kept] >= 0) & (best[q, :kept] < cs["n_pos"][q])).all()
        if not (cs["rows"][q, :, c - 1] >= 0).any():
            assert settled == kept                                    # no full list: everything is settled
    # the copies among the stored rows make equal scores: some query must show a tie broken by the row
    ties = sum(int((np.diff(_bits(score[q, :info[q, 0]]).astype(np.int64)) == 0).sum()) for q in range(9))
    assert ties > 0 or P * c < 20


def test_restatement_veto_is_strict_at_equality():
    """A negative ON a positive: every row that positive wins has ``p == n`` bit for bit and is vetoed; only the rows that
    another positive scores strictly higher survive."""
    raw, _ = rc.corpus(200, 384, seed=11)
    x = orc.preprocess(raw)
    pos, neg = [5, 60], [5]
    pre = orc.preprocess(x[pos])
    s, r = orc.search(x, pre, 50)
    ex = x[pos + neg][None]
    out = rc.recommend_select(s[None], r[None], x[r.reshape(-1)][None], ex, np.asarray([pos + neg]), 2, 1, 100)
    rows, score, nscore, best, info = (a[0] for a in out)
    mat = rc.example_scores(x[pos + neg], x)
    assert np.array_equal(_bits(mat[0]), _bits(mat[2]))
    won_by_0 = fuse_cases.ord_f32(mat[0]) >= fuse_cases.ord_f32(mat[1])
    kept = rows[rows >= 0]
    assert kept.size and not won_by_0[kept].any() and (best[:kept.size] == 1).all() and info[3] > 0
    cand = np.unique(r)
    assert set(kept.tolist()) == set(int(v) for v in cand if not won_by_0[v] and v not in pos)
    # one positive that is its own negative: nothing survives
    out = rc.recommend_select(s[None, :1], r[None, :1], x[r[0]][None], x[[5, 5]][None], np.asarray([[5, 5]]), 1, 1, 10)
    assert (out[0] == -1).all() and out[4][0].tolist() == [0, 0, 50, 50]


def test_restatement_best_without_negatives_is_the_max_fusion_minus_the_examples():
    raw, _ = rc.corpus(300, 384, seed=5)
    x = orc.preprocess(raw)
    seen_settled = 0
    for pos in ([3], [3, 299, 120], [7, 8, 9, 10, 11, 12, 13, 14]):
        P = len(pos)
        for c in (1, 10, 60):
            s, r = orc.search(x, orc.preprocess(x[pos]), c)
            got = rc.recommend_select(s[None], r[None], x[r.reshape(-1)][None], x[pos][None], np.asarray([pos]), P, 0, P * c)
            fr, ff, _, _, ffirst, _ = fuse_cases.fuse_select(s[None], r[None], P, P * c, "max")
            keep = (fr[0] >= 0) & ~np.isin(fr[0], pos)
            n = int(keep.sum())
            # (below T a row may score higher against a positive whose list does not reach it: only the settled prefix is the fusion's)
            st = int(got[4][0, 1])
            assert got[4][0, 0] == n and sorted(got[0][0, :n]) == sorted(fr[0][keep])
            assert np.array_equal(got[0][0, :st], fr[0][keep][:st]) and np.array_equal(_bits(got[1][0, :st]), _bits(ff[0][keep][:st]))
            seen_settled += st
            assert np.isneginf(got[2][0, :n]).all() and (got[0][0, n:] == -1).all()
            # the recomputed score of a list's own entry is the list's score, bit for bit
            mat = rc.example_scores(x[pos], x)
            for j in range(P):
                assert np.array_equal(_bits(mat[j, r[j]]), _bits(s[j]))
    assert seen_settled > 50


def test_restatement_average_query_and_selection():
    ex = np.asarray([[[1, 2, 3, 4], [3, 2, 1, 0], [9, 9, 9, 9], [1, 1, 1, 1], [0, 2, 0, 2]]], F32)
    q = rc.recommend_query(ex, 3, 2)
    sp, sn = F32(F32(1) + F32(3)) + F32(9), F32(1) + F32(0)
    ap = F32(sp / F32(3))
    assert _bits(q[0, 0]) == _bits(F32(F32(ap + ap) - F32(sn / F32(2))))
    q1 = rc.recommend_query(ex, 3, 2, [2], [0])
    assert np.array_equal(_bits(q1[0]), _bits((ex[0, 0] + ex[0, 1]) / F32(2)))
    cs = rc.case(6, 3, 2, 12, 384, seed=4)
    rows, score, neg, best, info = rc.recommend_select(cs["avg_scores"], cs["avg_rows"], None, None, cs["example_rows"], 3, 2, 12, "average",
                                                       n_pos=cs["n_pos"], n_neg=cs["n_neg"])
    for q in range(6):
        lr, ls = cs["avg_rows"][q, 0], cs["avg_scores"][q, 0]
        keep = (lr >= 0) & ~np.isin(lr, cs["example_rows"][q])
        n = int(keep.sum())
        assert np.array_equal(rows[q, :n], lr[keep]) and np.array_equal(_bits(score[q, :n]), _bits(ls[keep])) and (rows[q, n:] == -1).all()
        assert info[q].tolist() == [n, n, int((lr >= 0).sum()), int((lr >= 0).sum()) - n] and (best[q] == -1).all() and np.isneginf(neg[q]).all()


def test_settled_rows_are_a_prefix_of_the_brute_force():
    """The exactness argument on real lists: the settled rows of every depth are the first rows of the definition's answer."""
    raw, _ = rc.corpus(400, 384, seed=9)
    x = orc.preprocess(raw)
    rng = np.random.default_rng(0)
    seen_unsettled = 0
    for _ in range(6):
        pos, neg = rng.choice(380, 3, replace=False).tolist(), rng.choice(380, 2, replace=False).tolist()
        want = rc.brute_force(x, pos, neg, 400, "best")
        for c in (5, 40, 200):
            s, r = orc.search(x, orc.preprocess(x[pos]), c)
            rows, score, nscore, best, info = (a[0] for a in rc.recommend_select(s[None], r[None], x[r.reshape(-1)][None], x[pos + neg][None],
                                                                                 np.asarray([pos + neg]), 3, 2, 3 * c))
            settled = int(info[1])
            seen_unsettled += int(settled < info[0])
            got = [(int(a), int(b), int(d), int(e)) for a, b, d, e in zip(rows[:settled], _bits(score[:settled]), _bits(nscore[:settled]), best[:settled])]
            assert got == want[:settled], (pos, neg, c)
    assert seen_unsettled > 0


def test_end_to_end_inputs_need_round_2_and_come_back_short():
    """The inputs of the GPU tier's end-to-end test, checked with the brute force and the oracle's lists alone: some query needs
    round 2, some comes back short (one of them with a non-empty answer), every answer is the brute force's prefix, and at
    least half return a full ``limit``.  The kernel sweep's inputs hold padding, vetoed rows and unsettled rows."""
    raw, batches = rc.e2e_inputs()
    for bf16, filtered in ((True, False), (False, True)):
        x = orc.preprocess(raw, to_bf16=bf16)
        passing = (np.arange(len(x)) % 3 != 1) if filtered else None
        asked = full = round2 = short = short_rows = 0
        for limit, sets in batches:
            batch_p = max(len(p) for p, _ in sets)
            for pos, neg in sets:
                ans, r2, sh = rc.rounds(x, pos, neg, limit, bf16, passing, batch_p=batch_p)
                assert ans == rc.brute_force(x, pos, neg, limit, "best", bf16, passing)[:len(ans)]
                asked, full, round2, short = asked + 1, full + int(len(ans) == limit), round2 + int(r2), short + int(sh)
                short_rows += len(ans) if sh else 0
        assert round2 >= 1 and short >= 2 and short_rows > 0 and 2 * full >= asked, (round2, short, short_rows, full, asked)
    for P, N, c in ((2, 8, 64), (8, 8, 128), (1, 1, 7)):
        cs = rc.case(65, P, N, c, 384, seed=1)
        info = _select(cs, 1, P=P, N=N)[4]
        assert (info[:, 3] > 0).any() and (info[:, 1] < info[:, 0]).any() and ((cs["rows"] < 0).any() or c < 128)


# ------------------------------------------------------------------ ABI
def test_new_entries_are_declared_exported_and_check_their_arguments():
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    L = ffi.lib()
    header = open(os.path.join(ROOT, "include", "coderag_hip.h")).read()
    for name in ("crh_recommend_query", "crh_recommend_select"):
        assert name in ffi.EXPORTS and hasattr(L, name) and re.search(rf"\bint {name}\(", header)
    for name, value in (("CRH_MAX_POS", 8), ("CRH_MAX_NEG", 8), ("CRH_RECOMMEND_AVERAGE", 0), ("CRH_RECOMMEND_BEST", 1), ("CRH_ABI_VERSION", 4)):
        assert re.search(rf"#define {name} {value}\b", header), name
    assert L.crh_abi_version() == 4 and (ffi.MAX_POS, ffi.MAX_NEG) == (8, 8) and (ffi.RECOMMEND_AVERAGE, ffi.RECOMMEND_BEST) == (0, 1)
    one = 16   # (a non-NULL, never dereferenced pointer: every case below is refused before a launch)

    def select(nq, P, N, c, k, dim, method, bf16=0, n_pos=None, n_neg=None, p=one):
        return L.crh_recommend_select(nq, P, N, c, k, dim, method, bf16, p, p, p, p, p, None if n_pos is None else n_pos.ctypes.data,
                                      None if n_neg is None else n_neg.ctypes.data, p, p, p, p, p, None)

    def query(nq, P, N, dim, n_pos=None, n_neg=None, p=one):
        return L.crh_recommend_query(nq, P, N, dim, p, None if n_pos is None else n_pos.ctypes.data, None if n_neg is None else n_neg.ctypes.data, p, None)
    i32 = lambda *v: np.asarray(v, np.int32)   # noqa: E731
    for args, word in (((1, 0, 0, 8, 1, 384, 1), b"P="), ((1, 9, 0, 8, 1, 384, 1), b"P="), ((1, 2, 9, 8, 1, 384, 1), b"N="), ((1, 2, -1, 8, 1, 384, 1), b"N="),
                       ((-1, 2, 2, 8, 1, 384, 1), b"nq="), ((1, 2, 2, 0, 1, 384, 1), b"c="), ((1, 2, 2, 513, 1, 384, 1), b"lists * c"),
                       ((1, 8, 2, 129, 1, 384, 1), b"lists * c"), ((1, 8, 2, 1025, 1, 384, 0), b"lists * c"), ((1, 2, 2, 8, 0, 384, 1), b"k="),
                       ((1, 2, 2, 8, 17, 384, 1), b"k="), ((1, 2, 2, 8, 9, 384, 0), b"k="), ((1, 2, 2, 8, 4, 512, 1), b"dim"), ((1, 2, 2, 8, 4, 0, 1), b"dim"),
                       ((1, 2, 2, 8, 4, 384, 2), b"method"), ((1, 2, 2, 8, 4, 384, -1), b"method"), ((0, 2, 2, 8, 4, 384, 7), b"method")):
        assert select(*args) == ffi.E_INVALID, args
        assert word in L.crh_last_error(), (args, L.crh_last_error())
    assert select(1, 2, 2, 8, 4, 384, 1, bf16=2) == ffi.E_INVALID and b"round_bf16" in L.crh_last_error()
    for n_pos, n_neg in ((i32(0, 1), None), (i32(1, 3), None), (None, i32(0, 3)), (None, i32(-1, 0))):
        assert select(2, 2, 2, 8, 4, 384, 1, n_pos=n_pos, n_neg=n_neg) == ffi.E_INVALID and b"n_pos=" in L.crh_last_error()
        assert query(2, 2, 2, 384, n_pos, n_neg) == ffi.E_INVALID and b"n_pos=" in L.crh_last_error()
    far = np.full((70,), 2, np.int32)
    far[69] = 3                                                        # a bad count behind the first launch's queries: still nothing is launched
    assert select(70, 2, 2, 8, 4, 384, 1, n_pos=far) == ffi.E_INVALID and b"query 69" in L.crh_last_error()
    assert query(70, 2, 2, 384, far) == ffi.E_INVALID and b"query 69" in L.crh_last_error()
    for args in ((1, 0, 0, 384), (1, 9, 0, 384), (1, 1, 9, 384), (-1, 1, 0, 384), (1, 1, 0, 100)):
        assert query(*args) == ffi.E_INVALID, args
    assert select(1, 2, 2, 8, 4, 384, 1, p=None) == ffi.E_INVALID and b"NULL" in L.crh_last_error()
    assert query(1, 2, 2, 384, p=None) == ffi.E_INVALID and b"NULL" in L.crh_last_error()
    assert select(1, 2, 2, 8, 4, 384, 1, p=8) == ffi.E_INVALID and b"aligned" in L.crh_last_error()
    assert select(0, 2, 2, 8, 4, 384, 1, p=None) == ffi.OK and query(0, 8, 8, 1536, p=None) == ffi.OK       # nothing to do
    with pytest.raises(ffi.NativeError, match="device tensor"):
        ffi.recommend_select(np.zeros((1, 1, 4), F32), np.zeros((1, 1, 4), np.int64), None, None, np.zeros((1, 1), np.int64), 1, 0, 2, "average")
    with pytest.raises(ffi.NativeError, match="device tensor"):
        ffi.recommend_query(np.zeros((1, 1, 384), F32), 1, 0)
    with pytest.raises(ValueError, match="strategy"):
        ffi.recommend_strategy("worst")


# ------------------------------------------------------------------ store plumbing over the fake index
def _fake_device(monkeypatch):
    ffi = fake_device(monkeypatch, SetFakeIndex)
    monkeypatch.setattr(ffi, "recommend_select", rc.recommend_select)
    monkeypatch.setattr(ffi, "recommend_query", rc.recommend_query)
    return ffi


def _quads(hits):
    return [(h["id"], _bits(h["score"]).item(), _bits(h.get("negative_score", -np.inf)).item(), h.get("matched_positive")) for h in hits]


@pytest.mark.parametrize("shards", [1, 2])
def test_store_recommend_over_the_fake_index(monkeypatch, shards):
    from coderag_amd.errors import VectorStoreError
    from coderag_amd.shards import STRIDE
    from coderag_amd.store import HipVectorStore
    _fake_device(monkeypatch)
    rng, vecs, payloads, ids = _corpus()
    vecs[200:220] = vecs[20:40]                                                    # duplicated rows: ties
    lang = np.asarray([p["language"] for p in payloads])
    proj = np.asarray([p["project_name"] for p in payloads])
    stored = orc.preprocess(vecs)

    async def run():
        kw = {"shards": shards, "_merge_fn": orc.merge_topk} if shards > 1 else {}
        async with HipVectorStore(dim=768, dtype="f32", initial_capacity=512, device=0, compact_dead_fraction=0.0, **kw) as s:
            await s.create_collections()
            for a in range(0, 240, 60):
                await s.upsert("code_chunks", ids[a:a + 60], vecs[a:a + 60], payloads[a:a + 60])
            col = s._col("code_chunks")
            sh, lo = col.rows_of(np.arange(240))
            gid = np.asarray(sh, np.int64) * STRIDE + np.asarray(lo, np.int64)
            order = np.argsort(gid)                                               # the order ties follow
            inv = np.empty(240, np.int64)
            inv[order] = np.arange(240)

            def want(pos, neg, limit, strategy, passing=None):
                pas = None if passing is None else passing[order]
                got = rc.brute_force(stored[order], inv[pos], inv[neg], limit, strategy, passing=pas)
                return [(ids[order[r]], sb, nb if strategy == "best" else _bits(-np.inf).item(), ids[pos[b]] if strategy == "best" else None) for r, sb, nb, b in got]
            sets = [([3, 25, 100], [7]), ([25], []), ([205, 25], [26, 150, 9]), ([1, 2, 3, 4, 5, 6, 7, 8], [9, 10, 11, 12, 13, 14, 15, 16])]
            named = [([ids[i] for i in p], [ids[i] for i in n]) for p, n in sets]
            for strategy in ("average", "best"):
                for (p, n), (pn, nn) in zip(sets, named):
                    got = await s.recommend("code_chunks", pn, nn, limit=10, strategy=strategy)
                    assert _quads(got) == want(p, n, 10, strategy)[:len(got)], (strategy, p, n)
                    assert not {h["id"] for h in got} & set(pn + nn)
                    assert all(set(h) == {"id", "score", "payload"} | ({"negative_score", "matched_positive"} if strategy == "best" else set()) for h in got)
                    if strategy == "average":
                        assert len(got) == 10
                passing = np.isin(lang, ["python", "go"]) & (proj != "p2")
                batch = await s.recommend_batch("code_chunks", named, limit=7, strategy=strategy, filters={"language": ["python", "go"]},
                                                must_not={"project_name": "p2"})
                alone = [await s.recommend("code_chunks", pn, nn, limit=7, strategy=strategy, filters={"language": ["python", "go"]},
                                           must_not={"project_name": "p2"}) for pn, nn in named]
                assert [_quads(b) for b in batch] == [_quads(a) for a in alone] and len(batch) == 4
                for (p, n), got in zip(sets, batch):
                    assert _quads(got) == want(p, n, 7, strategy, passing)[:len(got)] and (len(got) == 7 or strategy == "best")
            assert col.recommend_rounds["queries"] == 2 * (4 + 4 + 4)
            # "best" with shallow lists: round 2 runs and the answer is still the brute force's
            before = dict(col.recommend_rounds)
            got = await s.recommend("code_chunks", named[0][0], named[0][1], limit=10, strategy="best", candidates=3)
            assert col.recommend_rounds["round2"] == before["round2"] + 1
            assert _quads(got) == want(sets[0][0], sets[0][1], 10, "best")[:len(got)] and len(got) >= 1
            assert await s.recommend("code_chunks", named[0][0], limit=5, filters={"language": "cobol"}) == []
            assert await s.recommend_batch("code_chunks", [], limit=5) == []
            # a string is one id; a deleted or unknown id fails its caller, named
            one = await s.recommend("code_chunks", ids[25], limit=3)
            assert _quads(one) == want([25], [], 3, "average")
            await s.delete("code_chunks", {"file_path": payloads[40]["file_path"]})
            gone = [i for i in range(240) if payloads[i]["file_path"] == payloads[40]["file_path"]]
            bad = [s.recommend("code_chunks", [ids[gone[0]]]), s.recommend("code_chunks", [ids[3]], ["no-such-id"]),
                   s.recommend("code_chunks", []), s.recommend("code_chunks", [ids[i] for i in range(9)]),
                   s.recommend("code_chunks", [ids[3]], strategy="worst"), s.recommend("code_chunks", [ids[3]], limit=2000),
                   s.recommend("code_chunks", [ids[3], ids[5]], strategy="best", candidates=600), s.recommend("nope", [ids[3]])]
            res = await asyncio.gather(*bad, return_exceptions=True)
            assert all(isinstance(r, VectorStoreError) for r in res), res
            assert ids[gone[0]] in str(res[0]) and "no-such-id" in str(res[1])
            assert all(isinstance(r.cause, ValueError) for r in res[:-1]), [r.cause for r in res]

    asyncio.run(run())


# ------------------------------------------------------------------ the searcher and the MCP tool
def test_searcher_and_tool_forward_the_examples():
    from coderag_amd import mcp_tools, vector_search
    from coderag_amd.errors import QueryError, VectorStoreError

    class Store:
        def __init__(self):
            self.calls = []

        async def recommend(self, **kw):
            self.calls.append(kw)
            if kw["positive"] == ["boom"]:
                raise VectorStoreError("Failed to recommend", cause=ValueError("unknown or deleted point id 'boom'"))
            return [{"id": "a", "score": 0.5, "negative_score": 0.1, "matched_positive": "p1",
                     "payload": {"file_path": "f.py", "entity_type": "function", "entity_name": "e", "content": "x", "start_line": 1, "end_line": 2}}]

    async def run():
        st = Store()
        vs = vector_search.VectorSearcher(st, None)
        got = await vs.find_similar_to(["p1", "p2"], ["n1"], limit=4, strategy="best", language="python", exclude_files=["a.py"])
        assert st.calls[-1] == {"collection": "code_chunks", "positive": ["p1", "p2"], "negative": ["n1"], "limit": 4, "strategy": "best",
                                "filters": {"language": "python"}, "must_not": {"file_path": ["a.py"]}}
        assert got == [{"score": 0.5, "file_path": "f.py", "entity_type": "function", "entity_name": "e", "content": "x", "start_line": 1,
                        "end_line": 2, "negative_score": 0.1, "matched_positive": "p1"}]
        await vs.find_similar_to("p1")
        assert st.calls[-1] == {"collection": "code_chunks", "positive": ["p1"], "negative": [], "limit": vector_search.DEFAULT_SEARCH_LIMIT,
                                "strategy": "average"}
        with pytest.raises(QueryError):
            await vs.find_similar_to([])
        with pytest.raises(QueryError, match="boom"):
            await vs.find_similar_to(["boom"])

        class Searcher:
            def __init__(self):
                self.kw = []

            async def search_code(self, **kw):
                self.kw.append(("search_code", kw))
                return []

            async def find_similar_to(self, **kw):
                self.kw.append(("find_similar_to", kw))
                return [{"score": 0.5, "file_path": "f.py", "entity_type": "function", "entity_name": "e"}]
        sr = Searcher()
        tool = mcp_tools.create_semantic_search_tool(lambda: sr)
        assert (await tool["function"]("find it")).success and (await tool["function"]("find it", like_ids=[], unlike_ids=None)).success
        res = await tool["function"]("find it", limit=3, like_ids=["a", "b"], unlike_ids=["c"])
        assert res.success and res.data[0]["qualified_name"] == "e" and res.data[0]["score"] == 0.5
        assert not (await tool["function"]("find it", unlike_ids=["c"])).success
        assert sr.kw == [("search_code", {"query": "find it", "limit": 5, "entity_type": None}),
                         ("search_code", {"query": "find it", "limit": 5, "entity_type": None}),
                         ("find_similar_to", {"positive_ids": ["a", "b"], "negative_ids": ["c"], "limit": 3})]
        assert "like_ids" in tool["parameters"] and "unlike_ids" in tool["parameters"]

    asyncio.run(run())
