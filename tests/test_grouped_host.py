"""Exact per-group cap (group_by / group_size) above the device: the CPU restatement of ``crh_group_select``
(tests/group_cases.py) against the brute-force definition and its properties; the new C entries' exports and argument checks;
the store's exactness rounds, argument errors, coalescing and ``search_groups`` on 1 and 2 local shards over a fake index with
``ffi.group_select`` replaced by the restatement; the fill-with-minus-one-and-MAX completion of the codes over two gloo ranks;
the searchers' and the MCP tool's forwarding of ``max_per_file``."""
import asyncio
import os
import socket
import sys

import numpy as np
import pytest

from oracle import search as orc
from tests import group_cases
from tests.fake_index import fake_device
from tests.test_filter_sets_host import SetFakeIndex, _corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = np.uint32


class GroupFakeIndex(SetFakeIndex):
    """SetFakeIndex that counts the ``gather_codes`` calls (the gather itself is ``FakeIndex``'s)."""
    gathers = 0

    def gather_codes(self, *args, **kw):
        GroupFakeIndex.gathers += 1
        return super().gather_codes(*args, **kw)


# ------------------------------------------------------------------ the restatement itself
def _filtered(which, lang, rng):
    """Some (passing rows, description) pairs: no filter, an equality + a not-in combined, tombstones."""
    alive = rng.random(which.size) > 0.1
    return ((None, "all"), ((lang != 1) & ~np.isin(which, [0, 3, 7]), "language != 1 and file not in {0, 3, 7}"),
            (alive & (lang == 2), "tombstones and language == 2"))


@pytest.mark.parametrize("group_size", [1, 2, 3, 50])
def test_restatement_matches_the_brute_force_definition(group_size):
    raw, which, lang = group_cases.files_corpus()
    assert (which == -1).sum() == 60 and len(set(which.tolist())) == 41 and raw.shape[0] > 1024
    x = orc.preprocess(raw)
    rng = np.random.default_rng(group_size)
    queries = orc.preprocess(np.concatenate([rng.standard_normal((2, raw.shape[1])).astype(np.float32), raw[[5, 77]]]))   # two of them ON duplicated rows
    n = x.shape[0]
    incomplete = 0
    for passing, what in _filtered(which, lang, rng):
        for limit in (1, 10, 100):
            # the whole corpus as the candidate list: the walk IS the definition
            cs, cr, cc = group_cases.candidate_lists(x, queries, which, n, passing)
            pos, r, s, g, info = group_cases.group_select(cs, cr, cc, limit, group_size)
            # and a MAX_K-candidate list: equal wherever its info calls it complete
            ks, kr, kc = group_cases.candidate_lists(x, queries, which, 1024, passing)
            _, r2, s2, _, info2 = group_cases.group_select(ks, kr, kc, limit, group_size)
            for qi in range(len(queries)):
                es, er = group_cases.brute_force(x, queries[qi], which, limit, group_size, passing)
                assert np.array_equal(r[qi, :er.size], er) and (r[qi, er.size:] == -1).all(), (what, limit, qi)
                assert np.array_equal(s[qi, :er.size].view(U32), es.view(U32)) and np.isneginf(s[qi, er.size:]).all()
                assert np.array_equal(g[qi, :er.size], which[er]) and np.array_equal(cr[qi][pos[qi, :er.size]], er)
                assert (np.diff(s[qi, :er.size]) <= 0).all()                                   # still sorted by score
                counts = np.unique(which[er][which[er] >= 0], return_counts=True)[1]
                assert counts.size == 0 or counts.max() <= group_size
                if info2[qi, 0] >= limit or info2[qi, 1] < 1024:
                    assert np.array_equal(r2[qi], r[qi]) and np.array_equal(s2[qi].view(U32), s[qi].view(U32))
                else:
                    incomplete += 1
    assert group_size > 1 or incomplete > 0          # (S = 1, limit 100, 41 groups: 1024 candidates cannot settle it)


def test_restatement_ties_follow_the_row_order_and_keyless_rows_are_never_capped():
    scores = np.asarray([[0.9, 0.9, 0.9, 0.8, 0.8, 0.7, -np.inf, -np.inf]], np.float32)
    rows = np.asarray([[4, 9, 11, 2, 30, 31, -1, -1]], np.int64)
    codes = np.asarray([[5, 5, 5, -1, -1, 5, 5, -1]], np.int32)                 # (the padding's codes are never looked at)
    pos, r, s, g, info = group_cases.group_select(scores, rows, codes, 6, 2)
    assert pos.tolist() == [[0, 1, 3, 4, -1, -1]] and r.tolist() == [[4, 9, 2, 30, -1, -1]] and g.tolist() == [[5, 5, -1, -1, -1, -1]]
    assert info.tolist() == [[4, 6]] and np.isneginf(s[0, 4:]).all()


def test_restatement_prefix_stability_large_cap_short_and_empty_lists():
    raw, which, _ = group_cases.files_corpus()
    x = orc.preprocess(raw)
    q = orc.preprocess(np.random.default_rng(1).standard_normal((3, raw.shape[1])).astype(np.float32))
    cs, cr, cc = group_cases.candidate_lists(x, q, which, 200)
    full = group_cases.group_select(cs, cr, cc, 100, 3)
    for j in (1, 7, 100):
        part = group_cases.group_select(cs, cr, cc, j, 3)
        for a, b in zip(part[:4], full[:4]):
            assert np.array_equal(a, b[:, :j])
        assert np.array_equal(part[4], full[4])                                   # kept is not clipped at k
    for cap in (200, 5000):                                                        # S >= c changes nothing
        pos, r, s, g, info = group_cases.group_select(cs, cr, cc, 200, cap)
        assert np.array_equal(r, cr) and np.array_equal(s.view(U32), cs.view(U32)) and np.array_equal(g, cc)
        assert np.array_equal(pos, np.tile(np.arange(200, dtype=np.int32), (3, 1))) and info.tolist() == [[200, 200]] * 3
    # a list shorter than c, and one that is all padding
    few = which == 2
    cs, cr, cc = group_cases.candidate_lists(x, q, which, 512, few)
    pos, r, s, g, info = group_cases.group_select(cs, cr, cc, 10, 3)
    assert int(few.sum()) < 512 and info.tolist() == [[3, int(few.sum())]] * 3
    assert np.array_equal(r[:, :3], cr[:, :3]) and (r[:, 3:] == -1).all() and (pos[:, 3:] == -1).all() and np.isneginf(s[:, 3:]).all()
    pos, r, s, g, info = group_cases.group_select(np.full((2, 8), -np.inf, np.float32), np.full((2, 8), -1), np.full((2, 8), 4), 8, 1)
    assert (pos == -1).all() and (r == -1).all() and np.isneginf(s).all() and (g == -1).all() and info.tolist() == [[0, 0]] * 2


# ------------------------------------------------------------------ ABI
def test_new_entries_are_exported_and_check_their_arguments():
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    L = ffi.lib()
    for name in ("crh_index_gather_codes", "crh_group_select"):
        assert name in ffi.EXPORTS and hasattr(L, name)
    assert L.crh_abi_version() == 4
    assert L.crh_index_gather_codes(None, 0, 1, None, 0, None, None) == ffi.E_INVALID and b"NULL" in L.crh_last_error()
    one = 16   # (a non-NULL, never dereferenced pointer: every case below is refused before a launch)
    for nq, c, k, gs, word in ((1, 8, 0, 1, b"k="), (1, 8, 9, 1, b"k="), (1, 2048, 8, 1, b"c="), (-1, 8, 8, 1, b"nq="), (1, 8, 8, 0, b"group_size"),
                               (1, 8, 8, -3, b"group_size")):
        assert L.crh_group_select(nq, c, k, gs, one, one, one, one, one, one, one, one, None) == ffi.E_INVALID, (nq, c, k, gs)
        assert word in L.crh_last_error()
    assert L.crh_group_select(1, 8, 8, 1, None, None, None, None, None, None, None, None, None) == ffi.E_INVALID and b"NULL" in L.crh_last_error()
    assert L.crh_group_select(0, 8, 8, 1, None, None, None, None, None, None, None, None, None) == ffi.OK       # nothing to do
    with pytest.raises(ffi.NativeError, match="device tensor"):
        ffi.group_select(np.zeros((1, 4), np.float32), np.zeros((1, 4), np.int64), np.zeros((1, 4), np.int32), 2, 1)


# ------------------------------------------------------------------ store plumbing over the fake index
def _fake_device(monkeypatch):
    ffi = fake_device(monkeypatch, GroupFakeIndex)
    monkeypatch.setattr(ffi, "group_select", group_cases.group_select)
    return ffi


def _rounds_payloads(which):
    """One payload per row; the rows of file 1 differ in every other filterable key (values a ``must_not`` can name)."""
    return [{"file_path": f"/proj/f{int(w)}.py", "entity_type": "class" if w == 1 else "function", "entity_name": f"ent{i}",
             "language": "go" if w == 1 else "python", "start_line": i, "end_line": i + 3, "content": f"def ent{i}(): pass",
             "graph_node_id": f"mod.ent{i}", "content_hash": "x" if w == 1 else "h", "project_name": "zz" if w == 1 else "p"}
            for i, w in enumerate(which)]


def _pairs(hits):
    return [(h["id"], np.float32(h["score"]).view(U32).item()) for h in hits]


def _brute_pairs(stored, q_pre, which, ids, limit, group_size, passing=None):
    es, er = group_cases.brute_force(stored, q_pre, which, limit, group_size, passing)
    return [(ids[r], s.view(U32).item()) for s, r in zip(es, er)]


@pytest.mark.parametrize("shards", [1, 2])
def test_exactness_rounds(monkeypatch, shards):
    """limit 10 / group_size 3 / candidates 40 (the default) on the three corpora: the answer is the brute force over the whole
    corpus, and the rounds taken are the ones the corpus was built to need."""
    from coderag_amd.store import HipVectorStore
    _fake_device(monkeypatch)

    async def run():
        for kind, want_round2, want_exclusion in (("exclusion", 1, 1), ("round2", 1, 0), ("round1", 0, 0)):
            raw, which, q = group_cases.rounds_corpus(kind, dim=384)
            n = len(raw)
            ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(n)]
            payloads = _rounds_payloads(which)
            kw = {"shards": shards, "_merge_fn": orc.merge_topk} if shards > 1 else {}
            async with HipVectorStore(dim=384, dtype="f32", initial_capacity=4096, device=0, compact_dead_fraction=0.0, **kw) as s:
                await s.create_collections()
                step = (n + 3) // 4
                for a in range(0, n, step):                                   # four appends: the blocks go round the shards
                    await s.upsert("code_chunks", ids[a:a + step], raw[a:a + step], payloads[a:a + step])
                col = s._col("code_chunks")
                assert all(r > 0 for r in col.shards.rows)
                got = await s.search("code_chunks", q.tolist(), limit=10, group_by="file_path", group_size=3)
                stored, qp = orc.preprocess(raw), orc.preprocess(q[None])[0]
                assert _pairs(got) == _brute_pairs(stored, qp, which, ids, 10, 3), kind
                assert len(got) == 10 and max(np.unique([h["payload"]["file_path"] for h in got], return_counts=True)[1]) <= 3
                assert col.group_rounds == {"queries": 1, "round2": want_round2, "exclusion": want_exclusion}, (kind, col.group_rounds)
                # a batch mixes queries that stop in different rounds; a must_not on the grouped column is merged with the exclusion
                qs = np.stack([q, raw[7], -q])
                batch = await s.search_batch("code_chunks", qs, limit=10, group_by="file_path", group_size=3, must_not={"file_path": "/proj/f5.py"})
                for qi in range(3):
                    assert _pairs(batch[qi]) == _brute_pairs(stored, orc.preprocess(qs[qi][None])[0], which, ids, 10, 3, which != 5), (kind, qi)
                if kind == "exclusion":
                    neg = [c for c in SetFakeIndex.seen[-1] if len(c) == 3 and c[2]]
                    assert len(SetFakeIndex.seen[-1]) == 1 and len(neg[0][1]) >= 2          # ONE negated set: /proj/f5.py and the hot file
                    with pytest.raises(Exception) as e:                                      # eight conditions already: no room for the exclusion
                        await s.search("code_chunks", q.tolist(), limit=10, group_by="file_path", group_size=3,
                                       filters={"language": ["python"], "entity_type": ["function"], "project_name": ["p"], "content_hash": ["h"]},
                                       must_not={"language": "go", "entity_type": "class", "project_name": "zz", "content_hash": "x"})
                    assert isinstance(e.value.cause, ValueError) and "condition" in str(e.value.cause)

    asyncio.run(run())


@pytest.mark.parametrize("shards", [1, 2])
def test_store_grouped_search_arguments_coalescing_and_groups(monkeypatch, shards):
    from coderag_amd.errors import VectorStoreError
    from coderag_amd.store import HipVectorStore
    ffi = _fake_device(monkeypatch)
    rng, vecs, payloads, ids = _corpus()
    for i in range(0, 240, 40):
        del payloads[i]["file_path"]                                               # rows without the key
    payloads[3]["file_path"] = None                                                # ... and one whose value is None
    q = rng.standard_normal(768).astype(np.float32)
    stored, qp = orc.preprocess(vecs), orc.preprocess(q[None])[0]
    book = {}
    which = np.asarray([-1 if p.get("file_path") is None else book.setdefault(p["file_path"], len(book)) for p in payloads], np.int32)
    lang = np.asarray([p["language"] for p in payloads])

    async def run():
        kw = {"shards": shards, "_merge_fn": orc.merge_topk} if shards > 1 else {}
        async with HipVectorStore(dim=768, dtype="f32", initial_capacity=512, device=0, compact_dead_fraction=0.0, **kw) as s:
            await s.create_collections()
            for a in range(0, 240, 60):
                await s.upsert("code_chunks", ids[a:a + 60], vecs[a:a + 60], payloads[a:a + 60])
            plain10 = await s.search("code_chunks", q.tolist(), limit=10)
            # group_by=None: the plain path, none of the new code
            GroupFakeIndex.gathers = 0
            assert _pairs(await s.search("code_chunks", q.tolist(), limit=10, group_by=None, group_size=4)) == _pairs(plain10)
            assert _pairs((await s.search_batch("code_chunks", q[None], limit=10, group_by=None))[0]) == _pairs(plain10)
            assert GroupFakeIndex.gathers == 0 and s._col("code_chunks").group_rounds["queries"] == 0
            # grouped: the definition; rows without a file are never capped; filters and must_not combined
            for limit, gs in ((10, 1), (10, 2), (30, 3), (240, 50)):
                got = await s.search("code_chunks", q.tolist(), limit=limit, group_by="file_path", group_size=gs)
                assert _pairs(got) == _brute_pairs(stored, qp, which, ids, limit, gs), (limit, gs)
                assert all(set(h) == {"id", "score", "payload"} for h in got)
            assert GroupFakeIndex.gathers > 0
            got = await s.search("code_chunks", q.tolist(), limit=12, filters={"language": ["python", "go"]}, must_not={"project_name": "p2"},
                                 group_by="file_path", group_size=2, candidates=12)
            passing = np.isin(lang, ["python", "go"]) & np.asarray([p["project_name"] != "p2" for p in payloads])
            assert _pairs(got) == _brute_pairs(stored, qp, which, ids, 12, 2, passing)
            assert await s.search("code_chunks", q.tolist(), limit=5, filters={"language": "cobol"}, group_by="file_path") == []
            # grouping on another key; a cap larger than any group is the plain search
            lcode = np.asarray([("python", "go", "typescript").index(v) for v in lang], np.int32)
            assert _pairs(await s.search("code_chunks", q.tolist(), limit=9, group_by="language", group_size=2)) == _brute_pairs(stored, qp, lcode, ids, 9, 2)
            assert _pairs(await s.search("code_chunks", q.tolist(), limit=10, group_by="file_path", group_size=1000)) == _pairs(plain10)
            # every bad value fails its own caller only, with a ValueError behind it
            good = s.search("code_chunks", q.tolist(), limit=10, group_by="file_path", group_size=2)
            bad = [s.search("code_chunks", q.tolist(), limit=10, group_by="file_path", group_size=0),
                   s.search("code_chunks", q.tolist(), limit=10, group_size=0),
                   s.search("code_chunks", q.tolist(), limit=10, group_by="file_path", diversity=0.5),
                   s.search("code_chunks", None, limit=10, group_by="file_path"),
                   s.search("code_chunks", q.tolist(), limit=10, group_by="file_path", candidates=5),
                   s.search("code_chunks", q.tolist(), limit=10, group_by="file_path", candidates=ffi.MAX_K + 1),
                   s.search("code_chunks", q.tolist(), limit=10, group_by="start_line"),
                   s.search_batch("code_chunks", q[None], limit=10, group_by="file_path", group_size=0),
                   s.search_batch("code_chunks", q[None], limit=10, group_by="file_path", diversity=0.5),
                   s.search_batch("code_chunks", q[None], limit=10, group_by="nope")]
            res = await asyncio.gather(good, *bad, return_exceptions=True)
            assert _pairs(res[0]) == _brute_pairs(stored, qp, which, ids, 10, 2)
            assert all(isinstance(r, VectorStoreError) and isinstance(r.cause, ValueError) for r in res[1:]), res[1:]
            # coalescing: equal (group_by, group_size, candidates) share ONE pass at the largest limit and each caller keeps its own
            # prefix; a plain call and another group_size beside them are passes of their own
            before = s.search_passes
            a, b, c, d = await asyncio.gather(s.search("code_chunks", q.tolist(), limit=4, group_by="file_path", group_size=2, candidates=60),
                                              s.search("code_chunks", vecs[100].tolist(), limit=15, group_by="file_path", group_size=2, candidates=60),
                                              s.search("code_chunks", q.tolist(), limit=10),
                                              s.search("code_chunks", q.tolist(), limit=4, group_by="file_path", group_size=1, candidates=60))
            assert s.search_passes - before == 3
            assert _pairs(a) == _brute_pairs(stored, qp, which, ids, 4, 2) and _pairs(c) == _pairs(plain10)
            assert _pairs(b) == _brute_pairs(stored, orc.preprocess(vecs[100][None])[0], which, ids, 15, 2)
            assert _pairs(d) == _brute_pairs(stored, qp, which, ids, 4, 1)
            # search_groups: the G groups with the best top hit, each with its exact best S hits; rows without the key are left out
            everything = [h for h in await s.search("code_chunks", q.tolist(), limit=240)]

            def grouping(pred, g, size):
                out = {}
                for h in everything:
                    f = h["payload"].get("file_path")
                    if f is not None and pred(h["payload"]) and (f in out or len(out) < g):
                        out.setdefault(f, [])
                        if len(out[f]) < size:
                            out[f].append(h["id"])
                return list(out.items())

            def shape(groups):
                return [(g["id"], [h["id"] for h in g["hits"]]) for g in groups]
            assert shape(await s.search_groups("code_chunks", q.tolist(), "file_path", limit=5, group_size=3)) == grouping(lambda p: True, 5, 3)
            assert shape(await s.search_groups("code_chunks", q.tolist(), "file_path", limit=20, group_size=4)) == grouping(lambda p: True, 20, 4)   # 12 files
            got = await s.search_groups("code_chunks", q.tolist(), "file_path", limit=3, group_size=2, filters={"file_path": ["/proj/f2.py", "/proj/f3.py", "/proj/f4.py"]},
                                        must_not={"language": "go"})
            assert shape(got) == grouping(lambda p: p["file_path"] in ("/proj/f2.py", "/proj/f3.py", "/proj/f4.py") and p["language"] != "go", 3, 2) and len(got) == 2   # (f4 is all go)
            assert await s.search_groups("code_chunks", q.tolist(), "file_path", filters={"language": "cobol"}) == []
            for kwargs in ({"limit": 64, "group_size": 17}, {"limit": 0}, {"group_size": 0}):
                with pytest.raises(VectorStoreError):
                    await s.search_groups("code_chunks", q.tolist(), "file_path", **kwargs)

    asyncio.run(run())


# ------------------------------------------------------------------ two ranks: fill with -1 + one all-reduce(MAX)
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gloo_worker(rank: int, world: int, port: int, out_dir: str) -> None:
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from coderag_amd.shards import STRIDE, ShardSet
    from tests import group_cases
    from tests.test_grouped_host import GroupFakeIndex
    ffi.group_select = group_cases.group_select
    raw, which, lang = group_cases.files_corpus()                       # the same on every rank
    dim = raw.shape[1]
    sh = ShardSet(world, lambda s: GroupFakeIndex(dim=dim, capacity_rows=8192, n_code_cols=2), backend="dist", block=50, merge_fn=orc.merge_topk)
    shard = sh.route(len(raw))
    codes = np.stack([lang, which], axis=1).astype(np.int32)
    sh.append({rank: raw[shard == rank]}, codes, shard=shard)
    assert all(r > 0 for r in sh.rows) and sh.index[rank].count()[0] == sh.rows[rank]
    # the all-reduce(MAX) alone: each rank wrote its own positions of a buffer full of -1
    t = torch.full((4, 6), -1, dtype=torch.int32)
    t[rank::2] = torch.arange(24, dtype=torch.int32).reshape(4, 6)[rank::2] - 1          # (a stored code may be -1 or 0)
    sh.reduce(t, "MAX")
    assert torch.equal(t, torch.arange(24, dtype=torch.int32).reshape(4, 6) - 1)
    gid = np.empty(len(raw), np.int64)                                  # global row of every input row
    for s in range(world):
        sel = np.flatnonzero(shard == s)
        gid[sel] = s * STRIDE + np.arange(sel.size)
    order = np.argsort(gid)                                             # ties go to the lower GLOBAL row, as the merge orders them
    x = orc.preprocess(raw)
    q = np.random.default_rng(4).standard_normal((2, dim)).astype(np.float32)
    scores, rows, gcodes, info = sh.search_grouped(q, 20, 1024, 1, 2, None)
    for qi in range(2):
        es, er = group_cases.brute_force(x[order], orc.preprocess(q[qi][None])[0], which[order], 20, 2)
        assert np.array_equal(scores[qi].view(np.uint32), es.view(np.uint32)), f"rank {rank}: scores differ"
        assert np.array_equal(rows[qi], gid[order][er]) and np.array_equal(gcodes[qi], which[order][er]), f"rank {rank}: rows differ"
        assert info[qi, 0] >= 20 and info[qi, 1] == 1024
    open(os.path.join(out_dir, f"ok{rank}"), "w").write("ok")
    dist.destroy_process_group()


def test_codes_complete_over_two_gloo_ranks(tmp_path):
    import torch.multiprocessing as mp
    port = _free_port()
    mp.spawn(_gloo_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert sorted(os.listdir(tmp_path)) == ["ok0", "ok1"]


# ------------------------------------------------------------------ searchers and the MCP tool
class _Recorder:
    def __init__(self):
        self.calls = []

    async def search(self, **kw):
        self.calls.append(("search", kw))
        return []

    async def search_batch(self, **kw):
        self.calls.append(("search_batch", kw))
        return [[] for _ in kw["query_vectors"]]


class _Embedder:
    async def embed(self, text):
        return [0.0] * 4

    async def embed_batch(self, texts):
        return [[0.0] * 4 for _ in texts]


def test_searchers_forward_max_per_file_only_when_given():
    from coderag_amd import indexer, mcp_tools, vector_search

    async def run():
        for cls in (vector_search.VectorSearcher, indexer.VectorSearcher):
            rec = _Recorder()
            vs = cls(rec, _Embedder())
            await vs.search_code("q", limit=3, language="python")
            await vs.search_summaries("q", limit=3)
            assert [set(kw) for _, kw in rec.calls] == [{"collection", "query_vector", "limit", "filters"}] * 2       # today's call shape
            rec.calls.clear()
            await vs.search_code("q", limit=3, max_per_file=2)
            await vs.search_summaries("q", limit=3, max_per_file=1)
            assert [(kw["group_by"], kw["group_size"]) for _, kw in rec.calls] == [("file_path", 2), ("file_path", 1)]
            assert all("candidates" not in kw and "diversity" not in kw for _, kw in rec.calls)
        rec = _Recorder()
        vs = vector_search.VectorSearcher(rec, _Embedder())
        await vs.find_similar_code("x = 1", limit=3)
        await vs.search_code_batch(["a", "b"], limit=3)
        assert set(rec.calls[0][1]) == {"collection", "query_vector", "limit"} and set(rec.calls[1][1]) == {"collection", "query_vectors", "limit", "filters"}
        rec.calls.clear()
        await vs.find_similar_code("x = 1", limit=3, exclude_file="a.py", exact_exclude=True, max_per_file=2)
        await vs.search_code_batch(["a", "b"], limit=3, max_per_file=4)
        assert rec.calls[0][1]["must_not"] == {"file_path": "a.py"} and (rec.calls[0][1]["group_by"], rec.calls[0][1]["group_size"]) == ("file_path", 2)
        assert (rec.calls[1][1]["group_by"], rec.calls[1][1]["group_size"]) == ("file_path", 4)

        class Searcher:
            def __init__(self):
                self.kw = []

            async def search_code(self, **kw):
                self.kw.append(kw)
                return []
        sr = Searcher()
        tool = mcp_tools.create_semantic_search_tool(lambda: sr)
        assert (await tool["function"]("find it")).success and (await tool["function"]("find it", limit=3, max_per_file=2)).success
        assert sr.kw == [{"query": "find it", "limit": 5, "entity_type": None}, {"query": "find it", "limit": 3, "entity_type": None, "max_per_file": 2}]
        assert "max_per_file" in tool["parameters"]

    asyncio.run(run())
