"""Keyword search above the device: the native term cutter against its Python restatement (tests/lex_cases.py); the
restatement against an independent brute force; the new C entries' declarations, exports and the binding's argument checks;
the store's lexical and hybrid logic on 1 and 2 local shards over a fake index, with ``ffi.Lex`` and ``ffi.fuse_select`` replaced
by the restatements; the searchers' and the MCP tool's forwarding of ``mode``."""
import asyncio
import math
import os
import re

import numpy as np
import pytest

from oracle import search as orc
from tests import fuse_cases
from tests import lex_cases as lc
from tests.test_spans_host import SpanFakeIndex, _fake_device, _ids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = np.uint32
NEW_ENTRIES = ("crh_index_row_mask", "crh_lex_create", "crh_lex_destroy", "crh_lex_clear", "crh_lex_count", "crh_lex_append",
               "crh_lex_stats", "crh_lex_search")

AWKWARD = ["", "!!! ... ;; --", "_", "__init__", "a_b", "getHTTPResponseCode2xx", "SHA256_digest", "HTTPServer",
           "x" * 35 + "Y" * 35,                                   # a 70-byte identifier: two sub-words, the whole word is too long
           "q" * 70,                                              # ... and one sub-word of 70 bytes: nothing at all
           "word " * 300,                                         # tf saturates at 255, dl = 300
           "größeÄnderung_naïveCafé 変数名_カウント Ünïcode9x",      # non-ASCII bytes are lower-case letters, never folded
           "a\udc80b foo\udc80Bar",                               # a lone surrogate
           "line_one\r\nlineTwo\r\n\r\nline3"]


def _big_text():
    return ("def parse_retry_after(resp): return min(MAX_BACKOFF_MS, int(resp.headers['Retry-After']))  # HTTPServerError\n" * 10000)[: 1 << 20]


# ------------------------------------------------------------------ the native term cutter
@pytest.mark.parametrize("threads", [1, 7])
def test_native_terms_equal_the_restatement(threads):
    import coderag_amd  # noqa: F401
    from coderag_amd import lexical
    texts = AWKWARD + [_big_text()]
    got = lexical.terms_batch(texts, threads=threads)
    want = lc.rows_from_texts(texts)
    for g, w, name in zip(got, want, ("row_off", "terms", "tf", "dl")):
        assert g.dtype == w.dtype and np.array_equal(g, w), name
    off, terms, tf, dl = got
    assert list(dl[:3]) == [0, 0, 0] and dl[9] == 0 and dl[8] == 2                 # the 70-byte identifiers
    assert dl[10] == 300 and tf[off[10]:off[11]].tolist() == [255]
    assert np.array_equal(lexical.query_terms("getHTTPResponseCode2xx"), np.sort(np.asarray(
        [lc.fnv1a(t) for t in (b"get", b"http", b"response", b"code", b"xx", b"gethttpresponsecode2xx")], U32)))
    assert [lc.terms_of(t) for t in ("__init__", "a_b", "SHA256_digest", "HTTPServer")] == [
        [b"init"], [b"a_b"], [b"sha", b"256", b"digest", b"sha256_digest"], [b"http", b"server", b"httpserver"]]
    assert lexical.point_text({"summary": "s", "content": "c", "entity_name": "n", "x": "no"}) == b"n\nc\ns"
    assert lexical.point_text({"content": 5, "summary": "a\udc80"}) == "a\udc80".encode("utf-8", "surrogatepass") == lc.point_text({"summary": "a\udc80"})
    assert lexical.LEXICAL_KEYS == lc.LEXICAL_KEYS and lexical.MAX_QUERY_TERMS == lc.MAX_QUERY_TERMS == 32


def test_weights_are_the_restatements():
    import coderag_amd  # noqa: F401
    from coderag_amd import lexical
    df = [0, 1, 7, 1000, 999999, 1000000]
    a, b = lexical.bm25_weights(df, 1000000, 123456789), lc.idf(df, 1000000, 123456789)
    assert np.array_equal(a[0].view(U32), b[0].view(U32)) and a[1] == b[1] and (a[0] > 0).all()
    assert a[0][0] == np.float32(math.log(1.0 + 1000000.5 / 0.5)) and a[1] == np.float32(123456789 / 1000000)
    assert lexical.bm25_weights([], 0, 0)[1] == 1.0
    terms, keep = lexical.rarest(np.arange(100, 140, dtype=U32), [5] * 10 + [1] * 10 + [5] * 20, 32)
    assert keep.tolist() == list(range(0, 32)) and terms.tolist() == list(range(100, 132))     # the 10 rare ones, then ties to the lower id


# ------------------------------------------------------------------ the restatement itself
def test_restatement_equals_an_independent_brute_force():
    """Row by row, term by term, in Python floats rounded to f32 after every operation (bit for bit) and in f64 (the ranking of
    well-separated scores)."""
    f32 = np.float32
    off, terms, tf, dl = lc.corpus(150)
    words, every, nowhere = lc.vocabulary()
    queries = [np.sort(np.asarray(q, U32)) for q in ([words[0]], [words[1], words[5], every], [nowhere], [], list(words[:31]) + [every])]
    ids = np.unique(np.concatenate(queries))
    mask = np.random.default_rng(2).random(150) < 0.8
    df, n, sum_dl = lc.stats(off, terms, dl, None, ids)
    w, avgdl = lc.idf(df, n, sum_dl)
    table = dict(zip(ids.tolist(), w))
    idf = [np.asarray([table[int(t)] for t in q], f32) for q in queries]
    k1, b = f32(1.2), f32(0.75)
    got = lc.bm25_search(off, terms, tf, dl, mask, queries, idf, k1, b, avgdl, 150, row_base=7)
    for qi, q in enumerate(queries):
        exact, wide = {}, {}
        for r in range(150):
            if not mask[r]:
                continue
            held = {int(t): int(c) for t, c in zip(terms[off[r]:off[r + 1]], tf[off[r]:off[r + 1]])}
            s32, s64, any_term = f32(0.0), 0.0, False
            for t, wt in zip(q.tolist(), idf[qi]):
                if t not in held:
                    continue
                any_term = True
                c = f32(held[t])
                norm = f32(k1 * f32(f32(f32(1.0) - b) + f32(b * f32(f32(dl[r]) / avgdl))))
                s32 = f32(s32 + f32(wt * f32(f32(c * f32(k1 + f32(1.0))) / f32(c + norm))))
                s64 += float(wt) * (held[t] * 2.2) / (held[t] + 1.2 * (0.25 + 0.75 * dl[r] / float(avgdl)))
            if any_term:
                exact[r], wide[r] = s32, s64
        order = sorted(exact, key=lambda r: (-float(exact[r]), r))
        assert got[2][qi] == len(order)
        assert got[1][qi, :len(order)].tolist() == [r + 7 for r in order] and (got[1][qi, len(order):] == -1).all()
        assert np.array_equal(got[0][qi, :len(order)].view(U32), np.asarray([exact[r] for r in order], f32).view(U32))
        for a, c in zip(order, order[1:]):                   # f64 agrees wherever two neighbours are well separated
            if float(exact[a]) - float(exact[c]) > 1e-4 * float(exact[a]):
                assert wide[a] > wide[c]
    assert got[2][2] == 0 and got[2][3] == 0 and got[2][1] == np.count_nonzero(mask & (np.diff(off) > 0)) - int(mask[10])   # (row 10 holds one word only)


# ------------------------------------------------------------------ header, exports, binding checks
def test_header_declares_and_binding_exports_the_new_entries():
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "coderag_hip.h")).read(), flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in ffi.EXPORTS and hasattr(ffi.lib(), name), name
    assert "#define CRH_LEX_MAX_QUERY_TERMS 32" in header and ffi.LEX_MAX_QUERY_TERMS == 32
    assert ffi.lib().crh_abi_version() == ffi.ABI_VERSION == 4


def test_binding_refuses_bad_queries_before_the_library():
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    ok = ffi.lex_queries([np.arange(32, dtype=U32), []], [np.ones(32, np.float32), []])
    assert ok[0].tolist() == [0, 32, 32] and ok[1].dtype == U32 and ok[2].dtype == np.float32
    for queries, idf in (([np.arange(33, dtype=U32)], [np.ones(33, np.float32)]), ([[3, 2]], [[1.0, 1.0]]), ([[3, 3]], [[1.0, 1.0]]),
                         ([[1, 2]], [[1.0]]), ([[1]], [])):
        with pytest.raises(ffi.NativeError) as e:
            ffi.lex_queries(queries, idf)
        assert e.value.code == ffi.E_INVALID
    lex = ffi.Lex.__new__(ffi.Lex)                            # (no handle: the checks come before anything touches it)
    lex._h, lex.device = None, 0
    for k in (0, -1, ffi.MAX_K + 1):
        with pytest.raises(ffi.NativeError, match="k="):
            lex.search([[1, 2]], [[1.0, 1.0]], k)
    with pytest.raises(ffi.NativeError, match="CSR"):
        lex.append([0, 2], [1], [1], [1])


# ------------------------------------------------------------------ store logic over the fake index
class FakeLex:
    """``ffi.Lex`` on host arrays: the restatement behind the interface, the refusals of ``crh_lex_append`` included."""
    instances: list = []
    stats_masks: list = []
    searched: list = []

    def __init__(self, capacity_rows=0, device=0):
        self.off, self.terms, self.tf, self.dl = np.zeros(1, np.int64), np.zeros(0, U32), np.zeros(0, np.uint8), np.zeros(0, np.int32)
        self.appends, self.closed = 0, False
        FakeLex.instances.append(self)

    def append(self, row_off, terms, tf, dl):
        row_off, terms, tf, dl = np.asarray(row_off, np.int64), np.asarray(terms, U32), np.asarray(tf, np.uint8), np.asarray(dl, np.int32)
        assert row_off[0] == 0 and (np.diff(row_off) >= 0).all() and (tf > 0).all()
        for i in range(len(dl)):
            t = terms[row_off[i]:row_off[i + 1]].astype(np.int64)
            assert (np.diff(t) > 0).all() and dl[i] >= tf[row_off[i]:row_off[i + 1]].astype(np.int64).sum()
        self.off = np.concatenate([self.off, self.off[-1] + row_off[1:]])
        self.terms, self.tf, self.dl = np.concatenate([self.terms, terms]), np.concatenate([self.tf, tf]), np.concatenate([self.dl, dl])
        self.appends += 1

    def count(self):
        return len(self.dl), len(self.terms)

    def clear(self):
        self.__init__()

    def close(self):
        self.closed = True

    def _mask(self, words):
        return None if words is None else lc.mask_from_words(words, len(self.dl))

    def stats(self, terms, mask=None):
        FakeLex.stats_masks.append(None if mask is None else self._mask(mask))
        return lc.stats(self.off, self.terms, self.dl, self._mask(mask), np.asarray(terms, U32))

    def search(self, queries, idf, k, k1=1.2, b=0.75, avgdl=1.0, mask=None, row_base=0, stream=0, **kw):
        from coderag_amd import ffi
        ffi.lex_queries(queries, idf)
        FakeLex.searched.append([np.asarray(q, U32) for q in queries])
        return lc.bm25_search(self.off, self.terms, self.tf, self.dl, self._mask(mask), queries, idf, k1, b, avgdl, k, row_base)


class LexFakeIndex(SpanFakeIndex):
    def row_mask(self, filters=None, out=None, stream=0):
        return lc.words_from_mask(self._mask(filters))


def _fake_lexical_device(monkeypatch):
    ffi = _fake_device(monkeypatch)
    monkeypatch.setattr(ffi, "Index", LexFakeIndex)
    monkeypatch.setattr(ffi, "Lex", FakeLex)
    monkeypatch.setattr(ffi, "fuse_select", fuse_cases.fuse_select)
    FakeLex.instances, FakeLex.stats_masks, FakeLex.searched = [], [], []
    return ffi


def _pairs(hits):
    return [(h["id"], int(np.float32(h["score"]).view(U32))) for h in hits]


N, DIM = 700, 384
TEXTS = ["retry_after", "parse request header", "HTTPServerError MAX_BACKOFF_MS", lc.RARE, "no_such_identifier_anywhere", "",
         "flushPayloadHTTPServer encode_token"]


def _store_kw(shards):
    return {"shards": shards, "_merge_fn": orc.merge_topk} if shards > 1 else {}


async def _check_lexical(s, col, passes=None, filters=None, must_not=None, limit=25):
    want, counts, _, _ = lc.store_expected(col, TEXTS, limit, passes)
    got = await s.search_lexical_batch("code_chunks", TEXTS, limit=limit, filters=filters, must_not=must_not)
    assert [_pairs(g) for g in got] == want
    for t, c in zip(TEXTS, counts):
        assert await s.lexical_count("code_chunks", t, filters=filters, must_not=must_not) == c
    assert _pairs(await s.search_lexical("code_chunks", TEXTS[0], limit=3, filters=filters, must_not=must_not)) == want[0][:3]
    return want, counts


@pytest.mark.parametrize("shards", [1, 2])
def test_store_lexical_search_lifecycle(monkeypatch, tmp_path, shards):
    from coderag_amd.store import HipVectorStore
    _fake_lexical_device(monkeypatch)
    pay = lc.chunks(N)
    pay[N - 1] = dict(pay[N - 1], content=pay[N - 1]["content"] + f" {lc.RARE}(x)")       # (RARE_AT is beyond this small corpus)
    raw = np.random.default_rng(0).standard_normal((N, DIM)).astype(np.float32)
    ids = _ids(N)
    snap = str(tmp_path / "snap")

    async def run():
        async with HipVectorStore(dim=DIM, dtype="f32", initial_capacity=4096, device=0, compact_dead_fraction=0.0, **_store_kw(shards)) as s:
            await s.create_collections()
            for a in (0, 250):                                                                 # (two appends: the blocks go round the shards)
                await s.upsert("code_chunks", ids[a:a + 250], raw[a:a + 250], pay[a:a + 250])
            col = s._col("code_chunks")
            assert FakeLex.instances == [] and col._lex == {}                                  # lazy: nothing built by an upsert
            want, counts = await _check_lexical(s, col)
            assert len(FakeLex.instances) == shards and all(x.appends == 1 for x in FakeLex.instances)
            assert counts[4] == 0 and counts[5] == 0 and want[5] == [] and counts[0] > 25 and 0 < counts[2]
            assert want[0][0][1] == want[0][1][1]                                              # the identical chunks tie
            calls = col.lex_stats_calls
            await _check_lexical(s, col)
            assert col.lex_stats_calls == calls                                                # every term's df was kept
            # the tail is brought up to date after an upsert, the statistics counted again
            for a in (500, 600):
                await s.upsert("code_chunks", ids[a:a + 100], raw[a:a + 100], pay[a:a + 100])
            assert sum(x.count()[0] for x in FakeLex.instances) == 500
            want2, counts2 = await _check_lexical(s, col)
            assert sum(x.count()[0] for x in FakeLex.instances) == N and col.lex_stats_calls > calls and counts2[0] > counts[0]
            assert [h for h, _ in want2[3]] == [ids[N - 1]] and counts2[3] == 1                # the rare identifier: one chunk, rank 1
            # a filter: the rows of the filter, the idf of the whole collection
            FakeLex.stats_masks.clear()
            go = lambda p: p.get("language") == "go"   # noqa: E731
            wf, cf = await _check_lexical(s, col, go, filters={"language": "go"})
            assert 0 < cf[0] < counts2[0]
            for q in (0, 1):                                                                    # same idf, same avgdl: same score bits
                by_id = dict(want2[q])
                assert all(by_id.get(i, b) == b for i, b in wf[q]) and any(i in by_id for i, _ in wf[q])
            await _check_lexical(s, col, lambda p: p.get("file_path") != "/proj/f3.py" and p.get("start_line", 0) >= 100,
                                 filters={"start_line": {"gte": 100}}, must_not={"file_path": "/proj/f3.py"})
            assert all(m is None or m.sum() == N for m in FakeLex.stats_masks)                  # statistics never saw the filter
            assert await s.search_lexical("code_chunks", "retry_after", filters={"language": "cobol"}) == []
            # delete: tombstones reach the keyword side through the row mask only
            await s.delete("code_chunks", {"file_path": "/proj/f3.py"})
            want3, counts3 = await _check_lexical(s, col)
            assert counts3[0] < counts2[0] and all(x.count()[0] > 0 for x in FakeLex.instances)
            # compact: dropped and rebuilt
            built = len(FakeLex.instances)
            assert await s.compact("code_chunks") > 0
            assert col._lex == {} and all(x.closed for x in FakeLex.instances)
            want4, counts4 = await _check_lexical(s, col)
            assert len(FakeLex.instances) == built + shards and counts4 == counts3
            assert [[b for _, b in w] for w in want4] == [[b for _, b in w] for w in want3]     # the same scores from the survivors
            await s.save(snap)
            assert not any("lex" in f.lower() for _, _, fs in os.walk(snap) for f in fs)        # never part of a snapshot
        async with HipVectorStore(dim=DIM, dtype="f32", initial_capacity=4096, device=0, compact_dead_fraction=0.0, **_store_kw(shards)) as s:
            await s.create_collections()
            await s.load(snap)
            col = s._col("code_chunks")
            assert col._lex == {}
            want5, counts5 = await _check_lexical(s, col)
            assert want5 == want4 and counts5 == counts4
        # a fresh build from the surviving points answers with the same scores
        keep = [i for i in range(N) if pay[i]["file_path"] != "/proj/f3.py"]
        async with HipVectorStore(dim=DIM, dtype="f32", initial_capacity=4096, device=0, compact_dead_fraction=0.0, **_store_kw(shards)) as s:
            await s.create_collections()
            await s.upsert("code_chunks", [ids[i] for i in keep], raw[keep], [pay[i] for i in keep])
            fresh = await s.search_lexical_batch("code_chunks", TEXTS, limit=N)
            assert [len(f) for f in fresh] == counts4
            assert [sorted(b for _, b in _pairs(f))[::-1][:25] for f in fresh] == [sorted((b for _, b in w), reverse=True) for w in want4]

    asyncio.run(run())


@pytest.mark.parametrize("shards", [1, 2])
def test_store_rarest_terms_hybrid_fields_and_refusals(monkeypatch, shards):
    from coderag_amd.errors import VectorStoreError
    from coderag_amd.shards import STRIDE
    from coderag_amd.store import HipVectorStore
    ffi = _fake_lexical_device(monkeypatch)
    pay = lc.chunks(N)
    pay[N - 1] = dict(pay[N - 1], content=pay[N - 1]["content"] + f" {lc.RARE}(x)")
    raw = np.random.default_rng(0).standard_normal((N, DIM)).astype(np.float32)
    ids = _ids(N)

    async def run():
        async with HipVectorStore(dim=DIM, dtype="f32", initial_capacity=4096, device=0, compact_dead_fraction=0.0, **_store_kw(shards)) as s:
            await s.create_collections()
            for a in (0, 350):
                await s.upsert("code_chunks", ids[a:a + 350], raw[a:a + 350], pay[a:a + 350])
            col = s._col("code_chunks")
            # more than 32 distinct terms: the 32 with the smallest df, ties to the lower id
            long_text = " ".join(lc._VERBS) + " " + " ".join(lc._NOUNS) + " " + " ".join(f"x{i}" for i in range(20)) + " " + lc.RARE
            all_terms = lc.query_terms(long_text)
            assert all_terms.size > 32
            want, counts, _, searched = lc.store_expected(col, [long_text], 10)
            got = await s.search_lexical("code_chunks", long_text, limit=10)
            assert _pairs(got) == want[0] and searched[0].size == 32
            assert np.array_equal(FakeLex.searched[-1][0], searched[0]) and lc.fnv1a(lc.RARE.lower().encode()) in searched[0].tolist()
            df = {int(t): sum(int(np.count_nonzero(x.terms == t)) for x in FakeLex.instances) for t in all_terms}
            order = sorted(all_terms.tolist(), key=lambda t: (df[t], t))
            assert sorted(order[:32]) == searched[0].tolist()
            # hybrid: the two candidate lists, the fusion's restatement, and where each score comes from
            qi = [N - 1, 3, 50]
            qv = raw[qi] + np.float32(0.01)
            texts = [lc.RARE, "retry_after MAX_BACKOFF_MS", "fetch shard cursor"]
            limit, c = 10, 40
            _, _, (ls, lr), _ = lc.store_expected(col, texts, c)
            stored = np.concatenate([ix.x for ix in col.shards.index.values()])
            grow = np.concatenate([np.arange(len(ix.x), dtype=np.int64) + sh * STRIDE for sh, ix in col.shards.index.items()])
            es, er = orc.search(stored, orc.preprocess(qv), c)
            dr = np.where(er >= 0, grow[np.maximum(er, 0)], -1)
            # (ties in the dense list would need the global-row order; random vectors have none)
            assert all(len(set(row.tolist())) == c for row in es)
            fused = fuse_cases.fuse_select(np.stack([es, ls], axis=1), np.stack([dr, lr], axis=1), 2, limit, "rrf", 60, None)
            got = await s.search_hybrid_batch("code_chunks", qv, texts, limit=limit)
            slot_of = {}
            for sh in col.shards.index:
                slots = lc.store_rows(col)[sh][0]
                slot_of.update({sh * STRIDE + i: int(t) for i, t in enumerate(slots)})
            for q in range(3):
                rows = [int(r) for r in fused[0][q] if r >= 0]
                assert [h["id"] for h in got[q]] == [ids[slot_of[r]] for r in rows] and len(rows) == limit
                for j, (h, r) in enumerate(zip(got[q], rows)):
                    assert np.float32(h["score"]).view(U32) == fused[1][q, j].view(U32)
                    in_d, in_l = np.flatnonzero(dr[q] == r), np.flatnonzero(lr[q] == r)
                    assert h["cosine"] == (float(es[q, in_d[0]]) if in_d.size else None)
                    assert h["lexical_score"] == (float(ls[q, in_l[0]]) if in_l.size else None)
                    assert h["matched"] == tuple(n for n, on in (("vector", in_d.size), ("lexical", in_l.size)) if on) and h["matched"]
                    assert set(h) == {"id", "score", "payload", "cosine", "lexical_score", "matched"}
            assert got[0][0]["id"] == ids[N - 1] and got[0][0]["matched"] == ("vector", "lexical")      # found by both: first
            one = await s.search_hybrid("code_chunks", qv[1].tolist(), texts[1], limit=limit)
            assert _pairs(one) == _pairs(got[1])
            w = await s.search_hybrid("code_chunks", qv[1].tolist(), texts[1], limit=5, candidates=20, rrf_k=10, weights=[0.0, 1.0])
            assert all("lexical" in h["matched"] for h in w)                                         # the dense list weighs nothing
            assert await s.search_hybrid("code_chunks", qv[1].tolist(), texts[1], filters={"language": "cobol"}) == []
            # refusals
            for kw in ({"fusion": "max"}, {"diversity": 0.5}, {"group_by": "file_path"}, {"max_overlap": 0.5}, {"score_threshold": 0.1},
                       {"filters": [None]}, {"candidates": 513}, {"candidates": 5}, {"rrf_k": -1}, {"weights": [1.0]}):
                with pytest.raises(VectorStoreError):
                    await s.search_hybrid("code_chunks", qv[0].tolist(), "retry", limit=10, **kw)
            with pytest.raises(VectorStoreError):
                await s.search_hybrid_batch("code_chunks", qv, texts[:2])
            for kw in ({"limit": 1025}, {"filters": [None]}, {"k1": -1.0}, {"b": 1.5}):
                with pytest.raises(VectorStoreError):
                    await s.search_lexical("code_chunks", "retry", **kw)
            with pytest.raises(VectorStoreError):
                await s.search_lexical("code_chunks", 5)
            # one process per shard: not available yet, and said so
            monkeypatch.setattr(col.shards, "backend", "dist")
            for call in (s.search_lexical("code_chunks", "retry"), s.lexical_count("code_chunks", "retry"),
                         s.search_hybrid("code_chunks", qv[0].tolist(), "retry")):
                with pytest.raises(VectorStoreError) as e:
                    await call
                assert "not available" in str(e.value.__cause__ or e.value)
            monkeypatch.setattr(col.shards, "backend", "local")

    asyncio.run(run())


# ------------------------------------------------------------------ the callers
class _SpyStore:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        async def call(**kw):
            self.calls.append((name, kw))
            hit = {"id": "i", "score": 0.5, "payload": {"entity_name": "f", "file_path": "/p.py"}}
            if name.startswith("search_hybrid"):
                hit.update(cosine=0.9, lexical_score=None, matched=("vector",))
            return [[hit] for _ in kw["texts"]] if name.endswith("_batch") and "texts" in kw else [[hit]] if name.endswith("_batch") else [hit]
        return call


class _SpyEmbedder:
    def __init__(self):
        self.calls = 0

    async def embed(self, text):
        self.calls += 1
        return [0.0] * 4

    async def embed_batch(self, texts):
        self.calls += 1
        return [[0.0] * 4 for _ in texts]


def test_mode_semantic_issues_the_calls_it_issued_before_and_the_others_forward():
    import coderag_amd  # noqa: F401
    from coderag_amd import indexer, vector_search
    from coderag_amd.mcp_tools import create_semantic_search_tool

    async def run():
        for Searcher in (vector_search.VectorSearcher, indexer.VectorSearcher):
            store, emb = _SpyStore(), _SpyEmbedder()
            vs = Searcher(store, emb)
            await vs.search_code("where is parse_retry_after", limit=7, language="python")
            await vs.search_code("where is parse_retry_after", limit=7, language="python", mode="semantic")
            await vs.search_summaries("what does it do", limit=3)
            assert [n for n, _ in store.calls] == ["search"] * 3 and emb.calls == 3
            assert store.calls[0] == store.calls[1] == ("search", {"collection": "code_chunks", "query_vector": [0.0] * 4, "limit": 7,
                                                                   "filters": {"language": "python"}})
            assert set(store.calls[2][1]) == {"collection", "query_vector", "limit", "filters"}
            store.calls.clear()
            await vs.search_code("parse_retry_after", limit=7, language="python", mode="lexical")
            assert emb.calls == 3 and store.calls == [("search_lexical", {"collection": "code_chunks", "text": "parse_retry_after", "limit": 7,
                                                                           "filters": {"language": "python"}})]
            store.calls.clear()
            got = await vs.search_code("parse_retry_after", limit=7, mode="hybrid", candidates=50)
            assert emb.calls == 4 and store.calls[0][0] == "search_hybrid"
            assert store.calls[0][1]["text"] == "parse_retry_after" and store.calls[0][1]["candidates"] == 50 and store.calls[0][1]["limit"] == 7
            assert len(got) == 1
            await vs.search_summaries("what", mode="lexical")
            assert store.calls[-1][0] == "search_lexical" and store.calls[-1][1]["collection"] == "summaries"
            with pytest.raises(Exception):
                await vs.search_code("x", mode="keyword")
            with pytest.raises(Exception):
                await vs.search_code("x", mode="lexical", diversity=0.5)
        store, emb = _SpyStore(), _SpyEmbedder()
        vs = vector_search.VectorSearcher(store, emb)
        hyb = await vs.search_code("q", mode="hybrid")
        assert hyb[0]["cosine"] == 0.9 and hyb[0]["lexical_score"] is None and hyb[0]["matched"] == ("vector",)
        store.calls.clear()
        await vs.search_code_batch(["a b", "c"], limit=4)
        await vs.search_code_batch(["a b", "c"], limit=4, mode="semantic")
        a, b = store.calls
        assert a[0] == b[0] == "search_batch" and list(a[1]) == list(b[1]) == ["collection", "query_vectors", "limit", "filters"]
        assert all(np.array_equal(a[1][k], b[1][k]) for k in a[1])
        out = await vs.search_code_batch(["a b", "c"], limit=4, mode="lexical", language="go")
        assert store.calls[-1] == ("search_lexical_batch", {"collection": "code_chunks", "texts": ["a b", "c"], "limit": 4, "filters": {"language": "go"}})
        assert len(out) == 2
        out = await vs.search_code_batch(["a b", "c"], limit=4, mode="hybrid")
        assert store.calls[-1][0] == "search_hybrid_batch" and out[0][0]["matched"] == ("vector",)
        with pytest.raises(Exception):
            await vs.search_code_batch(np.zeros((2, 4), np.float32), mode="lexical")
        # the MCP tool forwards `mode` only when it is given
        seen = []

        class Searcher:
            async def search_code(self, **kw):
                seen.append(kw)
                return []
        tool = create_semantic_search_tool(lambda: Searcher())
        assert "mode" in tool["parameters"]
        assert (await tool["function"](query="q")).success and (await tool["function"](query="q", mode="hybrid")).success
        assert "mode" not in seen[0] and seen[1]["mode"] == "hybrid"

    asyncio.run(run())
