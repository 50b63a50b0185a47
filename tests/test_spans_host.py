"""Line spans above the device: the CPU restatement of ``crh_span_select`` (tests/span_cases.py) against the brute-force
definition and its hand-written cases; the new C entry's exports and argument checks and the binding's packing of range
conditions; the store's range-bound conversion, numeric coding, ``ValueError``s, exactness rounds, ``chunks_at``, range deletes
and the format-4 snapshot path on 1 and 2 local shards over a fake index with ``ffi.span_select`` replaced by the restatement; the
fill-with-minus-one-and-MAX completion of the three gathers over two gloo ranks; the searchers' and the MCP tool's forwarding of
``max_overlap``."""
import asyncio
import ctypes as C
import json
import os
import socket
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest

from oracle import search as orc
from tests import span_cases
from tests.fake_index import fake_device
from tests.test_filter_sets_host import SetFakeIndex
from tests.test_grouped_host import GroupFakeIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = np.uint32
MAX_K = 1024


class SpanFakeIndex(GroupFakeIndex):
    """GroupFakeIndex + range conditions (``(col, lo, hi, "between" | "not_between")``, the semantics of ``CRH_COND_BETWEEN``) and
    the widening load of a snapshot that holds fewer code columns than the index."""

    def _mask(self, filters=None):
        SetFakeIndex.seen.append(filters)
        return span_cases.np_mask(self.codes, self.alive, filters)

    def search_multi(self, queries, k, class_filters, query_class, row_base=0, **kw):
        """One oracle search per distinct filter in use, as ``ffi.Index.search_multi`` answers a mixed batch."""
        from coderag_amd import ffi
        queries = np.asarray(queries, np.float32)
        classes, qclass, _ = ffi.multi_plan(class_filters, query_class)
        out_s, out_r = np.full((len(queries), k), -np.inf, np.float32), np.full((len(queries), k), -1, np.int64)
        for c in range(len(classes)):
            sel = np.flatnonzero(qclass == c)
            out_s[sel], out_r[sel] = self.search(queries[sel], k, filters=classes[c], row_base=row_base)
        return out_s, out_r

    def load(self, directory, widen=None):
        super().load(directory)
        if self.codes.shape[1] < self.n_code_cols:
            assert widen is not None, "a narrower snapshot needs the missing columns"
            extra = np.asarray(widen(0, len(self.x)), np.int32).reshape(self.n_code_cols - self.codes.shape[1], len(self.x))
            self.codes = np.ascontiguousarray(np.concatenate([self.codes, extra.T], axis=1))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(U32)


# ------------------------------------------------------------------ the restatement itself
def test_restatement_matches_the_brute_force_definition():
    raw, files, lo, hi, hot = span_cases.spans_corpus()
    n = raw.shape[0]
    assert (files == -1).sum() == 60 and len(set(files.tolist())) == 41 and n > MAX_K and (hi == -1).sum() > 5
    x = orc.preprocess(raw)
    rng = np.random.default_rng(2)
    dup = int(np.flatnonzero((files == 7))[0])
    queries = orc.preprocess(np.concatenate([rng.standard_normal((2, raw.shape[1])).astype(np.float32), raw[[hot, dup]]]))   # two of them ON stored rows
    lang = rng.integers(0, 3, n)
    alive = rng.random(n) > 0.1
    filters = ((None, "all"), ((lang != 1) & (lo >= 5) & (lo <= 200), "a set AND a range on the start line"), (alive, "tombstones"))
    complete = incomplete = 0
    for passing, what in filters:
        full_lists = span_cases.candidate_lists(x, queries, files, lo, hi, n, passing)           # the whole corpus as the list: the walk IS the definition
        k_lists = span_cases.candidate_lists(x, queries, files, lo, hi, MAX_K, passing)
        orders = [span_cases.plain_order(x, queries[qi], passing) for qi in range(len(queries))]
        for permille in (0, 200, 500, 1000):
            for limit in (1, 10, 100):
                pos, r, s, f, a, b, info = span_cases.span_select(*full_lists, limit, permille)
                _, r2, s2, _, _, _, info2 = span_cases.span_select(*k_lists, limit, permille)
                for qi in range(len(queries)):
                    es, er, total = span_cases.brute_force(x, queries[qi], files, lo, hi, limit, permille, passing, orders[qi])
                    assert np.array_equal(r[qi, :er.size], er) and (r[qi, er.size:] == -1).all(), (what, permille, limit, qi)
                    assert np.array_equal(_bits(s[qi, :er.size]), _bits(es)) and np.isneginf(s[qi, er.size:]).all()
                    assert np.array_equal(f[qi, :er.size], files[er]) and np.array_equal(a[qi, :er.size], lo[er]) and np.array_equal(b[qi, :er.size], hi[er])
                    assert np.array_equal(full_lists[1][qi][pos[qi, :er.size]], er) and info[qi, 0] == total
                    assert (np.diff(s[qi, :er.size]) <= 0).all()                                # still sorted by score
                    _assert_no_overlap(files[er], lo[er], hi[er], permille)
                    if info2[qi, 0] >= limit or info2[qi, 1] < MAX_K:                           # a MAX_K list that calls itself complete IS the answer
                        assert np.array_equal(r2[qi], r[qi]) and np.array_equal(_bits(s2[qi]), _bits(s[qi])), (what, permille, limit, qi)
                        complete += 1
                    else:                                                                       # ... and an incomplete one a strict prefix of it
                        kept = int(info2[qi, 0])
                        assert kept < limit and np.array_equal(r2[qi, :kept], r[qi, :kept]) and (r2[qi, kept:] == -1).all()
                        incomplete += 1
    assert complete > 0 and incomplete > 0, (complete, incomplete)


def _assert_no_overlap(files, lo, hi, permille):
    """No two kept rows of one file share more than permille of the shorter span (the property the walk guarantees)."""
    for i in range(len(files)):
        for j in range(i):
            if files[i] >= 0 and files[i] == files[j] and min(lo[i], lo[j]) >= 0 and hi[i] >= lo[i] and hi[j] >= lo[j]:
                ov = int(min(hi[i], hi[j])) - int(max(lo[i], lo[j])) + 1
                assert ov <= 0 or ov * 1000 <= permille * min(int(hi[i]) - int(lo[i]) + 1, int(hi[j]) - int(lo[j]) + 1), (i, j)


def _one(files, los, his, permille, k=None, scores=None, rows=None):
    c = len(files)
    scores = np.linspace(0.9, 0.1, c).astype(np.float32) if scores is None else np.asarray(scores, np.float32)
    rows = np.arange(c, dtype=np.int64) + 10 if rows is None else np.asarray(rows, np.int64)
    out = span_cases.span_select(scores[None], rows[None], np.asarray(files, np.int32)[None], np.asarray(los, np.int32)[None],
                                 np.asarray(his, np.int32)[None], k or c, permille)
    return [o[0] for o in out]


def test_restatement_hand_written_cases():
    # ties: equal scores keep the list's order (the lower row first), and the first of two equal spans wins
    pos, r, s, f, a, b, info = _one([5, 5, 5, 6], [10, 10, 40, 10], [30, 30, 60, 30], 500, scores=[0.9, 0.9, 0.9, 0.9], rows=[4, 9, 11, 30])
    assert pos.tolist() == [0, 2, 3, -1] and r.tolist() == [4, 11, 30, -1] and info.tolist() == [3, 4] and np.isneginf(s[3])
    # a nested span AFTER its container is dropped; BEFORE it, the container is dropped (the shorter span is the measure)
    assert _one([1, 1], [10, 20], [100, 30], 500)[0].tolist() == [0, -1]
    assert _one([1, 1], [20, 10], [30, 100], 500)[0].tolist() == [0, -1]
    assert _one([1, 2], [10, 20], [100, 30], 0)[0].tolist() == [0, 1]                       # another file: unrelated
    # a dropped candidate shields nobody: C overlaps only B, and B fell to A
    assert _one([1, 1, 1], [10, 18, 28], [20, 30, 40], 100)[0].tolist() == [0, 2, -1]
    # exactly permille of the shorter span is kept, one line more is dropped: spans of 10 lines sharing 5 (500) / 6 lines
    assert _one([1, 1], [1, 6], [10, 15], 500)[0].tolist() == [0, 1]
    assert _one([1, 1], [1, 5], [10, 14], 500)[0].tolist() == [0, -1]
    assert _one([1, 1], [1, 6], [10, 15], 499)[0].tolist() == [0, -1]
    assert _one([1, 1], [1, 10], [10, 19], 0)[0].tolist() == [0, -1] and _one([1, 1], [1, 11], [10, 19], 0)[0].tolist() == [0, 1]   # one shared line / touching
    assert _one([1, 1], [1, 1], [10, 10], 1000)[0].tolist() == [0, 1]                        # 1000: even an exact copy stays
    # hi < lo, lo = -1, file = -1: no span -- kept, and never a reason to drop somebody else
    pos, r, s, f, a, b, info = _one([1, 1, 1, -1, 1], [10, -1, 30, 10, 10], [20, 20, 12, 20, 20], 0)
    assert pos.tolist() == [0, 1, 2, 3, -1] and f.tolist() == [1, 1, 1, -1, -1] and a.tolist() == [10, -1, 30, 10, -1] and info.tolist() == [4, 5]
    assert _one([1, 1], [10, 10], [5, 20], 0)[0].tolist() == [0, 1]
    # the longest spans an int32 column can hold do not overflow
    big = 2 ** 31 - 1
    assert _one([1, 1, 2, 1], [0, 0, 0, big], [big, big, big, big], 999)[0].tolist() == [0, 2, -1, -1]    # (one shared line of a one-line span: all of it)
    assert _one([1, 1], [0, big], [big - 1, big], 0)[0].tolist() == [0, 1]
    # padding is skipped and counted nowhere
    out = span_cases.span_select(np.asarray([[0.5, -np.inf]], np.float32), np.asarray([[3, -1]]), np.asarray([[1, 1]]), np.asarray([[1, 1]]), np.asarray([[2, 2]]), 2, 0)
    assert out[0].tolist() == [[0, -1]] and out[6].tolist() == [[1, 1]]
    out = span_cases.span_select(np.full((2, 8), -np.inf, np.float32), np.full((2, 8), -1), np.full((2, 8), 4), np.full((2, 8), 1), np.full((2, 8), 9), 8, 0)
    assert (out[0] == -1).all() and (out[1] == -1).all() and np.isneginf(out[2]).all() and out[6].tolist() == [[0, 0]] * 2


def test_restatement_prefix_property_and_permille_1000():
    raw, files, lo, hi, hot = span_cases.spans_corpus()
    x = orc.preprocess(raw)
    q = orc.preprocess(np.random.default_rng(1).standard_normal((3, raw.shape[1])).astype(np.float32))
    lists = span_cases.candidate_lists(x, q, files, lo, hi, 200)
    full = span_cases.span_select(*lists, 100, 300)
    for j in (1, 7, 100):
        part = span_cases.span_select(*lists, j, 300)
        for a, b in zip(part[:6], full[:6]):
            assert np.array_equal(a, b[:, :j])
        assert np.array_equal(part[6], full[6])                                   # kept is not clipped at k
    pos, r, s, f, a, b, info = span_cases.span_select(*lists, 200, 1000)          # 1000 changes nothing
    assert np.array_equal(r, lists[1]) and np.array_equal(_bits(s), _bits(lists[0])) and np.array_equal(f, lists[2])
    assert np.array_equal(pos, np.tile(np.arange(200, dtype=np.int32), (3, 1))) and info.tolist() == [[200, 200]] * 3


# ------------------------------------------------------------------ ABI
def test_new_entry_is_exported_and_checks_its_arguments():
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    L = ffi.lib()
    assert "crh_span_select" in ffi.EXPORTS and hasattr(L, "crh_span_select")
    assert L.crh_abi_version() == 4 and C.sizeof(ffi.Condition) == 24
    assert (ffi.COND_IN, ffi.COND_NOT_IN, ffi.COND_BETWEEN, ffi.COND_NOT_BETWEEN) == (0, 1, 2, 3) and ffi.VALUE_MAX == 2 ** 31 - 1
    header = open(os.path.join(ROOT, "include", "coderag_hip.h")).read()
    for name, val in (("CRH_COND_IN", 0), ("CRH_COND_NOT_IN", 1), ("CRH_COND_BETWEEN", 2), ("CRH_COND_NOT_BETWEEN", 3)):
        assert f"#define {name} {val}\n" in header
    one = 16   # (a non-NULL, never dereferenced pointer: every case below is refused before a launch)
    ptrs = [one] * 12
    for nq, c, k, pm, word in ((1, 8, 0, 500, b"k="), (1, 8, 9, 500, b"k="), (1, 2048, 8, 500, b"c="), (-1, 8, 8, 500, b"nq="),
                               (1, 8, 8, -1, b"permille"), (1, 8, 8, 1001, b"permille")):
        assert L.crh_span_select(nq, c, k, pm, *ptrs, None) == ffi.E_INVALID, (nq, c, k, pm)
        assert word in L.crh_last_error()
    for hole in range(12):                                                          # every pointer is checked
        assert L.crh_span_select(1, 8, 8, 500, *[None if i == hole else one for i in range(12)], None) == ffi.E_INVALID and b"NULL" in L.crh_last_error()
    assert L.crh_span_select(0, 8, 8, 500, *[None] * 12, None) == ffi.OK            # nothing to do
    with pytest.raises(ffi.NativeError, match="device tensor"):
        ffi.span_select(np.zeros((1, 4), np.float32), np.zeros((1, 4), np.int64), *(np.zeros((1, 4), np.int32) for _ in range(3)), 2, 500)


def test_binding_packs_the_between_form():
    from coderag_amd import ffi
    assert ffi.is_set_condition((2, 5, 9, "between")) and ffi.is_range_condition((2, 5, 9, "not_between"))
    assert not ffi.is_range_condition((0, 3)) and not ffi.is_range_condition((0, [3], True))
    arr, n, keep = ffi._conditions([(0, 3), (7, 100, 160, "between"), (6, -4, 2 ** 40, "not_between"), (1, {9, 4}), (6, 9, 3, "between")])
    assert n == 5 and (arr[0].col, arr[0].negate, arr[0].n) == (0, 0, 1)
    assert (arr[1].col, arr[1].negate, arr[1].n) == (7, ffi.COND_BETWEEN, 2) and keep[1].tolist() == [100, 160] and arr[1].codes == keep[1].ctypes.data
    assert (arr[2].col, arr[2].negate, arr[2].n) == (6, ffi.COND_NOT_BETWEEN, 2) and keep[2].tolist() == [0, 2 ** 31 - 1]   # clipped to the column's values
    assert (arr[3].negate, arr[3].n) == (0, 2) and keep[3].tolist() == [4, 9]
    assert arr[4].negate == ffi.COND_BETWEEN and keep[4][0] > keep[4][1]              # lo > hi stays an empty range
    assert keep[1].dtype == np.int32
    with pytest.raises(ffi.NativeError, match="between"):
        ffi._conditions([(0, 1, 2, "within")])
    # the filter key tells ranges from sets, and from each other
    keys = {ffi.filter_key([c]) for c in ((3, 1, 2, "between"), (3, 1, 2, "not_between"), (3, 1, 3, "between"), (3, [1, 2]), (3, [1, 2], True))}
    assert len(keys) == 5 and ffi.filter_key([(3, 9, 3, "between")]) == ffi.filter_key([(3, 7, 1, "between")])


# ------------------------------------------------------------------ bounds, coding, ValueErrors
def test_range_bound_conversion():
    from coderag_amd import ffi
    from coderag_amd.store import range_bounds
    top = ffi.VALUE_MAX
    assert range_bounds("k", {"gte": 100, "lte": 160}) == (100, 160)
    assert range_bounds("k", {"gt": 100, "lt": 160}) == (101, 159)
    assert range_bounds("k", {"gte": 99.2, "lte": 160.9}) == (100, 160) and range_bounds("k", {"gt": 99.2, "lt": 160.9}) == (100, 160)
    assert range_bounds("k", {"gt": 99.0, "lt": 160.0}) == (100, 159) and range_bounds("k", {"gte": -3.5}) == (0, top)
    assert range_bounds("k", {}) == (0, top) and range_bounds("k", {"gte": 7}) == (7, top) and range_bounds("k", {"lt": 7}) == (0, 6)
    assert range_bounds("k", {"gte": None, "lte": 4}) == (0, 4)                       # Qdrant's Range(gte=None): open
    assert range_bounds("k", {"gte": 5, "gt": 7, "lte": 20, "lt": 12}) == (8, 11)     # every bound holds
    lo, hi = range_bounds("k", {"gte": 9, "lte": 3})
    assert lo > hi
    assert range_bounds("k", {"lte": float("inf")}) == (0, top) and range_bounds("k", {"gte": float("-inf")}) == (0, top)
    lo, hi = range_bounds("k", {"gt": float("inf")})
    assert lo > hi
    assert range_bounds("k", NS(gte=3, gt=None, lte=None, lt=10)) == (3, 9)           # a duck-typed Range
    assert range_bounds("k", {"gte": np.int64(4), "lte": np.float32(6.5)}) == (4, 6)
    for bad in ({"ge": 3}, {"gte": "3"}, {"lt": float("nan")}, {"gte": True}, {"lte": [1]}):
        with pytest.raises(ValueError, match="'start_line'"):
            range_bounds("start_line", bad)


def test_numeric_coding_of_odd_payload_values():
    from coderag_amd.tables import PayloadTable
    t = PayloadTable()
    vals = [7, 0, 2 ** 31 - 1, 2 ** 31, -3, True, "7", 7.0, None, 2 ** 70]
    t.extend([{"file_path": "a.py", "start_line": v, "end_line": 12} for v in vals] + [{"file_path": "a.py"}])
    got = t.numeric_codes(("start_line", "end_line"), 0, t.n)
    assert got.dtype == np.int32 and got[:, 0].tolist() == [7, 0, 2 ** 31 - 1, -1, -1, -1, -1, -1, -1, -1, -1]
    assert got[:, 1].tolist() == [12] * 10 + [-1]
    assert [t.get(i).get("start_line", "absent") for i in range(t.n)] == vals + ["absent"]        # the payloads come back as stored
    assert t.numeric_codes(("end_line",), 9, 11).tolist() == [[12], [-1]] and t.numeric_codes((), 0, 3).shape == (3, 0)
    t.truncate(2)
    t.extend([{"start_line": 5}])
    assert t.numeric_codes(("start_line", "end_line"), 0, t.n).tolist() == [[7, 12], [0, 12], [5, -1]]


# ------------------------------------------------------------------ store plumbing over the fake index
def _fake_device(monkeypatch=None):
    return fake_device(monkeypatch, SpanFakeIndex, span_select=span_cases.span_select)


def _pairs(hits):
    return [(h["id"], np.float32(h["score"]).view(U32).item()) for h in hits]


def _ids(n):
    return [f"00000000-0000-4000-8000-{i:012d}" for i in range(n)]


def _brute_pairs(col, stored, q_pre, files, lo, hi, ids, limit, permille, passing=None, depth=MAX_K):
    """The brute force in the order the store's shards define: ties go to the lower GLOBAL row (shard first, then local row).
    ``depth``: how far down the plain order the store may look (``MAX_K``: its deepest round) -- the answer is the corpus-wide
    walk's first ``limit`` kept rows, or, when fewer than that lie among the first ``depth`` rows, exactly those (the SHORT
    return); ``None``: the corpus-wide walk itself."""
    from coderag_amd.shards import STRIDE
    n = len(stored)
    sh, loc = col.rows_of(np.arange(n))
    order = np.argsort(np.asarray(sh, np.int64) * STRIDE + np.asarray(loc, np.int64))
    es, er = span_cases.plain_order(stored[order], q_pre, None if passing is None else np.asarray(passing)[order])
    kept = np.asarray(span_cases.walk(files[order][er], lo[order][er], hi[order][er], permille), np.int64)
    if depth is not None and kept.size and (kept < depth).sum() < limit:
        kept = kept[kept < depth]
    kept = kept[:limit]
    return [(ids[order[r]], s.view(U32).item()) for s, r in zip(es[kept], er[kept])]


async def _filled(s, ids, raw, payloads, parts=4):
    n = len(raw)
    await s.create_collections()
    step = (n + parts - 1) // parts
    for a in range(0, n, step):                                                    # several appends: the blocks go round the shards
        await s.upsert("code_chunks", ids[a:a + step], raw[a:a + step], payloads[a:a + step])
    col = s._col("code_chunks")
    assert all(r > 0 for r in col.shards.rows)
    return col


@pytest.mark.parametrize("shards", [1, 2])
def test_exactness_rounds_and_the_short_return(monkeypatch, shards):
    """limit 10 / max_overlap 0.5 / candidates 40 (the default) on the corpora built to settle in round 1 and in round 2, and
    limit 5 on the file of 2000 copies of one row: the answer is the brute force over the whole corpus -- for the short case
    its first kept hits -- and the rounds taken are the ones the corpus was built to need."""
    from coderag_amd.store import HipVectorStore
    _fake_device(monkeypatch)

    async def run():
        for kind, limit, want in (("round1", 10, {"queries": 1, "round2": 0, "short": 0}), ("round2", 10, {"queries": 1, "round2": 1, "short": 0}),
                                  ("short", 5, {"queries": 1, "round2": 1, "short": 1})):
            raw, files, lo, hi, q = span_cases.rounds_corpus(kind)
            n = len(raw)
            ids = _ids(n)
            kw = {"shards": shards, "_merge_fn": orc.merge_topk} if shards > 1 else {}
            async with HipVectorStore(dim=384, dtype="f32", initial_capacity=4096, device=0, compact_dead_fraction=0.0, **kw) as s:
                col = await _filled(s, ids, raw, span_cases.payloads(files, lo, hi))
                assert col.numeric_keys == ("start_line", "end_line") and col.keys[0] == "file_path"
                codes = np.concatenate([ix.codes for ix in col.shards.index.values()])
                assert codes.shape[1] == len(col.keys) + 2 and sorted(codes[:, -2].tolist()) == sorted(lo.tolist())   # the values themselves, last
                stored, qp = orc.preprocess(raw), orc.preprocess(q[None])[0]
                got = await s.search("code_chunks", q.tolist(), limit=limit, max_overlap=0.5)
                brute = _brute_pairs(col, stored, qp, files, lo, hi, ids, limit, 500, depth=None)
                assert len(brute) == limit and col.span_rounds == want, (kind, col.span_rounds)
                if kind == "short":
                    assert len(got) == 1 and _pairs(got) == brute[:1]               # SHORT: the first kept hits of the corpus-wide walk, only fewer
                    plain = await s.search("code_chunks", q.tolist(), limit=limit)
                    assert len({(h["payload"]["file_path"], h["payload"]["start_line"]) for h in plain}) == 1   # the plain list: one span five times
                else:
                    assert _pairs(got) == brute, kind
                    assert sum(h["payload"]["file_path"] == "/proj/f0.py" for h in got) == 1
                # a batch mixes queries that stop in different rounds; a range filter and a must_not ride along
                qs = np.stack([q, raw[7], -q])
                batch = await s.search_batch("code_chunks", qs, limit=limit, max_overlap=0.5, filters={"start_line": {"gte": 0, "lt": 1200}},
                                             must_not={"file_path": "/proj/f5.py"})
                passing = (lo < 1200) & (files != 5)
                for qi in range(3):
                    want_q = _brute_pairs(col, stored, orc.preprocess(qs[qi][None])[0], files, lo, hi, ids, limit, 500, passing)
                    assert _pairs(batch[qi]) == want_q and len(want_q) == (limit if kind != "short" or qi == 2 else 1 + (files[7] != 0) * (qi == 1)), (kind, qi)
                assert SetFakeIndex.seen[-1][0][3] == "between" and SetFakeIndex.seen[-1][0][0] == len(col.keys)

    asyncio.run(run())


@pytest.mark.parametrize("shards", [1, 2])
def test_store_ranges_chunks_at_arguments_and_default_path(monkeypatch, shards):
    from coderag_amd.errors import VectorStoreError
    from coderag_amd.store import HipVectorStore, _filter_key
    ffi = _fake_device(monkeypatch)
    raw, files, lo, hi, hot = span_cases.spans_corpus(dim=384, hot_copies=3)
    n = len(raw)
    ids = _ids(n)
    rng = np.random.default_rng(3)
    lang = rng.integers(0, 3, n)
    pay = span_cases.payloads(files, lo, hi, lang)
    q = rng.standard_normal(384).astype(np.float32)
    stored, qp = orc.preprocess(raw), orc.preprocess(q[None])[0]
    has_lo, has_hi = lo >= 0, hi >= 0

    def fc(key, **kw):
        return NS(key=key, match=None, range=NS(**{"gte": None, "gt": None, "lte": None, "lt": None, **kw}))

    async def run():
        kw = {"shards": shards, "_merge_fn": orc.merge_topk} if shards > 1 else {}
        async with HipVectorStore(dim=384, dtype="f32", initial_capacity=4096, device=0, compact_dead_fraction=0.0, **kw) as s:
            col = await _filled(s, ids, raw, pay)
            everything = await s.search("code_chunks", q.tolist(), limit=MAX_K)
            order = {h["id"]: i for i, h in enumerate(everything)}

            def host(pred, limit):
                return [(h["id"], np.float32(h["score"]).view(U32).item()) for h in everything if pred(h["payload"])][:limit]
            # max_overlap=None: the plain path, none of the new code -- no gather call, no round counted
            GroupFakeIndex.gathers = 0
            plain10 = await s.search("code_chunks", q.tolist(), limit=10)
            assert _pairs(await s.search("code_chunks", q.tolist(), limit=10, max_overlap=None)) == _pairs(plain10)
            assert _pairs((await s.search_batch("code_chunks", q[None], limit=10, max_overlap=None))[0]) == _pairs(plain10)
            assert GroupFakeIndex.gathers == 0 and col.span_rounds["queries"] == 0
            # max_overlap: the definition, for several shares and limits; 1.0 is the plain search
            for limit, share in ((10, 0.0), (10, 0.2), (30, 0.5), (100, 0.5)):
                got = await s.search("code_chunks", q.tolist(), limit=limit, max_overlap=share)
                assert _pairs(got) == _brute_pairs(col, stored, qp, files, lo, hi, ids, limit, round(share * 1000)), (limit, share)
                assert all(set(h) == {"id", "score", "payload"} for h in got)
            assert GroupFakeIndex.gathers >= 3 * shards
            assert _pairs(await s.search("code_chunks", q.tolist(), limit=10, max_overlap=1.0)) == _pairs(plain10)
            # ranges: gte / gt / lte / lt, floats, open ends, a plain int, ANDed with a set, under must_not (rows without the value pass)
            sl = lambda p: p.get("start_line")   # noqa: E731
            el = lambda p: p.get("end_line")     # noqa: E731
            cases = [({"start_line": {"gte": 100, "lte": 160}}, None, lambda p: sl(p) is not None and 100 <= sl(p) <= 160),
                     ({"start_line": {"gt": 99.5, "lt": 160.5}}, None, lambda p: sl(p) is not None and 100 <= sl(p) <= 160),
                     ({"end_line": {"lt": 40}}, None, lambda p: el(p) is not None and el(p) < 40),
                     ({"end_line": {}}, None, lambda p: el(p) is not None),
                     ({"start_line": int(lo[hot])}, None, lambda p: sl(p) == int(lo[hot])),
                     ({"start_line": {"lte": 120}, "end_line": {"gte": 120}, "language": ["python", "go"]}, None,
                      lambda p: sl(p) is not None and el(p) is not None and sl(p) <= 120 <= el(p) and p["language"] != "rust"),
                     (None, {"end_line": {"gte": 50}}, lambda p: el(p) is None or el(p) < 50),
                     ({"language": "go"}, {"start_line": {"lt": 100}, "file_path": "/proj/f3.py"},
                      lambda p: p["language"] == "go" and (sl(p) is None or sl(p) >= 100) and p.get("file_path") != "/proj/f3.py"),
                     ({"start_line": {"gte": 9, "lte": 3}}, None, lambda p: False),
                     ({"start_line": {"gt": 2 ** 40}}, None, lambda p: False), (None, {"start_line": -7}, lambda p: True)]
            for filters, must_not, pred in cases:
                got = await s.search("code_chunks", q.tolist(), limit=25, filters=filters, must_not=must_not)
                assert _pairs(got) == host(pred, 25), (filters, must_not)
                fetched = await s.search("code_chunks", None, limit=n, filters=filters, must_not=must_not)      # the filter-only fetch
                assert [h["id"] for h in fetched] == [ids[i] for i in range(n) if pred(pay[i])], (filters, must_not)
            # per-query filter lists: every query under its own range, as a lone search answers it
            per = [{"start_line": {"gte": 100}}, {"start_line": {"lt": 100}}, None, {"start_line": {"gte": 100}}]
            batch = await s.search_batch("code_chunks", np.stack([q] * 4), limit=12, filters=per)
            for f, hits in zip(per, batch):
                assert _pairs(hits) == _pairs(await s.search("code_chunks", q.tolist(), limit=12, filters=f))
            # the coalescing key tells ranges apart, and equal ranges written differently are one pass
            assert _filter_key({"start_line": {"gte": 4}}, None) == _filter_key({"start_line": {"gt": 3}}, None) == _filter_key({"start_line": {"gt": 3.5}}, None)
            assert len({_filter_key({"start_line": v}, None) for v in ({"gte": 4}, {"gte": 5}, {"lte": 4}, 4, [4], {})}) == 6
            before = s.search_passes
            a, b, c = await asyncio.gather(s.search("code_chunks", q.tolist(), limit=5, filters={"start_line": {"gte": 100}}),
                                           s.search("code_chunks", q.tolist(), limit=7, filters={"start_line": {"gt": 99}}),
                                           s.search("code_chunks", q.tolist(), limit=5, filters={"start_line": {"gte": 101}}))
            assert s.search_passes - before == 2 and _pairs(a) == _pairs(b)[:5] == host(lambda p: sl(p) is not None and sl(p) >= 100, 5)
            assert _pairs(c) == host(lambda p: sl(p) is not None and sl(p) >= 101, 5)
            # chunks_at: one filter-only device call per shard, payloads in insertion order
            f3 = "/proj/f3.py"
            line = int(np.median(lo[(files == 3) & has_lo]))
            calls = len(SetFakeIndex.seen)
            got = await s.chunks_at("code_chunks", f3, line)
            assert len(SetFakeIndex.seen) == calls + shards
            want = [pay[i] for i in range(n) if files[i] == 3 and has_lo[i] and has_hi[i] and lo[i] <= line <= hi[i]]
            assert got == want and len(want) >= 2                                                     # the class and a method at least
            got = await s.chunks_at("code_chunks", f3, line, last_line=line + 30)
            want = [pay[i] for i in range(n) if files[i] == 3 and has_lo[i] and has_hi[i] and lo[i] <= line + 30 and hi[i] >= line]
            assert got == want and got[:2] == (await s.chunks_at("code_chunks", f3, line, last_line=line + 30, limit=2))
            assert await s.chunks_at("code_chunks", "/never/stored.py", 3) == [] and await s.chunks_at("code_chunks", f3, 10 ** 6) == []
            # raw client: FieldCondition(key, range=Range(...)) under must and must_not
            raw_client = s.client
            cnt = (await raw_client.count("code_chunks", count_filter=NS(must=[fc("start_line", gte=50, lt=150)], must_not=None))).count
            assert cnt == int((has_lo & (lo >= 50) & (lo < 150)).sum())
            cnt = (await raw_client.count("code_chunks", count_filter=NS(must=[NS(key="language", match=NS(value="go"))], must_not=[fc("end_line", gt=80)]))).count
            assert cnt == int(((lang == 1) & ~(has_hi & (hi > 80))).sum())
            # every bad value fails its own caller only, with a ValueError behind it
            good = s.search("code_chunks", q.tolist(), limit=10, max_overlap=0.5)
            bad = [s.search("code_chunks", q.tolist(), limit=10, max_overlap=1.5), s.search("code_chunks", q.tolist(), limit=10, max_overlap=-0.1),
                   s.search("code_chunks", q.tolist(), limit=10, max_overlap=float("nan")), s.search("code_chunks", q.tolist(), limit=10, max_overlap="half"),
                   s.search("code_chunks", q.tolist(), limit=10, max_overlap=0.5, diversity=0.5),
                   s.search("code_chunks", q.tolist(), limit=10, max_overlap=0.5, group_by="file_path"),
                   s.search("code_chunks", q.tolist(), limit=10, max_overlap=0.5, score_threshold=0.1),
                   s.search("code_chunks", None, limit=10, max_overlap=0.5),
                   s.search("code_chunks", q.tolist(), limit=10, max_overlap=0.5, candidates=5),
                   s.search("code_chunks", q.tolist(), limit=10, max_overlap=0.5, candidates=ffi.MAX_K + 1),
                   s.search("summaries", q.tolist(), limit=10, max_overlap=0.5),
                   s.search_batch("code_chunks", q[None], limit=10, max_overlap=0.5, filters=[None]),
                   s.search_batch("code_chunks", q[None], limit=10, max_overlap=0.5, diversity=0.2),
                   s.search_batch("code_chunks", q[None], limit=10, max_overlap=0.5, score_threshold=0.3),
                   s.search("code_chunks", q.tolist(), limit=10, filters={"file_path": {"gte": 3}}),
                   s.search("code_chunks", q.tolist(), limit=10, must_not={"language": {"lt": 3}}),
                   s.search("code_chunks", q.tolist(), limit=10, filters={"start_line": [3, 4]}),
                   s.search("code_chunks", q.tolist(), limit=10, filters={"start_line": "12"}),
                   s.search("code_chunks", q.tolist(), limit=10, filters={"end_line": 3.5}),
                   s.search("code_chunks", q.tolist(), limit=10, filters={"end_line": {"gte": 1, "upto": 9}}),
                   s.search("summaries", q.tolist(), limit=10, filters={"start_line": {"gte": 3}}),
                   s.chunks_at("code_chunks", f3, -1), s.chunks_at("code_chunks", f3, 9, last_line=3), s.chunks_at("summaries", f3, 9),
                   raw_client.count("code_chunks", count_filter=NS(must=[fc("language", gte=1)], must_not=None))]
            res = await asyncio.gather(good, *bad, return_exceptions=True)
            assert _pairs(res[0]) == _brute_pairs(col, stored, qp, files, lo, hi, ids, 10, 500)
            for r in res[1:-1]:
                assert isinstance(r, VectorStoreError) and isinstance(r.cause, ValueError), r
            assert isinstance(res[-1], ValueError)
            named = {14: "file_path", 15: "language", 16: "start_line", 17: "start_line", 18: "end_line", 19: "end_line"}
            for i, key in named.items():
                assert repr(key) in str(res[1 + i].cause), (i, res[1 + i].cause)
            # delete with a range (one device call per shard), then the same through the raw client
            SetFakeIndex.tombstone_calls = 0
            await s.delete("code_chunks", {"file_path": f3, "start_line": {"gte": line}})
            assert SetFakeIndex.tombstone_calls == shards
            gone = (files == 3) & has_lo & (lo >= line)
            assert gone.sum() > 0 and (await s.get_collection_info("code_chunks")).points_count == n - int(gone.sum())
            await raw_client.delete("code_chunks", points_selector=NS(filter=NS(must=[NS(key="file_path", match=NS(value="/proj/f4.py")), fc("end_line", lte=10 ** 6)])))
            gone |= (files == 4) & has_hi
            assert (await s.get_collection_info("code_chunks")).points_count == n - int(gone.sum())
            left = await s.search("code_chunks", None, limit=n)
            assert [h["id"] for h in left] == [ids[i] for i in range(n) if not gone[i]] and order

    asyncio.run(run())


@pytest.mark.parametrize("shards", [1, 2])
def test_format_4_snapshot_is_widened_from_the_payload_tables(monkeypatch, tmp_path, shards):
    """A snapshot written with the numeric columns, stripped back to what the code before them wrote (format 4, ``len(keys)`` code
    columns): it loads, answers a range search, ``chunks_at`` and a ``max_overlap`` search as the original store does, and a save
    writes format 5 again.  (The device half -- ``codes.i32`` as a prefix, ``crh_index_import`` of the widened chunks -- is in
    tests/test_spans_gpu.py.)"""
    from coderag_amd.errors import VectorStoreError
    from coderag_amd.store import HipVectorStore
    _fake_device(monkeypatch)
    raw, files, lo, hi, hot = span_cases.spans_corpus(dim=384, hot_copies=3)
    n = len(raw)
    ids = _ids(n)
    pay = span_cases.payloads(files, lo, hi)
    pay[5]["start_line"], pay[6]["end_line"], pay[7]["start_line"] = "12", None, 2 ** 31       # values the device cannot hold: -1 there, kept in the payload
    q = np.random.default_rng(5).standard_normal(384).astype(np.float32)
    kw = {"shards": shards, "_merge_fn": orc.merge_topk} if shards > 1 else {}
    snap, snap2 = str(tmp_path / "snap"), str(tmp_path / "snap2")

    async def answers(s):
        return (_pairs(await s.search("code_chunks", q.tolist(), limit=20, filters={"start_line": {"gte": 30, "lte": 90}})),
                _pairs(await s.search("code_chunks", q.tolist(), limit=20, max_overlap=0.3)),
                await s.chunks_at("code_chunks", "/proj/f2.py", int(lo[files == 2].max())),
                _pairs(await s.search("code_chunks", q.tolist(), limit=20, must_not={"end_line": {"gte": 0}})))

    async def run():
        async with HipVectorStore(dim=384, dtype="f32", initial_capacity=4096, device=0, compact_dead_fraction=0.0, **kw) as s:
            await _filled(s, ids, raw, pay)
            await s.delete("code_chunks", {"file_path": "/proj/f9.py"})                         # tombstones travel too
            want = await answers(s)
            assert all(len(w) > 0 for w in want)
            await s.save(snap)
            codes_before = [ix.codes.copy() for ix in s._col("code_chunks").shards.index.values()]
        meta = json.load(open(os.path.join(snap, "code_chunks", "collection.json")))
        assert meta["format"] == 5 and meta["numeric_keys"] == ["start_line", "end_line"]
        assert json.load(open(os.path.join(snap, "summaries", "collection.json")))["numeric_keys"] == []
        kept = span_cases.strip_to_format4(snap)
        assert kept == len(meta["keys"]) and "numeric_keys" not in json.load(open(os.path.join(snap, "code_chunks", "collection.json")))
        async with HipVectorStore(dim=384, dtype="f32", initial_capacity=4096, device=0, compact_dead_fraction=0.0, **kw) as s:
            await s.create_collections()
            await s.load(snap)
            col = s._col("code_chunks")
            for ix, before in zip(col.shards.index.values(), codes_before):
                assert ix.codes.shape[1] == kept + 2 and np.array_equal(ix.codes, before)       # the columns are back, value for value
            assert await answers(s) == want
            await s.save(snap2)
        assert json.load(open(os.path.join(snap2, "code_chunks", "collection.json")))["format"] == 5
        async with HipVectorStore(dim=384, dtype="f32", initial_capacity=4096, device=0, compact_dead_fraction=0.0, **kw) as s:
            await s.create_collections()
            await s.load(snap2)
            assert await answers(s) == want
        # a snapshot naming other numeric keys is refused
        path = os.path.join(snap2, "code_chunks", "collection.json")
        meta = json.load(open(path))
        meta["numeric_keys"] = ["start_line"]
        json.dump(meta, open(path, "w"))
        async with HipVectorStore(dim=384, dtype="f32", initial_capacity=4096, device=0, compact_dead_fraction=0.0, **kw) as s:
            await s.create_collections()
            with pytest.raises(VectorStoreError) as e:
                await s.load(snap2)
            assert "numeric" in str(e.value.cause)

    asyncio.run(run())


# ------------------------------------------------------------------ two ranks: fill with -1 + ONE all-reduce(MAX) for the three gathers
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gloo_worker(rank: int, world: int, port: int, out_dir: str) -> None:
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import coderag_amd  # noqa: F401
    from coderag_amd.shards import STRIDE, ShardSet
    from coderag_amd.store import HipVectorStore
    from tests import span_cases
    from tests.test_spans_host import SpanFakeIndex, _brute_pairs, _fake_device, _ids, _pairs
    _fake_device()
    raw, files, lo, hi, hot = span_cases.spans_corpus()                  # the same on every rank
    dim = raw.shape[1]
    sh = ShardSet(world, lambda s: SpanFakeIndex(dim=dim, capacity_rows=8192, n_code_cols=4), backend="dist", block=50, merge_fn=orc.merge_topk)
    shard = sh.route(len(raw))
    codes = np.stack([files, np.zeros_like(files), lo, hi], axis=1).astype(np.int32)
    sh.append({rank: raw[shard == rank]}, codes, shard=shard)
    assert all(r > 0 for r in sh.rows) and sh.index[rank].count()[0] == sh.rows[rank]
    gid = np.empty(len(raw), np.int64)                                   # global row of every input row
    for s in range(world):
        sel = np.flatnonzero(shard == s)
        gid[sel] = s * STRIDE + np.arange(sel.size)
    order = np.argsort(gid)                                              # ties go to the lower GLOBAL row, as the merge orders them
    x = orc.preprocess(raw)
    q = np.concatenate([np.random.default_rng(4).standard_normal((2, dim)).astype(np.float32), raw[[hot]]])
    regimes = set()
    for permille, dfilt in ((500, None), (0, [(2, 10, 300, "between"), (0, [3, 4], True)])):
        passing = None if dfilt is None else span_cases.np_mask(codes, np.ones(len(raw), bool), dfilt)[order]
        scores, rows, info = sh.search_spans(q, 20, MAX_K, (0, 2, 3), permille, dfilt)
        for qi in range(3):
            es, er, total = span_cases.brute_force(x[order], orc.preprocess(q[qi][None])[0], files[order], lo[order], hi[order], 20, permille, passing)
            if info[qi, 0] >= 20 or info[qi, 1] < MAX_K:
                assert np.array_equal(scores[qi].view(np.uint32)[:er.size], es.view(np.uint32)), f"rank {rank}: scores differ"
                assert np.array_equal(rows[qi][:er.size], gid[order][er]) and (rows[qi][er.size:] == -1).all(), f"rank {rank}: rows differ"
            else:                                                        # the hot method's 1100 copies fill the list: a strict prefix of the answer
                kept = int(info[qi, 0])
                assert kept < 20 and np.array_equal(rows[qi][:kept], gid[order][er][:kept]) and (rows[qi][kept:] == -1).all(), f"rank {rank}: {permille} {qi}"
                regimes.add("incomplete")
                continue
            regimes.add("complete")
    assert regimes == {"complete", "incomplete"}, regimes
    # the store, one process per shard: max_overlap, a range filter and chunks_at answer alike on every rank
    import asyncio as aio
    pay = span_cases.payloads(files, lo, hi)
    ids = _ids(len(raw))
    raw384 = np.concatenate([raw, np.zeros((len(raw), 384 - dim), np.float32)], axis=1)
    qv = raw384[11] + 0.1

    async def run():
        async with HipVectorStore(dim=384, dtype="f32", initial_capacity=4096, device=0, shards=world, shard_backend="dist",
                                  compact_dead_fraction=0.0, _merge_fn=orc.merge_topk) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, raw384, pay)
            col = s._col("code_chunks")
            got = await s.search("code_chunks", qv.tolist(), limit=15, max_overlap=0.25, filters={"start_line": {"gte": 5}})
            want = _brute_pairs(col, orc.preprocess(raw384), orc.preprocess(qv[None])[0], files, lo, hi, ids, 15, 250, lo >= 5)
            assert _pairs(got) == want, f"rank {rank}"
            line = int(lo[(files == 6) & (lo >= 0)].max())
            at = await s.chunks_at("code_chunks", "/proj/f6.py", line)
            assert at == [pay[i] for i in range(len(raw)) if files[i] == 6 and lo[i] >= 0 and hi[i] >= 0 and lo[i] <= line <= hi[i]] and at, f"rank {rank}"
    aio.run(run())
    open(os.path.join(out_dir, f"ok{rank}"), "w").write("ok")
    dist.destroy_process_group()


def test_the_three_gathers_complete_over_two_gloo_ranks(tmp_path):
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

    async def chunks_at(self, **kw):
        self.calls.append(("chunks_at", kw))
        return [{"file_path": "a.py", "entity_type": "method", "entity_name": "Repo.save", "language": "python", "content": "def save(): ...",
                 "start_line": 100, "end_line": 140, "graph_node_id": "a.Repo.save", "content_hash": "h"}]


class _Embedder:
    async def embed(self, text):
        return [0.0] * 4

    async def embed_batch(self, texts):
        return [[0.0] * 4 for _ in texts]


def test_searchers_forward_max_overlap_only_when_given():
    from coderag_amd import indexer, mcp_tools, vector_search
    from coderag_amd.errors import QueryError

    async def run():
        rec = _Recorder()
        vs = vector_search.VectorSearcher(rec, _Embedder())
        await vs.search_code("q", limit=3, language="python")
        await vs.find_similar_code("x = 1", limit=3)
        await vs.search_code_batch(["a", "b"], limit=3)
        assert [set(kw) for _, kw in rec.calls] == [{"collection", "query_vector", "limit", "filters"}, {"collection", "query_vector", "limit"},
                                                    {"collection", "query_vectors", "limit", "filters"}]       # today's call shapes
        rec.calls.clear()
        await vs.search_code("q", limit=3, max_overlap=0.5)
        await vs.find_similar_code("x = 1", limit=3, exclude_file="a.py", exact_exclude=True, max_overlap=0.0)
        await vs.search_code_batch(["a", "b"], limit=3, max_overlap=0.25, candidates=64)
        assert [kw["max_overlap"] for _, kw in rec.calls] == [0.5, 0.0, 0.25]
        assert rec.calls[1][1]["must_not"] == {"file_path": "a.py"} and rec.calls[2][1]["candidates"] == 64
        assert all("group_by" not in kw and "diversity" not in kw and "score_threshold" not in kw for _, kw in rec.calls)
        with pytest.raises(ValueError):
            await vs.search_code("q", limit=3, max_overlap=0.5, extra_queries=["other words"])
        rec.calls.clear()
        iv = indexer.VectorSearcher(rec, _Embedder())
        await iv.search_code("q", limit=2, language="python")
        await iv.search_code("q", limit=2, max_overlap=0.4)
        assert "max_overlap" not in rec.calls[0][1] and rec.calls[1][1]["max_overlap"] == 0.4 and "group_by" not in rec.calls[1][1]
        rec.calls.clear()
        rows = await vs.chunks_at("a.py", 120)
        assert rec.calls == [("chunks_at", {"collection": "code_chunks", "file_path": "a.py", "line": 120, "last_line": None})]
        assert rows == [{"score": 0.0, "file_path": "a.py", "entity_type": "method", "entity_name": "Repo.save", "language": "python",
                         "content": "def save(): ...", "start_line": 100, "end_line": 140, "graph_node_id": "a.Repo.save"}]
        await vs.chunks_at("a.py", 100, last_line=160)
        assert rec.calls[-1][1]["last_line"] == 160
        with pytest.raises(QueryError):
            await vs.chunks_at("", 3)

        class Searcher:
            def __init__(self):
                self.kw = []

            async def search_code(self, **kw):
                self.kw.append(kw)
                return []
        sr = Searcher()
        tool = mcp_tools.create_semantic_search_tool(lambda: sr)
        assert (await tool["function"]("find it")).success and (await tool["function"]("find it", limit=3, max_overlap=0.5)).success
        assert sr.kw == [{"query": "find it", "limit": 5, "entity_type": None}, {"query": "find it", "limit": 3, "entity_type": None, "max_overlap": 0.5}]
        assert "max_overlap" in tool["parameters"]

    asyncio.run(run())
