"""Regular-expression match on the device: ``crh_text_regex`` fed by code-rag_amd/regex_dfa.py against Python's
``re`` on each row's own bytes (tests/regex_cases.py) -- the validity words and the count must be equal exactly.  The output
buffer is pre-filled with garbage and carries one guard word behind it that must come back untouched.  The store's
``{"matches": ...}`` filter is compared with the f32 oracle under the rows ``re`` keeps (ids and score BITS).  No tolerance
appears anywhere."""
import ctypes
import re

import numpy as np
import pytest

from tests import regex_cases as rc
from tests import test_text_gpu as tg

pytestmark = pytest.mark.gpu

U32 = np.uint32
GUARD = 0x5A5A5A5A


def _env():
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    return ffi


def _compile(pattern, case=True):
    from coderag_amd import regex_dfa
    return regex_dfa.compile_regex(pattern, case, "content")


def _regex(ffi, t, rows, pattern, case=True, mask=None):
    """One crh_text_regex into a garbage-filled buffer with a guard word behind it, compared with ``re``; returns the bool row mask."""
    import torch
    n = len(rows)
    nw = (n + 31) // 32
    buf = torch.full((nw + 1,), -77, dtype=torch.int32, device="cuda:0")
    buf[nw] = GUARD
    words, count = t.regex(_compile(pattern, case), mask=None if mask is None else tg._dev_words(rc.words_from_mask(mask)), out=buf)
    torch.cuda.synchronize()
    got = words.cpu().numpy().view(U32)
    want = rc.match_rows(rows, pattern, case, mask)
    assert np.array_equal(got[:nw], rc.words_from_mask(want)), (np.flatnonzero(tg.tc.mask_from_words(got[:nw], n) != want)[:10], pattern, case)
    assert int(got[nw]) == GUARD, "the word behind the result was written"
    assert count == int(want.sum())
    return want


def _check(ffi, rows, pattern, **kw):
    t = tg._arena(ffi, rows)
    try:
        return _regex(ffi, t, rows, pattern, **kw)
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------------- rows, tiles and pairs

@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 97, 128])
def test_row_counts_around_the_tile_and_the_pair(gpu, n):
    ffi = _env()
    rows = [rc.filler(1 + (7 * i) % 50, i) + (b"K9x" if i % 3 == 0 else b"K9") for i in range(n)]
    t = tg._arena(ffi, rows)
    want = _regex(ffi, t, rows, r"K\dx$")
    assert int(want.sum()) == (n + 2) // 3
    assert _regex(ffi, t, rows, "K9").all()                              # every row: every bit below `rows`, none at or past it
    assert not _regex(ffi, t, rows, "K8").any()
    t.close()


def _aligned_rows(plant):
    """For every length 0..40 and every start offset 0..15 (mod 16) one row, behind a pad row that brings it there; ``plant(row,
    start)`` writes the match into a copy of the row (or returns it unchanged)."""
    rows, at, planted = [], 0, 0
    for length in range(41):
        for o in range(16):
            pad = (o - at) % 16
            rows.append(rc.filler(pad, 3 * len(rows)))
            at += pad
            assert at % 16 == o
            row = plant(bytearray(rc.filler(length, 7 * len(rows) + 1)), at)
            planted += b"Q" in row
            rows.append(bytes(row))
            at += length
    return rows, planted


def test_every_alignment_and_length_with_a_match_at_the_first_and_last_byte_and_across_a_chunk_edge(gpu):
    ffi = _env()

    def first(row, start):
        if row:
            row[0:1] = b"Q"
        return row

    def last(row, start):
        if row:
            row[-1:] = b"Q"
        return row

    def edge(row, start):                                                # "QZ" with Q on the last byte of a 16-byte chunk
        i = (15 - start) % 16
        if i + 1 < len(row):
            row[i:i + 2] = b"QZ"
        return row

    for plant, pattern, count in ((first, "^Q", 16 * 40), (last, r"Q\Z", 16 * 40), (first, "Q", 16 * 40), (last, "Q", 16 * 40), (edge, "QZ", None)):
        rows, planted = _aligned_rows(plant)
        want = _check(ffi, rows, pattern)
        assert int(want.sum()) == planted == (count if count is not None else planted) > 300


def test_a_match_never_sees_the_neighbouring_row(gpu):
    ffi = _env()
    n = 130
    rows = [rc.filler(40, i) for i in range(n)]
    for a in (3, 31, 63):                                                # inside a tile, across tiles, across pairs
        rows[a] = rows[a][:-3] + b"foo"
        rows[a + 1] = b"bar" + rows[a + 1][3:]
    rows[n - 1] = rows[n - 1][:-3] + b"foo"                              # the arena's very last row ends at its last byte
    t = tg._arena(ffi, rows)
    assert not _regex(ffi, t, rows, "foobar").any()
    assert np.flatnonzero(_regex(ffi, t, rows, "^bar")).tolist() == [4, 32, 64]
    assert np.flatnonzero(_regex(ffi, t, rows, r"\Abar")).tolist() == [4, 32, 64]
    assert np.flatnonzero(_regex(ffi, t, rows, "foo$")).tolist() == [3, 31, 63, n - 1]
    assert np.flatnonzero(_regex(ffi, t, rows, r"foo\Z")).tolist() == [3, 31, 63, n - 1]
    assert np.flatnonzero(_regex(ffi, t, rows, r"\bbar")).tolist() == [4, 32, 64]
    assert np.flatnonzero(_regex(ffi, t, rows, r"foo\b")).tolist() == [3, 31, 63, n - 1]
    assert not _regex(ffi, t, rows, r"foo\B").any() and not _regex(ffi, t, rows, r"\Bbar").any()
    assert not _regex(ffi, t, rows, r"foo\n?bar").any()
    t.close()


def test_empty_rows_a_tile_and_a_pair_of_them(gpu):
    ffi = _env()
    rows = [b"", b"a", b"", b"\n", b"ab", b" ", b""] + [b"x"] * 25       # tile 0: mixed
    rows += [b""] * 32                                                  # tile 1: empty rows only
    rows += [b""] * 64                                                  # pair 1: empty rows only
    rows += [b"", b"a\n\nb", b"b", b""]
    t = tg._arena(ffi, rows)
    want = _regex(ffi, t, rows, "^$")
    assert want[0] and want[3] and not want[1] and want[32:128].all() and want[129] and not want[130]
    assert _regex(ffi, t, rows, "a*").all()
    want = _regex(ffi, t, rows, r"\B")
    assert not want[0] and not want[32:128].any() and want[4] and want[5] and not want[1]     # (re: never on a zero-byte row)
    want = _regex(ffi, t, rows, r"\b")
    assert not want[0] and want[1] and not want[32:128].any()
    _regex(ffi, t, rows, "x")
    t.close()
    _check(ffi, [b""] * 40, "a")
    _check(ffi, [b""] * 40, r"\A\Z")


def _random_arena(n=300, max_len=60, seed=11):
    return rc.random_rows(np.random.default_rng(seed), n, max_len)


def test_masks_zero_words_partial_words_and_no_mask(gpu):
    ffi = _env()
    rows = _random_arena(200)
    t = tg._arena(ffi, rows)
    rng = np.random.default_rng(8)
    every = _regex(ffi, t, rows, r"\w")
    assert every.sum() > 150
    one_of_a_pair = np.ones(200, bool)
    one_of_a_pair[32:64] = False                                        # pair 0: its second word 0, over rows that DO match
    one_of_a_pair[64:96] = False                                        # pair 1: its first word 0
    one_of_a_pair[192:] = False                                         # the last, partial word
    got = _regex(ffi, t, rows, r"\w", mask=one_of_a_pair)
    assert not got[32:96].any() and not got[192:].any() and got[:32].any() and got[96:128].any()
    both = np.ones(200, bool)
    both[0:64] = False                                                  # pair 0: both words 0
    both[128:192] = False
    got = _regex(ffi, t, rows, r"\w", mask=both)
    assert not got[:64].any() and got[64:128].any() and not got[128:192].any() and got[192:].any()
    _regex(ffi, t, rows, r"a\s", mask=rng.random(200) < 0.5)
    _regex(ffi, t, rows, r"a\s", mask=rng.random(200) < 0.03)
    _regex(ffi, t, rows, r"\w", mask=np.zeros(200, bool))
    _regex(ffi, t, rows, r"\w", mask=np.ones(200, bool))
    t.close()


def test_tombstoned_rows_arrive_through_the_index_row_mask(gpu):
    import torch
    ffi = _env()
    n = 200
    rows = _random_arena(n, seed=6)
    t = tg._arena(ffi, rows)
    rng = np.random.default_rng(2)
    idx = ffi.Index(384, ffi.DTYPE_BF16, capacity_rows=n, n_code_cols=1)
    codes = rng.integers(0, 3, (n, 1)).astype(np.int32)
    idx.append(rng.standard_normal((n, 384)).astype(np.float32), codes)
    dead = np.sort(rng.choice(n, 60, replace=False))
    idx.tombstone(dead)
    alive = np.ones(n, bool)
    alive[dead] = False
    for conds, keep in ((None, alive), ([(0, [1, 2], False)], alive & (codes[:, 0] > 0))):
        mask = idx.row_mask(conds)
        out = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device="cuda:0")
        words, count = t.regex(_compile(r"[ab]+_"), mask=mask, out=out)
        want = rc.match_rows(rows, r"[ab]+_", True, keep)
        assert np.array_equal(words.cpu().numpy().view(U32), rc.words_from_mask(want)) and count == int(want.sum()) > 0
    idx.close()
    t.close()


def test_one_64_kb_row_among_short_ones_in_the_same_wave(gpu):
    ffi = _env()
    big = bytearray(rc.filler(64 * 1024, 5))
    big[50_000:50_004] = b"X9#Q"
    rows = [rc.filler(30, i) for i in range(40)]
    rows[13] = bytes(big)
    rows[14] = b"X9#" + rows[14]                                        # all but the last byte
    rows[39] = rows[39] + b"X9#Q"
    want = _check(ffi, rows, r"X\d#Q")
    assert np.flatnonzero(want).tolist() == [13, 39]
    rows[13] = bytes(big[:50_000]) + bytes(big[50_004:])                # the long row without it: the rows behind still answer
    want = _check(ffi, rows, r"X\d#Q")
    assert np.flatnonzero(want).tolist() == [39]


def test_dfa_sizes_and_bytes_that_are_no_ascii(gpu):
    ffi = _env()
    rows = _random_arena(150, seed=4) + [b"a\x00b", b"\x00", b"aaa", b"a\x80", b"\xff\xfe", b"a\na", b"\n", "é".encode(), b"a12345b", b"xa1\n345b",
                                          b"Retry_After_Seconds_Total=17;  // ToDo", b"retry_after_seconds_total=;//todo"]
    t = tg._arena(ffi, rows)
    assert _compile("a").n_states <= 8
    _regex(ffi, t, rows, "a")
    assert _compile("a.{5}b").n_states >= 100
    want = _regex(ffi, t, rows, "a.{5}b")
    assert want[158] and not want[159]
    big = r"retry_after_seconds_total=[0-9]+;\s*//\s*todo"
    assert _compile(big, False).n_states >= 40
    want = _regex(ffi, t, rows, big, case=False)
    assert want[160] and not want[161] and not _regex(ffi, t, rows, big).any()
    want = _regex(ffi, t, rows, "[^a]")
    assert want[150] and want[151] and not want[152] and want[153] and want[154] and want[155]
    want = _regex(ffi, t, rows, ".")
    assert want[151] and not want[156] and want[157]
    _regex(ffi, t, rows, r"a.\Z")
    _regex(ffi, t, rows, "[^a]", case=False)
    t.close()


def test_invalid_tables_are_refused_and_leave_the_handle_usable(gpu):
    import torch
    ffi = _env()
    L = ffi.lib()
    rows = [b"alpha", b"beta", b"", b"a"]
    t = tg._arena(ffi, rows)
    out = torch.zeros((1,), dtype=torch.int32, device="cuda:0")
    cnt = ctypes.c_int64(-5)
    # the hand-made DFA of "holds an a": state 0 searching, state 1 = accept; classes: 0 other, 1 'a', 2 END
    class_of = np.zeros(256, np.uint8)
    class_of[ord("a")] = 1
    good = np.asarray([[0, 1, 0], [1, 1, 1]], np.uint8)

    def raw(n_states, n_classes, trans, end_class=2, accept=1, cls=class_of):
        trans = np.ascontiguousarray(trans, np.uint8).reshape(-1)
        return L.crh_text_regex(t._handle(), n_states, n_classes, cls.ctypes.data, end_class, trans.ctypes.data, accept, None, out.data_ptr(), ctypes.byref(cnt), 0)

    assert raw(2, 3, [[0, 2, 0], [1, 1, 1]]) == ffi.E_INVALID            # a state id out of range
    assert b"state" in L.crh_last_error()
    assert raw(2, 3, [[0, 1, 0], [1, 0, 1]]) == ffi.E_INVALID            # the accept row is not absorbing
    assert b"absorbing" in L.crh_last_error()
    assert raw(200, 200, np.zeros(40000, np.uint8), end_class=199, accept=0) == ffi.E_INVALID      # over CRH_REGEX_MAX_TABLE_BYTES
    assert raw(2, 1, [[0], [1]], end_class=0) == ffi.E_INVALID           # n_classes 1
    assert raw(0, 3, good) == ffi.E_INVALID and raw(257, 3, np.zeros(257 * 3, np.uint8)) == ffi.E_INVALID
    assert raw(2, 3, good, end_class=3) == ffi.E_INVALID and raw(2, 3, good, accept=2) == ffi.E_INVALID
    bad_cls = class_of.copy()
    bad_cls[200] = 3
    assert raw(2, 3, good, cls=bad_cls) == ffi.E_INVALID
    assert cnt.value == 0
    assert raw(2, 3, good) == ffi.OK and cnt.value == 3
    torch.cuda.synchronize()
    assert int(out.cpu().numpy().view(U32)[0]) == 0b1011
    with pytest.raises(ffi.NativeError):                                  # the binding: a table that is not n_states x n_classes
        t.regex(_compile("a")._replace(n_states=9))
    _regex(ffi, t, rows, "a")
    assert ffi.REGEX_MAX_STATES == 256 and ffi.REGEX_MAX_TABLE_BYTES == 32768
    t.clear()
    words, count = t.regex(_compile("a"))
    assert count == 0 and words.numel() == 0
    t.close()


def test_fuzz_200_patterns_over_one_arena(gpu):
    ffi = _env()
    rows = _random_arena(300, 60, seed=13)
    t = tg._arena(ffi, rows, pieces=3)
    done = hits = 0
    for pattern, case in rc.random_cases(seed=40, n=230):
        try:
            _compile(pattern, case)
        except ValueError:
            continue                                                    # (over the state cap: the CPU tier bounds how many)
        hits += int(_regex(ffi, t, rows, pattern, case).sum())
        done += 1
        if done == 200:
            break
    assert done == 200 and hits > 5000
    t.close()


# ---------------------------------------------------------------------------------------------------- the store

RX_LITERAL = r"retry_after=[a-z]"          # required literal: "retry_after="
RX_PLAIN = r"^(?:todo|TODO)\("             # no required literal (an alternation), anchored at a line
RX_END = r"[a-z]\.unwrap\(\)$"


def _rx_holds(p, pattern, case=True):
    text = p.get("content")
    return isinstance(text, str) and rc.row_matches(text.encode("utf-8", "surrogatepass"), pattern, case)


@pytest.mark.parametrize("shards", [1, 2])
def test_store_regex_filters_end_to_end(gpu, shards):
    import asyncio
    ffi = _env()
    from coderag_amd.errors import VectorStoreError
    from coderag_amd.store import HipVectorStore
    n_all, dim = tg.STORE_N, tg.STORE_DIM
    pay = tg._chunks()
    rng = np.random.default_rng(23)
    raw = rng.standard_normal((n_all, dim)).astype(np.float32)
    ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(n_all)]
    q = rng.standard_normal((3, dim)).astype(np.float32)
    has = {"content": {"matches": RX_LITERAL}}

    async def same_as_brute(s, col, filters, must_not, keep_fn, k=10):
        got = await s.search_batch("code_chunks", q, k, filters, must_not)
        want_ids, want_s, n = tg._brute(col, q, k, keep_fn)
        for i in range(len(q)):
            assert tg._ids(got[i]) == want_ids[i], (filters, must_not)
            assert np.array_equal(np.asarray([h["score"] for h in got[i]], np.float32).view(U32), want_s[i][: len(got[i])].view(U32))
        return n

    async def run():
        async with HipVectorStore(dim=dim, dtype="bf16", initial_capacity=4096, device=0, shards=shards, compact_dead_fraction=0.0) as s:
            await s.create_collections()
            for a in range(0, n_all, 500):
                await s.upsert("code_chunks", ids[a:a + 500], raw[a:a + 500], pay[a:a + 500])
            col = s._col("code_chunks")
            n = await same_as_brute(s, col, has, None, lambda p: _rx_holds(p, RX_LITERAL))
            assert 50 < n < len(range(0, n_all, 7))
            assert await same_as_brute(s, col, None, has, lambda p: not _rx_holds(p, RX_LITERAL)) == n_all - n       # absent / no str: passes must_not
            m = await same_as_brute(s, col, {"content": {"matches": RX_PLAIN}, "language": "python"}, None,
                                    lambda p: _rx_holds(p, RX_PLAIN) and p["language"] == "python")
            assert m > 10
            both = {"content": {"matches": RX_END, "contains": tg.NEEDLE}}
            assert await same_as_brute(s, col, both, None, lambda p: _rx_holds(p, RX_END) and tg._holds(p, tg.NEEDLE)) > 10
            nocase = {"content": {"matches": r"^todo\(", "case": False}}
            assert await same_as_brute(s, col, nocase, has, lambda p: _rx_holds(p, r"^todo\(", False) and not _rx_holds(p, RX_LITERAL)) > m
            await same_as_brute(s, col, {"content": {"matches": "no such string anywhere"}}, None, lambda p: False)

            # a repeated identical call does not run the matcher again; another expression does
            first = await s.search("code_chunks", q[0].tolist(), 10, has)
            calls, native = col.text_match_calls, ffi.Text.regex_calls
            again = await s.search("code_chunks", q[0].tolist(), 10, has)
            assert col.text_match_calls == calls and ffi.Text.regex_calls == native and tg._equal_hits(first, again)
            await s.search("code_chunks", q[0].tolist(), 10, {"content": {"matches": RX_LITERAL + "?"}})
            assert col.text_match_calls == calls + 1 and ffi.Text.regex_calls == native + shards

            # the literal prefilter changes no word: on (one crh_text_match per shard in front of the walk) and off (none)
            def words_of(prefilter):
                col._text_cache.clear()
                col.regex_prefilter = prefilter
                greps = ffi.Text.match_calls
                cond = col.device_filters(has)[-1]
                assert ffi.Text.match_calls - greps == (shards if prefilter else 0)
                return [cond.words[id(col.shards.index[sh])].cpu().numpy() for sh in col.shards.owned]
            on, off = words_of(True), words_of(False)
            assert all(np.array_equal(a, b) for a, b in zip(on, off)) and sum(int(np.unpackbits(a.view(np.uint8)).sum()) for a in on) == n
            del col.regex_prefilter

            # search_text: hits in insertion order, the exact count, the line where the first match starts
            out = await s.search_text("code_chunks", matches=RX_LITERAL, limit=25)
            want = [i for i in range(n_all) if _rx_holds(pay[i], RX_LITERAL)]
            assert out["count"] == len(want) == n and tg._ids(out["hits"]) == [ids[i] for i in want[:25]]
            for h in out["hits"]:
                text = h["payload"]["content"].encode()
                assert h["match_line"] == h["payload"]["start_line"] + text[: re.search(RX_LITERAL.encode(), text).start()].count(b"\n") and h["score"] == 0.0
            out = await s.search_text("code_chunks", tg.NEEDLE2, limit=5, filters={"language": "rust"}, matches=r"^TODO\(", case=False)
            want = [i for i in range(n_all) if pay[i]["language"] == "rust" and tg._holds(pay[i], tg.NEEDLE2, case=False) and _rx_holds(pay[i], r"^TODO\(", False)]
            assert out["count"] == len(want) > 5 and tg._ids(out["hits"]) == [ids[i] for i in want[:5]]
            assert all(h["match_line"] == h["payload"]["start_line"] for h in out["hits"])           # (the expression matches in the first line)
            # strings and expression together: the line of whichever is found FIRST -- here the string (in any line) comes before
            # the expression's match (in the last line) in most hits, and behind it in none that shares its line
            out = await s.search_text("code_chunks", tg.NEEDLE, limit=60, matches=RX_END)
            want = [i for i in range(n_all) if tg._holds(pay[i], tg.NEEDLE) and _rx_holds(pay[i], RX_END)]
            assert out["count"] == len(want) > 10 and tg._ids(out["hits"]) == [ids[i] for i in want[:60]]
            apart = 0
            for h in out["hits"]:
                text = h["payload"]["content"].encode()
                at_string, at_regex = text.find(tg.NEEDLE.encode()), re.search(RX_END.encode(), text, re.MULTILINE).start()
                assert h["match_line"] == h["payload"]["start_line"] + text[: min(at_string, at_regex)].count(b"\n")
                apart += text[:at_string].count(b"\n") != text[:at_regex].count(b"\n")
            assert apart > 5                                                                        # (the two definitions differ on these)
            assert await s.count_text("code_chunks", matches=RX_LITERAL) == n and await s.count_text("code_chunks", matches="nowhere at all") == 0

            # refused with a ValueError: per-query filter lists and deletes that carry the condition, and what the compiler refuses
            for call in (lambda: s.search_batch("code_chunks", q, 5, [has, None, None]), lambda: s.search_batch("code_chunks", q, 5, None, [None, has, None]),
                         lambda: s.delete("code_chunks", has), lambda: s.search("code_chunks", q[0].tolist(), 5, {"language": {"matches": "py"}}),
                         lambda: s.search("code_chunks", q[0].tolist(), 5, {"content": {"matches": r"(a)\1"}}),
                         lambda: s.search_text("code_chunks", matches=""), lambda: s.search_text("code_chunks"), lambda: s.search_text("code_chunks", matches="a.{6}b")):
                with pytest.raises(VectorStoreError) as e:
                    await call()
                assert isinstance(e.value.cause, ValueError), e.value
            assert (await s.get_collection_info("code_chunks")).points_count == n_all

    asyncio.run(run())


def test_searcher_matches(gpu):
    import asyncio
    _env()
    from coderag_amd.store import HipVectorStore
    from coderag_amd.vector_search import VectorSearcher
    pay = tg._chunks()[:400]
    rng = np.random.default_rng(29)
    raw = rng.standard_normal((400, tg.STORE_DIM)).astype(np.float32)
    ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(400)]

    class Embedder:
        async def embed(self, text):
            return raw[5].tolist()

    async def run():
        async with HipVectorStore(dim=tg.STORE_DIM, dtype="bf16", initial_capacity=1024, device=0) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, raw, pay)
            vs = VectorSearcher(s, Embedder())
            got = await vs.search_code("anything", limit=10, matches=RX_LITERAL)
            want = await s.search("code_chunks", raw[5].tolist(), 10, {"content": {"matches": RX_LITERAL}})
            assert len(got) == 10 and [g["entity_name"] for g in got] == [h["payload"]["entity_name"] for h in want]
            assert all(re.search(RX_LITERAL, g["content"]) for g in got)
            got = await vs.search_code("anything", limit=10, language="rust", matches=r"^todo\(", contains=tg.NEEDLE2, contains_case=False)
            assert got and all(g["language"] == "rust" and g["content"].lower().startswith("todo(") and tg.NEEDLE2 in g["content"] for g in got)

    asyncio.run(run())
