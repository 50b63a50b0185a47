"""CPU tier of the approximate substring match: the restatement of tests/fuzzy_cases.py against a brute force
over all substrings, the store's ``{"fuzzy": ..., "edits": ...}`` parser and its refusals, the coalescer's keys, the store's
plumbing over a fake ``Text`` (levels fetched in order, counts per distance, the cache, the pigeonhole pieces, the refusals),
the new entry point's export and argument checks, and the MCP tools' parameters.  Nothing here needs a device."""
import asyncio
import ctypes

import numpy as np
import pytest

from tests import fuzzy_cases as fc
from tests.fake_index import FakeIndex, fake_device


# ---------------------------------------------------------------------------------------------------- the restatement

def test_restatement_against_brute_force_over_all_substrings():
    rng = np.random.default_rng(4)
    seen = set()
    for _ in range(400):
        p = bytes(rng.choice(np.frombuffer(b"abc", np.uint8), size=int(rng.integers(1, 6))))
        t = bytes(rng.choice(np.frombuffer(b"abc\n", np.uint8), size=int(rng.integers(0, 10))))
        got = fc.distance_end(t, p)
        assert got == fc.brute_distance_end(t, p), (p, t)
        seen.add(got[0])
    assert seen >= {0, 1, 2, 3}


def test_restatement_against_hand_written_expectations():
    d = fc.distance_end
    assert d(b"def parse_retry_after(x):", b"parse_retry_aftr") == (1, 19)          # "parse_retry_aft" (the r deleted) ends first
    assert d(b"def parse_retry_after(x):", b"parse_retry_after") == (0, 21)
    assert d(b"class HTTPServerError:", b"HTTPServerEror") == (1, 19)
    assert d(b"x = parseRetryAfter()", b"parse_retry_after")[0] == 4               # two substitutions, two deletions
    assert d(b"x = parseRetryAfter()", b"parse_retry_after", True)[0] == 2          # folded: the two deletions remain
    assert d(b"", b"abc") == (3, 0) and d(b"zzzz", b"abc") == (3, 0)                # the empty row: distance m
    assert d(b"ab", b"abc") == (1, 2) and d(b"a", b"abc") == (2, 1)                 # rows shorter than the pattern
    assert d(b"xbay", b"ab")[0] == 1                                                # a transposition: "b" or "a" alone is 1 away ...
    assert d(b"xbay", b"abcd")[0] == 3 and d(b"xbacdy", b"abcd")[0] == 1            # (... "acd" is one deletion away)
    assert d(b"__badc__", b"abcd")[0] == 2                                          # two transpositions side by side: "bad" + 1, not 4
    assert d(b"x = cafe;", "café".encode())[0] == 2                            # bytes: the two bytes of e-acute against one
    assert d("CAFÉ".encode(), "café".encode(), True)[0] == 1              # non-ASCII is not folded: one byte differs
    lv = fc.levels([b"abcd", b"abxd", b"axxd", b"", b"abcd"], b"abcd", 2, mask=[True, True, True, True, False])
    assert lv.tolist() == [[True, False, False, False, False], [True, True, False, False, False], [True, True, True, False, False]]
    assert fc.level_words(lv).tolist() == [[1], [3], [7]]
    assert fc.match_line("a\nb\nparse_retry_after\nz", 10, "parse_retry_aftr") == 12


def test_case_builders():
    for n in (1, 4, 31, 32, 33, 62):
        p = fc.distinct_pattern(n)
        assert len(p) == n == len(set(p)) and not set(p) & set(fc.filler(4000, n)) and 0x7E not in p and 0x7C not in p
    p = fc.distinct_pattern(12)
    for i in (0, 6, 11):
        assert fc.levenshtein(p, fc.substitute(p, i)) == 1 and fc.levenshtein(p, fc.insert(p, i)) == 1 and fc.levenshtein(p, fc.delete(p, i)) == 1
    assert fc.levenshtein(p, fc.transpose(p, 5)) == 2 and fc.insert(p, 12) == p + b"~"


# ---------------------------------------------------------------------------------------------------- the store's parser

def _store(monkeypatch, **stand_ins):
    fake_device(monkeypatch, stand_ins.pop("index", FakeIndex), **stand_ins)
    from coderag_amd import store
    return store


def test_text_spec_with_fuzzy(monkeypatch):
    store = _store(monkeypatch)
    spec = store.text_spec
    assert spec("content", {"fuzzy": "parse_retry_aftr"}) == store.TextSpec((), False, True, None, b"parse_retry_aftr", 2)
    assert [spec("content", {"fuzzy": "x" * n}).edits for n in (1, 2, 5, 6, 64)] == [0, 1, 1, 2, 2]       # the defaults by length
    assert [store.default_edits(n) for n in (1, 2, 5, 6, 64)] == [0, 1, 1, 2, 2]
    assert spec("content", {"fuzzy": "HTTPServerEror", "edits": 1, "case": False}) == store.TextSpec((), False, False, None, b"httpservereror", 1)
    assert spec("content", {"fuzzy": "abcd", "edits": 3}).edits == 3 and spec("content", {"fuzzy": "abcd", "edits": 0}).edits == 0
    assert spec("content", {"fuzzy": "abcd", "edits": np.int64(2)}).edits == 2
    assert spec("content", {"fuzzy": "Éa", "case": False}).fuzzy == "Éa".encode()                  # no Unicode folding
    both = spec("content", {"contains": ["b", "a"], "matches": "x+", "fuzzy": "retry", "any": True})
    assert both == store.TextSpec((b"a", b"b"), True, True, b"x+", b"retry", 1)
    # specs without the new words are the 3- and 4-field specs of before
    assert spec("content", {"contains": "a"}) == store.TextSpec((b"a",), False, True) == store.TextSpec((b"a",), False, True, None)
    assert spec("content", {"matches": "x+"}) == store.TextSpec((), False, True, b"x+") == store.TextSpec((), False, True, b"x+", None, 0)
    assert store._is_text({"fuzzy": "x"}) and not store._is_range({"fuzzy": "x"}) and not store._is_text({"edits": 1})
    assert store.has_text_condition({"content": {"fuzzy": "x"}}) and store.has_text_condition(None, {"content": {"fuzzy": "x"}})
    assert store.has_text_condition([None, {"content": {"fuzzy": "x"}}]) and not store.has_text_condition({"language": "go"})


@pytest.mark.parametrize("spec,word", [
    ({"fuzzy": 5}, "'fuzzy' takes a str"), ({"fuzzy": b"abc"}, "'fuzzy' takes a str"), ({"fuzzy": ["abc"]}, "'fuzzy' takes a str"),
    ({"fuzzy": ""}, "0 bytes"), ({"fuzzy": "x" * 65}, "65 bytes"), ({"fuzzy": "é" * 33}, "66 bytes"),
    ({"fuzzy": "abcd", "edits": 4}, "edits=4"), ({"fuzzy": "abcd", "edits": -1}, "edits=-1"), ({"fuzzy": "abcd", "edits": True}, "edits=True"),
    ({"fuzzy": "abcd", "edits": 1.0}, "edits=1.0"), ({"fuzzy": "abcd", "edits": "1"}, "edits='1'"),
    ({"fuzzy": "ab", "edits": 2}, "not more than edits=2"), ({"fuzzy": "a", "edits": 1}, "not more than edits=1"), ({"fuzzy": "abc", "edits": 3}, "not more than edits=3"),
    ({"contains": "a", "edits": 1}, "'edits' stands beside 'fuzzy'"), ({"fuzzy": "abcd", "distance": 1}, "unknown word 'distance'"),
    ({"fuzzy": "abcd", "case": 0}, "case=0"), ({"fuzzy": "abcd", "contains": ""}, "0 bytes"), ({"fuzzy": "abcd", "matches": "("}, "missing )"),
    ({"any": True}, "'fuzzy' (a string within 'edits' edits)"),
])
def test_text_spec_refuses_fuzzy_with_the_key_named(monkeypatch, spec, word):
    store = _store(monkeypatch)
    with pytest.raises(ValueError) as e:
        store.text_spec("content", spec)
    assert "'content'" in str(e.value) and word in str(e.value)


def test_filter_keys_separate_pattern_edits_and_case(monkeypatch):
    store = _store(monkeypatch)
    key = store._filter_key
    a = key({"content": {"fuzzy": "parse_retry"}}, None)
    assert a != key({"content": {"fuzzy": "parse_retri"}}, None)
    assert a != key({"content": {"fuzzy": "parse_retry", "edits": 1}}, None)
    assert a != key({"content": {"fuzzy": "parse_retry", "case": False}}, None)
    assert a != key(None, {"content": {"fuzzy": "parse_retry"}})
    assert a != key({"content": {"contains": "parse_retry"}}, None) and a != key({"content": {"matches": "parse_retry"}}, None)
    assert a != key({"content": {"fuzzy": "parse_retry", "contains": "parse"}}, None)
    assert a == key({"content": {"fuzzy": "parse_retry", "edits": 2, "case": True, "any": False}}, None)      # the defaults spelled out
    assert key({"content": {"fuzzy": "ABCD", "case": False}}, None) == key({"content": {"fuzzy": "abcd", "case": False}}, None)
    assert key({"content": {"fuzzy": "ABCD"}}, None) != key({"content": {"fuzzy": "abcd"}}, None)
    bad = key({"content": {"fuzzy": "ab", "edits": 3}}, None)                           # malformed: a key of its own, no exception here
    assert bad != a and bad == key({"content": {"fuzzy": "ab", "edits": 3}}, None)


def test_pigeonhole_pieces(monkeypatch):
    store = _store(monkeypatch)
    pieces = store.fuzzy_pieces
    assert pieces(b"parse_retry_after", 0) == ()                                        # no edits: the walk is the grep
    assert pieces(b"parse_retry_after", 1) == (b"parse_re", b"try_after")
    for pattern, k in ((b"parse_retry_after", 1), (b"parse_retry_after", 2), (b"HTTPServerEror", 3), (b"abcdefghi", 2), (bytes(range(64)), 3)):
        got = pieces(pattern, k)
        cut = sorted(got, key=pattern.find)
        assert len(got) == k + 1 and b"".join(cut) == pattern and min(map(len, got)) >= 3 and max(map(len, got)) - min(map(len, got)) <= 1
    assert pieces(b"abcdefgh", 2) == () and pieces(b"abcde", 1) == () and pieces(b"abcdef", 1) == (b"abc", b"def")      # a piece under 3 bytes: no prefilter
    assert pieces(b"abcabc", 1) == (b"abc",)                                            # equal pieces are one pattern
    # the argument itself, on random strings: whatever lies within k edits of the pattern holds one of the pieces verbatim
    rng = np.random.default_rng(8)
    alphabet = np.frombuffer(b"abcdefgh", np.uint8)
    checked = 0
    for _ in range(300):
        k = int(rng.integers(1, 4))
        pattern = bytes(rng.choice(alphabet, size=int(rng.integers(3 * (k + 1), 20))))
        text = bytearray(pattern)
        for _ in range(k):                                                              # k random edits, then noise on both sides
            i = int(rng.integers(0, len(text) + 1))
            kind = int(rng.integers(0, 3))
            if kind == 0 and i < len(text):
                text[i] = int(rng.choice(alphabet))
            elif kind == 1:
                text.insert(i, int(rng.choice(alphabet)))
            elif i < len(text):
                del text[i]
        text = bytes(rng.choice(alphabet, size=3)) + bytes(text) + bytes(rng.choice(alphabet, size=3))
        if fc.distance_end(text, pattern)[0] <= k:
            assert any(p in text for p in pieces(pattern, k)), (pattern, text, k)
            checked += 1
    assert checked > 250


# ---------------------------------------------------------------------------------------------------- the store over a fake Text

class WordsIndex(FakeIndex):
    """FakeIndex that also answers ``row_mask`` and takes row-bitmap conditions (numpy words in place of device tensors)."""
    fetches = []          # (conditions as (kind, tag) / (col, code), limit) of every match_rows
    SET_CONDITIONS = True  # (takes a filter as it is: row bitmaps travel with the set conditions)

    def _mask(self, filters=None):
        from coderag_amd import ffi
        ok = self.alive.astype(bool).copy()
        for item in (filters or []):
            if isinstance(item, ffi.RowWords):
                w = item.words[id(self)] if isinstance(item.words, dict) else item.words
                bits = fc.mask_from_words(np.asarray(w).view(np.uint32), len(ok)) if len(ok) else ok
                ok &= ~bits if item.negate else bits
            elif len(item) == 3:                                         # (column, codes, negate)
                ok &= np.isin(self.codes[:, item[0]], list(item[1])) != bool(item[2])
            else:
                ok &= self.codes[:, item[0]] == item[1]
        return ok

    def search(self, queries, k, filters=None, row_base=0, **kw):
        from oracle import search as orc
        q = orc.preprocess(np.asarray(queries, np.float32), to_bf16=(self.dtype == 1))
        s, r = orc.search(self.x, q, k, alive=self._mask(filters).astype(np.uint8))
        return s, np.where(r >= 0, r + row_base, r)

    def row_mask(self, filters=None, stream=0):
        return fc.words_from_mask(self._mask(filters)).view(np.int32)

    def match_rows(self, filters=None, limit=1):
        from coderag_amd import ffi
        WordsIndex.fetches.append(([("not" if f.negate else "is", f.tag) if isinstance(f, ffi.RowWords) else tuple(f) for f in (filters or [])], limit))
        return np.flatnonzero(self._mask(filters))[:limit].astype(np.int64)


class FakeText:
    """``ffi.Text`` on the host: the restatements of tests/text_cases.py and tests/fuzzy_cases.py behind the binding's methods."""
    calls = []            # ("match", patterns, fold, any) / ("fuzzy", pattern, edits, fold, rows under the mask)
    match_calls = regex_calls = fuzzy_calls = 0

    def __init__(self, capacity_rows=0, capacity_bytes=0, device=0):
        self.rows = []

    def count(self):
        return len(self.rows), sum(map(len, self.rows))

    def append(self, row_off, data):
        data = bytes(data)
        self.rows += [data[a:b] for a, b in zip(row_off[:-1], row_off[1:])]

    def _bits(self, mask):
        return np.ones(len(self.rows), bool) if mask is None else fc.mask_from_words(np.asarray(mask).view(np.uint32), len(self.rows))

    def match(self, patterns, fold_case=False, any_of=False, mask=None, out=None, count=True, stream=0):
        from tests import text_cases as tc
        FakeText.calls.append(("match", tuple(patterns), fold_case, any_of))
        got = tc.match_rows(self.rows, list(patterns), fold_case, any_of, self._bits(mask))
        return fc.words_from_mask(got).view(np.int32), (int(got.sum()) if count else None)

    def fuzzy(self, pattern, edits, fold_case=False, mask=None, out=None, count=True, stream=0):
        bits = self._bits(mask)
        FakeText.calls.append(("fuzzy", bytes(pattern), edits, fold_case, int(bits.sum())))
        lv = fc.levels(self.rows, pattern, edits, fold_case, bits)
        return fc.level_words(lv).view(np.int32), ([int(m.sum()) for m in lv] if count else None)

    def close(self):
        pass


PATTERN = "parse_retry_after"


def _payloads(n=90):
    """Chunk i holds the pattern with i % 5 edits (4: nothing alike) in its line 1 + i % 3; chunk 7 has no content."""
    p = PATTERN.encode()
    forms = [p, fc.delete(p, 15), fc.substitute(fc.substitute(p, 0), 9), fc.insert(fc.delete(fc.substitute(p, 3), 8), 12), b"nothing alike here"]
    assert [fc.distance_end(f, p)[0] for f in forms[:4]] == [0, 1, 2, 3]
    pay = []
    for i in range(n):
        lines = [fc.filler(20, 3 * i + j).decode().replace("\n", " ") for j in range(4)]
        lines[1 + i % 3] = lines[1 + i % 3][:5] + forms[i % 5].decode() + lines[1 + i % 3][5:]
        pay.append({"file_path": f"src/m{i % 4}.py", "entity_type": "function", "entity_name": f"fn_{i}", "language": "python" if i % 2 else "rust",
                    "content": "\n".join(lines), "start_line": 10 * i, "end_line": 10 * i + 3, "project_name": "demo"})
    del pay[7]["content"]
    return pay


def _dist(p):
    return fc.distance_end(p["content"].encode(), PATTERN)[0] if isinstance(p.get("content"), str) else 99


@pytest.mark.parametrize("shards", [1, 2])
def test_store_plumbing_over_a_fake_text(monkeypatch, shards):
    store = _store(monkeypatch, index=WordsIndex, Text=FakeText)
    from coderag_amd import ffi
    from coderag_amd.errors import VectorStoreError
    FakeText.calls.clear()
    WordsIndex.fetches.clear()
    n, dim = 90, 64
    pay = _payloads(n)
    ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(n)]
    vecs = np.random.default_rng(2).standard_normal((n, dim)).astype(np.float32)
    dist = np.asarray([_dist(p) for p in pay])

    async def run():
        from oracle import search as orc
        kw = {"shards": shards, "_merge_fn": orc.merge_topk} if shards > 1 else {}
        async with store.HipVectorStore(dim=dim, dtype="f32", initial_capacity=256, device=0, **kw) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, vecs, pay)
            col = s._col("code_chunks")

            # the order: (distance, insertion order), fetched level by level -- level d as the condition, level d - 1 negated
            out = await s.search_text("code_chunks", fuzzy=PATTERN, limit=30)
            want = sorted((i for i in range(n) if dist[i] <= 2), key=lambda i: (dist[i], i))
            by = [int((dist == d).sum()) for d in range(3)]
            assert out["count"] == len(want) == sum(by) and out["counts_by_distance"] == by and min(by) >= 17
            assert [h["id"] for h in out["hits"]] == [ids[i] for i in want[:30]]
            assert [h["distance"] for h in out["hits"]] == [int(dist[i]) for i in want[:30]]
            for h in out["hits"]:
                i = ids.index(h["id"])
                assert h["match_line"] == pay[i]["start_line"] + 1 + i % 3 == fc.match_line(pay[i]["content"], pay[i]["start_line"], PATTERN) and h["score"] == 0.0
            walks = [c for c in FakeText.calls if c[0] == "fuzzy"]
            assert len(walks) == shards and all(c[1:4] == (PATTERN.encode(), 2, False) for c in walks)
            fetched = [f for f in WordsIndex.fetches]
            assert len(fetched) == 2 * shards                                         # level 0 gives 18, level 1 the other 12: level 2 is not fetched
            (c0, l0), (c1, l1) = fetched[0], fetched[shards]
            assert l0 == 30 and l1 == 30 - by[0] and len(c0) == 1 and c0[0][0] == "is" and len(c1) == 2
            assert c1[0][0] == "is" and c1[1] == ("not", c0[0][1]) and c1[0][1] != c0[0][1]

            # the same filter again: the walk is not repeated (count_text, a search under the condition, search_text with another limit)
            calls = col.text_match_calls
            assert await s.count_text("code_chunks", fuzzy=PATTERN) == len(want)
            assert len(await s.search("code_chunks", vecs[0].tolist(), 5, {"content": {"fuzzy": PATTERN}})) == 5
            full = await s.search_text("code_chunks", fuzzy=PATTERN, limit=1000, edits=2)
            assert [h["id"] for h in full["hits"]] == [ids[i] for i in want] and col.text_match_calls == calls
            assert len([c for c in FakeText.calls if c[0] == "fuzzy"]) == shards
            assert (await s.search_text("code_chunks", fuzzy=PATTERN, limit=0))["hits"] == []

            # other edits: another walk; every level is fetched when the limit asks for it
            out = await s.search_text("code_chunks", fuzzy=PATTERN, edits=3, limit=1000, filters={"language": "python"})
            want3 = sorted((i for i in range(n) if dist[i] <= 3 and i % 2), key=lambda i: (dist[i], i))
            assert [h["id"] for h in out["hits"]] == [ids[i] for i in want3] and col.text_match_calls == calls + 1
            assert out["counts_by_distance"] == [sum(1 for i in want3 if dist[i] == d) for d in range(4)] and out["count"] == len(want3)
            assert await s.count_text("code_chunks", fuzzy=PATTERN, edits=0) == by[0]
            none = await s.search_text("code_chunks", fuzzy="zzzzzzzzzzzz", edits=1)
            assert none == {"hits": [], "count": 0, "counts_by_distance": [0, 0]}
            assert (await s.search_text("code_chunks", fuzzy=PATTERN, filters={"language": "cobol"})) == {"hits": [], "count": 0, "counts_by_distance": [0, 0, 0]}

            # the prefilter: one any-of grep for the k + 1 pieces in front of the walk, which then sees fewer rows and finds the same
            FakeText.calls.clear()
            col._text_cache.clear()
            on = await s.search_text("code_chunks", fuzzy=PATTERN, limit=1000)
            greps = [c for c in FakeText.calls if c[0] == "match"]
            assert len(greps) == shards and all(c[1:] == (store.fuzzy_pieces(PATTERN.encode(), 2), False, True) for c in greps)
            assert sum(c[4] for c in FakeText.calls if c[0] == "fuzzy") < n - 10
            FakeText.calls.clear()
            col._text_cache.clear()
            col.fuzzy_prefilter = False
            off = await s.search_text("code_chunks", fuzzy=PATTERN, limit=1000)
            assert not [c for c in FakeText.calls if c[0] == "match"] and sum(c[4] for c in FakeText.calls if c[0] == "fuzzy") == n
            assert [h["id"] for h in on["hits"]] == [h["id"] for h in off["hits"]] == [ids[i] for i in want] and on["counts_by_distance"] == off["counts_by_distance"]
            del col.fuzzy_prefilter
            FakeText.calls.clear()
            await s.search_text("code_chunks", fuzzy="retry", limit=5)                 # 5 bytes, 1 edit: pieces of 2 bytes -- no prefilter
            assert [c[0] for c in FakeText.calls] == ["fuzzy"] * shards

            # beside contains: the grep first, the walk under its words
            FakeText.calls.clear()
            out = await s.search_text("code_chunks", "QQQ", fuzzy=PATTERN, limit=5)
            assert out["count"] == 0 and FakeText.calls[0][0] == "match" and FakeText.calls[0][1] == (b"QQQ",)
            out = await s.search_text("code_chunks", "_after", fuzzy=PATTERN, limit=1000, case=False)
            want_c = sorted((i for i in range(n) if dist[i] <= 2 and isinstance(pay[i].get("content"), str) and "_after" in pay[i]["content"]), key=lambda i: (dist[i], i))
            assert [h["id"] for h in out["hits"]] == [ids[i] for i in want_c] and 0 < len(want_c) < len(want)

            # under must_not the condition is negated like every text condition
            got = await s.search("code_chunks", None, 1000, None, {"content": {"fuzzy": PATTERN, "edits": 1}})
            assert sorted(h["id"] for h in got) == sorted(ids[i] for i in range(n) if dist[i] > 1)

            # a text condition of its own under must_not joins every fetch, and the rows per distance are counted under it
            for other, gone in (({"contains": PATTERN}, lambda i: dist[i] == 0), ({"fuzzy": PATTERN, "edits": 1}, lambda i: dist[i] <= 1),
                                ({"fuzzy": PATTERN}, lambda i: True), ({"contains": "fn_"}, lambda i: False)):
                not_this = {"content": other, "language": "rust"}
                out = await s.search_text("code_chunks", fuzzy=PATTERN, limit=1000, must_not=not_this)
                want_m = sorted((i for i in range(n) if dist[i] <= 2 and i % 2 and not gone(i)), key=lambda i: (dist[i], i))
                assert [h["id"] for h in out["hits"]] == [ids[i] for i in want_m] and out["count"] == len(want_m), other
                assert out["counts_by_distance"] == [sum(1 for i in want_m if dist[i] == d) for d in range(3)]
                assert [h["distance"] for h in out["hits"]] == [int(dist[i]) for i in want_m]
                assert await s.count_text("code_chunks", fuzzy=PATTERN, must_not=not_this) == len(want_m)
                got = await s.search("code_chunks", None, 1000, {"content": {"fuzzy": PATTERN}}, not_this)
                assert sorted(h["id"] for h in got) == sorted(ids[i] for i in want_m)
            few = await s.search_text("code_chunks", fuzzy=PATTERN, limit=20, must_not={"content": {"contains": PATTERN}})
            want_f = sorted((i for i in range(n) if 1 <= dist[i] <= 2), key=lambda i: (dist[i], i))
            assert [h["id"] for h in few["hits"]] == [ids[i] for i in want_f[:20]] and few["counts_by_distance"] == [0, by[1], by[2]]

            # refused where the other text conditions are
            has = {"content": {"fuzzy": PATTERN}}
            q = np.ones((2, dim), np.float32)
            for call in (lambda: s.search_batch("code_chunks", q, 5, [has, None]), lambda: s.search_batch("code_chunks", q, 5, None, [None, has]),
                         lambda: s.delete("code_chunks", has), lambda: s.delete("code_chunks", {"language": "rust"}, has),
                         lambda: s.search("code_chunks", q[0].tolist(), 5, {"language": {"fuzzy": "py"}}),
                         lambda: s.search_text("code_chunks", fuzzy="ab", edits=2), lambda: s.search_text("code_chunks", edits=2),
                         lambda: s.search_text("code_chunks", "x", edits=2), lambda: s.search_text("code_chunks", fuzzy=PATTERN, filters=has)):
                with pytest.raises(VectorStoreError) as e:
                    await call()
                assert isinstance(e.value.cause, ValueError), e.value
            assert (await s.get_collection_info("code_chunks")).points_count == n
            assert ffi.FUZZY_MAX_EDITS == 3

    asyncio.run(run())


def test_dist_backend_refuses_fuzzy(monkeypatch):
    store = _store(monkeypatch, index=WordsIndex, Text=FakeText)
    from coderag_amd.errors import VectorStoreError
    col = store._Collection("code_chunks", 64, 1, 1024, 0)
    col.shards.backend = "dist"
    with pytest.raises(VectorStoreError, match="dist"):
        col.device_filters({"content": {"fuzzy": "parse_retry"}})
    col.shards.backend = "local"
    with pytest.raises(ValueError, match="text condition"):
        col.delete({"content": {"fuzzy": "parse_retry"}})
    with pytest.raises(ValueError, match="'language'"):
        col.device_filters({"language": {"fuzzy": "py"}})
    with pytest.raises(ValueError, match="'content'"):
        col.device_filters({"content": {"edits": 1}})
    assert col.fuzzy_prefilter is True and col.text_match_calls == 0
    col.close()


# ---------------------------------------------------------------------------------------------------- the entry point, the searchers, the tools

def test_entry_point_is_exported_declared_and_checks_its_arguments_without_a_device():
    import pathlib
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    root = pathlib.Path(__file__).resolve().parents[1]
    header = (root / "include" / "coderag_hip.h").read_text()
    assert "crh_text_fuzzy" in ffi.EXPORTS and "int crh_text_fuzzy(" in header and "#define CRH_FUZZY_MAX_EDITS 3" in header
    assert "#define CRH_ABI_VERSION 4" in header and ffi.ABI_VERSION == 4 and ffi.FUZZY_MAX_EDITS == 3
    L = ffi.lib()
    assert hasattr(L, "crh_text_fuzzy") and L.crh_abi_version() == 4
    pat = (ctypes.c_uint8 * 8)(*b"abcdefgh")
    counts = (ctypes.c_int64 * 4)(7, 7, 7, 7)
    fuzzy = L.crh_text_fuzzy
    # the arguments are checked before the handle is looked at, so every refusal can be seen here; each names what it refuses
    for args, word in (((pat, 0, 0), b"len=0"), ((pat, 65, 1), b"len=65"), ((pat, -1, 0), b"len=-1"), ((pat, 8, 4), b"max_edits=4"), ((pat, 8, -1), b"max_edits=-1"),
                       ((pat, 3, 3), b"not above max_edits=3"), ((pat, 1, 1), b"not above max_edits=1"), ((None, 8, 1), b"pat_host is NULL"),
                       ((pat, 8, 1), b"handle is NULL"), ((pat, 1, 0), b"handle is NULL"), ((pat, 64, 3), b"handle is NULL")):
        assert fuzzy(None, args[0], args[1], args[2], 0, None, None, counts, None) == ffi.E_INVALID and word in L.crh_last_error(), (args[1:], L.crh_last_error())
    assert list(counts) == [7, 7, 7, 7]                                    # a refused call writes nothing


def test_searcher_filter_helper_and_mcp_forwarding():
    import coderag_amd  # noqa: F401
    from coderag_amd import vector_search as vs
    from coderag_amd.mcp_tools import create_code_facets_tool, create_semantic_search_tool
    assert vs._contains_filter("content", None, True) == {} == vs._contains_filter("content", None, False, None, None, None)
    assert vs._contains_filter("content", "a", True) == {"content": {"contains": "a"}}                      # as before
    assert vs._contains_filter("content", None, True, "x+") == {"content": {"matches": "x+"}}               # as before
    assert vs._contains_filter("content", None, True, None, "retry_aftr") == {"content": {"fuzzy": "retry_aftr"}}
    assert vs._contains_filter("summary", "a", False, "x+", "retry", 1) == {"summary": {"contains": "a", "matches": "x+", "fuzzy": "retry", "edits": 1, "case": False}}
    seen = []

    class Searcher:
        async def search_code(self, **kw):
            seen.append(kw)
            return []

        async def facet_code(self, **kw):
            seen.append(kw)
            return {"hits": [], "values": 0, "total": 0}

    tool = create_semantic_search_tool(lambda: Searcher())
    facets = create_code_facets_tool(lambda: Searcher())
    for t in (tool, facets):
        assert t["parameters"]["fuzzy"]["type"] == "string" and t["parameters"]["edits"]["type"] == "integer"
        assert not t["parameters"]["fuzzy"]["required"] and not t["parameters"]["edits"]["required"]
    asyncio.run(tool["function"]("q", fuzzy="parse_retry_aftr", edits=1, contains_case=False))
    asyncio.run(tool["function"]("q", fuzzy="parse_retry_aftr"))
    asyncio.run(tool["function"]("q"))
    asyncio.run(tool["function"]("q", edits=2))                             # (alone it asks for nothing)
    asyncio.run(facets["function"](fuzzy="HTTPServerEror", edits=2))
    assert seen[0] == {"query": "q", "limit": 5, "entity_type": None, "fuzzy": "parse_retry_aftr", "edits": 1, "contains_case": False}
    assert seen[1] == {"query": "q", "limit": 5, "entity_type": None, "fuzzy": "parse_retry_aftr"}
    assert seen[2] == seen[3] == {"query": "q", "limit": 5, "entity_type": None}
    assert seen[4] == {"key": "file_path", "limit": 10, "fuzzy": "HTTPServerEror", "edits": 2}
