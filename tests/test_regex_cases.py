"""CPU tier of the regular-expression match: the compiler of code-rag_amd/regex_dfa.py against Python's ``re`` on
bytes (a fuzz and hand-written expectations for every assertion), the required-literal extraction, the refusals, and the store's
``{"matches": ...}`` filter parser.  ``RegexDFA.search`` is the table walk the device does, so a failure here is the compiler's,
not the kernel's.  Nothing here needs a device."""
import numpy as np
import pytest

from tests import regex_cases as rc
from tests.fake_index import FakeIndex, fake_device


def _dfa(pattern, case=True):
    from coderag_amd import regex_dfa
    return regex_dfa.compile_regex(pattern, case, "content")


def _agrees(pattern, rows, case=True):
    dfa, want = _dfa(pattern, case), rc.match_rows(rows, pattern, case).tolist()
    got = [dfa.search(r) for r in rows]
    assert got == want, (pattern, case, [r for r, g, w in zip(rows, got, want) if g != w])
    return got


# ---------------------------------------------------------------------------------------------------- compiler against re

def test_compiler_fuzz_against_re():
    """2,000 generated patterns x 30 random rows of 0..14 bytes over ``abAB_1 \\n``; the compiler may refuse at most 2 % of what
    ``re`` accepts (the 256-state cap)."""
    cases = rc.random_cases(seed=20, n=2000)
    assert 0.2 < sum(not case for _, case in cases) / len(cases) < 0.4
    rng = np.random.default_rng(21)
    refused, wrong = [], []
    for pattern, case in cases:
        try:
            dfa = _dfa(pattern, case)
        except ValueError as e:
            assert "'content'" in str(e)
            refused.append(pattern)
            continue
        rx = rc.re_compile(pattern, case)
        for row in rc.random_rows(rng, 30, 14):
            if dfa.search(row) != (rx.search(row) is not None):
                wrong.append((pattern, case, row))
    assert not wrong, wrong[:5]
    assert len(refused) <= 0.02 * len(cases), refused[:5]


def test_line_and_row_anchors():
    assert _agrees("^bar", [b"bar", b"xbar", b"x\nbar", b"foo\n\nbar", b"", b"ba"]) == [True, False, True, True, False, False]
    assert _agrees("foo$", [b"foo", b"foox", b"foo\nx", b"foo\n", b"", b"xfoo"]) == [True, False, True, True, False, True]
    assert _agrees("^$", [b"", b"a", b"a\n", b"\na", b"a\n\nb", b"ab"]) == [True, False, True, True, True, False]
    assert _agrees(r"\Abar", [b"bar", b"x\nbar", b"\nbar"]) == [True, False, False]
    assert _agrees(r"foo\Z", [b"foo", b"foo\n", b"foo\nx", b"xfoo"]) == [True, False, False, True]
    assert _agrees(r"\A\Z", [b"", b"\n", b"a"]) == [True, False, False]
    assert _agrees(r"a$\n^b", [b"a\nb", b"ab", b"a\n\nb"]) == [True, False, False]


def test_word_boundaries_at_both_row_ends_and_on_the_empty_row():
    assert _agrees(r"\bbar", [b"bar", b"xbar", b" bar", b"_bar", b"-bar"]) == [True, False, True, False, True]
    assert _agrees(r"foo\b", [b"foo", b"foox", b"foo ", b"foo1", b"foo."]) == [True, False, True, False, True]
    assert _agrees(r"\Bar", [b"ar", b"bar", b" ar"]) == [False, True, False]
    assert _agrees(r"fo\B", [b"fo", b"foo", b"fo "]) == [False, True, False]
    assert _agrees(r"\B", [b"", b"a", b"ab", b" ", b"a "]) == [False, False, True, True, True]     # (re: never on a zero-byte subject)
    assert _agrees(r"\b", [b"", b"a", b" ", b"  "]) == [False, True, False, False]
    assert _agrees(r"^\B$", [b"", b" "]) == [False, False]
    assert _agrees("a*", [b"", b"b"]) == [True, True]


def test_dot_classes_high_bytes_and_folding():
    assert _agrees("a.b", [b"axb", b"a\nb", b"a\x00b", b"a\xffb", b"ab"]) == [True, False, True, True, False]
    assert _agrees("[^a]", [b"a", b"\x00", b"\x80", b"\xff", b"\n", b"aaa", b""]) == [False, True, True, True, True, False, False]
    assert _agrees("[^a]", [b"A", b"a"], case=False) == [False, False]
    assert _agrees("[a-c]x", [b"Bx", b"bx", b"dx"], case=False) == [True, True, False]
    assert _agrees(r"\w+\s\d", [b"ab_ 1", b"ab-1", "é 1".encode()]) == [True, False, False]              # \w is ASCII
    upper, lower = "É".encode(), "é".encode()
    assert _agrees("caf" + "É", [b"CAF" + upper, b"caf" + lower, b"CAF" + lower], case=False) == [True, False, False]    # É is not folded
    assert _agrees("é+", [lower, lower[:1] + lower[1:] * 3, lower * 2, lower[:1]]) == [True, True, True, False]        # + repeats é's LAST byte
    assert _agrees("\udc80", ["\udc80".encode("utf-8", "surrogatepass"), b"x"]) == [True, False]
    assert _agrees("a{2,}?b|c{2}", [b"aab", b"ab", b"cc", b"c"]) == [True, False, True, False]
    assert _agrees(r"0x[0-9a-fA-F]{8}", [b"0xDEADbeef", b"0xDEADbee", b"0xDEADbeeg"]) == [True, False, False]


def test_issue_patterns_compile_small_and_a_large_dfa_is_accepted():
    for p in (r"def \w+_retry\(", r"^\s*#include\s*<hip/", r"\bTODO\(\w+\)", r"[A-Z][a-z]+Error\b", r"0x[0-9a-fA-F]{8}"):
        d = _dfa(p)
        assert d.n_states <= 64 and d.n_classes <= 32, (p, d.n_states, d.n_classes)
    d = _dfa("a.{5}b")
    assert 100 <= d.n_states <= 256 and d.n_states * d.n_classes <= 32768
    assert d.search(b"xxa12345b") and not d.search(b"a1234b") and not d.search(b"a12\n45b")
    assert d.trans.dtype == np.uint8 and d.trans.size == d.n_states * d.n_classes and d.class_of.shape == (256,)
    assert d.end_class < d.n_classes and int(d.class_of.max()) < d.n_classes and int(d.trans.max()) < d.n_states
    assert (d.trans.reshape(d.n_states, d.n_classes)[d.accept] == d.accept).all()                          # ACCEPT is absorbing
    from coderag_amd import regex_dfa
    assert regex_dfa.compile_regex("a.{5}b") is d                                                           # the LRU keeps it


# ---------------------------------------------------------------------------------------------------- required literals

def test_required_literals_by_hand():
    assert set(_dfa(r"def \w+_retry\(").literals) == {b"def ", b"_retry("}
    assert _dfa(r"def \w+_retry\(").literals[0] == b"_retry("                                              # the longest first
    assert _dfa("foo|bar").literals == ()
    assert _dfa("(abc)?xyz").literals == (b"xyz",)
    assert _dfa("(abc)+x").literals == (b"abc",)
    assert _dfa("[fg]oo.bar").literals == (b"bar",)
    assert _dfa("ab.cd").literals == ()                                                                     # runs under 3 bytes are no use
    assert _dfa("(?:TODO|FIXME): fix").literals == (b": fix",)
    assert _dfa("ToDo_X", case=False).literals == (b"todo_x",)                                              # folded when the case is ignored
    assert _dfa("x" * 100).literals == (b"x" * 64,)
    many = _dfa(".".join("lit%02d" % i + "x" * i for i in range(12))).literals
    assert len(many) == 8 and [len(m) for m in many] == sorted((len(m) for m in many), reverse=True)


def test_required_literals_fuzz_every_match_holds_them():
    rng = np.random.default_rng(31)
    words = ["foo", "retry_", "Error", "ab1", "A_B"]
    with_literals = 0
    for i in range(400):
        parts = [rc.random_pattern(rng) if rng.random() < 0.5 else words[int(rng.integers(0, len(words)))] for _ in range(int(rng.integers(1, 4)))]
        pattern, case = "".join(parts), bool(rng.random() >= 0.3)
        rx = rc.re_compile(pattern, case)
        if rx is None:
            continue
        try:
            dfa = _dfa(pattern, case)
        except ValueError:
            continue
        with_literals += bool(dfa.literals)
        rows = rc.random_rows(rng, 20, 14) + [w.encode() + r for w in words for r in rc.random_rows(rng, 2, 8)]
        rows += [words[int(a)].encode() + r + words[int(b)].encode() for a, b, r in zip(rng.integers(0, 5, 10), rng.integers(0, 5, 10), rc.random_rows(rng, 10, 6))]
        for row in rows:
            if rx.search(row) is not None:
                held = row if case else row.translate(bytes(c + 32 if 65 <= c <= 90 else c for c in range(256)))
                assert all(lit in held for lit in dfa.literals), (pattern, case, row, dfa.literals)
    assert with_literals > 100


# ---------------------------------------------------------------------------------------------------- refusals

@pytest.mark.parametrize("pattern,word", [
    (r"(a)\1", "back-reference"), ("(?=a)b", "look-ahead"), ("(?<=a)b", "look-behind"), ("(?!a)b", "look-ahead"),
    ("(?i)x", "inline flags"), ("(?s)x.", "inline flags"), ("(?i:x)y", "inline flags"), ("(a)(?(1)b|c)", "conditional"),
    ("a{65}", "repeat bound over 64"), ("a{2,65}", "repeat bound over 64"), ("", "empty pattern"), ("x" * 257, "257 bytes"),
    ("é" * 129, "258 bytes"), ("a.{6}b", "more than 256 states"), ("(", "missing )"), ("a**", "multiple repeat"),
])
def test_compiler_refuses_with_the_key_and_the_construct_named(pattern, word):
    with pytest.raises(ValueError) as e:
        _dfa(pattern)
    assert "'content'" in str(e.value) and word in str(e.value)


def test_limits_just_inside():
    assert _dfa("a{64}").n_states <= 256 and _dfa("x" * 200).search(b"y" + b"x" * 200)     # (a literal of n bytes: n + 2 states)
    assert _dfa("[ab]" * 64).search(b"ab" * 32)                                             # 256 bytes of pattern


# ---------------------------------------------------------------------------------------------------- the store's parser

def _store(monkeypatch):
    fake_device(monkeypatch, FakeIndex)
    from coderag_amd import store
    return store


def test_text_spec_with_matches(monkeypatch):
    store = _store(monkeypatch)
    rx = r"def \w+_retry\("
    assert store.text_spec("content", {"matches": rx}) == store.TextSpec((), False, True, rx.encode())
    assert store.text_spec("content", {"matches": rx, "case": False}) == store.TextSpec((), False, False, rx.encode())
    assert store.text_spec("content", {"contains": ["b", "a"], "matches": "x+", "any": True}) == store.TextSpec((b"a", b"b"), True, True, b"x+")
    assert store.text_spec("content", {"contains": "ToDo", "matches": "ToDo", "case": False}) == store.TextSpec((b"todo",), False, False, b"ToDo")
    assert store.text_spec("content", {"matches": "é"}).regex == "é".encode()
    assert store.text_spec("content", {"contains": "a"}) == store.TextSpec((b"a",), False, True) == store.TextSpec((b"a",), False, True, None)
    assert store._is_text({"matches": "x"}) and not store._is_range({"matches": "x"}) and store._is_range({"gte": 1})
    assert store.has_text_condition({"content": {"matches": "x"}}) and store.has_text_condition(None, {"content": {"matches": "x"}})


@pytest.mark.parametrize("spec,word", [
    ({"matches": ""}, "empty pattern"), ({"matches": r"(a)\1"}, "back-reference"), ({"matches": "(?i)x"}, "inline flags"),
    ({"matches": "("}, "missing )"), ({"matches": 5}, "str"), ({"matches": b"a"}, "str"), ({"matches": ["a"]}, "str"),
    ({"matches": "a", "contains": ""}, "0 bytes"), ({"matches": "a", "contains": []}, "0 patterns"), ({"matches": "a", "regex": True}, "unknown word 'regex'"),
    ({"matches": "a", "case": 0}, "case=0"), ({"any": True}, "needs 'contains'"), ({}, "needs 'contains'"),
])
def test_text_spec_refuses_matches_with_the_key_named(monkeypatch, spec, word):
    store = _store(monkeypatch)
    with pytest.raises(ValueError) as e:
        store.text_spec("content", spec)
    assert "'content'" in str(e.value) and word in str(e.value)


def test_filter_keys_separate_regexes_and_flags(monkeypatch):
    store = _store(monkeypatch)
    key = store._filter_key
    a = key({"content": {"matches": "retry_\\w+"}}, None)
    assert a != key({"content": {"matches": "retry_\\w*"}}, None)
    assert a != key({"content": {"matches": "retry_\\w+", "case": False}}, None)
    assert a != key(None, {"content": {"matches": "retry_\\w+"}})
    assert a != key({"content": {"contains": "retry_\\w+"}}, None)
    assert a != key({"content": {"matches": "retry_\\w+", "contains": "retry_"}}, None)
    assert a == key({"content": {"matches": "retry_\\w+", "case": True, "any": False}}, None)
    assert key({"content": {"matches": "ABC", "case": False}}, None) != key({"content": {"matches": "abc", "case": False}}, None)   # (patterns are not folded)
    bad = key({"content": {"matches": "("}}, None)                                      # malformed: a key of its own, no exception here
    assert bad != a and bad == key({"content": {"matches": "("}}, None)


def test_collection_refuses_matches_where_contains_is_refused(monkeypatch):
    store = _store(monkeypatch)
    col = store._Collection("code_chunks", 64, 1, 1024, 0)
    assert col.regex_prefilter is True
    with pytest.raises(ValueError, match="'language'"):
        col.device_filters({"language": {"matches": "py"}})
    with pytest.raises(ValueError, match="'start_line'"):
        col.device_filters(None, {"start_line": {"matches": "1"}})
    with pytest.raises(ValueError, match="'content'"):
        col.device_filters({"content": {"matches": "(?=x)y"}})
    with pytest.raises(ValueError, match="text condition"):
        col.delete({"content": {"matches": "x"}})
    with pytest.raises(ValueError, match="text condition"):
        col.delete({"language": "python"}, {"content": {"matches": "x"}})
    assert col._text == {} and col.text_match_calls == 0                # nothing was built on the way
    col.close()


def test_per_query_filter_lists_refuse_matches(monkeypatch):
    """The store's batch path itself: a per-query list that carries the condition is a ValueError before anything is searched."""
    import asyncio
    store = _store(monkeypatch)
    from coderag_amd.errors import VectorStoreError
    has = {"content": {"matches": "x"}}
    assert store.has_text_condition([None, has]) and store.has_text_condition([{"language": "go"}], [has])
    q = np.ones((2, 768), np.float32)

    async def run():
        async with store.HipVectorStore(dim=768, dtype="f32", initial_capacity=64, device=0) as s:
            await s.create_collections()
            col = s._col("code_chunks")
            for filters, must_not in (([has, None], None), (None, [None, has]), ([{"language": "go"}, has], [None, None])):
                with pytest.raises(VectorStoreError) as e:
                    await s.search_batch("code_chunks", q, 5, filters, must_not)
                assert isinstance(e.value.cause, ValueError) and "per-query filter list" in str(e.value.cause) and "matches" in str(e.value.cause)
            with pytest.raises(VectorStoreError) as e:
                await s.delete("code_chunks", has)
            assert isinstance(e.value.cause, ValueError) and "text condition" in str(e.value.cause)
            assert col._text == {} and col.text_match_calls == 0

    asyncio.run(run())


# ---------------------------------------------------------------------------------------------------- searchers and the MCP tool

def test_searcher_filter_helper_and_mcp_forwarding():
    import asyncio
    import coderag_amd  # noqa: F401
    from coderag_amd import vector_search as vs
    from coderag_amd.mcp_tools import create_semantic_search_tool
    assert vs._contains_filter("content", None, True) == {} == vs._contains_filter("content", None, False)
    assert vs._contains_filter("content", "a", True) == {"content": {"contains": "a"}}                      # as before
    assert vs._contains_filter("content", "a", False) == {"content": {"contains": "a", "case": False}}
    assert vs._contains_filter("content", None, True, "x+") == {"content": {"matches": "x+"}}
    assert vs._contains_filter("summary", ["a", "b"], False, "x+") == {"summary": {"contains": ["a", "b"], "matches": "x+", "case": False}}
    seen = []

    class Searcher:
        async def search_code(self, **kw):
            seen.append(kw)
            return []

    tool = create_semantic_search_tool(lambda: Searcher())
    assert tool["parameters"]["matches"]["type"] == "string" and not tool["parameters"]["matches"]["required"]
    asyncio.run(tool["function"]("q", matches=r"a\d", contains_case=False))
    asyncio.run(tool["function"]("q"))
    asyncio.run(tool["function"]("q", contains_case=False))                 # (alone it asks for nothing)
    assert seen[0] == {"query": "q", "limit": 5, "entity_type": None, "matches": r"a\d", "contains_case": False}
    assert seen[1] == seen[2] == {"query": "q", "limit": 5, "entity_type": None}
