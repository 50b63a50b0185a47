"""CPU tier of the literal text match: the restatement of tests/text_cases.py against hand-written expectations,
the store's ``{"contains": ...}`` filter parser and its ``ValueError``s, the coalescer's keys, and range mappings parsing as
before.  Nothing here needs a device."""
import numpy as np
import pytest

from tests import text_cases as tc
from tests.fake_index import FakeIndex, fake_device


def test_fold_maps_ascii_letters_only():
    assert tc.fold(b"AZaz") == b"azaz"
    assert tc.fold(b"@[`{") == b"@[`{"                                  # the neighbours of A, Z, a, z stay themselves
    assert tc.fold(bytes(range(256)))[0x41:0x5b] == bytes(range(0x61, 0x7b))
    same = [c for c in range(256) if not 0x41 <= c <= 0x5a]
    assert all(tc.fold(bytes([c])) == bytes([c]) for c in same)         # NUL and every byte >= 0x80 among them
    upper, lower = "É".encode(), "é".encode()
    assert tc.fold(upper) == upper != lower
    assert not tc.row_matches(b"caf" + lower, [b"CAF" + upper], fold_case=True)
    assert tc.row_matches(b"caf" + upper, [b"CAF" + upper], fold_case=True)


def test_restatement_against_hand_written_expectations():
    rows = [b"retry_after=3", b"Retry_After=3", b"x.unwrap()", b"", b"#include <hip/hip_runtime.h>", b"aaaa", b"foo", b"bar"]
    assert tc.match_rows(rows, [b"retry_after="]).tolist() == [True, False, False, False, False, False, False, False]
    assert tc.match_rows(rows, [b"retry_after="], fold_case=True).tolist()[:2] == [True, True]
    assert tc.match_rows(rows, [b"RETRY_AFTER="], fold_case=True).tolist()[:2] == [True, True]
    assert tc.match_rows(rows, [b".unwrap()", b"x"]).tolist()[2] and not tc.match_rows(rows, [b".unwrap()", b"y"]).tolist()[2]
    assert tc.match_rows(rows, [b".unwrap()", b"y"], any_of=True).tolist()[2]
    assert tc.match_rows(rows, [b"aaa"]).tolist()[5] and not tc.match_rows(rows, [b"aaaaa"]).any()
    assert not tc.match_rows(rows, [b"foobar"]).any()                   # rows 6 and 7 side by side: never across a row end
    assert tc.match_rows(rows, [b"a"], mask=[False] * 5 + [True, False, False]).tolist() == [False] * 5 + [True, False, False]
    assert not tc.match_rows(rows, [b"a"], mask=np.zeros(8, bool)).any()
    assert not tc.match_rows([b""], [b"a"]).any()


def test_words_and_masks_round_trip():
    rng = np.random.default_rng(1)
    for n in (1, 31, 32, 33, 65, 200):
        m = rng.random(n) < 0.4
        w = tc.words_from_mask(m)
        assert w.dtype == np.uint32 and w.size == (n + 31) // 32
        assert np.array_equal(tc.mask_from_words(w, n), m)
        if n % 32:
            assert int(w[-1]) >> (n % 32) == 0                          # the bits past the last row are 0
    assert tc.words_from_mask([True, False, True]).tolist() == [0b101]


def test_case_generators():
    assert tc.WINDOW == 4 * tc.STEP and tc.STEP == 64 * tc.LANE
    for n in (1, 2, 3, 4, 5, 16, 17, 64):
        p = tc.pattern_of(n)
        assert len(p) == n and len(set(p[:4])) == min(n, 4)
        assert tc.filler(5000, n).find(p[:1]) < 0
    rows = tc.planted_rows(10, 50, [(120, b"X9#"), (499, b"Z")])
    assert [i for i, r in enumerate(rows) if b"X9#" in r] == [2] and rows[9].endswith(b"Z")
    off, blob = tc.csr([b"ab", b"", b"cde"])
    assert off.tolist() == [0, 2, 2, 5] and blob == b"abcde"


# ---------------------------------------------------------------------------------------------------- the store's parser

def _store(monkeypatch):
    fake_device(monkeypatch, FakeIndex)
    from coderag_amd import store
    return store


def test_text_spec_parses_and_normalises(monkeypatch):
    store = _store(monkeypatch)
    assert store.text_spec("content", {"contains": "retry_after="}) == store.TextSpec((b"retry_after=",), False, True)
    assert store.text_spec("content", {"contains": ["unwrap()", "expect("], "any": True}) == store.TextSpec((b"expect(", b"unwrap()"), True, True)
    assert store.text_spec("content", {"contains": "ToDo", "case": False}) == store.TextSpec((b"todo",), False, False)
    assert store.text_spec("content", {"contains": ["a", "a", "b"]}).patterns == (b"a", b"b")
    assert store.text_spec("content", {"contains": "É", "case": False}).patterns == ("É".encode(),)        # no Unicode folding
    assert store.text_spec("content", {"contains": "\udc80"}).patterns == ("\udc80".encode("utf-8", "surrogatepass"),)
    assert store.text_spec("content", {"contains": "x" * 64}).patterns == (b"x" * 64,)
    assert store.TEXT_KEYS == {"code_chunks": ("content",), "summaries": ("summary",)}


@pytest.mark.parametrize("spec,word", [
    ({"contains": ""}, "0 bytes"), ({"contains": ["ok", ""]}, "0 bytes"), ({"contains": "x" * 65}, "65 bytes"),
    ({"contains": "é" * 33}, "66 bytes"), ({"contains": ["a"] * 9}, "9 patterns"), ({"contains": []}, "0 patterns"),
    ({"contains": "a", "regex": True}, "unknown word 'regex'"), ({"contains": "a", "gte": 1}, "unknown word 'gte'"),
    ({"contains": 5}, "str"), ({"contains": ["a", 5]}, "str"), ({"contains": b"a"}, "str"), ({"contains": "a", "any": 1}, "any=1"),
    ({"contains": "a", "case": "no"}, "case='no'"),
])
def test_text_spec_refuses_with_the_key_named(monkeypatch, spec, word):
    store = _store(monkeypatch)
    with pytest.raises(ValueError) as e:
        store.text_spec("content", spec)
    assert "'content'" in str(e.value) and word in str(e.value)


def test_collection_refuses_text_conditions_on_the_wrong_key_and_plain_values_on_a_text_key(monkeypatch):
    store = _store(monkeypatch)
    col = store._Collection("code_chunks", 64, 1, 1024, 0)
    with pytest.raises(ValueError, match="'language'"):
        col.device_filters({"language": {"contains": "py"}})
    with pytest.raises(ValueError, match="'start_line'"):
        col.device_filters(None, {"start_line": {"contains": "1"}})
    with pytest.raises(ValueError, match="'summary'"):                  # the summaries' text key, not the code chunks'
        col.device_filters({"summary": {"contains": "x"}})
    for bad in ("retry", ["a", "b"], {"gte": 3}, None, 7):
        with pytest.raises(ValueError, match="'content'"):
            col.device_filters({"content": bad})
    with pytest.raises(ValueError, match="'content'"):
        col.device_filters(None, {"content": "retry"})
    with pytest.raises(ValueError, match="'content'"):
        col.device_filters({"content": {"contains": ""}})
    with pytest.raises(ValueError, match="text condition"):
        col.delete({"content": {"contains": "x"}})
    with pytest.raises(ValueError, match="text condition"):
        col.delete({"language": "python"}, {"content": {"contains": "x"}})
    assert col._text == {} and col.text_match_calls == 0                # nothing was built on the way
    summaries = store._Collection("summaries", 64, 1, 1024, 0)
    with pytest.raises(ValueError, match="'content'"):
        summaries.device_filters({"content": {"contains": "x"}})
    col.close()
    summaries.close()


def test_filter_keys_separate_patterns_flags_and_ranges(monkeypatch):
    store = _store(monkeypatch)
    key = store._filter_key
    a = key({"content": {"contains": "retry_after="}}, None)
    assert a != key({"content": {"contains": "retry_after"}}, None)                     # two patterns never share a pass
    assert a != key({"content": {"contains": "retry_after=", "case": False}}, None)
    assert a != key(None, {"content": {"contains": "retry_after="}})
    assert a != key({"content": {"contains": ["retry_after=", "x"]}}, None)
    assert key({"content": {"contains": ["a", "b"]}}, None) != key({"content": {"contains": ["a", "b"], "any": True}}, None)
    assert a == key({"content": {"contains": ["retry_after="], "any": False, "case": True}}, None)       # the defaults spelled out
    assert key({"content": {"contains": ["a", "b"]}}, None) == key({"content": {"contains": ["b", "a", "a"]}}, None)
    assert key({"content": {"contains": "ABC", "case": False}}, None) == key({"content": {"contains": "abc", "case": False}}, None)
    assert key({"content": {"contains": "ABC"}}, None) != key({"content": {"contains": "abc"}}, None)
    assert a != key({"content": {"contains": "retry_after="}, "language": "python"}, None)
    bad = key({"content": {"contains": ""}}, None)                                      # malformed: a key of its own, no exception here
    assert bad != a and bad == key({"content": {"contains": ""}}, None)
    assert store.has_text_condition({"content": {"contains": "x"}}) and store.has_text_condition(None, {"content": {"contains": "x"}})
    assert store.has_text_condition([None, {"content": {"contains": "x"}}])
    assert not store.has_text_condition({"language": "python", "start_line": {"gte": 3}}, {"file_path": ["a"]})
    assert not store.has_text_condition(None) and not store.has_text_condition([None, {"language": "go"}], None)


def test_a_plain_range_mapping_still_parses_as_before(monkeypatch):
    store = _store(monkeypatch)
    assert store._is_range({"gte": 3}) and store._is_range({}) and not store._is_range({"contains": "x"}) and not store._is_range(3)
    assert store._is_text({"contains": "x"}) and not store._is_text({"gte": 3}) and not store._is_text("contains")
    assert store._value_key({"gt": 3}) == store._value_key({"gte": 4}) == "range(4, 2147483647)"
    assert store._filter_key({"start_line": {"gt": 3}}, None) == store._filter_key({"start_line": {"gte": 4}}, None)
    col = store._Collection("code_chunks", 64, 1, 1024, 0)
    ncol = len(col.keys)
    assert col.device_filters({"start_line": {"gte": 10, "lt": 20}}) == [(ncol, 10, 19, "between")]
    assert col.device_filters(None, {"end_line": {"lte": 5}}) == [(ncol + 1, 0, 5, "not_between")]
    assert col.device_filters({"start_line": 7}) == [(ncol, 7, 7, "between")]
    with pytest.raises(ValueError, match="unknown bound"):
        col.device_filters({"start_line": {"gte": 1, "between": 2}})
    with pytest.raises(ValueError, match="dictionary-coded"):
        col.device_filters({"language": {"gte": 1}})
    col.close()
