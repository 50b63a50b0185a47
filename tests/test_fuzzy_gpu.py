"""Approximate substring match on the device: every level's words and counts of ``crh_text_fuzzy`` against the
restatement of tests/fuzzy_cases.py (Sellers' table per row) -- equal exactly, word for word.  The output buffer is pre-filled
with garbage and carries one guard word behind it that must come back untouched.  The store's ``{"fuzzy": ...}`` filter is
compared with the f32 oracle under the rows the restatement keeps (ids and score BITS), ``search_text(fuzzy=...)`` with the
restatement's order, distances and lines.  No tolerance appears anywhere."""
import ctypes
import functools
import re

import numpy as np
import pytest

from tests import fuzzy_cases as fc
from tests import test_text_gpu as tg

pytestmark = pytest.mark.gpu

U32 = np.uint32
GUARD = 0x5A5A5A5A


def _env():
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    return ffi


def _fuzzy(ffi, t, rows, pattern, k, fold=False, mask=None, dist=None):
    """One crh_text_fuzzy into a garbage-filled buffer with a guard word behind it, compared with the restatement level by level;
    returns the rows' distances (the restatement's)."""
    import torch
    n = len(rows)
    nw = (n + 31) // 32
    buf = torch.full(((k + 1) * nw + 1,), -77, dtype=torch.int32, device="cuda:0")
    buf[-1] = GUARD
    lv, counts = t.fuzzy(pattern, k, fold_case=fold, mask=None if mask is None else tg._dev_words(fc.words_from_mask(mask)),
                         out=buf[:(k + 1) * nw].view(k + 1, nw))
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(U32)
    dist = fc.distances(rows, pattern, fold) if dist is None else dist
    want = fc.levels(rows, pattern, k, fold, mask, dist=dist)
    for d in range(k + 1):
        level = got[d * nw:(d + 1) * nw]
        assert np.array_equal(level, fc.words_from_mask(want[d])), (d, np.flatnonzero(fc.mask_from_words(level, n) != want[d])[:10], pattern, k, fold)
    assert int(got[-1]) == GUARD, "the word behind the result was written"
    assert counts == [int(m.sum()) for m in want]
    assert lv.shape == (k + 1, nw)
    return dist


def _check(ffi, rows, pattern, k, **kw):
    t = tg._arena(ffi, rows)
    try:
        return _fuzzy(ffi, t, rows, pattern, k, **kw)
    finally:
        t.close()


def _variants(p: bytes) -> list:
    """(the distance of a pattern without a repeated byte, the edited pattern): the pattern itself; one substitution,
    insertion, deletion at the first, middle and last byte; a transposition there; two and three edits apart from each other;
    four.  The match is a SUBSTRING's: a byte put in front of the pattern or behind it costs nothing, and a transposition at
    either end costs 1 (the outer byte is left out), 2 everywhere else."""
    m = len(p)
    at = sorted({0, m // 2, m - 1})
    out = [(0, p)]
    for i in at:
        out += [(1, fc.substitute(p, i)), (1 if i else 0, fc.insert(p, i)), (1, fc.delete(p, i))]
    out.append((0, fc.insert(p, m)))
    if m >= 2:
        out += [(2 if 0 < i < m - 2 else 1, fc.transpose(p, i)) for i in sorted({0, (m - 1) // 2, m - 2}) if p[i] != p[i + 1]]
    if m >= 6:
        out += [(2, fc.substitute(fc.delete(p, m - 2), 1)), (2, fc.insert(fc.insert(p, m // 2), 1)),
                (3, fc.substitute(fc.delete(fc.insert(p, m - 1), m // 2), 0)), (3, fc.substitute(fc.substitute(fc.substitute(p, m - 1), m // 2), 0)),
                (4, fc.substitute(fc.substitute(fc.substitute(fc.substitute(p, m - 1), m // 2), 2), 0))]
    return out


# ---------------------------------------------------------------------------------------------------- lengths, edits, edit kinds

@pytest.mark.parametrize("m", [1, 2, 3, 4, 31, 32, 33, 63, 64])
def test_pattern_lengths_at_the_state_word_edges_every_edit_kind_and_every_k(gpu, m):
    ffi = _env()
    p = fc.distinct_pattern(m, seed=m)
    made, rows = [], []
    for i, (edits, v) in enumerate(_variants(p)):
        for lead, tail in ((0, 0), (5 + i, 9), (37, 0)):                   # alone in the row, in the middle, at the row's end
            made.append(edits)
            rows.append(fc.filler(lead, 2 * i) + v + fc.filler(tail, 2 * i + 1))
    rows += [fc.filler(70, 99), b"", p[: m // 2], p[m // 2:]]               # nothing alike, the empty row, the halves in neighbouring rows
    t = tg._arena(ffi, rows)
    dist = fc.distances(rows, p)
    if 6 <= m <= 62:                                                       # (no byte twice: an edit of the pattern is as far away as it was made to be)
        assert dist[: len(made)].tolist() == made and dist[len(made)] == m and dist[len(made) + 1] == m
    assert set(dist.tolist()) >= ({0, 1, 2, 3, 4} if m >= 6 else {0, 1})
    for k in range(min(m - 1, 3) + 1):                                     # m = k + 1 is among them for m <= 4
        _fuzzy(ffi, t, rows, p, k, dist=dist)
    t.close()


def test_a_transposition_costs_two_and_the_carry_crosses_the_halves_of_the_64_bit_state(gpu):
    ffi = _env()
    p = fc.distinct_pattern(48, seed=5)
    rows = [fc.filler(3, i) + fc.transpose(p, i) + fc.filler(4, i + 100) for i in range(47)]        # every position, 31|32 among them
    rows += [fc.filler(2, i) + fc.delete(p, i) + b"  " for i in range(48)] + [fc.insert(p, i) for i in range(49)]
    rows += [p[:32] + b"~~" + p[32:], p[:31] + p[33:], p[:30] + b"~" + p[30:33] + p[34:]]            # edits on both sides of bit 31 / 32
    dist = _check(ffi, rows, p, 3)
    assert (dist[1:46] == 2).all() and dist[0] == dist[46] == 1                                      # (at either end the outer byte is left out)
    assert (dist[47:95] == 1).all() and (dist[96:143] == 1).all() and dist[95] == dist[143] == 0 and dist[-3:].tolist() == [2, 2, 2]
    _check(ffi, rows, p, 1, dist=dist)
    # a pattern of equal bytes: the addition of the column step carries through all 64 bits
    for m in (32, 33, 64):
        q = b"a" * m
        runs = [b"a" * n for n in (0, 1, m - 4, m - 3, m - 2, m - 1, m, m + 5)] + [b"a" * (m - 20) + b"b" + b"a" * 19, b"b".join([b"a" * (m // 3)] * 3)]
        dist = _check(ffi, runs, q, 3)
        assert dist[:8].tolist() == [m, m - 1, 4, 3, 2, 1, 0, 0] and dist[8] == 1


# ---------------------------------------------------------------------------------------------------- rows, alignment, tiles

def test_empty_short_and_exact_rows_matches_at_both_row_ends_and_none_across_rows(gpu):
    ffi = _env()
    p = fc.distinct_pattern(12, seed=2)
    for k in range(4):
        cut = p[: 12 - k]                                                  # exactly m - k bytes: k deletions away
        rows = [b"", cut, cut[:-1], p[k:], p[k + 1:], b"", b"", p + fc.filler(30, 1), fc.filler(30, 2) + p, fc.delete(p, 0) + fc.filler(9, 3),
                fc.filler(9, 4) + fc.delete(p, 11), fc.filler(20, 5) + p[:6], p[6:] + fc.filler(20, 6), p[:6], p[6:], p[:11], p[11:], b"", p]
        dist = _check(ffi, rows, p, k)
        assert dist[:5].tolist() == [12, k, k + 1, k, k + 1] and dist[7:11].tolist() == [0, 0, 1, 1]
        assert dist[11:15].tolist() == [6, 6, 6, 6] and dist[15:].tolist() == [1, 11, 12, 0]      # a pattern split over two rows is in neither
    rows = [b""] * 70                                                      # a pair of tiles of empty rows, and a third
    assert (_check(ffi, rows, p, 3) == 12).all()


@pytest.mark.parametrize("m,k", [(8, 1), (40, 3)])
def test_every_row_start_mod_16_and_a_match_across_every_chunk_boundary(gpu, m, k):
    ffi = _env()
    p = fc.distinct_pattern(m, seed=7)
    near = fc.substitute(p, m // 2)
    rows, at = [], 0
    for o in range(16):
        for lead in range(0, 17, 1 if m == 8 else 4):                      # the match begins at every offset of a chunk: it crosses every boundary it can
            pad = (o - at) % 16
            rows.append(fc.filler(pad, 3 * len(rows)))                     # (the pad row brings the next row's first byte to offset o)
            at += pad
            assert at % 16 == o
            row = fc.filler(lead, len(rows)) + (near if (o + lead) % 3 == 0 else p) + fc.filler((o * 5 + lead) % 23, len(rows) + 1)
            rows.append(row)
            at += len(row)
    dist = _check(ffi, rows, p, k)
    assert (dist[1::2] <= 1).all() and (dist[1::2] == 1).sum() > 20 and (dist[0::2] >= m - 3).all()


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 129])
def test_row_counts_around_the_tile_and_the_pair(gpu, n):
    ffi = _env()
    p = fc.distinct_pattern(9, seed=3)
    forms = [p, fc.delete(p, 4), fc.substitute(fc.insert(p, 2), 7), b"none"]
    rows = [fc.filler(1 + (7 * i) % 50, i) + forms[i % 4] + fc.filler(i % 5, i + 1) for i in range(n)]
    t = tg._arena(ffi, rows)
    dist = _fuzzy(ffi, t, rows, p, 2)
    assert dist.tolist() == [(0, 1, 2, 9)[i % 4] if i % 4 < 3 else dist[i] for i in range(n)] and (dist[3::4] > 3).all()
    _fuzzy(ffi, t, rows, p, 0, dist=dist)
    full = [r + p for r in rows]                                           # every row: every bit below `rows`, none at or past it
    t2 = tg._arena(ffi, full)
    assert (_fuzzy(ffi, t2, full, p, 1) == 0).all()
    t.close()
    t2.close()


@pytest.mark.parametrize("total", [4096, 8192])
def test_the_arenas_last_row_hard_against_the_slack(gpu, total):
    """The arena's buffer holds 4096 bytes (doubling from there) and kTextSlack zeroed bytes behind them: rows that fill it to its
    last byte, the last one ending in the match, at every start offset mod 16 of that last row."""
    ffi = _env()
    p = fc.distinct_pattern(10, seed=4)
    for last_len in range(10, 27):
        body = total - last_len
        rows = [fc.filler(100, i) for i in range(body // 100)] + [fc.filler(body % 100, 77)]
        rows.append(fc.filler(last_len - 10, 5) + fc.substitute(p, 9 if last_len % 2 else 0))
        assert sum(map(len, rows)) == total
        dist = _check(ffi, rows, p, 2)
        assert dist[-1] == 1 and (dist[:-1] >= 7).all()


def test_high_bytes_and_case_folding_of_ascii_letters_only(gpu):
    ffi = _env()
    p = "naïve_Größe_Ünïcode".encode()                                     # 24 bytes, 5 of them pairs >= 0x80
    assert len(p) == 24 and sum(b >= 0x80 for b in p) == 10
    texts = ["naïve_Größe_Ünïcode", "NAÏVE_GRÖSSE_ÜNÏCODE", "naive_Große_Ünïcode", "naïve_größe_ünïcode", "NaÏvE_gRöSsE", "naïve_Größe_Ünïcod",
             "xx naïve_Grösse_Ünïcode yy", "", "ÿ" * 30, "\x00" * 20]
    rows = [fc.filler(i, i) + s.encode() + fc.filler(2 * i % 7, i + 50) for i, s in enumerate(texts)] + [bytes(range(128, 256)), bytes([0xC3]) * 40 + bytes([0xAF, 0xB6, 0x9C])]
    t = tg._arena(ffi, rows)
    exact = _fuzzy(ffi, t, rows, p, 3)
    folded = _fuzzy(ffi, t, rows, p, 3, fold=True)
    assert exact[0] == 0 and folded[0] == 0 and exact[3] == 2 and folded[3] == 1       # "größe_ünïcode": g folds, u-umlaut stays one byte away
    assert exact[1] == 16 and folded[1] == 5                               # upper case: 11 ASCII letters fold; the 3 two-byte letters and sharp s against SS do not
    assert exact[2] == 4 and exact[5] == 1 and folded[6] == 2              # two bytes against one: a substitution and a deletion each
    hi = bytes(range(0x80, 0x80 + 33))                                      # a 33-byte pattern of high bytes only: the 64-bit state, the upper half of the table
    assert _fuzzy(ffi, t, rows, hi, 2)[10] == 0
    _fuzzy(ffi, t, rows, "GRÖSSE".encode(), 2, fold=True)
    _fuzzy(ffi, t, rows, b"\x00\x00\x00\x00", 1)
    t.close()


# ---------------------------------------------------------------------------------------------------- masks and properties

def test_masks_zero_pairs_zero_tiles_single_rows_and_no_mask(gpu):
    ffi = _env()
    p = fc.distinct_pattern(14, seed=6)
    forms = [p, fc.delete(p, 3), fc.transpose(p, 8), fc.filler(14, 1)]
    n = 32 * 7 + 9
    rows = [fc.filler(i % 40, i) + forms[(i // 3) % 4] + fc.filler(i % 7, i + 1) for i in range(n)]     # matching text in every tile
    t = tg._arena(ffi, rows)
    dist = _fuzzy(ffi, t, rows, p, 2)
    rng = np.random.default_rng(5)
    masks = {"pair 1 (tiles 2, 3) off": np.ones(n, bool), "tile 4 off": np.ones(n, bool), "single rows off": np.ones(n, bool),
             "only the last tile": np.zeros(n, bool), "random": rng.random(n) < 0.5, "nothing": np.zeros(n, bool)}
    masks["pair 1 (tiles 2, 3) off"][64:128] = False
    masks["tile 4 off"][128:160] = False
    masks["single rows off"][[0, 31, 32, 63, 64, 100, n - 1]] = False
    masks["only the last tile"][32 * 7:] = True
    for name, mask in masks.items():
        _fuzzy(ffi, t, rows, p, 2, mask=mask, dist=dist)
        _fuzzy(ffi, t, rows, p, 0, mask=mask, dist=dist)
    assert (dist[64:128] <= 2).sum() > 30                                  # the masked pair held matches that were not reported
    t.close()


def test_levels_are_nested_level_zero_is_the_grep_and_calls_are_independent(gpu):
    import torch
    ffi = _env()
    rng = np.random.default_rng(9)
    rows = fc.random_rows(rng, 200, 90)
    t = tg._arena(ffi, rows, pieces=3)
    mask = rng.random(200) < 0.7
    dev_mask = tg._dev_words(fc.words_from_mask(mask))
    from coderag_amd.store import fuzzy_pieces
    prefiltered = 0
    for pattern in (b"ab_1", b"aAbB", b"a", b"ab ab\nAB", b"aB_1 ab\nAB 1", bytes(rng.choice(np.frombuffer(b"abAB_1 \n", np.uint8), size=40))):
        k = min(len(pattern) - 1, 3)
        for fold in (False, True):
            lv, counts = t.fuzzy(pattern, k, fold_case=fold, mask=dev_mask)
            got = lv.cpu().numpy().view(U32)
            for d in range(k):
                assert not (got[d] & ~got[d + 1]).any() and counts[d] <= counts[d + 1]
            grep, n0 = t.match([pattern], fold_case=fold, mask=dev_mask)
            assert np.array_equal(grep.cpu().numpy().view(U32), got[0]) and n0 == counts[0]
            zero, c0 = t.fuzzy(pattern, 0, fold_case=fold, mask=dev_mask)
            assert np.array_equal(zero.cpu().numpy().view(U32)[0], got[0]) and c0 == [n0]
            pieces = fuzzy_pieces(fc.fold(pattern) if fold else pattern, k)
            if pieces:                                                   # the pigeonhole grep in front of the walk changes no word of any level
                pre, _ = t.match(pieces, fold_case=fold, any_of=True, mask=dev_mask, count=False)
                under, cu = t.fuzzy(pattern, k, fold_case=fold, mask=pre)
                assert torch.equal(under, lv) and cu == counts
                prefiltered += 1
    assert prefiltered == 4                                               # (12 and 40 bytes with 3 edits: pieces of 3 and 10 bytes; exact and folded)
    # a second call with another pattern owes nothing to the first; without counts the call only enqueues
    first, c1 = t.fuzzy(b"ab_1 aB", 2)
    other, _ = t.fuzzy(b"B1\n_", 3, fold_case=True)
    again, c2 = t.fuzzy(b"ab_1 aB", 2)
    quiet, none = t.fuzzy(b"ab_1 aB", 2, count=False)
    torch.cuda.synchronize()
    assert torch.equal(first, again) and torch.equal(first, quiet) and c1 == c2 and none is None and other.shape == (4, 7)
    _fuzzy(ffi, t, rows, b"ab_1 aB", 2)
    t.close()


def test_fuzz_random_patterns_edits_folding_and_masks_over_one_arena(gpu):
    ffi = _env()
    rng = np.random.default_rng(21)
    rows = fc.random_rows(rng, 230, 70) + fc.random_rows(rng, 10, 700, b"ab")
    t = tg._arena(ffi, rows, pieces=2)
    alphabet = np.frombuffer(b"abAB_1 \n", np.uint8)
    seen = set()
    for i, m in enumerate([1, 2, 3, 5, 8, 13, 21, 31, 32, 33, 34, 47, 63, 64] * 3):
        pattern = bytes(rng.choice(alphabet[: 2 if m > 20 and i % 2 else 8], size=m))
        k = int(rng.integers(0, min(m - 1, 3) + 1))
        mask = None if i % 3 == 0 else rng.random(len(rows)) < 0.6
        dist = _fuzzy(ffi, t, rows, pattern, k, fold=bool(i % 2), mask=mask)
        seen |= set(np.minimum(dist, 4).tolist())
    assert seen == {0, 1, 2, 3, 4}
    t.close()


def test_invalid_arguments_are_refused_and_leave_the_arena_usable(gpu):
    import torch
    ffi = _env()
    L = ffi.lib()
    rows = [b"alpha", b"alpxa", b"", b"a"]
    t = tg._arena(ffi, rows)
    out = torch.zeros((4,), dtype=torch.int32, device="cuda:0")
    cnt = (ctypes.c_int64 * 4)(-5, -5, -5, -5)
    pat = (ctypes.c_uint8 * 5)(*b"alpha")

    def raw(pattern, n, k, words=out.data_ptr()):
        return L.crh_text_fuzzy(t._handle(), pattern, n, k, 0, None, words, cnt, None)

    for args, word in (((pat, 0, 0), b"len=0"), ((pat, 65, 1), b"len=65"), ((pat, 5, 4), b"max_edits=4"), ((pat, 5, -1), b"max_edits=-1"),
                       ((pat, 3, 3), b"max_edits=3"), ((None, 5, 1), b"pat_host"), ((pat, 5, 1, None), b"out_words_dev")):
        assert raw(*args) == ffi.E_INVALID and word in L.crh_last_error(), args[1:]
    assert raw(pat, 5, 1) == ffi.OK and list(cnt)[:2] == [1, 2]
    torch.cuda.synchronize()
    assert out.cpu().numpy().view(U32).tolist()[:2] == [0b0001, 0b0011]
    for bad in ((b"", 0), (b"x" * 65, 1), (b"abc", 4), (b"ab", 2)):
        with pytest.raises(ffi.NativeError):
            t.fuzzy(*bad)
    with pytest.raises(ffi.NativeError):                                  # the binding: levels x words, contiguous
        t.fuzzy(b"alpha", 1, out=torch.zeros((1, 1), dtype=torch.int32, device="cuda:0"))
    _fuzzy(ffi, t, rows, b"alpha", 2)
    t.clear()
    lv, counts = t.fuzzy(b"alpha", 2)
    assert counts == [0, 0, 0] and lv.shape == (3, 0)                      # no rows: CRH_OK, nothing launched
    t.close()


# ---------------------------------------------------------------------------------------------------- the store

PATTERN = "parse_retry_after"
FORMS = ("parse_retry_after", "parse_retry_aftr", "parseRetry_after", "pars_retry-aftxr")       # 0, 1, 2 and 3 edits away


@functools.lru_cache(maxsize=None)
def _chunks():
    """The 2 000 chunks of the text tests; every 6th also holds PATTERN with (i // 6) % 4 edits in a line of its own, and says so
    in ``content_hash`` ("f0" .. "f3"), so a fuzzy filter and a plain filter select the same points.  Computed once."""
    pay = [dict(p) for p in tg._chunks()]
    for i in range(0, len(pay), 6):
        if isinstance(pay[i].get("content"), str):
            e = (i // 6) % 4
            lines = pay[i]["content"].split("\n")
            at = (i // 24) % (len(lines) + 1)
            lines.insert(at, "    x = " + FORMS[e] + "(y)")
            pay[i].update(content="\n".join(lines), content_hash=f"f{e}", end_line=pay[i]["end_line"] + 1)
    return tuple(pay)


@functools.lru_cache(maxsize=None)
def _distances(pattern: str, fold: bool = False):
    return tuple(fc.distance_end(p["content"].encode(), pattern, fold)[0] if isinstance(p.get("content"), str) else 99 for p in _chunks())


def _by_distance():
    """How many chunks were planted 0, 1, 2 and 3 edits away."""
    return [sum(1 for p in _chunks() if p["content_hash"] == f"f{d}") for d in range(4)]


def _check_corpus():
    """The corpus is what the store test takes it for (by the restatement alone)."""
    dist = np.asarray(_distances(PATTERN))
    pay = _chunks()
    for i, p in enumerate(pay):
        planted = p["content_hash"].startswith("f")
        assert dist[i] == (int(p["content_hash"][1]) if planted else dist[i]) and (planted or dist[i] > 3), i
    assert [int((dist == d).sum()) for d in range(4)] == _by_distance() and min(_by_distance()) >= 83 and sum(_by_distance()) == 334


@pytest.mark.parametrize("shards", [1, 2])
def test_store_fuzzy_filters_end_to_end(gpu, shards):
    import asyncio
    ffi = _env()
    from coderag_amd.errors import VectorStoreError
    from coderag_amd.store import HipVectorStore
    n_all, dim = tg.STORE_N, tg.STORE_DIM
    pay = list(_chunks())
    dist = np.asarray(_distances(PATTERN))
    rng = np.random.default_rng(23)
    raw = rng.standard_normal((n_all, dim)).astype(np.float32)
    ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(n_all)]
    q = rng.standard_normal((3, dim)).astype(np.float32)
    _check_corpus()
    has = {"content": {"fuzzy": PATTERN}}                                  # 17 bytes: 2 edits by default
    same = {"content_hash": ["f0", "f1", "f2"]}

    def within(k, pattern=PATTERN, fold=False):
        d = _distances(pattern, fold)
        index = {p["entity_name"]: i for i, p in enumerate(pay)}
        return lambda p: d[index[p["entity_name"]]] <= k if p["entity_name"] in index else fc.distance_end(p["content"].encode(), pattern, fold)[0] <= k

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
            n = await same_as_brute(s, col, has, None, within(2))
            by = _by_distance()
            assert n == int((dist <= 2).sum()) == sum(by[:3])
            assert await same_as_brute(s, col, None, has, lambda p: not within(2)(p)) == n_all - n           # absent / no str: passes must_not
            for k in (0, 1, 3):
                assert await same_as_brute(s, col, {"content": {"fuzzy": PATTERN, "edits": k}}, None, within(k)) == int((dist <= k).sum())
            m = await same_as_brute(s, col, {"content": {"fuzzy": PATTERN, "edits": 3}, "language": "rust"}, {"file_path": "src/mod6.rs"},
                                    lambda p: within(3)(p) and p["language"] == "rust" and p["file_path"] != "src/mod6.rs")
            assert 0 < m < sum(by)                                         # (every planted chunk is a multiple of 6: rust)
            assert await same_as_brute(s, col, {**has, "language": "python"}, None, lambda p: False) == 0
            folded = _distances("PARSE_RETRY_AFTER", True)
            assert await same_as_brute(s, col, {"content": {"fuzzy": "PARSE_RETRY_AFTER", "edits": 1, "case": False}}, None,
                                       within(1, "PARSE_RETRY_AFTER", True)) == sum(d <= 1 for d in folded) > int((dist <= 1).sum())
            assert await same_as_brute(s, col, {"content": {"fuzzy": "PARSE_RETRY_AFTER", "edits": 3}}, None, lambda p: False) == 0
            # beside contains and matches: all must hold
            both = {"content": {"fuzzy": PATTERN, "contains": "_after", "matches": r"^\s+x = \w+\(y\)$"}}
            b = await same_as_brute(s, col, both, None, lambda p: within(2)(p) and "_after" in p["content"] and re.search(both["content"]["matches"], p["content"], re.M))
            assert 0 < b < n
            await same_as_brute(s, col, {"content": {"fuzzy": PATTERN, "contains": tg.NEEDLE2}}, None, lambda p: within(2)(p) and tg._holds(p, tg.NEEDLE2))

            # the condition answers like the plain filter that selects the same points, through the other search paths
            first = await s.search("code_chunks", q[0].tolist(), 10, has)
            assert tg._equal_hits(first, await s.search("code_chunks", q[0].tolist(), 10, same))
            assert await s.count_similar("code_chunks", q[0].tolist(), -2.0, has) == n
            assert await s.count_similar("code_chunks", q[0].tolist(), 0.0, has) == await s.count_similar("code_chunks", q[0].tolist(), 0.0, same) > 0
            lex = await s.search_lexical("code_chunks", "retry", 10, has)
            assert lex and tg._equal_hits(lex, await s.search_lexical("code_chunks", "retry", 10, same))
            assert await s.facet("code_chunks", "file_path", 50, has) == await s.facet("code_chunks", "file_path", 50, same)
            assert (await s.facet("code_chunks", "language", 5, None, has))["total"] == n_all - n

            # a repeated identical call walks nothing again; other edits do
            calls, native = col.text_match_calls, ffi.Text.fuzzy_calls
            again = await s.search("code_chunks", q[0].tolist(), 10, {"content": {"fuzzy": PATTERN, "edits": 2}})
            assert col.text_match_calls == calls and ffi.Text.fuzzy_calls == native and tg._equal_hits(first, again)

            # the pigeonhole prefilter changes no word of any level: on (one crh_text_match per shard in front of the walk) and off
            spec = {"fuzzy": PATTERN, "edits": 3}
            def levels_of(prefilter):
                col._text_cache.clear()
                col.fuzzy_prefilter = prefilter
                greps = ffi.Text.match_calls
                from coderag_amd.store import text_spec
                col.device_filters({"content": spec})
                lv, by = col._text_levels("content", text_spec("content", spec), [])
                assert ffi.Text.match_calls - greps == (shards if prefilter else 0)
                return [[w.words[id(col.shards.index[sh])].cpu().numpy() for sh in col.shards.owned] for w in lv], by
            (on, by_on), (off, by_off) = levels_of(True), levels_of(False)
            assert by_on == by_off == [int((dist == d).sum()) for d in range(4)]
            assert all(np.array_equal(a, b) for x, y in zip(on, off) for a, b in zip(x, y))
            del col.fuzzy_prefilter

            # search_text: (distance, insertion order), the distance, the line, the counts
            out = await s.search_text("code_chunks", fuzzy=PATTERN, limit=120)
            want = sorted((i for i in range(n_all) if dist[i] <= 2), key=lambda i: (dist[i], i))
            assert out["count"] == n and out["counts_by_distance"] == by[:3] and tg._ids(out["hits"]) == [ids[i] for i in want[:120]]
            lines = set()
            for h in out["hits"]:
                i = ids.index(h["id"])
                assert h["distance"] == dist[i] and h["score"] == 0.0
                assert h["match_line"] == fc.match_line(pay[i]["content"], pay[i]["start_line"], PATTERN)
                lines.add(h["match_line"] - pay[i]["start_line"])
            assert len(lines) > 4
            out = await s.search_text("code_chunks", tg.NEEDLE2, limit=1000, filters={"language": "rust"}, fuzzy="PARSE_RETRY_AFTER", edits=3, case=False)
            want = sorted((i for i in range(n_all) if folded[i] <= 3 and pay[i]["language"] == "rust" and tg._holds(pay[i], tg.NEEDLE2)), key=lambda i: (folded[i], i))
            assert out["count"] == len(want) > 10 and tg._ids(out["hits"]) == [ids[i] for i in want]
            assert [h["distance"] for h in out["hits"]] == [folded[i] for i in want] and out["counts_by_distance"] == [sum(1 for i in want if folded[i] == d) for d in range(4)]
            # a text condition of its own under must_not joins every fetch, and the rows per distance are counted under it
            for other, gone in (({"contains": PATTERN}, lambda i: dist[i] == 0), ({"fuzzy": PATTERN, "edits": 1}, lambda i: dist[i] <= 1),
                                ({"matches": r"parse\w+after\("}, lambda i: re.search(r"parse\w+after\(", pay[i]["content"]) is not None),
                                ({"contains": tg.NEEDLE2}, lambda i: tg._holds(pay[i], tg.NEEDLE2))):
                not_this = {"content": other, "file_path": "src/mod6.rs"}
                out = await s.search_text("code_chunks", fuzzy=PATTERN, limit=1000, must_not=not_this)
                want = sorted((i for i in range(n_all) if dist[i] <= 2 and pay[i]["file_path"] != "src/mod6.rs" and not gone(i)), key=lambda i: (dist[i], i))
                assert out["count"] == len(want) and tg._ids(out["hits"]) == [ids[i] for i in want], other
                assert out["counts_by_distance"] == [sum(1 for i in want if dist[i] == d) for d in range(3)] and 0 < len(want) < n
                assert [h["distance"] for h in out["hits"]] == [int(dist[i]) for i in want]
                assert await s.count_text("code_chunks", fuzzy=PATTERN, must_not=not_this) == len(want)
                assert len(await s.search("code_chunks", None, 1000, has, not_this)) == len(want)
            assert await s.count_text("code_chunks", fuzzy=PATTERN, edits=1) == by[0] + by[1] and await s.count_text("code_chunks", fuzzy="nowhere_at_all_in_here") == 0

            # refused with a ValueError
            for call in (lambda: s.search_batch("code_chunks", q, 5, [has, None, None]), lambda: s.search_batch("code_chunks", q, 5, None, [None, has, None]),
                         lambda: s.delete("code_chunks", has), lambda: s.search("code_chunks", q[0].tolist(), 5, {"language": {"fuzzy": "py"}}),
                         lambda: s.search("code_chunks", q[0].tolist(), 5, {"content": {"fuzzy": "abc", "edits": 3}}),
                         lambda: s.search_text("code_chunks", fuzzy=""), lambda: s.search_text("code_chunks", fuzzy="x" * 65), lambda: s.search_text("code_chunks", edits=1)):
                with pytest.raises(VectorStoreError) as e:
                    await call()
                assert isinstance(e.value.cause, ValueError), e.value
            assert (await s.get_collection_info("code_chunks")).points_count == n_all

            # after an append, and after a delete with compaction
            fresh = [dict(pay[1], content="brand new\n  " + FORMS[1 + i % 2] + "()\n", start_line=40, end_line=42, entity_name=f"new_{i}") for i in range(3)]
            await s.upsert("code_chunks", [f"00000000-0000-4000-9000-{i:012d}" for i in range(3)], rng.standard_normal((3, dim)).astype(np.float32), fresh)
            assert await same_as_brute(s, col, has, None, within(2)) == n + 3
            await s.delete("code_chunks", {"file_path": ["src/mod0.rs", "src/mod21.py"]})
            left = await same_as_brute(s, col, has, None, within(2))
            assert left < n and await s.compact("code_chunks") > 0 and col._text == {} and col._text_cache == {}
            assert await same_as_brute(s, col, has, None, within(2)) == left
            out = await s.search_text("code_chunks", fuzzy=PATTERN, limit=1000)
            assert out["count"] == left == len(out["hits"]) and [h["distance"] for h in out["hits"]] == sorted(h["distance"] for h in out["hits"])
            assert [(h["match_line"], h["distance"]) for h in out["hits"] if h["payload"]["entity_name"].startswith("new_")] == [(41, 1), (41, 1), (41, 2)]

    asyncio.run(run())


def test_searcher_fuzzy(gpu):
    import asyncio
    _env()
    from coderag_amd.store import HipVectorStore
    from coderag_amd.vector_search import VectorSearcher
    pay = list(_chunks())[:400]
    dist = _distances(PATTERN)[:400]
    rng = np.random.default_rng(29)
    raw = rng.standard_normal((400, tg.STORE_DIM)).astype(np.float32)
    ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(400)]

    class Embedder:
        async def embed(self, text):
            return raw[5].tolist()

        async def embed_batch(self, texts):
            return [raw[5].tolist() for _ in texts]

    async def run():
        async with HipVectorStore(dim=tg.STORE_DIM, dtype="bf16", initial_capacity=1024, device=0) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, raw, pay)
            vs = VectorSearcher(s, Embedder())
            got = await vs.search_code("anything", limit=10, fuzzy="parse_retry_aftr")
            want = await s.search("code_chunks", raw[5].tolist(), 10, {"content": {"fuzzy": "parse_retry_aftr"}})
            assert len(got) == 10 and [g["entity_name"] for g in got] == [h["payload"]["entity_name"] for h in want]
            assert all(fc.distance_end(g["content"].encode(), "parse_retry_aftr")[0] <= 2 for g in got)
            got = await vs.search_code("anything", limit=50, language="rust", fuzzy="PARSE_RETRY_AFTER", edits=0, contains_case=False)
            assert got and all(g["language"] == "rust" and "parse_retry_after" in g["content"].lower() for g in got)
            assert len(got) == sum(1 for i in range(400) if dist[i] == 0 and pay[i]["language"] == "rust")
            res = await vs.facet_code(key="language", fuzzy=PATTERN, edits=1)
            assert res["total"] == sum(1 for d in dist if d <= 1)
            sim = await vs.find_similar_code("def f(): pass", limit=5, fuzzy=PATTERN, edits=0)
            assert len(sim) == 5 and all(PATTERN in g["content"] for g in sim)

    asyncio.run(run())
