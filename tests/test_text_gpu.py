"""Literal substring match on the device: ``crh_text_*`` against the CPU restatement (tests/text_cases.py: ``bytes.find`` on each
row's own bytes) -- the validity words and the count must be equal exactly -- and the row-bitmap conditions ``CRH_COND_WORDS`` /
``CRH_COND_NOT_WORDS`` of the mask pipeline against the f32 oracle under the same bitmap (ids and score BITS).  The output buffers
are pre-filled with garbage.  No tolerance appears anywhere."""
import ctypes

import numpy as np
import pytest

from tests import text_cases as tc

pytestmark = pytest.mark.gpu

U32 = np.uint32


def _env():
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    return ffi


def _dev_words(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, dtype=U32).view(np.int32).copy()).to("cuda:0")


def _arena(ffi, rows, pieces: int = 1):
    """A device arena of `rows`, appended in `pieces` calls (buffers grow between them)."""
    t = ffi.Text(device=0)
    step = max(1, (len(rows) + pieces - 1) // pieces)
    for a in range(0, len(rows), step):
        t.append(*tc.csr(rows[a:a + step]))
    assert t.count() == (len(rows), sum(len(r) for r in rows))
    return t


def _match(ffi, t, rows, patterns, fold_case=False, any_of=False, mask=None):
    """One crh_text_match into a garbage-filled buffer, compared with the restatement; returns the bool row mask."""
    import torch
    n = len(rows)
    out = torch.full(((n + 31) // 32,), -77, dtype=torch.int32, device="cuda:0")
    words, count = t.match(patterns, fold_case=fold_case, any_of=any_of, mask=None if mask is None else _dev_words(tc.words_from_mask(mask)), out=out)
    torch.cuda.synchronize()
    got = words.cpu().numpy().view(U32)
    want = tc.match_rows(rows, patterns, fold_case, any_of, mask)
    assert np.array_equal(got, tc.words_from_mask(want)), (np.flatnonzero(tc.mask_from_words(got, n) != want)[:10], patterns)
    assert count == int(want.sum())
    return want


def _check(ffi, rows, patterns, **kw):
    t = _arena(ffi, rows)
    try:
        return _match(ffi, t, rows, patterns, **kw)
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------------- the kernel's boundaries

ROW = 400    # 32 rows = 12800 bytes = a multiple of 16: every tile's stream starts `shift` bytes before its first byte; the rows
             # around byte 1024, 4096 and 8192 of a tile (800..1200, 4000..4400, 8000..8400) leave 64 bytes on both sides


def _boundary_rows(length: int, shift: int):
    """One 32-row tile per placement: the pattern written so that its first i bytes lie BEFORE a boundary of the tile's stream --
    the 16-byte lane edge, the end of one wave step, the end of the in-flight window and of the window after it -- for every
    split i = 0 (starts at the boundary) .. length (ends at it).  `shift` > 0 puts one short row in front of the arena: every later
    tile then starts `shift` bytes after a 16-byte boundary, and the stream starts below the tile's first byte."""
    pat = tc.pattern_of(length)
    places = [(b, i) for b in (tc.LANE, 5 * tc.LANE, tc.STEP, tc.WINDOW, 2 * tc.WINDOW) for i in range(0, length + 1) if b - i >= shift]
    ntiles = len(places) + 1
    head = [tc.filler(shift, 99)] if shift else []
    body = bytearray(tc.filler(ntiles * 32 * ROW, length))
    planted = 0
    for t, (b, i) in enumerate(places, start=1):
        # tile t of the ARENA holds rows 32 t .. 32 t + 31; with the short row in front its first byte is body[(32 t - 1) * ROW]
        begin = (32 * t - (1 if shift else 0)) * ROW
        pos = begin - shift + b - i if shift else begin + b - i         # stream base + b - i
        if pos // ROW != (pos + length - 1) // ROW:
            continue                                                   # (would straddle a row end: that is another test)
        body[pos:pos + length] = pat
        planted += 1
    rows = head + [bytes(body[r * ROW:(r + 1) * ROW]) for r in range(ntiles * 32)]
    return rows, pat, planted, len(places)


@pytest.mark.parametrize("shift", [0, 7])
@pytest.mark.parametrize("length", [1, 2, 3, 4, 5, 16, 17, 64])
def test_a_match_across_every_lane_step_and_window_boundary(gpu, length, shift):
    ffi = _env()
    assert (32 * ROW) % tc.LANE == 0 and ROW > tc.MAX_PATTERN_BYTES
    rows, pat, planted, asked = _boundary_rows(length, shift)
    assert planted == asked >= 5
    want = _check(ffi, rows, [pat])
    assert int(want.sum()) == planted                                  # one row per placement, no other
    if length > 1:                                                     # folding on the same bytes, pattern given in the other case
        _check(ffi, rows, [pat.lower()], fold_case=True)


# ---------------------------------------------------------------------------------------------------- rows and tiles

def test_a_match_never_spans_two_rows(gpu):
    ffi = _env()
    rows = [tc.filler(40, i) for i in range(70)]
    rows[3] = rows[3][:-3] + b"foo"
    rows[4] = b"bar" + rows[4][3:]
    rows[31] = rows[31][:-3] + b"foo"          # across the tile boundary 31 | 32
    rows[32] = b"bar" + rows[32][3:]
    rows[40] = b"foobar" + rows[40][6:]        # at a row's first byte
    rows[41] = rows[41][:-6] + b"foobar"       # at a row's last byte
    rows[69] = rows[69][:-6] + b"foobar"       # at the last byte of the whole arena
    want = _check(ffi, rows, [b"foobar"])
    assert np.flatnonzero(want).tolist() == [40, 41, 69]
    want = _check(ffi, rows, [b"foo"])
    assert np.flatnonzero(want).tolist() == [3, 31, 40, 41, 69]
    want = _check(ffi, rows, [b"bar"])
    assert np.flatnonzero(want).tolist() == [4, 32, 40, 41, 69]
    want = _check(ffi, rows, [b"r"])           # one byte: the arena's very last byte is a match of its own
    assert want[69] and want[4]


@pytest.mark.parametrize("n", [1, 31, 32, 33, 65])
def test_row_counts_around_the_tile(gpu, n):
    ffi = _env()
    rows = [tc.filler(1 + (7 * i) % 50, i) + (b"K9" if i % 3 == 0 else b"") for i in range(n)]
    want = _check(ffi, rows, [b"K9"])
    assert int(want.sum()) == (n + 2) // 3


def test_empty_rows_a_tile_of_empty_rows_and_short_rows(gpu):
    ffi = _env()
    rows = [b""] * 3 + [b"needle"] + [b""] * 2 + [b"xxneedlexx", b"need", b"n", b""]      # a pattern longer than its row
    rows += [b""] * 32                                                 # rows 10..41: tile 1 (rows 32..63) starts with empty rows
    rows += [b""] * 22 + [b""] * 32                                    # tile 2 (rows 64..95) holds empty rows only
    rows += [b"the needle", b"", b"needl", b"eneedle"]
    want = _check(ffi, rows, [b"needle"])
    assert np.flatnonzero(want).tolist() == [3, 6, 96, 99]
    _check(ffi, [b""] * 40, [b"a"])
    _check(ffi, [b"", b"", b"a"], [b"a"])


def test_one_200_kb_row_among_short_ones(gpu):
    ffi = _env()
    big = bytearray(tc.filler(200 * 1024, 5))
    big[150_000:150_008] = b"X9#Q_7@Z"
    rows = [tc.filler(30, i) for i in range(40)]
    rows[13] = bytes(big)
    rows[14] = b"X9#Q_7@" + rows[14]           # all but the last byte
    rows[39] = rows[39] + b"X9#Q_7@Z"
    want = _check(ffi, rows, [b"X9#Q_7@Z"])
    assert np.flatnonzero(want).tolist() == [13, 39]
    big2 = bytes(big[:150_000]) + bytes(big[150_008:])                 # the long row without it: the rows behind still answer
    rows[13] = big2
    want = _check(ffi, rows, [b"X9#Q_7@Z"])
    assert np.flatnonzero(want).tolist() == [39]


def test_overlapping_false_prefixes_and_nul_bytes(gpu):
    ffi = _env()
    pat = tc.pattern_of(17)
    rows = [b"aaaa", b"aa", b"baaab", b"aabaa",
            pat[:4] * 700 + pat,                                       # 700 false 4-byte prefixes, then the match
            pat[:4] * 700 + pat[:16],                                  # ... and never the match
            pat[:16] * 50 + pat[:15] + b"!",
            b"ab\0\0cd", b"\0", b"ab\0cd\0\0", b"", b"\0\0\0\0\0"]
    want = _check(ffi, rows, [b"aaa"])
    assert np.flatnonzero(want).tolist() == [0, 2]
    want = _check(ffi, rows, [pat])
    assert np.flatnonzero(want).tolist() == [4]
    want = _check(ffi, rows, [b"\0\0"])                                # NUL is a byte like any other (the slack behind the arena is NULs)
    assert np.flatnonzero(want).tolist() == [7, 9, 11]
    want = _check(ffi, rows, [b"\0"])
    assert np.flatnonzero(want).tolist() == [7, 8, 9, 11]
    want = _check(ffi, rows, [b"\0\0\0\0\0\0"])
    assert not want.any()
    want = _check(ffi, rows, [b"d\0\0"])                               # ends at the last byte of row 9; row 10 is empty, row 11 NULs
    assert np.flatnonzero(want).tolist() == [9]


# ---------------------------------------------------------------------------------------------------- patterns, folding, masks

def _mixed_rows(n=300, seed=3):
    rng = np.random.default_rng(seed)
    bits = [b"retry_after=", b"Retry_After=", b".unwrap()", b"#include <hip/", b"TODO(", b"todo(", b"@[`{", b"\xc3\x89t\xc3\xa9", b"\xc3\xa9T\xc3\x89",
            b"Z[", b"z{", b"A@", b"a`"]
    rows = []
    for i in range(n):
        parts = [tc.filler(int(rng.integers(0, 120)), 1000 + i)]
        for j in rng.choice(len(bits), size=int(rng.integers(0, 4)), replace=False):
            parts += [bits[j], tc.filler(int(rng.integers(0, 60)), 5000 + 13 * i + int(j))]
        rows.append(b"".join(parts))
    return rows


@pytest.mark.parametrize("fold_case", [False, True])
@pytest.mark.parametrize("any_of", [False, True])
def test_all_and_any_with_one_two_and_eight_patterns(gpu, fold_case, any_of):
    ffi = _env()
    rows = _mixed_rows()
    t = _arena(ffi, rows, pieces=3)
    sets = [[b"retry_after="], [b"TODO("], [b"retry_after=", b".unwrap()"], [b"todo(", b"todo("], [b"TODO(", b"absent!"],
            [b"retry_after=", b".unwrap()", b"#include <hip/", b"TODO(", b"@[`{", b"Z[", b"A@", b"t"],
            [b"e", b"e", b"e", b"e", b"e", b"e", b"e", b"TODO("], [b"a", b"b", b"c"],
            [b"\xc3\x89", b"t"], [b"\xc3\xa9T"], [b"z[", b"Z{"], [b"a@"], [b"A`"], [b"@[`{"],
            [b"x" * 64], [b"retry_after=" + b"q" * 52]]
    hits = 0
    for pats in sets:
        hits += int(_match(ffi, t, rows, pats, fold_case=fold_case, any_of=any_of).sum())
    assert hits > 100
    t.close()


def test_masks_zero_words_partial_words_and_no_mask(gpu):
    ffi = _env()
    rows = _mixed_rows(n=200, seed=4)
    t = _arena(ffi, rows)
    rng = np.random.default_rng(8)
    every = _match(ffi, t, rows, [b"e"])                               # nearly every row matches
    assert every.sum() > 100
    zero_tiles = np.ones(200, bool)
    zero_tiles[32:64] = False                                          # a zero mask word over rows that DO match
    zero_tiles[192:] = False                                           # the last, partial word
    got = _match(ffi, t, rows, [b"e"], mask=zero_tiles)
    assert not got[32:64].any() and not got[192:].any() and got[:32].any()
    _match(ffi, t, rows, [b"e"], mask=rng.random(200) < 0.5)
    _match(ffi, t, rows, [b"e"], mask=rng.random(200) < 0.03)
    _match(ffi, t, rows, [b"TODO(", b"e"], mask=np.zeros(200, bool))
    _match(ffi, t, rows, [b"TODO(", b"e"], any_of=True, mask=np.ones(200, bool))
    t.close()


def test_tombstoned_rows_arrive_through_the_index_row_mask(gpu):
    import torch
    ffi = _env()
    n = 200
    rows = _mixed_rows(n=n, seed=6)
    t = _arena(ffi, rows)
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
        words, count = t.match([b"e"], mask=mask, out=out)
        want = tc.match_rows(rows, [b"e"], mask=keep)
        assert np.array_equal(words.cpu().numpy().view(U32), tc.words_from_mask(want)) and count == int(want.sum()) > 0
    idx.close()
    t.close()


def test_invalid_arguments_are_refused_and_leave_the_arena_usable(gpu):
    import torch
    ffi = _env()
    L = ffi.lib()
    rows = [b"alpha", b"beta needle", b"", b"needle"]
    t = _arena(ffi, rows)
    out = torch.zeros((1,), dtype=torch.int32, device="cuda:0")
    cnt = ctypes.c_int64(-5)

    def raw(pats, combine=ffi.TEXT_ALL):
        n, off, data = ffi.text_patterns(pats)
        return L.crh_text_match(t._handle(), n, off.ctypes.data, data.ctypes.data, 0, combine, None, out.data_ptr(), ctypes.byref(cnt), 0)

    assert raw([]) == ffi.E_INVALID
    assert raw([b"a"] * 9) == ffi.E_INVALID
    assert raw([b""]) == ffi.E_INVALID
    assert raw([b"a", b""]) == ffi.E_INVALID
    assert raw([b"x" * 65]) == ffi.E_INVALID
    assert raw([b"a"], combine=2) == ffi.E_INVALID
    assert raw([b"x" * 64]) == ffi.OK and cnt.value == 0
    assert raw([b"needle"]) == ffi.OK and cnt.value == 2
    torch.cuda.synchronize()
    assert int(out.cpu().numpy().view(U32)[0]) == 0b1010
    # append: offsets that do not start at 0, that decrease, a negative n -- nothing is stored
    bad = (np.asarray([1, 3], np.int64), np.asarray([0, 4, 2], np.int64))
    data = np.frombuffer(b"abcdefgh", np.uint8).copy()
    for off in bad:
        assert L.crh_text_append(t._handle(), off.size - 1, off.ctypes.data, data.ctypes.data) == ffi.E_INVALID
    assert L.crh_text_append(t._handle(), -1, bad[0].ctypes.data, data.ctypes.data) == ffi.E_INVALID
    assert t.count() == (4, sum(len(r) for r in rows))
    t.append(*tc.csr([b"needle again"]))
    _match(ffi, t, rows + [b"needle again"], [b"needle"])
    # cleared and refilled with less text: the old bytes behind the new end are not text
    t.clear()
    assert t.count() == (0, 0)
    words, count = t.match([b"needle"])
    assert count == 0 and words.numel() == 0
    t.append(*tc.csr([b"nee"]))
    _match(ffi, t, [b"nee"], [b"needle"])
    _match(ffi, t, [b"nee"], [b"e\0"])
    t.close()


# ---------------------------------------------------------------------------------------------------- the row-bitmap condition

def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(np.asarray(a[0]).view(U32), np.asarray(b[0]).view(U32))


@pytest.mark.parametrize("dtype_name", ["bf16", "f32"])
def test_words_conditions_equal_the_oracle_restricted_to_the_bitmap(gpu, dtype_name):
    ffi = _env()
    from oracle import search as orc
    bf16 = dtype_name == "bf16"
    rows, dim, nq, k = 3000, 768, 3, 10
    rng = np.random.default_rng(41 + bf16)
    x = rng.standard_normal((rows, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    codes = rng.integers(0, 4, (rows, 1)).astype(np.int32)
    idx = ffi.Index(dim, ffi.DTYPE_BF16 if bf16 else ffi.DTYPE_F32, capacity_rows=rows + 64, n_code_cols=1)
    idx.append(x, codes)
    xpre, qpre = orc.preprocess(x, to_bf16=bf16), orc.preprocess(q, to_bf16=bf16)
    alive = np.ones(rows, bool)
    dead = np.sort(rng.choice(rows, 300, replace=False))
    idx.tombstone(dead)
    alive[dead] = False
    ntiles = (rows + 31) // 32

    def oracle(mask):
        return orc.search(xpre, qpre, k, alive=mask.astype(np.uint8))

    dense = rng.random(rows) < 0.5
    sparse = np.zeros(rows, bool)
    sparse[rng.choice(rows, 12, replace=False)] = True                 # at most 12 of 94 tiles populated: the tile-list route
    for bits, tag in ((dense, 1), (sparse, 2)):
        w = _dev_words(tc.words_from_mask(bits))
        yes, no = ffi.RowWords(tag, w), ffi.RowWords(tag, w, negate=True)
        assert _same(idx.search(q, k, filters=[yes]), oracle(alive & bits))                      # the only condition
        read = idx.stats()["tiles"]
        assert (read < ntiles) == (bits is sparse), (read, ntiles)
        assert _same(idx.search(q, k, filters=[no]), oracle(alive & ~bits))
        assert _same(idx.search(q, k, filters=[(0, [1, 2], False), yes]), oracle(alive & bits & (codes[:, 0] > 0) & (codes[:, 0] < 3)))
        assert _same(idx.search(q, k, filters=[no, (0, 3)]), oracle(alive & ~bits & (codes[:, 0] == 3)))
        assert idx.count_matching([yes]) == int((alive & bits).sum())
        assert np.array_equal(idx.match_rows([yes, (0, [0], True)], limit=rows), np.flatnonzero(alive & bits & (codes[:, 0] != 0)))
        assert np.array_equal(idx.match_rows([no], limit=7), np.flatnonzero(alive & ~bits)[:7])
        assert np.array_equal(idx.row_mask([yes]).cpu().numpy().view(U32), tc.words_from_mask(alive & bits))
        s, r, c = idx.search_range(q, k, -2.0, filters=[yes])          # every score is above -2: the count is the bitmap's
        assert c.tolist() == [int((alive & bits).sum())] * nq and _same((s, r), oracle(alive & bits))
    # a rewritten buffer is honoured under a new tag (the mask cache cannot look into the buffer)
    w = _dev_words(tc.words_from_mask(dense))
    first = idx.search(q, k, filters=[ffi.RowWords(7, w)])
    assert _same(first, oracle(alive & dense))
    w.copy_(_dev_words(tc.words_from_mask(~dense)))
    assert _same(idx.search(q, k, filters=[ffi.RowWords(8, w)]), oracle(alive & ~dense))
    # too few words, and the entry points that do not take a bitmap
    short = ffi.RowWords(9, w[: ntiles - 1].contiguous())
    for call in (lambda: idx.search(q, k, filters=[short]), lambda: idx.count_matching([short]),
                 lambda: idx.tombstone_filter([ffi.RowWords(9, w)]),
                 lambda: idx.search_multi(q, k, [[ffi.RowWords(9, w)], [(0, 1)]], [0, 1, 0])):
        with pytest.raises(ffi.NativeError) as e:
            call()
        assert e.value.code == ffi.E_INVALID
    assert idx.count()[1] == int(alive.sum())
    assert _same(idx.search(q, k, filters=[(0, [1], False)]), oracle(alive & (codes[:, 0] == 1)))
    idx.close()


# ---------------------------------------------------------------------------------------------------- the store

STORE_N, STORE_DIM = 2000, 384
NEEDLE, NEEDLE2, MIXED = "retry_after=", ".unwrap()", "ToDo("


def _chunks():
    """2 000 synthetic chunks.  NEEDLE is in every 7th, NEEDLE2 in every 5th, MIXED (in changing case) in every 11th; chunk 13
    has no content at all and chunk 14 a content that is no str; ``content_hash`` says "n1" exactly where NEEDLE is planted, so a
    text filter and a plain filter select the same points."""
    rng = np.random.default_rng(17)
    pay = []
    for i in range(STORE_N):
        lines = [tc.filler(int(rng.integers(5, 60)), 7000 + 31 * i + j).decode().replace("\n", " ") for j in range(int(rng.integers(2, 9)))]
        if i % 7 == 0:
            at = int(rng.integers(0, len(lines)))
            lines[at] = lines[at][:3] + NEEDLE + lines[at][3:]
        if i % 5 == 0:
            lines[-1] += NEEDLE2
        if i % 11 == 0:
            lines[0] = (MIXED, MIXED.lower(), MIXED.upper())[i % 3] + lines[0]
        p = {"file_path": f"src/mod{i % 50}.{'py' if i % 3 else 'rs'}", "entity_type": "function", "entity_name": f"fn_{i}",
             "language": "python" if i % 3 else "rust", "content": "\n".join(lines), "start_line": 1 + (i * 13) % 400,
             "end_line": 1 + (i * 13) % 400 + len(lines) - 1, "project_name": "demo", "content_hash": "n1" if i % 7 == 0 else "n0"}
        pay.append(p)
    del pay[13]["content"]
    pay[14].update(content=12345, content_hash="n0")
    return pay


def _holds(p, strings, any_of=False, case=True):
    text = p.get("content")
    if not isinstance(text, str):
        return False
    raw = text.encode("utf-8", "surrogatepass")
    return tc.row_matches(raw, [s.encode("utf-8", "surrogatepass") for s in ([strings] if isinstance(strings, str) else strings)], not case, any_of)


def _brute(col, q, k, keep_fn):
    """ids and f32 scores of the oracle's top-k over the stored rows (``read_rows`` of every shard) of the alive points whose
    payload passes ``keep_fn``."""
    from oracle import search as orc
    n = col.payloads.n
    xs = np.zeros((n, STORE_DIM), np.float32)
    alive = np.zeros(n, bool)
    for s in col.shards.owned:
        sl = np.arange(col.shards.rows[s]) if col.shards.ns == 1 else col.slot_of[s]
        xs[sl] = col.shards.index[s].read_rows(0, len(sl))
        alive[sl] = col.shards.rows_alive(np.full(len(sl), s, np.int32), np.arange(len(sl), dtype=np.int64))
    keep = alive & np.asarray([bool(keep_fn(col.payloads.get(t))) for t in range(n)], bool)
    sc, r = orc.search(xs, orc.preprocess(q, to_bf16=True), k, alive=keep.astype(np.uint8))
    return [[col.ids.get(int(t)) for t in row if t >= 0] for row in r], sc, int(keep.sum())


def _ids(hits):
    return [h["id"] for h in hits]


def _equal_hits(a, b):
    return _ids(a) == _ids(b) and [np.float32(h["score"]).view(U32) for h in a] == [np.float32(h["score"]).view(U32) for h in b]


@pytest.mark.parametrize("shards", [1, 2])
def test_store_text_filters_end_to_end(gpu, shards):
    import asyncio
    ffi = _env()
    from coderag_amd.errors import VectorStoreError
    from coderag_amd.store import HipVectorStore
    pay = _chunks()
    rng = np.random.default_rng(23)
    raw = rng.standard_normal((STORE_N, STORE_DIM)).astype(np.float32)
    ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(STORE_N)]
    q = rng.standard_normal((3, STORE_DIM)).astype(np.float32)
    has = {"content": {"contains": NEEDLE}}

    async def same_as_brute(s, col, filters, must_not, keep_fn, k=10):
        got = await s.search_batch("code_chunks", q, k, filters, must_not)
        want_ids, want_s, n = _brute(col, q, k, keep_fn)
        for i in range(len(q)):
            assert _ids(got[i]) == want_ids[i], (filters, must_not)
            assert np.array_equal(np.asarray([h["score"] for h in got[i]], np.float32).view(U32), want_s[i][: len(got[i])].view(U32))
        return n

    async def run():
        async with HipVectorStore(dim=STORE_DIM, dtype="bf16", initial_capacity=4096, device=0, shards=shards, compact_dead_fraction=0.0) as s:
            await s.create_collections()
            for a in range(0, STORE_N, 500):
                await s.upsert("code_chunks", ids[a:a + 500], raw[a:a + 500], pay[a:a + 500])
            col = s._col("code_chunks")
            # a collection never filtered by text has built nothing
            await s.search("code_chunks", q[0].tolist(), 5, {"language": "python"})
            assert col._text == {} and col.text_match_calls == 0

            n = await same_as_brute(s, col, has, None, lambda p: _holds(p, NEEDLE))
            assert n == len(range(0, STORE_N, 7)) - 1                   # (chunk 14 is a multiple of 7 and holds no str)
            assert await same_as_brute(s, col, None, has, lambda p: not _holds(p, NEEDLE)) == STORE_N - n      # absent / no str: passes must_not
            await same_as_brute(s, col, {**has, "language": "rust"}, None, lambda p: _holds(p, NEEDLE) and p["language"] == "rust")
            await same_as_brute(s, col, {"content": {"contains": [NEEDLE, NEEDLE2]}}, {"language": "rust"},
                                lambda p: _holds(p, [NEEDLE, NEEDLE2]) and p["language"] != "rust")
            await same_as_brute(s, col, {"content": {"contains": [NEEDLE, NEEDLE2], "any": True}}, None, lambda p: _holds(p, [NEEDLE, NEEDLE2], any_of=True))
            m = await same_as_brute(s, col, {"content": {"contains": "todo(", "case": False}}, None, lambda p: _holds(p, "todo(", case=False))
            m1 = await same_as_brute(s, col, {"content": {"contains": "todo("}}, None, lambda p: _holds(p, "todo("))
            assert m == len(range(0, STORE_N, 11)) and 0 < m1 < m
            await same_as_brute(s, col, {"content": {"contains": "todo(", "case": False}, "start_line": {"gte": 100, "lt": 300}}, has,
                                lambda p: _holds(p, "todo(", case=False) and 100 <= p["start_line"] < 300 and not _holds(p, NEEDLE))
            await same_as_brute(s, col, {"content": {"contains": "no such string anywhere"}}, None, lambda p: False)

            # a repeated identical call does not grep again; another pattern does; the cache is keyed by the other conditions too
            first = await s.search("code_chunks", q[0].tolist(), 10, has)      # (nine greps so far: the oldest result has left the cache of 8)
            calls, native = col.text_match_calls, ffi.Text.match_calls
            again = await s.search("code_chunks", q[0].tolist(), 10, has)
            assert col.text_match_calls == calls and ffi.Text.match_calls == native and _equal_hits(first, again)
            await s.search("code_chunks", q[1].tolist(), 10, {"content": {"contains": [NEEDLE]}})
            assert col.text_match_calls == calls
            await s.search("code_chunks", q[0].tolist(), 10, {"content": {"contains": NEEDLE[:-1]}})
            assert col.text_match_calls == calls + 1 and ffi.Text.match_calls == native + shards

            # a text filter and the plain filter that selects the same points answer alike, through every feature
            same = {"content_hash": "n1"}
            assert _equal_hits(first, await s.search("code_chunks", q[0].tolist(), 10, same))
            for kw in ({"diversity": 0.5}, {"group_by": "file_path", "group_size": 1}, {"max_overlap": 0.5}, {"score_threshold": 0.0}):
                assert _equal_hits(await s.search("code_chunks", q[0].tolist(), 10, has, **kw), await s.search("code_chunks", q[0].tolist(), 10, same, **kw)), kw
            pending = [s.search("code_chunks", q[i % 3].tolist(), 5 + i, has if i % 2 else None) for i in range(8)]      # coalesced calls
            for i, hits in enumerate(await asyncio.gather(*pending)):
                assert _equal_hits(hits, (await s.search_batch("code_chunks", q[i % 3][None], 5 + i, same if i % 2 else None))[0])
            assert await s.count_similar("code_chunks", q[0].tolist(), 0.0, has) == await s.count_similar("code_chunks", q[0].tolist(), 0.0, same) > 0
            assert await s.count_similar("code_chunks", q[0].tolist(), -2.0, has) == n
            hyb = await s.search_hybrid("code_chunks", q[0].tolist(), "fn retry", 10, filters=has)
            ref = await s.search_hybrid("code_chunks", q[0].tolist(), "fn retry", 10, filters=same)
            assert _equal_hits(hyb, ref) and hyb and all(NEEDLE in h["payload"]["content"] for h in hyb)
            lex = await s.search_lexical("code_chunks", "retry", 10, has)
            assert _equal_hits(lex, await s.search_lexical("code_chunks", "retry", 10, same))
            fetched = await s.search("code_chunks", None, 20, has)
            assert _ids(fetched) == _ids(await s.search("code_chunks", None, 20, same)) == [ids[i] for i in range(0, STORE_N, 7) if i != 14][:20]

            # search_text: hits in insertion order, the exact count, the line of the first match
            out = await s.search_text("code_chunks", NEEDLE, limit=25)
            want = [i for i in range(0, STORE_N, 7) if i != 14]
            assert out["count"] == len(want) == n and _ids(out["hits"]) == [ids[i] for i in want[:25]]
            for h in out["hits"]:
                text = h["payload"]["content"]
                assert h["match_line"] == h["payload"]["start_line"] + text[: text.index(NEEDLE)].count("\n") and h["score"] == 0.0
            out = await s.search_text("code_chunks", ["TODO(", NEEDLE2], limit=5, filters={"language": "rust"}, must_not={"content": {"contains": NEEDLE}},
                                      any=True, case=False)
            want = [i for i in range(STORE_N) if pay[i]["language"] == "rust" and _holds(pay[i], ["todo(", NEEDLE2], any_of=True, case=False)
                    and not _holds(pay[i], NEEDLE)]
            assert out["count"] == len(want) > 5 and _ids(out["hits"]) == [ids[i] for i in want[:5]]
            for h in out["hits"]:
                low = h["payload"]["content"].lower()
                first_at = min(p for p in (low.find("todo("), low.find(NEEDLE2)) if p >= 0)
                assert h["match_line"] == h["payload"]["start_line"] + low[:first_at].count("\n")
            assert await s.count_text("code_chunks", NEEDLE) == n and await s.count_text("code_chunks", "nowhere at all") == 0
            assert (await s.search_text("code_chunks", "nowhere at all"))["hits"] == []

            # refused with a ValueError: per-query filter lists and deletes that carry a text condition, and what the parser refuses
            for call in (lambda: s.search_batch("code_chunks", q, 5, [has, None, None]), lambda: s.search_batch("code_chunks", q, 5, None, [None, has, None]),
                         lambda: s.delete("code_chunks", has), lambda: s.search("code_chunks", q[0].tolist(), 5, {"content": "plain"}),
                         lambda: s.search("code_chunks", q[0].tolist(), 5, {"language": {"contains": "py"}}),
                         lambda: s.search("code_chunks", q[0].tolist(), 5, {"content": {"contains": "x" * 65}}),
                         lambda: s.search_text("code_chunks", ""), lambda: s.search_text("code_chunks", ["a"] * 9)):
                with pytest.raises(VectorStoreError) as e:
                    await call()
                assert isinstance(e.value.cause, ValueError), e.value
            assert (await s.get_collection_info("code_chunks")).points_count == STORE_N

            # delete + compact() + another upsert: the arena is dropped and rebuilt, appended rows are added before the next match
            await s.delete("code_chunks", {"file_path": ["src/mod0.rs", "src/mod21.py"]})
            await same_as_brute(s, col, has, None, lambda p: _holds(p, NEEDLE))
            assert await s.compact("code_chunks") > 0 and col._text == {} and col._text_cache == {}
            left = await same_as_brute(s, col, has, None, lambda p: _holds(p, NEEDLE))
            fresh = [dict(pay[1], content="brand new\n  " + NEEDLE + "1\n", start_line=40, end_line=42, entity_name=f"new_{i}") for i in range(3)]
            await s.upsert("code_chunks", [f"00000000-0000-4000-9000-{i:012d}" for i in range(3)], rng.standard_normal((3, STORE_DIM)).astype(np.float32), fresh)
            assert await same_as_brute(s, col, has, None, lambda p: _holds(p, NEEDLE)) == left + 3
            out = await s.search_text("code_chunks", NEEDLE, limit=1000)
            assert out["count"] == left + 3 and [h["match_line"] for h in out["hits"][-3:]] == [41, 41, 41]
            assert all(a.count()[0] == col.shards.rows[sh] for sh, a in col._text["content"].items())

    asyncio.run(run())


def test_searcher_contains_and_the_summaries_text_key(gpu):
    import asyncio
    _env()
    from coderag_amd.store import HipVectorStore
    from coderag_amd.vector_search import VectorSearcher
    pay = _chunks()[:400]
    rng = np.random.default_rng(29)
    raw = rng.standard_normal((400, STORE_DIM)).astype(np.float32)
    ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(400)]

    class Embedder:
        async def embed(self, text):
            return raw[5].tolist()

        async def embed_batch(self, texts):
            return [raw[5 + i].tolist() for i in range(len(texts))]

    async def run():
        async with HipVectorStore(dim=STORE_DIM, dtype="bf16", initial_capacity=1024, device=0) as s:
            await s.create_collections()
            await s.upsert("code_chunks", ids, raw, pay)
            sums = [{"file_path": p["file_path"], "entity_type": "function", "entity_name": p["entity_name"], "project_name": "demo",
                     "summary": ("Parses the Retry-After header. " if i % 4 == 0 else "Does something else. ") + p["entity_name"]} for i, p in enumerate(pay)]
            await s.upsert("summaries", ids, raw, sums)
            vs = VectorSearcher(s, Embedder())
            plain = await vs.search_code("anything", limit=10)
            assert plain[0]["entity_name"] == "fn_5" and NEEDLE not in plain[0]["content"] and s._col("code_chunks")._text == {}
            got = await vs.search_code("anything", limit=10, contains=NEEDLE)
            want = await s.search("code_chunks", raw[5].tolist(), 10, {"content_hash": "n1"})
            assert [g["entity_name"] for g in got] == [h["payload"]["entity_name"] for h in want] and all(NEEDLE in g["content"] for g in got)
            got = await vs.search_code("anything", limit=10, language="rust", contains=["todo(", NEEDLE2], contains_case=False)
            assert got and all(g["language"] == "rust" and "todo(" in g["content"].lower() and NEEDLE2 in g["content"] for g in got)
            batch = await vs.search_code_batch(["a", "b"], limit=5, contains=NEEDLE)
            assert len(batch) == 2 and all(NEEDLE in g["content"] for hits in batch for g in hits) and all(len(hits) == 5 for hits in batch)
            sim = await vs.find_similar_code("def f(): pass", limit=5, contains=NEEDLE)
            assert len(sim) == 5 and [g["entity_name"] for g in sim] == [h["payload"]["entity_name"] for h in want[:5]]
            su = await vs.search_summaries("anything", limit=10, contains="retry-after", contains_case=False)
            assert len(su) == 10 and all("Retry-After" in g["summary"] for g in su)
            assert (await s.search_text("summaries", "Retry-After header"))["count"] == 100
            assert (await s.search_text("summaries", "Retry-After header"))["hits"][0]["match_line"] is None      # no start_line there

    asyncio.run(run())
