"""The keyword-search cases of tests/lex_walk_cases.py are what they claim to be -- shown without a GPU, or a pass on the device
would mean nothing: the constants the builders assume against the text of ``crh_lex.hip``; the table sizes, key counts, slots
and probe lengths against a restatement of ``LexTable::build``; the buckets, chunk positions, ``M_q`` and counts of the cut
cases against a restatement of ``k_lex_cut``; the closed form against the restatement ``lex_cases.bm25_search``, bit for bit,
wherever a case has both; the CSR rules of ``crh_lex_append`` and the size limits on every corpus."""
import os
import re

import numpy as np
import pytest

from tests import lex_cases as lc
from tests import lex_walk_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = np.uint32
FAMILIES = sorted(wc.families())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(U32)


def _same(got, want):
    return np.array_equal(got[2], want[2]) and np.array_equal(got[1], want[1]) and np.array_equal(_bits(got[0]), _bits(want[0]))


def _fam(name):
    return wc.families()[name]


def _call(fam, name):
    return next(c for c in fam.calls if c.name == name)


# ------------------------------------------------------------------ the source
def test_constants_equal_the_source():
    src = open(os.path.join(ROOT, "code-rag_amd", "csrc", "crh_lex.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "coderag_hip.h")).read()

    def const(name):
        return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    terms = int(re.search(r"#define CRH_LEX_MAX_QUERY_TERMS (\d+)", hdr).group(1))
    assert const("kLexPassQ") == wc.PASS_Q and terms == lc.MAX_QUERY_TERMS == 32
    assert re.search(r"constexpr int kLexMaxKeys = kLexPassQ \* CRH_LEX_MAX_QUERY_TERMS;", src) and wc.PASS_Q * terms == wc.MAX_KEYS
    assert re.search(r"constexpr int kLexMaxSlots = 2 \* kLexMaxKeys;", src)
    assert const("kLexBuckets") == wc.BUCKETS and const("kLexSteps") == wc.STEPS and const("kLexWaves") == wc.WAVES
    assert int(re.search(r"#define CRH_MAX_K (\d+)", hdr).group(1)) == wc.MAX_K
    assert re.search(r"lex_slot\(uint32_t id, int log2_slots\) \{ return \(id \* (\d+)u\) >> \(32 - log2_slots\); \}", src).group(1) == str(wc.MULT)
    assert "int log2_slots = 6;" in src and "while ((size_t)(1 << log2_slots) < 2 * ids.size()) ++log2_slots;" in src
    assert "const unsigned int *h = hist + (size_t)q * kLexBuckets + (size_t)tid * 256;" in src        # thread tid owns 256 buckets
    assert "s0 += 64u * kLexSteps" in src                                                               # an outer iteration is 256 entries


# ------------------------------------------------------------------ every corpus and call
@pytest.mark.parametrize("name", FAMILIES)
def test_corpus_passes_the_append_checks_and_the_size_limits(name):
    fam = _fam(name)
    c = fam.corpus
    assert c.n <= wc.MAX_ROWS and c.terms.size <= wc.MAX_ENTRIES and c.row_off[0] == 0 and c.row_off[-1] == c.terms.size == c.tf.size
    assert (np.diff(c.row_off) >= 0).all() and c.dl.size == c.n and (c.tf >= 1).all()
    er = lc.row_ids(c.row_off)
    inside = er[1:] == er[:-1]
    assert (c.terms[1:].astype(np.int64) > c.terms[:-1].astype(np.int64))[inside].all(), "ids strictly ascending inside a row"
    assert (c.dl.astype(np.int64) >= np.bincount(er, weights=c.tf, minlength=c.n).astype(np.int64)).all()
    for one in fam.calls + [wc.interloper(fam)]:
        assert len(one.queries) <= wc.MAX_NQ and 1 <= one.k <= wc.MAX_K
        assert all(q.size <= lc.MAX_QUERY_TERMS and (np.diff(q.astype(np.int64)) > 0).all() for q in one.queries)
        assert all(np.isfinite(w).all() for w in one.idf) and one.avgdl > 0
        assert one.words is None or one.words.size == (c.n + 31) // 32
    own, other = (max(len(wc.pass_keys(p)) for one in calls for p in wc.passes(one.queries)) for calls in (fam.calls, [wc.interloper(fam)]))
    assert wc.build_table(range(own))[0] != wc.build_table(range(other))[0], "the interloper's table has another size"


@pytest.mark.parametrize("name", FAMILIES)
def test_closed_form_equals_the_restatement(name):
    fam = _fam(name)
    for one in fam.calls:
        if wc.has_closed_form(one):
            assert _same(wc.closed_form(fam.corpus, one), wc.expected(fam.corpus, one)), one.name
    if name.startswith(("cut_", "crowded", "order_")):
        assert any(wc.has_closed_form(one) for one in fam.calls)


@pytest.mark.parametrize("name", FAMILIES)
def test_stated_tables(name):
    for one in _fam(name).calls:
        if "log2" in one.facts:
            built = [wc.build_table(wc.pass_keys(p)) for p in wc.passes(one.queries)]
            assert [len(wc.pass_keys(p)) for p in wc.passes(one.queries)] == one.facts["keys"], one.name
            assert [b[0] for b in built] == one.facts["log2"], one.name
            assert all(2 * sum(s is not None for s in b[1]) <= len(b[1]) for b in built)


# ------------------------------------------------------------------ table families
def test_full_pass_fills_the_largest_table():
    fam = _fam("full_pass")
    full = _call(fam, "2048_keys")
    assert len(full.queries) == 64 and all(q.size == 32 for q in full.queries) and len(wc.pass_keys(full.queries)) == wc.MAX_KEYS
    log2, slots = wc.build_table(wc.pass_keys(full.queries))
    assert log2 == 12 and (1 << log2) * 16 + wc.MAX_KEYS * 4 == 72 * 1024
    assert sorted(q.size for q in _call(fam, "2047_keys").queries)[:2] == [31, 32]
    second = _call(fam, "second_pass")
    assert len(second.queries) == 128 and all(np.array_equal(a, b) for a, b in zip(second.queries[64:], full.queries))
    lens = np.diff(fam.corpus.row_off)
    assert lens.min() == 0 and lens.max() == 400 and 1800 <= fam.corpus.n <= 2200
    keys = set(wc.pass_keys(full.queries))
    held = np.isin(fam.corpus.terms, np.asarray(sorted(keys), U32))
    assert 0.4 < held.mean() < 0.6, "about as many foreign ids as keys"
    reads = [wc.probe(log2, slots, int(t))[1] for t in np.unique(fam.corpus.terms)[::7].tolist()]
    assert max(reads) >= 4, "a table this full has real chains"
    want = wc.expected(fam.corpus, full)
    assert (want[2] > 10).all()


def test_half_full_is_exactly_half_full():
    fam = _fam("half_full")
    log2, slots = wc.build_table(wc.pass_keys(_call(fam, "32_keys").queries))
    assert (log2, sum(s is not None for s in slots)) == (6, 32)
    log2, slots = wc.build_table(wc.pass_keys(_call(fam, "33_keys").queries))
    assert (log2, sum(s is not None for s in slots)) == (7, 33)


@pytest.mark.parametrize("name, last", [("log2_6", 63), ("log2_12", 4095)])
def test_wrapped_chain_occupies_the_stated_slots(name, last):
    fam = _fam("wrapped_chain")
    one = _call(fam, name)
    chain, foreign = one.facts["chain"], one.facts["foreign"]
    assert (chain[:5] == [55, 144, 199, 288, 343]) if last == 63 else (chain[:3] == [2584, 6765, 13530])
    log2, slots = wc.build_table(wc.pass_keys(one.queries))
    assert (1 << log2) - 1 == last and len(chain) == len(foreign) == wc.CHAIN
    assert all(wc.lex_slot(t, log2) == last for t in chain + foreign) and not set(chain) & set(foreign)
    where = [last] + list(range(wc.CHAIN - 1))
    assert [slots[s] for s in where] == chain and slots[wc.CHAIN - 1] is None and slots[last - 1] is None
    for t in foreign:
        assert wc.probe(log2, slots, t) == (False, wc.CHAIN, wc.CHAIN - 1), "the probe reads the whole chain and ends at the empty slot"
        assert (fam.corpus.terms == U32(t)).any(), "and a row holds the id"
    assert wc.probe(log2, slots, chain[-1]) == (True, wc.CHAIN, wc.CHAIN - 2)
    want = wc.expected(fam.corpus, one)
    assert want[2][0] > 10


def test_edge_ids_variants():
    have, lack = _fam("edge_ids"), _fam("edge_ids_query_only")
    for fam in (have, lack):
        off = fam.corpus.row_off
        totals = [int(off[min(t + 32, fam.corpus.n)] - off[t]) for t in range(0, fam.corpus.n, 32)]
        assert all(n > 0 and n % 64 for n in totals), "padded lanes (id 0) in every tile's last step"
    for t in wc.EDGE_IDS:
        assert (have.corpus.terms == U32(t)).sum() > 5 and not (lack.corpus.terms == U32(t)).any()
        assert any(t in q.tolist() for q in _call(have, "query_and_rows").queries) and any(t in q.tolist() for q in _call(lack, "query_only").queries)
        assert not any(t in q.tolist() for q in _call(have, "rows_only").queries)
    want = wc.expected(lack.corpus, _call(lack, "query_only"))
    assert want[2].tolist() == [int(np.count_nonzero(lack.corpus.terms == U32(7))), 0, 0, 0]


def test_shared_terms_membership():
    one = _fam("shared_terms").calls[0]
    member = {name: [q for q, ids in enumerate(one.queries) if t in ids.tolist()] for name, t in wc.SHARED.items()}
    assert member["all"] == list(range(64)) and member["ends"] == [0, 63] and member["odd"] == list(range(1, 64, 2)) and member["one"] == [17]
    at = [ids.tolist().index(wc.SHARED["all"]) for ids in one.queries]
    assert len(set(float(w[i]) for w, i in zip(one.idf, at))) == 64, "64 distinct idf values of one term"
    for ids in one.queries:
        shared = [i for i, t in enumerate(ids.tolist()) if t in wc.SHARED.values()]
        assert min(shared) >= 2 and max(shared) <= ids.size - 3, "private terms on both sides"
    keys = wc.pass_keys(one.queries)
    assert keys.index(wc.SHARED["all"]) < keys.index(wc.SHARED["ends"])                  # bases follow first appearance
    want = wc.expected(_fam("shared_terms").corpus, one)
    assert (want[2] > 10).all() and len(set(_bits(want[0][:, 0]).tolist())) > 32


# ------------------------------------------------------------------ walk families
def _tile_entry(corpus, row, j=0):
    """The position of entry j of ``row`` among its tile's entries."""
    return int(corpus.row_off[row] + j - corpus.row_off[row // 32 * 32])


def test_one_ballot_rows_finish_in_one_step():
    for n in (32, 64):
        fam = _fam("one_ballot_%d" % n)
        assert fam.corpus.n == n and (np.diff(fam.corpus.row_off) == 1).all()
        want = wc.expected(fam.corpus, fam.calls[0])
        assert want[2][0] == n and want[2][1] + want[2][2] == n, "every entry is a hit"


def test_long_row_straddles_every_edge():
    fam = _fam("long_row")
    c, one = fam.corpus, fam.calls[0]
    longs = np.flatnonzero(np.diff(c.row_off) == 1000)
    assert longs.size == len(wc.LONG_BEFORE) and [_tile_entry(c, int(r)) for r in longs] == [0, 1, 62, 193, 256]
    assert [int(r) % 32 for r in longs] == [0, 1, 1, 1, 3]
    hits = set(one.queries[0].tolist())
    for r in longs.tolist():
        ids = c.terms[c.row_off[r]:c.row_off[r + 1]].tolist()
        at = [_tile_entry(c, r, j) for j, t in enumerate(ids) if t in hits]
        assert len(at) == 32
        steps, outers = set(a // 64 for a in at), set(a // (64 * wc.STEPS) for a in at)
        assert outers == set(range(min(outers), max(outers) + 1)) and len(outers) >= 4, "hits in every outer iteration of the row"
        assert [a - _tile_entry(c, r) for a in at] == sorted(wc.LONG_AT) and len(steps) >= 12
        if _tile_entry(c, r) % 256 == 0:
            assert all({e - 1, e} <= set(a - _tile_entry(c, r) for a in at) for e in (64, 128, 192, 256, 320, 384, 512, 640, 768, 896, 960))
        last, nxt = _tile_entry(c, r, 999), _tile_entry(c, r + 1)
        assert nxt == last + 1 and last // 64 == nxt // 64 and ids[999] in hits and int(c.terms[c.row_off[r + 1]]) in hits
    first = longs[0]
    at0 = [j for j, t in enumerate(c.terms[c.row_off[first]:c.row_off[first + 1]].tolist()) if t in hits]
    assert at0 == sorted(wc.LONG_AT) and {63, 64, 127, 128, 255, 256, 257, 511, 512, 767, 768, 999} <= set(at0)
    want = wc.expected(c, one)
    assert want[2][0] == 10 and set(want[1][0, :5].tolist()) == set(longs.tolist())


def test_empty_rows_layout():
    fam = _fam("empty_rows")
    lens = np.diff(fam.corpus.row_off)
    assert fam.corpus.n == 128 and np.flatnonzero(lens).tolist() == [5, 10, 95, 96, 98, 127]
    assert _call(fam, "all_set").words.tolist() == [0xFFFFFFFF] * 4
    assert wc.expected(fam.corpus, fam.calls[0])[2].tolist() == [6, 6, 6]


def test_masked_between_layout():
    fam = _fam("masked_between")
    c, one = fam.corpus, _call(fam, "middle_out")
    mask = wc.call_mask(c, one)
    assert np.flatnonzero(~mask).tolist() == one.facts["masked"] == [1, 34]
    assert (np.diff(c.row_off)[:3] == 1).all() and c.terms[:3].tolist() == [40, 40, 40]
    ids = c.terms[c.row_off[34]:c.row_off[35]].tolist()
    at = [_tile_entry(c, 34, j) for j, t in enumerate(ids) if t in (40, 41)]
    assert at == [63, 64], "the masked row's hits lie on both sides of a step edge"
    assert {40, 41} & set(c.terms[c.row_off[33]:c.row_off[34]].tolist()) and 40 in c.terms[c.row_off[35]:c.row_off[36]].tolist()
    with_mask, without = wc.expected(c, one), wc.expected(c, _call(fam, "no_mask"))
    assert with_mask[2].tolist() == [4, 4, 1] and without[2].tolist() == [6, 6, 2]
    assert not set(with_mask[1].ravel().tolist()) & {1, 34}


def test_tails_shapes():
    for n, tiles, nrow in ((1, 1, 1), (31, 1, 31), (95, 3, 31), (129, 5, 1)):
        fam = _fam("tails_%d" % n)
        assert fam.corpus.n == n and (n + 31) // 32 == tiles and n - 32 * (tiles - 1) == nrow
        words = _call(fam, "all_set").words
        assert words.size == tiles and (words == 0xFFFFFFFF).all()
        a, b = wc.expected(fam.corpus, _call(fam, "all_set")), wc.expected(fam.corpus, _call(fam, "no_mask"))
        assert _same(a, b) and a[2][0] >= 1 and n - 1 in a[1][0].tolist(), "the last row qualifies"
    assert sorted((1, 3, 5)) == [1, 3, 5] and wc.WAVES == 4                              # fewer tiles than waves, one short, one more


def test_order_matters_under_another_order():
    fam = _fam("order_matters")
    c, one = fam.corpus, _call(fam, "closed")
    assert [tuple(w.tolist()) for w in one.idf] == [tuple(np.float32(v) for v in w) for w in wc.ORDER_WEIGHTS]
    assert sorted(set(tuple(sorted(w)) for w in wc.ORDER_WEIGHTS)) == [(-2.0 ** 25, 1.0, 2.0 ** 25)] and len(set(wc.ORDER_WEIGHTS)) == 6
    up, down = wc.row_scores(c, one), wc.row_scores(c, one, order="descending")
    full = [r for r in range(c.n) if c.row_off[r + 1] - c.row_off[r] == 3 and c.terms[c.row_off[r]] == 60]
    assert len(full) == 4
    for q in range(6):
        rows, scores, _ = up[q]
        for r in full:
            assert float(scores[rows.tolist().index(r)]) == wc.ORDER_SUMS[q], "the sum worked out by hand"
    assert any(not np.array_equal(_bits(a[1]), _bits(b[1])) for a, b in zip(up, down)), "descending ids give other bits"
    assert not _same(wc.closed_form(c, one, order="descending"), wc.closed_form(c, one))
    bm = _call(fam, "bm25")
    assert (c.dl == 2 ** 24 + 1).sum() >= 4 and (c.tf == 255).sum() >= 8 and bm.k1 == wc.K1
    assert np.float32(2 ** 24 + 1) == np.float32(2 ** 24)


# ------------------------------------------------------------------ cut and select families
@pytest.mark.parametrize("name", [n for n in FAMILIES if n.startswith("cut_")])
def test_cut_cases_sit_in_the_stated_buckets(name):
    fam = _fam(name)
    one = fam.calls[0]
    k = one.k
    per_query = wc.row_scores(fam.corpus, one)
    seen = {}
    for sub, facts, (rows, scores, exact) in zip(one.facts["subs"], one.facts["sub_facts"], per_query):
        assert exact, "no addition rounds: the closed form is the exact sum"
        B, M, count, tid, i = wc.cut_model(scores, k)
        assert count == facts["count"] == rows.size, sub
        ranked = sorted((wc.ord32(s) for s in scores), reverse=True)
        if "kth" in facts:
            assert B == facts["kth"] == ranked[k - 1] >> 16, sub
        if "nxt" in facts:
            assert ranked[k] >> 16 == facts["nxt"], sub
        if "m" in facts:
            assert M == facts["m"], sub
        if "kth_chunk" in facts and count >= k:
            assert tid == facts["kth_chunk"], sub
        seen[sub] = (B, M, count, tid, i)
    if set(seen) >= {"i0", "neg_i0"}:
        assert seen["i0"][3:] == (0xC0, 0) and seen["i255"][3:] == (0xBF, 255) and seen["neg_i0"][3:] == (0x40, 0) and seen["neg_i255"][3:] == (0x3F, 255)
        assert seen["i0"][1] == k and seen["zero"][0] == 0x8000
        zero = per_query[one.facts["subs"].index("zero")][1]
        assert (zero > 0).sum() == k - 1 and (zero < 0).sum() > 5 and (_bits(zero) == 0).sum() == 2, "+0.0 itself, rows above and below"
    if set(seen) >= {"chunk0", "m_eq_k"}:
        assert seen["chunk0"][3] == 0 and seen["chunk255"][3] == 255
        assert seen["m_eq_k"][1] == k and seen["count_eq_k"][:3] == (seen["count_eq_k"][0], k, k) and seen["count_eq_km1"][:3] == (0, k - 1, k - 1)
        bottom = per_query[one.facts["subs"].index("chunk0")][1]
        assert np.isfinite(bottom).all() and (bottom < 0).all()
    want = wc.expected(fam.corpus, one)
    assert want[2].tolist() == [f["count"] for f in one.facts["sub_facts"]]


def test_crowded_bucket_and_identical_rows():
    fam = _fam("crowded")
    c = fam.corpus
    assert c.n == 5000 and (c.n + 31) // 32 == 157
    one = _call(fam, "crowded_k10")
    rows, scores, exact = wc.row_scores(c, one)[0]
    assert exact and rows.size == 5000 and set(wc.bucket(s) for s in scores) == {0xC000} and np.unique(_bits(scores)).size == 3000
    assert wc.cut_model(scores, 10)[:3] == (0xC000, 5000, 5000)
    same = _call(fam, "identical_k1024")
    rows, scores, exact = wc.row_scores(c, same)[0]
    assert exact and rows.size == 5000 and np.unique(_bits(scores)).size == 1 and same.row_base == 3 << 32
    want = wc.closed_form(c, same)
    assert want[1][0].tolist() == list(range(3 << 32, (3 << 32) + 1024)) and want[2][0] == 5000
    assert sorted(set(one.k for one in fam.calls)) == [1, 10, 1024]


# ------------------------------------------------------------------ statistics
@pytest.mark.parametrize("name", sorted(wc.stats_families()))
def test_stats_cases(name):
    corpus, ids = wc.stats_families()[name]
    distinct = len(dict.fromkeys(ids.tolist()))
    walks = {"ids_2048": 1, "ids_2049": 2, "ids_4100": 3}.get(name)
    if walks:
        assert distinct == ids.size == int(name[4:]) and -(-distinct // wc.MAX_KEYS) == walks
    if name == "repeats":
        first = list(dict.fromkeys(ids.tolist()))
        chunk = {t: i // wc.MAX_KEYS for i, t in enumerate(first)}
        again = [t for i, t in enumerate(ids.tolist()) if t in ids[:i].tolist()]
        assert {chunk[t] for t in again} == {0, 1} and len(again) >= 10, "repeated ids of both chunks"
    er = lc.row_ids(corpus.row_off)
    for kind in wc.STATS_MASKS:
        df, rows, sum_dl = wc.stats_expected(name, kind)
        words = wc.stats_mask(corpus, kind)
        ok = np.ones(corpus.n, bool) if words is None else lc.mask_from_words(words, corpus.n)
        order = np.argsort(corpus.terms, kind="stable")                          # an independent count: sort, then bisect
        st, sok = corpus.terms[order], ok[er[order]]
        cum = np.concatenate([[0], np.cumsum(sok)])
        lo, hi = np.searchsorted(st, ids.astype(U32), "left"), np.searchsorted(st, ids.astype(U32), "right")
        assert np.array_equal(df, cum[hi] - cum[lo]) and rows == int(ok.sum()) and sum_dl == int(corpus.dl[ok].sum())
        if kind == "clear":
            assert rows == 0 and not df.any()
        if kind == "random":
            assert 0 < rows < corpus.n // 8
    if name.startswith("ids_"):
        assert (wc.stats_expected(name, "none")[0] > 0).sum() >= 2048
