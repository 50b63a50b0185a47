"""The keyword search on the device at the inputs of tests/lex_walk_cases.py -- the largest term table, probe chains that wrap,
term ids 0 and 0xFFFFFFFF, terms shared between queries under different idf values, tile walks over step and outer-iteration
edges, histogram cuts in chosen buckets, a crowded bucket, identical rows, several walks of ``crh_lex_stats`` -- against the
restatement ``lex_cases.bm25_search`` and, where a case has one, the closed form: counts, rows, score BITS and padding, into
outputs pre-filled with garbage.  No tolerance appears anywhere.  tests/test_lex_walk_cases_host.py proves without a GPU that
each case is the case it claims to be.  Every family runs twice on its handle, with a call of another table size in between:
stale workspace (histogram, control words, a larger previous table image, a longer candidate list) must not leak in."""
import numpy as np
import pytest

from tests import lex_walk_cases as wc

pytestmark = pytest.mark.gpu

U32 = np.uint32
FAMILIES = sorted(wc.families())

_handles = {}            # one device index per corpus, kept for the module


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(U32)


def _lex(corpus):
    from coderag_amd import ffi
    if id(corpus) not in _handles:
        lex = ffi.Lex(capacity_rows=corpus.n, device=0)
        lex.append(corpus.row_off, corpus.terms, corpus.tf, corpus.dl)
        assert lex.count() == (corpus.n, int(corpus.row_off[-1]))
        _handles[id(corpus)] = (lex, corpus)
    return _handles[id(corpus)][0]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for lex, _ in _handles.values():
        lex.close()
    _handles.clear()


def _words_dev(words):
    import torch
    return None if words is None else torch.from_numpy(np.asarray(words, U32).view(np.int32).copy()).to("cuda:0")


def _search(corpus, one):
    import torch
    nq = len(one.queries)
    outs = (torch.full((nq, one.k), -77.0, dtype=torch.float32, device="cuda:0"), torch.full((nq, one.k), -77, dtype=torch.int64, device="cuda:0"),
            torch.full((nq,), -77, dtype=torch.int64, device="cuda:0"))
    got = _lex(corpus).search(one.queries, one.idf, one.k, one.k1, one.b, float(one.avgdl), mask=_words_dev(one.words), row_base=one.row_base,
                              out_scores=outs[0], out_rows=outs[1], out_count=outs[2])
    torch.cuda.synchronize()
    return tuple(g.cpu().numpy() for g in got)


def _equal(got, want, what):
    s, r, c = got
    assert np.array_equal(c, want[2]), what + ": counts differ"
    assert np.array_equal(r, want[1]), what + ": rows differ"
    assert np.array_equal(_bits(s), _bits(want[0])), what + ": score bits differ"
    assert np.isneginf(s[r < 0]).all() and (_bits(s[r < 0]) == 0xFF800000).all(), what + ": padding is not (-inf, -1)"


@pytest.mark.parametrize("name", FAMILIES)
def test_search_family(gpu, name):
    fam = wc.families()[name]
    wants = []
    for one in fam.calls:
        want = wc.expected(fam.corpus, one)                                  # (a) the restatement
        if wc.has_closed_form(one):                                          # (b) the closed form, where the case has one
            closed = wc.closed_form(fam.corpus, one)
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(want, closed)), one.name
        wants.append(want)
    for one, want in zip(fam.calls, wants):
        _equal(_search(fam.corpus, one), want, one.name)
    between = wc.interloper(fam)
    _equal(_search(fam.corpus, between), wc.expected(fam.corpus, between), between.name)
    for one, want in zip(fam.calls, wants):
        _equal(_search(fam.corpus, one), want, one.name + " (again, after a table of another size)")


@pytest.mark.parametrize("kind", wc.STATS_MASKS)
@pytest.mark.parametrize("name", sorted(wc.stats_families()))
def test_stats_family(gpu, name, kind):
    import torch
    corpus, ids = wc.stats_families()[name]
    df, rows, sum_dl = _lex(corpus).stats(ids.astype(U32), _words_dev(wc.stats_mask(corpus, kind)))
    torch.cuda.synchronize()
    wdf, wrows, wsum = wc.stats_expected(name, kind)
    assert np.array_equal(df, wdf) and (rows, sum_dl) == (wrows, wsum)
