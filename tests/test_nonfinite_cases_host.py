"""The cases of tests/nonfinite_cases.py proved on the CPU, so that tests/test_nonfinite_gpu.py cannot pass vacuously: the
restated oracle leaves NaN scores out, the corpora really hold what their builders promise, and every *_cases.py restatement the
store-level test leans on follows the rule (a NaN score is no score)."""
import asyncio

import numpy as np
import pytest

from oracle import search as orc
from tests import lifecycle_cases as lc
from tests import nonfinite_cases as nf

F32 = np.float32
DIMS = (768, 384, 1536)
LISTS = [(10, False), (100, True), (1024, False)]            # (k, under the 40-row filter)


def test_the_70_row_probe_returns_67_hits():
    """70 Gaussian rows of dim 768, a NaN in row 0, +inf in row 33, -inf in row 69, k = 100 and k = 10: before the rule the oracle
    returned 70 hits with the three rows at list positions 0, 33 and 69 under score NaN."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal((70, 768)).astype(F32)
    x[0, 5], x[33, 7], x[69, 9] = np.nan, np.inf, -np.inf
    q = rng.standard_normal((1, 768)).astype(F32)
    for bf16 in (False, True):
        s, r = orc.cosine_search(x, q, 100, bf16=bf16)
        assert int((r >= 0).sum()) == 67 and not set(r[0].tolist()) & {0, 33, 69} and nf.well_formed(s, r)
        s10, r10 = orc.cosine_search(x, q, 10, bf16=bf16)
        assert nf.same_lists(s10, r10, s[:, :10], r[:, :10])
        al = orc.scores(orc.preprocess(x, bf16), orc.preprocess(q, bf16))
        assert np.isnan(al[0, [0, 33, 69]]).all() and int(np.isnan(al).sum()) == 3          # orc_scores reports the NaN as it is


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("kind", ["gauss", "sunk"])
def test_expected_lists_are_sorted_free_of_nan_and_hold_no_bad_row(kind, bf16):
    _, codes, bad = nf.corpus(kind)
    q, qbad = nf.queries(kind)
    al = orc.scores(nf.stored(kind, 768, bf16), orc.preprocess(q, to_bf16=bf16))
    assert np.array_equal(np.isnan(al), qbad[:, None] | bad[None, :])                       # NaN exactly where a bad row or query is involved
    passing = codes[:, 1] == 9
    assert passing.sum() == 40 and (passing & bad).sum() == 3 and np.array_equal(np.flatnonzero(passing), nf.FILTER_ROWS)
    tiles = np.unique(nf.FILTER_ROWS // nf.TILE)
    assert tiles.size * 4 <= (nf.N + 31) // 32                                               # sparse by the library's crossover of 1 tile in 4
    assert np.unique(np.flatnonzero(bad) // nf.TILE).size >= 10                             # bad rows in at least k = 10 tiles
    for k, filtered in LISTS:
        s, r = nf.expected(kind, 768, bf16, 64, k, filtered)
        assert nf.well_formed(s, r)
        hits = (r >= 0).sum(1)
        ok = (passing if filtered else np.ones(nf.N, bool)) & ~bad
        assert (hits[qbad] == 0).all() and (hits[~qbad] == min(k, int(ok.sum()))).all()
        assert not bad[r[r >= 0]].any()
        if filtered:
            assert int(ok.sum()) == 37 < k                                                   # fewer than k rows pass: every one is a survivor
        # an independent statement of the same lists: numpy on the score matrix, NaN left out by `>=`
        from tests import range_cases
        ws, wr, _ = range_cases.select(al, -np.inf, k, passing if filtered else None)
        assert nf.same_lists(s, r, ws, wr)
    if kind == "sunk":
        finite = np.where(bad[None, :], -np.inf, al)[~qbad]
        assert (np.sort(finite, axis=1)[:, -1] < 0).all()                                   # the BEST finite score is below 0, the k-th too


@pytest.mark.parametrize("bf16", [False, True])
def test_a_bad_query_changes_nothing_for_its_neighbours(bf16):
    for kind in ("gauss", "sunk"):
        for nq in (64, 65, 200):
            _, qbad = nf.queries(kind, 768, nq)
            assert qbad[[0, 31, 32, 63]].all() and 4 < qbad.sum() < nq // 4
            s, r = nf.expected(kind, 768, bf16, nq, 10)
            zs, zr = nf.expected(kind, 768, bf16, nq, 10, False, False)
            assert (r[qbad] == -1).all() and np.isneginf(s[qbad]).all()
            assert nf.same_lists(s[~qbad], r[~qbad], zs[~qbad], zr[~qbad]) and (zr[~qbad][:, -1] >= 0).all()


@pytest.mark.parametrize("dim", DIMS)
def test_each_bad_raw_row_preprocesses_to_the_nan_pattern(dim):
    raw, _, bad = nf.corpus("gauss", dim)
    for bf16 in (False, True):
        st = nf.stored("gauss", dim, bf16)
        assert np.array_equal(np.isnan(st).any(1), bad) and not np.isinf(st).any()
        for r in np.flatnonzero(bad):
            assert np.array_equal(np.isnan(st[r]), nf.nan_pattern(raw[r])), r
            assert not st[r][~np.isnan(st[r])].any() or np.isnan(raw[r]).any()              # an infinite row: zeros around its NaN
        assert nf.same_stored(st, st.copy()) and not nf.same_stored(st, np.where(np.isnan(st), F32(0), st))
    kinds = set(nf.bad_rows().values())
    assert kinds == set(nf.KINDS) and {0, 31, 32, nf.N - 1} <= set(nf.bad_rows()) and len(nf.bad_rows()) == 43


def test_the_store_model_follows_the_rule_on_every_vector_scored_path():
    """tests/lifecycle_cases.py with five non-finite points among 300: every vector-scored expectation is that of the model
    WITHOUT them (so range_cases, mmr_cases, group_cases, span_cases, fuse_cases and recommend_cases leave NaN out wherever they
    rank or count), every other one still sees them."""
    for bf16 in (False, True):
        with_, without = nf.store_models(bf16)
        names = []
        for (name, feature, want, _), (_, _, ref, _) in zip(lc.checks(with_.view(bf16), nf.sums_model().view(bf16)), lc.checks(without.view(bf16), nf.sums_model().view(bf16))):
            if feature in nf.SCORED or name in nf.SCORED_NAMES:
                w, r = want(), ref()
                if hasattr(w, "__await__"):
                    w, r = asyncio.run(_both(w, r))
                assert w == r, name
                assert not lc._nothing(w) or name == "a value never stored", name
                names.append(name)
            elif name in nf.SEES_THEM:
                assert want() != ref(), name
                names.append(name)
        assert set(nf.SCORED_NAMES) | set(nf.SEES_THEM) <= set(names) and len(names) >= 25, names
        for strategy, want in (("average", []), ("best", None)):
            got = lc._recommend(with_.view(bf16), [nf.BAD_IDS[0], lc.EXAMPLES[0][1]], lc.EXAMPLES[1], 6, strategy, with_.view(bf16).mask(None, lc.F_NOT, "recommend"))
            ref = lc._recommend(without.view(bf16), [lc.EXAMPLES[0][1]], lc.EXAMPLES[1], 6, strategy, without.view(bf16).mask(None, lc.F_NOT, "recommend"))
            if want is None:                       # best: the bad positive scores nothing, the answer is that of the other positive alone
                assert [g[:4] for g in got] == [g[:4] for g in ref] and len(got) == 6 and all(g[4] == lc.EXAMPLES[0][1] for g in got)
            else:                                  # average: the query is NaN, similar to nothing
                assert got == want


async def _both(a, b):
    return await a, await b
