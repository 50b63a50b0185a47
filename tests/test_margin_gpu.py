"""The worst-case rounding inputs of tests/margin_cases.py on the real index, every route, both stores, both nomination policies:
rows, score bits, counts and stored bits all EQUAL the oracle's -- there is no tolerance in this file.

The adversarial pair (proved on the host by tests/test_margin_cases_host.py): for the query q the oracle ranks row A above row
B by 8e-5, while a scan over the bf16 images of an f32 store scores B 1.0e-2 above A.  A margin below the true bound of
|scan - canonical| (margin_for in crh_index.hip) drops A before the canonical re-score and returns the wrong top-1.  On a bf16
store the scan and the canonical score read the same values, B leads there, and the same cases pin that nothing changed.

The boundary rows sit one ulp either side of each threshold of cosine preprocessing, depend on the order of its sum, overflow
it, or divide into subnormals; they are checked as stored rows (k_append) and as queries (k_prep_queries)."""
import functools

import numpy as np
import pytest

from oracle import search as orc
from tests import margin_cases as mc
from tests import range_cases

pytestmark = pytest.mark.gpu
U32, F32 = np.uint32, np.float32
N_BY = 2048             # Gaussian bystander rows (their scores against q stay below 0.2)
NQ = 65                 # one query more than a 64-query pass: the wide scan's smallest batch
Q_AT = 33               # where q sits in the batch (second 32-column block)
RARE = 99               # the code only the rows around A and B carry: 2-3 of the 65 tiles


def _ffi():
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    return ffi


@pytest.fixture(params=["int8 copy from 0 rows", "product default"])
def policy(request, monkeypatch):
    """tests/conftest.py lets every index of the GPU tier nominate from its int8 copy (CODERAG_HIP_I8_MIN_ROWS=0); at these row
    counts the PRODUCT's default is the scan over the bf16 tiles, whose margin this file is about: every case runs under both
    (the fixture of tests/test_search_gpu.py)."""
    if request.param == "product default":
        monkeypatch.delenv("CODERAG_HIP_I8_MIN_ROWS", raising=False)
    return request.param


def _same(got, want, what):
    assert np.array_equal(np.asarray(got[1]), want[1]), f"{what}: rows differ: {np.asarray(got[1])[:, :3].tolist()[:3]} vs {want[1][:, :3].tolist()[:3]}"
    assert np.array_equal(np.ascontiguousarray(got[0], F32).view(U32), want[0].view(U32)), f"{what}: score bits differ"


@functools.lru_cache(maxsize=4)
def _case(dim: int, bf16: bool, variant: str, layout: str):
    """One corpus with the pair in it, the batch of queries and everything the oracle says about them (read only).
    layout "edge": A and B in rows 31 and 32, either side of a tile edge, searched with k = 1;
    layout "tail": ten copies of B and then A in the last row of a ragged last tile, searched with k = 10."""
    q, a, b, _ = mc.adversarial_pair(dim, variant)
    rng = np.random.default_rng(dim + 7 * bf16)
    by = rng.standard_normal((N_BY, dim), dtype=F32) * rng.uniform(0.2, 5.0, size=(N_BY, 1)).astype(F32)
    if layout == "edge":
        x = np.concatenate([by[:31], a[None], b[None], by[31:]])
        ia, ibs, k = 31, [32], 1
    else:
        x = np.concatenate([by, np.repeat(b[None], 10, axis=0), a[None]])
        ia, ibs, k = N_BY + 10, list(range(N_BY, N_BY + 10)), 10
    n = len(x)
    codes = (np.arange(n) % 5).astype(np.int32)[:, None].copy()
    codes[max(0, ia - 20):ia + 15, 0] = RARE
    rare = codes[:, 0] == RARE
    assert rare[ia] and rare[ibs].all()
    qs = rng.standard_normal((NQ, dim), dtype=F32)
    qs[Q_AT] = q
    xp, qp = orc.preprocess(x, bf16), orc.preprocess(qs, bf16)
    if not bf16:                                                           # stored and used as built
        assert np.array_equal(xp[[ia] + ibs].view(U32), x[[ia] + ibs].view(U32)) and np.array_equal(qp[Q_AT].view(U32), q.view(U32))
    scores = orc.scores(xp, qp)
    sa, sb = scores[Q_AT, ia], scores[Q_AT, ibs[0]]
    assert (sa > sb) == (not bf16) and sa != sb                            # f32: A leads; bf16: the rounded rows are ranked, B leads
    assert np.delete(scores[Q_AT], [ia] + ibs).max() < 0.3 < min(sa, sb)
    thr = np.sort(scores, axis=1)[:, -3].copy()                            # the other queries: their third best score, inclusive
    thr[Q_AT] = F32((np.float64(sa) + np.float64(sb)) / 2)                 # q: half-way between A and B
    return dict(x=x, codes=codes, rare=rare, qs=qs, xp=xp, qp=qp, scores=scores, thr=thr.astype(F32), ia=ia, ibs=ibs, k=k, n=n,
                plain=orc.search(xp, qp, k), filtered=orc.search(xp, qp, k, alive=rare.astype(np.uint8)))


def _take(want, sel):
    return want[0][sel], want[1][sel]


@pytest.mark.parametrize("variant", mc.VARIANTS)
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("dim", mc.DIMS)
def test_adversarial_pair_on_every_route(gpu, monkeypatch, policy, dim, bf16, variant):
    ffi = _ffi()
    dt = ffi.DTYPE_BF16 if bf16 else ffi.DTYPE_F32
    per_pass = 32 if dim > 1024 else 64
    for layout in ("edge", "tail"):
        c = _case(dim, bf16, variant, layout)
        k, n, ia, ibs, qs = c["k"], c["n"], c["ia"], c["ibs"], c["qs"]
        first = [ia] + ibs[:k - 1] if not bf16 else (ibs + [ia])[:k]
        assert c["plain"][1][Q_AT].tolist() == first                       # what the oracle says: A first (f32) / B first (bf16)
        default = ffi.Index(dim, dt, capacity_rows=n, n_code_cols=1)
        monkeypatch.setenv("CODERAG_HIP_FUSED_SCAN", "0")
        three = ffi.Index(dim, dt, capacity_rows=n, n_code_cols=1)          # seed scan, thresholds, main scan as three launches
        monkeypatch.delenv("CODERAG_HIP_FUSED_SCAN")
        try:
            for idx in (default, three):
                idx.append(c["x"], c["codes"])
            tag = f"{layout} dim {dim} {'bf16' if bf16 else 'f32'} {variant}"
            # the policy's own route (int8 copy / one-launch bf16 scan; dim 1024 has no one-launch form), q alone and in a batch
            _same(default.search(qs[Q_AT:Q_AT + 1], k), _take(c["plain"], slice(Q_AT, Q_AT + 1)), f"{tag}: default, q alone")
            _same(default.search(qs[:64], k), _take(c["plain"], slice(0, 64)), f"{tag}: default, 64 queries")
            if policy == "product default":
                assert default.nomination() in (ffi.NOMINATE_BF16, ffi.NOMINATE_BF16_3)
            # the three-launch form
            _same(three.search(qs[Q_AT:Q_AT + 1], k), _take(c["plain"], slice(Q_AT, Q_AT + 1)), f"{tag}: three launches, q alone")
            _same(three.search(qs[:64], k), _take(c["plain"], slice(0, 64)), f"{tag}: three launches, 64 queries")
            assert three.nomination() == ffi.NOMINATE_BF16_3
            # the bf16-tile scans whatever the policy: one launch where the width has it, and the wide scan (65 queries, one pass)
            default.set_nomination(ffi.NOMINATE_BF16)
            _same(default.search(qs[:64], k), _take(c["plain"], slice(0, 64)), f"{tag}: bf16 tiles, 64 queries")
            if dim <= 768:
                _same(default.search(qs, k), c["plain"], f"{tag}: wide scan")
                assert default.stats()["batches"] == 1
            # the tile-list route behind a filter that leaves 2-3 tiles
            listed = len(np.unique(np.flatnonzero(c["rare"]) // 32))
            assert listed * 4 <= (n + 31) // 32
            default.set_sparse_route(True)
            got = default.search(qs[:64], k, filters=[(0, RARE)])
            st = default.stats()
            assert st["tiles"] == listed * st["batches"], st
            _same(got, _take(c["filtered"], slice(0, 64)), f"{tag}: tile list")
            # a mixed-filter batch: q once under each class
            sel = np.arange(Q_AT + 1 - per_pass, Q_AT + 1) if per_pass <= Q_AT else np.arange(per_pass)      # one pass of queries, q among them
            for flip in (0, 1):
                qclass = (sel + flip) % 2
                want_s = np.where((qclass == 1)[:, None], c["filtered"][0][sel], c["plain"][0][sel])
                want_r = np.where((qclass == 1)[:, None], c["filtered"][1][sel], c["plain"][1][sel])
                _same(default.search_multi(qs[sel], k, [None, [(0, RARE)]], qclass), (want_s, want_r),
                      f"{tag}: search_multi, q in class {(Q_AT + flip) % 2}")
            # the threshold half-way between the two: one row in range on an f32 store (A), B's copies on a bf16 store
            want = range_cases.select(c["scores"][:64], c["thr"][:64], 10, None)
            assert want[2][Q_AT] == (len(ibs) if bf16 else 1) and want[1][Q_AT, 0] == (ibs[0] if bf16 else ia)
            for counts in (True, False):
                s, r, cnt = three.search_range(qs[:64], 10, c["thr"][:64], counts=counts)
                _same((s, r), want[:2], f"{tag}: search_range counts={counts}")
                assert cnt is None if not counts else np.array_equal(cnt, want[2]), f"{tag}: in-range counts"
            s, r, cnt = default.search_range(qs[Q_AT:Q_AT + 1], 10, c["thr"][Q_AT:Q_AT + 1], filters=[(0, RARE)])
            _same((s, r), (want[0][Q_AT:Q_AT + 1], want[1][Q_AT:Q_AT + 1]), f"{tag}: search_range over the tile list")
            assert cnt.tolist() == [want[2][Q_AT]]
        finally:
            default.close()
            three.close()


def _rows_on_device(ffi, idx, rows):
    import torch
    out = idx.gather_vectors(torch.from_numpy(np.asarray(rows, np.int64)).cuda())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("dim", mc.DIMS)
def test_boundary_rows_stored_gathered_compacted_and_as_queries(gpu, policy, dim, bf16):
    ffi = _ffi()
    b = mc.boundary_rows(dim)
    nb, nv = len(b.raw), len(b.verbatim)
    rng = np.random.default_rng(dim)
    by = rng.standard_normal((300, dim), dtype=F32) * rng.uniform(0.2, 5.0, size=(300, 1)).astype(F32)
    # rows 0..39 bystanders, 40..40+nb-1 the boundary rows, bystanders; the second append starts mid-tile AND inside the boundary rows
    raw = np.concatenate([by[:40], b.raw, by[40:200]])
    cut = 40 + nb // 2
    assert cut % 32 != 0 and 40 < cut < 40 + nb
    want = np.concatenate([orc.preprocess(raw, bf16), mc.bf16_round(b.verbatim) if bf16 else b.verbatim, orc.preprocess(by[200:], bf16)])
    idx = ffi.Index(dim, ffi.DTYPE_BF16 if bf16 else ffi.DTYPE_F32, capacity_rows=512)
    try:
        idx.append(raw[:cut])
        idx.append(raw[cut:])
        assert idx.append(b.verbatim, preprocessed=True) == len(raw)         # stored verbatim (a bf16 store rounds them, ties to even)
        idx.append(by[200:])
        n = len(want)
        assert idx.count() == (n, n)
        kept = ~b.divided
        assert np.array_equal(want[40:40 + nb][kept].view(U32), b.raw[kept].view(U32)) or bf16      # the rows preprocessing keeps, bit for bit
        pick = np.concatenate([np.arange(38, 42 + nb), [-1], np.arange(len(raw) - 1, len(raw) + nv + 1), [n - 1, 0]])
        want_pick = np.where((pick >= 0)[:, None], want[pick], F32(0))

        def stored(tag):
            assert np.array_equal(idx.read_rows(0, idx.count()[0]).view(U32), want.view(U32)), f"{tag}: read_rows"
            assert np.array_equal(_rows_on_device(ffi, idx, pick).view(U32), want_pick.view(U32)), f"{tag}: gather_vectors"

        stored("after the appends")
        # every boundary row as a query (k_prep_queries), the zero query among them
        queries = np.concatenate([b.raw, b.verbatim])
        qp = orc.preprocess(queries, bf16)
        k = 10
        got = idx.search(queries, k)
        _same(got, orc.search(want, qp, k), "boundary rows as queries")
        for name in ("zero", "overflow"):                                  # nothing to rank by: rows 0 .. k-1 at score +0
            i = b.names.index(name)
            assert not qp[i].any() and got[1][i].tolist() == list(range(k)) and not got[0][i].view(U32).any(), name
        stored("after a search")                                           # (a bf16 store has built its row-major side copy by now)
        dead = np.asarray([3, 39, 40 + nb, n - 2])                          # bystanders next to the boundary rows and at the ends
        idx.tombstone(dead)
        alive = np.ones(n, bool)
        alive[dead] = False
        _same(idx.search(queries, k), orc.search(want, qp, k, alive=alive.astype(np.uint8)), "with tombstones")
        o2n = idx.compact()
        assert np.array_equal(o2n, np.where(alive, np.cumsum(alive) - 1, -1))
        want = want[alive]
        pick = np.concatenate([np.arange(36, 40 + nb), [-1, len(want) - 1, 0]])
        want_pick = np.where((pick >= 0)[:, None], want[pick], F32(0))
        stored("after compact()")
        _same(idx.search(queries, k), orc.search(want, qp, k), "after compact()")
        stored("after compact() and a search")
    finally:
        idx.close()
