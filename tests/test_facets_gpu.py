"""Facets on the device against the CPU restatement (tests/facet_cases.py): crh_index_facet on both of its routes,
crh_facet_select on synthesised histograms, crh_search_range_facet on the thresholds of tests/range_cases.py, and the store on one
and three shards against the store over fake indexes.  Every count is exact."""
import asyncio

import numpy as np
import pytest

from tests import facet_cases as fc, range_cases

pytestmark = pytest.mark.gpu
DIM = 384
GENS = tuple(fc.GENERATORS)
COL_A, COL_B, COL_LINE, COL_RARE = len(GENS), len(GENS) + 1, len(GENS) + 2, len(GENS) + 3


def _columns(n):
    """One facet column per generator, then the filter columns: row % 7, row % 5, the row number (a numeric column) and a value
    only 40 consecutive rows carry (two or three tiles: the tile-list route from a few thousand rows on)."""
    cols = [fc.codes_for(g, n, seed=i) for i, g in enumerate(GENS)]
    rare = np.zeros((n,), np.int32)
    rare[n // 3:n // 3 + 40] = 99
    return np.stack(cols + [np.arange(n) % 7, np.arange(n) % 5, np.arange(n), rare], 1).astype(np.int32)


def _index(ffi, raw, codes, dtype, dead):
    idx = ffi.Index(raw.shape[1], dtype, capacity_rows=len(raw), n_code_cols=codes.shape[1], device=0)
    idx.append(raw, codes)
    if len(dead):
        idx.tombstone(dead)
    return idx


def _host(pair):
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


@pytest.mark.parametrize("n,bf16", [(1, True), (31, False), (32, True), (33, False), (255, True), (257, False), (4099, True), (20011, False)])
def test_index_facet_equals_the_restatement_on_both_routes(gpu, n, bf16):
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from tests import span_cases
    rng = np.random.default_rng(n)
    raw = rng.standard_normal((n, DIM), dtype=np.float32)
    codes = _columns(n)
    dead = np.arange(5, n, 11).astype(np.int64)
    alive = np.ones((n,), bool)
    alive[dead] = False
    # a row bitmap with whole empty tiles: only every third tile holds bits at all
    bits = rng.random(n) < 0.5
    bits[(np.arange(n) // 32) % 3 != 0] = False
    padded = np.zeros(((n + 31) // 32) * 32, np.uint8)
    padded[:n] = bits
    words = torch.from_numpy(np.packbits(padded, bitorder="little").view(np.int32).copy()).cuda()
    conds = {"none": (None, alive),
             "equality": ([(COL_A, 3)], None),
             "negated set": ([(COL_B, [1, 2], True)], None),
             "line range": ([(COL_LINE, n // 4, (3 * n) // 4, "between")], None),
             "row bitmap": ([ffi.RowWords(ffi.next_words_tag(), words)], alive & bits),
             "sparse": ([(COL_RARE, 99)], None)}
    L = ffi.FACET_LDS_BINS
    idx = _index(ffi, raw, codes, ffi.DTYPE_BF16 if bf16 else ffi.DTYPE_F32, dead)
    try:
        for name, (filt, passing) in conds.items():
            if passing is None:
                passing = span_cases.np_mask(codes, alive, filt)
            assert idx.count_matching(filt) == int(passing.sum()), name
            if name == "sparse" and n >= 4099:
                assert len(np.unique(np.flatnonzero(passing) // 32)) * 4 <= (n + 31) // 32       # sparse enough for the tile list
            for g, gen in enumerate(GENS):
                top = int(codes[:, g].max())
                got = {}
                for n_bins in (L - 1, L, L + 1, 1, top + 5, max(top // 2, 1)):
                    bins, info = _host(idx.facet(g, n_bins, filters=filt))
                    wb, wi = fc.histogram(codes[:, g], passing, n_bins)
                    assert np.array_equal(info, wi), f"{name} {gen} n_bins {n_bins}: info {info.tolist()} vs {wi.tolist()}"
                    assert np.array_equal(bins, wb), f"{name} {gen} n_bins {n_bins}: bins differ at {np.flatnonzero(bins != wb)[:8].tolist()}"
                    assert bins.sum() + info[1] + info[2] == info[0] == passing.sum()
                    got[n_bins] = bins
                assert np.array_equal(got[L][: L - 1], got[L - 1]) and np.array_equal(got[L + 1][:L], got[L])      # the two routes agree
        # every slot is overwritten, an output pair is reused
        out = (torch.full((7,), -9, dtype=torch.int64, device="cuda"), torch.full((3,), -9, dtype=torch.int64, device="cuda"))
        assert idx.facet(COL_A, 7, out=out)[0] is out[0]
        assert np.array_equal(out[0].cpu().numpy(), np.bincount(codes[alive, COL_A], minlength=7)) and out[1].cpu().tolist() == [int(alive.sum()), 0, 0]
    finally:
        idx.close()


def test_index_facet_arguments_and_the_empty_index(gpu):
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    empty = ffi.Index(DIM, ffi.DTYPE_BF16, capacity_rows=64, n_code_cols=2, device=0)
    try:
        bins, info = empty.facet(1, 5)
        assert bins.cpu().tolist() == [0] * 5 and info.cpu().tolist() == [0, 0, 0]
        bins, info = empty.search_range_facet(np.ones((3, DIM), np.float32), 0.5, 0, 4)
        assert bins.cpu().tolist() == [[0] * 4] * 3 and info.cpu().tolist() == [[0, 0, 0]] * 3
        L = ffi.lib()
        b, i = torch.zeros((4,), dtype=torch.int64, device="cuda"), torch.zeros((3,), dtype=torch.int64, device="cuda")
        for col, n_bins, word in ((2, 4, b"column"), (-1, 4, b"column"), (0, 0, b"n_bins")):
            assert L.crh_index_facet(empty._handle(), col, None, 0, n_bins, b.data_ptr(), i.data_ptr(), None) == ffi.E_INVALID
            assert word in L.crh_last_error()
            q, t = np.ones((1, DIM), np.float32), np.zeros((1,), np.float32)
            assert L.crh_search_range_facet(empty._handle(), 1, q.ctypes.data, 0, t.ctypes.data, None, 0, col, n_bins, b.data_ptr(), i.data_ptr(), None) == ffi.E_INVALID
        with pytest.raises(ffi.NativeError, match="finite"):
            empty.search_range_facet(np.ones((1, DIM), np.float32), np.nan, 0, 4)
        with pytest.raises(ffi.NativeError, match="column"):
            empty.facet(0, 4, filters=[(5, [1, 2])])
        for k in (0, ffi.MAX_K + 1):
            with pytest.raises(ffi.NativeError, match="facet_select"):
                ffi.facet_select(torch.zeros((1, 4), dtype=torch.int64, device="cuda"), k)
    finally:
        empty.close()


def _synth(n_bins, rng):
    """Histograms of ``n_bins`` bins, one per edge case of the selection."""
    big = np.int64(1) << 33
    zero = np.zeros((n_bins,), np.int64)
    few = zero.copy()
    few[rng.choice(n_bins, min(n_bins, 4), replace=False)] = rng.integers(1, 50, min(n_bins, 4))
    ties = rng.integers(0, 3, n_bins).astype(np.int64) * 7                      # hundreds of bins at 7 and at 14: the cut falls among equals
    ties[rng.choice(n_bins, min(n_bins, 5), replace=False)] = 1000
    wide = np.where(rng.random(n_bins) < 0.5, 1, 0).astype(np.int64)            # counts above 2^32 next to counts of 1
    wide[rng.choice(n_bins, min(n_bins, 6), replace=False)] = big + rng.integers(0, 3, min(n_bins, 6))
    spread = rng.integers(0, 1 << 20, n_bins).astype(np.int64) * rng.integers(0, 2, n_bins)
    ones = np.ones((n_bins,), np.int64)
    top = zero.copy()
    top[-1] = np.iinfo(np.int64).max                                            # the largest int64 in the last bin
    return np.stack([zero, few, ties, wide, spread, ones, top])


@pytest.mark.parametrize("n_bins", [1, 255, 257, 100003])
def test_facet_select_on_synthesised_bins(gpu, n_bins):
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    bins = _synth(n_bins, np.random.default_rng(n_bins))
    dev = torch.from_numpy(bins).cuda()
    lists = {}
    for k in (1, 10, 1024):
        codes, counts, info = (t.cpu().numpy() for t in ffi.facet_select(dev, k))
        wc, wn, wi = fc.facet_list(bins, k)
        assert np.array_equal(info, wi), f"k {k}: info {info.tolist()} vs {wi.tolist()}"
        assert np.array_equal(counts, wn), f"k {k}: counts differ in lists {np.flatnonzero((counts != wn).any(1)).tolist()}"
        assert np.array_equal(codes, wc), f"k {k}: codes differ in lists {np.flatnonzero((codes != wc).any(1)).tolist()}"
        assert ((codes == -1) == (counts == 0)).all()
        lists[k] = (codes, counts)
    for j, k in ((1, 10), (10, 1024)):                                          # the first j entries of a k-entry list are the j-entry list
        assert np.array_equal(lists[k][0][:, :j], lists[j][0]) and np.array_equal(lists[k][1][:, :j], lists[j][1])
    one = ffi.facet_select(dev[2], 10)                                          # a single histogram, without the leading axis
    assert np.array_equal(one[0].cpu().numpy(), lists[10][0][2:3])


@pytest.fixture(scope="module")
def ranged():
    """One 6 000-row corpus with its facet columns, tombstones and oracle scores for 65 queries on both stored precisions
    (read only): column 2 holds file-like runs (-1 sprinkled in), column 3 ten values of which a histogram of 6 bins leaves
    four out of range."""
    n, nq = 6000, 65
    raw, codes, block = range_cases.corpus(n, DIM, seed=11)
    codes = np.concatenate([codes, fc.codes_for("files", n, 1)[:, None], fc.codes_for("random10", n, 2)[:, None]], 1).astype(np.int32)
    dead = np.unique(np.concatenate([np.arange(5, n, 11), block[0] + np.asarray([0, 7, block[1] - 1])])).astype(np.int64)
    alive = np.ones((n,), bool)
    alive[dead] = False
    out = {"raw": raw, "codes": codes, "dead": dead, "alive": alive, "n": n, "nq": nq}
    for bf16 in (True, False):
        q, thr, scores, _, want = range_cases.batch(raw, block, nq, 10, bf16, alive, seed=3)
        out[bf16] = {"q": q, "thr": thr, "scores": scores, "counts": want[2]}
    return out


@pytest.mark.parametrize("bf16", [True, False])
def test_range_facet_equals_the_restatement(gpu, ranged, bf16):
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from tests import span_cases
    c, codes, alive = ranged[bf16], ranged["codes"], ranged["alive"]
    idx = _index(ffi, ranged["raw"], codes, ffi.DTYPE_BF16 if bf16 else ffi.DTYPE_F32, ranged["dead"])
    files = int(codes[:, 2].max()) + 1
    try:
        for filt in (None, [(0, [1, 3, 4]), (1, [2], True)]):
            passing = span_cases.np_mask(codes, alive, filt)
            for nq in (1, 16, 65):                                              # 65: two batches
                q, thr = c["q"][:nq], c["thr"][:nq]
                counts = idx.search_range(q, 1, thr, filters=filt)[2]
                for col, n_bins in ((2, files), (3, 6)):
                    bins, info = _host(idx.search_range_facet(q, thr, col, n_bins, filters=filt))
                    wb, wi = fc.histograms(codes[:, col], c["scores"][:nq], thr, passing, n_bins)
                    what = f"filter {filt} nq {nq} col {col}"
                    assert np.array_equal(info, wi), f"{what}: info differs for queries {np.flatnonzero((info != wi).any(1)).tolist()}"
                    assert np.array_equal(bins, wb), f"{what}: bins differ for queries {np.flatnonzero((bins != wb).any(1)).tolist()}"
                    assert np.array_equal(bins.sum(1) + info[:, 1] + info[:, 2], counts) and np.array_equal(info[:, 0], counts), what
                    if filt is None and nq == 65:
                        assert np.array_equal(counts, c["counts"]) and (info[:, 1] > 0).any() and (info[:, 2] > 0).any() == (col == 3)
        # candidate buffers too small for the batch: it overflows, is run again and gives what the roomy run gave
        roomy = _host(idx.search_range_facet(c["q"], c["thr"], 2, files))
        idx.set_tuning(force_fallback=1)
        again = _host(idx.search_range_facet(c["q"], c["thr"], 2, files))
        assert idx.stats()["fallback_used"] & 1
        idx.set_tuning(force_fallback=0)
        assert np.array_equal(again[0], roomy[0]) and np.array_equal(again[1], roomy[1])
        # a filter sparse enough for the tile list, and one that matches nothing
        rare = np.zeros((ranged["n"],), bool)
        rare[2000:2040] = True
        few = alive & rare
        w = np.zeros(((ranged["n"] + 31) // 32) * 32, np.uint8)
        w[: ranged["n"]] = rare
        import torch
        words = torch.from_numpy(np.packbits(w, bitorder="little").view(np.int32).copy()).cuda()
        thr = np.where(np.arange(ranged["nq"]) % 2 == 0, np.float32(-2.0), c["thr"]).astype(np.float32)
        bins, info = _host(idx.search_range_facet(c["q"], thr, 2, files, filters=[ffi.RowWords(ffi.next_words_tag(), words)]))
        wb, wi = fc.histograms(codes[:, 2], c["scores"], thr, few, files)
        assert np.array_equal(bins, wb) and np.array_equal(info, wi) and info[0, 0] == few.sum()
        bins, info = _host(idx.search_range_facet(c["q"], thr, 2, files, filters=[(0, 12345)]))
        assert not bins.any() and not info.any()
    finally:
        idx.close()


@pytest.fixture(scope="module")
def fake_script():
    """The store script of tests/facet_cases.py on the CPU tier's store over fake indexes, once (read only)."""
    from oracle import search as orc
    from tests.fake_index import fake_device
    with pytest.MonkeyPatch.context() as mp:
        fake_device(mp, fc.FacetFakeIndex, Text=fc.FakeText, facet_select=fc.np_facet_select)
        from coderag_amd.store import HipVectorStore
        return asyncio.run(fc.store_script(lambda: HipVectorStore(dim=fc.SCRIPT_DIM, dtype="f32", initial_capacity=256, device=0, compact_dead_fraction=0.0,
                                                                   shards=2, _merge_fn=orc.merge_topk), None))


@pytest.mark.parametrize("shards", [1, 3])
def test_store_equals_the_store_over_fake_indexes(gpu, fake_script, tmp_path, shards):
    import coderag_amd  # noqa: F401
    from coderag_amd.store import HipVectorStore
    got = asyncio.run(fc.store_script(lambda: HipVectorStore(dim=fc.SCRIPT_DIM, dtype="f32", initial_capacity=256, device=0, shards=shards,
                                                             compact_dead_fraction=0.0), fc.FacetModel(), str(tmp_path)))
    assert len(fake_script) == 3 * 14 and len(got) == 4 * 14
    for name, want in fake_script.items():
        assert got[name] == want, f"{name}: {got[name]} vs {want}"
    assert got["compacted: files holding TODO("]["total"] > 0 and got["loaded: batch"] == got["compacted: batch"]
