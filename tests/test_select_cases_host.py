"""The key sets of tests/select_cases.py are what they claim, their references are what they claim, and they are SHARP: a model
of wg_kth_largest_fast (crh_kernels.hpp) that carries one plausible slip at a time gives, for every slip, a wrong answer on at
least one named case.  CPU tier -- nothing here touches a GPU; tests/test_select_gpu.py runs the same cases on the kernels.

The slips (``DEFECTS``), each a one-token change of the helper:

  no_clamp            ``b < NB ? b : NB - 1`` left out: once hi - lo >= 2^24 the bucket of hi is NB and its count is lost
  cap_ge              ``pop >= CAP`` instead of ``>``.  The radix passes are exact too, so this one changes no ANSWER -- only which
                      branch gives it; it counts as caught when the model leaves the branch a case was built (and asserted, by
                      bucket_model) to take.  On the device the two branches are pinned from both sides by pop = CAP and CAP + 1.
  floor_ge_range      ``key >= floor_key`` in the range pass alone: lo becomes the floor key, n_above counts the floor keys
  floor_ge_hist       ``key >= floor_key`` in the histogram and collection passes alone: floor keys are filed (below lo)
  k_ge_n_above        ``k >= n_above`` instead of ``>``: the smallest key above the floor is never returned
  rem_from_bottom     the rank inside the bucket counted from its smallest key
  drop_partial_block  a for_each_key that handles whole 8 * NT blocks only

``>=`` at ALL THREE comparisons with the floor at once is not among them because it is no defect: the keys equal to the floor
then take part as ordinary keys, the bucketing stays exact, and the answer is the floor key exactly when it was before
(test_floor_comparison_at_every_site_is_answer_preserving holds the model to that on every case).
"""
import numpy as np
import pytest

from tests import select_cases as sc

F32, U32, U64 = np.float32, np.uint32, np.uint64
DEFECTS = ("no_clamp", "cap_ge", "floor_ge_range", "floor_ge_hist", "k_ge_n_above", "rem_from_bottom", "drop_partial_block")
# the family that is BUILT to catch each slip (others may catch it as well)
BUILT_FOR = {"no_clamp": "span", "cap_ge": "ties", "floor_ge_range": "floor", "floor_ge_hist": "floor", "k_ge_n_above": "floor",
             "rem_from_bottom": "crowded", "drop_partial_block": "sizes"}

_CASES = {}


def cases(variant):
    if variant not in _CASES:
        _CASES[variant] = sc.kth_cases(*variant)
    return _CASES[variant]


def fast_model(keys, k, floor, NT, NB, CAP, defect=None):
    """(key, branch) of wg_kth_largest_fast<NT, NB, CAP>, step by step, with at most one slip."""
    keys = np.asarray(keys, U32)
    n = keys.size
    seen = keys[: n // (8 * NT) * (8 * NT)] if defect == "drop_partial_block" else keys       # what for_each_key visits

    def above(ge):
        return seen >= U32(floor) if ge else seen > U32(floor)

    # 1. range and count
    a1 = above(defect in ("floor_ge_range", "floor_ge_all"))
    lo = int(seen[a1].min()) if a1.any() else 0xffffffff
    hi = int(seen[a1].max()) if a1.any() else 0
    n_above = n - int((~a1).sum())
    if k > n_above or (defect == "k_ge_n_above" and k == n_above):
        return floor, "floor"
    if lo == hi:
        return lo, "flat"
    scale = F32(NB) / (F32(U32((hi - lo) & 0xffffffff)) + F32(1.0))
    # 2. histogram (the keys the second comparison lets through; a key below lo wraps around)
    filed = seen[above(defect in ("floor_ge_hist", "floor_ge_all"))]
    prod = ((filed.astype(np.int64) - lo) & 0xffffffff).astype(U32).astype(F32) * scale
    raw = np.minimum(np.floor(prod.astype(np.float64)), 2.0 ** 32 - 1).astype(np.int64)         # (the conversion saturates)
    if defect == "no_clamp":
        filed, raw = filed[raw < NB], raw[raw < NB]                                           # (the count lands outside the histogram)
    bucket = np.minimum(raw, NB - 1)
    hist = np.bincount(bucket, minlength=NB)
    # 3. the bucket of the k-th
    before, found = 0, None
    for b in range(NB - 1, -1, -1):
        if before < k <= before + hist[b]:
            found = (b, k - before, int(hist[b]))
            break
        before += int(hist[b])
    if found is None:
        return 0, "lost"                                                                      # (ctl[] still holds its zeros)
    bsel, rem, pop = found
    if pop > CAP or (defect == "cap_ge" and pop == CAP):
        return sc.ref_kth(keys, k), "radix"                                                   # (wg_kth_largest walks the keys itself)
    # 4. rank inside the bucket
    members = np.sort(filed[bucket == bsel])
    return int(members[rem - 1] if defect == "rem_from_bottom" else members[::-1][rem - 1]), "fast"


# ------------------------------------------------------------------ the maps

def test_key_maps_agree_with_the_other_restatement_and_with_float_order():
    from tests import fuse_cases as fc
    r = np.random.default_rng(1)
    x = np.r_[r.standard_normal(2000).astype(F32), r.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(U32).view(F32),
              np.asarray([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 3.4e38, -3.4e38], F32)]
    x = x[~np.isnan(x)]
    o = sc.ord_f32(x)
    assert np.array_equal(o, fc.ord_f32(x)) and np.array_equal(sc.unord_f32(o).view(U32), x.view(U32))
    assert np.array_equal(sc.unord_f32(o).view(U32), fc.unord_f32(o).view(U32))
    order = np.argsort(o, kind="stable")
    assert np.all(np.diff(x[order].astype(np.float64)) >= 0)                                  # larger key <=> larger float
    assert int(sc.ord_f32(F32(-0.0))) + 1 == int(sc.ord_f32(F32(0.0))) == 0x80000000
    assert int(sc.ord_f32(F32(-np.inf))) == sc.ORD_NEG_INF == sc.I8_FLOOR == (sc.ORD_NEG_INF | 31)
    assert sc.FLOORS == (0, 0x007fffff, 0x007fffff)
    keys = sc.score_key(np.asarray([0.5, np.nan, -np.inf, 0.5], F32), np.asarray([7, 7, 0xfffffffe, 0]))
    assert [int(v) for v in keys] == [(0xbf000000 << 32) | 0xfffffff8, sc.NO_KEY, (0x007fffff << 32) | 1, (0xbf000000 << 32) | 0xffffffff]
    assert keys[3] > keys[0] > keys[2] > keys[1]                                              # score, then the LOWER row; kNoKey below all


# ------------------------------------------------------------------ k-th key

@pytest.mark.parametrize("variant", sc.FAST_VARIANTS, ids=lambda v: f"NT{v[0]}")
def test_kth_cases_cover_what_they_are_listed_for(variant):
    NT, NB, CAP = variant
    cs = cases(variant)
    assert len({c.name for c in cs}) == len(cs)
    by = {}
    for c in cs:
        by.setdefault(c.family, []).append(c)
    assert set(by) == {"sizes", "floor", "flat", "span", "ties", "crowded", "float"}
    assert {c.n for c in by["sizes"]} == {1, 2, NT - 1, NT, NT + 1, 8 * NT - 1, 8 * NT, 8 * NT + 1, 70001}
    assert any(c.k == 1 for c in by["sizes"]) and any(c.k == c.n > 1 for c in by["sizes"])
    assert {c.floor for c in cs} == set(sc.FLOORS)
    # the floor family: nothing above, k on either side of n_above, keys equal to floor + 1, payload keys under the int8 floor
    fl = by["floor"]
    n_above = lambda c: int((c.keys > c.floor).sum())
    assert any(n_above(c) == 0 for c in fl) and any(c.k == n_above(c) > 1 for c in fl) and any(c.k == n_above(c) + 1 for c in fl)
    assert any(sc.ref_kth_fast(c.keys, c.k, c.floor) == c.floor + 1 for c in fl)
    assert any(c.floor == sc.I8_FLOOR and (c.keys & 31).any() and (c.keys == c.floor).any() and ((c.keys < c.floor) & (c.keys > c.floor - 32)).any() for c in fl)
    assert all(c.path in ("flat", "floor") for c in by["flat"]) and any((c.keys <= c.floor).any() for c in by["flat"])
    # spans: every listed width, hi = 0xffffffff among them, and the answer at hi, at lo and between
    spans = {c.note["span"] for c in by["span"]}
    assert {1, NB - 1, NB, 2 ** 24 - 1, 2 ** 24 + 1, 0xffffffff - 1, 0xffffffff - 0x00800000} <= spans
    assert any(int(c.keys.max()) == 0xffffffff for c in by["span"])
    for c in by["span"]:
        bm = sc.bucket_model(c.keys, c.floor, NB)
        assert bm.hi - bm.lo == c.note["span"] and (int(bm.raw.max()) == NB) == (c.note["span"] >= 2 ** 24)
    for what in ("hi", "lo", "middle"):
        assert any(c.name.endswith("answer=" + what) for c in by["span"])
    # tie runs: the selected bucket holds exactly m keys, and the branch follows
    pops = {}
    for c in by["ties"] + by["crowded"]:
        if "pop" in c.note:
            b, rem, pop = sc.bucket_model(c.keys, c.floor, NB).select(c.k)
            assert pop == c.note["pop"] and c.path == ("fast" if pop <= CAP else "radix")
            pops.setdefault(c.family, set()).add((pop, "first" if rem == 1 else "last" if rem == pop else "inside"))
    assert {(m, e) for m in (CAP - 1, CAP, CAP + 1) for e in ("first", "last")} | {(1, "first")} <= pops["ties"]
    assert {p for p, _ in pops["crowded"]} >= {CAP, CAP + 1} and any(e == "inside" for _, e in pops["crowded"])
    for c in by["crowded"]:
        if "pop" in c.note:
            bm = sc.bucket_model(c.keys, c.floor, NB)
            members = bm.keys[bm.bucket() == bm.select(c.k)[0]]
            assert np.unique(members).size == members.size == c.note["pop"]                 # crowded WITHOUT ties
    assert {c.path for c in cs} == {"fast", "radix", "flat", "floor"}


@pytest.mark.parametrize("variant", sc.FAST_VARIANTS, ids=lambda v: f"NT{v[0]}")
def test_kth_references_by_counting_and_the_sound_model_agrees(variant):
    """The reference is a sort; independently, v is the k-th largest iff fewer than k keys exceed it and at least k reach it.  The
    model without a slip returns the reference on every case, by the branch bucket_model predicts."""
    for c in cases(variant):
        for keys, want in ((c.keys, sc.ref_kth(c.keys, c.k)), (np.maximum(c.keys, U32(c.floor)), sc.ref_kth_fast(c.keys, c.k, c.floor))):
            assert int((keys > want).sum()) < c.k <= int((keys >= want).sum()), c.name
        assert sc.ref_kth_fast(c.keys, c.k, c.floor) == max(sc.ref_kth(c.keys, c.k), c.floor)
        assert fast_model(c.keys, c.k, c.floor, *variant) == (sc.ref_kth_fast(c.keys, c.k, c.floor), c.path), c.name


@pytest.mark.parametrize("variant", sc.FAST_VARIANTS, ids=lambda v: f"NT{v[0]}")
@pytest.mark.parametrize("defect", DEFECTS)
def test_every_slip_is_caught_by_a_named_case(defect, variant):
    caught = []
    for c in cases(variant):
        key, path = fast_model(c.keys, c.k, c.floor, *variant, defect=defect)
        wrong = key != sc.ref_kth_fast(c.keys, c.k, c.floor)
        if wrong or (defect == "cap_ge" and path != c.path):
            caught.append(c.name)
    print(f"{defect} NT={variant[0]}: {len(caught)} cases, e.g. {caught[:3]}")
    assert any(name.startswith(BUILT_FOR[defect] + "/") for name in caught), f"no {BUILT_FOR[defect]} case catches {defect}: {caught[:5]}"


@pytest.mark.parametrize("variant", sc.FAST_VARIANTS, ids=lambda v: f"NT{v[0]}")
def test_floor_comparison_at_every_site_is_answer_preserving(variant):
    for c in cases(variant):
        assert fast_model(c.keys, c.k, c.floor, *variant, defect="floor_ge_all")[0] == sc.ref_kth_fast(c.keys, c.k, c.floor), c.name


def test_u64_cases():
    cs = sc.kth64_cases()
    assert len({c.name for c in cs}) == len(cs)
    assert {c.n for c in cs} >= {1, 2, 2047, 2049, 5000} and min(c.n for c in cs) < 2048 < max(c.n for c in cs)
    for c in cs:
        assert c.keys.dtype == U64 and 1 <= c.k <= c.n
        want = sc.ref_kth(c.keys, c.k)
        assert int((c.keys > U64(want)).sum()) < c.k <= int((c.keys >= U64(want)).sum()), c.name
        high = (c.keys >> U64(32)).astype(U32)
        if "high-words-equal" in c.name:
            assert np.unique(high).size == 1
        if "top-byte" in c.name and c.n > 2:
            assert np.unique(high & U32(0x00ffffff)).size == 1 and np.unique(high >> U32(24)).size > 1
        if "bottom-byte" in c.name and c.n > 2:
            assert np.unique(high >> U32(8)).size == 1 and np.unique(high & U32(0xff)).size > 1
    for n in (300, 5000):
        assert {c.k for c in cs if c.n == n and "high-words-equal" in c.name} == {1, 2, n // 2, n - 1, n}
    assert any((c.keys == sc.NO_KEY).any() and sc.ref_kth(c.keys, c.k) == sc.NO_KEY for c in cs)


# ------------------------------------------------------------------ select_tail

def _slow_tail(keys, k, row_base):
    """Independent of ref_select_tail's sort: the place of a key is the number of keys that go before it."""
    keys = np.asarray(keys, U64)
    real = keys != U64(sc.NO_KEY)
    scores, rows = np.full((k,), -np.inf, F32), np.full((k,), -1, np.int64)
    for i in np.flatnonzero(real):
        place = int((keys > keys[i]).sum())
        if place < k:
            scores[place] = sc.unord_f32(U32(int(keys[i]) >> 32))
            rows[place] = row_base + (0xffffffff - (int(keys[i]) & 0xffffffff))
    return scores, rows


def test_tail_cases_and_their_reference():
    cs = sc.tail_cases()
    assert len({c.name for c in cs}) == len(cs)
    assert {c.keys.size for c in cs} >= {1, 2, 2047, 2048, 2049, 5000} and {c.k for c in cs} >= {1, 2, 3, 100, 1023, 1024}
    assert {c.row_base for c in cs} == {0, 3 << 32} and {c.in_lds for c in cs} == {True, False}
    assert any(c.k > c.keys.size for c in cs) and any(not c.in_lds and c.k & (c.k - 1) for c in cs)
    for lds in (True, False):       # 0, 1 and many kNoKey entries, and fewer real keys than k, on both paths
        sub = [c for c in cs if c.in_lds == lds]
        assert {min(int((c.keys == sc.NO_KEY).sum()), 2) for c in sub} == {0, 1, 2}
        assert any(0 < int((c.keys != sc.NO_KEY).sum()) < min(c.k, c.keys.size) for c in sub)
    assert any(int((~c.keys & U64(0xffffffff)).max()) == 0xfffffffe for c in cs)
    for c in cs:
        real = c.keys[c.keys != sc.NO_KEY]
        assert np.unique(real).size == real.size and 1 <= c.k <= sc.MAX_K
        s, r = sc.ref_select_tail(c.keys, c.k, c.row_base)
        if c.keys.size <= 2049:
            s2, r2 = _slow_tail(c.keys, c.k, c.row_base)
            assert np.array_equal(s.view(U32), s2.view(U32)) and np.array_equal(r, r2), c.name
        m = min(c.k, real.size)
        assert np.all(r[:m] >= c.row_base) and np.all(r[m:] == -1) and np.all(np.isneginf(s[m:]))
        assert np.all(np.diff(sc.ord_f32(s[:m]).astype(np.int64)) <= 0)
        ties = np.flatnonzero(np.diff(sc.ord_f32(s[:m]).astype(np.int64)) == 0)
        assert np.all(r[ties] < r[ties + 1])                                                   # equal scores: ascending row


# ------------------------------------------------------------------ tile list

def test_tile_masks_and_their_reference():
    assert set(sc.TILE_SIZES) == {1, 255, 256, 257, 65536, 65537, 65793, 70001, 140000, 312500}
    assert (65793 + 255) // 256 == 258 and (65792 + 255) // 256 == 257          # workgroup 257: the prefix loop's second iteration
    seen = set()
    for ntiles, kind in sc.tile_cases():
        w = sc.tile_mask(ntiles, kind)
        assert w.dtype == U32 and w.shape == (ntiles,)
        ref = sc.ref_tile_list(w)
        if ntiles <= 257:
            assert list(ref) == [t for t in range(ntiles) if int(w[t]) != 0]
        assert ref.size == np.count_nonzero(w) and np.all(np.diff(ref.astype(np.int64)) > 0)
        frac = ref.size / ntiles
        if kind == "zero":
            assert ref.size == 0
        elif kind == "all":
            assert ref.size == ntiles
        elif kind == "first-word":
            assert list(ref) == [0]
        elif kind == "last-word":
            assert list(ref) == [ntiles - 1]
        elif kind == "last-workgroup":
            assert ref[0] == (ntiles - 1) // 256 * 256 and ref.size == ntiles - int(ref[0])
        elif kind.startswith("words="):
            assert set(np.unique(w)) <= {0, int(kind[6:], 0)} and ref.size
        elif kind.startswith("random") and ntiles >= 65536:
            assert abs(frac - float(kind[7:-1]) / 100) < 0.01
        seen.add(kind)
    assert seen == set(sc.TILE_MASKS)
