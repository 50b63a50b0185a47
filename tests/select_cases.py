"""Key sets for the workgroup-wide selection helpers (code-rag_amd/csrc/crh_kernels.hpp: wg_kth_largest_fast, wg_kth_largest,
wg_bitonic_desc, select_tail) and for the tile list of a row mask (k_tilelist_count / k_tilelist_fill), with their references.
Test infrastructure only, importable without a GPU; tests/test_select_cases_host.py checks the builders, tests/test_select_gpu.py
runs them through crh_debug_kth_largest / crh_debug_select_tail / crh_debug_tile_list.

The keys are integers, so every reference is a sort and no tolerance appears anywhere:

  k-th key     np.sort(keys)[::-1][k - 1]; for wg_kth_largest_fast with the keys at or below the floor raised to the floor first
               (the helper returns the floor key when the k-th largest is one of them: they all mean "no valid row");
  select_tail  a plain Python ranking: descending key, kNoKey entries last in list order, decoded as score_key encodes;
  tile list    np.flatnonzero(mask).

``bucket_model`` restates the bucket function of wg_kth_largest_fast in numpy f32.  It is used ONLY to assert what a case claims
about itself ("the selected bucket holds exactly CAP keys", "the unclamped bucket of hi is NB") and to record which branch a case
takes for the coverage table; it never judges the kernel.
"""
from dataclasses import dataclass, field

import numpy as np

F32, U32, U64 = np.float32, np.uint32, np.uint64

NO_KEY = 0                                   # kNoKey
ORD_NEG_INF = 0x007fffff                     # ord_f32(-inf): the floor of k_tau / k_scan_fused
I8_FLOOR = 0x007fffff                        # kFloorKey of k_scan_i8: ord(-inf) | 31 (keys carry a row in their low five bits)
FLOORS = (0, ORD_NEG_INF, I8_FLOOR)          # what the product passes (two of them are the same number)
FAST_VARIANTS = ((1024, 1024, 256), (512, 512, 256), (256, 256, 256))      # (NT, NB, CAP) of wg_kth_largest_fast
RADIX_U32_NT = (1024, 512, 256)
RADIX_U64_NT = (1024, 256)
TAIL_NT = (1024, 256)
LCAP = 2048                                  # kSelectLdsKeys
MAX_K = 1024                                 # CRH_MAX_K
TILE_SENTINEL = 0xa5a5a5a5


# ------------------------------------------------------------------ the key maps

def ord_f32(x) -> np.ndarray:
    """ord_f32 of crh_kernels.hpp: larger float <=> larger uint32 (-0.0 < +0.0)."""
    a = np.asarray(x, dtype=F32)
    u = a.reshape(-1).view(U32).reshape(a.shape)
    return np.where(u & U32(0x80000000), ~u, u | U32(0x80000000)).astype(U32)


def unord_f32(o) -> np.ndarray:
    o = np.asarray(o, dtype=U32)
    return np.where(o & U32(0x80000000), o & U32(0x7fffffff), ~o).astype(U32).reshape(-1).view(F32).reshape(o.shape)


def score_key(score, row) -> np.ndarray:
    """score_key: (ord(score) << 32) | ~row, and kNoKey for a NaN score."""
    s = np.asarray(score, dtype=F32)
    r = np.asarray(row, dtype=np.int64)
    key = (ord_f32(s).astype(U64) << U64(32)) | ((~r) & 0xffffffff).astype(U64)
    return np.where(np.isnan(s), U64(NO_KEY), key).astype(U64)


# ------------------------------------------------------------------ references

def ref_kth(keys, k: int) -> int:
    """The k-th largest key (1-based): a sort."""
    return int(np.sort(np.asarray(keys))[::-1][k - 1])


def ref_kth_fast(keys, k: int, floor: int) -> int:
    """What wg_kth_largest_fast owes its callers: the k-th largest key, or the floor key when that is at or below the floor."""
    return int(np.sort(np.maximum(np.asarray(keys, U32), U32(floor)))[::-1][k - 1])


def ref_select_tail(keys, k: int, row_base: int):
    """(scores f32 [k], rows i64 [k]): descending key, kNoKey entries behind every real key in list order (they come out as
    padding), the tail of a short list (-inf, -1)."""
    keys = [int(v) for v in np.asarray(keys, U64)]
    order = sorted(range(len(keys)), key=lambda i: (keys[i] == NO_KEY, -keys[i], i))
    scores, rows = np.full((k,), -np.inf, F32), np.full((k,), -1, np.int64)
    for place, i in enumerate(order[:k]):
        if keys[i] != NO_KEY:
            scores[place] = unord_f32(U32(keys[i] >> 32))
            rows[place] = row_base + ((~keys[i]) & 0xffffffff)
    return scores, rows


def ref_tile_list(words) -> np.ndarray:
    return np.flatnonzero(np.asarray(words, U32)).astype(U32)


# ------------------------------------------------------------------ the bucket function, restated (preconditions only)

@dataclass
class Buckets:
    n_above: int
    lo: int = 0
    hi: int = 0
    raw: np.ndarray = None          # unclamped bucket of every key above the floor (int64)
    keys: np.ndarray = None         # those keys
    NB: int = 0

    def bucket(self) -> np.ndarray:
        return np.minimum(self.raw, self.NB - 1)

    def select(self, k: int):
        """(bucket, rank inside it from the top, population) of the k-th largest key above the floor."""
        hist = np.bincount(self.bucket(), minlength=self.NB)
        above = 0
        for b in range(self.NB - 1, -1, -1):
            if above < k <= above + hist[b]:
                return b, k - above, int(hist[b])
            above += int(hist[b])
        raise AssertionError("k is larger than the number of keys above the floor")


def bucket_model(keys, floor: int, NB: int, scale_ulps: int = 0) -> Buckets:
    """lo / hi of the keys above ``floor`` and ``(unsigned)((float)(key - lo) * scale)`` with ``scale = (float)NB / ((float)(hi - lo)
    + 1.0f)``, every step rounded to f32 as the kernel's are.  ``scale_ulps`` moves the scale that many f32 steps: a precondition
    that holds for -1, 0 and +1 does not hang on how the device rounds one division."""
    keys = np.asarray(keys, U32)
    above = keys[keys > U32(floor)]
    if above.size == 0:
        return Buckets(0, NB=NB)
    lo, hi = int(above.min()), int(above.max())
    scale = F32(NB) / (F32(U32(hi - lo)) + F32(1.0))
    for _ in range(abs(scale_ulps)):
        scale = np.nextafter(scale, F32(np.inf if scale_ulps > 0 else 0.0), dtype=F32)
    prod = (above - U32(lo)).astype(F32) * scale
    assert prod.dtype == F32
    return Buckets(int(above.size), lo, hi, np.floor(prod).astype(np.int64), above, NB)


def predicted_path(keys, k: int, floor: int, NB: int, CAP: int) -> str:
    """Which branch of wg_kth_largest_fast answers: "floor" (k > n_above), "flat" (lo == hi), "fast" or "radix" (pop > CAP)."""
    bm = bucket_model(keys, floor, NB)
    if k > bm.n_above:
        return "floor"
    if bm.lo == bm.hi:
        return "flat"
    return "radix" if bm.select(k)[2] > CAP else "fast"


# ------------------------------------------------------------------ k-th key: u32 cases for one fast variant

@dataclass
class KthCase:
    name: str
    family: str
    keys: np.ndarray                 # uint32 [n]
    k: int
    floor: int
    path: str = ""                   # predicted_path for the variant the case was built for
    note: dict = field(default_factory=dict)

    @property
    def n(self) -> int:
        return int(self.keys.size)


def _shuffled(parts, seed: int) -> np.ndarray:
    keys = np.concatenate([np.asarray(p, U32).reshape(-1) for p in parts]).astype(U32)
    np.random.default_rng(seed).shuffle(keys)
    return keys


def _gauss_keys(n: int, seed: int) -> np.ndarray:
    """ord of Gaussian scores of unit vectors in 768 dimensions: the band the end-to-end tests feed the helpers."""
    return ord_f32((np.random.default_rng(seed).standard_normal(n) / np.sqrt(768.0)).astype(F32))


def kth_cases(NT: int, NB: int, CAP: int) -> list:
    """Every family of u32 key sets for wg_kth_largest_fast<NT, NB, CAP>; the same sets go through wg_kth_largest<u32, NT>."""
    out = []

    def add(name, family, keys, k, floor, want_path=None, **note):
        keys = np.ascontiguousarray(keys, dtype=U32)
        assert keys.ndim == 1 and 1 <= k <= keys.size, name
        path = predicted_path(keys, k, floor, NB, CAP)
        assert want_path is None or path == want_path, f"{name}: takes the {path} branch, built for {want_path}"
        out.append(KthCase(f"{family}/{name}", family, keys, int(k), int(floor), path, note))

    # ---- sizes: the edges of for_each_key's eight-deep sweep; the extreme keys sit in the LAST positions
    for n in (1, 2, NT - 1, NT, NT + 1, 8 * NT - 1, 8 * NT, 8 * NT + 1, 70001):
        keys = _gauss_keys(n, 100 + n)
        order = np.argsort(keys, kind="stable")
        top_last, low_last = keys.copy(), keys.copy()
        top_last[[order[-1], n - 1]] = top_last[[n - 1, order[-1]]]          # the largest key at index n - 1
        low_last[[order[0], n - 1]] = low_last[[n - 1, order[0]]]            # the smallest key at index n - 1
        add(f"n={n},k=1,largest-last", "sizes", top_last, 1, 0)
        add(f"n={n},k=n,smallest-last", "sizes", low_last, n, 0)
        if n > 2:
            add(f"n={n},k=mid", "sizes", keys, (n + 1) // 2, 0)
            add(f"n={n},k=min(100,n-1)", "sizes", low_last, min(100, n - 1), ORD_NEG_INF)

    # ---- floor
    n = 3 * NT + 5
    r = np.random.default_rng(7)
    add("floor=0,all-keys-0", "floor", np.zeros(n, U32), 5, 0, "floor")
    add("floor=ord(-inf),all-at-or-below", "floor", r.integers(0, ORD_NEG_INF + 1, n), 1, ORD_NEG_INF, "floor")
    add("floor=ord(-inf),all-at-or-below,k=n", "floor", np.r_[r.integers(0, ORD_NEG_INF + 1, n - 1), ORD_NEG_INF], n, ORD_NEG_INF, "floor")
    for floor in (0, ORD_NEG_INF):
        below = np.full(n - 37, floor, U32)
        below[::3] = 0
        above = _gauss_keys(37, 11)
        keys = _shuffled([below, above], 12)
        add(f"floor={floor:#x},k=n_above", "floor", keys, 37, floor, "fast")
        add(f"floor={floor:#x},k=n_above+1", "floor", keys, 38, floor, "floor")
        add(f"floor={floor:#x},k=n", "floor", keys, n, floor, "floor")
        add(f"floor={floor:#x},one-above,k=1", "floor", _shuffled([below, above[:1]], 13), 1, floor, "flat")
        add(f"floor={floor:#x},one-above,k=2", "floor", _shuffled([below, above[:1]], 13), 2, floor, "floor")
        # keys equal to floor + 1: the smallest key that counts
        keys = _shuffled([below[:-20], np.full(20, floor + 1, U32), above], 14)
        add(f"floor={floor:#x},floor+1,k=last-of-them", "floor", keys, 57, floor)
        add(f"floor={floor:#x},floor+1,k=first-of-them", "floor", keys, 38, floor)
        add(f"floor={floor:#x},floor+1,k=past-them", "floor", keys, 58, floor, "floor")
        add(f"floor={floor:#x},only-floor+1-above", "floor", _shuffled([below, np.full(37, floor + 1, U32)], 15), 37, floor, "flat")
    # k_scan_i8's keys: (ord(lower end) & ~31) | row inside the tile; a tile without a valid row has (ord(-inf) & ~31) | row <= floor
    for dens, tag in ((0.0, "none"), (0.3, "some"), (0.97, "most")):
        ends = (r.standard_normal(n) / np.sqrt(768.0) - 0.02).astype(F32)
        ends[r.random(n) < dens] = -np.inf
        keys = (ord_f32(ends) & U32(~np.uint32(31))) | r.integers(0, 32, n).astype(U32)
        if dens:
            keys[np.flatnonzero(np.isinf(ends))[0]] = I8_FLOOR          # ord(-inf) | 31: the largest key that is no row's
        n_above = int((keys > I8_FLOOR).sum())
        for k in sorted({1, min(10, n_above), min(100, n_above), n_above, min(n_above + 1, n)} - {0}):
            add(f"i8-payload,-inf={tag},k={k}", "floor", keys, k, I8_FLOOR)
    # equal scores, different payloads: the k-th key is decided by the low five bits alone
    keys = (ord_f32(np.full(200, 0.125, F32)) & U32(~np.uint32(31))) | (np.arange(200) % 32).astype(U32)
    keys = _shuffled([keys, np.full(n - 200, I8_FLOOR - 5, U32)], 16)
    for k in (1, 7, 100, 200, 201):
        add(f"i8-payload,one-score,k={k}", "floor", keys, k, I8_FLOOR)

    # ---- flat: lo == hi
    for floor in (0, ORD_NEG_INF):
        v = int(ord_f32(F32(0.25)))
        add(f"floor={floor:#x},all-equal,k=1", "flat", np.full(n, v, U32), 1, floor, "flat")
        add(f"floor={floor:#x},all-equal,k=n", "flat", np.full(n, v, U32), n, floor, "flat")
        mixed = _shuffled([np.full(n - 500, v, U32), np.full(500, floor, U32)], 21)
        add(f"floor={floor:#x},equal+floor-keys,k=n_above", "flat", mixed, n - 500, floor, "flat")
        add(f"floor={floor:#x},equal+floor-keys,k=n_above+1", "flat", mixed, n - 499, floor, "floor")
        add(f"floor={floor:#x},equal-to-0xffffffff", "flat", _shuffled([np.full(300, 0xffffffff, U32), np.full(9, floor, U32)], 22), 300, floor, "flat")
    add("n=1", "flat", np.asarray([0x80000000], U32), 1, 0, "flat")

    # ---- span: hi - lo from 1 to the whole range; the answer is hi, lo and a key between
    for floor in (0, ORD_NEG_INF):
        whole = 0xffffffff - (floor + 1)
        for span in (1, NB - 1, NB, 2 ** 24 - 1, 2 ** 24 + 1, whole):
            for top in ("hi=0xffffffff", "low"):
                hi = 0xffffffff if top == "hi=0xffffffff" else floor + 1 + span
                lo = hi - span
                if top == "low" and span == whole:
                    continue                                  # (the same set as hi = 0xffffffff)
                inner = np.unique(np.random.default_rng(span % 9973).integers(lo, hi + 1, 150, dtype=np.uint64).astype(U32)) if span > 1 else np.asarray([], U32)
                inner = inner[(inner != lo) & (inner != hi)]
                keys = _shuffled([[lo, hi], inner, np.full(40, floor, U32)], 31)
                na = 2 + inner.size
                bm = bucket_model(keys, floor, NB)
                assert (bm.lo, bm.hi) == (lo, hi)
                if span >= 2 ** 24:
                    assert int(bm.raw.max()) == NB, f"span {span}: the unclamped bucket of hi is {int(bm.raw.max())}, not NB = {NB}"
                else:
                    assert int(bm.raw.max()) == NB - 1 or span < NB
                for k, what in ((1, "hi"), (na, "lo"), ((na + 1) // 2, "middle")):
                    add(f"floor={floor:#x},span={span},{top},answer={what}", "span", keys, k, floor, None, span=span)
                assert ref_kth_fast(keys, 1, floor) == hi and ref_kth_fast(keys, na, floor) == lo

    # ---- tie runs at the cut: m equal keys alone in their bucket, the k-th place on the first and on the last of them.  The band
    # is lo .. lo + NB * W - 1 with W a power of two, so the scale is exactly 1 / W and a key's bucket is (key - lo) / W in any
    # rounding; the rest of the band is sparse (one key in every 16th bucket).
    W = 4096
    lo = int(ord_f32(F32(0.05))) & ~(W - 1)
    hi = lo + NB * W - 1
    for m in (1, CAP - 1, CAP, CAP + 1):
        for b in (NB // 2 + 3, NB - 1, 0):
            sparse = [lo + ob * W + 17 for ob in range(5, NB, 16) if ob != b]
            run_key = lo + b * W + W // 2 if 0 < b < NB - 1 else (hi if b else lo)
            ends = [v for v in (lo, hi) if v != run_key]
            keys = _shuffled([sparse, ends, np.full(m, run_key, U32), np.full(30, ORD_NEG_INF, U32)], 41 + m)
            n_over = int((keys > run_key).sum())
            for scale_ulps in (-1, 0, 1):
                bm = bucket_model(keys, ORD_NEG_INF, NB, scale_ulps)
                assert bm.select(n_over + 1) == (b, 1, m) and bm.select(n_over + m) == (b, m, m), (m, b, scale_ulps)
            want = "fast" if m <= CAP else "radix"
            add(f"m={m},bucket={b},k=first-of-run", "ties", keys, n_over + 1, ORD_NEG_INF, want, pop=m)
            add(f"m={m},bucket={b},k=last-of-run", "ties", keys, n_over + m, ORD_NEG_INF, want, pop=m)
            if n_over:
                add(f"m={m},bucket={b},k=just-above-run", "ties", keys, n_over, ORD_NEG_INF, "fast")
            add(f"m={m},bucket={b},k=just-below-run", "ties", keys, n_over + m + 1, ORD_NEG_INF)
    add(f"m=n={2 * NT + 3}", "ties", np.full(2 * NT + 3, lo + 5, U32), NT, ORD_NEG_INF, "flat")
    # a run that shares its bucket: CAP keys in the bucket of which CAP - 2 are equal
    b = NB // 4
    keys = _shuffled([[lo, hi, lo + b * W + 1, lo + b * W + W - 1], np.full(CAP - 2, lo + b * W + 9, U32)], 47)
    for k in (2, 3, CAP - 1, CAP, CAP + 1, CAP + 2):
        add(f"shared-bucket,k={k}", "ties", keys, k, 0, "fast" if 2 <= k <= CAP + 1 else None)

    # ---- crowded bucket without ties: two far outliers make the range, everything else is packed into less than one bucket
    for count, want in ((CAP, "fast"), (CAP + 1, "radix"), (3 * CAP + 7, "radix"), (8 * NT + 1, "radix")):
        lo_c, hi_c = ORD_NEG_INF + 1, 0xfffffff0
        width = (hi_c - lo_c) // NB
        start = lo_c + (NB // 3) * width + width // 4
        assert count < width // 2
        crowd = start + np.random.default_rng(count).choice(width // 2, count, replace=False).astype(np.int64)
        keys = _shuffled([[lo_c, hi_c], crowd], 51)
        for scale_ulps in (-1, 0, 1):
            assert bucket_model(keys, ORD_NEG_INF, NB, scale_ulps).select(2)[2] == count
        for k, what in ((2, "top"), (1 + count, "bottom"), (1 + (count + 1) // 2, "middle"), (1 + min(100, count), "100th")):
            add(f"distinct={count},answer={what}-of-crowd", "crowded", keys, k, ORD_NEG_INF, want, pop=count)
        add(f"distinct={count},answer=hi", "crowded", keys, 1, ORD_NEG_INF, "fast")
        add(f"distinct={count},answer=lo", "crowded", keys, count + 2, ORD_NEG_INF, "fast")

    # ---- float-shaped keys
    r = np.random.default_rng(61)
    n = 4096 + 37
    binade = ord_f32((1.0 + r.random(n)).astype(F32))
    zero = np.r_[-r.random(n // 4).astype(F32), np.zeros(n // 4, F32), -np.zeros(n // 8, F32),
                 (r.integers(1, 2 ** 23, n // 8).astype(U32)).view(F32), -(r.integers(1, 2 ** 23, n // 8).astype(U32)).view(F32),
                 r.random(n // 8).astype(F32) * F32(1e-3)].astype(F32)
    zero_keys = _shuffled([ord_f32(zero)], 62)
    for k in (1, 10, 100, 256, n // 2, n):
        add(f"one-binade,k={k}", "float", binade, k, 0)
        add(f"gaussian,k={k}", "float", _gauss_keys(n, 63), k, ORD_NEG_INF)
    for k in (1, 100, n // 4, n // 4 + 1, n // 2, zero_keys.size - 5, zero_keys.size):
        add(f"around-zero,k={k}", "float", zero_keys, k, 0)
    for dens in (0.01, 0.5, 0.9, 0.999):
        maxima = (r.standard_normal(n) / np.sqrt(768.0)).astype(F32)
        maxima[r.random(n) < dens] = -np.inf
        keys = ord_f32(maxima)
        na = int((keys > ORD_NEG_INF).sum())
        for k in sorted({1, min(100, na), na, min(na + 1, n), n} - {0}):
            add(f"-inf-density={dens},k={k}", "float", keys, k, ORD_NEG_INF)
    add("gaussian,n=60000,k=100", "float", _gauss_keys(60000, 64), 100, ORD_NEG_INF)
    # tile maxima (the largest of 32 Gaussian scores each): the narrow positive band of the thresholds' samples -- the baseline
    for n_max, k in ((4096, 100), (60000, 100), (8192, 10), (8192, 256)):
        maxima = (np.random.default_rng(65 + n_max).standard_normal((n_max, 32)) / np.sqrt(768.0)).astype(F32).max(axis=1)
        add(f"tile-maxima,n={n_max},k={k}", "float", ord_f32(maxima), k, ORD_NEG_INF, "fast")
    return out


# ------------------------------------------------------------------ k-th key: u64 cases

@dataclass
class Kth64Case:
    name: str
    keys: np.ndarray                 # uint64 [n]
    k: int

    @property
    def n(self) -> int:
        return int(self.keys.size)


def kth64_cases() -> list:
    """(ord << 32) | ~row keys for wg_kth_largest<u64, NT>: the eight radix passes on high words that agree in all, in their upper
    or in their lower bytes, below and above 2 048 keys."""
    out = []
    for n in (1, 2, 300, 1500, 2047, 2049, 5000):
        r = np.random.default_rng(700 + n)
        rows = r.choice(1 << 22, n, replace=False).astype(np.int64)
        rows[r.integers(0, n)] = 0xfffffffe
        rows[r.integers(0, n)] = 0
        rows = np.unique(rows)
        while rows.size < n:
            rows = np.unique(np.r_[rows, r.integers(1, 1 << 31, n - rows.size)])
        r.shuffle(rows)
        base = int(ord_f32(F32(0.3671875)))
        highs = {
            "high-words-equal": np.full(n, base, np.int64),
            "high-words-differ-in-top-byte": (base & 0x00ffffff) | (r.integers(0x80, 0x100, n) << 24),
            "high-words-differ-in-bottom-byte": (base & 0xffffff00) | r.integers(0, 0x100, n),
            "gaussian-scores": _gauss_keys(n, 800 + n).astype(np.int64),
        }
        for tag, high in highs.items():
            keys = (high.astype(U64) << U64(32)) | ((~rows) & 0xffffffff).astype(U64)
            assert np.unique(keys).size == n
            if tag == "high-words-equal":
                assert ref_kth(keys, 1) & 0xffffffff == (~int(rows.min())) & 0xffffffff       # the order is the row's alone
            for k in sorted({1, min(2, n), max(1, n // 2), max(1, n - 1), n}):
                out.append(Kth64Case(f"u64/{tag},n={n},k={k}", keys, k))
        # kNoKey entries among real keys (what select_tail's general path hands the radix)
        keys = (highs["gaussian-scores"].astype(U64) << U64(32)) | ((~rows) & 0xffffffff).astype(U64)
        keys[:: 3] = NO_KEY
        for k in sorted({1, max(1, int((keys != NO_KEY).sum())), min(n, int((keys != NO_KEY).sum()) + 1), n}):
            out.append(Kth64Case(f"u64/with-no-key-entries,n={n},k={k}", keys, k))
    return out


# ------------------------------------------------------------------ select_tail

@dataclass
class TailCase:
    name: str
    keys: np.ndarray                 # uint64 [Ms], unique apart from kNoKey
    k: int
    row_base: int

    @property
    def in_lds(self) -> bool:
        return self.keys.size <= LCAP


def tail_keys(Ms: int, n_nokey: int, seed: int) -> np.ndarray:
    """Ms keys, ``n_nokey`` of them kNoKey spread through the list, the others score_key of scores with ties, zeros of both signs and
    -inf, over unique rows up to 0xfffffffe."""
    r = np.random.default_rng(seed)
    rows = np.unique(1 + r.integers(0, 1 << 32, 2 * Ms + 8, dtype=np.uint64).astype(np.int64) % 0xfffffffd)      # 1 .. 0xfffffffd
    rows = r.permutation(rows)[:Ms]
    if Ms >= 2:
        rows[r.permutation(Ms)[:2]] = (0xfffffffe, 0)
    assert np.unique(rows).size == Ms
    pool = np.r_[(r.standard_normal(max(4, Ms // 3)) / 27.7).astype(F32), F32(0.0), -F32(0.0), F32(-np.inf), F32(1.0), F32(-1.0)]
    scores = r.choice(pool, Ms).astype(F32)                       # many equal scores: the row decides among them
    keys = score_key(scores, rows)
    where = r.permutation(Ms)[:n_nokey]
    keys[where] = NO_KEY
    real = keys[keys != NO_KEY]
    assert np.unique(real).size == real.size and int((keys == NO_KEY).sum()) == n_nokey
    return keys


def tail_cases() -> list:
    out = []
    i = 0
    for Ms in (1, 2, 2047, 2048, 2049, 5000):
        for k in (1, 2, 3, 100, 1023, 1024):
            for n_nokey in sorted({0, 1, min(Ms, Ms // 3 + 1)}):
                i += 1
                out.append(TailCase(f"Ms={Ms},k={k},nokey={n_nokey}", tail_keys(Ms, n_nokey, 900 + i), k, (0, 3 << 32)[i % 2]))
    # fewer real keys than k: the k-th key of the general path is kNoKey itself
    for Ms, real, k in ((5000, 50, 100), (2049, 1, 3), (2049, 0, 2), (4096, 1023, 1024), (2048, 10, 100), (300, 0, 5)):
        out.append(TailCase(f"Ms={Ms},k={k},real-keys={real}", tail_keys(Ms, Ms - real, 990 + real), k, 3 << 32))
    # the whole list is wanted and k is no power of two
    out.append(TailCase("Ms=2049,k=1000,nokey=0", tail_keys(2049, 0, 997), 1000, 0))
    out.append(TailCase("Ms=700,k=700,nokey=5", tail_keys(700, 5, 998), 700, 0))
    return out


# ------------------------------------------------------------------ tile list

TILE_SIZES = (1, 255, 256, 257, 65536, 65537, 65793, 70001, 140000, 312500)
TILE_MASKS = ("zero", "all", "alternating", "first-word", "last-word", "last-workgroup", "words=1", "words=0x80000000", "random-1%",
              "random-50%", "every-256th", "all-but-workgroup-0")


def tile_mask(ntiles: int, kind: str) -> np.ndarray:
    """Mask words [ntiles]; a tile is listed iff its word is not 0."""
    w = np.zeros(ntiles, U32)
    r = np.random.default_rng(ntiles * 31 + TILE_MASKS.index(kind))
    if kind == "all":
        w[:] = r.integers(1, 1 << 32, ntiles, dtype=np.uint64).astype(U32)
    elif kind == "alternating":
        w[1::2] = 0xffffffff
    elif kind == "first-word":
        w[0] = 0x00010000
    elif kind == "last-word":
        w[-1] = 2
    elif kind == "last-workgroup":
        w[(ntiles - 1) // 256 * 256:] = 0xffffffff
    elif kind == "words=1":
        w[r.random(ntiles) < 0.3] = 1
        w[-1] = 1
    elif kind == "words=0x80000000":
        w[r.random(ntiles) < 0.3] = 0x80000000
        w[0] = 0x80000000
    elif kind == "random-1%":
        hit = r.random(ntiles) < 0.01
        w[hit] = r.integers(1, 1 << 32, int(hit.sum()), dtype=np.uint64).astype(U32)
    elif kind == "random-50%":
        hit = r.random(ntiles) < 0.5
        w[hit] = r.integers(1, 1 << 32, int(hit.sum()), dtype=np.uint64).astype(U32)
    elif kind == "every-256th":
        w[255::256] = 4                                             # one word per workgroup, in its last lane
    elif kind == "all-but-workgroup-0":
        w[256:] = 0xffffffff
    else:
        assert kind == "zero"
    return w


def tile_cases() -> list:
    return [(ntiles, kind) for ntiles in TILE_SIZES for kind in TILE_MASKS]
