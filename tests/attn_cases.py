"""Inputs whose attention output is known exactly, mask geometries, and CPU references (numpy / torch on the CPU; no GPU import).

Two regimes of softmax attention are predictable to the bit whatever the order of accumulation:
  * pointer (one-hot weights): keys k_j = 4 s_j with s_j random +-1 vectors, queries equal to one of the valid keys.  The winner's
    raw score is 16 * 64 = 1024; every other key's is lower by `gap`, which the builder computes in f64.  With gap >= 256 the
    losers' exponents lie >= 256 * 0.125 * log2(e) = 46 below the winner's, their total weight is below 1024 * 2^-46 = 2^-36, and
    neither the sum (1.0) nor an output element (|V| >= 0.5) moves in f32: the output is the winner's V row, bit for bit;
  * uniform (exact counting): q = 0, so every valid key weighs exactly 1, the sum is the number of valid keys and, with
    V[j, h, d] = [(j + h) % 64 == d], the PV sums are integer counts.  Element d of the output is count_d / n_valid.

Every input value is exact in bf16.  MIN_GAP and UNIFORM_REL are the limits the tests assert.
"""
import functools
from typing import NamedTuple, Optional

import numpy as np
import torch

H = 12                  # heads, except where a case varies it
HD = 64                 # head dimension (fixed by the kernels)
MIN_GAP = 256.0         # raw-score gap every pointer case must have
UNIFORM_REL = 2.0 ** -8     # one bf16 rounding (2^-9) + two f32 roundings (reciprocal, product), x2 for a hardware reciprocal
V_SET = np.array([0.5, 0.75, 1.0, 1.5, 2.0, 3.0, -0.5, -0.75, -1.0, -1.5, -2.0, -3.0], np.float32)   # bf16-exact, never 0

# ---------------------------------------------------------------- mask geometries (functions of the row length L)

GEOMETRIES = ("full", "interior_tile", "tile0", "last_tile_only", "alternate_tiles", "one_first", "one_last", "odd_keys",
              "window0", "interior_window", "last_window_only", "empty")


def n_tiles(L: int) -> int:
    return (L + 63) // 64


def applies(name: str, L: int) -> bool:
    """Whether geometry `name` exists at row length L (and leaves a valid key, unless it is the empty row)."""
    if name in ("full", "one_first", "one_last", "odd_keys", "empty"):
        return True
    if name == "interior_tile":
        return n_tiles(L) >= 3
    if name in ("tile0", "last_tile_only", "alternate_tiles"):
        return n_tiles(L) >= 2
    if name in ("window0", "interior_window", "last_window_only"):
        return L > 512
    raise KeyError(name)


def geometry(name: str, L: int) -> np.ndarray:
    """bool [L]: which keys of a row of L tokens are valid.  Tiles are 64 keys, windows 256 (k_attn_long's staging unit)."""
    assert applies(name, L), (name, L)
    j = np.arange(L)
    nt = n_tiles(L)
    if name == "full":
        return np.ones(L, bool)
    if name == "empty":
        return np.zeros(L, bool)
    if name == "interior_tile":
        return j // 64 != nt // 2
    if name == "tile0":
        return j >= 64
    if name == "last_tile_only":
        return j >= (nt - 1) * 64
    if name == "alternate_tiles":
        return (j // 64) % 2 == 0
    if name == "one_first":
        return j == 0
    if name == "one_last":
        return j == L - 1
    if name == "odd_keys":
        return j % 2 == 0
    if name == "window0":
        return j >= 256
    if name == "interior_window":
        return (j < 256) | (j >= 512)
    if name == "last_window_only":
        return j >= (L - 1) // 256 * 256
    raise KeyError(name)


def geometries_at(L: int):
    return [g for g in GEOMETRIES if applies(g, L)]


def mask_words(valid_rows, Lpad: int) -> np.ndarray:
    """Rows of bool validity (each no longer than Lpad) -> int64 [B, ceil(Lpad / 64)] bit words, bit i of word w = key 64 w + i."""
    nw = (Lpad + 63) // 64
    bits = np.zeros((len(valid_rows), nw * 64), np.uint64)
    for b, v in enumerate(valid_rows):
        assert len(v) <= Lpad
        bits[b, : len(v)] = v
    words = (bits.reshape(len(valid_rows), nw, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)
    return np.ascontiguousarray(words.view(np.int64))


def live_queries(valid: np.ndarray) -> int:
    """Queries [0, live) of a row are computed: those before the end of the last 64-key tile that holds a valid key.  The kernels
    write zeros for the rest (pad tokens behind the text: never read as keys, never pooled)."""
    nz = np.flatnonzero(valid)
    return 0 if len(nz) == 0 else min(len(valid), (int(nz[-1]) // 64 + 1) * 64)


def winner_subset(mode: str, valid: np.ndarray) -> np.ndarray:
    """bool [L]: the valid keys the queries may point at.  "cover": all of them; "first_tile" / "last_tile": those of the first /
    last 64-key tile that has one (every later tile rescaled to nothing / the running maximum moves in the final step);
    "window<w>": those of 256-key window w."""
    j = np.arange(len(valid))
    nz = np.flatnonzero(valid)
    if mode == "cover" or len(nz) == 0:
        return valid.copy()
    if mode == "first_tile":
        return valid & (j // 64 == nz[0] // 64)
    if mode == "last_tile":
        return valid & (j // 64 == nz[-1] // 64)
    if mode.startswith("window"):
        return valid & (j // 256 == int(mode[6:]))
    raise KeyError(mode)


# ---------------------------------------------------------------- pointer case

class PointerRow(NamedTuple):
    qkv: np.ndarray         # f32 [L, 3 * H * 64]: q | k | v thirds, head-major inside a third (bf16-exact values)
    ref: np.ndarray         # f32 [L, H * 64]: V's winner row per (query, head); zeros for a row without a valid key
    gap: float              # smallest raw-score distance winner - any other valid key, over all queries and heads (f64)
    pi: np.ndarray          # int [H, L]: the key each query points at (-1: none)


def _keys(L: int, nh: int, seed: int, head: Optional[np.ndarray]) -> np.ndarray:
    return _keys_cached(L, nh, seed) if head is None else _draw_keys(L, nh, seed, head)


@functools.lru_cache(maxsize=None)
def _keys_cached(L: int, nh: int, seed: int) -> np.ndarray:
    k = _draw_keys(L, nh, seed, None)
    k.setflags(write=False)
    return k


def _draw_keys(L: int, nh: int, seed: int, head: Optional[np.ndarray]) -> np.ndarray:
    """+-4 keys [L, nh, 64] no two of which (valid or not) come closer than MIN_GAP in raw score: drawn again until that holds,
    so that every mask and every query map over them has the gap.  `head`: keys copied to the front (see packed_batch)."""
    for attempt in range(32):
        rng = np.random.default_rng([seed, L, nh, attempt])
        k = (4 * (2 * rng.integers(0, 2, (L, nh, HD)) - 1)).astype(np.float32)
        if head is not None:
            k[: len(head)] = head
        kk = k.transpose(1, 0, 2) @ k.transpose(1, 2, 0)    # [nh, L, L], exact in f32: integers up to 1024
        kk[:, np.arange(L), np.arange(L)] = -np.inf
        if L == 1 or 1024.0 - kk.max() >= MIN_GAP:
            return k
    raise AssertionError("no key set with the gap")


def pointer_row(L: int, valid: np.ndarray, seed: int, nh: int = H, winners: str = "cover", head: Optional[np.ndarray] = None) -> PointerRow:
    k = _keys(L, nh, seed, head)
    rng = np.random.default_rng([seed, L, nh, 77])
    v = V_SET[rng.integers(0, len(V_SET), (L, nh, HD))]
    tgt = np.flatnonzero(winner_subset(winners, valid))
    vk = np.flatnonzero(valid)
    if len(tgt) == 0:
        assert len(vk) == 0
        qkv = np.concatenate([k.reshape(L, -1), k.reshape(L, -1), v.reshape(L, -1)], 1)
        return PointerRow(qkv, np.zeros((L, nh * HD), np.float32), float("inf"), np.full((nh, L), -1))
    # query i of head h points at tgt[perm_h[i mod n]]: onto, every target hit once L >= n, another map per head
    pi = np.stack([tgt[rng.permutation(len(tgt))[np.arange(L) % len(tgt)]] for _ in range(nh)])
    hh = np.arange(nh)[:, None]
    q = k[pi, hh].transpose(1, 0, 2)                    # [L, nh, 64]
    ref = v[pi, hh].transpose(1, 0, 2)
    gap = float("inf")
    for h in range(nh):
        s = q[:, h].astype(np.float64) @ k[vk, h].astype(np.float64).T      # [L, n_valid]
        col = np.searchsorted(vk, pi[h])
        assert np.all(s[np.arange(L), col] == 1024.0)
        s[np.arange(L), col] = -np.inf
        if len(vk) > 1:
            gap = min(gap, float(1024.0 - s.max()))
    qkv = np.concatenate([q.reshape(L, -1), k.reshape(L, -1), v.reshape(L, -1)], 1)
    return PointerRow(np.ascontiguousarray(qkv), np.ascontiguousarray(ref.reshape(L, -1)), gap, pi)


# ---------------------------------------------------------------- uniform case

class UniformRow(NamedTuple):
    qkv: np.ndarray         # f32 [L, 3 * H * 64]
    ref: np.ndarray         # f64 [H * 64]: count_d / n_valid, the same for every query of the row (zeros without a valid key)
    counts: np.ndarray      # int64 [H, 64]
    n_valid: int


def uniform_counts(valid: np.ndarray, nh: int = H) -> np.ndarray:
    """counts[h, d] = number of valid keys j with (j + h) % 64 == d."""
    c = np.zeros((nh, HD), np.int64)
    j = np.flatnonzero(valid)
    for h in range(nh):
        np.add.at(c[h], (j + h) % 64, 1)
    return c


def uniform_row(L: int, valid: np.ndarray, seed: int, nh: int = H) -> UniformRow:
    g = torch.Generator(device="cpu").manual_seed(seed * 7919 + L)
    k = torch.randn((L, nh * HD), generator=g).bfloat16().float().numpy()        # arbitrary: q = 0 makes every score 0
    j, h, d = np.arange(L)[:, None, None], np.arange(nh)[None, :, None], np.arange(HD)[None, None, :]
    v = ((j + h) % 64 == d).astype(np.float32)
    counts = uniform_counts(valid, nh)
    n = int(valid.sum())
    ref = counts.reshape(-1).astype(np.float64) / n if n else np.zeros(nh * HD)
    qkv = np.concatenate([np.zeros((L, nh * HD), np.float32), k, v.reshape(L, -1)], 1)
    return UniformRow(np.ascontiguousarray(qkv), ref, counts, n)


# ---------------------------------------------------------------- the shapes the GPU file runs (and the host file proves)

VARLEN_L = (16, 64, 80, 320, 336, 512, 528, 768, 1024)      # both sides of attn_launch's boundaries: nqt 4|5, 20|21, L 512|528 (3, 4 windows)
HEAD_CASES = ((1, 64), (5, 64), (1, 528), (5, 528))          # (H, L)
PACKED_LENS = {512: (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512), 1024: (1, 17, 256, 511, 513, 767, 769, 1023, 1024)}


def varlen_rows(L: int):
    """(geometry, winners) of every row run at padded length L: each geometry that exists there with queries over all its valid
    keys, then both running-maximum extremes on the masks with more than one valid tile, then (L > 512) each window in turn."""
    rows = [(g, "cover") for g in geometries_at(L)]
    for g in ("full", "alternate_tiles", "tile0", "interior_window"):
        if applies(g, L) and n_tiles(L) >= 2:
            rows += [(g, "first_tile"), (g, "last_tile")]
    if L > 512:
        rows += [("full", f"window{w}") for w in range((L + 255) // 256)]
    return rows


# one geometry per row of the packed batches, in the order the rows sit in; one row of each batch has no valid key
PACKED_GEOMS = {
    (512, False): ("full", "odd_keys", "one_last", "one_first", "full", "odd_keys", "tile0", "empty", "alternate_tiles", "last_tile_only",
                   "interior_tile", "tile0"),
    (512, True): ("interior_tile", "alternate_tiles", "tile0", "last_tile_only", "one_last", "last_tile_only", "empty", "one_first",
                  "odd_keys", "full", "one_last", "full"),
    (1024, False): ("full", "odd_keys", "last_tile_only", "empty", "window0", "interior_window", "last_window_only", "alternate_tiles",
                    "interior_tile"),
    (1024, True): ("window0", "last_window_only", "interior_window", "tile0", "last_tile_only", "alternate_tiles", "empty", "one_last", "full"),
}


def packed_lens(Lmax: int, reverse: bool):
    return PACKED_LENS[Lmax][::-1] if reverse else PACKED_LENS[Lmax]


class PackedBatch(NamedTuple):
    qkv: np.ndarray         # f32 [T, 3 * H * 64]
    off: np.ndarray         # int32 [B + 1]
    valid: list             # bool [len] per row
    rows: list              # PointerRow / UniformRow per row
    geoms: list


@functools.lru_cache(maxsize=None)
def packed_batch(kind: str, Lmax: int, reverse: bool, seed: int, nh: int = H) -> PackedBatch:
    """Rows back to back.  Pointer rows: the keys of the NEXT row that this row's last 64-key tile reaches into are copies of this
    row's first valid keys (with that row's own V): if one of them were counted, the queries that point at the original would see
    a tie and return the mean of two different V rows.  Uniform rows: V is indexed by the row-local key, so a neighbour's key
    always adds to a count."""
    lens, geoms = packed_lens(Lmax, reverse), list(PACKED_GEOMS[(Lmax, reverse)])
    rows, valid, head = [], [], None
    for b, (L, g) in enumerate(zip(lens, geoms)):
        v = geometry(g, L)
        valid.append(v)
        if kind == "pointer":
            r = pointer_row(L, v, seed + b, nh, head=None if head is None else head[:L])
            reach = n_tiles(L) * 64 - L
            vk = np.flatnonzero(v)[:reach]
            head = r.qkv[vk, nh * HD: 2 * nh * HD].reshape(len(vk), nh, HD) if len(vk) else None
        else:
            r = uniform_row(L, v, seed + b, nh)
        rows.append(r)
    off = np.zeros(len(lens) + 1, np.int32)
    np.cumsum(lens, out=off[1:])
    return PackedBatch(np.ascontiguousarray(np.concatenate([r.qkv for r in rows])), off, valid, rows, geoms)


@functools.lru_cache(maxsize=None)
def varlen_row(kind: str, L: int, geom: str, winners: str, seed: int, nh: int = H):
    v = geometry(geom, L)
    return pointer_row(L, v, seed, nh, winners) if kind == "pointer" else uniform_row(L, v, seed, nh)


# ---------------------------------------------------------------- references for the randn cases

def _split(x: torch.Tensor, nh: int):
    n = x.shape[0]
    return (t.reshape(n, nh, HD).transpose(0, 1) for t in x.split(nh * HD, dim=-1))


def attention_plain(x: torch.Tensor, valid: torch.Tensor, nh: int = H, dtype=torch.float32) -> torch.Tensor:
    """Softmax attention of one row in `dtype` (float32: what the existing tests compare with; float64: the reference of the
    scaled limit).  x [n, 3 * nh * 64] holding bf16-exact values, valid bool [n] over the keys.  -> [n, nh * 64]."""
    q, k, v = _split(x.to(dtype), nh)
    s = (q @ k.transpose(-1, -2) * 0.125).masked_fill(~valid[None, None, :], float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(0, 1).reshape(x.shape[0], nh * HD)


def attention_bf16p(x: torch.Tensor, valid: torch.Tensor, nh: int = H) -> torch.Tensor:
    """The kernels' documented rounding points in one pass, no tiling: f32 scores and exponentials, P rounded to bf16 for the PV
    product, the normalising sum taken from the unrounded P, the output rounded to bf16.  -> bf16 [n, nh * 64]."""
    q, k, v = _split(x.float(), nh)
    s = (q @ k.transpose(-1, -2) * 0.125).masked_fill(~valid[None, None, :], float("-inf"))
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    o = (p.bfloat16().float() @ v) / p.sum(-1, keepdim=True)
    return o.transpose(0, 1).reshape(x.shape[0], nh * HD).bfloat16()


def row_rel_l2(got: torch.Tensor, ref64: torch.Tensor) -> torch.Tensor:
    """Relative L2 error per output row (one token, all heads) against the f64 reference."""
    return (got.double() - ref64).norm(dim=-1) / ref64.norm(dim=-1)


class RandnCase(NamedTuple):
    packed: bool
    qkv: torch.Tensor       # bf16, [B, L, 3*H*64] or [T, 3*H*64]
    valid: torch.Tensor     # bool [B, L] (padded) / [B, Lmax] (packed)
    lens: tuple             # padded: index past the last valid key per row (the specified rows); packed: row lengths
    L: int                  # L / Lmax


@functools.lru_cache(maxsize=None)
def randn_case(name: str) -> RandnCase:
    """The seeded inputs of tests/test_encoder_gpu.py::test_attention (L 64, 512), of test_long_attention_padded_rows (L 1024) and
    the 3 * randn packed batch of test_rows_that_fit_k_attn_give_the_same_bits_from_k_attn_long (Lmax 512 and 1024)."""
    if name in ("L64", "L512"):
        B, L = (3, 64) if name == "L64" else (4, 512)
        g = torch.Generator(device="cpu").manual_seed(B * L)
        qkv = torch.randn((B, L, 3 * H * HD), generator=g).bfloat16()
        lens = torch.randint(5, L + 1, (B,), generator=g)
        lens[0] = L
        valid = torch.arange(L)[None, :] < lens[:, None]
        if L > 64:
            valid[1, 70:75] = False
    elif name == "L1024":
        B, L = 4, 1024
        g = torch.Generator(device="cpu").manual_seed(L)
        qkv = torch.randn((B, L, 3 * H * HD), generator=g).bfloat16()
        lens = torch.tensor([L, L - 7, min(L, 600), 100])
        valid = torch.arange(L)[None, :] < lens[:, None]
        valid[1, 511] = False
        valid[1, 512] = False
        valid[2, 300:320] = False
    elif name in ("sharp512", "sharp1024"):
        L = int(name[5:])
        rng = np.random.default_rng(4)
        lens = [5, 16, 17, 63, 64, 65, 127, 200, 255, 256, 257, 300, 383, 448, 500, 511, 512] + rng.integers(5, 513, 15).tolist()
        g = torch.Generator(device="cpu").manual_seed(5)
        qkv = (3 * torch.randn((sum(lens), 3 * H * HD), generator=g)).bfloat16()
        valid = torch.zeros((len(lens), L), dtype=torch.bool)
        for b, n in enumerate(lens):
            valid[b, :n] = True
        valid[7, 70:75] = False
        return RandnCase(True, qkv, valid, tuple(lens), L)
    else:
        raise KeyError(name)
    last = tuple(int(torch.nonzero(valid[b])[-1]) + 1 for b in range(B))
    return RandnCase(False, qkv, valid, last, L)


RANDN_CASES = ("L64", "L512", "L1024", "sharp512", "sharp1024")


def randn_rows(case: RandnCase):
    """(slice of the flat token axis, x [n, 3*H*64] bf16, valid bool [n]) per row: the rows whose output is specified."""
    out = []
    if case.packed:
        off = np.concatenate([[0], np.cumsum(case.lens)])
        for b, n in enumerate(case.lens):
            out.append((slice(int(off[b]), int(off[b + 1])), case.qkv[off[b]:off[b + 1]], case.valid[b, :n]))
    else:
        for b, n in enumerate(case.lens):
            out.append((slice(b * case.L, b * case.L + n), case.qkv[b, :n], case.valid[b, :n]))
    return out


# ---------------------------------------------------------------- masked mean pool: integer tokens, exact quotients

def pool_tokens(T: int, D: int = 768) -> np.ndarray:
    """tok[t, d] = ((7 t + d) % 9) - 4 over the flat token axis: integers in [-4, 4], exact in bf16; sums of <= 1024 of them are exact in f32."""
    t, d = np.arange(T)[:, None], np.arange(D)[None, :]
    return (((t * 7 + d) % 9) - 4).astype(np.float32)


def pool_expected(tok_row: np.ndarray, valid: np.ndarray) -> np.ndarray:
    """float32(sum) / float32(count): one correctly rounded division of two exact integers (0 / 0 = NaN for a row without a valid token)."""
    s = tok_row[valid].astype(np.int64).sum(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return s.astype(np.float32) / np.float32(int(valid.sum()))
