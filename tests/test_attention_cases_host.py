"""The preconditions of tests/test_attention_exact_gpu.py, proved without a GPU on exactly the inputs that file runs
(tests/attn_cases.py): every pointer case has its raw-score gap, every uniform reference counts what it claims, every mask
geometry leaves the validity it claims, the mask-word packer is the existing tests' one, the bf16-P emulation lies inside the
existing tests' tolerance of fp32 attention -- and the uniform limit sees one dropped or doubled key out of 1024."""
import numpy as np
import pytest
import torch

from tests import attn_cases as ac
from tests.test_encoder_gpu import _close, _kmask
from tests.test_long_context_gpu import _words


def _check_pointer(r, valid):
    assert r.gap >= ac.MIN_GAP, r.gap
    L = len(valid)
    nh = r.pi.shape[0]
    q, k, v = (r.qkv[:, i * nh * 64:(i + 1) * nh * 64].reshape(L, nh, 64) for i in range(3))
    assert set(np.unique(np.abs(k))) == {4.0} and set(np.unique(v)) <= set(ac.V_SET.tolist()) and not (v == 0).any()
    if not valid.any():
        assert not r.ref.any()
        return
    assert valid[r.pi].all()                                   # queries point at valid keys only
    if L >= valid.sum():
        for h in range(nh):                                    # ... and, over the row, at every one of them
            assert set(r.pi[h]) == set(np.flatnonzero(valid)) or r.pi[h].size < valid.sum()
    assert len({r.pi[h].tobytes() for h in range(nh)}) == nh or valid.sum() == 1     # another map per head
    h, i = nh - 1, L // 2
    assert np.array_equal(q[i, h], k[r.pi[h, i], h]) and np.array_equal(r.ref[i, h * 64:(h + 1) * 64], v[r.pi[h, i], h])


@pytest.mark.parametrize("L", ac.VARLEN_L)
def test_pointer_gap_of_every_padded_row(L):
    for geom, winners in ac.varlen_rows(L):
        valid = ac.geometry(geom, L)
        r = ac.varlen_row("pointer", L, geom, winners, 0)
        assert r.qkv.shape == (L, 3 * ac.H * 64) and r.ref.shape == (L, ac.H * 64)
        assert np.array_equal(torch.from_numpy(r.qkv).bfloat16().float().numpy(), r.qkv)      # exact in bf16
        if winners == "cover":
            _check_pointer(r, valid)
        else:
            assert r.gap >= ac.MIN_GAP and ac.winner_subset(winners, valid)[r.pi].all(), (geom, winners)


def test_winner_subsets_are_the_tiles_and_windows_they_name():
    valid = ac.geometry("tile0", 1024)
    assert np.flatnonzero(ac.winner_subset("first_tile", valid)).tolist() == list(range(64, 128))
    assert np.flatnonzero(ac.winner_subset("last_tile", valid)).tolist() == list(range(960, 1024))
    assert np.flatnonzero(ac.winner_subset("window2", ac.geometry("full", 528))).tolist() == list(range(512, 528))
    assert np.flatnonzero(ac.winner_subset("last_tile", ac.geometry("alternate_tiles", 336))).tolist() == list(range(256, 320))


@pytest.mark.parametrize("nh,L", ac.HEAD_CASES)
def test_pointer_gap_with_other_head_counts(nh, L):
    for geom in ("full", "odd_keys", "tile0" if L > 64 else "one_last"):
        _check_pointer(ac.varlen_row("pointer", L, geom, "cover", 1, nh), ac.geometry(geom, L))


@pytest.mark.parametrize("Lmax", [512, 1024])
@pytest.mark.parametrize("reverse", [False, True])
def test_packed_batches(Lmax, reverse):
    lens = ac.packed_lens(Lmax, reverse)
    p = ac.packed_batch("pointer", Lmax, reverse, 3)
    u = ac.packed_batch("uniform", Lmax, reverse, 3)
    assert p.geoms == u.geoms and p.geoms.count("empty") == 1 and p.off[-1] == sum(lens) == len(p.qkv) == len(u.qkv)
    assert all(a != b for a, b in zip(p.geoms, p.geoms[1:]))   # neighbours differ
    if Lmax == 1024:
        assert len(set(p.geoms)) == len(lens)                  # every row another geometry
        assert {"window0", "interior_window", "last_window_only"} <= set(p.geoms)
    nh = ac.H
    for b, L in enumerate(lens):
        assert np.array_equal(p.valid[b], ac.geometry(p.geoms[b], L))
        _check_pointer(p.rows[b], p.valid[b])
        assert u.rows[b].counts.sum() == nh * p.valid[b].sum()
        # what the row's last tile reaches into: copies of its own first valid keys, under other V values
        reach = min(ac.n_tiles(L) * 64 - L, int(p.valid[b].sum()), lens[b + 1] if b + 1 < len(lens) else 0)
        if reach:
            vk = np.flatnonzero(p.valid[b])[:reach]
            mine, nxt = p.rows[b].qkv, p.rows[b + 1].qkv
            assert np.array_equal(nxt[:reach, nh * 64:2 * nh * 64], mine[vk, nh * 64:2 * nh * 64])
            assert not np.array_equal(nxt[:reach, 2 * nh * 64:], mine[vk, 2 * nh * 64:])
            un, um = u.rows[b + 1].qkv, u.rows[b].qkv
            assert un[0, 2 * nh * 64:].sum() == nh              # a leaked neighbour key adds one count per head
            assert um.shape[1] == un.shape[1]


@pytest.mark.parametrize("L", ac.VARLEN_L + (1, 15, 17, 63, 65, 255, 257, 511, 513, 767, 769, 1023))
def test_uniform_counts_and_geometries(L):
    j = np.arange(L)
    for geom in ac.geometries_at(L):
        valid = ac.geometry(geom, L)
        assert valid.shape == (L,) and valid.dtype == bool
        assert valid.any() == (geom != "empty")
        u = ac.uniform_row(L, valid, 0)
        assert u.n_valid == valid.sum() and (u.counts.sum(1) == u.n_valid).all()
        if u.n_valid:
            assert abs(u.ref.reshape(ac.H, 64).sum(1) - 1).max() < 1e-12
        v = u.qkv[:, 2 * ac.H * 64:].reshape(L, ac.H, 64)
        assert np.array_equal((v[valid].sum(0)).astype(np.int64), u.counts) and not u.qkv[:, : ac.H * 64].any()
        tiles = [bool(valid[t * 64:(t + 1) * 64].any()) for t in range(ac.n_tiles(L))]
        wins = [bool(valid[w * 256:(w + 1) * 256].any()) for w in range((L + 255) // 256)]
        nt = len(tiles)
        if geom == "full":
            assert valid.all()
        elif geom == "interior_tile":
            assert tiles == [t != nt // 2 for t in range(nt)] and 0 < nt // 2 < nt - 1 and valid[j // 64 != nt // 2].all()
        elif geom == "tile0":
            assert np.flatnonzero(valid)[0] == 64 and valid[64:].all()
        elif geom == "last_tile_only":
            assert tiles == [False] * (nt - 1) + [True] and valid[(nt - 1) * 64:].all()
        elif geom == "alternate_tiles":
            assert tiles == [t % 2 == 0 for t in range(nt)]
        elif geom == "one_first":
            assert np.flatnonzero(valid).tolist() == [0]
        elif geom == "one_last":
            assert np.flatnonzero(valid).tolist() == [L - 1]
        elif geom == "odd_keys":
            assert not valid[1::2].any() and valid[0::2].all()
        elif geom == "window0":
            assert L > 512 and wins == [False] + [True] * (len(wins) - 1) and valid[256:].all()
        elif geom == "interior_window":
            assert L > 512 and wins == [True, False] + [True] * (len(wins) - 2) and len(wins) >= 3
        elif geom == "last_window_only":
            assert L > 512 and wins == [False] * (len(wins) - 1) + [True]
    assert [g for g in ac.GEOMETRIES if g.endswith("window") or g.startswith("window") or g == "last_window_only"] \
        == ["window0", "interior_window", "last_window_only"]
    assert all(ac.applies(g, L) == (L > 512) for g in ("window0", "interior_window", "last_window_only"))


def test_live_queries():
    assert ac.live_queries(ac.geometry("one_first", 1024)) == 64
    assert ac.live_queries(ac.geometry("one_last", 80)) == 80
    assert ac.live_queries(ac.geometry("alternate_tiles", 512)) == 448
    assert ac.live_queries(ac.geometry("empty", 64)) == 0
    assert ac.live_queries(ac.geometry("full", 17)) == 17


@pytest.mark.parametrize("L", [16, 80, 144, 512, 1024])
def test_mask_words_agree_with_the_existing_packers(L):
    rows = [ac.geometry(g, L) for g in ac.geometries_at(L)]
    valid = torch.from_numpy(np.stack(rows))
    w = ac.mask_words(rows, L)
    assert w.dtype == np.int64 and np.array_equal(w, _kmask(torch, valid).numpy()) and np.array_equal(w, _words(torch, valid).numpy())
    short = [r[: L - 5] for r in rows]                        # packed rows shorter than Lmax: the tail bits are 0
    padded = valid.clone()
    padded[:, L - 5:] = False
    assert np.array_equal(ac.mask_words(short, L), _words(torch, padded).numpy())


@pytest.mark.parametrize("name", ac.RANDN_CASES)
def test_bf16p_emulation_lies_inside_the_existing_tolerance(name):
    """The reference of the scaled limit is the same operation the existing tests compare with: on their inputs the emulation is
    within their rel = 2^-6, abs = 1.5e-2 of plain fp32 attention, so `e_k <= 2 e_m` is the stricter limit, not another one."""
    case = ac.randn_case(name)
    worst = 0.0
    for _, x, valid in ac.randn_rows(case):
        em = ac.attention_bf16p(x, valid)
        f32 = ac.attention_plain(x, valid)
        _close(torch, em, f32, rel=2 ** -6, abs_=1.5e-2)
        e = ac.row_rel_l2(em, ac.attention_plain(x, valid, dtype=torch.float64))
        worst = max(worst, float(e.max()))
        assert float(e.max()) < 2 ** -7                       # the emulation's own error: bf16 roundings, far below the old limit
    print(f"{name}: worst relative L2 of the emulation per row {worst:.3e}")


def test_uniform_limit_sees_one_key_of_1024():
    """The mutation argument, on the CPU: at L = 1024 (16 keys per element) the reference with one key dropped, or one key counted
    twice, leaves the 2^-8 limit by a factor of 15.7 in the element that key feeds; the old absolute term 1.5e-2 is 0.96 of the
    output itself (16 / 1024) and sees neither."""
    valid = ac.geometry("full", 1024)
    ref = ac.uniform_row(1024, valid, 0).ref.reshape(ac.H, 64)
    assert (ref == 16 / 1024).all()
    dropped = valid.copy()
    dropped[333] = False
    c_drop = ac.uniform_counts(dropped) / 1023.0
    c_dbl = ac.uniform_counts(valid).astype(np.float64)
    for h in range(ac.H):
        c_dbl[h, (333 + h) % 64] += 1
    c_dbl /= 1025.0
    for mutant in (c_drop, c_dbl):
        excess = np.abs(mutant - ref) / (ac.UNIFORM_REL * ref)
        print(f"worst |err| / limit of the mutant: {excess.max():.2f}")
        assert 15.5 < excess.max() < 16 and (excess.max(1) > 15.5).all()          # every head, far outside
        assert (np.abs(mutant - ref) <= 2 ** -6 * ref + 1.5e-2).all()              # ... and inside the old tolerance


def test_pool_reference():
    tok = ac.pool_tokens(200)
    assert tok.min() == -4 and tok.max() == 4 and np.array_equal(torch.from_numpy(tok).bfloat16().float().numpy(), tok)
    valid = ac.geometry("odd_keys", 144)
    e = ac.pool_expected(tok[:144], valid)
    assert e.dtype == np.float32 and np.allclose(e, tok[:144][valid].mean(0), rtol=1e-6)
    assert np.isnan(ac.pool_expected(tok[:16], ac.geometry("empty", 16))).all()
