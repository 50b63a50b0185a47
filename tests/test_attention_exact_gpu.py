"""k_attn / k_attn_long, k_pool and k_embed_ln on inputs whose result is known exactly (tests/attn_cases.py; its preconditions are
proved on the CPU by tests/test_attention_cases_host.py):
  * pointer rows (one-hot attention): the output is the winner's V row, compared as bf16 words;
  * uniform rows (q = 0, 0/1 V): the output is count_d / n_valid within 2^-8 relative, zero counts exactly zero;
  * every mask geometry: whole 64-key tiles and 256-key windows masked, first tile / window empty, one valid key, no valid key;
  * padded rows on both sides of every launch boundary, packed rows back to back in both orders, other head counts;
  * randn inputs of the older tests with a limit that scales with the output: the kernel's relative L2 error per output row is at
    most twice that of the one-pass bf16-P emulation, both against f64 attention;
  * masked mean pool on integer tokens: float32(sum) / float32(count) bit for bit, NaN for a row without a valid token;
  * the embedding at the end of the 1026-row position table.
Queries past the end of the last 64-key tile that holds a valid key are pad tokens behind the text; the kernels write zeros there
(DESIGN.md section 4.1), which is asserted as such."""
import numpy as np
import pytest

from tests import attn_cases as ac

pytestmark = pytest.mark.gpu


def _env():
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    return torch, ffi, torch.device("cuda:0")


def _close(torch, got, ref, rel, abs_):
    err = (got.float() - ref.float()).abs()
    lim = rel * ref.float().abs() + abs_
    assert bool((err <= lim).all()), f"max err {err.max().item():.4g} (worst excess {(err - lim).max().item():.4g})"


def _varlen(qkv_rows, valid_rows, nh):
    """Padded rows of one length through crh_attn_fwd_varlen -> bf16 [B, L, nh * 64] on the CPU; the output starts as NaN."""
    torch, ffi, dev = _env()
    B, L = len(qkv_rows), len(valid_rows[0])
    qkv = torch.from_numpy(np.stack(qkv_rows)).to(dev, torch.bfloat16)
    km = torch.from_numpy(ac.mask_words(valid_rows, L)).to(dev)
    out = torch.full((B, L, nh * 64), float("nan"), dtype=torch.bfloat16, device=dev)
    ffi.check(ffi.lib().crh_attn_fwd_varlen(qkv.data_ptr(), km.data_ptr(), out.data_ptr(), B, L, nh, 0))
    torch.cuda.synchronize()
    return out.cpu()


GUARD = 16


def _packed(qkv_flat, off, valid_rows, Lmax, nh):
    """Packed rows through crh_attn_fwd_packed -> bf16 [T, nh * 64] on the CPU; 16 guard rows behind the output must keep their 7.0."""
    torch, ffi, dev = _env()
    T, B = len(qkv_flat), len(valid_rows)
    qkv = (qkv_flat if isinstance(qkv_flat, torch.Tensor) else torch.from_numpy(qkv_flat)).to(dev, torch.bfloat16)
    km = torch.from_numpy(ac.mask_words(valid_rows, Lmax)).to(dev)
    off_d = torch.from_numpy(np.asarray(off, np.int32)).to(dev)
    out = torch.full((T + GUARD, nh * 64), 7.0, dtype=torch.bfloat16, device=dev)
    ffi.check(ffi.lib().crh_attn_fwd_packed(qkv.data_ptr(), off_d.data_ptr(), km.data_ptr(), out.data_ptr(), B, T, Lmax, nh, 0))
    torch.cuda.synchronize()
    assert ffi.lib().crh_encoder_finish(0) == ffi.OK
    out = out.cpu()
    assert bool((out[T:] == 7.0).all()), "nothing is written past the last token"
    return out[:T]


def _check_row(torch, kind, got, row, valid, what):
    """One row's output (bf16 [L, nh * 64]) against its exact reference."""
    live = ac.live_queries(valid)
    assert bool(torch.isfinite(got.float()).all()), what
    assert bool((got[live:].float() == 0).all()), f"{what}: queries past the last valid key tile are zeros"
    if live == 0:
        return
    if kind == "pointer":
        assert row.gap >= ac.MIN_GAP, (what, row.gap)
        want = torch.from_numpy(row.ref[:live]).bfloat16()
        bad = torch.nonzero((got[:live].view(torch.int16) != want.view(torch.int16)).any(-1)).flatten()
        if len(bad):
            i = int(bad[0])
            h = int(torch.nonzero(got[i].view(torch.int16) != want[i].view(torch.int16))[0]) // 64
            pytest.fail(f"{what}: {len(bad)} query rows differ from V's winner row; first: query {i} head {h} -> key {int(row.pi[h, i])}: "
                        f"got {got[i, h * 64:h * 64 + 4].tolist()} want {want[i, h * 64:h * 64 + 4].tolist()}")
    else:
        ref = torch.from_numpy(row.ref)[None, :]
        err = (got[:live].double() - ref).abs()
        lim = ac.UNIFORM_REL * ref.abs()                      # no absolute term: zero counts must be exactly zero
        if not bool((err <= lim).all()):
            i, e = np.unravel_index(int((err - lim).argmax()), err.shape)
            pytest.fail(f"{what}: query {i} head {e // 64} d {e % 64}: got {float(got[i, e])} want {float(ref[0, e])} "
                        f"(count {int(row.counts.reshape(-1)[e])} of {row.n_valid}), |err| / limit {float(err[i, e] / max(float(lim[0, e]), 1e-30)):.1f}")


def _run_varlen_rows(kind, L, nh, rows, seed):
    """rows: (geometry, winners) list; run in batches of up to 4 padded rows."""
    torch, _, _ = _env()
    for c in range(0, len(rows), 4):
        chunk = rows[c:c + 4]
        built = [ac.varlen_row(kind, L, g, w, seed, nh) for g, w in chunk]
        valid = [ac.geometry(g, L) for g, _ in chunk]
        out = _varlen([r.qkv for r in built], valid, nh)
        for b, (g, w) in enumerate(chunk):
            _check_row(torch, kind, out[b], built[b], valid[b], f"{kind} L={L} H={nh} {g}/{w} (row {b} of its batch)")


@pytest.mark.parametrize("L", ac.VARLEN_L)
@pytest.mark.parametrize("kind", ["pointer", "uniform"])
def test_padded_rows_exact(gpu, kind, L):
    """Every geometry that exists at L (the row without a valid key among its neighbours), and for the pointer case the winner in
    the first valid tile, in the last one, and in each 256-key window in turn."""
    rows = ac.varlen_rows(L)
    if kind == "uniform":
        rows = [r for r in rows if r[1] == "cover"]
    _run_varlen_rows(kind, L, ac.H, rows, 0)


@pytest.mark.parametrize("nh,L", ac.HEAD_CASES)
@pytest.mark.parametrize("kind", ["pointer", "uniform"])
def test_other_head_counts_exact(gpu, kind, nh, L):
    """H = 1 and H = 5 with B = 3: B * H is no multiple of 8, which k_attn_long's grid is rounded up to."""
    rows = [("full", "cover"), ("odd_keys", "cover"), ("tile0" if L > 64 else "one_last", "cover")]
    _run_varlen_rows(kind, L, nh, rows, 1)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("Lmax", [512, 1024])
@pytest.mark.parametrize("kind", ["pointer", "uniform"])
def test_packed_rows_exact(gpu, kind, Lmax, reverse):
    torch, _, _ = _env()
    p = ac.packed_batch(kind, Lmax, reverse, 3)
    out = _packed(p.qkv, p.off, p.valid, Lmax, ac.H)
    for b, row in enumerate(p.rows):
        _check_row(torch, kind, out[p.off[b]:p.off[b + 1]], row, p.valid[b], f"{kind} packed Lmax={Lmax} row {b} (len {len(p.valid[b])}, {p.geoms[b]})")


@pytest.mark.parametrize("reverse", [False, True])
def test_both_kernels_agree_on_masks_with_empty_tiles(gpu, reverse):
    """The rows of <= 512 tokens of the packed batch -- whole tiles masked, tile 0 empty, one valid key, none -- give the same bits
    from k_attn (Lmax 512) and k_attn_long (Lmax 1024): on the two exact inputs and on 3 * randn, where the running maximum moves."""
    torch, _, _ = _env()
    p = ac.packed_batch("pointer", 512, reverse, 3)
    u = ac.packed_batch("uniform", 512, reverse, 3)
    g = torch.Generator(device="cpu").manual_seed(5)
    sharp = (3 * torch.randn((len(p.qkv), 3 * ac.H * 64), generator=g)).bfloat16()
    for what, qkv in (("pointer", p.qkv), ("uniform", u.qkv), ("3 * randn", sharp)):
        a = _packed(qkv, p.off, p.valid, 512, ac.H)
        b = _packed(qkv, p.off, p.valid, 1024, ac.H)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), what
        assert bool(torch.isfinite(a.float()).all())


# Worst e_k / e_m per shape measured on an MI355X (python -m pytest -s prints them): see DESIGN.md section 4.1.
@pytest.mark.parametrize("name", ac.RANDN_CASES)
def test_randn_error_scales_with_the_output(gpu, name):
    """Per output row (token, all heads): relative L2 error against f64 attention, e_k of the kernel and e_m of the bf16-P emulation
    (fp32, P rounded to bf16 for the PV product, sum from the unrounded P, output rounded to bf16: the kernel's rounding points,
    in one pass).  e_k <= 2 e_m: the factor is room for the tile-wise accumulation order and the hardware exp2."""
    torch, ffi, dev = _env()
    case = ac.randn_case(name)
    if case.packed:
        off = np.concatenate([[0], np.cumsum(case.lens)])
        out = _packed(case.qkv, off, [case.valid[b, :n].numpy() for b, n in enumerate(case.lens)], case.L, ac.H)
    else:
        B = case.qkv.shape[0]
        out = _varlen([case.qkv[b].float().numpy() for b in range(B)], [case.valid[b].numpy() for b in range(B)], ac.H).reshape(B * case.L, -1)
    worst, where = 0.0, None
    for sl, x, valid in ac.randn_rows(case):
        ref = ac.attention_plain(x, valid, dtype=torch.float64)
        e_m = ac.row_rel_l2(ac.attention_bf16p(x, valid), ref)
        e_k = ac.row_rel_l2(out[sl], ref)
        _close(torch, out[sl], ref, rel=2 ** -6, abs_=1.5e-2)            # (the older tests' limit holds a fortiori)
        ratio = e_k / e_m
        if float(ratio.max()) > worst:
            worst, where = float(ratio.max()), (sl.start, int(ratio.argmax()), float(e_k[ratio.argmax()]), float(e_m[ratio.argmax()]))
    print(f"attention {name}: worst e_k / e_m = {worst:.3f} (row at token {where[0]}, query {where[1]}: e_k {where[2]:.3e}, e_m {where[3]:.3e})")
    assert worst <= 2.0, (worst, where)


# ---------------------------------------------------------------- masked mean pool

def _check_pool(torch, sent, guard, tok, rows):
    """rows: (slice of the token axis, valid) per batch row."""
    assert bool((guard == 7.0).all())
    for b, (sl, valid) in enumerate(rows):
        want = ac.pool_expected(tok[sl], valid)
        got = sent[b].numpy()
        if not valid.any():
            assert np.isnan(got).all(), f"row {b}: a row without a valid token is 0 / 0"
        else:
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (b, np.abs(got - want).max())


@pytest.mark.parametrize("L", [16, 144, 1024])
def test_pool_is_one_exact_division(gpu, L):
    torch, ffi, dev = _env()
    geoms = ac.geometries_at(L)
    for c in range(0, len(geoms), 4):
        chunk = geoms[c:c + 4]
        B = len(chunk)
        valid = [ac.geometry(g, L) for g in chunk]
        tok = ac.pool_tokens(B * L)
        tok_d = torch.from_numpy(tok).to(dev, torch.bfloat16)
        km = torch.from_numpy(ac.mask_words(valid, L)).to(dev)
        sent = torch.full((B + 2, 768), 7.0, dtype=torch.float32, device=dev)
        ffi.check(ffi.lib().crh_masked_mean_pool(tok_d.data_ptr(), km.data_ptr(), sent.data_ptr(), B, L, 768, 0))
        torch.cuda.synchronize()
        sent = sent.cpu()
        _check_pool(torch, sent[:B], sent[B:], tok, [(slice(b * L, (b + 1) * L), valid[b]) for b in range(B)])


@pytest.mark.parametrize("lens,geoms", [((1, 63, 65, 1023), ("full", "odd_keys", "tile0", "alternate_tiles")),
                                        ((1023, 65, 63, 1), ("interior_window", "empty", "one_last", "one_first")),
                                        ((63, 1023, 1, 65), ("empty", "last_window_only", "full", "last_tile_only"))])
def test_pool_packed_is_one_exact_division(gpu, lens, geoms):
    torch, ffi, dev = _env()
    B, Lmax = len(lens), 1024
    off = np.zeros(B + 1, np.int32)
    np.cumsum(lens, out=off[1:])
    T = int(off[-1])
    valid = [ac.geometry(g, n) for g, n in zip(geoms, lens)]
    tok = ac.pool_tokens(T)
    tok_d = torch.from_numpy(tok).to(dev, torch.bfloat16)
    km = torch.from_numpy(ac.mask_words(valid, Lmax)).to(dev)
    off_d = torch.from_numpy(off).to(dev)
    sent = torch.full((B + 2, 768), 7.0, dtype=torch.float32, device=dev)
    ffi.check(ffi.lib().crh_masked_mean_pool_packed(tok_d.data_ptr(), off_d.data_ptr(), km.data_ptr(), sent.data_ptr(), B, T, Lmax, 768, 0))
    torch.cuda.synchronize()
    assert ffi.lib().crh_encoder_finish(0) == ffi.OK
    sent = sent.cpu()
    _check_pool(torch, sent[:B], sent[B:], tok, [(slice(int(off[b]), int(off[b + 1])), valid[b]) for b in range(B)])


# ---------------------------------------------------------------- embedding at the end of the position table

def test_embed_ln_reaches_the_last_row_of_the_position_table(gpu):
    """L = 1024, pad_id = 1: a full row's position ids run 2 .. 1025, the last row of a 1026-row table; interior pads push the
    positions of the real tokens behind them down.  Against the torch reference and tolerance of test_embed_ln_and_pool."""
    torch, ffi, dev = _env()
    B, L, D, V, pad = 3, 1024, 768, 2000, 1
    g = torch.Generator(device="cpu").manual_seed(19)
    word = torch.randn((V, D), generator=g).to(dev, torch.bfloat16)
    pos = torch.randn((L + 2, D), generator=g).to(dev, torch.bfloat16)
    typ = torch.randn((D,), generator=g).to(dev, torch.bfloat16)
    gam = (1 + 0.1 * torch.randn((D,), generator=g)).to(dev)
    bet = (0.1 * torch.randn((D,), generator=g)).to(dev)
    ids = torch.randint(3, V, (B, L), generator=g, dtype=torch.int32)
    ids[1, 5] = pad                                          # interior pads, real tokens up to the row's end
    ids[1, 100:130] = pad
    ids[1, 511:513] = pad
    ids[1, 960] = pad
    ids[2, 700:] = pad
    ids[2, 64:128] = pad                                     # a whole mask word of pads inside the text
    ids_d = ids.to(dev)
    out = torch.full((B + 1, L, D), 7.0, dtype=torch.bfloat16, device=dev)
    km = torch.full((B + 1, L // 64), 7, dtype=torch.int64, device=dev)
    ffi.check(ffi.lib().crh_embed_ln(ids_d.data_ptr(), word.data_ptr(), pos.data_ptr(), typ.data_ptr(), gam.data_ptr(), bet.data_ptr(),
                                     1e-5, pad, out.data_ptr(), km.data_ptr(), B, L, D, 0))
    valid = ids_d != pad
    pid = torch.cumsum(valid.long(), 1) * valid.long() + pad
    assert int(pid[0, -1]) == L + 1 == pos.shape[0] - 1 and int(pid[1, -1]) == L + 1 - 34 and int(pid.max()) == L + 1
    ref = torch.nn.functional.layer_norm((word[ids_d.long()].float() + typ.float()) + pos[pid].float(), (D,), gam, bet, 1e-5)
    torch.cuda.synchronize()
    assert np.array_equal(km[:B].cpu().numpy(), ac.mask_words(list(valid.cpu().numpy()), L))
    assert bool((km[B:] == 7).all()) and bool((out[B:] == 7.0).all())
    _close(torch, out[:B], ref, rel=2 ** -7, abs_=4e-3)
