"""GPU tier for rows of 513..1024 tokens (k_attn_long behind crh_attn_fwd_varlen / crh_attn_fwd_packed): the kernel against
fp32 torch attention, bit-identity with k_attn for every row that k_attn can take, the whole 12-layer forward against the
long-row HF fixture, and the provider end to end at max_length = 1023."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
H = 12


def _env():
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    return torch, ffi, torch.device("cuda:0")


def _close(torch, got, ref, rel, abs_):
    err = (got.float() - ref.float()).abs()
    lim = rel * ref.float().abs() + abs_
    assert bool((err <= lim).all()), f"max err {err.max().item():.4g} (worst excess {(err - lim).max().item():.4g})"


def _words(torch, valid):                                   # valid: bool [B, L] -> int64 [B, ceil(L/64)] bit words
    B, L = valid.shape
    Lp = (L + 63) // 64 * 64
    v = torch.zeros((B, Lp), dtype=torch.bool)
    v[:, :L] = valid
    return (v.reshape(B, Lp // 64, 64).to(torch.int64) << torch.arange(64, dtype=torch.int64)).sum(-1).contiguous()


def _ref_rows(torch, x, valid_row):
    """fp32 softmax attention of one row: x bf16 [n, 3*H*64], valid_row bool [n] (keys)."""
    n = x.shape[0]
    q, k, v = (t.reshape(n, H, 64).transpose(0, 1) for t in x.float().split(H * 64, dim=-1))
    s = q @ k.transpose(-1, -2) * 0.125
    s = s.masked_fill(~valid_row.to(x.device)[None, None, :], float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(0, 1).reshape(n, H * 64)


@pytest.mark.parametrize("L", [528, 640, 1008, 1024])
def test_long_attention_padded_rows(gpu, L):
    torch, ffi, dev = _env()
    B = 4
    g = torch.Generator(device="cpu").manual_seed(L)
    qkv = torch.randn((B, L, 3 * H * 64), generator=g).to(dev, torch.bfloat16)
    lens = torch.tensor([L, L - 7, min(L, 600), 100])         # row 3: its last valid key lies in the first 256-key window
    valid = torch.arange(L)[None, :] < lens[:, None]
    valid[1, 511] = False                                     # masked keys on either side of the 512-key boundary
    valid[1, 512] = False
    valid[2, 300:320] = False
    km = _words(torch, valid).to(dev)
    out = torch.full((B, L, H * 64), float("nan"), dtype=torch.bfloat16, device=dev)
    ffi.check(ffi.lib().crh_attn_fwd_varlen(qkv.data_ptr(), km.data_ptr(), out.data_ptr(), B, L, H, 0))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all()), "every output row must be finite (pad rows included)"
    for b in range(B):
        last = int(torch.nonzero(valid[b])[-1]) + 1
        _close(torch, out[b, :last], _ref_rows(torch, qkv[b, :last], valid[b, :last]), rel=2 ** -6, abs_=1.5e-2)
        lk = (last + 63) // 64 * 64                           # query tiles past the last valid key tile: zeros
        assert bool((out[b, lk:].float() == 0).all())


def test_long_attention_packed_rows_leave_their_neighbours_alone(gpu):
    torch, ffi, dev = _env()
    lens = [1024, 7, 513, 1000, 64, 777, 1, 900, 530]
    off = np.zeros(len(lens) + 1, np.int32)
    np.cumsum(lens, out=off[1:])
    T, Lmax = int(off[-1]), 1024
    g = torch.Generator(device="cpu").manual_seed(11)
    qkv = torch.randn((T, 3 * H * 64), generator=g).to(dev, torch.bfloat16)
    valid = torch.zeros((len(lens), Lmax), dtype=torch.bool)
    for b, n in enumerate(lens):
        valid[b, :n] = True
    valid[3, 511] = valid[3, 512] = False                     # interior masked keys around the boundary
    km = _words(torch, valid).to(dev)
    out = torch.full((T + 16, H * 64), 7.0, dtype=torch.bfloat16, device=dev)          # 16 guard rows
    off_d = torch.from_numpy(off).to(dev)
    ffi.check(ffi.lib().crh_attn_fwd_packed(qkv.data_ptr(), off_d.data_ptr(), km.data_ptr(), out.data_ptr(), len(lens), T, Lmax, H, 0))
    torch.cuda.synchronize()
    assert bool((out[T:] == 7.0).all()), "nothing is written past the last token"
    assert bool(torch.isfinite(out[:T].float()).all())
    for b, n in enumerate(lens):
        _close(torch, out[off[b]:off[b + 1]], _ref_rows(torch, qkv[off[b]:off[b + 1]], valid[b, :n]), rel=2 ** -6, abs_=1.5e-2)


def test_rows_that_fit_k_attn_give_the_same_bits_from_k_attn_long(gpu):
    """Rows of 5..512 tokens in a batch whose Lmax is 1024 (k_attn_long) against the same rows with Lmax 512 (k_attn): the same
    64-key tile update in the same key order, so the same bits -- the property that makes an embedding independent of its batch."""
    torch, ffi, dev = _env()
    rng = np.random.default_rng(4)
    lens = [5, 16, 17, 63, 64, 65, 127, 200, 255, 256, 257, 300, 383, 448, 500, 511, 512] + rng.integers(5, 513, 15).tolist()
    off = np.zeros(len(lens) + 1, np.int32)
    np.cumsum(lens, out=off[1:])
    T = int(off[-1])
    g = torch.Generator(device="cpu").manual_seed(5)
    qkv = (3 * torch.randn((T, 3 * H * 64), generator=g)).to(dev, torch.bfloat16)     # sharp scores: the running max moves
    off_d = torch.from_numpy(off).to(dev)
    outs = {}
    for Lmax in (512, 1024):
        valid = torch.zeros((len(lens), Lmax), dtype=torch.bool)
        for b, n in enumerate(lens):
            valid[b, :n] = True
        valid[7, 70:75] = False
        km = _words(torch, valid).to(dev)
        out = torch.full((T, H * 64), 7.0, dtype=torch.bfloat16, device=dev)
        ffi.check(ffi.lib().crh_attn_fwd_packed(qkv.data_ptr(), off_d.data_ptr(), km.data_ptr(), out.data_ptr(), len(lens), T, Lmax, H, 0))
        outs[Lmax] = out
    torch.cuda.synchronize()
    assert torch.equal(outs[512].view(torch.int16), outs[1024].view(torch.int16))


def _model(cfg_kw=None, seed=23, **kw):
    from coderag_amd import encoder as drv
    cfg = drv.EncoderConfig(**(cfg_kw or {}), **kw)
    return drv, drv.HipUniXcoder(drv.synthetic_weights(cfg, seed), cfg, drv.HashTokenizer(cfg.vocab_size), 0)


def test_a_short_chunk_keeps_its_vector_beside_a_long_one(gpu):
    torch, ffi, dev = _env()
    drv, model = _model(num_layers=2)
    rng = np.random.default_rng(8)
    row = lambda n: [0, 6, 2] + rng.integers(16, model.cfg.vocab_size, n - 4).tolist() + [2]   # noqa: E731
    shorts = [row(n) for n in (5, 40, 130, 300, 512)]
    longs = [row(1000), row(1024), row(700)]
    alone = model.embed_ids(shorts).cpu().numpy()
    mixed = model.embed_ids(shorts + longs).cpu().numpy()               # one packed batch, Lmax 1024: k_attn_long for all rows
    assert np.array_equal(alone, mixed[: len(shorts)])
    for i, r in enumerate(shorts):
        assert np.array_equal(model.embed_ids([r, longs[0]]).cpu().numpy()[0], alone[i]), len(r)
    assert np.array_equal(model.embed_ids(longs).cpu().numpy(), mixed[len(shorts):])
    assert np.isfinite(mixed).all()


# (min cosine, max relative L2) vs the bf16-storage oracle and vs the fp32 HF fixture: ENCODER_TOL["hfinit"] of test_encoder_gpu.py
LONG_TOL = ((0.99995, 1e-2), (0.9999, 1.5e-2))


@pytest.mark.parametrize("form", ["two LayerNorm kernels", "ln_fold", "residual_f32"])
def test_long_encoder_against_hf_fixture(gpu, form):
    """Padded (1024-token rows) and packed forwards of the 12-layer HF-init geometry on rows of 1024 / 1023 / 777 / 520 tokens
    against the bf16-storage oracle and the HF fp32 vectors; padded and packed give the same bits."""
    torch, ffi, dev = _env()
    from coderag_amd import encoder as drv
    from oracle import encoder as orc
    z = np.load(os.path.join(GOLD, "encoder_long.npz"))
    c = [int(v) for v in z["cfg"]]
    kw = dict(vocab_size=c[0], hidden_size=c[1], num_layers=c[2], num_heads=c[3], intermediate_size=c[4],
              max_position_embeddings=c[5], type_vocab_size=c[6], pad_token_id=c[7], layer_norm_eps=float(z["eps"]))
    fold, res32 = form == "ln_fold", form == "residual_f32"
    cfg = drv.EncoderConfig(**kw, ln_fold=fold, residual_f32=res32)
    weights = drv.synthetic_weights(cfg, int(z["seed"]), init=str(z["init"]))
    model = drv.HipUniXcoder(weights, cfg, drv.HashTokenizer(cfg.vocab_size), 0)
    padded = model.forward_ids(torch.from_numpy(z["ids"].astype(np.int32)).to(dev)).cpu().numpy()
    rows = [r[: int(np.flatnonzero(r != cfg.pad_token_id)[-1]) + 1].astype(np.int32) for r in z["ids"]]
    flat, off, Lmax = model.pack_rows(rows, list(range(len(rows))))
    assert Lmax == 1024
    packed = model.forward_packed(torch.from_numpy(flat).to(dev), torch.from_numpy(off).to(dev), Lmax, verify=True).cpu().numpy()
    oracle = orc.forward(weights, orc.EncoderConfig(**kw), z["ids"], bf16_storage=True, ln_fold=fold, residual_f32=res32)

    def dist(got, ref):
        cos = (got * ref).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(ref, axis=1))
        return cos.min(), (np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)).max()
    (ca, ra), (cb, rb) = LONG_TOL
    for what, got in (("padded", padded), ("packed", packed)):
        cos_a, rel_a = dist(got, oracle)
        cos_b, rel_b = dist(got, z["sent"])
        print(f"long encoder {what} [{form}] vs bf16-storage oracle: cos {cos_a:.6f} rel {rel_a:.5f}; vs HF fp32: cos {cos_b:.6f} rel {rel_b:.5f}")
        assert cos_a >= ca and rel_a <= ra, (what, cos_a, rel_a)
        assert cos_b >= cb and rel_b <= rb, (what, cos_b, rel_b)
    assert np.array_equal(padded, packed)


def test_provider_embeds_the_whole_chunk_at_max_length_1023(gpu):
    import asyncio
    _env()
    from coderag_amd.encoder import wrap_encoder_only
    from coderag_amd.providers import HipUniXcoderProvider, ProviderConfig
    extra = {"synthetic_weights": 3, "num_layers": 2}
    by_arg = HipUniXcoderProvider(ProviderConfig(provider="unixcoder-hip", model="synthetic", extra=dict(extra)), max_length=1023)
    by_extra = HipUniXcoderProvider(ProviderConfig(provider="unixcoder-hip", model="synthetic", extra=dict(extra, max_length=1023)))
    short = HipUniXcoderProvider(ProviderConfig(provider="unixcoder-hip", model="synthetic", extra=dict(extra)))
    model = by_arg._load()
    tok = model.tok
    text = "\n".join(f"def f{i}(a{i}, b{i}): return a{i} * {i} + b{i}" for i in range(54))
    assert 1400 <= len(tok.encode_body(text)) <= 1600, len(tok.encode_body(text))
    words = [f"v{i}" for i in range(210)]
    a = " ".join(words + [f"x{i}" for i in range(300)])                 # the two share their first 600 tokens and no more
    b = " ".join(words + [f"y{i}" for i in range(300)])
    assert tok.encode_body(a)[:600] == tok.encode_body(b)[:600] and tok.encode_body(a)[:1019] != tok.encode_body(b)[:1019]

    async def go(p):
        return await p.embed(text), await p.embed_batch([a, b])
    one, (va, vb) = asyncio.run(go(by_arg))
    one_x, (va_x, vb_x) = asyncio.run(go(by_extra))
    _, (sa, sb) = asyncio.run(go(short))
    want = model.embed_ids([wrap_encoder_only(tok, text, 1023)]).cpu().numpy()[0]
    assert len(one) == 768 and np.array_equal(np.asarray(one, np.float32), want)
    assert one == one_x and va == va_x and vb == vb_x
    assert va != vb and not np.allclose(va, vb, atol=1e-4)              # the tail past token 512 is really used
    assert sa == sb                                                      # ... and cut at 512
