#!/usr/bin/env python3
"""Long-row attention (k_attn_long, rows of 513..1024 tokens) on ~65k tokens of equal-length packed rows, next to k_attn at
L = 512, counted as attn_bench_packed.py counts (4 B H L^2 64 FLOP); then chunks/s of embed_ids on a lognormal chunk mix
clipped at 1023 tokens against the same chunks truncated at 512.  python tools/attn_bench_long.py"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import coderag_amd
from coderag_amd import ffi
from coderag_amd import encoder as drv
dev = torch.device("cuda:0"); Lb = ffi.lib(); H = 12
for L in (512, 528, 640, 768, 1024):
    B = max(1, 65536 // L)
    T = B * L
    qkv = torch.randn((T, 3 * H * 64), device=dev).to(torch.bfloat16)
    out = torch.empty((T, H * 64), dtype=torch.bfloat16, device=dev)
    nw = (L + 63) // 64
    km = torch.zeros((B, nw), dtype=torch.int64)
    for w in range(nw):
        bits = min(64, max(0, L - 64 * w))
        km[:, w] = -1 if bits == 64 else (1 << bits) - 1
    km = km.to(dev)
    off = torch.arange(0, T + 1, L, dtype=torch.int32, device=dev)
    ts = []
    for rnd in range(5):
        for _ in range(3):
            ffi.check(Lb.crh_attn_fwd_packed(qkv.data_ptr(), off.data_ptr(), km.data_ptr(), out.data_ptr(), B, T, L, H, 0))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            ffi.check(Lb.crh_attn_fwd_packed(qkv.data_ptr(), off.data_ptr(), km.data_ptr(), out.data_ptr(), B, T, L, H, 0))
        e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 20 * 1e3)
    fl = 4.0 * B * H * L * L * 64
    med = float(np.median(ts))
    kern = "k_attn" if L <= 512 else "k_attn_long"
    print(f"attn packed {kern:11s} B={B:3d} L={L:4d} T={T}: median {med:7.1f} us  {fl / med / 1e6:6.0f} TFLOP/s", flush=True)

cfg = drv.EncoderConfig()
model = drv.HipUniXcoder(drv.synthetic_weights(cfg, 23), cfg, drv.HashTokenizer(cfg.vocab_size), 0)
rng = np.random.default_rng(1234)
n = 4000
lens = np.clip(np.round(np.exp(rng.normal(np.log(400), 0.8, n))), 8, 1023).astype(int)
ids = [[0, 6, 2] + rng.integers(16, cfg.vocab_size, int(m) - 4).tolist() + [2] for m in lens]
cut = [row[:511] + [2] if len(row) > 512 else row for row in ids]
for name, rows in (("max_length 1023", ids), ("max_length 512", cut)):
    model.embed_ids(rows); torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        model.embed_ids(rows); torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    tok = sum(len(r) for r in rows)
    med = float(np.median(ts))
    print(f"embed_ids {name}: {n} chunks, {tok / n:.0f} tokens/chunk (lognormal mean-400 mix, {int((lens > 512).sum())} chunks > 512): "
          f"{med * 1e3:7.1f} ms  {n / med:8.0f} chunks/s  {1e6 * med / n:6.1f} us/chunk", flush=True)
