#!/usr/bin/env python3
"""Times the LayerNorm-folded GEMM entries (epilogues 3, 4 and 5 of the tiled kernels) on the encoder's shapes, as
tools/gemm_bench.py times epilogues 0-2: `lnin0` = crh_gemm_bf16_lnin act 0 on the QKV shape, `lnin1` = the same with act 1 on
FFN1, `res5` = crh_gemm_bf16_res_lnstats with residual statistics on the O-projection and FFN2.  Random data; per entry ROUNDS
rounds of 3 + 20 calls between device events, median / min / quartiles of the rounds.  Which kernel runs is the cost model's
choice (k_gemm_mid at T = 300 and 2048, the ping-pong kernel at 65536).  To compare two builds, alternate processes with
CODERAG_HIP_LIB pointing at each library.

    python tools/gemm_epi_bench.py [T,T,...] [lnin0,lnin1,res5] [ROUNDS]          (default: 300,2048,65536  all three  5)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import coderag_amd
from coderag_amd import ffi
TS = tuple(int(t) for t in sys.argv[1].split(",")) if len(sys.argv) > 1 else (300, 2048, 65536)
KINDS = sys.argv[2].split(",") if len(sys.argv) > 2 else ["lnin0", "lnin1", "res5"]
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev = torch.device("cuda:0")
L = ffi.lib()
g = torch.Generator(device="cpu").manual_seed(1)
for T in TS:
    for name, N, K, kind in (("qkv", 2304, 768, "lnin0"), ("ffn1", 3072, 768, "lnin1"), ("oproj", 768, 768, "res5"), ("ffn2", 768, 3072, "res5")):
        if kind not in KINDS:
            continue
        a = torch.randn((T, K), generator=g).to(dev, torch.bfloat16)
        w = (torch.randn((N, K), generator=g) / K ** 0.5).to(dev, torch.bfloat16)
        b = torch.randn((N,), generator=g).to(dev)
        col = torch.randn((N,), generator=g).to(dev)
        y = torch.empty((T, N), dtype=torch.bfloat16, device=dev)
        rst = torch.stack([torch.rand((T,), generator=g) + 0.5, torch.randn((T,), generator=g)], 1).contiguous().to(dev)
        res = torch.randn((T, 768), generator=g).to(dev, torch.bfloat16)
        gam = torch.ones((768,), device=dev)
        part = torch.empty((T, 24, 2), device=dev)
        so = torch.empty((T, 2), device=dev)
        def call():
            if kind == "res5":
                ffi.check(L.crh_gemm_bf16_res_lnstats(a.data_ptr(), w.data_ptr(), b.data_ptr(), res.data_ptr(), rst.data_ptr(), gam.data_ptr(), 1e-5,
                                                      y.data_ptr(), part.data_ptr(), so.data_ptr(), T, N, K, 0))
            else:
                ffi.check(L.crh_gemm_bf16_lnin(a.data_ptr(), rst.data_ptr(), w.data_ptr(), col.data_ptr(), b.data_ptr(), y.data_ptr(), T, N, K, int(kind == "lnin1"), 0))
        ts = []
        for rnd in range(ROUNDS):
            for _ in range(3):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                call()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 20 * 1e3)
        print(f"{name:6s} T={T} N={N} K={K} entry {kind}: median {float(np.median(ts)):7.2f} us  min {min(ts):7.1f}  "
              f"p25 {float(np.percentile(ts, 25)):7.2f} p75 {float(np.percentile(ts, 75)):7.2f}", flush=True)
