"""The f32 store's 64-query top-100 batch by nomination mode, one process per library (profiles/f32_margin.md).

    CODERAG_HIP_LIB=/path/to/other/libcoderag_hip.so python tools/f32_margin_ab.py 10000000 parent
    python tools/f32_margin_ab.py 10000000 fixed

Builds an f32-store index of ROWS Gaussian rows on the device (seeded: every process sees the same corpus and queries), then for
the int8-copy nomination, the one-launch bf16-tile scan and its three-launch form: warm-up, 4 x 30 batches, wall time around a
synchronise per 30.  Prints one line "AB {json}": ms per batch of each repetition, the candidates the last batch nominated, and
a hash of its rows and score bits (equal across libraries when the results are).  Run the two libraries alternately."""
import hashlib
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import coderag_amd  # noqa: F401,E402
from coderag_amd import ffi  # noqa: E402

N, tag = int(sys.argv[1]), sys.argv[2]
D, B, K, STEPS, REPS = 768, 64, 100, 30, 4
dev = torch.device("cuda:0")
gen = torch.Generator(device=dev)
gen.manual_seed(20251226)
idx = ffi.Index(D, ffi.DTYPE_F32, capacity_rows=N)
chunk = 500_000
for a in range(0, N, chunk):
    idx.append(torch.randn((min(chunk, N - a), D), generator=gen, device=dev))
torch.cuda.synchronize()
qd = torch.randn((B, D), generator=gen, device=dev)
out_s = torch.empty((B, K), dtype=torch.float32, device=dev)
out_r = torch.empty((B, K), dtype=torch.int64, device=dev)


def run(n):
    for _ in range(n):
        idx.search(qd, K, out_scores=out_s, out_rows=out_r)
    idx.search_finish()
    torch.cuda.synchronize()


res = {"lib": tag, "rows": N}
for name, mode in (("int8_copy", ffi.NOMINATE_INT8), ("bf16_one_launch", ffi.NOMINATE_BF16), ("bf16_three_launches", ffi.NOMINATE_BF16_3)):
    idx.set_nomination(mode)
    run(5)
    t = time.perf_counter()
    while time.perf_counter() - t < 0.1:
        run(4)
    ms = []
    for _ in range(REPS):
        t = time.perf_counter()
        run(STEPS)
        ms.append((time.perf_counter() - t) * 1e3 / STEPS)
    run(1)
    st = idx.stats()
    res[name] = {"ms_per_batch": [round(m, 4) for m in ms], "nomination": idx.nomination(), "candidates": st["candidates"],
                 "max_query_cands": st["max_query_cands"], "fallback_used": st["fallback_used"],
                 "rows_sha": hashlib.sha1(out_r.cpu().numpy().tobytes() + out_s.cpu().numpy().tobytes()).hexdigest()[:12]}
idx.close()
print("AB " + json.dumps(res), flush=True)
