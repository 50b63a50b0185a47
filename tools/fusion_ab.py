"""What does multi-query fusion (RRF / best match) add to the plain 64-query step it starts from, and what does
the host alternative cost?  (profiles/fused.md.)

    python tools/fusion_ab.py [--rows 10000000] [--out FILE.json]

A bf16 index of random unit rows, dim 768; 16 logical queries x 4 sub-queries = one 64-query batch (a sub-query is its logical
query plus noise of a quarter of its norm, so the four lists of a question overlap and differ), limit 10 / candidates 40,
device queries and device outputs.

* plain:  crh_search + crh_search_finish for the 64 queries at k = 40 -- what the parent commit runs for the same fetch
* fused:  the same search + crh_fuse_select (rrf, and max)
  Both under a host clock around work that ends in a synchronise, one step of each alternating, after a warm-up.
* select: crh_fuse_select alone, between device events
* host:   the alternative the launch replaces -- copy the 64 x 40 scores and rows to the host and fuse them with the numpy
  restatement of the definition (tests/fuse_cases.py: np.unique plus one vector step per list, written to be read, not tuned;
  no payload is looked up).  Its rows must equal the device's: the tool fails otherwise.

(The issue that asked for this tool called it tools/fused_ab.py; that name belongs to the one-launch-scan A/B.)

Every timing: median, p10, p90 over the steps (ms per batch of 16 logical queries).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NQ, M, LIMIT, CAND = 16, 4, 10, 40


def summary(ms):
    return {"ms_median": round(float(np.median(ms)), 4), "ms_p10": round(float(np.percentile(ms, 10)), 4),
            "ms_p90": round(float(np.percentile(ms, 90)), 4), "steps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from tests import fuse_cases
    g = torch.Generator(device="cuda").manual_seed(a.rows)
    idx = ffi.Index(a.dim, ffi.DTYPE_BF16, capacity_rows=a.rows, device=0)
    for first in range(0, a.rows, 1 << 20):
        idx.append(torch.randn((min(1 << 20, a.rows - first), a.dim), generator=g, device="cuda"))
        torch.cuda.synchronize()
    base = torch.randn((NQ, 1, a.dim), generator=g, device="cuda")
    q = (base + 0.25 * torch.randn((NQ, M, a.dim), generator=g, device="cuda")).reshape(NQ * M, a.dim).contiguous()
    cs = torch.empty((NQ * M, CAND), dtype=torch.float32, device="cuda")
    cr = torch.empty((NQ * M, CAND), dtype=torch.int64, device="cuda")
    results = []

    def emit(row):
        results.append(row)
        print(json.dumps(row), flush=True)

    def search():
        idx.search(q, CAND, out_scores=cs, out_rows=cr)
        idx.search_finish()

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for method in ("rrf", "max"):
        def fused():
            search()
            return ffi.fuse_select(cs, cr, M, LIMIT, method)
        for _ in range(a.warmup):
            timed(search)
            timed(fused)
        plain_ms, fused_ms = [], []
        for _ in range(a.steps):
            plain_ms.append(timed(search))
            fused_ms.append(timed(fused))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        alone = []
        for _ in range(a.steps):
            ev[0].record()
            out = ffi.fuse_select(cs, cr, M, LIMIT, method)
            ev[1].record()
            torch.cuda.synchronize()
            alone.append(ev[0].elapsed_time(ev[1]))
        dev_rows = out[0].cpu().numpy()
        overlap = float(np.mean(out[5].cpu().numpy()[:, 0])) / (M * CAND)
        host = []
        for _ in range(a.host_steps):
            t0 = time.perf_counter()
            hs, hr = cs.cpu().numpy(), cr.cpu().numpy()
            want = fuse_cases.fuse_select(hs, hr, M, LIMIT, method)
            host.append((time.perf_counter() - t0) * 1e3)
        if not np.array_equal(want[0], dev_rows):
            raise SystemExit(f"{method}: the host restatement and the device disagree on the fused rows")
        emit({"rows": a.rows, "dim": a.dim, "logical": NQ, "sub_queries": M, "limit": LIMIT, "candidates": CAND, "method": method,
              "plain": summary(plain_ms), "fused": summary(fused_ms), "added_ms_median": round(float(np.median(fused_ms) - np.median(plain_ms)), 4),
              "select_events": summary(alone), "host_copy_and_numpy": summary(host), "host_equals_device": bool(np.array_equal(want[0], dev_rows)),
              "distinct_share_of_entries": round(overlap, 3)})
    idx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
