"""One classed pass for a mixed-filter batch against one pass per filter (the table is profiles/multi_filter.md).

    python tools/multi_filter_ab.py --rows 1000000 10000000 [--out FILE.json]

64 queries, top-100, bf16 store, one index per size.  Cases: F in {2, 4, 8} equal-share classes on an INTERLEAVED column (every
tile holds every class: a dense union), and F = 8 CONTIGUOUS 1/64 slices (a sparse union: 1/8 of the tiles).  Per case two ways
of answering the same 64 queries, query i under class i mod F:

  multi      ONE crh_search_multi call (the classed three-launch bf16 scan)
  per-class  what the library did before: one crh_search_cond per class over that class's 64 / F queries

Both run in the same process on the same index, in alternating blocks; every block is `iters` repetitions between two device
events on the search stream (device outputs, crh_search_finish after the second event is recorded and synchronised).  Per
case and way: median ms per 64-query batch over the blocks, their min..max (the run-to-run spread), crh_search_stats.tiles of
one batch, and whether both ways return the same ids and score bits.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1000000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    nq, k = 64, 100
    stream = torch.cuda.current_stream().cuda_stream
    results = []
    for rows in a.rows:
        idx = ffi.Index(a.dim, ffi.DTYPE_BF16, capacity_rows=rows, n_code_cols=2)
        g = torch.Generator(device="cuda").manual_seed(rows)
        for first in range(0, rows, 1 << 20):
            n = min(1 << 20, rows - first)
            x = torch.randn((n, a.dim), generator=g, device="cuda", dtype=torch.float32)
            r = np.arange(first, first + n)
            codes = np.stack([r % 8, r * 64 // rows], axis=1).astype(np.int32)      # column 0 interleaved, column 1 contiguous 1/64 slices
            idx.append(x, torch.from_numpy(codes).cuda())
            torch.cuda.synchronize()
        q = torch.randn((nq, a.dim), generator=torch.Generator(device="cuda").manual_seed(1), device="cuda")
        cases = [(f"interleaved F={f}", [[(0, list(range(c * 8 // f, (c + 1) * 8 // f)), False)] for c in range(f)]) for f in (2, 4, 8)]
        cases.append(("contiguous 1/64 slices F=8", [[(1, 5 + 7 * c)] for c in range(8)]))
        for name, classes in cases:
            f = len(classes)
            qc = (np.arange(nq) % f).astype(np.int32)
            order = np.argsort(qc, kind="stable")
            qsorted = q[torch.as_tensor(order, device="cuda")].contiguous()          # per-class: each class's queries contiguous
            per = nq // f
            out = {w: (torch.empty((nq, k), dtype=torch.float32, device="cuda"), torch.empty((nq, k), dtype=torch.int64, device="cuda"))
                   for w in ("multi", "per-class")}

            def multi():
                idx.search_multi(q, k, classes, qc, out_scores=out["multi"][0], out_rows=out["multi"][1], stream=stream)

            def per_class():
                for c in range(f):
                    s = slice(c * per, (c + 1) * per)
                    idx.search(qsorted[s], k, filters=classes[c], out_scores=out["per-class"][0][s], out_rows=out["per-class"][1][s], stream=stream)

            ways = {"multi": multi, "per-class": per_class}
            info = {}
            for w, fn in ways.items():                           # warm-up, the results and the stats of one batch
                for _ in range(3):
                    fn()
                    idx.search_finish(stream)
                st = idx.stats()
                info[w] = {"tiles_last_call": st["tiles"], "fallback_used": st["fallback_used"]}
            torch.cuda.synchronize()
            ms, mr = out["multi"][0].cpu().numpy().view(np.uint32), out["multi"][1].cpu().numpy()
            ps, pr = out["per-class"][0].cpu().numpy().view(np.uint32), out["per-class"][1].cpu().numpy()
            same = bool(np.array_equal(ms[order], ps) and np.array_equal(mr[order], pr))
            times = {w: [] for w in ways}
            for _ in range(a.blocks):                            # alternating blocks
                for w, fn in ways.items():
                    fn()
                    idx.search_finish(stream)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        fn()
                    e1.record()
                    e1.synchronize()
                    idx.search_finish(stream)
                    times[w].append(e0.elapsed_time(e1) / a.iters)
            for w in ways:
                row = {"rows": rows, "case": name, "way": w, "ms_median": round(statistics.median(times[w]), 4), "ms_min": round(min(times[w]), 4),
                       "ms_max": round(max(times[w]), 4), "same_bits": same, **info[w]}
                results.append(row)
                print(json.dumps(row), flush=True)
        idx.close()
        del idx
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
