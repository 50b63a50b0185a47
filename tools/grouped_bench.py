"""What does the per-group cap (group_by / group_size) cost on top of the plain search it starts from, and how often does the
first round settle the answer?  (profiles/grouped.md)

    python tools/grouped_bench.py --rows 1000000 10000000 [--out FILE.json]

Per row count, a bf16 index of CLUSTERED rows with one code column (the file of every row), batch 64, device queries and
device outputs.  A file is a unit centre plus unit-norm noise (rows of one file have cosine ~0.5 to each other, ~0 to the rest);
file sizes are log-normal (median 30 rows, a tail beyond 1024); a query is a stored row plus noise, so its best hits lie in
its own file -- the case the feature exists for.  For (limit, group_size, candidates) in (10, 3, 40) and (100, 3, 400):

* plain:   crh_search + crh_search_finish at k = candidates -- what the parent commit runs for the same fetch
* grouped: the same search + crh_index_gather_codes + crh_group_select (one round of the store's grouped search)
  Both under a host clock around work that ends in a synchronise, one step of each alternating, after a warm-up.
* gather / select alone, between device events
* host:    the alternative the device path replaces -- copy the candidates' scores and rows to the host, look every hit's file up in a
  Python list (the payload lookup, without building the payload) and walk the list with a dict of counters
* rounds:  the share of the 64 queries whose list is incomplete after round 1 (candidates) and still after round 2 (1024)

Every timing: median, p10, p90 over the steps (ms per batch of 64 queries).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((10, 3, 40), (100, 3, 400))


def summary(ms):
    return {"ms_median": round(float(np.median(ms)), 4), "ms_p10": round(float(np.percentile(ms, 10)), 4),
            "ms_p90": round(float(np.percentile(ms, 90)), 4), "steps": len(ms)}


def build(ffi, torch, rows, dim, seed):
    """The clustered index; returns (index, file of every row as a host int32 array, the queries on the device)."""
    rng = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < rows:
        sizes += np.clip(rng.lognormal(np.log(30.0), 1.5, 4096), 1, 3000).astype(np.int64).tolist()
    which = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)[:rows]
    which = which[rng.permutation(rows)]
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.randn((int(which.max()) + 1, dim), generator=g, device="cuda")
    centres /= centres.norm(dim=1, keepdim=True)
    idx = ffi.Index(dim, ffi.DTYPE_BF16, capacity_rows=rows, n_code_cols=1, device=0)
    qsrc = rng.choice(min(rows, 1 << 20), 64, replace=False)
    queries = None
    for first in range(0, rows, 1 << 20):
        n = min(1 << 20, rows - first)
        w = torch.from_numpy(which[first:first + n]).cuda()
        x = centres[w.long()] + torch.randn((n, dim), generator=g, device="cuda") / dim ** 0.5
        if first == 0:
            queries = (x[torch.from_numpy(qsrc).cuda()] + 0.3 * torch.randn((64, dim), generator=g, device="cuda") / dim ** 0.5).contiguous()
        idx.append(x, w.reshape(-1, 1).contiguous())
        torch.cuda.synchronize()
        del x, w
    return idx, which, queries


def host_walk(scores, rows, files, limit, cap):
    out = []
    for srow, rrow in zip(scores.tolist(), rows.tolist()):
        seen, one = {}, []
        for sc, r in zip(srow, rrow):
            if r < 0 or len(one) == limit:
                break
            f = files[r]
            n = seen.get(f, 0)
            if n < cap:
                seen[f] = n + 1
                one.append((r, sc))
        out.append(one)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1000000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    nq = 64
    results = []

    def emit(row):
        results.append(row)
        print(json.dumps(row), flush=True)

    for rows in a.rows:
        idx, which, q = build(ffi, torch, rows, a.dim, seed=rows)
        files = which.tolist()                                     # (the file of every row: the host's payload table, at its cheapest)

        def search(c, cs, cr):
            idx.search(q, c, out_scores=cs, out_rows=cr)
            idx.search_finish()

        for limit, cap, c in SHAPES:
            cs = torch.empty((nq, c), dtype=torch.float32, device="cuda")
            cr = torch.empty((nq, c), dtype=torch.int64, device="cuda")
            codes = torch.empty((nq, c), dtype=torch.int32, device="cuda")

            def grouped():
                search(c, cs, cr)
                codes.fill_(-1)
                idx.gather_codes(cr, 0, out=codes)
                return ffi.group_select(cs, cr, codes, limit, cap)

            for _ in range(a.warmup):
                search(c, cs, cr)
                grouped()
            torch.cuda.synchronize()
            tp, tg = [], []
            for _ in range(a.steps):                                   # one step of each, alternating
                t0 = time.perf_counter()
                search(c, cs, cr)
                torch.cuda.synchronize()
                tp.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                out = grouped()
                torch.cuda.synchronize()
                tg.append((time.perf_counter() - t0) * 1e3)
            base = {"rows": rows, "limit": limit, "group_size": cap, "candidates": c}
            emit({**base, "what": "plain search at k = candidates (host clock)", **summary(tp)})
            emit({**base, "what": "search + gather_codes + group_select (host clock)", **summary(tg)})
            te, ts = [], []
            for _ in range(a.steps):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ev[0].record()
                codes.fill_(-1)
                idx.gather_codes(cr, 0, out=codes)
                ev[1].record()
                ffi.group_select(cs, cr, codes, limit, cap)
                ev[2].record()
                torch.cuda.synchronize()
                te.append(ev[0].elapsed_time(ev[1]))
                ts.append(ev[1].elapsed_time(ev[2]))
            emit({**base, "what": "fill + gather_codes (device events)", **summary(te)})
            emit({**base, "what": "group_select (device events)", **summary(ts)})
            # the host alternative on the same lists
            th = []
            for _ in range(max(a.steps // 6, 5)):
                t0 = time.perf_counter()
                walked = host_walk(cs.cpu().numpy(), cr.cpu().numpy(), files, limit, cap)
                th.append((time.perf_counter() - t0) * 1e3)
            got_rows = out[1].cpu().numpy()
            agree = sum(int([r for r, _ in walked[qi]] == [int(r) for r in got_rows[qi] if r >= 0]) for qi in range(nq))
            emit({**base, "what": "host: copy the candidates, look the files up, walk (host clock)", **summary(th), "queries_with_the_device_rows": agree})
            # rounds: incomplete after round 1, and after a round at MAX_K candidates
            info1 = out[4].cpu().numpy()
            need2 = (info1[:, 0] < limit) & (info1[:, 1] >= c)
            ks = torch.empty((nq, ffi.MAX_K), dtype=torch.float32, device="cuda")
            kr = torch.empty((nq, ffi.MAX_K), dtype=torch.int64, device="cuda")
            search(ffi.MAX_K, ks, kr)
            info2 = ffi.group_select(ks, kr, idx.gather_codes(kr, 0), limit, cap)[4].cpu().numpy()
            need3 = need2 & (info2[:, 0] < limit) & (info2[:, 1] >= ffi.MAX_K)
            emit({**base, "what": "rounds", "queries": nq, "need_round_2": int(need2.sum()), "need_exclusion_rounds": int(need3.sum()),
                  "median_kept_in_round_1": float(np.median(info1[:, 0]))})
        idx.close()
        del idx
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
