"""What does the overlap-free top-k (max_overlap; crh_span_select) cost beside the plain 64-query step, what does
the host alternative cost, and what does the mask of a range condition cost beside that of a one-value set?  (profiles/spans.md.)

    python tools/span_ab.py [--rows 10000000] [--out FILE.json]

One bf16 index of random rows, dim 768, with three code columns: a file (row % files), a first line and a last line -- the
spans of one file overlap their neighbours by two thirds, so the walk has something to drop.  One batch of 64 queries, limit 10,
candidates 40, device queries and device outputs.  Legs, timed in interleaved blocks (block 0 of every leg, then block 1 of every
leg, ...) between device events, after a warm-up of every leg:

  a  plain      crh_search + crh_search_finish at k = 10
  a40 plain-40  the same at k = 40: the candidate list the walk needs
  b  spans      k = 40 search, three crh_index_gather_codes into one buffer full of -1, crh_span_select at permille 500, k = 10
  c  host       the alternative: the k = 40 search with HOST outputs, the three columns looked up in host copies, the walk in
                Python (tests/span_cases.walk) -- host clock, it ends in a copy
  d  select     crh_span_select ALONE at c = 1024, k = 10, nq = 64 on lists of the corpus (b's search at k = 1024, not timed) and
                on 1024 pairwise disjoint spans of one file (the longest kept list: every candidate meets every earlier one)
  m  masks      crh_index_match_rows_cond (count only: mask + count, host clock) under one range condition and under a
                one-value set condition, bounds / values alternating so that no call finds its mask kept

The tool fails if leg b's rows differ from the Python walk over leg a40's list.  Every timing: median, p10, p90 (ms per batch).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NQ, K, C, DIM, PERMILLE = 64, 10, 40, 768, 500


def summary(ms):
    return {"ms_median": round(float(np.median(ms)), 4), "ms_p10": round(float(np.percentile(ms, 10)), 4),
            "ms_p90": round(float(np.percentile(ms, 90)), 4), "steps": len(ms)}


def columns(torch, first, n, files):
    """(file, lo, hi) int32 [n, 3] of the rows first .. first + n: 50-line spans every 17 lines inside each file."""
    r = torch.arange(first, first + n, device="cuda", dtype=torch.int64)
    lo = (r // files) * 17
    return torch.stack([(r % files).to(torch.int32), lo.to(torch.int32), (lo + 49).to(torch.int32)], dim=1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--files", type=int, default=20_000)
    ap.add_argument("--steps", type=int, default=20, help="timed steps per leg and block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from tests import span_cases
    results = []

    def emit(row):
        results.append(row)
        print(json.dumps(row), flush=True)

    g = torch.Generator(device="cuda").manual_seed(a.rows)
    idx = ffi.Index(DIM, ffi.DTYPE_BF16, capacity_rows=a.rows, n_code_cols=3, device=0)
    host_cols = []
    for first in range(0, a.rows, 1 << 20):
        n = min(1 << 20, a.rows - first)
        cols = columns(torch, first, n, a.files)
        idx.append(torch.randn((n, DIM), generator=g, device="cuda"), cols)
        host_cols.append(cols.cpu().numpy())
        torch.cuda.synchronize()
    host_cols = np.concatenate(host_cols)
    q = torch.randn((NQ, DIM), generator=g, device="cuda")

    def outs(k):
        return torch.empty((NQ, k), dtype=torch.float32, device="cuda"), torch.empty((NQ, k), dtype=torch.int64, device="cuda")
    s10, r10 = outs(K)
    s40, r40 = outs(C)
    s1k, r1k = outs(1024)
    codes = torch.empty((3, NQ, C), dtype=torch.int32, device="cuda")
    picked = {}

    def plain():
        idx.search(q, K, out_scores=s10, out_rows=r10)
        idx.search_finish()

    def plain40():
        idx.search(q, C, out_scores=s40, out_rows=r40)
        idx.search_finish()

    def spans():
        idx.search(q, C, out_scores=s40, out_rows=r40)
        idx.search_finish()
        codes.fill_(-1)
        for col in range(3):
            idx.gather_codes(r40, col, out=codes[col])
        picked["b"] = ffi.span_select(s40, r40, codes[0], codes[1], codes[2], K, PERMILLE)

    def timed_event(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    legs = {"a": plain, "a40": plain40, "b": spans}
    for fn in legs.values():
        for _ in range(a.warmup):
            timed_event(fn)
    ms = {name: [] for name in legs}
    for _ in range(a.blocks):
        for name, fn in legs.items():
            ms[name] += [timed_event(fn) for _ in range(a.steps)]
    spans()
    torch.cuda.synchronize()
    got_rows, info = picked["b"][1].cpu().numpy(), picked["b"][6].cpu().numpy()
    rows40 = r40.cpu().numpy()
    for qi in range(NQ):                                       # the device's selection is the Python walk over the same list
        real = rows40[qi][rows40[qi] >= 0]
        kept = span_cases.walk(*(host_cols[real, c] for c in range(3)), PERMILLE)
        want = real[kept][:K]
        if not np.array_equal(got_rows[qi][:want.size], want) or (got_rows[qi][want.size:] != -1).any():
            raise SystemExit(f"query {qi}: crh_span_select differs from the Python walk")
    for name in legs:
        emit({"leg": name, "rows": a.rows, "nomination": idx.nomination(), **summary(ms[name]),
              **({"kept_of_40_median": int(np.median(info[:, 0])), "queries_with_a_drop": int((info[:, 0] < info[:, 1]).sum())} if name == "b" else {})})

    # c: the host alternative
    qh = q.cpu().numpy()
    host = []
    for _ in range(a.host_steps):
        t0 = time.perf_counter()
        hs, hr = idx.search(qh, C)
        for qi in range(NQ):
            real = hr[qi][hr[qi] >= 0]
            kept = span_cases.walk(host_cols[real, 0], host_cols[real, 1], host_cols[real, 2], PERMILLE)[:K]
        host.append((time.perf_counter() - t0) * 1e3)
    emit({"leg": "c", **summary(host)})

    # d: crh_span_select alone at c = 1024
    idx.search(q, 1024, out_scores=s1k, out_rows=r1k)
    idx.search_finish()
    big = torch.full((3, NQ, 1024), -1, dtype=torch.int32, device="cuda")
    for col in range(3):
        idx.gather_codes(r1k, col, out=big[col])
    disjoint = torch.stack([torch.zeros((NQ, 1024), dtype=torch.int32, device="cuda"),
                            (torch.arange(1024, device="cuda", dtype=torch.int32) * 10).repeat(NQ, 1),
                            (torch.arange(1024, device="cuda", dtype=torch.int32) * 10 + 5).repeat(NQ, 1)]).contiguous()
    one_file = big.clone()
    one_file[0].fill_(0)                                       # every candidate in ONE file: the spans overlap as the corpus makes them
    for name, cols in (("d corpus lists", big), ("d one file", one_file), ("d 1024 disjoint spans", disjoint)):
        fn = lambda cols=cols: picked.__setitem__("d", ffi.span_select(s1k, r1k, cols[0], cols[1], cols[2], K, PERMILLE))   # noqa: E731
        for _ in range(a.warmup):
            timed_event(fn)
        t = [timed_event(fn) for _ in range(a.steps * a.blocks)]
        kept = picked["d"][6].cpu().numpy()[:, 0]
        emit({"leg": name, "c": 1024, "kept_median": int(np.median(kept)), **summary(t)})

    # m: the mask of a range condition against that of a one-value set condition
    for name, make in (("m range", lambda i: [(1, 17 * (i % 7), 17 * (i % 7) + 400, "between")]), ("m one-value set", lambda i: [(0, [i % 7], False)])):
        for i in range(a.warmup):
            idx.count_matching(make(i))
        t = []
        for i in range(a.steps * a.blocks):
            t0 = time.perf_counter()
            n = idx.count_matching(make(i))
            t.append((time.perf_counter() - t0) * 1e3)
        emit({"leg": name, "rows": a.rows, "matching_last": int(n), **summary(t)})
    idx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
