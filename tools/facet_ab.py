"""What does a facet cost (crh_index_facet, crh_search_range_facet, crh_facet_select), and what does the host
route it replaces cost?  (profiles/facet.md.)

    python tools/facet_ab.py [--rows 1000000,10000000] [--out FILE.json]

Per row count one bf16 index of random rows, dim 384, with three code columns: a LANGUAGE column of 10 values (random), a FILE
column of rows / 10 values (ten consecutive rows per file, as chunks of a file are stored) and a column row % 64 to filter on.
Legs, each the median / p10 / p90 of --steps launches between device events after a warm-up:

  lang, file            the histogram of the column, unfiltered: the LDS route, the run route
  lang/64, file/64      the same under an equality filter that keeps 1 row in 64 (the mask is in the index's cache)
  lang/words, file/words  the same under a row bitmap that keeps about 1 row in 100 (what a `contains` filter hands over)
  select                crh_facet_select, k = 10, on the file histogram
  host lang, host file  the route the parent commit offers: match_rows of everything + numpy.bincount over the host's code column
                        (host clock)
  count, facet          64 queries at a threshold that admits about 1 row in 1000: crh_search_range with counts (k = 1) -- what
                        count_similar runs -- and crh_search_range_facet over the file column with the same arguments
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIM, NQ = 384, 64


def summary(ms):
    return {"ms_median": round(float(np.median(ms)), 4), "ms_p10": round(float(np.percentile(ms, 10)), 4),
            "ms_p90": round(float(np.percentile(ms, 90)), 4), "steps": len(ms)}


def run(rows, a, emit):
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    g = torch.Generator(device="cuda").manual_seed(rows)
    idx = ffi.Index(DIM, ffi.DTYPE_BF16, capacity_rows=rows, n_code_cols=3, device=0)
    host_codes = []
    for first in range(0, rows, 1 << 20):
        m = min(1 << 20, rows - first)
        r = torch.arange(first, first + m, device="cuda")
        codes = torch.stack([torch.randint(0, 10, (m,), generator=g, device="cuda"), r // 10, r % 64], 1).to(torch.int32).contiguous()
        idx.append(torch.randn((m, DIM), generator=g, device="cuda"), codes)
        host_codes.append(codes.cpu().numpy())
        torch.cuda.synchronize()
    host_codes = np.concatenate(host_codes)
    n_files = (rows + 9) // 10
    q = torch.randn((NQ, DIM), generator=g, device="cuda")
    words = (torch.rand(((rows + 31) // 32, 32), generator=g, device="cuda") < 0.01).to(torch.int64)
    words = (words << torch.arange(32, device="cuda")).sum(1).to(torch.int32).contiguous()            # (bit 31 wraps into the sign: the words are bits)
    bitmap = [ffi.RowWords(ffi.next_words_tag(), words)]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    def leg(name, fn, **more):
        for _ in range(a.warmup):
            timed(fn)
        emit({"rows": rows, "leg": name, **summary([timed(fn) for _ in range(a.steps)]), **more})
    outs = {0: (torch.empty((10,), dtype=torch.int64, device="cuda"), torch.empty((3,), dtype=torch.int64, device="cuda")),
            1: (torch.empty((n_files,), dtype=torch.int64, device="cuda"), torch.empty((3,), dtype=torch.int64, device="cuda"))}
    for col, name, n_bins in ((0, "lang", 10), (1, "file", n_files)):
        for suffix, filt in (("", None), ("/64", [(2, 5)]), ("/words", bitmap)):
            leg(name + suffix, lambda: idx.facet(col, n_bins, filters=filt, out=outs[col]), counted=int(idx.facet(col, n_bins, filters=filt)[1][0].item()),
                route="lds" if n_bins <= ffi.FACET_LDS_BINS else "runs")
    idx.facet(1, n_files, out=outs[1])
    leg("select", lambda: ffi.facet_select(outs[1][0], 10))
    assert np.array_equal(outs[1][0].cpu().numpy(), np.bincount(host_codes[:, 1], minlength=n_files))
    for col, name, n_bins in ((0, "host lang", 10), (1, "host file", n_files)):
        host = []
        for _ in range(a.host_steps):
            t0 = time.perf_counter()
            got = np.bincount(host_codes[idx.match_rows(None, rows), col], minlength=n_bins)
            host.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(got, idx.facet(col, n_bins)[0].cpu().numpy())
        emit({"rows": rows, "leg": name, **summary(host), "clock": "host"})
    thr = np.full((NQ,), 3.09 / np.sqrt(DIM), np.float32)                                           # random rows: about 1 in 1000 scores above
    os_, or_ = torch.empty((NQ, 1), dtype=torch.float32, device="cuda"), torch.empty((NQ, 1), dtype=torch.int64, device="cuda")
    oc = torch.empty((NQ,), dtype=torch.int64, device="cuda")
    sem = (torch.empty((NQ, n_files), dtype=torch.int64, device="cuda"), torch.empty((NQ, 3), dtype=torch.int64, device="cuda"))

    def count():
        idx.search_range(q, 1, thr, out_scores=os_, out_rows=or_, out_counts=oc)
        idx.search_finish()
    leg("count", count)
    leg("facet", lambda: idx.search_range_facet(q, thr, 1, n_files, out=sem))
    assert np.array_equal(sem[1][:, 0].cpu().numpy(), oc.cpu().numpy()) and np.array_equal(sem[0].sum(1).cpu().numpy(), oc.cpu().numpy())
    emit({"rows": rows, "leg": "in range per query", "median": int(oc.median().item()), "max": int(oc.max().item())})
    idx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,10000000")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    results = []

    def emit(row):
        results.append(row)
        print(json.dumps(row), flush=True)
    for rows in (int(r) for r in a.rows.split(",")):
        run(rows, a, emit)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
