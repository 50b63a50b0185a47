"""What does a keyword batch (crh_lex_search) and a hybrid batch cost beside the plain dense search of the same
batch?  (profiles/lexical.md.)

    python tools/lexical_ab.py [--rows 1000000] [--out FILE.json]

One bf16 index of random rows, dim 768, and a forward index beside it: every row draws 130 tokens from a 50 000-word vocabulary
with Zipf weights (about 100 distinct terms a row, dl = 130).  One batch of 64 queries of 3 mid-frequency terms each, device
outputs.  Legs, timed in interleaved blocks between device events after a warm-up of every leg (a lexical call waits on its
stream once per pass, so its event time includes those host gaps: it is what a caller sees):

  a  dense     crh_search + crh_search_finish at k = 10
  b  lexical   crh_lex_search at k = 10 under the alive words (crh_index_row_mask)
  c  hybrid    limit 10 / candidates 40: the dense search at k = 40, crh_index_row_mask + crh_lex_search at k = 40, the two lists
               stacked [nq, 2, 40], crh_fuse_select (m = 2, rrf) at k = 10
  s  stats     crh_lex_stats of the batch's terms under the alive words (host clock; synchronous): ONE walk over the index

A lexical call is two scoring walks over the forward index (histogram, append) plus the cut, the select and a 16 MB memset; the
tool reports the index's bytes over HALF the lexical batch's time as a lower bound of one walk's rate, and over the stats
walk's time, against the 8 TB/s peak.  The tool fails if leg b's rows differ from the restatement on a 20 000-row prefix.
Every timing: median, p10, p90 (ms per batch).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NQ, K, C, DIM, VOCAB, TOKENS = 64, 10, 40, 768, 50_000, 130


def summary(ms):
    return {"ms_median": round(float(np.median(ms)), 4), "ms_p10": round(float(np.percentile(ms, 10)), 4),
            "ms_p90": round(float(np.percentile(ms, 90)), 4), "steps": len(ms)}


def rows_csr(rng, n, cdf, ids):
    """n rows of TOKENS Zipf draws: (row_off, terms, tf, dl), vectorised (sort each row, run lengths of equal neighbours)."""
    draw = np.sort(ids[np.searchsorted(cdf, rng.random((n, TOKENS)))], axis=1)
    first = np.ones((n, TOKENS), bool)
    first[:, 1:] = draw[:, 1:] != draw[:, :-1]
    at = np.flatnonzero(first.ravel())
    tf = np.diff(np.append(at, n * TOKENS)).astype(np.uint8)          # (a row starts a run: no run crosses rows)
    off = np.concatenate([[0], np.cumsum(first.sum(1))]).astype(np.int64)
    return off, draw.ravel()[at].astype(np.uint32), tf, np.full(n, TOKENS, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10, help="timed steps per leg and block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi, lexical
    from tests import lex_cases
    results = []

    def emit(row):
        results.append(row)
        print(json.dumps(row), flush=True)

    rng = np.random.default_rng(a.rows)
    ids = np.sort(rng.choice(1 << 32, VOCAB, replace=False).astype(np.uint32))
    rng.shuffle(ids)                                                    # (rank and id unrelated)
    w = 1.0 / np.arange(1, VOCAB + 1)
    cdf = np.cumsum(w / w.sum())
    cdf[-1] = 1.0
    g = torch.Generator(device="cuda").manual_seed(a.rows)
    idx = ffi.Index(DIM, ffi.DTYPE_BF16, capacity_rows=a.rows, device=0)
    lex = ffi.Lex(capacity_rows=a.rows, device=0)
    prefix = None
    for first in range(0, a.rows, 1 << 18):
        n = min(1 << 18, a.rows - first)
        idx.append(torch.randn((n, DIM), generator=g, device="cuda"))
        part = rows_csr(rng, n, cdf, ids)
        if prefix is None:
            m = min(n, 20_000)
            prefix = (part[0][: m + 1], part[1][: part[0][m]], part[2][: part[0][m]], part[3][:m])
        lex.append(*part)
        torch.cuda.synchronize()
    rows, entries = lex.count()
    index_bytes = entries * 5 + rows * 12
    q = torch.randn((NQ, DIM), generator=g, device="cuda")
    queries = [np.sort(ids[rng.choice(np.arange(200, 5000), 3, replace=False)]) for _ in range(NQ)]
    every = np.unique(np.concatenate(queries))
    alive = idx.row_mask(None)
    torch.cuda.synchronize()
    df, n_rows, sum_dl = lex.stats(every, alive)
    wts, avgdl = lexical.bm25_weights(df, n_rows, sum_dl)
    table = dict(zip(every.tolist(), wts))
    idf = [np.asarray([table[int(t)] for t in one], np.float32) for one in queries]
    emit({"leg": "setup", "rows": rows, "entries": entries, "entries_per_row": round(entries / rows, 1), "index_mb": round(index_bytes / 2**20, 1),
          "avgdl": float(avgdl), "df_min": int(df.min()), "df_max": int(df.max())})

    # parity on the prefix before anything is timed
    small = ffi.Lex(capacity_rows=len(prefix[3]), device=0)
    small.append(*prefix)
    got = [t.cpu().numpy() for t in small.search(queries, idf, K, 1.2, 0.75, float(avgdl))]
    want = lex_cases.bm25_search(*prefix, None, queries, idf, 1.2, 0.75, avgdl, K)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[2], want[2]), \
        "crh_lex_search differs from the restatement"
    small.close()

    dev = "cuda:0"
    s10, r10 = torch.empty((NQ, K), dtype=torch.float32, device=dev), torch.empty((NQ, K), dtype=torch.int64, device=dev)
    s40, r40 = torch.empty((NQ, 2, C), dtype=torch.float32, device=dev), torch.empty((NQ, 2, C), dtype=torch.int64, device=dev)
    ds, dr = torch.empty((NQ, C), dtype=torch.float32, device=dev), torch.empty((NQ, C), dtype=torch.int64, device=dev)
    ls, lr = torch.empty((NQ, C), dtype=torch.float32, device=dev), torch.empty((NQ, C), dtype=torch.int64, device=dev)
    cnt = torch.empty((NQ,), dtype=torch.int64, device=dev)
    mask = torch.empty_like(alive)

    def dense():
        idx.search(q, K, out_scores=s10, out_rows=r10)
        idx.search_finish()

    def lexical_leg():
        idx.row_mask(None, out=mask)
        lex.search(queries, idf, K, 1.2, 0.75, float(avgdl), mask=mask, out_scores=s10, out_rows=r10, out_count=cnt)

    def hybrid():
        idx.search(q, C, out_scores=ds, out_rows=dr)
        idx.search_finish()
        idx.row_mask(None, out=mask)
        lex.search(queries, idf, C, 1.2, 0.75, float(avgdl), mask=mask, out_scores=ls, out_rows=lr, out_count=cnt)
        s40[:, 0], s40[:, 1], r40[:, 0], r40[:, 1] = ds, ls, dr, lr
        ffi.fuse_select(s40, r40, 2, K, "rrf", 60, None)

    legs = {"dense": dense, "lexical": lexical_leg, "hybrid": hybrid}
    for fn in legs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(a.blocks):
        for name, fn in legs.items():
            for _ in range(a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
    for name in legs:
        emit(dict(leg=name, **summary(times[name])))
    host = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        lex.stats(every, alive)
        host.append((time.perf_counter() - t0) * 1e3)
    emit(dict(leg="stats", **summary(host)))
    lex_ms, stats_ms, dense_ms, hyb_ms = (float(np.median(v)) for v in (times["lexical"], host, times["dense"], times["hybrid"]))
    emit({"leg": "rates", "qualifying_rows_median": int(np.median(cnt.cpu().numpy())),
          "walk_gbps_lower_bound_from_half_a_lexical_batch": round(index_bytes / (lex_ms / 2 * 1e-3) / 1e9, 1),
          "walk_gbps_from_the_stats_walk": round(index_bytes / (stats_ms * 1e-3) / 1e9, 1), "peak_gbps": 8000,
          "hybrid_over_dense": round(hyb_ms / dense_ms, 2), "lexical_over_dense": round(lex_ms / dense_ms, 2)})
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
