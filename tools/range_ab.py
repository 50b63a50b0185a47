"""What do a score threshold and an exact in-range count cost beside the plain 64-query step (crh_search_range),
and what does the host alternative cost -- and get wrong?  (profiles/range.md.)

    python tools/range_ab.py [--rows 1000000] [--parent-lib PATH/libcoderag_hip.so] [--out FILE.json]

One bf16 index of random unit rows, dim 768; one batch of 64 queries, k = 10, device queries and device outputs.  Legs, timed in
interleaved blocks (block 0 of every leg, then block 1 of every leg, ...) between device events, after a warm-up of every leg:

  a  plain      crh_search + crh_search_finish at k = 10 (the library's default nomination at this size)
  a3 plain-3    the same with nomination held at the three-launch bf16 scan: the form every range batch takes
  b  list@10    list-only range, each query's threshold one ulp below its 10th score (nothing is cut; tau barely moves)
  c  list@1000  list-only range at each query's 1000th score (the list is the plain one; the threshold costs nothing extra)
  d2/d4/d5      count mode at thresholds that admit about 1e2 / 1e4 / 1e5 rows per query (each query's own 100th / 10 000th /
                100 000th score, found by bisection on the device's exact counts before anything is timed)
  e  host       the alternative: crh_search at k = 1024 with host outputs + numpy `scores >= thr` (host clock, it ends in a copy);
                its count is clipped at 1024: the tool records at which of d2/d4/d5 it is wrong, and by how much

--parent-lib: the parent commit's library.  Leg a is then ALSO timed on it, in fresh child processes that alternate with children
on this tree's library (parent, this, parent, this; same process order, same seed), so "plain search is no slower" is a
comparison of two libraries under the same conditions, not of two runs an hour apart.  The children call the C ABI through
plain ctypes -- the entry points both libraries export -- because this tree's binding refuses a library without the new one.

Every timing: median, p10, p90 over the steps (ms per batch of 64 queries).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NQ, K, DIM = 64, 10, 768


def summary(ms):
    return {"ms_median": round(float(np.median(ms)), 4), "ms_p10": round(float(np.percentile(ms, 10)), 4),
            "ms_p90": round(float(np.percentile(ms, 90)), 4), "steps": len(ms)}


def build(a):
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    g = torch.Generator(device="cuda").manual_seed(a.rows)
    idx = ffi.Index(DIM, ffi.DTYPE_BF16, capacity_rows=a.rows, device=0)
    for first in range(0, a.rows, 1 << 20):
        idx.append(torch.randn((min(1 << 20, a.rows - first), DIM), generator=g, device="cuda"))
        torch.cuda.synchronize()
    q = torch.randn((NQ, DIM), generator=g, device="cuda")
    return torch, ffi, idx, q


def event_timer(torch):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])
    return timed


def plain_only(a):
    """Leg a alone on the library CODERAG_HIP_LIB names, through plain ctypes: prints one JSON line."""
    import ctypes as C
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    ffi._preload_hip_runtime()
    L = C.CDLL(os.environ["CODERAG_HIP_LIB"])
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    L.crh_index_create.argtypes = [i32, i32, i64, i32, i32, C.POINTER(vp)]
    L.crh_index_append.argtypes = [vp, i64, vp, i32, vp, vp, vp]
    L.crh_search.argtypes = [vp, i32, vp, i32, i32, vp, i32, i64, vp, vp, i32, vp]
    L.crh_search_finish.argtypes = [vp, vp]
    L.crh_index_destroy.argtypes = [vp]
    L.crh_last_error.restype = C.c_char_p

    def ok(rc):
        if rc != 0:
            raise SystemExit(f"{os.environ['CODERAG_HIP_LIB']}: error {rc}: {L.crh_last_error()}")
    g = torch.Generator(device="cuda").manual_seed(a.rows)
    h = vp()
    ok(L.crh_index_create(DIM, ffi.DTYPE_BF16, a.rows, 0, 0, C.byref(h)))
    for first in range(0, a.rows, 1 << 20):
        x = torch.randn((min(1 << 20, a.rows - first), DIM), generator=g, device="cuda")
        ok(L.crh_index_append(h, x.shape[0], x.data_ptr(), 1, None, None, None))
        torch.cuda.synchronize()
    q = torch.randn((NQ, DIM), generator=g, device="cuda")
    os_ = torch.empty((NQ, K), dtype=torch.float32, device="cuda")
    or_ = torch.empty((NQ, K), dtype=torch.int64, device="cuda")
    timed = event_timer(torch)

    def plain():
        ok(L.crh_search(h, NQ, q.data_ptr(), 1, K, None, 0, 0, os_.data_ptr(), or_.data_ptr(), 1, None))
        ok(L.crh_search_finish(h, None))
    for _ in range(a.warmup):
        timed(plain)
    ms = [timed(plain) for _ in range(a.steps * a.blocks)]
    print(json.dumps({"lib": os.environ["CODERAG_HIP_LIB"], "plain": summary(ms), "rows_checksum": int(or_.sum().item())}), flush=True)
    L.crh_index_destroy(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20, help="timed steps per leg and block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--plain-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.plain_only:
        return plain_only(a)
    results = []

    def emit(row):
        results.append(row)
        print(json.dumps(row), flush=True)

    if a.parent_lib:                                          # fresh children, alternating: parent, this tree, parent, this tree
        this_lib = os.environ.get("CODERAG_HIP_LIB", os.path.join(ROOT, "code-rag_amd", "lib", "libcoderag_hip.so"))
        for which, path in (("parent", a.parent_lib), ("this", this_lib)) * 2:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--rows", str(a.rows), "--steps", str(a.steps),
                                  "--blocks", str(a.blocks), "--warmup", str(a.warmup)], env=dict(os.environ, CODERAG_HIP_LIB=path),
                                 check=True, capture_output=True, text=True, timeout=600).stdout.strip().splitlines()[-1]
            emit(dict(json.loads(out), leg="a in a child process", library=which))

    torch, ffi, idx, q = build(a)
    os_ = torch.empty((NQ, K), dtype=torch.float32, device="cuda")
    or_ = torch.empty((NQ, K), dtype=torch.int64, device="cuda")
    oc = torch.zeros((NQ,), dtype=torch.int64, device="cuda")
    # the exact scores of the batch, as the store holds them (bf16 rows, bf16 queries): ranks -> thresholds
    big_s, _ = idx.search(q.cpu().numpy(), 1024)
    want_counts = {"d2": 100, "d4": 10_000, "d5": 100_000}
    thr = {"b": np.nextafter(big_s[:, 9], np.float32(-4)), "c": big_s[:, 999].copy()}
    for name, c in want_counts.items():                       # count mode tells the c-th score itself: bisect on the device's own exact counts
        lo, hi = np.zeros((NQ,), np.float32), big_s[:, 0].copy()      # (random unit rows: half of them score above 0)
        for _ in range(24):
            mid = ((lo.astype(np.float64) + hi) / 2).astype(np.float32)
            n = idx.search_range(q.cpu().numpy(), K, mid)[2]
            lo, hi = np.where(n >= c, mid, lo), np.where(n >= c, hi, mid)
        thr[name] = lo
    plain_mode = idx.nomination()

    def plain():
        idx.search(q, K, out_scores=os_, out_rows=or_)
        idx.search_finish()

    def plain3():
        idx.set_nomination(ffi.NOMINATE_BF16_3)
        idx.search(q, K, out_scores=os_, out_rows=or_)
        idx.search_finish()
        idx.set_nomination(ffi.NOMINATE_INT8)

    def ranged(name, counts):
        def run():
            idx.search_range(q, K, thr[name], counts=counts, out_scores=os_, out_rows=or_, out_counts=oc if counts else None)
            idx.search_finish()
        return run
    legs = {"a": plain, "a3": plain3, "b": ranged("b", False), "c": ranged("c", False),
            "d2": ranged("d2", True), "d4": ranged("d4", True), "d5": ranged("d5", True)}
    timed = event_timer(torch)
    for fn in legs.values():
        for _ in range(a.warmup):
            timed(fn)
    ms = {name: [] for name in legs}
    for _ in range(a.blocks):
        for name, fn in legs.items():
            ms[name] += [timed(fn) for _ in range(a.steps)]
    plain()
    base_rows = or_.cpu().numpy().copy()
    counts = {}
    for name in ("b", "c"):
        legs[name]()
        if not np.array_equal(or_.cpu().numpy(), base_rows):
            raise SystemExit(f"leg {name}: a threshold at or below the 10th score changed the list")
    for name in want_counts:
        legs[name]()
        counts[name] = oc.cpu().numpy().copy()
        st = idx.stats()
        emit({"leg": name, "count_median": int(np.median(counts[name])), "count_min": int(counts[name].min()), "count_max": int(counts[name].max()),
              "candidates_per_query_max": st["max_query_cands"], "fallback_used": st["fallback_used"], **summary(ms[name])})
    for name in ("a", "a3", "b", "c"):
        emit({"leg": name, "nomination": plain_mode if name == "a" else ffi.NOMINATE_BF16_3, **summary(ms[name])})
    # e: the host alternative and where it is wrong
    qh = q.cpu().numpy()
    for name in want_counts:
        host = []
        for _ in range(a.host_steps):
            t0 = time.perf_counter()
            hs, hr = idx.search(qh, 1024)
            n_host = (hs >= thr[name][:, None]).sum(1)
            host.append((time.perf_counter() - t0) * 1e3)
        wrong = n_host != counts[name]
        emit({"leg": f"e at {name}", "host_count_wrong_queries": int(wrong.sum()), "of": NQ, "host_count_max": int(n_host.max()),
              "true_count_median": int(np.median(counts[name])), **summary(host)})
    idx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
