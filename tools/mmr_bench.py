"""What does the diversity-aware top-k (MMR) cost, and did the plain search stay where it was?  (profiles/mmr.md; DESIGN.md,
"Diversity-aware top-k".)

    python tools/mmr_bench.py --rows 1000000 10000000 [--libs PARENT.so THIS.so] [--out FILE.json]

Per row count, a bf16 index of seeded Gaussian rows per library, batch 64, device queries and device outputs:

* plain: crh_search + crh_search_finish at k = 10 and at every candidate count C -- a host clock around work that ends in a
  synchronise, the repeats alternating between the libraries.  A library built from the parent commit can be timed beside this
  one (the script binds the entry points it needs by itself and asks the first library for nothing newer than crh_search);
  the min..max of one library's repeats is the run-to-run spread the two medians are to be read against.
* mmr (the last library): for C in {40, 100, 256} and k in {10, 25}, crh_index_gather_vectors and crh_mmr_select each between
  device events, and the whole call search(C) + gather + select under the host clock.
* host: the alternative the device path replaces, on the same candidate lists -- one crh_index_read_rows per candidate row, then
  per query a Gram matrix with BLAS and the greedy loop in numpy.

Every figure: median, p10, p90 over the repeats (ms per batch of 64 queries).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CANDIDATES = (40, 100, 256)
PICKS = (10, 25)


class Lib:
    def __init__(self, path):
        self.path, self.L = path, C.CDLL(path)
        L, vp, i32, i64 = self.L, C.c_void_p, C.c_int, C.c_int64
        L.crh_last_error.restype = C.c_char_p
        L.crh_index_create.argtypes = [i32, i32, i64, i32, i32, C.POINTER(vp)]
        L.crh_index_append.argtypes = [vp, i64, vp, i32, vp, C.POINTER(i64), vp]
        L.crh_search.argtypes = [vp, i32, vp, i32, i32, vp, i32, i64, vp, vp, i32, vp]
        L.crh_search_finish.argtypes = [vp, vp]
        L.crh_index_read_rows.argtypes = [vp, i64, i64, vp]
        L.crh_index_destroy.argtypes = [vp]
        self.has_mmr = hasattr(L, "crh_mmr_select")
        if self.has_mmr:
            L.crh_index_gather_vectors.argtypes = [vp, i64, vp, i64, vp, vp]
            L.crh_mmr_select.argtypes = [i32, i32, i32, i32, vp, vp, vp, C.c_float, vp, vp, vp, vp, vp]
        self.h = vp()

    def check(self, rc):
        if rc != 0:
            raise RuntimeError(f"{self.path}: error {rc}: {self.L.crh_last_error().decode()}")


def build(lib, torch, rows, dim, seed):
    lib.check(lib.L.crh_index_create(dim, 1, rows, 0, 0, C.byref(lib.h)))
    g = torch.Generator(device="cuda").manual_seed(seed)
    for first in range(0, rows, 1 << 20):
        n = min(1 << 20, rows - first)
        x = torch.randn((n, dim), generator=g, device="cuda", dtype=torch.float32)
        out = C.c_int64(0)
        lib.check(lib.L.crh_index_append(lib.h, n, x.data_ptr(), 1, None, C.byref(out), None))
        torch.cuda.synchronize()


def summary(ms):
    return {"ms_median": round(float(np.median(ms)), 4), "ms_p10": round(float(np.percentile(ms, 10)), 4),
            "ms_p90": round(float(np.percentile(ms, 90)), 4), "ms_min": round(float(min(ms)), 4), "ms_max": round(float(max(ms)), 4)}


def host_mmr(scores, vecs, k, diversity):
    """numpy greedy loop over one query's candidates, similarities from one BLAS Gram matrix"""
    gram = vecs @ vecs.T
    lam = 1.0 - diversity
    picks, pen = [0], gram[0].copy()
    taken = np.zeros(len(scores), bool)
    taken[0] = True
    while len(picks) < k:
        obj = np.where(taken, -np.inf, lam * scores - diversity * pen)
        p = int(np.argmax(obj))
        picks.append(p)
        taken[p] = True
        np.maximum(pen, gram[p], out=pen)
    return picks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1000000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--libs", nargs="+", default=[os.path.join(ROOT, "code-rag_amd", "lib", "libcoderag_hip.so")])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--diversity", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import coderag_amd  # noqa: F401  (loads torch's HIP runtime globally before the libraries, as ffi.py does)
    from coderag_amd import ffi
    ffi._preload_hip_runtime()
    nq, dim = 64, a.dim
    results = []

    def emit(row):
        results.append(row)
        print(json.dumps(row), flush=True)

    for rows in a.rows:
        libs = [Lib(p) for p in a.libs]
        for lib in libs:
            build(lib, torch, rows, dim, seed=rows)
        q = torch.randn((nq, dim), generator=torch.Generator(device="cuda").manual_seed(1), device="cuda")
        bufs = {k: (torch.empty((nq, k), dtype=torch.float32, device="cuda"), torch.empty((nq, k), dtype=torch.int64, device="cuda"))
                for k in (10,) + CANDIDATES}

        def search(lib, k, n):
            s, r = bufs[k]
            for _ in range(n):
                lib.check(lib.L.crh_search(lib.h, nq, q.data_ptr(), 1, k, None, 0, 0, s.data_ptr(), r.data_ptr(), 1, None))
                lib.check(lib.L.crh_search_finish(lib.h, None))
            torch.cuda.synchronize()

        # ---- plain searches, the libraries alternating
        for k in (10,) + CANDIDATES:
            times = {i: [] for i in range(len(libs))}
            ref = None
            for i, lib in enumerate(libs):
                search(lib, k, 3)
                got = (bufs[k][0].cpu().numpy().view(np.uint32).copy(), bufs[k][1].cpu().numpy().copy())
                ref = ref or got
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), "the libraries disagree on a plain search"
            for _ in range(a.repeats):
                for i, lib in enumerate(libs):
                    search(lib, k, 2)
                    t0 = time.perf_counter()
                    search(lib, k, a.iters)
                    times[i].append((time.perf_counter() - t0) * 1e3 / a.iters)
            for i, lib in enumerate(libs):
                emit({"rows": rows, "what": "plain search", "k": k, "lib": os.path.relpath(lib.path, ROOT), **summary(times[i])})

        # ---- the added cost of diversity (the last library)
        lib = libs[-1]
        if lib.has_mmr:
            for c in CANDIDATES:
                cs, cr = bufs[c]
                vecs = torch.empty((nq, c, dim), dtype=torch.float32, device="cuda")
                for k in PICKS:
                    outs = (torch.empty((nq, k), dtype=torch.int32, device="cuda"), torch.empty((nq, k), dtype=torch.int64, device="cuda"),
                            torch.empty((nq, k), dtype=torch.float32, device="cuda"), torch.empty((nq, k), dtype=torch.float32, device="cuda"))

                    def gather():
                        lib.check(lib.L.crh_index_gather_vectors(lib.h, nq * c, cr.data_ptr(), 0, vecs.data_ptr(), None))

                    def select():
                        lib.check(lib.L.crh_mmr_select(nq, c, k, dim, cs.data_ptr(), cr.data_ptr(), vecs.data_ptr(), a.diversity,
                                                       *(o.data_ptr() for o in outs), None))
                    search(lib, c, 2)
                    gather()
                    select()
                    torch.cuda.synchronize()
                    tg, ts, tw = [], [], []
                    for _ in range(a.repeats):
                        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                        ev[0].record()
                        for _ in range(a.iters):
                            gather()
                        ev[1].record()
                        for _ in range(a.iters):
                            select()
                        ev[2].record()
                        torch.cuda.synchronize()
                        tg.append(ev[0].elapsed_time(ev[1]) / a.iters)
                        ts.append(ev[1].elapsed_time(ev[2]) / a.iters)
                        t0 = time.perf_counter()
                        for _ in range(a.iters):
                            lib.check(lib.L.crh_search(lib.h, nq, q.data_ptr(), 1, c, None, 0, 0, cs.data_ptr(), cr.data_ptr(), 1, None))
                            lib.check(lib.L.crh_search_finish(lib.h, None))
                            gather()
                            select()
                        torch.cuda.synchronize()
                        tw.append((time.perf_counter() - t0) * 1e3 / a.iters)
                    base = {"rows": rows, "candidates": c, "k": k, "diversity": a.diversity}
                    emit({**base, "what": "gather (device events)", **summary(tg)})
                    emit({**base, "what": "select (device events)", **summary(ts)})
                    emit({**base, "what": "search + gather + select (host clock)", **summary(tw)})
                    # ---- the host alternative on the same lists
                    sc, rw = cs.cpu().numpy(), cr.cpu().numpy()
                    picked = outs[0].cpu().numpy()
                    tf, tl = [], []
                    agree = 0
                    for rep in range(a.host_repeats):
                        t0 = time.perf_counter()
                        hv = np.empty((nq, c, dim), np.float32)
                        for qi in range(nq):
                            for j in range(c):
                                lib.check(lib.L.crh_index_read_rows(lib.h, int(rw[qi, j]), 1, hv[qi, j].ctypes.data))
                        tf.append((time.perf_counter() - t0) * 1e3)
                        t0 = time.perf_counter()
                        hp = [host_mmr(sc[qi], hv[qi], k, a.diversity) for qi in range(nq)]
                        tl.append((time.perf_counter() - t0) * 1e3)
                        agree = sum(int(hp[qi] == picked[qi].tolist()) for qi in range(nq))
                    emit({**base, "what": "host: read_rows per candidate", **summary(tf)})
                    emit({**base, "what": "host: BLAS Gram + numpy greedy", **summary(tl), "queries_with_the_device_picks": agree})
                del vecs
        for lib in libs:
            lib.L.crh_index_destroy(lib.h)
        del libs
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
