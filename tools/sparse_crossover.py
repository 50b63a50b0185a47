"""Where does the sparse route of a filtered search pay?  (the table is profiles/sparse_crossover.md.)

    python tools/sparse_crossover.py --rows 1000000 10000000 [--libs OLD.so NEW.so] [--out FILE.json]

Times filtered batch-64 top-100 searches (device queries, device outputs, crh_search + crh_search_finish, a host clock around
work that ends in a synchronise) under masks that leave 1/4, 1/16, 1/64 and 1/256 of the 32-row tiles populated -- one contiguous
"project" block each, starting inside a tile, as rows arrive project by project -- and under one scattered 1-of-3 column that
leaves every tile populated.  Every library given with --libs (default: the tree's own) gets its own index over the same seeded
rows; the repeats of one case alternate between the libraries and, inside a library that has crh_index_set_sparse_route,
between the route forced on (max_fraction_den = 1), switched off, and left to the default rule.  A library built from an earlier
commit can be timed beside the current one: the script binds the handful of entry points it needs by itself and asks for
nothing newer than crh_search.

Per case and variant: median ms per batch over the repeats, their min..max (the run-to-run spread), crh_search_stats.tiles and
fallback_used of one batch, and the nomination mode the batch used (crh_index_get_nomination; "list" = the sparse route).
Also checks that every variant returns the same ids and score bits as the first.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRACTIONS = (4, 16, 64, 256)
MODES = {0: "bf16x3", 1: "bf16", 2: "int8"}


class Filter(C.Structure):
    _fields_ = [("col", C.c_int32), ("code", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("rows", C.c_int64), ("tiles", C.c_int64), ("seed_tiles", C.c_int64), ("candidates", C.c_int64),
                ("max_query_cands", C.c_int64), ("fallback_used", C.c_int32), ("batches", C.c_int32)]


class Lib:
    def __init__(self, path):
        self.path, self.L = path, C.CDLL(path)
        L, vp, i32, i64 = self.L, C.c_void_p, C.c_int, C.c_int64
        L.crh_last_error.restype = C.c_char_p
        L.crh_index_create.argtypes = [i32, i32, i64, i32, i32, C.POINTER(vp)]
        L.crh_index_append.argtypes = [vp, i64, vp, i32, vp, C.POINTER(i64), vp]
        L.crh_search.argtypes = [vp, i32, vp, i32, i32, C.POINTER(Filter), i32, i64, vp, vp, i32, vp]
        L.crh_search_finish.argtypes = [vp, vp]
        L.crh_search_get_stats.argtypes = [vp, C.POINTER(Stats)]
        L.crh_index_get_nomination.argtypes = [vp, C.POINTER(i32)]
        L.crh_index_destroy.argtypes = [vp]
        self.has_route = hasattr(L, "crh_index_set_sparse_route")
        if self.has_route:
            L.crh_index_set_sparse_route.argtypes = [vp, i32, i32]
        self.h = vp()

    def check(self, rc):
        if rc != 0:
            raise RuntimeError(f"{self.path}: error {rc}: {self.L.crh_last_error().decode()}")

    def variants(self, den):
        return [("list", 1, 1), ("dense", 0, 0), ("default", 1, den)] if self.has_route else [("dense", None, None)]


def build(lib, torch, rows, dim, seed):
    lib.check(lib.L.crh_index_create(dim, 1, rows, len(FRACTIONS) + 1, 0, C.byref(lib.h)))
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    for first in range(0, rows, 1 << 20):
        n = min(1 << 20, rows - first)
        x = torch.randn((n, dim), generator=g, device="cuda", dtype=torch.float32)
        r = np.arange(first, first + n)
        cols = [((r >= 1003) & (r < 1003 + rows // den)).astype(np.int32) for den in FRACTIONS]   # one block per fraction, unaligned start
        cols.append(rng.integers(0, 3, n).astype(np.int32))
        codes = torch.from_numpy(np.ascontiguousarray(np.stack(cols, axis=1))).cuda()
        out = C.c_int64(0)
        lib.check(lib.L.crh_index_append(lib.h, n, x.data_ptr(), 1, codes.data_ptr(), C.byref(out), None))
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1000000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--libs", nargs="+", default=[os.path.join(ROOT, "code-rag_amd", "lib", "libcoderag_hip.so")])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--den", type=int, default=4, help="max_fraction_den of the 'default' variant (the library's own default)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import coderag_amd  # noqa: F401  (loads torch's HIP runtime globally before the libraries, as ffi.py does)
    from coderag_amd import ffi
    ffi._preload_hip_runtime()
    nq, k = 64, 100
    results = []
    for rows in a.rows:
        libs = [Lib(p) for p in a.libs]
        for lib in libs:
            build(lib, torch, rows, a.dim, seed=rows)
        q = torch.randn((nq, a.dim), generator=torch.Generator(device="cuda").manual_seed(1), device="cuda")
        os_ = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        or_ = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        cases = [(f"block 1/{den}", c, 1) for c, den in enumerate(FRACTIONS)] + [("scattered 1/3", len(FRACTIONS), 1)]
        for name, col, code in cases:
            flt = (Filter * 1)(Filter(col, code))
            runs = [(li, lib, v) for li, lib in enumerate(libs) for v in lib.variants(a.den)]
            times = {i: [] for i in range(len(runs))}
            info, ref = {}, None

            def one(lib, v, n):
                if v[1] is not None:
                    lib.check(lib.L.crh_index_set_sparse_route(lib.h, v[1], v[2]))
                for _ in range(n):
                    lib.check(lib.L.crh_search(lib.h, nq, q.data_ptr(), 1, k, flt, 1, 0, os_.data_ptr(), or_.data_ptr(), 1, None))
                    lib.check(lib.L.crh_search_finish(lib.h, None))
                torch.cuda.synchronize()
            for i, (li, lib, v) in enumerate(runs):             # warm-up, results, stats of one batch
                mode = C.c_int(0)
                lib.check(lib.L.crh_index_get_nomination(lib.h, C.byref(mode)))
                one(lib, v, 3)
                st = Stats()
                lib.check(lib.L.crh_search_get_stats(lib.h, C.byref(st)))
                got = (os_.cpu().numpy().view(np.uint32).copy(), or_.cpu().numpy().copy())
                ref = ref or got
                same = bool(np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]))
                ntiles = (rows + 31) // 32
                info[i] = {"tiles": int(st.tiles), "seed_tiles": int(st.seed_tiles), "fallback_used": int(st.fallback_used),
                           "nomination": "list" if (v[0] == "list" or st.tiles < ntiles) else MODES[mode.value], "same_bits_as_first": same}
            for _ in range(a.repeats):                           # the repeats alternate between the variants
                for i, (li, lib, v) in enumerate(runs):
                    one(lib, v, 2)
                    t0 = time.perf_counter()
                    one(lib, v, a.iters)
                    times[i].append((time.perf_counter() - t0) * 1e3 / a.iters)
            for i, (li, lib, v) in enumerate(runs):
                row = {"rows": rows, "case": name, "lib": os.path.relpath(lib.path, ROOT), "variant": v[0],
                       "ms_median": round(statistics.median(times[i]), 4), "ms_min": round(min(times[i]), 4), "ms_max": round(max(times[i]), 4), **info[i]}
                results.append(row)
                print(json.dumps(row), flush=True)
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
