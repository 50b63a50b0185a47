#!/usr/bin/env python3
"""Personalised PageRank on the device (crh_graph_ppr) against a numpy restatement: time per step and bit
equality, at both ends of the state width (QS = 1: one lane per node; QS = 64: one wave per node), with and without a hub.

    python tools/ppr_ab.py --nodes 100000 1000000 --out profiles/ppr_ab.json

Per case one JSON line: the graph, the device time of a whole call and per step (device events around `reps` calls after a
warm-up), the bytes a step must move by the model  E * QS * 4 (gathered rows) + 3 * n * QS * 4 (p0 read, p and contrib written)
and the rate that gives, the numpy restatement's time per step on the host, and whether the two agree bit for bit.

The restatement here keeps every pull list's ORDER while staying vectorised: round k adds, for every node with more than k
entries, the contribution of its k-th entry -- one f32 addition per node per round, the additions of one node in list order."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
F32 = np.float32


def make_graph(n: int, mean_degree: int, hub_degree: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    pairs = rng.integers(0, n, size=(mean_degree * n, 2), dtype=np.int64)
    if hub_degree:
        others = rng.choice(n - 1, size=min(hub_degree, n - 1), replace=False) + 1
        pairs = np.concatenate([pairs, np.stack([others, np.zeros_like(others)], 1), np.stack([np.zeros_like(others), others], 1)])
    return pairs


def numpy_ppr(csr, direction: str, seeds: np.ndarray, weights: np.ndarray, restart: float, steps: int):
    """(scores f32 [n, nq], seconds per step).  ``csr`` = (off_fwd, adj_fwd, off_rev, adj_rev)."""
    off_f, adj_f, off_r, adj_r = csr
    n = off_f.size - 1
    lists = {"callees": [(off_r, adj_r)], "callers": [(off_f, adj_f)], "both": [(off_r, adj_r), (off_f, adj_f)]}[direction]
    out = {"callees": np.diff(off_f), "callers": np.diff(off_r), "both": np.diff(off_f) + np.diff(off_r)}[direction]
    inv = np.zeros(n, F32)
    inv[out > 0] = F32(1.0) / out[out > 0].astype(F32)
    nq, c = seeds.shape
    p0 = np.zeros((n, nq), F32)
    for q in range(nq):
        total, per = F32(0.0), {}
        for v, w in zip(seeds[q].tolist(), weights[q]):
            if v < 0 or not w > 0:
                continue
            per[v] = F32(per.get(v, F32(0.0)) + w)
            total = F32(total + w)
        for v, w in per.items():
            p0[v, q] = F32(w / total)
    r = F32(restart)
    a = F32(F32(1.0) - r)
    base = (r * p0).astype(F32)
    p = p0.copy()
    t0 = time.perf_counter()
    for _ in range(steps):
        contrib = (p * inv[:, None]).astype(F32)
        acc = np.zeros((n, nq), F32)
        for off, adj in lists:
            deg = np.diff(off)
            order = np.argsort(-deg, kind="stable")                      # nodes by falling degree: round k touches a prefix
            sorted_deg = deg[order]
            for k in range(int(deg.max()) if n else 0):
                m = int(np.searchsorted(-sorted_deg, -k, side="left"))   # nodes with more than k entries
                who = order[:m]
                acc[who] = (acc[who] + contrib[adj[off[who] + k]]).astype(F32)
        p = (base + (a * acc).astype(F32)).astype(F32)
    return p, (time.perf_counter() - t0) / steps


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--mean-degree", type=int, default=5)
    ap.add_argument("--hub-degree", type=int, nargs="+", default=[0, 20_000], help="callers and callees of node 0 (0: no hub)")
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--check-steps", type=int, default=2, help="steps of the run compared with numpy (0: no comparison)")
    ap.add_argument("--seeds", type=int, default=40)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--direction", default="both")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi, graph
    if not torch.cuda.is_available():
        print("ppr_ab needs a GPU: a CPU timing says nothing about the device", file=sys.stderr)
        return 2
    rows = []
    for n in args.nodes:
        for hub in args.hub_degree:
            csr = graph.build_csr(make_graph(n, args.mean_degree, hub, n), n)
            edges = int(csr[1].size)
            pull = {"both": 2 * edges}.get(args.direction, edges)
            g = ffi.Graph(n, device=0)
            g.set_relation(0, *csr)
            for nq in args.nq:
                rng = np.random.default_rng(nq)
                seeds = rng.integers(0, n, size=(nq, args.seeds)).astype(np.int32)
                weights = rng.random((nq, args.seeds)).astype(F32)
                s_dev, w_dev = torch.from_numpy(seeds).cuda(), torch.from_numpy(weights).cuda()
                qs = 1
                while qs < nq:
                    qs *= 2
                row = {"nodes": n, "edges": edges, "hub_degree": hub, "max_pull_list": int(max(np.diff(csr[0]).max(), np.diff(csr[2]).max())) * (2 if args.direction == "both" else 1),
                       "direction": args.direction, "nq": nq, "QS": qs, "steps": args.steps}
                if args.check_steps:
                    want, host_step = numpy_ppr(csr, args.direction, seeds, weights, 0.15, args.check_steps)
                    got = g.ppr(0, args.direction, s_dev, w_dev, 0.15, args.check_steps)
                    torch.cuda.synchronize()
                    row["bit_exact"] = bool(np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)))
                    row["numpy_ms_per_step"] = round(host_step * 1e3, 3)
                for _ in range(2):
                    g.ppr(0, args.direction, s_dev, w_dev, 0.15, args.steps)
                torch.cuda.synchronize()
                for steps, key in ((args.steps, "call_ms"), (1, "call_1step_ms")):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(args.reps):
                        g.ppr(0, args.direction, s_dev, w_dev, 0.15, steps)
                    t1.record()
                    torch.cuda.synchronize()
                    row[key] = round(t0.elapsed_time(t1) / args.reps, 4)
                step_ms = (row["call_ms"] - row["call_1step_ms"]) / max(args.steps - 1, 1)          # (the seed kernel and the memset cancel)
                model = pull * qs * 4 + 3 * n * qs * 4
                row.update(step_ms=round(step_ms, 4), model_bytes_per_step=model, model_gb_per_s=round(model / (step_ms * 1e-3) / 1e9, 1) if step_ms > 0 else None)
                print(json.dumps(row), flush=True)
                rows.append(row)
            g.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
