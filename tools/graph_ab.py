"""What do the device BFS (crh_graph_bfs), its listing and the reachability filter cost, against a host BFS over
the same CSR?  (profiles/graph.md.)

    python tools/graph_ab.py [--edges 100000,1000000,10000000] [--batch 1,64] [--hops 3] [--steps 20] [--out FILE.json]

Graph: ``edges`` random edges over ``edges / 4`` nodes (mean out-degree 4) plus 16 hubs with 2 000 callers each; the rows of the
filter's bitmap: 4 per node.  Source sets: one random node each.

Every (edges, batch) pair is a STEP that runs in a process of its own under its own time limit (``--step-timeout`` seconds); a
step that fails, faults or runs out of time ends the tool -- nothing more is started on the device after it.  Legs of a step,
timed between device events on one stream after a warm-up (median, p10, p90 of ``--steps`` repetitions):

  bfs     crh_graph_bfs alone ("callers", ``--hops`` levels)
  list    crh_graph_bfs + crh_graph_list (limit 50)
  filter  crh_graph_bfs (one query bit) + crh_graph_row_words: what a "graph" filter condition costs before the search
  host    a level-synchronous numpy BFS over the same reverse CSR, per source set, host clock (batch x one BFS)

A step fails if the device's level words for the first source set differ from the host BFS's.
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


def make_graph(n_edges: int, seed: int = 0):
    rng = np.random.default_rng(seed)
    n = max(64, n_edges // 4)
    pairs = rng.integers(0, n, size=(n_edges, 2), dtype=np.int64)
    hubs = rng.choice(n, size=16, replace=False)
    extra = np.stack([rng.integers(0, n, size=16 * 2000), np.repeat(hubs, 2000)], axis=1)
    return n, np.concatenate([pairs, extra])


def host_bfs(off, adj, n, sources, hops):
    """Minimum depths (-1: not reached) by a level-synchronous frontier walk over one CSR."""
    depth = np.full(n, -1, np.int32)
    front = np.unique(np.asarray(sources, np.int64))
    depth[front] = 0
    for d in range(1, hops + 1):
        if not front.size:
            break
        starts, cnt = off[front], off[front + 1] - off[front]
        idx = np.repeat(starts - (np.cumsum(cnt) - cnt), cnt) + np.arange(int(cnt.sum()))      # every entry of the frontier's lists
        nxt = np.unique(adj[idx]) if idx.size else np.zeros((0,), np.int64)
        nxt = nxt[depth[nxt] < 0]
        depth[nxt] = d
        front = nxt
    return depth


def timed(torch, fn, steps: int):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for i in range(steps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = np.asarray([ev[i].elapsed_time(ev[i + 1]) for i in range(steps)])
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90))}


def step(n_edges: int, batch: int, hops: int, steps: int) -> dict:
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi, graph
    n, pairs = make_graph(n_edges)
    off_f, adj_f, off_r, adj_r = graph.build_csr(pairs, n)
    g = ffi.Graph(n, device=0)
    g.set_relation(0, off_f, adj_f, off_r, adj_r)
    rng = np.random.default_rng(1)
    sets = [[int(v)] for v in rng.integers(0, n, size=batch)]
    stream = ffi.current_stream(0)
    row_node = torch.from_numpy(np.repeat(np.arange(n, dtype=np.int32), 4)).to("cuda:0")
    levels, _, _ = g.bfs(0, "callers", sets, hops, stream=stream)
    torch.cuda.synchronize()
    got = levels.cpu().numpy().view(np.uint64)
    t0 = time.perf_counter()
    want = host_bfs(off_r, adj_r, n, sets[0], hops)          # (towards the callers: a node's next nodes are its sources, the reverse CSR)
    host_one = time.perf_counter() - t0
    for d in range(hops + 1):
        if not np.array_equal((got[d] & np.uint64(1)).astype(bool), want == d):
            raise SystemExit(f"graph_ab: level {d} differs from the host BFS at {n_edges} edges")
    out = {"edges": int(len(adj_f)), "nodes": n, "batch": batch, "hops": hops, "reached_by_set_0": int((want >= 0).sum()),
           "bfs": timed(torch, lambda: g.bfs(0, "callers", sets, hops, stream=stream), steps),
           "list": timed(torch, lambda: (g.bfs(0, "callers", sets, hops, stream=stream), g.list(50, stream=stream)), steps),
           "filter": timed(torch, lambda: (g.bfs(0, "callers", sets[:1], hops, include_self=True, stream=stream), g.row_words(row_node, 0, stream=stream)), steps),
           "host": {"one_bfs_ms": host_one * 1e3, "batch_ms": host_one * 1e3 * batch}}
    g.close()
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", default="100000,1000000,10000000")
    ap.add_argument("--batch", default="1,64")
    ap.add_argument("--hops", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one-step", default=None, help=argparse.SUPPRESS)     # "edges,batch": run that step here and print its JSON
    args = ap.parse_args()
    if args.one_step:
        e, b = (int(v) for v in args.one_step.split(","))
        print(json.dumps(step(e, b, args.hops, args.steps)))
        return
    results = []
    for e in (int(v) for v in args.edges.split(",")):
        for b in (int(v) for v in args.batch.split(",")):
            cmd = [sys.executable, os.path.abspath(__file__), "--one-step", f"{e},{b}", "--hops", str(args.hops), "--steps", str(args.steps)]
            try:
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"graph_ab: the step edges={e} batch={b} ran out of its {args.step_timeout} s; nothing more is started")
            if done.returncode != 0:
                raise SystemExit(f"graph_ab: the step edges={e} batch={b} ended with status {done.returncode}; nothing more is started\n{done.stderr[-2000:]}")
            results.append(json.loads(done.stdout.strip().splitlines()[-1]))
            print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
