"""What do chains in full (crh_graph_sigma / _chains / _between / _bfs_avoiding) cost, against a host restatement
over the same CSRs?  (profiles/chains.md.)

    python tools/chains_ab.py [--nodes 100000,1000000] [--steps 5] [--hops 8] [--out FILE.json]

Graph, per node count: 3 random edges per node and a few hubs (as tests/graph_cases.random_graph).  64 pairs: random sources,
every target a node the host's BFS finds at the greatest depth within ``--hops`` of its source.

Every node count is a STEP that runs in a process of its own under its own time limit (``--step-timeout`` seconds); a step that
fails, faults or runs out of time ends the tool -- nothing more is started on the device after it.  Legs of a step (the host
clock around enqueue + synchronize; median, min, max of ``--steps`` repetitions after a warm-up):

  chains     one BFS of 64 source sets + crh_graph_sigma + crh_graph_chains (K = 10) + the copy of the chains to the host
  between    what the ``between`` filter runs for one pair: two BFS of one set, crh_graph_between, crh_graph_row_words over 4 rows
             per node
  must_pass  crh_graph_bfs_avoiding for the interior nodes of 64 pairs' first chains, 64 (pair, node) bits per pass, + the gather
             of the targets' bits
  host       the same three answers from numpy over the same CSRs (a level-synchronous BFS by ``np.repeat``, counts by
             ``np.add.at`` in u64, must-pass by one BFS per candidate), for the first ``--host-pairs`` pairs, per pair

A step fails if a device answer differs from the host's.
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


def make_graph(n: int, seed: int = 0):
    rng = np.random.default_rng(seed)
    pairs = rng.integers(0, n, size=(3 * n, 2), dtype=np.int64)
    hubs = rng.choice(n, size=3, replace=False)
    extra = [np.stack([np.repeat(h, 150), rng.integers(0, n, size=150)], axis=1) for h in hubs]
    extra += [np.stack([rng.integers(0, n, size=150), np.repeat(h, 150)], axis=1) for h in hubs]
    return np.concatenate([pairs] + extra)


def host_bfs(off, adj, sources, hops: int, banned: int = -1):
    """Minimum depths (-1: not reached within ``hops``) over one CSR, never entering ``banned``."""
    depth = np.full(len(off) - 1, -1, np.int32)
    front = np.unique(np.asarray(sources, np.int64))
    front = front[front != banned]
    depth[front] = 0
    for d in range(1, hops + 1):
        if not front.size:
            break
        cnt = off[front + 1] - off[front]
        idx = np.repeat(off[front] - np.cumsum(cnt) + cnt, cnt) + np.arange(int(cnt.sum()))
        front = np.unique(adj[idx])
        front = front[(depth[front] < 0) & (front != banned)]
        depth[front] = d
    return depth


def host_sigma(tails, heads, depth, hops: int):
    """The number of shortest chains to every node, u64; refuses a sum that would not fit (the graphs here stay far below)."""
    sigma = (depth == 0).astype(np.uint64)
    shadow = sigma.astype(np.float64)
    for d in range(1, hops + 1):
        on = (depth[tails] == d - 1) & (depth[heads] == d)
        np.add.at(sigma, heads[on], sigma[tails[on]])
        np.add.at(shadow, heads[on], shadow[tails[on]])
    if shadow.max(initial=0.0) >= 2.0 ** 63:
        raise SystemExit("chains_ab: a chain count leaves the u64 range of the host restatement")
    return sigma


def host_chain(off_r, adj_r, depth, sigma, target: int, rank: int):
    rem, u, chain = rank, target, [target]
    for d in range(int(depth[target]), 0, -1):
        for v in adj_r[off_r[u]:off_r[u + 1]].tolist():
            if depth[v] != d - 1:
                continue
            if rem < int(sigma[v]):
                u = v
                break
            rem -= int(sigma[v])
        chain.append(u)
    return chain[::-1]


def clocked(torch, fn, steps: int):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def step(n: int, steps: int, hops: int, host_pairs: int) -> dict:
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi, graph
    pairs = make_graph(n)
    off_f, adj_f, off_r, adj_r = graph.build_csr(pairs, n)
    tails, heads = np.repeat(np.arange(n, dtype=np.int64), np.diff(off_f)), adj_f.astype(np.int64)
    rng = np.random.default_rng(1)
    sources = rng.integers(0, n, size=64).tolist()
    targets, K = [], 10
    for s in sources:
        depth = host_bfs(off_f, adj_f, [s], hops)
        targets.append(int(np.flatnonzero(depth == depth.max())[0]))
    g = ffi.Graph(n, device=0)
    g.set_relation(0, off_f, adj_f, off_r, adj_r)
    stream = ffi.current_stream(0)
    sets = [[s] for s in sources]

    def chains():
        g.bfs(0, "callees", sets, hops, include_self=True, stream=stream)
        g.sigma(0, "callees", stream=stream)
        return [t.cpu().numpy() for t in g.chains(0, "callees", targets, K, stream=stream)]

    row_node = torch.from_numpy(np.repeat(np.arange(n, dtype=np.int32), 4)).to("cuda:0")

    def between(q=0):
        g.bfs(0, "callees", [sets[q]], hops, include_self=True, stream=stream)
        g.bfs(0, "callers", [[targets[q]]], hops, include_self=True, stream=stream, back=True)
        words, dist = g.between(mode="any", stream=stream)
        return words, dist, g.row_words(row_node, 0, seen=words, stream=stream)

    nodes, length, count = chains()
    count = count.view(np.uint64)
    cand = [(q, int(v)) for q in range(64) for v in nodes[q, 0, 1:max(int(length[q]) - 1, 1)]]

    def must_pass():
        found = []
        for b in range(0, len(cand), 64):
            some = cand[b:b + 64]
            g.bfs_avoiding(0, "callees", [sets[q] for q, _ in some], hops, [v for _, v in some], include_self=True, stream=stream)
            found += [c for c, still in zip(some, g.seen_bits([targets[q] for q, _ in some])) if not still]
        return found

    must = must_pass()
    host = {"chains_ms": [], "between_ms": [], "must_pass_ms": []}
    for q in range(host_pairs):
        t0 = time.perf_counter()
        depth = host_bfs(off_f, adj_f, sets[q], hops)
        sigma = host_sigma(tails, heads, depth, hops)
        want = [host_chain(off_r, adj_r, depth, sigma, targets[q], r) for r in range(min(K, int(sigma[targets[q]])))]
        t1 = time.perf_counter()
        back = host_bfs(off_r, adj_r, [targets[q]], hops)
        ahead = host_bfs(off_f, adj_f, sets[q], hops)                   # (the filter has no BFS of the chains to lean on)
        inside = (ahead >= 0) & (back >= 0) & (ahead + back <= hops)
        t2 = time.perf_counter()
        mine = [v for v in want[0][1:-1] if host_bfs(off_f, adj_f, sets[q], hops, banned=v)[targets[q]] < 0]
        t3 = time.perf_counter()
        host["chains_ms"].append((t1 - t0) * 1e3)
        host["between_ms"].append((t2 - t1) * 1e3)
        host["must_pass_ms"].append((t3 - t2) * 1e3)
        if int(count[q]) != int(sigma[targets[q]]) or [nodes[q, r, :length[q]].tolist() for r in range(len(want))] != want:
            raise SystemExit(f"chains_ab: the chains of pair {q} differ from the host's ({n} nodes)")
        words = between(q)[0].cpu().numpy().view(np.uint64)
        if not np.array_equal(words != 0, inside):
            raise SystemExit(f"chains_ab: the nodes between of pair {q} differ from the host's ({n} nodes)")
        if [v for p, v in must if p == q] != mine:
            raise SystemExit(f"chains_ab: the must-pass nodes of pair {q} differ from the host's ({n} nodes)")
    out = {"nodes": n, "edges": int(len(adj_f)), "hops": hops, "pairs": 64, "K": K, "chain_length_nodes": [int(length.min()), int(length.max())],
           "count_max": int(count.max()), "candidates": len(cand), "must_pass_found": len(must), "bfs_avoiding_passes": (len(cand) + 63) // 64,
           "chains": clocked(torch, chains, steps), "between": clocked(torch, between, steps), "must_pass": clocked(torch, must_pass, steps),
           "host_per_pair": {k: float(np.median(v)) for k, v in host.items()}, "host_pairs": host_pairs}
    g.close()
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", default="100000,1000000")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--hops", type=int, default=8)
    ap.add_argument("--host-pairs", type=int, default=4)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one-step", default=None, help=argparse.SUPPRESS)     # "nodes": run that step here and print its JSON
    args = ap.parse_args()
    if args.one_step:
        print(json.dumps(step(int(args.one_step), args.steps, args.hops, args.host_pairs)))
        return
    results = []
    for n in [int(v) for v in args.nodes.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--one-step", str(n), "--steps", str(args.steps), "--hops", str(args.hops),
               "--host-pairs", str(args.host_pairs)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"chains_ab: the step nodes={n} ran out of its {args.step_timeout} s; nothing more is started")
        if done.returncode != 0:
            raise SystemExit(f"chains_ab: the step nodes={n} ended with status {done.returncode}; nothing more is started\n{done.stderr[-2000:]}")
        results.append(json.loads(done.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
