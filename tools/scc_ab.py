"""What do the device components and layers (crh_graph_scc / crh_graph_layers) cost, against an iterative Tarjan
and a Kahn pass on the host over the same CSRs?  (profiles/scc.md.)

    python tools/scc_ab.py [--nodes 100000,1000000] [--steps 5] [--out FILE.json]

Graphs, per node count: ``random`` (3 random edges per node, a few hubs: as tests/graph_cases.random_graph), ``planted`` (a
random DAG with cycles of 2 .. 2 000 nodes planted in it), and -- at the first node count only -- ``chain`` (0 -> 1 -> ... -> n -
1: the worst case for the trim, one node's worth of progress per sweep and wave).

Every graph is a STEP that runs in a process of its own under its own time limit (``--step-timeout`` seconds); a step that
fails, faults or runs out of time ends the tool -- nothing more is started on the device after it.  Legs of a step (both device
calls wait on their stream, so the host clock around them is the cost; median, min, max of ``--steps`` repetitions after a
warm-up):

  scc      crh_graph_scc + crh_graph_scc_bins, with the sweeps it launched
  layers   crh_graph_layers, both directions, with the sweeps
  words    crh_graph_node_words ("in_cycle") + crh_graph_row_words over 4 rows per node: a filter once the components are kept
  host     an iterative Tarjan (min-id labels) and Kahn layers over the same CSRs, plain Python over numpy arrays, once

A step fails if the device's labels or layers differ from the host's.
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


def make_graph(kind: str, n: int, seed: int = 0):
    rng = np.random.default_rng(seed)
    if kind == "chain":
        return np.stack([np.arange(n - 1), np.arange(1, n)], axis=1).astype(np.int64)
    pairs = rng.integers(0, n, size=(3 * n, 2), dtype=np.int64)
    if kind == "random":
        hubs = rng.choice(n, size=3, replace=False)
        extra = [np.stack([np.repeat(h, 150), rng.integers(0, n, size=150)], axis=1) for h in hubs]
        extra += [np.stack([rng.integers(0, n, size=150), np.repeat(h, 150)], axis=1) for h in hubs]
        return np.concatenate([pairs] + extra)
    order = rng.permutation(n)                                            # planted: a DAG along a random order ...
    pairs = np.stack([order[pairs.min(axis=1)], order[pairs.max(axis=1)]], axis=1)
    free, cycles = rng.permutation(n), []
    for size in (2, 3, 7, 70, 200, 2000):                                 # ... and cycles over random node sets
        if size * 4 > n:
            break
        members, free = free[:size], free[size:]
        cycles.append(np.stack([members, np.roll(members, -1)], axis=1))
    return np.concatenate([pairs] + cycles)


def host_components(off, adj, n):
    """Iterative Tarjan over the forward CSR; the label of a component is its smallest node id."""
    index = np.full(n, -1, np.int64)
    low = np.zeros(n, np.int64)
    on = np.zeros(n, bool)
    comp = np.full(n, -1, np.int32)
    nxt = off[:-1].copy()
    stack, counter = [], 0
    for root in range(n):
        if index[root] >= 0:
            continue
        work = [root]
        index[root] = low[root] = counter
        counter += 1
        stack.append(root)
        on[root] = True
        while work:
            v = work[-1]
            if nxt[v] < off[v + 1]:
                w = int(adj[nxt[v]])
                nxt[v] += 1
                if index[w] < 0:
                    index[w] = low[w] = counter
                    counter += 1
                    stack.append(w)
                    on[w] = True
                    work.append(w)
                elif on[w]:
                    low[v] = min(low[v], index[w])
                continue
            work.pop()
            if low[v] == index[v]:
                members = []
                while True:
                    w = stack.pop()
                    on[w] = False
                    members.append(w)
                    if w == v:
                        break
                comp[members] = min(members)
            if work:
                low[work[-1]] = min(low[work[-1]], low[v])
    return comp


def host_layers(pairs, comp, n):
    """Kahn over the condensation: the longest-path layer of every node's component, along the edges."""
    a, b = comp[pairs[:, 0]].astype(np.int64), comp[pairs[:, 1]].astype(np.int64)
    arcs = np.unique(np.stack([a, b], axis=1)[a != b], axis=0)
    indeg = np.bincount(arcs[:, 1], minlength=n)
    order = np.argsort(arcs[:, 0], kind="stable")
    heads = arcs[order, 1]
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(arcs[:, 0], minlength=n), out=off[1:])
    level = np.zeros(n, np.int32)
    ready = [int(c) for c in np.flatnonzero((comp == np.arange(n)) & (indeg == 0))]
    while ready:
        c = ready.pop()
        for d in heads[off[c]:off[c + 1]].tolist():
            level[d] = max(level[d], level[c] + 1)
            indeg[d] -= 1
            if indeg[d] == 0:
                ready.append(d)
    return level[comp]


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


def step(kind: str, n: int, steps: int) -> dict:
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi, graph
    pairs = make_graph(kind, n)
    off_f, adj_f, off_r, adj_r = graph.build_csr(pairs, n)
    g = ffi.Graph(n, device=0)
    g.set_relation(0, off_f, adj_f, off_r, adj_r)
    stream = ffi.current_stream(0)
    comp, info = g.scc(0, stream=stream)
    depth, dinfo = g.layers(0, "callees", comp, stream=stream)
    _, hinfo = g.layers(0, "callers", comp, stream=stream)
    t0 = time.perf_counter()
    want = host_components(off_f, adj_f, n)
    t1 = time.perf_counter()
    want_depth = host_layers(graph.unique_edges(pairs, n).astype(np.int64), want, n)
    t2 = time.perf_counter()
    if not np.array_equal(comp.cpu().numpy(), want):
        raise SystemExit(f"scc_ab: the components differ from the host's Tarjan ({kind}, {n} nodes)")
    if not np.array_equal(depth.cpu().numpy(), want_depth):
        raise SystemExit(f"scc_ab: the layers differ from the host's Kahn pass ({kind}, {n} nodes)")
    bins = g.scc_bins(comp, stream=stream)
    row_node = torch.from_numpy(np.repeat(np.arange(n, dtype=np.int32), 4)).to("cuda:0")
    out = {"graph": kind, "nodes": n, "edges": int(len(adj_f)), "components": int(info[0]), "cyclic": int(info[1]), "nodes_in_cycles": int(info[2]),
           "layers": int(dinfo[0]), "scc_sweeps": int(info[3]), "layer_sweeps": [int(dinfo[1]), int(hinfo[1])],
           "scc": clocked(torch, lambda: g.scc_bins(g.scc(0, stream=stream)[0], stream=stream), steps),
           "layers_ms": clocked(torch, lambda: (g.layers(0, "callees", comp, stream=stream), g.layers(0, "callers", comp, stream=stream)), steps),
           "words": clocked(torch, lambda: g.row_words(row_node, 0, seen=g.node_words("in_cycle", comp, bins=bins, stream=stream), stream=stream), steps),
           "host": {"tarjan_ms": (t1 - t0) * 1e3, "kahn_ms": (t2 - t1) * 1e3}}
    g.close()
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", default="100000,1000000")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one-step", default=None, help=argparse.SUPPRESS)     # "kind,nodes": run that step here and print its JSON
    args = ap.parse_args()
    if args.one_step:
        kind, n = args.one_step.split(",")
        print(json.dumps(step(kind, int(n), args.steps)))
        return
    sizes = [int(v) for v in args.nodes.split(",")]
    plan = [(kind, n) for n in sizes for kind in ("random", "planted")] + [("chain", sizes[0])]
    results = []
    for kind, n in plan:
        cmd = [sys.executable, os.path.abspath(__file__), "--one-step", f"{kind},{n}", "--steps", str(args.steps)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"scc_ab: the step {kind} nodes={n} ran out of its {args.step_timeout} s; nothing more is started")
        if done.returncode != 0:
            raise SystemExit(f"scc_ab: the step {kind} nodes={n} ended with status {done.returncode}; nothing more is started\n{done.stderr[-2000:]}")
        results.append(json.loads(done.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
