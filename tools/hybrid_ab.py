"""What does the hybrid re-rank with graph results cost on the device, against today's alternative, per 64-query
batch?  (profiles/hybrid.md.)

    python tools/hybrid_ab.py [--rows 20000] [--dim 384] [--batch 64] [--hops 2] [--steps 20] [--out FILE.json]

Collection: ``rows`` random vectors, six rows per graph node, ``4 x nodes`` random call edges.  Every query is a find_callers plan
about one random node, ``--hops`` hops.  Two legs, each a whole call on the host clock after a warm-up (median, p10, p90 of
``--steps`` repetitions; the store's stream is drained inside each call):

  device  engine_helpers.search_and_rank_hybrid_batch_device: search, BFS, list, candidates, gathers, crh_rerank_hybrid
  host    the same search (search_batch), the BFS lists to the host (graph_neighbors_batch), GraphNode / GraphContext objects from
          the payloads of the nodes' representative rows, HybridRanker.rank_results in Python, one query at a time

The run fails if the two legs rank a query differently (order, f64 scores, sources).  One process, one time limit
(``--timeout`` seconds, enforced by an alarm): nothing is started on the device after a failure.
"""
import argparse
import asyncio
import json
import os
import signal
import sys
import time
from types import SimpleNamespace as NS

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(xs):
    xs = np.sort(np.asarray(xs)) * 1e3
    return {"median_ms": float(np.median(xs)), "p10_ms": float(xs[int(0.1 * (len(xs) - 1))]), "p90_ms": float(xs[int(0.9 * (len(xs) - 1))])}


async def run(args):
    import coderag_amd  # noqa: F401
    from coderag_amd.engine_helpers import centrality_candidates, search_and_rank_hybrid_batch_device
    from coderag_amd.query_types import GraphContext, GraphNode
    from coderag_amd.ranking import HybridRanker
    from coderag_amd.ranking.device import HybridDeviceReranker
    from coderag_amd.store import HipVectorStore
    from coderag_amd.vector_search import _CODE_KEYS, _project

    rng = np.random.default_rng(0)
    n, nodes = args.rows, max(8, args.rows // 6)
    pay = [{"file_path": f"src/m{i % 997}.py", "entity_name": f"n{i % nodes}", "graph_node_id": f"n{i % nodes}", "entity_type": "function",
            "language": "python", "content": "x" * (60 + i % 400), "start_line": i, "end_line": i + 9, "summary": "s" if i % 2 else None}
           for i in range(n)]
    raw = rng.standard_normal((n, args.dim)).astype(np.float32)
    ids = [f"00000000-0000-4000-8000-{i:012d}" for i in range(n)]
    edges = [(f"n{a}", f"n{b}") for a, b in rng.integers(0, nodes, size=(4 * nodes, 2)).tolist() if a != b]
    qv = rng.standard_normal((args.batch, args.dim)).astype(np.float32)
    targets = rng.integers(0, nodes, size=args.batch).tolist()
    plans = [NS(primary_intent="find_callers", entities=[NS(name=f"n{t}", is_primary=True)], requires_multi_hop=True, max_hops=args.hops)
             for t in targets]
    first_row = {}
    for i, p in enumerate(pay):
        first_row.setdefault(p["entity_name"], i)                        # nothing is deleted: the representative row is the first one

    async with HipVectorStore(dim=args.dim, dtype="bf16", initial_capacity=n, device=0) as s:
        await s.create_collections()
        for a in range(0, n, 8192):
            await s.upsert("code_chunks", ids[a:a + 8192], raw[a:a + 8192], pay[a:a + 8192])
        await s.set_graph_edges("code_chunks", edges, derive_degrees=True)
        deg = s._col("code_chunks")._degrees or {}
        rr, host = HybridDeviceReranker(), HybridRanker()

        async def device_leg():
            return await search_and_rank_hybrid_batch_device(s, rr, host, qv, plans, limit=args.limit)

        def node(name, depth=None):
            p = pay[first_row[name]]
            return GraphNode(node_type=p["entity_type"], name=p["entity_name"], qualified_name=name, file_path=p["file_path"], summary=p["summary"],
                             start_line=p["start_line"], end_line=p["end_line"], metadata={} if depth is None else {"depth": depth})

        async def host_leg():
            lists = await s.search_batch("code_chunks", qv, args.limit)
            near = await s.graph_neighbors_batch("code_chunks", [[f"n{t}"] for t in targets], direction="callers", max_hops=args.hops, limit=50)
            out = []
            for plan, t, hits, res in zip(plans, targets, lists, near):
                known = f"n{t}" in first_row and not res["unresolved"]
                ctx = GraphContext(primary_entities=[node(f"n{t}")] if known else [],
                                   callers=[node(h["name"], h["depth"]) for h in res["hits"] if h["name"] in first_row])
                flat = [_project(h, _CODE_KEYS) for h in hits]
                out.append(host.rank_results(plan, ctx, flat, {m: {"total_degree": deg[m]} for m in centrality_candidates(ctx, flat) if m in deg}))
            return out

        a, b = await device_leg(), await host_leg()
        for q, (x, y) in enumerate(zip(a, b)):
            if [(r.file_path, r.start_line, r.final_score, r.source) for r in x] != [(r.file_path, r.start_line, r.final_score, r.source) for r in y]:
                raise SystemExit(f"query {q}: the device and the host leg rank differently")
        times = {"device": [], "host": []}
        for name, leg in (("device", device_leg), ("host", host_leg)):
            for i in range(args.steps + 3):
                t0 = time.perf_counter()
                await leg()
                if i >= 3:
                    times[name].append(time.perf_counter() - t0)
        graph_results = sum(r.source != "vector" for x in a for r in x)
    return {"rows": n, "dim": args.dim, "batch": args.batch, "hops": args.hops, "limit": args.limit, "steps": args.steps, "nodes": nodes,
            "graph_or_hybrid_results": int(graph_results), "device": stats(times["device"]), "host": stats(times["host"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--hops", type=int, default=2)
    ap.add_argument("--limit", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out")
    args = ap.parse_args()
    signal.alarm(args.timeout)                 # one time limit for the whole run: the process ends, nothing more is started
    res = asyncio.run(run(args))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
