"""What does recommend by example cost next to the plain search it starts from, and what does the host
alternative cost?  (profiles/recommend.md.)

    python tools/recommend_ab.py [--rows 1000000] [--out FILE.json]

A bf16 store of clustered rows, dim 768; one batch of 64 logical queries at P = 4 positives and N = 2 negatives (stored points of
one cluster each), limit 10, both strategies through ``HipVectorStore.recommend_batch``.

* recommend: ``recommend_batch`` of the 64 example sets ("average", then "best"), ids in, hits out
* (a) plain: ``search_batch`` of the same 64 x 4 positive vectors at limit 10 -- what the parent commit can run for these examples
* (b) host:  the same selection in numpy: ``read_rows`` of the examples, the 256 lists from the device at the depth round 1
  uses, ``read_rows`` of every candidate, then tests/recommend_cases.recommend_select (written to be read, not tuned).  Its
  rows must equal the device's round-1 selection: the tool fails otherwise.

Every timing under a host clock around work that ends with the hits on the host: median, p10, p90 over the steps (ms per batch
of 64 logical queries).  ``recommend_rounds`` of the run is reported too: a batch that needs round 2 pays for it here.
"""
import argparse
import asyncio
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NQ, P, N, LIMIT = 64, 4, 2, 10


def summary(ms):
    return {"ms_median": round(float(np.median(ms)), 4), "ms_p10": round(float(np.percentile(ms, 10)), 4),
            "ms_p90": round(float(np.percentile(ms, 90)), 4), "steps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import coderag_amd  # noqa: F401
    from coderag_amd.store import HipVectorStore
    from tests import recommend_cases as rc
    rng = np.random.default_rng(a.rows)
    clusters = 256
    centres = rng.standard_normal((clusters, a.dim)).astype(np.float32)
    results = []

    def emit(row):
        results.append(row)
        print(json.dumps(row), flush=True)

    async def run():
        async with HipVectorStore(dim=a.dim, dtype="bf16", initial_capacity=a.rows, device=0, compact_dead_fraction=0.0) as s:
            await s.create_collections()
            which = np.empty((a.rows,), np.int64)
            for first in range(0, a.rows, 1 << 17):
                m = min(1 << 17, a.rows - first)
                w = rng.integers(0, clusters, m)
                which[first:first + m] = w
                x = centres[w] + 0.5 * rng.standard_normal((m, a.dim)).astype(np.float32)
                await s.upsert("code_chunks", [f"id{first + i}" for i in range(m)], x, [{"file_path": f"f{(first + i) % 997}.py", "language": "python"}] * m)
            col = s._col("code_chunks")
            sets = []
            for q in range(NQ):
                members = np.flatnonzero(which[:min(a.rows, 1 << 17)] == q % clusters)
                others = np.flatnonzero(which[:min(a.rows, 1 << 17)] == (q + 1) % clusters)
                sets.append(([f"id{i}" for i in members[:P]], [f"id{i}" for i in others[:N]]))
            slots = np.asarray([[int(i[2:]) for i in p + n] for p, n in sets], np.int64)
            pos_vecs = np.concatenate([col.index.read_rows(int(t), 1) for t in slots[:, :P].reshape(-1)])

            async def timed(fn):
                t0 = time.perf_counter()
                out = await fn()
                return (time.perf_counter() - t0) * 1e3, out

            async def plain():
                return await s.search_batch("code_chunks", pos_vecs, limit=LIMIT)
            for strategy in ("average", "best"):
                async def rec():
                    return await s.recommend_batch("code_chunks", sets, limit=LIMIT, strategy=strategy)
                for _ in range(a.warmup):
                    await timed(plain)
                    await timed(rec)
                before = dict(col.recommend_rounds)
                plain_ms, rec_ms = [], []
                for _ in range(a.steps):
                    plain_ms.append((await timed(plain))[0])
                    t, hits = await timed(rec)
                    rec_ms.append(t)
                rounds = {k: col.recommend_rounds[k] - before[k] for k in before}
                host, equal = [], None
                if strategy == "best":
                    c = min(1024 // P, 4 * LIMIT)
                    for _ in range(a.host_steps):
                        t0 = time.perf_counter()
                        ex = np.stack([np.concatenate([col.index.read_rows(int(t), 1) for t in row]) for row in slots])
                        cs, _, cr = col.shards.search(np.ascontiguousarray(ex[:, :P].reshape(NQ * P, a.dim)), c, [])
                        vecs = np.zeros((NQ * P * c, a.dim), np.float32)
                        flat = cr.reshape(-1)
                        for i in np.flatnonzero(flat >= 0):
                            vecs[i] = col.index.read_rows(int(flat[i]), 1)[0]
                        want = rc.recommend_select(cs.reshape(NQ, P, c), cr.reshape(NQ, P, c), vecs.reshape(NQ, P * c, a.dim), ex, slots, P, N, LIMIT, "best", True)
                        host.append((time.perf_counter() - t0) * 1e3)
                    dev = col.shards.recommend(slots, P, N, LIMIT, c, [], "best")
                    equal = bool(np.array_equal(dev[0], want[0]) and np.array_equal(dev[1].view(np.uint32), want[1].view(np.uint32)))
                    if not equal:
                        raise SystemExit("best: the host restatement and the device disagree")
                emit({"rows": a.rows, "dim": a.dim, "logical": NQ, "P": P, "N": N, "limit": LIMIT, "strategy": strategy,
                      "plain_search_batch_256": summary(plain_ms), "recommend_batch": summary(rec_ms),
                      "full_lists": int(sum(len(h) == LIMIT for h in hits)), "rounds": rounds,
                      "host_read_rows_and_numpy": summary(host) if host else None, "host_equals_device": equal})

    asyncio.run(run())
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
