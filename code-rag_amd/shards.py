"""Row shards of one collection behind ``HipVectorStore`` (BASELINE configs[3] / [4]: "corpus row-sharded across the GPUs").

``north_star`` keeps the reference's ``VectorStore`` surface (``embeddings/client.py:18-228``) and shards the corpus behind it;
this is the piece between the two.  A ``ShardSet`` looks like one index to ``store._Collection`` -- append, tombstone,
delete / count / match by filter, search, compact, save / load -- and spreads the rows over ``n`` ``crh_index`` handles:

* ``backend="local"``: all shards live in this process (on one device, or one per listed device).  What a one-GPU box can run;
  the search is n scans -> ``crh_merge_topk_strided`` on the device.
* ``backend="dist"``: one process per GPU under ``torch.distributed`` (``nccl`` = RCCL over xGMI); every rank makes the SAME
  calls and owns shard ``rank``: its rows' vectors, and -- since round 4 -- their embedding work and their payload TEXT
  (``append`` takes the rows of the owned shards only; ``exchange_bytes`` completes what only an owner holds).  Ids, the coded
  payload columns and the slot maps stay replicated.  The search is the path of ``sharded.ShardedIndex``: local scan with
  ``row_base``, ONE all-gather of the ``[scores | rows]`` records, merge on every rank.  Counts, matching rows and compaction maps travel in tensor
  collectives as well (round 4; a compaction map is one entry per row).  An append's outcome is agreed in ONE one-integer all-reduce;
  only a FAILED append exchanges small host objects (the reason, and the rows that landed before the failure).

Rows are dealt to the shards in blocks of ``block`` rows, round robin, so shards stay balanced under incremental upserts.
A row's global id is ``shard * STRIDE + local row`` (``STRIDE`` = 2^32, a ``crh_index`` holds at most 2^31 rows): stable under
appends and capacity growth.  Ties between equal scores go to the lower global id (lower shard first) -- Qdrant leaves tie
order unspecified.
"""

from __future__ import annotations

import os
from typing import Any, Callable, Sequence

import numpy as np

from . import ffi

STRIDE = 1 << 32


class AppendFailed(RuntimeError):
    """An append that failed after some shards had taken their rows: ``done`` = {shard: (first local row, rows)} of the rows
    that ARE on the device (tombstoned by the time this is raised); the caller's slot maps must step over them."""

    def __init__(self, cause: BaseException, done: dict[int, tuple[int, int]]):
        super().__init__(f"append failed: {cause!r}")
        self.cause, self.done = cause, done


class ShardSet:
    def __init__(self, nshards: int, make_index: Callable[[int], Any], device: int = 0, backend: str = "local", group=None,
                 block: int = 4096, merge_fn: Callable | None = None):
        if nshards < 1:
            raise ValueError("a collection needs at least one shard")
        self.ns, self.block, self.device, self._merge_host = int(nshards), int(block), device, merge_fn
        self.backend, self.group, self.dist, self.rank = backend, group, None, None
        if backend == "dist":
            import torch.distributed as dist
            if not dist.is_initialized():
                raise RuntimeError("shard backend 'dist' needs an initialised torch.distributed process group (one process per GPU)")
            if dist.get_world_size(group) != self.ns:
                raise ValueError(f"{self.ns} shards but a process group of {dist.get_world_size(group)} ranks")
            self.dist, self.rank = dist, dist.get_rank(group)
            self.owned = [self.rank]
        elif backend == "local":
            self.owned = list(range(self.ns))
        else:
            raise ValueError(f"unknown shard backend {backend!r} (use 'local' or 'dist')")
        self.index = {s: make_index(s) for s in self.owned}
        self.stream = 0                           # raw hipStream_t of the stream searches run on (0: the default stream); the store sets it
        self.rows = [0] * self.ns                 # rows appended to every shard so far (replicated bookkeeping: same on every rank)
        self._next_block = 0
        first = self.index[self.owned[0]]
        self.dim, self.dtype = first.dim, first.dtype

    # ------------------------------------------------------------------ plumbing
    def _everyone(self, mine: Any) -> list:
        """``mine`` of every rank, in rank order (backend "dist"); a one-element list otherwise."""
        if self.dist is None:
            return [mine]
        out = [None] * self.ns
        self.dist.all_gather_object(out, mine, group=self.group)
        return out

    def _tensor_device(self):
        import torch
        return torch.device("cuda", self.device) if self.dist.get_backend(self.group) == "nccl" else torch.device("cpu")

    def _sum_everyone(self, value: int) -> int:
        """Sum of one integer per rank: ONE tensor all-reduce (counts of deleted / matching / alive rows)."""
        if self.dist is None:
            return int(value)
        import torch
        t = torch.tensor([int(value)], dtype=torch.int64, device=self._tensor_device())
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group)
        return int(t.item())

    def _arrays_everyone(self, mine: dict[int, np.ndarray]) -> dict[int, np.ndarray]:
        """{shard: int64 array} of every rank, united -- two tensor collectives (lengths, then the padded arrays) instead of
        pickled objects: compaction maps are one entry per ROW (80 MB per 10M-row shard)."""
        if self.dist is None:
            return {s: np.asarray(a, np.int64) for s, a in mine.items()}
        import torch
        dev = self._tensor_device()
        arr = np.asarray(mine[self.rank], np.int64) if self.rank in mine else np.zeros((0,), np.int64)
        lens = torch.zeros((self.ns,), dtype=torch.int64, device=dev)
        self.dist.all_gather_into_tensor(lens, torch.tensor([arr.size], dtype=torch.int64, device=dev), group=self.group)
        lens_h = lens.cpu().numpy()
        width = max(1, int(lens_h.max()))
        pad = np.zeros((width,), np.int64)
        pad[:arr.size] = arr
        out = torch.empty((self.ns, width), dtype=torch.int64, device=dev)
        self.dist.all_gather_into_tensor(out.view(-1), torch.from_numpy(pad).to(dev), group=self.group)
        out_h = out.cpu().numpy()
        return {r: out_h[r, : int(lens_h[r])].copy() for r in range(self.ns)}

    def barrier(self) -> None:
        if self.dist is not None:
            self.dist.barrier(group=self.group)

    @property
    def capacity_rows(self) -> int:
        return sum(ix.capacity_rows for ix in self.index.values())

    def count(self) -> tuple[int, int]:
        alive = self._sum_everyone(sum(ix.count()[1] for ix in self.index.values()))
        return sum(self.rows), int(alive)

    # ------------------------------------------------------------------ build
    def route(self, n: int) -> np.ndarray:
        """Shard of each of the next ``n`` appended rows: blocks of ``block`` rows, round robin, continuing where the previous
        append stopped."""
        if self.ns == 1:
            return np.zeros((n,), np.int32)
        blocks = (n + self.block - 1) // self.block
        sh = (np.arange(blocks, dtype=np.int64) + self._next_block) % self.ns
        self._next_block = int((self._next_block + blocks) % self.ns)
        return np.repeat(sh, self.block)[:n].astype(np.int32)

    def append(self, vecs, codes, preprocessed: bool = False, stream: int = 0, shard: np.ndarray | None = None,
               failure: BaseException | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Append n rows.  ``vecs``: numpy [n, dim] or a CUDA tensor holding ALL n rows -- or, with ``shard`` (the routing of the
        n rows, from :meth:`route`), a dict {owned shard: its rows in order}: the form a rank uses when it has embedded only its
        own share.  ``codes``: numpy [n, cols] for all n rows, or None.  Returns (shard [n], local row [n]).

        Nothing is committed until every owned shard has the capacity; if a shard's append still fails, the rows the earlier
        shards took are tombstoned and :class:`AppendFailed` tells the caller where they sit.  Under backend "dist" the ranks
        agree on the outcome before anyone returns (one one-integer all-reduce when all is well).

        ``failure``: an error this process met while PREPARING its rows (its share of the texts would not embed): nothing is
        appended here, but the call is still made so that every rank takes part in the same agreement and leaves the same way --
        a rank that raised before this point would leave the others waiting in the collective."""
        per_shard = isinstance(vecs, dict)
        if per_shard and shard is None:
            raise ValueError("per-shard rows need the routing they were cut by")
        n = int(len(shard) if shard is not None else vecs.shape[0])
        saved_next = self._next_block
        if shard is None:
            shard = self.route(n)
        local = np.empty((n,), np.int64)
        plan = []                                     # (shard, rows of the call, first local row)
        for s in range(self.ns):
            sel = np.flatnonzero(shard == s) if self.ns > 1 else np.arange(n)
            if sel.size:
                local[sel] = self.rows[s] + np.arange(sel.size)
                plan.append((s, sel, self.rows[s]))
        done: dict[int, tuple[int, int]] = {}
        try:
            if failure is not None:
                raise failure
            for s, sel, first in plan:                # capacity first, on every owned shard: a refusal here leaves nothing behind
                if s in self.index and first + sel.size > self.index[s].capacity_rows:
                    self.index[s].reserve(max(first + int(sel.size), 2 * self.index[s].capacity_rows))
            for s, sel, first in plan:
                if s not in self.index:
                    continue
                ix = self.index[s]
                if per_shard:
                    v = vecs[s]
                elif self.ns == 1:
                    v = vecs
                elif isinstance(vecs, np.ndarray):
                    v = vecs[sel]
                else:
                    import torch
                    v = vecs.index_select(0, torch.from_numpy(sel).to(vecs.device))
                if int(v.shape[0]) != sel.size:
                    raise ValueError(f"shard {s}: {int(v.shape[0])} rows for {sel.size} routed to it")
                c = None if codes is None else (codes if self.ns == 1 else codes[sel])
                on_dev = not isinstance(v, np.ndarray)
                if on_dev and c is not None:
                    import torch
                    c = torch.from_numpy(np.ascontiguousarray(c)).to(v.device)
                got = ix.append(v, c, stream=stream, preprocessed=preprocessed) if on_dev else ix.append(v, c, preprocessed=preprocessed)
                done[s] = (int(got), int(sel.size))
                if got != first:
                    raise RuntimeError(f"shard {s}: append landed at row {got}, the bookkeeping expected {first}")
        except BaseException as e:  # noqa: BLE001 -- rolled back below, then re-raised
            failure = e
        if self.dist is not None:                     # one rank's failure is everybody's: the replicated bookkeeping must not part ways
            if self._sum_everyone(0 if failure is None else 1):
                outcomes = self._everyone(None if failure is None else repr(failure))
                if failure is None:
                    failure = RuntimeError(f"append failed on another rank: {[o for o in outcomes if o is not None][0]}")
        if failure is not None:
            for s, (got, m) in done.items():          # the rows that did land: dead, and accounted for
                self.index[s].tombstone(np.arange(got, got + m, dtype=np.int64))
            all_done: dict[int, tuple[int, int]] = {}
            for part in self._everyone(done):
                all_done.update(part)
            for s, (got, m) in all_done.items():
                self.rows[s] = got + m
            self._next_block = saved_next if not all_done else self._next_block
            if all_done:
                raise AppendFailed(failure, all_done) from failure
            raise failure
        for s, sel, first in plan:
            self.rows[s] = first + int(sel.size)
        return shard, local

    def exchange_bytes(self, parts: list) -> list:
        """``parts[i]``: bytes where THIS rank holds item i, None elsewhere (every item is held by exactly one rank, and every rank
        passes a list of the same length).  Returns the complete list on every rank -- two tensor all-reduces (lengths, then one
        byte buffer), no pickled objects: what a search's hits need from the ranks that own their payload text."""
        if self.dist is None:
            return parts
        import torch
        dev = torch.device("cuda", self.device) if self.dist.get_backend(self.group) == "nccl" else torch.device("cpu")
        lens = torch.tensor([0 if p is None else len(p) for p in parts], dtype=torch.int64, device=dev)
        self.dist.all_reduce(lens, op=self.dist.ReduceOp.SUM, group=self.group)
        lens_h = lens.cpu().numpy()
        off = np.zeros((len(parts) + 1,), np.int64)
        np.cumsum(lens_h, out=off[1:])
        buf = np.zeros((max(int(off[-1]), 1),), np.uint8)
        for i, p in enumerate(parts):
            if p:
                if len(p) != int(lens_h[i]):
                    raise RuntimeError("exchange_bytes: an item is held by more than one rank")
                buf[off[i]:off[i + 1]] = np.frombuffer(p, np.uint8)
        t = torch.from_numpy(buf).to(dev)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group)
        out_b = t.cpu().numpy().tobytes()
        return [out_b[off[i]:off[i + 1]] for i in range(len(parts))]

    def tombstone(self, shard: np.ndarray, local: np.ndarray) -> None:
        for s, ix in self.index.items():
            sel = local[shard == s] if self.ns > 1 else local
            if len(sel):
                ix.tombstone(np.asarray(sel, np.int64))

    # A filter (``dfilt``) is a list of conditions as ``ffi.Index`` takes them: ``(column, code)`` equalities and
    # ``(column, codes, negate)`` sets and ``(column, lo, hi, "between" | "not_between")`` ranges.  It travels to every shard as it is -- in this process or, under backend "dist", in the
    # same call every rank makes -- so set conditions need nothing of the collectives.
    def _plans(self, dfilt) -> list:
        """``[dfilt]`` -- or, for injected indexes that know equalities only (no ``SET_CONDITIONS``), the disjoint equality
        filters whose union it is: one per combination of the sets' codes (a negated set has no such form)."""
        if all(getattr(ix, "SET_CONDITIONS", False) for ix in self.index.values()) or not any(ffi.is_set_condition(c) for c in dfilt or []):
            return [dfilt]
        plans: list[list] = [[]]
        for cond in dfilt:
            if not ffi.is_set_condition(cond):
                opts = [(cond[0], cond[1])]
            elif len(cond) == 3 and cond[2]:
                raise ValueError("this index takes equality filters only: no 'not in' condition")
            elif ffi.is_range_condition(cond):
                raise ValueError("this index takes equality filters only: no range condition")
            else:
                opts = [(cond[0], int(c)) for c in sorted(set(cond[1]))]
            plans = [p + [o] for p in plans for o in opts]
        return plans

    def tombstone_filter(self, dfilt) -> int:
        return self._sum_everyone(sum(ix.tombstone_filter(p) for ix in self.index.values() for p in self._plans(dfilt)))

    def count_matching(self, dfilt) -> int:
        return self._sum_everyone(sum(ix.count_matching(p) for ix in self.index.values() for p in self._plans(dfilt)))

    def match_rows(self, dfilt, limit: int) -> tuple[np.ndarray, np.ndarray]:
        """(shard, local row) of up to ``limit`` alive matching rows PER SHARD, ascending inside each shard (a caller that wants
        the first ``limit`` in insertion order sorts the union by slot and cuts)."""
        allr = self._arrays_everyone({s: ix.match_rows(dfilt, limit) for s, ix in self.index.items()})
        sh = np.concatenate([np.full((len(allr[s]),), s, np.int32) for s in sorted(allr)]) if allr else np.zeros((0,), np.int32)
        lo = np.concatenate([np.asarray(allr[s], np.int64) for s in sorted(allr)]) if allr else np.zeros((0,), np.int64)
        return sh, lo

    # ------------------------------------------------------------------ query
    def search(self, queries: np.ndarray, k: int, dfilt) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Exact top-k over all shards: (scores [nq, k], shard [nq, k], local row [nq, k]); -1 rows are padding."""
        if self.ns == 1:
            s, r = self.index[0].search(queries, k, filters=dfilt, **({"stream": self.stream} if self.stream else {}))
            return s, np.zeros(r.shape, np.int32), r
        if self._merge_host is not None:            # injected host-side index + merge (CPU test tier)
            scores, rows = self._search_host(queries, k, dfilt)
        else:
            sd, rd = self.search_device(queries, k, dfilt)
            scores, rows = sd.cpu().numpy(), rd.cpu().numpy()
        return scores, np.where(rows >= 0, rows // STRIDE, 0).astype(np.int32), np.where(rows >= 0, rows % STRIDE, -1)

    def search_multi(self, queries: np.ndarray, k: int, class_filters, query_class) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """:meth:`search` for a batch whose queries carry different filters (``ffi.Index.search_multi``): query ``i`` under
        ``class_filters[query_class[i]]``.  The same per-shard plan as :meth:`search` -- every shard answers the whole batch
        under the same classes, [one all-gather,] one merge."""
        multi = (list(class_filters), np.asarray(query_class, np.int32))
        if self.ns == 1:
            s, r = self.index[0].search_multi(queries, k, *multi, **({"stream": self.stream} if self.stream else {}))
            return s, np.zeros(r.shape, np.int32), r
        if self._merge_host is not None:
            scores, rows = self._search_host(queries, k, None, multi)
        else:
            sd, rd = self.search_device(queries, k, None, multi)
            scores, rows = sd.cpu().numpy(), rd.cpu().numpy()
        return scores, np.where(rows >= 0, rows // STRIDE, 0).astype(np.int32), np.where(rows >= 0, rows % STRIDE, -1)

    @staticmethod
    def _shard_search(ix, queries, k, dfilt, multi, **kw):
        """One shard's part of a search: under one filter, or -- ``multi`` = (class_filters, query_class) -- under every query's own."""
        if multi is None:
            return ix.search(queries, k, filters=dfilt, **kw)
        return ix.search_multi(queries, k, multi[0], multi[1], **kw)

    def _search_host(self, queries, k, dfilt, multi=None):
        nq = int(queries.shape[0])
        mine = {s: self._shard_search(ix, queries, k, dfilt, multi, row_base=s * STRIDE) for s, ix in self.index.items()}
        if self.dist is None:
            parts = mine
        else:                                        # the same single all-gather of [scores | rows] records as on the device
            import torch
            local, loc_s, loc_r, gathered, all_s, all_r = ffi.topk_exchange_buffers(torch, self.ns, nq, k, torch.device("cpu"))
            ms, mr = mine[self.rank]
            loc_s.copy_(torch.from_numpy(np.ascontiguousarray(ms)))
            loc_r.copy_(torch.from_numpy(np.ascontiguousarray(mr)))
            self.dist.all_gather_into_tensor(gathered.view(-1), local, group=self.group)
            return self._merge_host(all_s.numpy(), all_r.numpy())
        ss = np.stack([parts[s][0] for s in range(self.ns)])
        rr = np.stack([parts[s][1] for s in range(self.ns)])
        return self._merge_host(ss, rr)

    def search_device(self, queries, k: int, dfilt, multi=None):
        """The same on the device, results left there: (scores f32 [nq, k], GLOBAL rows i64 [nq, k]) CUDA tensors -- per-shard
        ``crh_search`` with ``row_base`` = shard * STRIDE, [one all-gather of the records,] ``crh_merge_topk_strided``.
        ``multi`` = (class_filters, query_class): every query under its own filter (``crh_search_multi``), ``dfilt`` unused."""
        import torch
        dev = torch.device("cuda", self.device)
        ffi.use_device(self.device)
        stream = torch.cuda.current_stream(dev).cuda_stream
        qd = queries if torch.is_tensor(queries) else torch.from_numpy(np.ascontiguousarray(queries, dtype=np.float32)).to(dev)
        nq = int(qd.shape[0])
        local, loc_s, loc_r, gathered, all_s, all_r = ffi.topk_exchange_buffers(torch, self.ns, nq, k, dev)
        if self.dist is None:
            for s, ix in self.index.items():         # every shard writes its own record of the "gathered" buffer
                self._shard_search(ix, qd, k, dfilt, multi, row_base=s * STRIDE, out_scores=all_s[s], out_rows=all_r[s], stream=stream)
            for ix in self.index.values():
                ix.search_finish(stream)
        else:
            ix = self.index[self.rank]
            self._shard_search(ix, qd, k, dfilt, multi, row_base=self.rank * STRIDE, out_scores=loc_s, out_rows=loc_r, stream=stream)
            ix.search_finish(stream)
            self.dist.all_gather_into_tensor(gathered.view(-1), local, group=self.group)
        out_s = torch.empty((nq, k), dtype=torch.float32, device=dev)
        out_r = torch.empty((nq, k), dtype=torch.int64, device=dev)
        ffi.merge_topk(all_s, all_r, out_s, out_r, stream)
        return out_s, out_r

    # ------------------------------------------------------------------ score threshold and in-range counts
    def complete_counts(self, counts) -> None:
        """In-range counts of a range search: every rank summed its own shards; ONE all-reduce(sum) of the ``[nq]`` int64 vector
        completes them.  Like :meth:`complete_vectors` it has never run on more than one RCCL rank: the two-rank form is
        exercised with gloo on host tensors only."""
        if self.dist is not None:
            self.dist.all_reduce(counts, op=self.dist.ReduceOp.SUM, group=self.group)

    def search_range_device(self, queries, k: int, thresholds, dfilt, counts: bool = True):
        """The range search on the device, results left there: every shard runs ``crh_search_range`` with ``row_base`` =
        shard * STRIDE, the lists merge as in :meth:`search_device` (a shard's cut list is padded, and padding merges as it does
        there: the merged list is the first ``min(k, count)`` in-range rows of the whole collection), the counts are summed over
        the local shards and, under backend "dist", completed by :meth:`complete_counts`.  Returns CUDA tensors ``(scores f32
        [nq, k], GLOBAL rows i64 [nq, k], counts i64 [nq] or None)``."""
        import torch
        dev = torch.device("cuda", self.device)
        ffi.use_device(self.device)
        stream = torch.cuda.current_stream(dev).cuda_stream
        qd = queries if torch.is_tensor(queries) else torch.from_numpy(np.ascontiguousarray(queries, dtype=np.float32)).to(dev)
        nq = int(qd.shape[0])
        thr = ffi.range_thresholds(thresholds, nq)
        local, loc_s, loc_r, gathered, all_s, all_r = ffi.topk_exchange_buffers(torch, self.ns, nq, k, dev)
        part = torch.zeros((len(self.owned), nq), dtype=torch.int64, device=dev) if counts else None
        for i, s in enumerate(self.owned):           # every local shard writes its own record of the "gathered" buffer
            on = self.dist is None
            self.index[s].search_range(qd, k, thr, filters=dfilt, row_base=s * STRIDE, counts=counts, out_scores=all_s[s] if on else loc_s,
                                       out_rows=all_r[s] if on else loc_r, out_counts=part[i] if counts else None, stream=stream)
        for s in self.owned:
            self.index[s].search_finish(stream)
        if self.dist is not None:
            self.dist.all_gather_into_tensor(gathered.view(-1), local, group=self.group)
        total = None
        if counts:
            total = part.sum(0)
            self.complete_counts(total)
        out_s = torch.empty((nq, k), dtype=torch.float32, device=dev)
        out_r = torch.empty((nq, k), dtype=torch.int64, device=dev)
        ffi.merge_topk(all_s, all_r, out_s, out_r, stream)
        return out_s, out_r, total

    def search_range(self, queries: np.ndarray, k: int, thresholds, dfilt, counts: bool = True):
        """:meth:`search` with a score threshold per query: ``(scores [nq, k], shard [nq, k], local row [nq, k], counts int64
        [nq] or None)``; -1 rows are padding.  One native shard answers directly; several take :meth:`search_range_device`;
        injected host-side indexes (CPU test tier) run the same steps on numpy arrays."""
        nq = int(np.asarray(queries).shape[0]) if not hasattr(queries, "is_cuda") else int(queries.shape[0])
        thr = ffi.range_thresholds(thresholds, nq)
        if self.ns == 1:
            s, r, c = self.index[0].search_range(queries, k, thr, filters=dfilt, counts=counts, **({"stream": self.stream} if self.stream else {}))
            return s, np.zeros(r.shape, np.int32), r, c
        if self._merge_host is None:
            sd, rd, cd = self.search_range_device(queries, k, thr, dfilt, counts)
            scores, rows, total = sd.cpu().numpy(), rd.cpu().numpy(), (cd.cpu().numpy() if counts else None)
        else:
            mine = {s: ix.search_range(queries, k, thr, filters=dfilt, row_base=s * STRIDE, counts=counts) for s, ix in self.index.items()}
            total = sum(np.asarray(m[2], np.int64) for m in mine.values()) if counts else None
            if self.dist is None:
                ss = np.stack([mine[s][0] for s in range(self.ns)])
                rr = np.stack([mine[s][1] for s in range(self.ns)])
            else:                                        # the list records travel as in _search_host, the counts in one all-reduce
                import torch
                local, loc_s, loc_r, gathered, all_s, all_r = ffi.topk_exchange_buffers(torch, self.ns, nq, k, torch.device("cpu"))
                loc_s.copy_(torch.from_numpy(np.ascontiguousarray(mine[self.rank][0])))
                loc_r.copy_(torch.from_numpy(np.ascontiguousarray(mine[self.rank][1])))
                self.dist.all_gather_into_tensor(gathered.view(-1), local, group=self.group)
                ss, rr = all_s.numpy(), all_r.numpy()
                if counts:
                    t = torch.from_numpy(np.ascontiguousarray(total, dtype=np.int64))
                    self.complete_counts(t)
                    total = t.numpy()
            scores, rows = self._merge_host(ss, rr)
        return scores, np.where(rows >= 0, rows // STRIDE, 0).astype(np.int32), np.where(rows >= 0, rows % STRIDE, -1), total

    def complete_columns(self, packed) -> None:
        """Side columns of a merged candidate table: every rank gathered the rows it owns (zeros elsewhere); ONE all-reduce of
        the packed buffer completes them (``sharded.ShardedIndex.gather_columns``).  Local shards are summed by the caller."""
        if self.dist is not None:
            self.dist.all_reduce(packed, op=self.dist.ReduceOp.SUM, group=self.group)

    # ------------------------------------------------------------------ diversity-aware top-k (MMR)
    def complete_vectors(self, vecs) -> None:
        """Candidate vectors of a merged list: every rank gathered the rows it owns (zeros elsewhere); ONE all-reduce(sum)
        completes them, as :meth:`complete_columns` does for the side columns.  It moves ``nq * candidates * dim * 4`` bytes
        (3 MB for one 768-wide query at 1024 candidates) and has never run on more than one RCCL rank: the two-rank form is
        exercised with gloo on host tensors only."""
        if self.dist is not None:
            self.dist.all_reduce(vecs, op=self.dist.ReduceOp.SUM, group=self.group)

    def search_mmr_device(self, queries, k: int, candidates: int, diversity: float, dfilt):
        """Diversity-aware top-k on the device, results left there: :meth:`search_device` for ``candidates`` hits per query,
        every local shard gathers the stored vectors of the rows it owns into one ``[nq, candidates, dim]`` buffer (a row has
        one owner and the others contribute zeros: the local shards' gathers are summed, and under backend "dist" one
        all-reduce(sum) of ``nq * candidates * dim * 4`` bytes completes the buffer -- :meth:`complete_vectors`; never run on
        more than one RCCL rank), then ``crh_mmr_select``.  Returns CUDA tensors ``(pos i32, GLOBAL rows i64, scores f32,
        obj f32)``, each [nq, k]; ``scores`` are the hits' cosines, -1 rows are padding."""
        import torch
        cs, cr = self.search_device(queries, candidates, dfilt)
        stream = torch.cuda.current_stream(cs.device).cuda_stream
        vecs = None
        for s in self.owned:
            part = self.index[s].gather_vectors(cr, row_base=s * STRIDE, stream=stream)
            if vecs is None:
                vecs = part
            else:
                vecs += part
        self.complete_vectors(vecs)
        return ffi.mmr_select(cs, cr, vecs, k, diversity, stream=stream)

    def search_mmr(self, queries: np.ndarray, k: int, candidates: int, diversity: float, dfilt) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """:meth:`search` with diversity: (scores [nq, k], shard [nq, k], local row [nq, k]) of the MMR picks among the
        ``candidates`` best hits of every query; -1 rows are padding.  Indexes that hold a native handle take
        :meth:`search_mmr_device`; injected host-side indexes (CPU test tier) run the same steps on numpy arrays."""
        if all(hasattr(ix, "_handle") for ix in self.index.values()):
            _, rd, sd, _ = self.search_mmr_device(queries, k, candidates, diversity, dfilt)
            scores, rows = sd.cpu().numpy(), rd.cpu().numpy()
        else:
            if self.ns == 1:
                cs, cr = self.index[0].search(queries, candidates, filters=dfilt)
            else:
                cs, cr = self._search_host(queries, candidates, dfilt)
            cs, cr = np.asarray(cs, np.float32), np.asarray(cr, np.int64)
            vecs = sum(self.index[s].gather_vectors(cr, row_base=s * STRIDE) for s in self.owned)
            if self.dist is not None:
                import torch
                t = torch.from_numpy(np.ascontiguousarray(vecs, dtype=np.float32))
                self.complete_vectors(t)
                vecs = t.numpy()
            _, rows, scores, _ = ffi.mmr_select(cs, cr, vecs, k, diversity)
            scores, rows = np.asarray(scores), np.asarray(rows)
        return scores, np.where(rows >= 0, rows // STRIDE, 0).astype(np.int32), np.where(rows >= 0, rows % STRIDE, -1)

    # ------------------------------------------------------------------ per-group cap (group_by / group_size)
    def complete_codes(self, codes) -> None:
        """Group codes of a merged candidate list: the buffer starts full of -1 and every rank wrote the codes of the rows it
        owns (stored codes are >= -1, a row has one owner); ONE all-reduce(MAX) of ``nq * candidates`` int32 completes it.
        Like :meth:`complete_vectors` it has never run on more than one RCCL rank: the two-rank form is exercised with gloo
        on host tensors only."""
        if self.dist is not None:
            self.dist.all_reduce(codes, op=self.dist.ReduceOp.MAX, group=self.group)

    def search_grouped_device(self, queries, k: int, candidates: int, col: int, group_size: int, dfilt, ungrouped: int | None = None):
        """The capped walk on the device, results left there: :meth:`search_device` for ``candidates`` hits per query, every
        local shard writes the column-``col`` codes of the rows it owns into one ``[nq, candidates]`` int32 buffer pre-filled
        with -1 (:meth:`complete_codes` finishes it under backend "dist"), then ``crh_group_select``.  ``ungrouped``: a code
        that names no group (the store's code of "no value"): candidates that carry it are never capped.  Returns CUDA tensors
        ``(pos i32, GLOBAL rows i64, scores f32, codes i32)``, each [nq, k], and ``info`` i32 [nq, 2] = (kept, real)."""
        import torch
        cs, cr = self.search_device(queries, candidates, dfilt)
        stream = torch.cuda.current_stream(cs.device).cuda_stream
        codes = torch.full(tuple(cr.shape), -1, dtype=torch.int32, device=cr.device)
        for s in self.owned:
            self.index[s].gather_codes(cr, col, row_base=s * STRIDE, out=codes, stream=stream)
        self.complete_codes(codes)
        if ungrouped is not None:
            codes.masked_fill_(codes == int(ungrouped), -1)
        return ffi.group_select(cs, cr, codes, k, group_size, stream=stream)

    def search_grouped(self, queries: np.ndarray, k: int, candidates: int, col: int, group_size: int, dfilt, ungrouped: int | None = None):
        """One round of the grouped search as host arrays: ``(scores f32 [nq, k], GLOBAL rows i64 [nq, k], codes i32 [nq, k],
        info i32 [nq, 2])`` -- the first ``k`` of the ``candidates`` best hits whose rank in their column-``col`` group is below
        ``group_size`` (a candidate whose code is negative or ``ungrouped`` is never capped and comes back with code -1); -1 rows
        are padding; ``info`` = (kept in the whole list, real candidates), what the store's exactness
        rounds decide on.  Indexes that hold a native handle take :meth:`search_grouped_device`; injected host-side indexes
        (CPU test tier) run the same steps on numpy arrays."""
        if all(hasattr(ix, "_handle") for ix in self.index.values()):
            _, rd, sd, cd, info = self.search_grouped_device(queries, k, candidates, col, group_size, dfilt, ungrouped)
            return sd.cpu().numpy(), rd.cpu().numpy(), cd.cpu().numpy(), info.cpu().numpy()
        if self.ns == 1:
            cs, cr = self.index[0].search(queries, candidates, filters=dfilt)
        else:
            cs, cr = self._search_host(queries, candidates, dfilt)
        cs, cr = np.asarray(cs, np.float32), np.asarray(cr, np.int64)
        codes = np.full(cr.shape, -1, np.int32)
        for s in self.owned:
            self.index[s].gather_codes(cr, col, row_base=s * STRIDE, out=codes)
        if self.dist is not None:
            import torch
            t = torch.from_numpy(codes)
            self.complete_codes(t)
            codes = t.numpy()
        if ungrouped is not None:
            codes = np.where(codes == int(ungrouped), -1, codes).astype(np.int32)
        _, rows, scores, gcodes, info = ffi.group_select(cs, cr, codes, k, group_size)
        return np.asarray(scores, np.float32), np.asarray(rows, np.int64), np.asarray(gcodes, np.int32), np.asarray(info, np.int32)

    # ------------------------------------------------------------------ overlap-free hit lists (max_overlap)
    def search_spans_device(self, queries, k: int, candidates: int, cols: tuple[int, int, int], permille: int, dfilt, no_file: int | None = None):
        """The overlap-free walk on the device, results left there: :meth:`search_device` for ``candidates`` hits per query,
        every local shard writes the codes of the columns ``cols`` = (file, first line, last line) of the rows it owns into
        one ``[3, nq, candidates]`` int32 buffer pre-filled with -1 (ONE :meth:`complete_codes` -- all-reduce(MAX) -- finishes
        the three under backend "dist"), then ``crh_span_select``.  ``no_file``: the file code that names no file (the store's
        code of "no value"): candidates that carry it have no span.  Returns CUDA tensors ``(pos i32, GLOBAL rows i64, scores
        f32, file i32, lo i32, hi i32)``, each [nq, k], and ``info`` i32 [nq, 2] = (kept, real)."""
        import torch
        cs, cr = self.search_device(queries, candidates, dfilt)
        stream = torch.cuda.current_stream(cs.device).cuda_stream
        codes = torch.full((3,) + tuple(cr.shape), -1, dtype=torch.int32, device=cr.device)
        for s in self.owned:
            for i, col in enumerate(cols):
                self.index[s].gather_codes(cr, col, row_base=s * STRIDE, out=codes[i], stream=stream)
        self.complete_codes(codes)
        if no_file is not None:
            codes[0].masked_fill_(codes[0] == int(no_file), -1)
        return ffi.span_select(cs, cr, codes[0], codes[1], codes[2], k, permille, stream=stream)

    def search_spans(self, queries: np.ndarray, k: int, candidates: int, cols: tuple[int, int, int], permille: int, dfilt, no_file: int | None = None):
        """One round of the ``max_overlap`` search as host arrays: ``(scores f32 [nq, k], GLOBAL rows i64 [nq, k], info i32
        [nq, 2])`` -- the first ``k`` of the ``candidates`` best hits that repeat at most ``permille`` thousandths of the shorter
        span of any better kept hit of their file; -1 rows are padding; ``info`` = (kept in the whole list, real candidates),
        what the store's exactness rounds decide on.  Indexes that hold a native handle take :meth:`search_spans_device`;
        injected host-side indexes (CPU test tier) run the same steps on numpy arrays."""
        if all(hasattr(ix, "_handle") for ix in self.index.values()):
            out = self.search_spans_device(queries, k, candidates, cols, permille, dfilt, no_file)
            return out[2].cpu().numpy(), out[1].cpu().numpy(), out[6].cpu().numpy()
        if self.ns == 1:
            cs, cr = self.index[0].search(queries, candidates, filters=dfilt)
        else:
            cs, cr = self._search_host(queries, candidates, dfilt)
        cs, cr = np.asarray(cs, np.float32), np.asarray(cr, np.int64)
        codes = np.full((3,) + cr.shape, -1, np.int32)
        for s in self.owned:
            for i, col in enumerate(cols):
                self.index[s].gather_codes(cr, col, row_base=s * STRIDE, out=codes[i])
        if self.dist is not None:
            import torch
            t = torch.from_numpy(codes)
            self.complete_codes(t)
            codes = t.numpy()
        if no_file is not None:
            codes[0] = np.where(codes[0] == int(no_file), -1, codes[0])
        out = ffi.span_select(cs, cr, codes[0], codes[1], codes[2], k, permille)
        return np.asarray(out[2], np.float32), np.asarray(out[1], np.int64), np.asarray(out[6], np.int32)

    # ------------------------------------------------------------------ multi-query fusion (RRF / best match)
    def search_fused_device(self, queries, k: int, candidates: int, dfilt, method: str = "rrf", rrf_k: int = 60, weights=None, live=None):
        """Fusion on the device, results left there: ``queries`` [nq, m, dim] -- the ``m`` sub-queries of ``nq`` logical ones --
        are searched as ``nq * m`` plain queries (:meth:`search_device`, ``candidates`` hits each: the merged lists carry
        GLOBAL rows), then ``crh_fuse_select`` turns every ``m`` lists into one.  ``live`` (bool [nq, m], host): the real
        members of ragged sets; the lists of the others are overwritten with padding before the fusion.  Under backend "dist"
        every rank holds the same merged lists and fuses them itself: no collective is added.  Returns CUDA tensors ``(GLOBAL
        rows i64, fused f32, cos f32, lists i32, first i32)``, each [nq, k], and ``info`` i32 [nq, 2] = (distinct, real)."""
        import torch
        nq, m = int(queries.shape[0]), int(queries.shape[1])
        flat = queries.reshape(nq * m, int(queries.shape[2]))
        cs, cr = self.search_device(flat, candidates, dfilt)
        stream = torch.cuda.current_stream(cs.device).cuda_stream
        if live is not None:
            dead = torch.from_numpy(~np.asarray(live, bool).reshape(nq * m)).to(cs.device)
            cs.masked_fill_(dead[:, None], float("-inf"))
            cr.masked_fill_(dead[:, None], -1)
        return ffi.fuse_select(cs, cr, m, k, method, rrf_k, weights, stream=stream)

    def search_fused(self, queries: np.ndarray, k: int, candidates: int, dfilt, method: str = "rrf", rrf_k: int = 60, weights=None, live=None):
        """:meth:`search_fused_device` as host arrays: ``(GLOBAL rows i64, fused f32, cos f32, lists i32, first i32)``, each
        [nq, k], and ``info`` i32 [nq, 2]; -1 rows are padding.  Indexes that hold a native handle take the device form;
        injected host-side indexes (CPU test tier) run the same steps on numpy arrays."""
        if all(hasattr(ix, "_handle") for ix in self.index.values()):
            return tuple(t.cpu().numpy() for t in self.search_fused_device(queries, k, candidates, dfilt, method, rrf_k, weights, live))
        queries = np.asarray(queries, np.float32)
        nq, m = int(queries.shape[0]), int(queries.shape[1])
        flat = np.ascontiguousarray(queries.reshape(nq * m, queries.shape[2]))
        if self.ns == 1:
            cs, cr = self.index[0].search(flat, candidates, filters=dfilt)
        else:
            cs, cr = self._search_host(flat, candidates, dfilt)
        cs, cr = np.array(cs, np.float32), np.array(cr, np.int64)
        if live is not None:
            dead = ~np.asarray(live, bool).reshape(nq * m)
            cs[dead], cr[dead] = -np.inf, -1
        return tuple(np.asarray(a) for a in ffi.fuse_select(cs, cr, m, k, method, rrf_k, weights))

    # ------------------------------------------------------------------ keyword search (BM25)
    # ``lex`` = {shard: ffi.Lex}: the forward indexes beside the owned shards, rows numbered like the shards' (the collection
    # builds and keeps them).  Tombstones and filters reach them as the validity words of ``Index.row_mask`` only.
    def _native(self) -> bool:
        return all(hasattr(ix, "_handle") for ix in self.index.values())

    def _stream(self) -> int:
        if not self._native():
            return 0
        import torch
        ffi.use_device(self.device)
        return torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream

    def lex_stats(self, lex: dict, terms) -> tuple[np.ndarray, int, int]:
        """``(df int64 per term, N, sum_dl)`` over the ALIVE rows of every shard, summed: the statistics of the whole
        collection, whatever filter a search runs under."""
        terms = np.ascontiguousarray(terms, dtype=np.uint32)
        df, rows, total = np.zeros(terms.size, np.int64), 0, 0
        for s, ix in self.index.items():
            if self.rows[s] == 0:
                continue
            mask = ix.row_mask(None)                 # (default stream, like the synchronous crh_lex_stats behind it)
            d, r, t = lex[s].stats(terms, mask)
            df, rows, total = df + d, rows + r, total + t
        return df, rows, total

    def lex_search_device(self, lex: dict, queries, idf, k: int, k1: float, b: float, avgdl: float, dfilt):
        """Exact BM25 top-k over all shards, results left where the indexes live: ``(scores f32 [nq, k], GLOBAL rows i64 [nq, k],
        counts i64 [nq])`` -- per shard ``crh_index_row_mask`` + ``crh_lex_search`` with ``row_base`` = shard * STRIDE, then
        ``crh_merge_topk_strided``; the counts are summed.  Injected host-side indexes (CPU test tier) return numpy arrays."""
        nq, native = len(queries), self._native()
        stream = self._stream()
        if native:
            import torch
            dev = torch.device("cuda", self.device)
            all_s = torch.full((self.ns, nq, k), float("-inf"), dtype=torch.float32, device=dev)
            all_r = torch.full((self.ns, nq, k), -1, dtype=torch.int64, device=dev)
            counts = torch.zeros((nq,), dtype=torch.int64, device=dev)
        else:
            all_s, all_r = np.full((self.ns, nq, k), -np.inf, np.float32), np.full((self.ns, nq, k), -1, np.int64)
            counts = np.zeros((nq,), np.int64)
        for s, ix in self.index.items():
            if self.rows[s] == 0:
                continue
            mask = ix.row_mask(dfilt, stream=stream)
            out = {"out_scores": all_s[s], "out_rows": all_r[s]} if native else {}      # (every shard writes its own part of the table)
            ps, pr, pc = lex[s].search(queries, idf, k, k1, b, avgdl, mask=mask, row_base=s * STRIDE, stream=stream, **out)
            if not native:
                all_s[s], all_r[s] = ps, pr
            counts += pc
        if self.ns == 1:
            return all_s[0], all_r[0], counts
        if not native:
            ms, mr = self._merge_host(all_s, all_r)
            return ms, mr, counts
        out_s = torch.empty((nq, k), dtype=torch.float32, device=dev)
        out_r = torch.empty((nq, k), dtype=torch.int64, device=dev)
        ffi.merge_topk(all_s, all_r, out_s, out_r, stream)
        return out_s, out_r, counts

    def lex_search(self, lex: dict, queries, idf, k: int, k1: float, b: float, avgdl: float, dfilt):
        """:meth:`lex_search_device` as host arrays."""
        return tuple(_host(a) for a in self.lex_search_device(lex, queries, idf, k, k1, b, avgdl, dfilt))

    def search_hybrid(self, lex: dict, vectors: np.ndarray, queries, idf, k: int, candidates: int, k1: float, b: float, avgdl: float,
                      dfilt, rrf_k: int = 60, weights=None):
        """Dense + keyword, fused: the dense top-``candidates`` (:meth:`search_device`) and the BM25 top-``candidates``
        (:meth:`lex_search_device`) of every query under the same filter, as ``[nq, 2, candidates]``, into ``crh_fuse_select``
        with ``m = 2`` and reciprocal-rank fusion.  Returns host arrays: the fusion's ``(GLOBAL rows, fused, cos, lists, first,
        info)`` and the two candidate tables ``(dense scores, dense rows, lexical scores, lexical rows)``."""
        nq = len(queries)
        if self._native():
            import torch
            ds, dr = self.search_device(vectors, candidates, dfilt)
            ls, lr, _ = self.lex_search_device(lex, queries, idf, candidates, k1, b, avgdl, dfilt)
            cs, cr = torch.stack([ds, ls], dim=1).contiguous(), torch.stack([dr, lr], dim=1).contiguous()
            fused = ffi.fuse_select(cs, cr, 2, k, "rrf", rrf_k, weights, stream=self._stream())
        else:
            vectors = np.ascontiguousarray(vectors, dtype=np.float32)
            ds, dr = self.index[0].search(vectors, candidates, filters=dfilt) if self.ns == 1 else self._search_host(vectors, candidates, dfilt)
            ls, lr, _ = self.lex_search_device(lex, queries, idf, candidates, k1, b, avgdl, dfilt)
            cs = np.stack([np.asarray(ds, np.float32), np.asarray(ls, np.float32)], axis=1).reshape(nq, 2, candidates)
            cr = np.stack([np.asarray(dr, np.int64), np.asarray(lr, np.int64)], axis=1).reshape(nq, 2, candidates)
            fused = ffi.fuse_select(cs, cr, 2, k, "rrf", rrf_k, weights)
        return tuple(_host(a) for a in fused), tuple(_host(a) for a in (ds, dr, ls, lr))

    # ------------------------------------------------------------------ recommend by example
    def rows_alive(self, shard: np.ndarray, local: np.ndarray) -> np.ndarray:
        """Whether every row (shard, local) is alive, from the owners' validity words (one all-reduce under backend "dist")."""
        shard, local = np.asarray(shard, np.int64), np.asarray(local, np.int64)
        out = np.zeros(local.shape, np.int64)
        for s in self.owned:
            m = shard == s
            if m.any():
                words = np.asarray(self.index[s].alive_words(), np.uint32)
                out[m] = (words[local[m] >> 5] >> (local[m] & 31).astype(np.uint32)) & 1
        if self.dist is not None:
            import torch
            t = torch.from_numpy(out).to(self._tensor_device())
            self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group)
            out = t.cpu().numpy()
        return out.astype(bool)

    def _gather_everywhere(self, rows_dev, stream):
        """Stored vectors of a table of GLOBAL rows, completed across the shards as :meth:`search_mmr_device` does."""
        vecs = None
        for s in self.owned:
            part = self.index[s].gather_vectors(rows_dev, row_base=s * STRIDE, stream=stream)
            if vecs is None:
                vecs = part
            else:
                vecs += part
        self.complete_vectors(vecs)
        return vecs

    def recommend_device(self, example_rows, P: int, N: int, k: int, candidates: int, dfilt, strategy: str = "average", n_pos=None, n_neg=None):
        """Recommend by example on the device, results left there.  ``example_rows`` (host int64 [nq, P + N]): the GLOBAL rows
        of every query's examples, positives first, -1 for an unused slot; ``n_pos`` / ``n_neg`` (host int [nq] or None) the
        live counts of ragged sets.  The examples' stored vectors are gathered across the shards (:meth:`complete_vectors`
        under backend "dist").  ``"average"``: ``crh_recommend_query`` makes one query per set, :meth:`search_device` answers it
        with ``candidates`` hits and ``crh_recommend_select`` drops the example rows.  ``"best"``: the ``nq * P`` positives are
        searched as plain device queries (``candidates`` hits each; the lists of absent positives are overwritten with
        padding), the candidates' vectors gathered, and ``crh_recommend_select`` applies the veto, ranks and counts the settled
        prefix.  Returns CUDA tensors ``(GLOBAL rows i64, score f32, neg f32, best i32)``, each [nq, k], ``info`` i32 [nq, 4] =
        (kept, settled, distinct, vetoed) and ``full`` bool [nq]: whether any of the query's lists came back full."""
        import torch
        code = ffi.recommend_strategy(strategy)
        dev = torch.device("cuda", self.device)
        ffi.use_device(self.device)
        stream = torch.cuda.current_stream(dev).cuda_stream
        er = torch.from_numpy(np.ascontiguousarray(example_rows, dtype=np.int64)).to(dev)
        nq, E = int(er.shape[0]), P + N
        examples = self._gather_everywhere(er, stream)                    # [nq, P + N, dim]
        bf16 = self.dtype == ffi.DTYPE_BF16
        if code == ffi.RECOMMEND_AVERAGE:
            q = ffi.recommend_query(examples, P, N, n_pos, n_neg, stream=stream)
            cs, cr = self.search_device(q, candidates, dfilt)
            cs, cr = cs.view(nq, 1, candidates), cr.view(nq, 1, candidates)
            vecs = None
        else:
            cs, cr = self.search_device(examples[:, :P].reshape(nq * P, self.dim), candidates, dfilt)
            if n_pos is not None:
                dead = torch.from_numpy((np.arange(P)[None, :] >= np.asarray(n_pos).reshape(nq, 1)).reshape(nq * P)).to(dev)
                cs.masked_fill_(dead[:, None], float("-inf"))
                cr.masked_fill_(dead[:, None], -1)
            vecs = self._gather_everywhere(cr, stream).view(nq, P * candidates, self.dim)
            cs, cr = cs.view(nq, P, candidates), cr.view(nq, P, candidates)
        full = (cr[:, :, -1] >= 0).any(1)
        return ffi.recommend_select(cs, cr, vecs, examples, er, P, N, k, strategy, bf16, n_pos, n_neg, stream=stream) + (full,)

    def _read_global(self, rows: np.ndarray) -> np.ndarray:
        """``read_rows`` of a table of GLOBAL rows on host arrays (zeros for padding and for rows of shards owned elsewhere,
        which :meth:`complete_vectors` adds)."""
        rows = np.asarray(rows, np.int64)
        out = np.zeros(rows.shape + (self.dim,), np.float32)
        flat_r, flat_o = rows.reshape(-1), out.reshape(-1, self.dim)
        for i in np.flatnonzero(flat_r >= 0):
            s, lo = int(flat_r[i] // STRIDE), int(flat_r[i] % STRIDE)
            if s in self.index:
                flat_o[i] = self.index[s].read_rows(lo, 1)[0]
        if self.dist is not None:
            import torch
            t = torch.from_numpy(out)
            self.complete_vectors(t)
        return out

    def recommend(self, example_rows, P: int, N: int, k: int, candidates: int, dfilt, strategy: str = "average", n_pos=None, n_neg=None):
        """:meth:`recommend_device` as host arrays: ``(GLOBAL rows i64, score f32, neg f32, best i32)``, each [nq, k], ``info``
        i32 [nq, 4] and ``full`` bool [nq]; -1 rows are padding.  Indexes that hold a native handle take the device form;
        injected host-side indexes (CPU test tier) run the same steps on numpy arrays out of ``search`` and ``read_rows``."""
        if all(hasattr(ix, "_handle") for ix in self.index.values()):
            return tuple(t.cpu().numpy() for t in self.recommend_device(example_rows, P, N, k, candidates, dfilt, strategy, n_pos, n_neg))
        code = ffi.recommend_strategy(strategy)
        er = np.ascontiguousarray(example_rows, dtype=np.int64)
        nq = int(er.shape[0])
        examples = self._read_global(er)

        def search(queries):
            if self.ns == 1:
                s, r = self.index[0].search(queries, candidates, filters=dfilt)
            else:
                s, r = self._search_host(queries, candidates, dfilt)
            return np.array(s, np.float32), np.array(r, np.int64)
        bf16 = self.dtype == ffi.DTYPE_BF16
        if code == ffi.RECOMMEND_AVERAGE:
            cs, cr = search(np.asarray(ffi.recommend_query(examples, P, N, n_pos, n_neg), np.float32))
            cs, cr, vecs = cs.reshape(nq, 1, candidates), cr.reshape(nq, 1, candidates), None
        else:
            cs, cr = search(np.ascontiguousarray(examples[:, :P].reshape(nq * P, self.dim)))
            if n_pos is not None:
                dead = (np.arange(P)[None, :] >= np.asarray(n_pos).reshape(nq, 1)).reshape(nq * P)
                cs[dead], cr[dead] = -np.inf, -1
            vecs = self._read_global(cr).reshape(nq, P * candidates, self.dim)
            cs, cr = cs.reshape(nq, P, candidates), cr.reshape(nq, P, candidates)
        full = (cr[:, :, -1] >= 0).any(1)
        return tuple(np.asarray(a) for a in ffi.recommend_select(cs, cr, vecs, examples, er, P, N, k, strategy, bf16, n_pos, n_neg)) + (full,)

    # ------------------------------------------------------------------ maintenance
    def compact(self) -> dict[int, np.ndarray]:
        """``crh_index_compact`` on every shard; returns {shard: old_to_new local rows} for ALL shards on every rank."""
        maps = self._arrays_everyone({s: ix.compact() for s, ix in self.index.items()})
        for s, o2n in maps.items():
            self.rows[s] = int((o2n >= 0).sum())
        return maps

    def stats(self) -> dict:
        out: dict[str, int] = {}
        for ix in self.index.values():
            for k, v in ix.stats().items():
                out[k] = (max(out.get(k, 0), v) if k in ("max_query_cands", "fallback_used") else out.get(k, 0) + v)
        return out

    def save(self, directory: str) -> None:
        for s, ix in self.index.items():
            ix.save(directory if self.ns == 1 else os.path.join(directory, f"shard{s}"))

    def load(self, directory: str, widen=None) -> None:
        """``widen(shard, first_row, rows)`` -> int32 ``[extra columns, rows]``: the snapshot's shards hold fewer code columns
        than these indexes (a collection snapshot from before the numeric columns); every imported chunk is completed with them."""
        for s, ix in self.index.items():
            sub = directory if self.ns == 1 else os.path.join(directory, f"shard{s}")
            if widen is None:
                ix.load(sub)
            else:
                ix.load(sub, widen=lambda first, rows, s=s: widen(s, first, rows))
        counts = self._arrays_everyone({s: np.asarray([ix.count()[0]], np.int64) for s, ix in self.index.items()})
        self.rows = [int(counts[s][0]) for s in range(self.ns)]

    def close(self) -> None:
        for ix in self.index.values():
            ix.close()


def _host(a) -> np.ndarray:
    """A device tensor or a host array as a host array."""
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def shard_sizes(rows: Sequence[int]) -> str:
    return "/".join(str(int(r)) for r in rows)
