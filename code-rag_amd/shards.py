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
    # Every search feature is ONE pipeline on arrays "where the indexes live" -- CUDA tensors for native indexes, numpy arrays
    # for the injected host-side indexes of the CPU test tier (whose ``ffi.*_select`` are numpy restatements):
    #   1. the top-c candidate lists with GLOBAL rows (_candidates: per-shard search, [one all-gather,] merge);
    #   2. optionally the lists of absent members overwritten with padding (_mask_lists);
    #   3. the candidates' codes or vectors gathered from the owning shards into a pre-filled buffer and completed by one
    #      all-reduce (_gather_codes, _gather_everywhere; reduce);
    #   4. one ``ffi.*_select``;  5. ``_host``.
    # Only the helpers of this first part know which kind of array they hold; no feature below does.
    def _native(self) -> bool:
        return all(hasattr(ix, "_handle") for ix in self.index.values())

    def _stream(self) -> int:
        if not self._native():
            return 0
        import torch
        ffi.use_device(self.device)
        return torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream

    def _local(self, a: np.ndarray):
        """A host array where the indexes live."""
        if not self._native():
            return a
        import torch
        return torch.from_numpy(a).to(torch.device("cuda", self.device))

    def _full(self, shape, value, dtype: str):
        """A buffer full of ``value`` where the indexes live."""
        if not self._native():
            return np.full(shape, value, dtype)
        import torch
        return torch.full(shape, value, dtype=getattr(torch, dtype), device=torch.device("cuda", self.device))

    def reduce(self, x, op: str):
        """The one all-reduce (``op``: "SUM" | "MAX") of a buffer every rank filled for the rows it owns, in place; nothing to
        do without ``dist``.  A host array travels as the tensor that shares its memory (gloo).  Candidate vectors (zeros
        elsewhere, SUM: ``nq * candidates * dim * 4`` bytes, 3 MB for one 768-wide query at 1024 candidates), codes (-1 elsewhere,
        stored codes are >= -1: MAX), in-range counts and the re-rank's side columns (SUM) are completed by it.  On more than one
        RCCL rank it has never run: the two-rank form is exercised with gloo on host tensors only."""
        if self.dist is not None:
            import torch
            self.dist.all_reduce(x if torch.is_tensor(x) else torch.from_numpy(x), op=getattr(self.dist.ReduceOp, op), group=self.group)
        return x

    @staticmethod
    def _shard_search(ix, queries, k, dfilt, multi, thr, **kw):
        """One shard's part of a search: under one filter; or -- ``multi`` = (class_filters, query_class) -- under every query's
        own; or -- ``thr`` -- with a score threshold per query (``counts`` among ``kw``)."""
        if thr is not None:
            return ix.search_range(queries, k, thr, filters=dfilt, **kw)
        if multi is None:
            return ix.search(queries, k, filters=dfilt, **kw)
        return ix.search_multi(queries, k, multi[0], multi[1], **kw)

    def _scan(self, queries, k: int, dfilt, multi=None, thr=None, counts: bool = False):
        """The per-shard dispatch and the exchange-and-merge of every search: each owned shard searches with ``row_base`` =
        shard * STRIDE (``crh_search`` / ``crh_search_multi`` / ``crh_search_range``), under backend "dist" ONE all-gather moves
        the ``[scores | rows]`` records, and the lists merge (a cut list's padding merges like any other: the merged list of a
        range search is the first ``min(k, count)`` in-range rows of the whole collection).  ``counts``: the in-range counts
        are summed over the owned shards and completed by :meth:`reduce`.  Native shards write their own record of the
        gathered buffer on the current stream; injected host indexes return theirs.  Returns ``(scores f32 [nq, k], GLOBAL rows
        i64 [nq, k], counts i64 [nq] or None)`` where the indexes live."""
        native, on = self._native(), self.dist is None
        if native:
            import torch
            dev, stream = torch.device("cuda", self.device), self._stream()
            if not torch.is_tensor(queries):
                queries = torch.from_numpy(np.ascontiguousarray(queries, dtype=np.float32)).to(dev)
        elif not on:
            import torch
            dev = torch.device("cpu")
        nq = int(queries.shape[0])
        if native or not on:
            local, loc_s, loc_r, gathered, all_s, all_r = ffi.topk_exchange_buffers(torch, self.ns, nq, k, dev)
        part = torch.zeros((len(self.owned), nq), dtype=torch.int64, device=dev) if native and counts else None
        got = {}
        for i, s in enumerate(self.owned):
            kw = {"row_base": s * STRIDE}
            if thr is not None:
                kw["counts"] = counts
            if native:                               # every shard writes its own record of the "gathered" buffer
                kw.update(out_scores=all_s[s] if on else loc_s, out_rows=all_r[s] if on else loc_r, stream=stream)
                if thr is not None:
                    kw["out_counts"] = part[i] if counts else None
            got[s] = self._shard_search(self.index[s], queries, k, dfilt, multi, thr, **kw)
        if native:
            for s in self.owned:
                self.index[s].search_finish(stream)
        elif on:
            all_s, all_r = (np.stack([got[s][j] for s in range(self.ns)]) for j in (0, 1))
        else:
            loc_s.copy_(torch.from_numpy(np.ascontiguousarray(got[self.rank][0])))
            loc_r.copy_(torch.from_numpy(np.ascontiguousarray(got[self.rank][1])))
        if not on:
            self.dist.all_gather_into_tensor(gathered.view(-1), local, group=self.group)
            if not native:
                all_s, all_r = all_s.numpy(), all_r.numpy()
        total = None
        if counts:
            total = self.reduce(part.sum(0) if native else sum(np.asarray(got[s][2], np.int64) for s in self.owned), "SUM")
        return self._merge(all_s, all_r, stream if native else 0) + (total,)

    def _merge(self, all_s, all_r, stream: int):
        """Per-shard lists ``[ns, nq, k]`` (padding -inf / -1) -> the merged ``(scores, rows)`` [nq, k], ties to the lower GLOBAL
        row: ``crh_merge_topk_strided`` on ``stream``, or the injected host merge."""
        if not self._native():
            s, r = self._merge_host(all_s, all_r)
            return np.asarray(s, np.float32), np.asarray(r, np.int64)
        import torch
        out_s = torch.empty(tuple(all_s.shape[1:]), dtype=torch.float32, device=all_s.device)
        out_r = torch.empty(tuple(all_r.shape[1:]), dtype=torch.int64, device=all_r.device)
        ffi.merge_topk(all_s, all_r, out_s, out_r, stream)
        return out_s, out_r

    def _plain(self, queries, k: int, dfilt, multi=None, thr=None, counts: bool = False) -> tuple:
        """A plain, mixed-filter or thresholded search as host arrays: ``(scores [nq, k], shard [nq, k], local row [nq, k])``
        and, with ``thr``, ``counts int64 [nq] or None``; -1 rows are padding.  ONE shard answers directly -- no row base, no
        merge, no torch allocation: the coalescer's and the benchmark's path."""
        ranged = () if thr is None else (counts,)
        if self.ns == 1:
            kw = {"counts": counts} if ranged else {}
            if self.stream:
                kw["stream"] = self.stream
            out = self._shard_search(self.index[0], queries, k, dfilt, multi, thr, **kw)
            return (out[0], np.zeros(out[1].shape, np.int32), out[1]) + tuple(out[2:])
        scores, rows, total = self._scan(queries, k, dfilt, multi, thr, *ranged)
        return (_host(scores),) + split_global(_host(rows)) + ((_host(total) if counts else None,) if ranged else ())

    def search(self, queries: np.ndarray, k: int, dfilt) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Exact top-k over all shards: (scores [nq, k], shard [nq, k], local row [nq, k]); -1 rows are padding."""
        return self._plain(queries, k, dfilt)

    def search_multi(self, queries: np.ndarray, k: int, class_filters, query_class) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """:meth:`search` for a batch whose queries carry different filters (``ffi.Index.search_multi``): query ``i`` under
        ``class_filters[query_class[i]]``.  The same per-shard plan as :meth:`search` -- every shard answers the whole batch
        under the same classes, [one all-gather,] one merge."""
        return self._plain(queries, k, None, multi=(list(class_filters), np.asarray(query_class, np.int32)))

    def search_range(self, queries: np.ndarray, k: int, thresholds, dfilt, counts: bool = True):
        """:meth:`search` with a score threshold per query: ``(scores [nq, k], shard [nq, k], local row [nq,
        k], counts int64 [nq] or None)``; -1 rows are padding."""
        return self._plain(queries, k, dfilt, thr=ffi.range_thresholds(thresholds, len(queries)), counts=counts)

    def search_device(self, queries, k: int, dfilt, multi=None):
        """:meth:`search` on the device, results left there: (scores f32 [nq, k], GLOBAL rows i64 [nq, k]) CUDA tensors -- per-shard
        ``crh_search`` with ``row_base`` = shard * STRIDE, [one all-gather of the records,] ``crh_merge_topk_strided``, at one
        shard too.  ``multi`` = (class_filters, query_class): every query under its own filter (``crh_search_multi``), ``dfilt``
        unused.  What the device re-rank starts from."""
        return self._scan(queries, k, dfilt, multi)[:2]

    def _candidates(self, queries, c: int, dfilt):
        """The top-``c`` lists of ``queries`` with GLOBAL rows, where the indexes live: ``(scores f32 [nq, c], rows i64 [nq, c])``.
        Native shards take :meth:`search_device`, one shard included; ONE injected index answers directly."""
        if self._native() or self.ns > 1:
            return self._scan(queries, c, dfilt)[:2]
        s, r = self.index[0].search(queries, c, filters=dfilt)
        return np.array(s, np.float32), np.array(r, np.int64)

    def _mask_lists(self, cs, cr, dead: np.ndarray) -> None:
        """Overwrite the lists of the absent members of ragged sets (``dead``: host bool, one per list) with padding, in place."""
        dead = self._local(dead)[:, None]
        _put(cs, dead, float("-inf"))
        _put(cr, dead, -1)

    def _gather_codes(self, rows, cols, none_code: int | None = None):
        """Codes of the payload column(s) ``cols`` of a table of GLOBAL rows: int32 of ``rows``' shape -- one plane per column
        for a tuple of columns -- pre-filled with -1, every owned shard writes the rows it owns, ONE :meth:`reduce` (MAX)
        completes all planes.  ``none_code``: the store's code of "no value" in the (first) column becomes -1 too."""
        one = isinstance(cols, (int, np.integer))
        codes = self._full((() if one else (len(cols),)) + tuple(rows.shape), -1, "int32")
        stream = self._stream()
        for s in self.owned:
            for i, col in enumerate([cols] if one else cols):
                self.index[s].gather_codes(rows, col, row_base=s * STRIDE, out=codes if one else codes[i], stream=stream)
        self.reduce(codes, "MAX")
        if none_code is not None:
            first = codes if one else codes[0]
            _put(first, first == int(none_code), -1)
        return codes

    def _gather_everywhere(self, rows, stream: int = 0):
        """Stored vectors of a table of GLOBAL rows, f32 ``rows.shape + (dim,)``: a row has one owner and the others contribute
        zeros (padding too), so the owned shards' gathers are summed and ONE :meth:`reduce` (SUM) completes the buffer."""
        vecs = None
        for s in self.owned:
            part = self.index[s].gather_vectors(rows, row_base=s * STRIDE, stream=stream)
            if vecs is None:
                vecs = part
            else:
                vecs += part
        return self.reduce(vecs, "SUM")

    # ------------------------------------------------------------------ diversity-aware top-k (MMR)
    def search_mmr(self, queries: np.ndarray, k: int, candidates: int, diversity: float, dfilt) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """:meth:`search` with diversity: (scores [nq, k], shard [nq, k], local row [nq, k]) of the ``crh_mmr_select`` picks among
        the ``candidates`` best hits of every query, over their gathered stored vectors; ``scores`` are the picks' cosines, -1
        rows are padding."""
        cs, cr = self._candidates(queries, candidates, dfilt)
        stream = self._stream()
        _, rows, scores, _ = ffi.mmr_select(cs, cr, self._gather_everywhere(cr, stream), k, diversity, stream=stream)
        return (_host(scores),) + split_global(_host(rows))

    # ------------------------------------------------------------------ per-group cap (group_by / group_size)
    def search_grouped(self, queries: np.ndarray, k: int, candidates: int, col: int, group_size: int, dfilt, ungrouped: int | None = None):
        """One round of the grouped search as host arrays: ``(scores f32 [nq, k], GLOBAL rows i64 [nq, k], codes i32 [nq, k],
        info i32 [nq, 2])`` -- the first ``k`` of the ``candidates`` best hits whose rank in their column-``col`` group is below
        ``group_size`` (``crh_group_select`` over the gathered codes; a candidate whose code is negative or ``ungrouped`` -- the
        store's code of "no value" -- is never capped and comes back with code -1); -1 rows are padding; ``info`` = (kept in the
        whole list, real candidates), what the store's exactness rounds decide on."""
        cs, cr = self._candidates(queries, candidates, dfilt)
        codes = self._gather_codes(cr, col, ungrouped)
        _, rows, scores, gcodes, info = ffi.group_select(cs, cr, codes, k, group_size, stream=self._stream())
        return _host(scores), _host(rows), _host(gcodes), _host(info)

    # ------------------------------------------------------------------ overlap-free hit lists (max_overlap)
    def search_spans(self, queries: np.ndarray, k: int, candidates: int, cols: tuple[int, int, int], permille: int, dfilt, no_file: int | None = None):
        """One round of the ``max_overlap`` search as host arrays: ``(scores f32 [nq, k], GLOBAL rows i64 [nq, k], info i32
        [nq, 2])`` -- the first ``k`` of the ``candidates`` best hits that repeat at most ``permille`` thousandths of the shorter
        span of any better kept hit of their file (``crh_span_select`` over the gathered codes of ``cols`` = (file, first line,
        last line): three planes, ONE all-reduce; a candidate whose file code is ``no_file`` -- the store's code of "no value" --
        has no span); -1 rows are padding; ``info`` = (kept in the whole list, real candidates), what the store's exactness
        rounds decide on."""
        cs, cr = self._candidates(queries, candidates, dfilt)
        codes = self._gather_codes(cr, cols, no_file)
        out = ffi.span_select(cs, cr, codes[0], codes[1], codes[2], k, permille, stream=self._stream())
        return _host(out[2]), _host(out[1]), _host(out[6])

    # ------------------------------------------------------------------ multi-query fusion (RRF / best match)
    def search_fused(self, queries: np.ndarray, k: int, candidates: int, dfilt, method: str = "rrf", rrf_k: int = 60, weights=None, live=None):
        """Fusion as host arrays: ``queries`` [nq, m, dim] -- the ``m`` sub-queries of ``nq`` logical ones -- are searched as
        ``nq * m`` plain queries, ``candidates`` hits each, then ``crh_fuse_select`` turns every ``m`` lists into one.  ``live``
        (bool [nq, m], host): the real members of ragged sets; the lists of the others are overwritten with padding before the
        fusion.  Under backend "dist" every rank holds the same merged lists and fuses them itself: no collective is added.
        Returns ``(GLOBAL rows i64, fused f32, cos f32, lists i32, first i32)``, each [nq, k], and ``info`` i32 [nq, 2] =
        (distinct, real); -1 rows are padding."""
        nq, m = int(queries.shape[0]), int(queries.shape[1])
        cs, cr = self._candidates(queries.reshape(nq * m, int(queries.shape[2])), candidates, dfilt)
        if live is not None:
            self._mask_lists(cs, cr, ~np.asarray(live, bool).reshape(nq * m))
        return tuple(_host(a) for a in ffi.fuse_select(cs, cr, m, k, method, rrf_k, weights, stream=self._stream()))

    # ------------------------------------------------------------------ facets
    def facet(self, dfilt, col: int, n_bins: int, k: int, queries=None, thr=None):
        """Exact per-code counts of column ``col`` over all shards and their top-``k`` list, as host arrays: ``(codes i32 [nq,
        k], counts i64 [nq, k], sel i64 [nq, 2] = (codes counted, rows counted under a code), info i64 [nq, 3] = (counted,
        missing, out of range))``; the tail of a list is (-1, 0).  Without ``queries`` (``nq`` = 1) the rows ``dfilt`` keeps
        count (``crh_index_facet``); with ``queries`` [nq, dim] and ``thr`` [nq] those of them whose score reaches the query's
        threshold (``crh_search_range_facet``).  Every owned shard fills a slab of its own -- dictionary codes are the
        collection's, the same on every shard --, the slabs are summed, ONE :meth:`reduce` (SUM) completes bins and info in
        one buffer, and ONE ``crh_facet_select`` runs on the sum."""
        nq = 1 if queries is None else int(len(queries))
        n_bins, k = int(n_bins), int(k)
        if queries is not None and nq * n_bins > ffi.FACET_MAX_ENTRIES:
            raise ValueError(f"a semantic facet of {nq} queries x {n_bins} values asks for {nq * n_bins} bin entries per shard, "
                             f"more than {ffi.FACET_MAX_ENTRIES}: send fewer queries per call")
        stream = self._stream()
        slab = self._full((nq * (n_bins + 3),), 0, "int64")                # [bins | info]: one buffer, one all-reduce
        bins, info = slab[: nq * n_bins].reshape(nq, n_bins), slab[nq * n_bins:].reshape(nq, 3)
        if queries is not None and self._native() and not hasattr(queries, "data_ptr"):
            queries = self._local(np.ascontiguousarray(queries, dtype=np.float32))
        for i, s in enumerate(self.owned):
            ix = self.index[s]
            kw = {"stream": stream} if self._native() else {}
            if i == 0 and self._native():
                kw["out"] = (bins if queries is not None else bins[0], info if queries is not None else info[0])
            if queries is None:
                b, f = ix.facet(col, n_bins, filters=dfilt, **kw)
            else:
                b, f = ix.search_range_facet(queries, thr, col, n_bins, filters=dfilt, **kw)
            if "out" not in kw:
                bins += b.reshape(nq, n_bins)
                info += f.reshape(nq, 3)
        self.reduce(slab, "SUM")
        codes, counts, sel = ffi.facet_select(bins, k, stream=stream)
        return _host(codes), _host(counts), _host(sel), _host(info)

    # ------------------------------------------------------------------ keyword search (BM25)
    # ``lex`` = {shard: ffi.Lex}: the forward indexes beside the owned shards, rows numbered like the shards' (the collection
    # builds and keeps them).  Tombstones and filters reach them as the validity words of ``Index.row_mask`` only.
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

    def _lex_lists(self, lex: dict, queries, idf, k: int, k1: float, b: float, avgdl: float, dfilt):
        """Exact BM25 top-k over all shards, where the indexes live: ``(scores f32 [nq, k], GLOBAL rows i64 [nq, k], counts i64
        [nq])`` -- per shard ``crh_index_row_mask`` + ``crh_lex_search`` with ``row_base`` = shard * STRIDE into its own part of
        one table full of padding, then the merge of :meth:`_scan` (none at one shard); the counts are summed."""
        nq, stream = len(queries), self._stream()
        all_s, all_r = self._full((self.ns, nq, k), float("-inf"), "float32"), self._full((self.ns, nq, k), -1, "int64")
        counts = self._full((nq,), 0, "int64")
        for s, ix in self.index.items():
            if self.rows[s] == 0:
                continue
            mask = ix.row_mask(dfilt, stream=stream)
            mine_s, mine_r = all_s[s], all_r[s]      # (every shard writes its own part of the table)
            ps, pr, pc = lex[s].search(queries, idf, k, k1, b, avgdl, mask=mask, row_base=s * STRIDE, stream=stream, out_scores=mine_s, out_rows=mine_r)
            if ps is not mine_s:                     # (a host-side index returns its lists)
                mine_s[...], mine_r[...] = ps, pr
            counts += pc
        if self.ns == 1:
            return all_s[0], all_r[0], counts
        return self._merge(all_s, all_r, stream) + (counts,)

    def lex_search(self, lex: dict, queries, idf, k: int, k1: float, b: float, avgdl: float, dfilt):
        """Exact BM25 top-k over all shards as host arrays: ``(scores f32 [nq, k], GLOBAL rows i64 [nq, k], counts i64 [nq])``."""
        return tuple(_host(a) for a in self._lex_lists(lex, queries, idf, k, k1, b, avgdl, dfilt))

    def search_hybrid(self, lex: dict, vectors: np.ndarray, queries, idf, k: int, candidates: int, k1: float, b: float, avgdl: float,
                      dfilt, rrf_k: int = 60, weights=None):
        """Dense + keyword, fused: the dense top-``candidates`` and the BM25 top-``candidates`` (:meth:`_lex_lists`) of every
        query under the same filter, as ``[nq, 2, candidates]``, into ``crh_fuse_select`` with ``m = 2`` and reciprocal-rank
        fusion.  Returns host arrays: the fusion's ``(GLOBAL rows, fused, cos, lists, first, info)`` and the two candidate
        tables ``(dense scores, dense rows, lexical scores, lexical rows)``."""
        ds, dr = self._candidates(vectors, candidates, dfilt)
        ls, lr, _ = self._lex_lists(lex, queries, idf, candidates, k1, b, avgdl, dfilt)
        fused = ffi.fuse_select(_pair(ds, ls), _pair(dr, lr), 2, k, "rrf", rrf_k, weights, stream=self._stream())
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

    def recommend(self, example_rows, P: int, N: int, k: int, candidates: int, dfilt, strategy: str = "average", n_pos=None, n_neg=None):
        """Recommend by example as host arrays.  ``example_rows`` (host int64 [nq, P + N]): the GLOBAL rows of every query's
        examples, positives first, -1 for an unused slot; ``n_pos`` / ``n_neg`` (host int [nq] or None) the live counts of ragged
        sets.  The examples' stored vectors are gathered across the shards.  ``"average"``: ``crh_recommend_query`` makes one
        query per set, its ``candidates`` best hits are searched and ``crh_recommend_select`` drops the example rows.
        ``"best"``: the ``nq * P`` positives are searched as plain queries (``candidates`` hits each; the lists of absent
        positives are overwritten with padding), the candidates' vectors gathered, and ``crh_recommend_select`` applies the
        veto, ranks and counts the settled prefix.  Returns ``(GLOBAL rows i64, score f32, neg f32, best i32)``, each [nq, k],
        ``info`` i32 [nq, 4] = (kept, settled, distinct, vetoed) and ``full`` bool [nq]: whether any of the query's lists came
        back full; -1 rows are padding."""
        code = ffi.recommend_strategy(strategy)
        stream = self._stream()
        er = self._local(np.ascontiguousarray(example_rows, dtype=np.int64))
        nq = int(er.shape[0])
        examples = self._gather_everywhere(er, stream)                    # [nq, P + N, dim]
        if code == ffi.RECOMMEND_AVERAGE:
            m, vecs = 1, None
            cs, cr = self._candidates(ffi.recommend_query(examples, P, N, n_pos, n_neg, stream=stream), candidates, dfilt)
        else:
            m = P
            cs, cr = self._candidates(examples[:, :P].reshape(nq * P, self.dim), candidates, dfilt)
            if n_pos is not None:
                self._mask_lists(cs, cr, (np.arange(P)[None, :] >= np.asarray(n_pos).reshape(nq, 1)).reshape(nq * P))
            vecs = self._gather_everywhere(cr, stream).reshape(nq, P * candidates, self.dim)
        cs, cr = cs.reshape(nq, m, candidates), cr.reshape(nq, m, candidates)
        full = (cr[:, :, -1] >= 0).any(1)
        picked = ffi.recommend_select(cs, cr, vecs, examples, er, P, N, k, strategy, self.dtype == ffi.DTYPE_BF16, n_pos, n_neg, stream=stream)
        return tuple(_host(a) for a in tuple(picked) + (full,))

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


def _put(a, mask, value) -> None:
    """``a[mask] = value`` in place, ``mask`` broadcast: on a device tensor (nothing waits for the device) or a host array."""
    if hasattr(a, "masked_fill_"):
        a.masked_fill_(mask, value)
    else:
        np.copyto(a, value, where=mask)


def _pair(a, b):
    """Two ``[nq, c]`` tables as one contiguous ``[nq, 2, c]``, where they live."""
    if hasattr(a, "cpu"):
        import torch
        return torch.stack([a, b], dim=1).contiguous()
    return np.stack([a, b], axis=1)


def split_global(rows: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """GLOBAL rows (host) as ``(shard int32, local row int64)``; padding (-1) as ``(0, -1)``."""
    return np.where(rows >= 0, rows // STRIDE, 0).astype(np.int32), np.where(rows >= 0, rows % STRIDE, -1)


def shard_sizes(rows: Sequence[int]) -> str:
    return "/".join(str(int(r)) for r in rows)
