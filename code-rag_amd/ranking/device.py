"""Device-side hybrid re-rank of vector hits (BASELINE config 5).

``HybridRanker.rank_results`` (``src/lattice/query/ranking/ranker.py:24-54``) walks one query's hits in Python: about
0.65 ms per 100 hits, 40 ms for a 64-query batch whose corpus scan takes 2.4 ms.  For candidate lists that hold vector hits
only (no graph context -- what ``QueryEngine.search`` has when the graph finds nothing, and what BASELINE config 5
measures), the same arithmetic runs in one kernel launch over the whole batch (``crh_rerank_vector``), reading the payload
facts it needs from per-row SIDE COLUMNS that live on the device beside the vectors:

    content_len  len(payload["content"])            -> code_quality       (scorer.py:105-114)
    degree       total_degree of the row's node      -> centrality         (scorer.py:48-54; -1 = unknown to the graph)
    file_code    dictionary code of file_path        -> per-file cap       (ranker.py:204-229)
    key_code     code of file:entity_name:start_line -> merge of duplicates (models.py:55-56, ranker.py:171-202)
    node_code    code of graph_node_id or entity_name-> centrality lookup key
    name         lower-cased entity name, 64 bytes   -> query_entity_match (scorer.py:92-96)

Results are bit-identical to ``HybridRanker`` (f64, same operand order); ``tests/test_rerank_gpu.py`` checks that.  Only
the <= 50 survivors per query are turned into ``RankedResult`` objects on the host.
"""

from __future__ import annotations

import contextlib
import ctypes as C
import struct
import threading
from dataclasses import dataclass
from typing import Any, Sequence

import numpy as np

from .. import ffi
from ..query_types import ResultSource
from .model import RankedResult, RankingConfig, RankingSignal

SIGNALS = (RankingSignal.VECTOR_SIMILARITY.value, RankingSignal.QUERY_ENTITY_MATCH.value,
           RankingSignal.CENTRALITY.value, RankingSignal.CODE_QUALITY.value)


def node_key(payload: dict[str, Any]) -> str:
    """The centrality lookup key of a vector hit: ``graph_node_id or entity_name`` (scorer.py:48-54 through
    ranker.py:253-264, where ``qualified_name`` is the hit's ``graph_node_id``)."""
    return payload.get("graph_node_id") or payload.get("entity_name", "") or ""


def merge_key(payload: dict[str, Any]) -> str:
    return f"{payload.get('file_path', '')}:{payload.get('entity_name', '')}:{payload.get('start_line')}"


class SideColumns:
    """Per-row side data of one collection shard, resident on the device; rows are appended in store order.  Host and device
    copies grow geometrically and an append uploads ONLY the new rows (a re-rank after every upsert does not re-send the
    collection); replacing a whole column (graph degrees) re-sends that column alone."""

    INT_COLS = ("content_len", "degree", "file_code", "key_code", "node_code", "name_len")

    def __init__(self, device: int = 0, books: dict[str, dict[str, int]] | None = None):
        import torch
        self._torch = torch
        self.device = torch.device("cuda", device)
        self.rows = 0
        self._host: dict[str, np.ndarray] = {c: np.zeros((0,), np.int32) for c in self.INT_COLS}
        self._names = np.zeros((0, ffi.RR_NAME_BYTES), np.uint8)
        # value -> code dictionaries of file path / merge key / centrality key; the shards of one collection SHARE them
        # (candidates of different shards are compared by code)
        self._books: dict[str, dict[str, int]] = books if books is not None else {"file": {}, "key": {}, "node": {}}
        self._node_keys: list[str] = []
        self._dev: dict[str, Any] | None = None      # device tensors with capacity >= rows
        self._dev_rows = 0                           # rows already uploaded
        self._dirty: set[str] = set()                # columns replaced wholesale since the last upload

    def _code(self, book: str, value: str) -> int:
        b = self._books[book]
        return b.setdefault(value, len(b) + 1)

    def _grow_host(self, need: int) -> None:
        cap = len(self._names)
        if need <= cap:
            return
        cap = max(need, 2 * cap, 1024)
        for c in self.INT_COLS:
            new = np.zeros((cap,), np.int32)
            new[: self.rows] = self._host[c][: self.rows]
            self._host[c] = new
        names = np.zeros((cap, ffi.RR_NAME_BYTES), np.uint8)
        names[: self.rows] = self._names[: self.rows]
        self._names = names

    def append(self, payloads: Sequence[dict[str, Any] | None]) -> None:
        """Rows in store order; ``None`` (a tombstoned row) keeps the numbering aligned."""
        n = len(payloads)
        if n == 0:
            return
        self._grow_host(self.rows + n)
        h, r0 = self._host, self.rows
        width = ffi.RR_NAME_BYTES
        for j, p in enumerate(payloads):
            p = p or {}
            r = r0 + j
            content = p.get("content")
            name = (p.get("entity_name", "") or "").lower().encode("utf-8")
            # (a payload may carry anything under "content": what has no length counts as no content -- one odd point must not
            # take the re-rank of the whole collection down; every row passes here, whether a query ever meets it or not)
            h["content_len"][r] = len(content) if content and hasattr(content, "__len__") else 0
            h["degree"][r] = -1
            h["file_code"][r] = self._code("file", p.get("file_path", "") or "")
            h["key_code"][r] = self._code("key", merge_key(p))
            nk = node_key(p)
            h["node_code"][r] = self._code("node", nk)
            h["name_len"][r] = len(name)
            self._node_keys.append(nk)
            if name:
                self._names[r, : min(len(name), width)] = np.frombuffer(name[:width], dtype=np.uint8)
        self.rows = r0 + n

    def select(self, keep: np.ndarray) -> None:
        """Keep the rows ``keep`` (ascending), renumbered 0..len(keep)-1: what a compaction of the index does to its rows."""
        keep = np.asarray(keep, np.int64)
        for c in self.INT_COLS:
            self._host[c] = np.ascontiguousarray(self._host[c][: self.rows][keep])
        self._names = np.ascontiguousarray(self._names[: self.rows][keep])
        if self._node_keys:
            self._node_keys = [self._node_keys[int(i)] for i in keep]
        self.rows = int(keep.size)
        self._dev, self._dev_rows = None, 0          # re-uploaded on the next gather
        self._dirty.clear()

    def set_degrees(self, total_degree: dict[str, int]) -> None:
        """``{centrality key: total_degree}`` as the graph reports it; keys it does not know stay at -1."""
        self._host["degree"][: self.rows] = np.fromiter((int(total_degree.get(k, -1)) for k in self._node_keys), np.int32, self.rows)
        self._dirty.add("degree")

    def set_int_column(self, name: str, values) -> None:
        """Bulk load of one column (synthetic corpora: arrays generated without payload dictionaries)."""
        v = np.asarray(values, dtype=np.int32)
        if v.shape != (self.rows,):
            raise ValueError(f"column {name} needs {self.rows} values")
        self._host[name][: self.rows] = v
        self._dirty.add(name)

    @classmethod
    def from_arrays(cls, device: int, **cols) -> "SideColumns":
        """Columns given as arrays (``name`` as uint8 [rows, 64]); no dictionaries are kept."""
        self = cls(device)
        self.rows = int(len(cols["content_len"]))
        self._host = {c: np.ascontiguousarray(cols[c], dtype=np.int32) for c in cls.INT_COLS}
        self._names = np.ascontiguousarray(cols["name"], dtype=np.uint8).reshape(self.rows, ffi.RR_NAME_BYTES)
        return self

    def _resident(self) -> dict[str, Any]:
        t = self._torch
        if self._dev is None or int(self._dev["name"].shape[0]) < self.rows:         # (re)allocate with headroom, keep what is there
            cap = max(self.rows, 2 * (int(self._dev["name"].shape[0]) if self._dev else 0), 1024)
            new = {c: t.zeros((cap,), dtype=t.int32, device=self.device) for c in self.INT_COLS}
            new["name"] = t.zeros((cap, ffi.RR_NAME_BYTES), dtype=t.uint8, device=self.device)
            if self._dev is not None and self._dev_rows:
                for c in new:
                    new[c][: self._dev_rows].copy_(self._dev[c][: self._dev_rows])
            self._dev = new
        lo, hi = self._dev_rows, self.rows
        if hi > lo:
            for c in self.INT_COLS:
                self._dev[c][lo:hi].copy_(t.from_numpy(self._host[c][lo:hi]))
            self._dev["name"][lo:hi].copy_(t.from_numpy(self._names[lo:hi]))
            self._dev_rows = hi
        for c in self._dirty:
            self._dev[c][: self.rows].copy_(t.from_numpy(self._host[c][: self.rows]))
        self._dirty.clear()
        return self._dev

    def gather(self, rows_dev, row_base: int = 0, stream: int | None = None) -> dict[str, Any]:
        """Side data of a candidate table ``rows_dev`` (int64 CUDA tensor [nq, k]); rows of other shards give zeros
        (degree: 0 as well, so that the shards' gathers add up -- the owner contributes the real value).
        ``stream=None``: torch's current stream on this device (where ``rows_dev`` was produced)."""
        t = self._torch
        ffi.use_device(self.device.index)
        stream = ffi.current_stream(self.device) if stream is None else stream
        dev = self._resident()
        n = int(rows_dev.numel())
        # all columns are views of ONE int32 buffer ([n] per integer column, then 64 name bytes = 16 words per candidate), so
        # that a sharded caller completes the table with one all-reduce of ``out.packed`` (sharded.gather_columns)
        words = ffi.RR_NAME_BYTES // 4
        buf = t.empty((n * (len(self.INT_COLS) + words),), dtype=t.int32, device=self.device)
        out = PackedColumns()
        out.packed = buf
        # one launch for the seven columns (crh_gather_rerank_columns; six launches of crh_gather_rows_* until round 4)
        cc = ffi.RerankColumns(*(dev[c].data_ptr() for c in (*self.INT_COLS, "name")))
        ffi.check(ffi.lib().crh_gather_rerank_columns(n, rows_dev.data_ptr(), row_base, self.rows, C.byref(cc), buf.data_ptr(), stream))
        for i, c in enumerate(self.INT_COLS):
            out[c] = buf[i * n:(i + 1) * n]
        out["name"] = buf[len(self.INT_COLS) * n:].view(t.uint8).view(n, ffi.RR_NAME_BYTES)
        return out


class PackedColumns(dict):
    """Column name -> tensor, all of them views of ``packed`` (one int32 buffer).  At most one shard contributes a non-zero
    value per element, so summing the buffers of all shards word by word completes every column, the name bytes included."""
    packed: Any = None


@dataclass
class RerankOutput:
    """Per query, in final order: ``index[q, :count[q]]`` are positions in the candidate list; ``count[q] == -1`` means the
    device declined the query (more than 8 entities, an entity name longer than 64 bytes) and the host ranker must run."""
    index: np.ndarray     # int32 [nq, max_total]
    score: np.ndarray     # float64 [nq, max_total]
    signals: np.ndarray   # float64 [nq, max_total, 4] in SIGNALS order
    count: np.ndarray     # int32 [nq]
    hybrid: np.ndarray    # bool [nq, max_total]


_Q_SIZE = C.sizeof(ffi.RerankQuery)
_Q_HEAD = struct.Struct(f"<ddi{ffi.RR_MAX_ENTITIES}i")          # weights, n_entities, entity_len[]
_Q_ENT = ffi.RerankQuery.entity.offset
assert _Q_HEAD.size == _Q_ENT and _Q_ENT + ffi.RR_MAX_ENTITIES * ffi.RR_ENTITY_BYTES + 4 == _Q_SIZE


def pack_queries(plans, config: RankingConfig, weights: dict | None = None) -> np.ndarray:
    """``crh_rerank_query`` array (as bytes) from query plans: the intent's weights and the set of lower-cased entity names
    (ranker.py:33-35).  Too many or too long entities are signalled with n_entities = -1.  (struct.pack_into + slice copies
    into one bytearray: field-by-field ctypes or numpy-record assignment cost 7 us per plan -- more than the kernel takes for
    the whole batch.)"""
    buf = bytearray(_Q_SIZE * len(plans))
    weights = {} if weights is None else weights      # intent -> (vector_weight, centrality_weight); a caller may keep it
    pad = [0] * ffi.RR_MAX_ENTITIES
    for i, plan in enumerate(plans):
        w = weights.get(plan.primary_intent)
        if w is None:
            ww = config.weights_for(plan.primary_intent)
            w = weights[plan.primary_intent] = (ww["vector_weight"], ww["centrality_weight"])
        enc = [n.encode("utf-8") for n in sorted({e.name.lower() for e in plan.entities})]
        base = i * _Q_SIZE
        lens = [len(b) for b in enc]
        if len(enc) > ffi.RR_MAX_ENTITIES or (lens and max(lens) > ffi.RR_ENTITY_BYTES):
            _Q_HEAD.pack_into(buf, base, w[0], w[1], -1, *pad)
            continue
        _Q_HEAD.pack_into(buf, base, w[0], w[1], len(enc), *(lens + pad[len(enc):]))
        for j, b in enumerate(enc):
            o = base + _Q_ENT + j * ffi.RR_ENTITY_BYTES
            buf[o:o + len(b)] = b
    return np.frombuffer(buf, dtype=np.uint8)


class DeviceReranker:
    """``HybridRanker`` for batches of vector-only candidate lists, on the device."""

    def __init__(self, config: RankingConfig | None = None, centrality_top: int = 5, device: int = 0):
        import torch
        self._torch = torch
        self.config = config or RankingConfig()
        self.centrality_top = centrality_top   # QueryEngine looks up the first 5 vector hits (engine.py:358-362)
        self.device = torch.device("cuda", device)
        self._lock = threading.Lock()          # the cached device / pinned output buffers below serve one call at a time

    def rank(self, scores_dev, rows_dev, cols: dict[str, Any], plans, stream: int | None = None) -> RerankOutput:
        with self._lock:
            return self._rank(scores_dev, rows_dev, cols, plans, stream)()

    def rank_async(self, scores_dev, rows_dev, cols: dict[str, Any], plans, stream: int | None = None):
        """:meth:`rank` in two halves: everything is enqueued on ``stream`` (the copy back included) and a callable is returned
        that waits for it and builds the :class:`RerankOutput`.  Between the two the caller may enqueue more work on the stream
        -- a serving loop enqueues the next search there, so that the device has something to do while the host collects this
        batch.  ONE call may be outstanding per reranker (its device and pinned buffers are reused), from one thread."""
        return self._rank(scores_dev, rows_dev, cols, plans, stream)

    def _rank(self, scores_dev, rows_dev, cols: dict[str, Any], plans, stream: int | None = None):
        t = self._torch
        ffi.use_device(self.device.index)
        stream = ffi.current_stream(self.device) if stream is None else stream
        nq, k = (int(v) for v in scores_dev.shape)
        if len(plans) != nq:
            raise ValueError(f"{len(plans)} plans for {nq} candidate lists")
        mt = self.config.max_total
        # ONE device buffer and ONE pinned host mirror hold every output (f64 parts first: alignment), cached per shape; the
        # packed queries go up from pinned memory: one H2D, the kernel, one D2H and one wait per call
        # (five allocations + fills and five synchronising .cpu() copies were 0.3 ms of a 0.43 ms call)
        n = nq * mt
        nbytes = 8 * n + 32 * n + 4 * n + 4 * n + 4 * nq
        ws = self.__dict__.setdefault("_ws", {})
        key = (nq, mt)
        if key not in ws:
            ws[key] = (t.empty((nbytes,), dtype=t.uint8, device=self.device), t.empty((nbytes,), dtype=t.uint8, pin_memory=True))
        dbuf, hbuf = ws[key]
        o_sc = dbuf[:8 * n].view(t.float64).view(nq, mt)
        o_sig = dbuf[8 * n:40 * n].view(t.float64).view(nq, mt, 4)
        o_idx = dbuf[40 * n:44 * n].view(t.int32).view(nq, mt)
        o_flg = dbuf[44 * n:48 * n].view(t.int32).view(nq, mt)
        o_cnt = dbuf[48 * n:].view(t.int32)
        packed = pack_queries(plans, self.config, self.__dict__.setdefault("_weights", {}))
        qkey = ("q", packed.nbytes)
        if qkey not in ws:
            ws[qkey] = (t.empty((packed.nbytes,), dtype=t.uint8, device=self.device), t.empty((packed.nbytes,), dtype=t.uint8, pin_memory=True))
        qdev, qhost = ws[qkey]
        # torch's own work for this call (copies, fills) must sit on the stream the kernel is launched on
        cur = t.cuda.current_stream(self.device)
        on = contextlib.nullcontext() if stream == cur.cuda_stream else t.cuda.stream(t.cuda.ExternalStream(stream, device=self.device))
        with on:
            qhost.numpy()[:] = packed       # (every call ends synchronised: the pinned buffers are free again)
            qdev.copy_(qhost, non_blocking=True)     # (the kernel pads the slots behind a query's survivors itself: no fills here)
            cc = ffi.RerankColumns(*(cols[c].data_ptr() for c in ("content_len", "degree", "file_code", "key_code", "node_code", "name_len", "name")))
            ffi._typed(scores_dev, "float32", "scores")
            ffi._typed(rows_dev, "int64", "rows")
            ffi.check(ffi.lib().crh_rerank_vector(nq, k, scores_dev.data_ptr(), rows_dev.data_ptr(), C.byref(cc), qdev.data_ptr(),
                                                  self.config.entity_match_bonus, self.config.max_per_file, mt, self.centrality_top,
                                                  o_idx.data_ptr(), o_sc.data_ptr(), o_sig.data_ptr(), o_cnt.data_ptr(), o_flg.data_ptr(), stream))
            hbuf.copy_(dbuf, non_blocking=True)
            done = t.cuda.Event()
            done.record()

        def collect() -> RerankOutput:
            done.synchronize()
            h = hbuf.numpy()
            return RerankOutput(h[40 * n:44 * n].view(np.int32).reshape(nq, mt).copy(), h[:8 * n].view(np.float64).reshape(nq, mt).copy(),
                                h[8 * n:40 * n].view(np.float64).reshape(nq, mt, 4).copy(), h[48 * n:].view(np.int32).copy(),
                                h[44 * n:48 * n].view(np.int32).reshape(nq, mt).astype(bool))
        return collect

    @staticmethod
    def materialise(out: RerankOutput, q: int, hits: Sequence[dict[str, Any]]) -> list[RankedResult]:
        """The survivors of query ``q`` as ``RankedResult`` objects, built from the flattened hit dicts of its candidate
        list exactly as ``HybridRanker._from_vector_hit`` builds them (fields of an absorbed duplicate are not filled in --
        the device keeps no payload text; a caller that needs them uses the host ranker)."""
        res = []
        for s in range(int(out.count[q])):
            hit = hits[int(out.index[q, s])]
            res.append(RankedResult(
                file_path=hit.get("file_path", ""), entity_name=hit.get("entity_name", ""), entity_type=hit.get("entity_type", ""),
                qualified_name=hit.get("graph_node_id"), content=hit.get("content"), summary=hit.get("summary"),
                start_line=hit.get("start_line"), end_line=hit.get("end_line"), graph_node_id=hit.get("graph_node_id"),
                final_score=float(out.score[q, s]),
                signal_scores={name: float(out.signals[q, s, j]) for j, name in enumerate(SIGNALS)},
                source=ResultSource.HYBRID.value if out.hybrid[q, s] else ResultSource.VECTOR.value))
        return res


# ---------------------------------------------------------------------------------------------------------------------------
# Both branches on the device (crh_rerank_hybrid): graph candidates built from the BFS lists of the device call
# graph, ranked together with the vector hits exactly as ``HybridRanker.rank_results`` ranks a ``GraphContext`` and a hit list.

HYBRID_SIGNALS = (RankingSignal.GRAPH_MATCH.value, RankingSignal.QUERY_ENTITY_MATCH.value, RankingSignal.RELATIONSHIP_RELEVANCE.value,
                  RankingSignal.CENTRALITY.value, RankingSignal.CONTEXT_RICHNESS.value, RankingSignal.VECTOR_SIMILARITY.value,
                  RankingSignal.CODE_QUALITY.value)
assert len(HYBRID_SIGNALS) == ffi.RR_HYBRID_SIGNALS
# ffi.ROLE_* (CRH_ROLE_*) -> (GraphContext attribute, relationship_path, carries a traversal depth): ranker.py:70-169
ROLES = {ffi.ROLE_PRIMARY: ("primary_entities", None, False), ffi.ROLE_CALLER: ("callers", "caller", True),
         ffi.ROLE_CALLEE: ("callees", "callee", True), ffi.ROLE_METHOD: ("methods", "method", False),
         ffi.ROLE_PARENT: ("parent_classes", "parent_class", False), ffi.ROLE_CHILD: ("child_classes", "child_class", False)}


def richness_bits(payload: dict[str, Any] | None) -> int:
    """What ``context_richness`` reads of a graph node (scorer.py:56-66): bit 0 summary, bit 1 docstring, bit 2 signature."""
    p = payload or {}
    return (1 if p.get("summary") else 0) | (2 if p.get("docstring") else 0) | (4 if p.get("signature") else 0)


class RichnessColumn:
    """One more int32 per row beside :class:`SideColumns`: the richness bits of the row's payload.  Derived (never persisted);
    grows with the rows, an append uploads the new rows only."""

    def __init__(self, device: int = 0):
        import torch
        self._torch = torch
        self.device = torch.device("cuda", device)
        self.rows = 0
        self._host = np.zeros((0,), np.int32)
        self._dev = None
        self._dev_rows = 0

    def append(self, payloads: Sequence[dict[str, Any] | None]) -> None:
        n = len(payloads)
        if n == 0:
            return
        if self.rows + n > len(self._host):
            new = np.zeros((max(self.rows + n, 2 * len(self._host), 1024),), np.int32)
            new[: self.rows] = self._host[: self.rows]
            self._host = new
        self._host[self.rows: self.rows + n] = np.fromiter((richness_bits(p) for p in payloads), np.int32, n)
        self.rows += n

    def select(self, keep: np.ndarray) -> None:
        """Keep the rows ``keep`` (ascending), renumbered: what a compaction does to the rows."""
        self._host = np.ascontiguousarray(self._host[: self.rows][np.asarray(keep, np.int64)])
        self.rows = int(self._host.size)
        self._dev, self._dev_rows = None, 0

    def _resident(self):
        t = self._torch
        if self._dev is None or int(self._dev.shape[0]) < self.rows:
            new = t.zeros((max(self.rows, 2 * (int(self._dev.shape[0]) if self._dev is not None else 0), 1024),), dtype=t.int32, device=self.device)
            if self._dev is not None and self._dev_rows:
                new[: self._dev_rows].copy_(self._dev[: self._dev_rows])
            self._dev = new
        if self.rows > self._dev_rows:
            self._dev[self._dev_rows: self.rows].copy_(t.from_numpy(self._host[self._dev_rows: self.rows]))
            self._dev_rows = self.rows
        return self._dev

    def gather(self, rows_dev, row_base: int = 0, stream: int | None = None):
        """Bits of a candidate table (int64 CUDA tensor); rows of other shards and padding give 0, so the shards' gathers add up."""
        t = self._torch
        ffi.use_device(self.device.index)
        stream = ffi.current_stream(self.device) if stream is None else stream
        out = t.empty((int(rows_dev.numel()),), dtype=t.int32, device=self.device)
        ffi.check(ffi.lib().crh_gather_rows_i32(int(rows_dev.numel()), rows_dev.data_ptr(), row_base, self.rows, self._resident().data_ptr(), 0,
                                                out.data_ptr(), stream))
        return out


def graph_node_rows(row_node_dev, n_nodes: int, alive_words_dev=None, row_base: int = 0, out=None, stream: int | None = None):
    """``crh_graph_node_rows``: min the alive rows of one shard (``row_node_dev`` int32 [rows], ``alive_words_dev`` int32 validity words or
    None) into ``out`` (int64 [n_nodes], created filled with -1 when not given; several shards pass the same tensor)."""
    import torch
    dev = row_node_dev.device
    ffi.use_device(dev.index)
    stream = ffi.current_stream(dev) if stream is None else stream
    if out is None:
        out = torch.full((int(n_nodes),), -1, dtype=torch.int64, device=dev)
    ffi._typed(row_node_dev, "int32", "row_node")
    n_rows = int(row_node_dev.numel())
    if alive_words_dev is not None and int(alive_words_dev.numel()) * 32 < n_rows:
        raise ValueError(f"{int(alive_words_dev.numel())} alive words for {n_rows} rows")
    if int(out.numel()) < int(n_nodes):
        raise ValueError(f"node rows: {int(out.numel())} entries for {n_nodes} nodes")
    ffi.check(ffi.lib().crh_graph_node_rows(n_rows, row_node_dev.data_ptr(), alive_words_dev.data_ptr() if alive_words_dev is not None else None,
                                            int(row_base), int(n_nodes), out.data_ptr(), stream))
    return out


@dataclass
class GraphTable:
    """A batch's graph candidates, device tensors [nq, G]: node id, representative row (int64, -1 = padding), CRH_ROLE_*, depth."""
    node: Any
    row: Any
    role: Any
    depth: Any


def segment_table(per_query: Sequence[Sequence[tuple]]) -> tuple[list[tuple[int, int, int, int, int]], int]:
    """The segment table of ``crh_graph_candidates`` from, per query, the role lists in ANY order: items are
    ``(role, node, list_row, take)`` with ``node >= 0`` for an explicit node (a primary) or ``node = -1`` for the first ``take``
    entries of a list row.  Returned: ``[(query, role, node, list_row, take)]`` sorted by query and, within a query, in the order
    ``HybridRanker`` walks the roles (primaries, callers, callees, methods, parents, children; the given order inside a role --
    i.e. primary order), and G = the largest number of entries one query can yield."""
    segs, G = [], 0
    for q, items in enumerate(per_query):
        total = 0
        for role in range(len(ROLES)):
            for r, node, list_row, take in items:
                if r != role:
                    continue
                segs.append((q, role, int(node), int(list_row), int(take)))
                total += 1 if node >= 0 else int(take)
        G = max(G, total)
    return segs, G


def graph_candidates(segments: Sequence[tuple[int, int, int, int, int]], nq: int, G: int, node_rows_dev, list_nodes_dev=None,
                     list_depth_dev=None, stream: int | None = None) -> GraphTable:
    """``crh_graph_candidates``: the [nq, G] candidate table from a segment table (:func:`segment_table`), the list tables of
    ``crh_graph_list`` ([n_lists, limit] int32 device tensors; several calls' tables concatenated) and the representative rows."""
    import torch
    dev = node_rows_dev.device
    ffi.use_device(dev.index)
    stream = ffi.current_stream(dev) if stream is None else stream
    ffi._typed(node_rows_dev, "int64", "node_rows")
    n_lists, limit = (int(v) for v in list_nodes_dev.shape) if list_nodes_dev is not None else (0, 0)
    if list_nodes_dev is not None:
        ffi._typed(list_nodes_dev, "int32", "list nodes")
        ffi._typed(list_depth_dev, "int32", "list depth")
        if tuple(list_depth_dev.shape) != (n_lists, limit):
            raise ValueError("list nodes and depths differ in shape")
    arr = (ffi.GraphSegment * max(1, len(segments)))()
    for i, (q, role, node, list_row, take) in enumerate(segments):
        arr[i] = ffi.GraphSegment(q, role, node, list_row, take, 0)
    i32 = dict(dtype=torch.int32, device=dev)
    # everything is allocated with `stream` as torch's current stream: the caching allocator hands the scratch tensors out again
    # on that stream only, i.e. behind the kernel that reads them
    cur = torch.cuda.current_stream(dev)
    on = contextlib.nullcontext() if stream == cur.cuda_stream else torch.cuda.stream(torch.cuda.ExternalStream(stream, device=dev))
    with on:
        table = GraphTable(torch.empty((nq, G), **i32), torch.empty((nq, G), dtype=torch.int64, device=dev), torch.empty((nq, G), **i32),
                           torch.empty((nq, G), **i32))
        segs_dev = torch.empty((max(1, len(segments)) * C.sizeof(ffi.GraphSegment),), dtype=torch.uint8, device=dev)
        off_dev = torch.empty((nq + 1,), **i32)
        ffi.check(ffi.lib().crh_graph_candidates(nq, G, len(segments), C.cast(arr, C.c_void_p), list_nodes_dev.data_ptr() if n_lists and limit else None,
                                                 list_depth_dev.data_ptr() if n_lists and limit else None, n_lists, limit, node_rows_dev.data_ptr(),
                                                 int(node_rows_dev.numel()), segs_dev.data_ptr(), off_dev.data_ptr(), table.node.data_ptr(),
                                                 table.row.data_ptr(), table.role.data_ptr(), table.depth.data_ptr(), stream))
    return table


@dataclass
class HybridRerankOutput:
    """Per query, in final order: ``index[q, :count[q]]`` are positions in the concatenated candidate list (``< G``: a graph entry);
    ``count[q] == -1``: the device declined the query and the host ranker must run.  ``role`` / ``depth`` / ``key`` are host copies of
    the candidate tables ([nq, G] and the merge-key codes [nq, G + k]) that :meth:`HybridDeviceReranker.materialise` reads."""
    index: np.ndarray     # int32 [nq, max_total]
    score: np.ndarray     # float64 [nq, max_total]
    signals: np.ndarray   # float64 [nq, max_total, 7] in HYBRID_SIGNALS order
    mask: np.ndarray      # int32 [nq, max_total]: bit t set = signal t present
    count: np.ndarray     # int32 [nq]
    hybrid: np.ndarray    # bool [nq, max_total]
    G: int
    role: np.ndarray      # int32 [nq, G]
    depth: np.ndarray     # int32 [nq, G]
    key: np.ndarray       # int32 [nq, G + k]; 0 = padding


_HQ_SIZE = C.sizeof(ffi.RerankHybridQuery)
_HQ_TAIL = struct.Struct("<ddd")
assert _HQ_SIZE == _Q_SIZE + _HQ_TAIL.size and ffi.RerankHybridQuery.graph_weight.offset == _Q_SIZE


def pack_hybrid_queries(plans, config: RankingConfig) -> np.ndarray:
    """``crh_rerank_hybrid_query`` array (as bytes): :func:`pack_queries`' record + graph_weight, context_weight, relationship_bonus."""
    base = pack_queries(plans, config).reshape(len(plans), _Q_SIZE) if len(plans) else np.zeros((0, _Q_SIZE), np.uint8)
    out = np.zeros((len(plans), _HQ_SIZE), np.uint8)
    out[:, :_Q_SIZE] = base
    for i, plan in enumerate(plans):
        w = config.weights_for(plan.primary_intent)
        out[i, _Q_SIZE:] = np.frombuffer(_HQ_TAIL.pack(w["graph_weight"], w["context_weight"], config.relationship_bonus), np.uint8)
    return out.reshape(-1)


class HybridDeviceReranker:
    """``HybridRanker`` for batches whose candidates are graph entries AND vector hits, on the device (``crh_rerank_hybrid``)."""

    def __init__(self, config: RankingConfig | None = None, primary_top: int = 5, centrality_top: int = 5, centrality_limit: int | None = None,
                 device: int = 0):
        import torch
        from ..settings import get_settings
        self._torch = torch
        self.config = config or RankingConfig()
        self.primary_top = primary_top            # engine.py:353-357: the first 5 primary entities
        self.centrality_top = centrality_top      # engine.py:358-362: the first 5 vector hits
        self.centrality_limit = get_settings().max_centrality_lookups if centrality_limit is None else centrality_limit
        self.device = torch.device("cuda", device)

    def rank(self, graph: GraphTable | None, g_cols: dict[str, Any] | None, g_rich, scores_dev, rows_dev, cols: dict[str, Any] | None, plans,
             stream: int | None = None) -> HybridRerankOutput:
        """``graph`` / ``g_cols`` / ``g_rich``: the graph table, ``SideColumns.gather(graph.row)`` and ``RichnessColumn.gather(graph.row)``
        (all None: no graph entries); ``scores_dev`` / ``rows_dev`` / ``cols``: the hits as :meth:`DeviceReranker.rank` takes them
        (all None: no hits)."""
        t = self._torch
        ffi.use_device(self.device.index)
        stream = ffi.current_stream(self.device) if stream is None else stream
        nq = len(plans)
        G = int(graph.row.shape[1]) if graph is not None else 0
        k = int(rows_dev.shape[1]) if rows_dev is not None else 0
        if (graph is not None and int(graph.row.shape[0]) != nq) or (rows_dev is not None and int(rows_dev.shape[0]) != nq):
            raise ValueError(f"{nq} plans do not match the candidate tables")
        mt = self.config.max_total
        n = nq * mt
        S = ffi.RR_HYBRID_SIGNALS
        dbuf = t.empty((8 * n + 8 * S * n + 12 * n + 4 * nq,), dtype=t.uint8, device=self.device)
        o_sc = dbuf[:8 * n].view(t.float64)
        o_sig = dbuf[8 * n:8 * (1 + S) * n].view(t.float64)
        at = 8 * (1 + S) * n
        o_idx, o_flg, o_msk, o_cnt = (dbuf[at:at + 4 * n].view(t.int32), dbuf[at + 4 * n:at + 8 * n].view(t.int32),
                                      dbuf[at + 8 * n:at + 12 * n].view(t.int32), dbuf[at + 12 * n:].view(t.int32))
        names = ("content_len", "degree", "file_code", "key_code", "node_code", "name_len", "name")
        cur = t.cuda.current_stream(self.device)
        on = contextlib.nullcontext() if stream == cur.cuda_stream else t.cuda.stream(t.cuda.ExternalStream(stream, device=self.device))
        with on:
            qdev = t.from_numpy(pack_hybrid_queries(plans, self.config).copy()).to(self.device)
            gc = ffi.RerankColumns(*(g_cols[c].data_ptr() for c in names)) if G else None
            vc = ffi.RerankColumns(*(cols[c].data_ptr() for c in names)) if k else None
            if G:
                ffi._typed(graph.row, "int64", "graph rows")
                ffi._typed(graph.role, "int32", "graph roles")
                ffi._typed(graph.depth, "int32", "graph depths")
                ffi._typed(g_rich, "int32", "richness bits")
            if k:
                ffi._typed(scores_dev, "float32", "scores")
                ffi._typed(rows_dev, "int64", "rows")
            ffi.check(ffi.lib().crh_rerank_hybrid(
                nq, G, k, graph.row.data_ptr() if G else None, graph.role.data_ptr() if G else None, graph.depth.data_ptr() if G else None,
                C.cast(C.pointer(gc), C.c_void_p) if G else None, g_rich.data_ptr() if G else None, scores_dev.data_ptr() if k else None,
                rows_dev.data_ptr() if k else None, C.cast(C.pointer(vc), C.c_void_p) if k else None, qdev.data_ptr(),
                self.config.entity_match_bonus, self.config.max_per_file, mt, self.primary_top, self.centrality_top, self.centrality_limit,
                o_idx.data_ptr(), o_sc.data_ptr(), o_sig.data_ptr(), o_msk.data_ptr(), o_cnt.data_ptr(), o_flg.data_ptr(), stream))
            # what materialise reads of the candidate tables -- role, depth, the merge-key codes (0 = padding) -- is packed on the
            # device: ONE more copy beside the outputs'
            parts = []
            if G:
                parts += [graph.role, graph.depth, t.where(graph.row >= 0, g_cols["key_code"].view(nq, G), 0)]
            if k:
                parts.append(t.where(rows_dev >= 0, cols["key_code"].view(nq, k), 0))
            aux_dev = t.cat(parts, dim=1)
            h = dbuf.cpu().numpy()                       # (waits for the stream)
            aux = aux_dev.cpu().numpy()
            i32 = np.int32
            role, depth, key = aux[:, :G], aux[:, G:2 * G], aux[:, 2 * G:]
        return HybridRerankOutput(h[at:at + 4 * n].view(i32).reshape(nq, mt), h[:8 * n].view(np.float64).reshape(nq, mt),
                                  h[8 * n:at].view(np.float64).reshape(nq, mt, S), h[at + 8 * n:at + 12 * n].view(i32).reshape(nq, mt),
                                  h[at + 12 * n:].view(i32), (h[at + 4 * n:at + 8 * n].view(i32).reshape(nq, mt) & 1).astype(bool), G, role, depth, key)

    @staticmethod
    def materialise(out: HybridRerankOutput, q: int, graph_items, hits) -> list[RankedResult]:
        """The survivors of query ``q`` as ``RankedResult`` objects.  ``graph_items[i]`` (i < G) is the payload of graph entry i's
        representative row with the node's name under ``"graph_node_id"``; ``hits[j]`` the flattened hit dict of vector entry j; both
        may build their dicts on demand -- only survivors and what they absorbed are asked for.  A graph entry becomes what
        ``HybridRanker._from_graph_node`` makes of the node, a hit what ``_from_vector_hit`` makes of it; a merged result fills its
        missing content / summary / signature / docstring from the entries it absorbed, in list order (ranker.py:171-202)."""
        G = out.G

        def candidate(i: int) -> RankedResult:
            if i >= G:
                hit = hits[i - G]
                return RankedResult(file_path=hit.get("file_path", ""), entity_name=hit.get("entity_name", ""), entity_type=hit.get("entity_type", ""),
                                    qualified_name=hit.get("graph_node_id"), content=hit.get("content"), summary=hit.get("summary"),
                                    start_line=hit.get("start_line"), end_line=hit.get("end_line"), graph_node_id=hit.get("graph_node_id"))
            p = graph_items[i]
            _, path, has_depth = ROLES[int(out.role[q, i])]
            name = p.get("graph_node_id")
            r = RankedResult(file_path=p.get("file_path", ""), entity_name=p.get("entity_name", ""), entity_type=p.get("entity_type", ""),
                             qualified_name=name, summary=p.get("summary"), signature=p.get("signature"), docstring=p.get("docstring"),
                             start_line=p.get("start_line"), end_line=p.get("end_line"), graph_node_id=name,
                             metadata={"depth": int(out.depth[q, i])} if has_depth else {})
            r.relationship_path = path
            if has_depth:
                r.depth_from_query = int(out.depth[q, i])
            return r

        res = []
        for s in range(int(out.count[q])):
            i = int(out.index[q, s])
            r = candidate(i)
            if out.hybrid[q, s]:
                for j in np.flatnonzero(out.key[q, i + 1:] == out.key[q, i]) + i + 1:
                    other = candidate(int(j))
                    for field in ("content", "summary", "signature", "docstring"):
                        if not getattr(r, field) and getattr(other, field):
                            setattr(r, field, getattr(other, field))
            r.final_score = float(out.score[q, s])
            r.signal_scores = {name: float(out.signals[q, s, t]) for t, name in enumerate(HYBRID_SIGNALS) if (int(out.mask[q, s]) >> t) & 1}
            r.source = (ResultSource.HYBRID if out.hybrid[q, s] else ResultSource.GRAPH if i < G else ResultSource.VECTOR).value
            res.append(r)
        return res
