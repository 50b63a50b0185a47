"""Deferred searches: scripts of mutations and searches with device outputs over one small index, what every
search must answer, the runner that plays a script against an index, and the fake index of the CPU tier.  Test
infrastructure only.

A search called with device outputs is only enqueued; ``search_finish`` reads its status later and runs it AGAIN when a
candidate buffer overflowed or the one-launch scan timed out.  The answer owed is the one for the index at the search's
place in the order of calls, however often the batch had to run.  So every script is built such that an answer for a LATER
state of the index is a different answer, for every query of every search:

  * appended rows hold near copies of the queries -- ``scale * (q + eps * noise)``, eps shrinking from append to append down to
    0, the exact scaled copy -- with codes that pass every filter in use: they take rank 1 of every later search;
  * a tombstone removes every query's current top hit, under no filter and under each filter in use;
  * the filter delete removes the code value (column 1 == 3) that the SECOND near copy of every query carries: rank 2 before
    the tombstone above it, rank 1 after;
  * every script ends with a mutation, and the expected list of every query of every search differs from the list the FINAL
    state would give (tests/test_deferred_cases_host.py asserts all of this on the oracle).

Expected answers come from ``oracle.search`` (``cosine_search`` = ``preprocess`` + ``search``) under the numpy mask of the
step's filter, and from ``tests.range_cases.select`` for the range kind, on the model state at that step.  Nothing is taken
from the code under test."""
import functools

import numpy as np

from oracle import search as orc
from tests import range_cases
from tests.range_cases import RangeFakeIndex
from tests.span_cases import np_mask

F32 = np.float32
DIM = 384
POOL = 65                       # queries of a script: a search of nq queries sends the first nq
BASE = 7_000_000_000            # the row_base beyond 2^32
GUARD = 2                       # guard rows before and after every output slice
FILL_S, FILL_R, FILL_C = F32(123.0), -77, -7

# The filters of the four kinds.  A row with codes (1, 2) or (1, 3) passes every one of them -- the near copies carry those.
PLAIN = [(0, 1)]                                                   # crh_search: equalities
COND = [(0, [1, 3]), (1, [4], True), (1, 0, 3, "between")]         # crh_search_cond: any-of, NOT, range
CLASSES = [[(0, 1)], [(1, [2, 3])], []]                            # crh_search_multi: three classes
RANGE = [(1, 0, 3, "between")]                                     # crh_search_range
FILTERS_IN_USE = [None, PLAIN, COND, RANGE] + CLASSES[:2]
DELETED_CODE = [(1, 3)]                                            # the filter delete


class State:
    """The model: raw rows, their stored form, two code columns, alive bits."""

    def __init__(self, bf16: bool):
        self.bf16 = bf16
        self.clear()

    def clear(self):
        self.pre = np.zeros((0, DIM), F32)
        self.codes = np.zeros((0, 2), np.int32)
        self.alive = np.zeros((0,), bool)

    def append(self, rows, codes):
        self.pre = np.concatenate([self.pre, orc.preprocess(rows, to_bf16=self.bf16)])
        self.codes = np.concatenate([self.codes, np.asarray(codes, np.int32)])
        self.alive = np.concatenate([self.alive, np.ones(len(rows), bool)])

    def tombstone(self, rows):
        self.alive[np.asarray(rows, np.int64)] = False

    def passing(self, filters=None):
        return np_mask(self.codes, self.alive, filters)

    def copy(self):
        c = State(self.bf16)
        c.pre, c.codes, c.alive = self.pre.copy(), self.codes.copy(), self.alive.copy()
        return c


def _topk(state: State, qpre, k: int, ok, row_base: int):
    if len(state.pre) == 0:
        return np.full((len(qpre), k), -np.inf, F32), np.full((len(qpre), k), -1, np.int64)
    s, r = orc.search(state.pre, qpre, k, alive=ok.astype(np.uint8))
    return s, np.where(r >= 0, r + row_base, r)


def expect(state: State, step: dict):
    """What the search ``step`` answers on ``state``: ``(scores [nq, k] f32, rows [nq, k] i64, counts [nq] i64 or None)``."""
    qpre = orc.preprocess(step["queries"], to_bf16=state.bf16)
    k, base = step["k"], step["row_base"]
    if step["kind"] == "multi":
        s, r = np.empty((len(qpre), k), F32), np.empty((len(qpre), k), np.int64)
        for c, filters in enumerate(step["classes"]):
            sel = np.flatnonzero(step["qclass"] == c)
            if sel.size:
                s[sel], r[sel] = _topk(state, qpre[sel], k, state.passing(filters), base)
        return s, r, None
    if step["kind"] == "range":
        if len(state.pre) == 0:
            return np.full((len(qpre), k), -np.inf, F32), np.full((len(qpre), k), -1, np.int64), np.zeros((len(qpre),), np.int64)
        return range_cases.select(orc.scores(state.pre, qpre), step["thr"], k, state.passing(step["filters"]), base)
    return _topk(state, qpre, k, state.passing(step["filters"]), base) + (None,)


def thresholds(state: State, queries, k: int, filters):
    """Thresholds for a range step, query i taking kind i % 4: the score of the k-th best passing row (inclusive: count k), one
    ulp above it (count k - 1), -2.0 (every passing row), the score of rank 3k.  An empty index: -2.0."""
    nq = len(queries)
    ok = state.passing(filters)
    if not ok.any():
        return np.full((nq,), -2.0, F32)
    sc = orc.scores(state.pre, orc.preprocess(queries, to_bf16=state.bf16))
    live = int(ok.sum())
    thr = np.empty((nq,), F32)
    for i in range(nq):
        ranked = np.sort(sc[i, ok])[::-1]
        kth = ranked[min(k, live) - 1]
        thr[i] = (kth, np.nextafter(kth, F32(4)), F32(-2.0), ranked[min(3 * k, live) - 1])[i % 4]
    return thr


def search_step(state: State, kind: str, queries, k: int, row_base: int = 0) -> dict:
    nq = len(queries)
    step = {"op": "search", "kind": kind, "nq": nq, "k": k, "row_base": row_base, "queries": np.ascontiguousarray(queries, F32)}
    if kind == "multi":
        step["classes"], step["qclass"] = CLASSES, (np.arange(nq) * 7 % 3).astype(np.int32)
    else:
        step["filters"] = {"plain": PLAIN, "cond": COND, "range": RANGE}[kind]
    if kind == "range":
        step["thr"] = thresholds(state, queries, k, RANGE)
    step["want"] = expect(state, step)
    return step


def base_rows(rng, n: int):
    """``n`` random rows; column 0 is 1 or 3 for four rows in five (0, 2: fails PLAIN / COND), column 1 is 2 or 3 for four in
    five (4, 5: fails COND / RANGE)."""
    rows = rng.standard_normal((n, DIM), dtype=F32) * rng.uniform(0.2, 5.0, size=(n, 1)).astype(F32)
    codes = np.stack([rng.choice([1, 3, 1, 3, 0, 2, 1, 3, 1, 3], n), rng.choice([2, 3, 2, 3, 4, 5, 2, 3, 2, 3], n)], 1).astype(np.int32)
    return rows, codes


def near_copies(rng, queries, eps: float, scale: float, code1: int):
    """``scale * (q + eps * noise)`` per query (cosine with q about 1 / sqrt(1 + eps^2)), codes (1, ``code1``)."""
    noise = rng.standard_normal(queries.shape, dtype=F32)
    rows = (F32(scale) * (queries + F32(eps) * noise)).astype(F32)
    return rows, np.tile(np.asarray([[1, code1]], np.int32), (len(queries), 1))


def top_hits(state: State, queries):
    """Every query's best alive row, under no filter and under each filter in use (unique, ascending)."""
    qpre = orc.preprocess(queries, to_bf16=state.bf16)
    hits = [_topk(state, qpre, 1, state.passing(f), 0)[1].ravel() for f in FILTERS_IN_USE]
    hits = np.unique(np.concatenate(hits))
    return hits[hits >= 0]


class Script:
    """``steps`` in order (dicts with ``op``), the index to play them on (``bf16``, ``capacity``), the query pool, the model
    state after the last step (``final``), and ``tail``: one more search, answered under the final state, which the GPU test
    leaves pending while it asks for a compaction."""

    def __init__(self, name: str, bf16: bool, capacity: int, row_base: int, seed: int):
        self.name, self.bf16, self.capacity, self.row_base = name, bf16, capacity, row_base
        self.rng = np.random.default_rng(seed)
        self.queries = self.rng.standard_normal((POOL, DIM), dtype=F32)
        self.state = State(bf16)
        self.steps = []
        self.final = self.tail = None

    # the steps, applied to the model as they are recorded
    def append(self, rows, codes):
        self.state.append(rows, codes)
        self.steps.append({"op": "append", "rows": np.ascontiguousarray(rows, F32), "codes": np.ascontiguousarray(codes, np.int32)})

    def append_copies(self, eps: float, scale: float, second_eps: float = 0.0, filler: int = 0):
        parts = [near_copies(self.rng, self.queries, eps, scale, 2)]
        if second_eps:
            parts.append(near_copies(self.rng, self.queries, second_eps, scale, DELETED_CODE[0][1]))
        if filler:
            parts.append(base_rows(self.rng, filler))
        order = self.rng.permutation(sum(len(p[0]) for p in parts))     # (the copies lie scattered among the filler)
        self.append(np.concatenate([p[0] for p in parts])[order], np.concatenate([p[1] for p in parts])[order])

    def tombstone_top(self):
        rows = top_hits(self.state, self.queries)
        self.steps.append({"op": "tombstone", "rows": rows})
        self.state.tombstone(rows)

    def tombstone_filter(self, filters):
        m = self.state.passing(filters)
        self.steps.append({"op": "tombstone_filter", "filters": filters, "cleared": int(m.sum())})
        self.state.alive[m] = False

    def reserve(self, capacity: int):
        self.steps.append({"op": "reserve", "capacity": capacity})

    def clear(self):
        self.steps.append({"op": "clear"})
        self.state.clear()

    def search(self, kind: str, nq: int, k: int):
        self.steps.append(search_step(self.state, kind, self.queries[:nq], k, self.row_base))

    def done(self):
        assert self.steps[-1]["op"] != "search", "a script ends with a mutation"
        self.final = self.state.copy()
        self.tail = search_step(self.final, "plain", self.queries[:33], 10, self.row_base)
        for step in self.searches():
            step["final"] = expect(self.final, step)
        return self

    def searches(self):
        return [s for s in self.steps if s["op"] == "search"]


@functools.lru_cache(maxsize=None)
def script(name: str, bf16: bool) -> Script:
    """The two scripts, per stored precision; built once per process and shared (read only)."""
    if name == "grow":
        # rows come and go under searches of every kind; the capacity is there from the start, row_base 0
        s = Script(name, bf16, capacity=4000, row_base=0, seed=11 + bf16)
        s.append(*base_rows(s.rng, 2000))
        s.search("plain", 33, 10)
        s.append_copies(0.5, 3.0, second_eps=0.7, filler=300)
        s.search("cond", 64, 1)
        s.tombstone_top()
        s.search("multi", 65, 10)
        s.tombstone_filter(DELETED_CODE)
        s.search("range", 1, 257)
        s.append_copies(0.3, 0.25, filler=500)
        s.search("plain", 65, 257)
        s.tombstone_top()
        s.search("cond", 33, 10)
        s.append_copies(0.0, 2.0)
        return s.done()
    if name == "wipe":
        # the index is created full, grows by reserve, is cleared and filled again; row_base beyond 2^32
        s = Script(name, bf16, capacity=2016, row_base=BASE, seed=21 + bf16)
        s.append(*base_rows(s.rng, 2000))
        s.search("range", 64, 10)
        s.reserve(4000)
        s.append_copies(0.5, 0.5, second_eps=0.7, filler=300)
        s.search("multi", 33, 1)
        s.tombstone_filter(DELETED_CODE)
        s.search("plain", 1, 257)
        s.tombstone_top()
        s.search("cond", 65, 10)
        s.clear()
        s.search("plain", 33, 10)
        s.search("range", 65, 1)
        rows, codes = base_rows(s.rng, 2000)
        exact = near_copies(s.rng, s.queries, 0.0, 4.0, 2)
        s.append(np.concatenate([rows, exact[0]]), np.concatenate([codes, exact[1]]))
        return s.done()
    raise KeyError(name)


SCRIPTS = [(name, bf16) for name in ("grow", "wipe") for bf16 in (True, False)]


@functools.lru_cache(maxsize=None)
def window(bf16: bool, row_base_hi: int = BASE):
    """Twelve searches over ONE state -- the four kinds in turn, each with queries of its own, k, nq and row_base varying:
    ``(state, rows, codes, dead, steps)``."""
    rng = np.random.default_rng(31 + bf16)
    rows, codes = base_rows(rng, 3000)
    dead = np.arange(5, 3000, 11)
    state = State(bf16)
    state.append(rows, codes)
    state.tombstone(dead)
    steps = []
    for i in range(12):
        kind = ("plain", "cond", "multi", "range")[i % 4]
        nq, k = (1, 33, 64, 65, 33)[(i + i // 4) % 5], (10, 1, 257)[(i + i // 4) % 3]
        q = rng.standard_normal((nq, DIM), dtype=F32) * F32(rng.uniform(0.1, 10.0))
        q[::3] += F32(0.4) * rows[rng.integers(0, 3000, size=len(q[::3]))]          # (a third lean on stored rows)
        steps.append(search_step(state, kind, q, k, row_base_hi if i % 2 else 0))
    return state, rows, codes, dead, steps


@functools.lru_cache(maxsize=None)
def slot_wrap(n_calls: int, bf16: bool = True):
    """A 96-row index and ``n_calls`` distinct single queries, k = 3: ``(rows, queries, want_scores, want_rows)``."""
    rng = np.random.default_rng(41)
    rows = rng.standard_normal((96, DIM), dtype=F32)
    queries = rng.standard_normal((n_calls, DIM), dtype=F32)
    s, r = orc.cosine_search(rows, queries, 3, bf16=bf16)
    assert len({tuple(x) for x in r.tolist()}) > n_calls // 2, "the answers tell the queries apart"
    return rows, queries, s, r


# ------------------------------------------------------------------ the runner

class NumpyBackend:
    """Host arrays standing for device tensors (the CPU tier)."""
    stream = 0

    @staticmethod
    def put(a):
        return np.array(a, copy=True)

    @staticmethod
    def full(shape, fill, dtype):
        return np.full(shape, fill, dtype)

    @staticmethod
    def get(t):
        return np.asarray(t)


def outputs(step: dict, be) -> dict:
    """The step's outputs as slices of larger buffers, ``GUARD`` rows of fill on either side."""
    nq, k = step["nq"], step["k"]
    big = {"s": be.full((nq + 2 * GUARD, k), FILL_S, "float32"), "r": be.full((nq + 2 * GUARD, k), FILL_R, "int64")}
    if step["kind"] == "range":
        big["c"] = be.full((nq + 2 * GUARD,), FILL_C, "int64")
    return {"big": big, "out": {name: t[GUARD:GUARD + nq] for name, t in big.items()}}


def enqueue(idx, step: dict, io: dict, q, stream) -> None:
    """One deferred search: device queries, device outputs, nothing waited for."""
    o = io["out"]
    if step["kind"] == "multi":
        idx.search_multi(q, step["k"], step["classes"], step["qclass"], row_base=step["row_base"], out_scores=o["s"], out_rows=o["r"], stream=stream)
    elif step["kind"] == "range":
        idx.search_range(q, step["k"], step["thr"], filters=step["filters"], row_base=step["row_base"], out_scores=o["s"], out_rows=o["r"],
                         out_counts=o["c"], stream=stream)
    else:
        idx.search(q, step["k"], filters=step["filters"], row_base=step["row_base"], out_scores=o["s"], out_rows=o["r"], stream=stream)


def prepare(steps, be) -> list:
    """Everything a step needs on the device -- rows and codes of an append, queries and outputs of a search -- made before
    the first step plays, so that nothing between the steps waits."""
    held = []
    for step in steps:
        if step["op"] == "append":
            held.append({"rows": be.put(step["rows"]), "codes": be.put(step["codes"])})
        elif step["op"] == "search":
            held.append(dict(outputs(step, be), q=be.put(step["queries"])))
        else:
            held.append(None)
    return held


def play(idx, steps, held, be) -> None:
    """The steps in order on ``be.stream``; no finish, no wait."""
    for step, h in zip(steps, held):
        op = step["op"]
        if op == "append":
            idx.append(h["rows"], h["codes"], stream=be.stream)
        elif op == "tombstone":
            idx.tombstone(step["rows"])
        elif op == "tombstone_filter":
            assert idx.tombstone_filter(step["filters"]) == step["cleared"]
        elif op == "reserve":
            idx.reserve(step["capacity"])
        elif op == "clear":
            idx.clear()
        else:
            enqueue(idx, step, h, h["q"], be.stream)


def differences(steps, held, be) -> list:
    """After the finish: every search's rows, score bits and counts against its ``want``, and the guard rows against their
    fill.  Returns one line per difference (empty: all equal)."""
    bad = []
    for i, (step, h) in enumerate(zip(steps, held)):
        if step["op"] != "search":
            continue
        what = f"step {i} ({step['kind']} nq={step['nq']} k={step['k']})"
        ws, wr, wc = step["want"]
        big = {name: be.get(t) for name, t in h["big"].items()}
        nq = step["nq"]
        gr, gs = big["r"][GUARD:GUARD + nq], np.ascontiguousarray(big["s"][GUARD:GUARD + nq], dtype=F32)
        if not np.array_equal(gr, wr):
            q = int(np.argwhere((gr != wr).any(1))[0, 0])
            bad.append(f"{what}: rows differ, first at query {q}: {gr[q, :4].tolist()} for {wr[q, :4].tolist()}")
        if not np.array_equal(gs.view(np.uint32), ws.view(np.uint32)):
            bad.append(f"{what}: score bits differ")
        if wc is not None and not np.array_equal(big["c"][GUARD:GUARD + nq], wc):
            bad.append(f"{what}: counts differ: {big['c'][GUARD:GUARD + nq][:6].tolist()} for {wc[:6].tolist()}")
        for name, fill in (("s", FILL_S), ("r", FILL_R), ("c", FILL_C)):
            if name in big and not ((big[name][:GUARD] == fill).all() and (big[name][GUARD + nq:] == fill).all()):
                bad.append(f"{what}: guard rows of '{name}' were written")
    return bad


# ------------------------------------------------------------------ the fake index of the CPU tier

class DeferredFakeIndex(RangeFakeIndex):
    """``RangeFakeIndex`` with range conditions, ``search_multi``, ``clear`` and DEFERRED calls: a search given ``out_*`` arrays
    writes nothing until ``search_finish``.  ``late=False`` is the contract: the answer is computed at the call, for the index
    as it is then.  ``late=True`` is the fault the scripts are made to catch: the answer is computed at the finish, for the
    index as it is by then (a forced re-run on a library that lets mutations pass pending searches)."""
    late = False

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.pending = []

    def _mask(self, filters=None):
        return np_mask(self.codes, self.alive, filters)

    def clear(self):
        self.x, self.codes, self.alive = self.x[:0], self.codes[:0], self.alive[:0]
        if self.late:
            self.pending = []

    def tombstone_filter(self, filters):
        m = self._mask(filters)
        self.alive[m] = 0
        return int(m.sum())

    def compact(self):
        if self.pending:
            raise RuntimeError("compact: searches with device outputs are pending")
        return super().compact()

    def _multi(self, queries, k, class_filters, query_class, row_base):
        queries, query_class = np.asarray(queries, F32), np.asarray(query_class)
        s, r = np.empty((len(queries), k), F32), np.empty((len(queries), k), np.int64)
        for c, filters in enumerate(class_filters):
            sel = np.flatnonzero(query_class == c)
            if sel.size:
                s[sel], r[sel] = _fake_search(self, queries[sel], k, filters, row_base)
        return s, r

    def _defer(self, compute, outs):
        if not self.late:
            vals = compute()
            compute = lambda: vals
        self.pending.append((compute, outs))

    def search(self, queries, k, filters=None, row_base=0, out_scores=None, out_rows=None, stream=0):
        compute = lambda: _fake_search(self, queries, k, filters, row_base)
        if out_scores is None:
            return compute()
        self._defer(compute, (out_scores, out_rows))

    def search_multi(self, queries, k, class_filters, query_class, row_base=0, out_scores=None, out_rows=None, stream=0):
        compute = lambda: self._multi(queries, k, class_filters, query_class, row_base)
        if out_scores is None:
            return compute()
        self._defer(compute, (out_scores, out_rows))

    def search_range(self, queries, k, thresholds, filters=None, row_base=0, counts=True, out_scores=None, out_rows=None, out_counts=None, stream=0):
        compute = lambda: RangeFakeIndex.search_range(self, queries, k, thresholds, filters=filters, row_base=row_base, counts=counts)
        if out_scores is None:
            return compute()
        self._defer(compute, (out_scores, out_rows, out_counts))

    def search_finish(self, stream=0):
        todo, self.pending = self.pending, []
        for compute, outs in todo:
            for o, v in zip(outs, compute()):
                o[...] = v


def _fake_search(idx, queries, k, filters, row_base):
    """``FakeIndex.search`` under any filter ``np_mask`` knows."""
    q = orc.preprocess(np.asarray(queries, F32).reshape(-1, idx.dim), to_bf16=(idx.dtype == 1))
    if len(idx.x) == 0:
        return np.full((len(q), k), -np.inf, F32), np.full((len(q), k), -1, np.int64)
    s, r = orc.search(idx.x, q, k, alive=idx._mask(filters).astype(np.uint8))
    return s, np.where(r >= 0, r + row_base, r)
