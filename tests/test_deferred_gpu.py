"""Searches with device outputs that stay pending -- across calls of other kinds, across mutations of the index, across more
calls than there are status slots, across streams -- and have to be RUN AGAIN at the finish (tests/deferred_cases.py,
DESIGN.md 3.29).  Every search must answer for the index at its place in the order of calls: ids and f32 score bits against
the oracle, counts against the range restatement.  The re-runs are forced through the three bounded tuning hooks
(``set_tuning(force_fallback=1 | 2 | 3)``); every output is a slice of a larger tensor whose guard rows must keep their fill."""
import numpy as np
import pytest

from tests import deferred_cases as dc
from tests.test_search_gpu import policy  # noqa: F401  (the fixture: int8 copy from 0 rows / the product's default)

pytestmark = pytest.mark.gpu
G = dc.GUARD


def _ffi():
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    return ffi


class TorchBackend:
    """Device tensors on cuda:0; ``stream`` is the raw handle the calls are enqueued on."""

    def __init__(self, stream=None):
        import torch
        self.torch = torch
        self.stream = torch.cuda.current_stream().cuda_stream if stream is None else stream

    def put(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    def full(self, shape, fill, dtype):
        return self.torch.full(tuple(shape), float(fill) if dtype == "float32" else int(fill), dtype=getattr(self.torch, dtype), device="cuda:0")

    @staticmethod
    def get(t):
        return t.cpu().numpy()


def _index(ffi, bf16, capacity, rows=None, codes=None, dead=None, cols=2):
    idx = ffi.Index(dc.DIM, ffi.DTYPE_BF16 if bf16 else ffi.DTYPE_F32, capacity_rows=capacity, n_code_cols=cols, device=0)
    if rows is not None:
        idx.append(rows, codes)
    if dead is not None:
        idx.tombstone(dead)
    return idx


def _window(idx, steps, be, mode):
    """The twelve calls enqueued under ``force_fallback=mode``, one finish: ``(held, fallback bits)``."""
    held = dc.prepare(steps, be)
    be.torch.cuda.synchronize()
    idx.set_tuning(force_fallback=mode)
    dc.play(idx, steps, held, be)
    idx.search_finish(be.stream)
    bits = idx.stats()["fallback_used"]
    idx.set_tuning(force_fallback=0)
    return held, bits


def _bits(held):
    return [{name: t.cpu().numpy().tobytes() for name, t in h["big"].items()} for h in held]


# ------------------------------------------------------------------ A. mixed kinds, one window

@pytest.mark.parametrize("bf16", [True, False])
def test_all_four_kinds_pending_in_one_window_and_run_again(gpu, bf16, policy):
    """crh_search, crh_search_cond, crh_search_multi and crh_search_range in turn, twelve calls with k, nq and row_base of
    their own, nothing finished in between; then ONE finish that has to run every batch again (1: regrown buffers; 3: the int8
    batches are sent to the bf16 scan).  The re-run of one kind works in the workspace the next kind's first run left."""
    ffi = _ffi()
    state, rows, codes, dead, steps = dc.window(bf16)
    idx = _index(ffi, bf16, len(rows), rows, codes, dead)
    be = TorchBackend()
    try:
        plain, bits0 = _window(idx, steps, be, 0)
        assert dc.differences(steps, plain, be) == [] and bits0 == 0
        for mode in (1, 3):
            held, bits = _window(idx, steps, be, mode)
            print(f"bf16 {bf16} {policy} force_fallback {mode}: fallback_used {bits} nomination {idx.nomination()}")
            assert dc.differences(steps, held, be) == [], mode
            assert bits & 1, (mode, bits)                      # (multi and range batches always regrow the bf16 scan's buffers)
            if mode == 3 and policy == "int8 copy from 0 rows":
                assert bits & 4, bits                          # the int8-nominated batches gave way to the bf16 scan
            assert _bits(held) == _bits(plain), "forced re-runs give the bits of the plain window, guard rows included"
    finally:
        idx.close()


def test_one_launch_scans_that_time_out_in_a_window_of_mixed_kinds(gpu):
    """The same window on the one-launch scan over the bf16 tiles with its first grid-wide wait made to give up
    (``force_fallback=2`` on ``NOMINATE_BF16``, the hook of test_fused_scan_that_times_out_is_run_again_in_the_three_kernel_form:
    a bounded wait of milliseconds).  The void batches are found at the finish, behind batches of the other kinds."""
    ffi = _ffi()
    state, rows, codes, dead, steps = dc.window(True)
    idx = _index(ffi, True, len(rows), rows, codes, dead)
    be = TorchBackend()
    try:
        idx.set_nomination(ffi.NOMINATE_BF16)
        plain, bits0 = _window(idx, steps, be, 0)
        assert dc.differences(steps, plain, be) == [] and bits0 == 0 and idx.nomination() == ffi.NOMINATE_BF16
        held, bits = _window(idx, steps, be, 2)
        assert dc.differences(steps, held, be) == []
        assert bits & 2, bits
        assert _bits(held) == _bits(plain)
    finally:
        idx.close()


# ------------------------------------------------------------------ B. mutations between pending searches

@pytest.mark.parametrize("mode", [0, 1, 3])
@pytest.mark.parametrize("name,bf16", dc.SCRIPTS)
def test_mutations_between_pending_searches(gpu, name, bf16, mode, policy):
    """The scripts of tests/deferred_cases.py, nothing waited for between the steps, the finish at the very end: later appends
    are not visible to a search, later tombstones still are, a search before ``reserve`` or ``clear`` keeps its answer and one
    after ``clear`` is all padding -- also when every batch has to run again (modes 1 and 3).  ``compact`` with searches
    pending is refused and works after the finish.

    Before mutations completed the pending searches, modes 1 and 3 failed here with id mismatches at every search step (the
    re-run answered for the final index; ``clear`` dropped the batches and left their clipped first answers): DESIGN.md 3.29."""
    ffi = _ffi()
    s = dc.script(name, bf16)
    steps = s.steps + [s.tail]
    idx = _index(ffi, bf16, s.capacity)
    be = TorchBackend()
    try:
        held = dc.prepare(steps, be)
        be.torch.cuda.synchronize()
        idx.set_tuning(force_fallback=mode)
        dc.play(idx, steps, held, be)
        with pytest.raises(ffi.NativeError, match="pending") as refused:
            idx.compact()
        assert refused.value.code == ffi.E_INVALID
        idx.search_finish(be.stream)
        bits = idx.stats()["fallback_used"]
        idx.set_tuning(force_fallback=0)
        bad = dc.differences(steps, held, be)
        print(f"{name} bf16 {bf16} {policy} force_fallback {mode}: fallback_used {bits}, {len(bad)} differences")
        assert bad == []
        assert (bits & 5) if mode else bits == 0, bits
        assert idx.count() == (len(s.final.pre), int(s.final.alive.sum()))
        o2n = idx.compact()
        assert np.array_equal(o2n >= 0, s.final.alive) and np.array_equal(o2n[s.final.alive], np.arange(int(s.final.alive.sum())))
        assert idx.count() == (int(s.final.alive.sum()),) * 2
    finally:
        idx.close()


# ------------------------------------------------------------------ C. more pending calls than status slots

@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("bf16", [True, False])
def test_more_pending_searches_than_status_slots(gpu, bf16, mode, policy):
    """1 030 single-query searches with no finish in between: kStatusSlots + 6 (``constexpr int kStatusSlots = 1024`` in
    code-rag_amd/csrc/crh_index.hip), so the call that finds every slot taken completes the 1 024 pending batches itself and the
    slots are handed out again from 0.  Every call has a query of its own and its own row of one [1030, 3] output."""
    ffi = _ffi()
    n_calls = 1030
    rows, queries, ws, wr = dc.slot_wrap(n_calls, bf16)
    idx = _index(ffi, bf16, 96, rows, None, cols=0)
    be = TorchBackend()
    try:
        qd = be.put(queries)
        out_s, out_r = be.full((n_calls + 2 * G, 3), dc.FILL_S, "float32"), be.full((n_calls + 2 * G, 3), dc.FILL_R, "int64")
        be.torch.cuda.synchronize()
        idx.set_tuning(force_fallback=mode)
        for i in range(n_calls):
            idx.search(qd[i:i + 1], 3, out_scores=out_s[G + i:G + i + 1], out_rows=out_r[G + i:G + i + 1], stream=be.stream)
        idx.search_finish(be.stream)
        print(f"bf16 {bf16} {policy} force_fallback {mode}: fallback_used {idx.stats()['fallback_used']}")
        idx.set_tuning(force_fallback=0)
        gs, gr = out_s.cpu().numpy(), out_r.cpu().numpy()
        assert np.array_equal(gr[G:-G], wr), f"rows differ first at call {int(np.argwhere((gr[G:-G] != wr).any(1))[0, 0])}"
        assert np.array_equal(gs[G:-G].view(np.uint32), ws.view(np.uint32))
        assert (gs[:G] == dc.FILL_S).all() and (gs[-G:] == dc.FILL_S).all() and (gr[:G] == dc.FILL_R).all() and (gr[-G:] == dc.FILL_R).all()
    finally:
        idx.close()


# ------------------------------------------------------------------ D. the finish is handed another stream

def _behind_a_long_kernel(torch, stream, qd):
    """The matmul chain of test_searches_see_what_the_stream_did_before_them on ``stream``, and the queries as a result of it."""
    with torch.cuda.stream(stream):
        big = torch.randn((6144, 6144), device=qd.device)
        for _ in range(4):
            big = big @ big * 1e-3
        q2 = torch.empty_like(qd)
        q2.copy_(qd + big[:qd.shape[0], :qd.shape[1]] * 0.0)
    return q2, big


def _two_concurrent_streams(torch):
    """``(A, B, shown)``: two streams, and whether work on B was SEEN to run while A was busy.  Streams are mapped onto a few
    hardware queues, and two that share one run their work in the order it was queued: B is then no "other stream" to A, and a
    finish that waits for B alone has waited for A as well.  So: a few milliseconds of matmuls on A, one small kernel on each
    candidate B, and B is taken if its kernel is done while A's are not."""
    import time
    cands = [torch.cuda.Stream() for _ in range(8)]
    a = cands[0]
    x = torch.randn((4096, 4096), device="cuda:0")
    flag = torch.zeros(1, device="cuda:0")
    _ = x @ x                                                    # (the BLAS library is loaded before anything is timed)
    torch.cuda.synchronize()
    for b in cands[1:]:
        with torch.cuda.stream(a):
            y = x
            for _ in range(3):
                y = y @ x * 1e-2
            ea = torch.cuda.Event()
            ea.record()
        with torch.cuda.stream(b):
            flag.add_(1)
            eb = torch.cuda.Event()
            eb.record()
        t0 = time.perf_counter()
        while not eb.query() and not ea.query() and time.perf_counter() - t0 < 0.05:
            pass
        shown = eb.query() and not ea.query()
        torch.cuda.synchronize()
        if shown:
            return a, b, True
    return a, cands[1], False


@pytest.mark.parametrize("bf16", [True, False])
def test_finish_through_another_stream(gpu, bf16, policy):
    """A search enqueued on stream A behind milliseconds of matmuls, its re-run forced, and ``search_finish`` called with an
    idle stream B: the outputs are final when the call returns (they are read on a third stream that waits for neither).  Then
    batches pending on A (behind the chain again) and on B at once, and one finish.

    Each form opens with searches of the same kinds BEFORE the chain: the first call under ``force_fallback=1`` reallocates
    the workspace to the hook's tiny buffers, the first call of a kind allocates that kind's masks, and freeing device memory
    waits for the whole device -- such a call behind the chain waits the chain out itself and leaves nothing to prove (the
    first version of this test did, and passed on the old library three times in four).

    This test cannot fail spuriously: if the chain happens to end before the finish is called -- a host that stalls between the
    two calls -- or if no stream is found that runs beside A (``_two_concurrent_streams``; the test prints which), a finish that
    waits for the wrong stream reads a status that is already there, and the test passes without having proved anything.  Before ``Pending`` recorded its stream both forms failed here (the status was read before the
    batch had run, its clipped first answer was returned as final): DESIGN.md 3.29."""
    import torch
    ffi = _ffi()
    state, rows, codes, dead, steps = dc.window(bf16)
    idx = _index(ffi, bf16, len(rows), rows, codes, dead)
    A, B, shown = _two_concurrent_streams(torch)
    print(f"bf16 {bf16} {policy}: work on B seen to overtake work on A: {shown}")
    on_a, on_b = TorchBackend(A.cuda_stream), TorchBackend(B.cuda_stream)
    try:
        # a mixed-filter search (k = 1), then -- behind the chain -- another (64 queries, k = 257) on A; finished through B
        mine = [steps[6], steps[2]]
        held = dc.prepare(mine, on_a)
        torch.cuda.synchronize()
        idx.set_tuning(force_fallback=1)
        dc.enqueue(idx, mine[0], held[0], held[0]["q"], A.cuda_stream)
        q2, keep = _behind_a_long_kernel(torch, A, held[1]["q"])
        dc.enqueue(idx, mine[1], held[1], q2, A.cuda_stream)
        idx.search_finish(B.cuda_stream)
        bits = idx.stats()["fallback_used"]
        bad = dc.differences(mine, held, on_a)                   # (read at once, on the default stream: no wait for A)
        assert bad == [] and bits & 1, (bad, bits)
        # pending on A and on B at once: cond on B and range on A; then, behind the chain, range (65 queries, counts) on A,
        # multi on B, plain on A
        torch.cuda.synchronize()
        mine_a, mine_b = [steps[7], steps[3], steps[4]], [steps[5], steps[10]]
        held_a, held_b = dc.prepare(mine_a, on_a), dc.prepare(mine_b, on_b)
        torch.cuda.synchronize()
        dc.enqueue(idx, mine_b[0], held_b[0], held_b[0]["q"], B.cuda_stream)
        dc.enqueue(idx, mine_a[0], held_a[0], held_a[0]["q"], A.cuda_stream)
        q2, keep = _behind_a_long_kernel(torch, A, held_a[1]["q"])
        dc.enqueue(idx, mine_a[1], held_a[1], q2, A.cuda_stream)
        dc.enqueue(idx, mine_b[1], held_b[1], held_b[1]["q"], B.cuda_stream)
        dc.enqueue(idx, mine_a[2], held_a[2], held_a[2]["q"], A.cuda_stream)
        idx.search_finish(B.cuda_stream)
        bits = idx.stats()["fallback_used"]
        bad = dc.differences(mine_a, held_a, on_a) + dc.differences(mine_b, held_b, on_b)
        assert bad == [] and bits & 1, (bad, bits)
    finally:
        torch.cuda.synchronize()
        idx.close()
