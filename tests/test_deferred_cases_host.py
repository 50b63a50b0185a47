"""The scripts of tests/deferred_cases.py hold what they claim, their expectations agree with a float64 ranking, and the
runner tells an index that answers for the state at the call from one that answers for the state at the finish.  No GPU."""
import numpy as np
import pytest

from oracle import search as orc
from tests import deferred_cases as dc

F32 = np.float32
# |f32 canonical score - exact score| for unit vectors: at most dim roundings of 2^-24 each on terms whose absolute sum is <= 1
# (a bf16 store rounds the VECTORS, which both sides then share); twice that separates two scores whatever their errors
TOL = 2.0 * dc.DIM * 2.0 ** -24


@pytest.mark.parametrize("name,bf16", dc.SCRIPTS)
def test_every_mutation_changes_every_answer(name, bf16):
    s = dc.script(name, bf16)
    kinds = {st["kind"] for st in s.searches()}
    assert kinds == {"plain", "cond", "multi", "range"} and s.steps[-1]["op"] != "search"
    assert {st["nq"] for st in s.searches()} >= {1, 33, 65} and {st["k"] for st in s.searches()} == {1, 10, 257}
    qpre = orc.preprocess(s.queries, to_bf16=bf16)
    state = dc.State(bf16)
    appended = 0
    for i, st in enumerate(s.steps):
        if st["op"] == "append":
            first = len(state.pre)
            state.append(st["rows"], st["codes"])
            if appended:                                         # (the first append is the corpus itself)
                # the appended rows take rank 1 of every query, under every filter in use
                for f in dc.FILTERS_IN_USE:
                    top = orc.search(state.pre, qpre, 1, alive=state.passing(f).astype(np.uint8))[1].ravel()
                    assert (top >= first).all(), (i, f)
            appended += 1
        elif st["op"] == "tombstone":
            # each query's current top hit goes, under every filter in use
            for f in dc.FILTERS_IN_USE:
                top = orc.search(state.pre, qpre, 1, alive=state.passing(f).astype(np.uint8))[1].ravel()
                assert np.isin(top, st["rows"]).all(), (i, f)
            state.tombstone(st["rows"])
        elif st["op"] == "tombstone_filter":
            # the deleted code value holds a hit of every query: in its top 10 under every filter that lets the value through
            m = state.passing(st["filters"])
            assert int(m.sum()) == st["cleared"] > 0
            for f in dc.FILTERS_IN_USE:
                top = orc.search(state.pre, qpre, 10, alive=state.passing(f).astype(np.uint8))[1]
                assert m[top].any(1).all(), (i, f)
            state.alive[m] = False
        elif st["op"] == "clear":
            state.clear()
        elif st["op"] == "search":
            got = dc.expect(state, st)                           # the replayed model gives the recorded expectation
            assert all(np.array_equal(a, b) for a, b in zip(got[:2], st["want"][:2]))
            # ... and the final state would answer EVERY query differently
            same = (st["want"][1] == st["final"][1]).all(1)
            assert not same.any(), f"step {i}: queries {np.flatnonzero(same).tolist()} have the final state's answer"
            if len(state.pre) == 0:
                assert (st["want"][1] == -1).all() and np.isneginf(st["want"][0]).all()
    assert np.array_equal(state.alive, s.final.alive) and len(s.final.pre) > 0
    assert s.row_base in (0, dc.BASE) and {x.row_base for x in map(lambda nb: dc.script(*nb), dc.SCRIPTS)} == {0, dc.BASE}


def _check_fp64(state, st):
    """The expected lists against a float64 ranking of the same stored vectors, wherever its score gaps exceed ``TOL``."""
    nq, k = st["nq"], st["k"]
    ws, wr, wc = st["want"]
    if len(state.pre) == 0:
        return 0
    q64 = orc.preprocess(st["queries"], to_bf16=state.bf16).astype(np.float64)
    s64 = q64 @ state.pre.astype(np.float64).T
    checked = 0
    for q in range(nq):
        filters = st["classes"][st["qclass"][q]] if st["kind"] == "multi" else st["filters"]
        ok = state.passing(filters)
        if st["kind"] == "range":
            thr = float(st["thr"][q])
            sure, maybe = ok & (s64[q] >= thr + TOL), ok & (s64[q] >= thr - TOL)
            assert sure.sum() <= wc[q] <= maybe.sum()
            ok = maybe
            limit = int(sure.sum())                              # (ranks beyond this may or may not be in range)
        else:
            limit = int(ok.sum())
        rows = np.flatnonzero(ok)
        order = rows[np.lexsort((rows, -s64[q, rows]))]
        vals = s64[q, order]
        for j in range(min(k, limit)):
            clear_above = j == 0 or vals[j - 1] - vals[j] > TOL
            clear_below = j + 1 >= len(vals) or vals[j] - vals[j + 1] > TOL
            if clear_above and clear_below:
                assert wr[q, j] == order[j] + st["row_base"], (q, j)
                assert abs(float(ws[q, j]) - vals[j]) <= TOL
                checked += 1
        if st["kind"] != "range":
            assert (wr[q, limit:] == -1).all()
    return checked


@pytest.mark.parametrize("name,bf16", dc.SCRIPTS)
def test_expectations_agree_with_a_float64_ranking(name, bf16):
    s = dc.script(name, bf16)
    state = dc.State(bf16)
    checked = total = 0
    for st in s.steps:
        if st["op"] == "search":
            checked += _check_fp64(state, st)
            total += int((st["want"][1] >= 0).sum())
        elif st["op"] == "append":
            state.append(st["rows"], st["codes"])
        elif st["op"] in ("tombstone", "tombstone_filter"):
            state.alive[st["rows"] if st["op"] == "tombstone" else state.passing(st["filters"])] = False
        elif st["op"] == "clear":
            state.clear()
    # (the k = 257 lists reach into the bulk of ~1 500 random scores of spread 0.05, where neighbours lie about 1e-4 apart --
    # the size of TOL -- and many ranks are skipped; the short lists and the near copies at their heads are all clear)
    assert checked > total // 2, (checked, total)


@pytest.mark.parametrize("bf16", [True, False])
def test_the_window_mixes_kinds_shapes_and_row_bases(bf16):
    state, rows, codes, dead, steps = dc.window(bf16)
    assert [st["kind"] for st in steps] == ["plain", "cond", "multi", "range"] * 3
    assert {st["nq"] for st in steps} == {1, 33, 64, 65} and {st["k"] for st in steps} == {1, 10, 257}
    assert {st["row_base"] for st in steps} == {0, dc.BASE}
    assert len({(st["nq"], st["k"], st["kind"]) for st in steps}) == 12
    assert sum(_check_fp64(state, st) for st in steps) > sum(int((st["want"][1] >= 0).sum()) for st in steps) // 2
    for st in steps:
        hit = st["want"][1] >= 0
        assert (st["want"][1][hit] >= st["row_base"]).all() and not np.isin(st["want"][1][hit] - st["row_base"], dead).any()
    want = dc.slot_wrap(40)
    assert want[3].shape == (40, 3) and (want[3] >= 0).all()


def _fake(s, late):
    idx = dc.DeferredFakeIndex(dc.DIM, int(s.bf16), capacity_rows=s.capacity, n_code_cols=2)
    idx.late = late
    return idx


@pytest.mark.parametrize("name,bf16", dc.SCRIPTS)
def test_the_runner_against_the_fake_index(name, bf16):
    """The contract (answers computed at the call) passes; the fault (answers computed at the finish, pending searches dropped
    by clear) is reported for EVERY search step -- the harness sees what it was built to see."""
    s = dc.script(name, bf16)
    be = dc.NumpyBackend
    steps = s.steps + [s.tail]
    idx = _fake(s, late=False)
    held = dc.prepare(steps, be)
    dc.play(idx, steps, held, be)
    with pytest.raises(RuntimeError, match="pending"):
        idx.compact()
    idx.search_finish()
    assert dc.differences(steps, held, be) == []
    o2n = idx.compact()
    assert np.array_equal(o2n >= 0, s.final.alive) and idx.count() == (int(s.final.alive.sum()),) * 2

    idx = _fake(s, late=True)
    held = dc.prepare(steps, be)
    dc.play(idx, steps, held, be)
    idx.search_finish()
    bad = dc.differences(steps, held, be)
    for i, st in enumerate(s.steps):
        if st["op"] == "search":
            assert any(line.startswith(f"step {i} ") and "rows differ" in line for line in bad), (i, bad)
    assert not any(line.startswith(f"step {len(s.steps)} ") for line in bad)       # (the tail has no later state to be confused with)


def test_the_runner_reports_written_guard_rows():
    s = dc.script("grow", True)
    be = dc.NumpyBackend
    steps = [s.tail]
    idx = _fake(s, late=False)
    idx.append(s.final.pre, s.final.codes, preprocessed=True)
    idx.alive[:] = s.final.alive
    held = dc.prepare(steps, be)
    dc.play(idx, steps, held, be)
    assert (held[0]["big"]["r"] == dc.FILL_R).all()              # deferred: nothing is written before the finish
    idx.search_finish()
    assert dc.differences(steps, held, be) == []
    held[0]["big"]["s"][0, 0] = 0.0
    held[0]["big"]["r"][-1, -1] = 5
    assert len(dc.differences(steps, held, be)) == 2
