"""The life-cycle script of tests/lifecycle_cases.py without a device: what the script promises, read from the model alone; the
model's placement against ``ShardSet.route``; and the warm and the cold schedule on an oracle-backed fake index for the read
paths such an index serves (tests/test_lifecycle_gpu.py runs every read path on the HIP index)."""
import asyncio

import pytest

import coderag_amd  # noqa: F401
from coderag_amd import ffi, shards as shards_mod, store as store_mod
from oracle import search as orc
from tests import lifecycle_cases as lc, span_cases
from tests.fake_index import FakeIndex
from tests.test_filter_sets_host import SetFakeIndex
from tests.test_store_host import fake  # noqa: F401  (the fixture)

BLOCK = 32


class LifeFakeIndex(SetFakeIndex):
    """``FakeIndex`` with set and range conditions (``span_cases.np_mask``: the numpy form of ``crh_condition``)."""

    def _mask(self, filters=None):
        return span_cases.np_mask(self.codes, self.alive, filters)


@pytest.fixture(scope="module")
def dry():
    """The warm script on the model alone (one and three shards), with the model's state after every phase."""
    out = {}
    for ns in (1, 3):
        sc = lc.Script(None, ns, BLOCK, "warm", lc.FULL, False)
        seen = {}

        def hook(phase, script, seen=seen):
            m = script.model
            seen[phase] = {"slot": {r[0]: t for t, r in m.live()}, "place": {r[0]: (r[4], r[5]) for _, r in m.live()},
                           "vec": {r[0]: r[1].tobytes() for _, r in m.live()}, "pay": {r[0]: r[2] for _, r in m.live()},
                           "rows": len(m.rows), "alive": m.alive, "shard_rows": list(m.shard_rows)}
        sc.hook = hook
        asyncio.run(sc.run())
        out[ns] = (sc, seen)
    return out


def test_the_scripts_preconditions_hold_on_the_model(dry):
    assert lc.STRIDE == shards_mod.STRIDE
    for ns, (sc, seen) in dry.items():
        ids = [lc.point(i)[0] for i in range(400)]
        two = seen[2]
        # the ties exist: two live points with bit-identical vectors, both at the top of the query beside them
        a, b = ids[lc.TIE[0]], ids[lc.TIE[1]]
        assert two["vec"][a] == two["vec"][b] and two["pay"][a] != two["pay"][b]
        v = _model_at(ns, 2).view(False)
        s, r, _ = v.top(lc.Q[2], 2)
        assert {v.pids[j] for j in r[0]} == {a, b} and lc.bits(s[0, 0]) == lc.bits(s[0, 1])
        assert [v.pids[j] for j in r[0]] == sorted((a, b), key=lambda i: two["place"][i][0] * lc.STRIDE + two["place"][i][1])
        # identical texts (BM25 ties) and the payload edge cases are live
        texts = [p.get("content") for p in two["pay"].values()]
        assert texts.count(lc.TIED_TEXT) >= 3 and None in texts and 12345 in texts
        assert any("file_path" not in p for p in two["pay"].values()) and any("start_line" not in p for p in two["pay"].values())
        assert any(len(p["entity_name"].lower().encode()) != len(p["entity_name"].encode()) for p in two["pay"].values())
        # the merge key collides, and both points are among the candidates of the re-rank's fourth query
        c, d = two["pay"][ids[lc.MERGE[0]]], two["pay"][ids[lc.MERGE[1]]]
        assert (c["file_path"], c["entity_name"], c["start_line"]) == (d["file_path"], d["entity_name"], d["start_line"])
        ok = v.mask({"language": "python"})
        _, r, _ = v.top(lc.Q[3], 20, ok)
        assert {ids[lc.MERGE[0]], ids[lc.MERGE[1]]} <= {v.pids[j] for j in r[0]}
        # the repeated id of phase 2: the last one won
        assert two["pay"][ids[110]]["content"].endswith("first_copy\n") and two["rows"] == 180
        # the replaced example moved to the end, and with more than one shard to another row
        ex = lc.EXAMPLES[0][0]
        assert seen[3]["slot"][ex] == 7 and seen[4]["slot"][ex] == seen[3]["rows"] and seen[4]["vec"][ex] != seen[3]["vec"][ex]
        assert seen[4]["place"][ex] != seen[3]["place"][ex] and seen[4]["rows"] - seen[4]["alive"] == 5
        assert all(all(i in seen[p]["slot"] for i in lc.EXAMPLES[0] + lc.EXAMPLES[1]) for p in range(2, 13))
        # compaction keeps the order; phase 7 goes on at the new end
        order5 = [i for i in seen[5]["slot"]]
        assert [i for i in seen[6]["slot"]] == order5 and seen[6]["rows"] == seen[6]["alive"] == seen[5]["alive"] < seen[5]["rows"]
        assert list(seen[7]["slot"])[: len(order5)] == order5 and sum(seen[7]["shard_rows"]) == seen[6]["rows"] + 100
        # phase 8 crosses the threshold in exactly the two named calls, nowhere else
        assert [e[0] for e in sc.model.log if e[1]] == list(lc.AUTO_CALLS)
        for label, crossed, dead, rows in sc.model.log:
            assert crossed == (dead >= sc.model.min_dead and dead >= sc.model.dead_fraction * rows), label
        # phase 11 saves with dead rows present
        assert seen[11]["rows"] > seen[11]["alive"]
        # no check is vacuous: outside the empty phases every filter keeps some and drops some, every answer holds something
        assert len(sc.report) == 15
        for where, vacuous in sc.report:
            if where in ("after phase 1", "phase 12, cleared"):
                assert len(vacuous) > 30, where
            else:
                assert vacuous == [], (where, vacuous)
        assert max(s["rows"] for s in seen.values()) < 400


def _model_at(ns: int, phase: int):
    """The model of a fresh dry run stopped at the end of ``phase``."""
    class Stop(Exception):
        pass
    sc = lc.Script(None, ns, BLOCK, "cold", (), False)

    def hook(p, script):
        if p == phase:
            raise Stop
    sc.hook = hook
    try:
        asyncio.run(sc.run())
    except Stop:
        pass
    return sc.model


@pytest.mark.parametrize("ns", [1, 2, 3])
def test_the_models_placement_is_shardsets(ns):
    sh = shards_mod.ShardSet(ns, lambda s: FakeIndex(dim=8, capacity_rows=64), block=5)
    m = lc.Model(ns=ns, block=5)
    for n in (3, 5, 12, 1, 26, 4, 10):
        assert m.route(n) == sh.route(n).tolist() and m.next_block == sh._next_block
    saved = sh._next_block                                   # a refused call puts the round robin back
    sh.route(7)
    sh._next_block = saved
    m.refused(7)
    assert m.route(11) == sh.route(11).tolist()
    # rows, per shard, in the order they came: the local row of every point, before and after a compaction
    m = lc.Model(ns=ns, block=5)
    ids, vecs, pays = lc.points(range(23))
    m.upsert(ids[:9], vecs[:9], pays[:9])
    m.upsert(ids[9:], vecs[9:], pays[9:])
    per = {s: [r[5] for r in m.rows if r[4] == s] for s in range(ns)}
    assert all(v == list(range(len(v))) for v in per.values()) and m.shard_rows == [len(per[s]) for s in range(ns)]
    m.delete(lambda p: p["language"] == "go")
    before = [(r[0], r[4]) for _, r in m.live()]
    assert m.compact() == 23 - len(before) and [(r[0], r[4]) for r in m.rows] == before
    per = {s: [r[5] for r in m.rows if r[4] == s] for s in range(ns)}
    assert all(v == list(range(len(v))) for v in per.values()) and m.compact() == 0 and m.compactions == 1


@pytest.mark.parametrize("schedule", ["warm", "cold"])
@pytest.mark.parametrize("ns", [1, 3])
def test_the_script_on_the_fake_index(fake, monkeypatch, ns, schedule):  # noqa: F811
    monkeypatch.setattr(ffi, "Index", LifeFakeIndex)
    monkeypatch.setattr(ffi, "use_device", lambda d: None)
    orig = shards_mod.ShardSet.__init__

    def small_blocks(self, *a, **kw):
        kw["block"] = BLOCK
        orig(self, *a, **kw)
    monkeypatch.setattr(shards_mod.ShardSet, "__init__", small_blocks)

    def make_store():
        return store_mod.HipVectorStore(dim=lc.DIM, initial_capacity=64, shards=ns, stream="default", _merge_fn=orc.merge_topk, **lc.AUTO_COMPACT)
    sc = lc.Script(make_store, ns, BLOCK, schedule, lc.HOST, False)
    asyncio.run(sc.run())
    assert sc.checked == (16 if schedule == "warm" else 6) and len(sc.compared) == lc.checks_in(lc.HOST) * sc.checked > 15 * sc.checked
    assert [e[0] for e in sc.model.log if e[1]] == list(lc.AUTO_CALLS)
