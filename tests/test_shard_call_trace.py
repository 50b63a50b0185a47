"""What the store's search features ask of the indexes, the selectors, the merge and the collectives -- as a recorded trace.

One call of every select-on-device feature goes through the public ``HipVectorStore`` API over a seeded 600-row, dim-32
collection on the fake indexes, at 1 and 3 local shards and on two gloo ranks.  A recording subclass of the fake index, recording
wrappers around the patched ``ffi.*_select`` / the injected merge and a recording ``dist`` shim log every call: the method, ``k``,
``row_base``, the filter, array shapes and dtypes, the reduce op.  The log and the returned hits (score bits included) must equal
``tests/golden/shard_call_trace.json``, which this very recorder wrote on the commit BEFORE the candidate pipeline of
``shards.py`` was consolidated: the host half of "same index calls, same selector calls, same collectives".  Regenerate with
``python -m tests.test_shard_call_trace`` (only when a change of the trace is intended).

One difference is known and wanted: recommend used to read its examples' and candidates' vectors row by row (``read_rows``, not
recorded) and now gathers them like MMR does, so ``gather_vectors`` entries are left out of the recommend traces -- their
all-reduce is recorded, and unchanged.  Lexical and hybrid do not run on the gloo ranks (not available under ``dist``)."""
import asyncio
import json
import os
import socket
import sys

import numpy as np
import pytest

from oracle import search as orc
from tests import fuse_cases, group_cases, lex_cases as lc, mmr_cases, recommend_cases, span_cases
from tests.range_cases import RangeFakeIndex
from tests.test_lexical_host import FakeLex, LexFakeIndex
from tests.test_mmr_host import MmrFakeIndex
from tests.test_spans_host import _fake_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "shard_call_trace.json")
N, DIM, C = 600, 32, "code_chunks"
LOG: list = []
_depth = [0]


def _d(x):
    """A JSON description of one argument: arrays by dtype and shape, filters and scalars by value."""
    if x is None or isinstance(x, (bool, str)):
        return x
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        return float(x)
    if isinstance(x, (set, frozenset)):
        return sorted(_d(v) for v in x)
    if isinstance(x, (list, tuple)):
        return [_d(v) for v in x]
    if isinstance(x, dict):
        return {str(k): _d(v) for k, v in sorted(x.items())}
    return [str(x.dtype).replace("torch.", ""), [int(v) for v in x.shape]]


def _logged(name, fn, skip=()):
    """``fn``, every outermost call logged as ``[name, positional arguments, keyword arguments]`` -- without the stream and the
    output buffers (``out*``), which say where a result goes, not what is asked."""
    def call(*args, **kw):
        if _depth[0] == 0:
            LOG.append([name, [_d(a) for a in args],
                        {k: _d(v) for k, v in sorted(kw.items()) if k != "stream" and not k.startswith("out") and k not in skip}])
        _depth[0] += 1
        try:
            return fn(*args, **kw)
        finally:
            _depth[0] -= 1
    return call


class TraceIndex(LexFakeIndex, MmrFakeIndex, RangeFakeIndex):
    """Every fake of the CPU tier in one index; the calls a ``ShardSet`` makes are logged (not what they call in turn)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        for name in ("search", "search_multi", "search_range", "gather_codes", "gather_vectors", "row_mask"):
            setattr(self, name, _logged(name, getattr(self, name)))


class TraceLex(FakeLex):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.search = _logged("lex.search", self.search, skip=("mask",))
        self.stats = _logged("lex.stats", self.stats)


class TraceDist:
    """``torch.distributed`` with the two tensor collectives of the search path logged."""

    def __init__(self, dist):
        self._dist = dist

    def __getattr__(self, name):
        return getattr(self._dist, name)

    def all_reduce(self, t, op=None, group=None):
        LOG.append(["all_reduce", str(op).split(".")[-1].split(":")[0], _d(t)])
        return self._dist.all_reduce(t, op=op, group=group)

    def all_gather_into_tensor(self, out, t, group=None):
        LOG.append(["all_gather_into_tensor", _d(out), _d(t)])
        return self._dist.all_gather_into_tensor(out, t, group=group)


def _patch(monkeypatch=None):
    ffi = _fake_device(monkeypatch)
    put = (lambda name, val: monkeypatch.setattr(ffi, name, val)) if monkeypatch is not None else (lambda name, val: setattr(ffi, name, val))
    put("Index", TraceIndex)
    put("Lex", TraceLex)
    for name, fn in (("mmr_select", mmr_cases.mmr_select), ("group_select", group_cases.group_select), ("span_select", span_cases.span_select),
                     ("fuse_select", fuse_cases.fuse_select), ("recommend_select", recommend_cases.recommend_select),
                     ("recommend_query", recommend_cases.recommend_query)):
        put(name, _logged(name, fn))


def _corpus():
    rng = np.random.default_rng(600)
    raw = rng.standard_normal((N, DIM)).astype(np.float32)
    raw[300:330] = raw[0:30]                                             # exact copies: ties
    raw[330:360] = raw[30:60] + 1e-3 * rng.standard_normal((30, DIM)).astype(np.float32)
    qs = (raw[[5, 40, 310, 77, 500, 123]] + 0.3 * rng.standard_normal((6, DIM))).astype(np.float32)
    return raw, qs, lc.chunks(N), [f"00000000-0000-4000-8000-{i:012d}" for i in range(N)]


def _bits(v):
    return None if v is None else int(np.float32(v).view(np.uint32))


def _enc(x):
    """Hits as JSON: ids, the f32 bits of every score, the other fields by value (payloads are the ids' own)."""
    if isinstance(x, dict) and "id" in x and "score" in x:
        return {k: (_bits(v) if isinstance(v, float) else _d(v)) for k, v in sorted(x.items()) if k != "payload"}
    if isinstance(x, dict):
        return {k: _enc(v) for k, v in sorted(x.items())}
    if isinstance(x, (list, tuple)):
        return [_enc(v) for v in x]
    return _d(x)


async def _drive(shards: int, lexical: bool, dist: bool = False) -> dict:
    from coderag_amd.store import HipVectorStore
    raw, qs, pay, ids = _corpus()
    out = {}
    kw = {"shards": shards, "_merge_fn": _logged("merge", orc.merge_topk)} if shards > 1 else {}
    async with HipVectorStore(dim=DIM, dtype="f32", initial_capacity=1024, device=0, compact_dead_fraction=0.0, **kw) as s:
        await s.create_collections()
        if dist:
            assert s._shard_backend == "dist"
            for col in s._collections.values():
                col.shards.dist = TraceDist(col.shards.dist)
        for a in range(0, N, 100):                                        # six appends: the blocks go round the shards
            await s.upsert(C, ids[a:a + 100], raw[a:a + 100], pay[a:a + 100])
        assert all(r > 0 for r in s._col(C).shards.rows)

        async def step(name, call, drop=()):
            LOG.clear()
            hits = await call
            out[name] = {"trace": [e for e in LOG if e[0] not in drop], "hits": _enc(hits)}
        go, f12 = {"language": "go"}, {"file_path": ["/proj/f1.py", "/proj/f2.py", "/proj/f7.py"]}
        await step("plain", s.search(C, qs[0].tolist(), limit=7))
        await step("plain_batch", s.search_batch(C, qs[:5], limit=6, filters={"language": "python"}, must_not={"file_path": "/proj/f3.py"}))
        await step("per_query_filters", s.search_batch(C, qs[:4], limit=5, filters=[go, None, {"language": "python"}, f12],
                                                       must_not=[None, {"file_path": "/proj/f3.py"}, None, None]))
        await step("threshold", s.search(C, qs[1].tolist(), limit=5, score_threshold=0.2))
        await step("threshold_counts", s.search_range_batch(C, qs[:3], [0.1, 0.4, -1.0], limit=8, filters=go))
        await step("count_similar", s.count_similar(C, qs[2].tolist(), 0.15))
        await step("diversity", s.search_batch(C, qs[:3], limit=6, diversity=0.5, candidates=24))
        await step("group_by", s.search_batch(C, qs[:3], limit=10, filters={"language": "python"}, group_by="file_path", group_size=1, candidates=12))
        await step("max_overlap", s.search_batch(C, qs[:3], limit=8, max_overlap=0.2))
        await step("fused_rrf_ragged", s.search_fused_batch(C, [qs[0:3], qs[3:4], qs[4:6]], limit=6, filters=go))
        await step("fused_max", s.search_fused(C, qs[1:3], limit=5, fusion="max"))
        sets = [([ids[3], ids[25], ids[310]], [ids[7]]), ([ids[100]], []), ([ids[41], ids[42]], [ids[500], ids[501]])]
        for strategy in ("average", "best"):
            await step(f"recommend_{strategy}", s.recommend_batch(C, sets, limit=6, strategy=strategy, must_not={"file_path": "/proj/f3.py"}),
                       drop=("gather_vectors",))
        await step("recommend_best_round2", s.recommend(C, [ids[3], ids[25]], [ids[7]], limit=8, strategy="best", candidates=8), drop=("gather_vectors",))
        if lexical:
            texts = ["retry_after", "parse request header", "no_such_identifier_anywhere"]
            await step("lexical", s.search_lexical_batch(C, texts, limit=6, filters=go))
            await step("lexical_count", s.lexical_count(C, texts[1]))
            await step("hybrid", s.search_hybrid_batch(C, qs[:3], texts, limit=6, must_not={"file_path": "/proj/f3.py"}))
    return out


def _gloo_worker(rank: int, world: int, port: int, out_dir: str) -> None:
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _patch()
    got = asyncio.run(_drive(world, lexical=False, dist=True))
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(got, f)
    dist.destroy_process_group()


def _gloo(out_dir: str) -> dict:
    import torch.multiprocessing as mp
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    mp.spawn(_gloo_worker, args=(2, port, out_dir), nprocs=2, join=True)
    return {f"rank{r}": json.load(open(os.path.join(out_dir, f"rank{r}.json"))) for r in range(2)}


def _assert_equal(got: dict, want: dict, where: str) -> None:
    got = json.loads(json.dumps(got))
    assert sorted(got) == sorted(want), where
    for name in want:
        assert got[name]["trace"] == want[name]["trace"], f"{where} {name}: the calls differ"
        assert got[name]["hits"] == want[name]["hits"], f"{where} {name}: the hits differ"


@pytest.mark.parametrize("shards", [1, 3])
def test_every_feature_makes_the_recorded_calls_and_returns_the_recorded_hits(monkeypatch, shards):
    _patch(monkeypatch)
    want = json.load(open(GOLDEN))[f"shards{shards}"]
    assert len(want) == 17 and all(v["trace"] for v in want.values())
    _assert_equal(asyncio.run(_drive(shards, lexical=True)), want, f"shards={shards}")


def test_two_gloo_ranks_make_the_recorded_calls_and_collectives(tmp_path):
    want = json.load(open(GOLDEN))["gloo2"]
    assert any(e[0] == "all_reduce" for e in want["rank0"]["diversity"]["trace"])
    for rank, got in _gloo(str(tmp_path)).items():
        _assert_equal(got, want[rank], f"gloo {rank}")


if __name__ == "__main__":
    import tempfile
    with pytest.MonkeyPatch.context() as mp_:
        _patch(mp_)
        golden = {f"shards{ns}": asyncio.run(_drive(ns, lexical=True)) for ns in (1, 3)}
    with tempfile.TemporaryDirectory() as tmp:
        golden["gloo2"] = _gloo(tmp)
    with open(GOLDEN, "w") as f:
        json.dump(golden, f, separators=(",", ":"))
        f.write("\n")
