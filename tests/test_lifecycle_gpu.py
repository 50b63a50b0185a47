"""The life-cycle script of tests/lifecycle_cases.py on the HIP index: every public read path after every phase (warm) or only
late (cold), compared exactly with the model -- ids as lists, scores as f32 bit patterns, the re-rank's f64 scores as they are."""
import asyncio
import time

import pytest

pytestmark = pytest.mark.gpu

BLOCK = 32
CASES = [("bf16", 1, "warm", False), ("f32", 1, "warm", False), ("bf16", 1, "cold", False), ("f32", 2, "warm", False), ("bf16", 1, "warm", True)]


@pytest.mark.parametrize("dtype,shards,schedule,int8", CASES, ids=[f"{d}-{n}shard-{s}{'-int8' if i else ''}" for d, n, s, i in CASES])
def test_every_read_path_equals_the_model_through_the_life_cycle(gpu, monkeypatch, dtype, shards, schedule, int8):
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi, shards as shards_mod
    from coderag_amd.ranking.device import DeviceReranker
    from coderag_amd.store import HipVectorStore
    from tests import lifecycle_cases as lc
    # crh_index_create reads the variable once, when an index is made: set before the first store exists.  tests/conftest.py
    # switches the int8 nomination on for every index; here one case runs with it and the others with the product's default
    # (these indexes are far below the default's million rows: the bf16 / f32 tiles nominate)
    if int8:
        monkeypatch.setenv("CODERAG_HIP_I8_MIN_ROWS", "1")
    else:
        monkeypatch.delenv("CODERAG_HIP_I8_MIN_ROWS", raising=False)
    orig = shards_mod.ShardSet.__init__

    def small_blocks(self, *a, **kw):
        kw["block"] = BLOCK
        orig(self, *a, **kw)
    monkeypatch.setattr(shards_mod.ShardSet, "__init__", small_blocks)
    stores = []

    def make_store():
        stores.append(HipVectorStore(dim=lc.DIM, dtype=dtype, initial_capacity=64, device=0, shards=shards, **lc.AUTO_COMPACT))
        return stores[-1]
    sc = lc.Script(make_store, shards, BLOCK, schedule, lc.FULL, dtype == "bf16", cuda=True, reranker=DeviceReranker(device=0))
    nominations = []

    def hook(phase, script):
        if phase == 7:
            nominations.extend(ix.nomination() for ix in script.store._col(lc.CODE).shards.index.values())
    sc.hook = hook
    t0 = time.perf_counter()
    asyncio.run(sc.run())
    print(f"life cycle {dtype} x {shards} {schedule}{' int8' if int8 else ''}: {sc.checked} check_all rounds, {len(sc.compared)} comparisons, {time.perf_counter() - t0:.2f} s")
    assert sc.checked == (16 if schedule == "warm" else 6) and len(stores) == 2 and len(sc.compared) == lc.checks_in(lc.FULL) * sc.checked > 40 * sc.checked
    assert [e[0] for e in sc.model.log if e[1]] == list(lc.AUTO_CALLS)
    assert nominations and all((n == ffi.NOMINATE_INT8) == int8 for n in nominations), nominations
