"""Every encoder GEMM kernel x epilogue x public entry at the tile edges of THAT kernel, the kernel forced rather than left to the
cost model: one fresh child process per kernel (tests/gemm_cases.py's runner under the environment of gemm_cases.ENV -- the
library reads its kernel switches once per process), one after another, never two at once.  The exact cases are compared on
bits, the others against float64 with the bounds derived in tests/gemm_cases.py; tests/test_gemm_cases_host.py proves the
premises on the CPU.  Which kernel a given T reaches on the default path is the cost model's business (choose_gemm) and moves
whenever a kernel gets faster; this file is what pins kernels."""
import json
import os
import subprocess
import sys
import time

import pytest

from tests import gemm_cases as gc
from tests import ln_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 300       # what tests/test_bench_launch.py gives its children: starting Python and torch dominates
CASES = [c for k in gc.KERNELS for c in gc.cases(k)]


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    """kernel -> the child's JSON ({"records": [...], ...}) or {"not_run": reason}.  A child that does not end with exit status 0
    (a signal, an abort, the time limit, an error return from the library) is the last one started: whatever killed it may have
    left the device in a state no further work should be piled on."""
    out, dead = {}, None
    d = tmp_path_factory.mktemp("gemm_matrix")
    for k in gc.KERNELS:
        if dead is not None:
            out[k] = {"not_run": f"not run: an earlier child died ({dead})"}
            continue
        path = str(d / f"{k}.json")
        env = dict(os.environ, **gc.ENV[k])
        t0 = time.time()
        try:
            p = subprocess.run([sys.executable, "-m", "tests.gemm_cases", "--kernel", k, "--out", path], cwd=ROOT, env=env,
                               capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)      # (kills the child at the limit)
        except subprocess.TimeoutExpired:
            dead = f"{k}: no end after {CHILD_TIMEOUT_S} s, killed"
            out[k] = {"not_run": f"the {k} child was killed at its time limit"}
            continue
        if p.returncode != 0:
            dead = f"{k}: exit status {p.returncode}"
            out[k] = {"not_run": f"the {k} child ended with status {p.returncode}: {p.stderr[-1500:]}"}
            continue
        out[k] = json.load(open(path))
        out[k]["by_id"] = {r["id"]: r for r in out[k]["records"]}
        print(f"gemm matrix [{k}]: {len(out[k]['records'])} cases, child wall {time.time() - t0:.1f} s, "
              f"library calls (synchronised) {out[k]['gpu_call_s']:.3f} s")
    return out


def _record(runs, kernel, cid):
    assert "not_run" not in runs[kernel], runs[kernel]["not_run"]
    assert cid in runs[kernel]["by_id"], f"the {kernel} child wrote no record for {cid}"
    return runs[kernel]["by_id"][cid]


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case(runs, case):
    """Exact cases: no bf16 word differs from bf16_rne(float64 result).  GELU cases: within one bf16 rounding + gelu_erf2's own
    4e-6 (1 + |x|) of float64 erf-GELU at the exact pre-activation.  LayerNorm cases: within one bf16 rounding + the derived f32
    term of the float64 LayerNorm of the exactly known rows (gemm_cases.layernorm64 / ln_apply64); the f32 residual that
    ..._res32_ln writes back within the f32 term alone.  Epilogue 5's statistics: rtol 2e-5 (nmr: + 2e-6) of the float64 statistics of
    the rows as stored.  crh_layernorm_apply in place gives the bits it gives out of place.  Guard rows around every written
    buffer keep their sentinel.
    The hard LayerNorm rows of tests/ln_cases.py (hard_*: tiny variance, large offsets, outliers, eps = 1e-12) reach every site
    through identity weights and are read the same way: the standalone kernels and k_embed_ln against layernorm64's bound, epilogue
    5's stored rows on bits and its stats_out against ln_cases.stats_bound, crh_layernorm_apply and epilogue 3 fed with the
    device's own stats_out against ln_cases.dev_stats_tolerance; the embedding records count wrong mask words in diff_words."""
    r = _record(runs, case.kernel, case.id)
    assert r["guards_ok"], r
    if case.variant == "ln_apply":
        assert r["excess"] <= 0 and r["diff_words"] == 0, r
        return
    if case.variant in ln_cases.NO_GEMM_VARIANTS:
        assert (r["T"], r["variant"]) == (case.T, case.variant) and r["excess"] is not None and r["excess"] <= 0, r
        assert r["diff_words"] == 0 if "embed" in case.variant else r["diff_words"] is None, r
        return
    assert (r["kernel"], r["T"], r["N"], r["K"], r["variant"]) == (case.kernel, case.T, case.N, case.K, case.variant)
    if gc.VARIANTS[case.variant][2] == "exact":
        assert r["diff_words"] == 0, r
    else:
        assert r["excess"] is not None and r["excess"] <= 0, r
    if case.variant in ("res_raw", "res_norm") + ln_cases.STATS_VARIANTS:
        assert r["stats_excess"] is not None and r["stats_excess"] <= 0, r
    if case.variant in ("bias_res32_ln", "hard_bias_res32_ln", "hard_bias_res32_ln_e12"):
        assert r["aux_excess"] is not None and r["aux_excess"] <= 0, r


def test_the_three_kernels_agree_to_the_bit(runs):
    """k_gemm_mid, k_gemm_nt and the ping-pong kernel add the same products in the same order (one 16x16x32 MFMA chain along K per
    output block) and build epilogue 5's statistics from the same per-lane sums joined the same way: for every (variant, shape)
    that more than one kernel's list holds -- the product's four GEMMs at T = 300 in all three, (3841, 768, 256) and
    (4100, 2304, 256) in k_gemm_nt's and the ping-pong kernel's, (1, 128, 64) in k_gemm_nt's and k_gemm_mid's -- the outputs of
    epilogues 0, 2, 3 and 5 are the same bytes, and so are epilogue 5's stats_out."""
    seen = {}
    for k in gc.KERNELS:
        for c in gc.cases(k):
            if c.variant in gc.AGREE_VARIANTS:
                seen.setdefault((c.variant, c.T, c.N, c.K), []).append(c)
    shared = {key: cs for key, cs in seen.items() if len(cs) > 1}
    assert sum(len(cs) == 3 for cs in shared.values()) == 7 + 2 + 2 + 6 and len(shared) >= 17 + 6 + 2 + 2 and {gc.VARIANTS[v][1] for (v, _, _, _) in shared} == {0, 2, 3, 5}
    for key, cs in sorted(shared.items()):
        recs = [_record(runs, c.kernel, c.id) for c in cs]
        assert len({r["sha_out"] for r in recs}) == 1, (key, [(r["kernel"], r["sha_out"][:12]) for r in recs])
        if key[0] in ("res_raw", "res_norm"):
            assert recs[0]["sha_stats"] and len({r["sha_stats"] for r in recs}) == 1, (key, [(r["kernel"], r["sha_stats"][:12]) for r in recs])


def test_the_three_kernels_agree_to_the_bit_on_the_hard_layernorm_rows(runs):
    """What the comment above struct LnAcc promises, where it is hardest to keep: on rows of tiny variance, large offset and single
    outliers every kernel stores the same bytes and builds the same stats_out -- and so does everything computed from them (the
    LayerNorm kernels after the GEMM, epilogue 3 fed with those statistics)."""
    seen = {}
    for k in gc.KERNELS:
        for c in ln_cases.cases(k):
            if c.variant in ln_cases.AGREE:
                seen.setdefault((c.variant, c.T, c.K), []).append(c)
    assert {v for (v, _, _) in seen} == set(ln_cases.AGREE) and all(len(cs) == len(gc.KERNELS) for cs in seen.values())
    for key, cs in sorted(seen.items()):
        recs = [_record(runs, c.kernel, c.id) for c in cs]
        assert len({r["sha_out"] for r in recs}) == 1, (key, [(r["kernel"], r["sha_out"][:12]) for r in recs])
        if key[0] in ln_cases.STATS_VARIANTS:
            assert recs[0]["sha_stats"] and len({r["sha_stats"] for r in recs}) == 1, (key, [(r["kernel"], r["sha_stats"][:12]) for r in recs])


def test_the_hard_row_records_are_the_ones_design_md_tabulates(runs):
    """DESIGN.md's second coverage table (the hard LayerNorm rows) against what the children ran."""
    records = [r for k in gc.KERNELS for r in _record_list(runs, k)]
    table = gc.coverage_table(records, hard=True)
    assert table == gc.coverage_table(CASES, hard=True) and table in open(os.path.join(ROOT, "DESIGN.md")).read()
    for k in gc.KERNELS:        # every tiled kernel ran every site that goes through one
        assert {e for (kk, e, _) in gc.coverage(records, hard=True) if kk == k} == {0, 2, 3, 5}


def _record_list(runs, kernel):
    assert "not_run" not in runs[kernel], runs[kernel]["not_run"]
    return runs[kernel]["records"]


def test_the_records_cover_every_kernel_epilogue_pair_as_design_md_says(runs):
    """The children wrote one record per case of the lists, so the coverage DESIGN.md tabulates (checked against the lists by
    tests/test_gemm_cases_host.py) is what ran: every kernel x epilogue with a ragged-T and a multi-tile record."""
    records = []
    for k in gc.KERNELS:
        assert "not_run" not in runs[k], runs[k]["not_run"]
        assert runs[k]["error"] is None and sorted(runs[k]["by_id"]) == sorted(c.id for c in gc.cases(k))
        records += runs[k]["records"]
    assert gc.coverage_table(records) == gc.coverage_table(CASES)
    assert gc.coverage_table(records) in open(os.path.join(ROOT, "DESIGN.md")).read()
    for k in gc.KERNELS:
        for epi in range(6):
            mine = [r for r in records if r["kernel"] == k and r["epilogue"] == epi]
            assert any(r["ragged"] for r in mine) and any(r["multi_tile"] for r in mine), (k, epi)
