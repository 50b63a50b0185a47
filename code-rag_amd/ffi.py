"""ctypes binding of ``libcoderag_hip.so`` (declared in ``include/coderag_hip.h``).

This is the only module that touches the native library.  There is no fallback:
if the shared object is missing or a call fails, a :class:`NativeError` is raised.
"""

from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("CODERAG_HIP_LIB", PKG_DIR / "lib" / "libcoderag_hip.so"))

OK, E_INVALID, E_HIP, E_CAPACITY, E_NODEVICE, E_INTERNAL = 0, -1, -2, -3, -4, -5
DTYPE_F32, DTYPE_BF16 = 0, 1
NOMINATE_BF16_3, NOMINATE_BF16, NOMINATE_INT8 = 0, 1, 2
MAX_FILTERS, MAX_K = 8, 1024
MAX_LISTS = 16         # CRH_MAX_LISTS: candidate lists one crh_fuse_select call fuses per logical query
FUSE_RRF, FUSE_MAX = 0, 1
FUSE_METHODS = {"rrf": FUSE_RRF, "max": FUSE_MAX}
MAX_POS, MAX_NEG = 8, 8   # CRH_MAX_POS / CRH_MAX_NEG: live examples of one recommend query (crh_recommend_*)
RECOMMEND_AVERAGE, RECOMMEND_BEST = 0, 1
RECOMMEND_STRATEGIES = {"average": RECOMMEND_AVERAGE, "best": RECOMMEND_BEST}
COND_IN, COND_NOT_IN, COND_BETWEEN, COND_NOT_BETWEEN = 0, 1, 2, 3   # CRH_COND_*: the modes of crh_condition.negate
COND_WORDS, COND_NOT_WORDS = 4, 5   # a row bitmap in device memory (RowWords) instead of a column
RANGE_MODES = {"between": COND_BETWEEN, "not_between": COND_NOT_BETWEEN}
VALUE_MAX = 2 ** 31 - 1   # largest value a numeric column stores (int32); -1 stands for "absent"
MAX_CLASSES = 8        # CRH_MAX_CLASSES: distinct filters that share one pass of crh_search_multi
ABI_VERSION = 4        # CRH_ABI_VERSION of include/coderag_hip.h
LEX_MAX_QUERY_TERMS = 32   # CRH_LEX_MAX_QUERY_TERMS: distinct term ids of one crh_lex_search query
TEXT_MAX_PATTERNS, TEXT_MAX_PATTERN_BYTES = 8, 64   # CRH_TEXT_MAX_PATTERNS / CRH_TEXT_MAX_PATTERN_BYTES of one crh_text_match
REGEX_MAX_STATES, REGEX_MAX_TABLE_BYTES = 256, 32768   # CRH_REGEX_MAX_STATES / CRH_REGEX_MAX_TABLE_BYTES of one crh_text_regex
FUZZY_MAX_EDITS = 3    # CRH_FUZZY_MAX_EDITS: byte edits one crh_text_fuzzy allows at most
TEXT_ALL, TEXT_ANY = 0, 1   # CRH_TEXT_ALL / CRH_TEXT_ANY
FACET_LDS_BINS = 8192       # CRH_FACET_LDS_BINS: up to this many bins crh_index_facet counts in LDS, above it by runs of equal codes
GRAPH_MAX_RELATIONS, GRAPH_MAX_QUERIES, GRAPH_MAX_HOPS = 8, 64, 16   # CRH_GRAPH_MAX_RELATIONS / _MAX_QUERIES / _MAX_HOPS
GRAPH_WAVE_DEGREE = 64      # CRH_GRAPH_WAVE_DEGREE: adjacency lists of at least so many entries are walked by a whole wave
GRAPH_ALONG, GRAPH_AGAINST, GRAPH_BOTH = 0, 1, 2   # CRH_GRAPH_*: the direction of travel
GRAPH_DIRECTIONS = {"callees": GRAPH_ALONG, "callers": GRAPH_AGAINST, "both": GRAPH_BOTH}
GRAPH_SCC_WORK_EXTRA = 32   # CRH_GRAPH_SCC_WORK_EXTRA: int32 words of crh_graph_scc's work array beyond one per node
GRAPH_WORDS = {"in_cycle": 0, "same_component": 1, "range": 2}    # CRH_GRAPH_WORDS_*: the conditions of crh_graph_node_words
GRAPH_PPR_MAX_STEPS = 64    # CRH_GRAPH_PPR_MAX_STEPS: steps of one crh_graph_ppr
GRAPH_MAX_CHAINS = 64       # CRH_GRAPH_MAX_CHAINS: chains per query of one crh_graph_chains
GRAPH_SATURATED = 2 ** 64 - 1   # a chain count of crh_graph_sigma that means "at least that many"
GRAPH_BETWEEN = {"any": 0, "shortest": 1}   # CRH_GRAPH_BETWEEN_*: the modes of crh_graph_between
FACET_MAX_ENTRIES = 2 ** 26  # bin entries (queries x bins) one semantic facet call may ask of a shard set: 512 MB of int64 per slab

# every symbol include/coderag_hip.h declares (tests check the library exports all of them)
EXPORTS = (
    "crh_abi_version", "crh_last_error", "crh_device_count", "crh_device_info",
    "crh_index_create", "crh_index_destroy", "crh_index_append", "crh_index_append_preprocessed", "crh_index_tombstone",
    "crh_index_tombstone_filter", "crh_index_compact", "crh_index_export", "crh_index_import",
    "crh_index_count", "crh_index_clear", "crh_index_reserve", "crh_index_read_rows",
    "crh_search", "crh_search_finish", "crh_search_get_stats", "crh_index_set_tuning",
    "crh_index_set_nomination", "crh_index_get_nomination",
    "crh_merge_topk", "crh_merge_topk_strided", "crh_index_match_rows", "crh_index_set_profiling", "crh_index_get_profile",
    "crh_search_cond", "crh_index_match_rows_cond", "crh_index_tombstone_cond", "crh_index_set_sparse_route",
    "crh_gemm_bf16_bias", "crh_gemm_bf16_bias_res_ln", "crh_gemm_bf16_res_lnstats", "crh_gemm_bf16_lnin", "crh_layernorm_apply", "crh_gemm_bf16_bias_res32_ln", "crh_attn_fwd_varlen", "crh_embed_ln",
    "crh_masked_mean_pool", "crh_gather_rows_i32", "crh_gather_rows_bytes", "crh_gather_rerank_columns", "crh_rerank_vector",
    "crh_embed_ln_packed", "crh_attn_fwd_packed", "crh_masked_mean_pool_packed", "crh_encoder_finish",
    "crh_index_gather_vectors", "crh_mmr_select",
    "crh_index_gather_codes", "crh_group_select",
    "crh_search_multi",
    "crh_fuse_select",
    "crh_recommend_query", "crh_recommend_select",
    "crh_search_range",
    "crh_span_select",
    "crh_index_row_mask", "crh_lex_create", "crh_lex_destroy", "crh_lex_clear", "crh_lex_count", "crh_lex_append", "crh_lex_stats",
    "crh_lex_search",
    "crh_text_create", "crh_text_destroy", "crh_text_clear", "crh_text_count", "crh_text_append", "crh_text_match", "crh_text_regex",
    "crh_text_fuzzy",
    "crh_index_facet", "crh_search_range_facet", "crh_facet_select",
    "crh_graph_create", "crh_graph_destroy", "crh_graph_count", "crh_graph_set_relation", "crh_graph_bfs", "crh_graph_list",
    "crh_graph_row_words", "crh_graph_path",
    "crh_graph_node_rows", "crh_graph_candidates", "crh_rerank_hybrid",
    "crh_graph_ppr", "crh_graph_ppr_bins", "crh_graph_ppr_order",
    "crh_graph_scc", "crh_graph_scc_bins", "crh_graph_layers", "crh_graph_node_words",
    "crh_graph_sigma", "crh_graph_chains", "crh_graph_between", "crh_graph_bfs_avoiding",
)
# exported by lib/libcoderag_hip_debug.so only (same sources built with -DCRH_ENABLE_DEBUG; tools/ and kernel tests)
DEBUG_EXPORTS = ("crh_debug_gemm_variant", "crh_debug_read_ceiling", "crh_debug_i8_move", "crh_debug_i8_intervals",
                 "crh_debug_kth_largest", "crh_debug_select_tail", "crh_debug_tile_list")
DEBUG_LIB_PATH = Path(os.environ.get("CODERAG_HIP_DEBUG_LIB", PKG_DIR / "lib" / "libcoderag_hip_debug.so"))

RR_NAME_BYTES, RR_MAX_ENTITIES, RR_ENTITY_BYTES = 64, 8, 48
RR_MAX_HYBRID, RR_HYBRID_SIGNALS, RR_HYBRID_TABLE = 512, 7, 128   # CRH_RR_MAX_HYBRID / _HYBRID_SIGNALS / _HYBRID_TABLE
ROLE_PRIMARY, ROLE_CALLER, ROLE_CALLEE, ROLE_METHOD, ROLE_PARENT, ROLE_CHILD = range(6)   # CRH_ROLE_*
GRAPH_CAND_MAX_QUERIES = 1024   # CRH_GRAPH_CAND_MAX_QUERIES


class NativeError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"libcoderag_hip error {code}: {message}")
        self.code = code


class Filter(C.Structure):
    _fields_ = [("col", C.c_int32), ("code", C.c_int32)]


class Condition(C.Structure):
    """``crh_condition``: column ``col`` is (``negate`` = 0) / is not (1) one of the ``n`` int32 codes at ``codes``; ``negate`` =
    ``COND_BETWEEN`` / ``COND_NOT_BETWEEN``: the column's value lies / does not lie in ``codes[0] .. codes[1]`` (``n`` = 2)."""
    _fields_ = [("col", C.c_int32), ("negate", C.c_int32), ("n", C.c_int64), ("codes", C.c_void_p)]


class RerankQuery(C.Structure):
    """``crh_rerank_query``: one query's weights and lower-cased entity names."""
    _fields_ = [("vector_weight", C.c_double), ("centrality_weight", C.c_double), ("n_entities", C.c_int32),
                ("entity_len", C.c_int32 * 8), ("entity", (C.c_uint8 * 48) * 8), ("pad_", C.c_int32)]


class RerankHybridQuery(C.Structure):
    """``crh_rerank_hybrid_query``: ``crh_rerank_query`` + the graph branch's weights."""
    _fields_ = [("base", RerankQuery), ("graph_weight", C.c_double), ("context_weight", C.c_double), ("relationship_bonus", C.c_double)]


class GraphSegment(C.Structure):
    """``crh_graph_segment``: an explicit node, or the first ``take`` entries of a list row, in one role of one query."""
    _fields_ = [(n, C.c_int32) for n in ("query", "role", "node", "list_row", "take", "pad_")]


class RerankColumns(C.Structure):
    """``crh_rerank_columns``: device pointers of the gathered per-candidate side data."""
    _fields_ = [(n, C.c_void_p) for n in ("content_len", "degree", "file_code", "key_code", "node_code", "name_len", "name")]


class SearchStats(C.Structure):
    _fields_ = [("rows", C.c_int64), ("tiles", C.c_int64), ("seed_tiles", C.c_int64),
                ("candidates", C.c_int64), ("max_query_cands", C.c_int64),
                ("fallback_used", C.c_int32), ("batches", C.c_int32)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


_lib = None
_debug_lib = None


def _preload_hip_runtime() -> None:
    """libcoderag_hip.so is not linked against a HIP runtime (code-rag_amd/build.sh): it binds to the one already
    in the process.  PyTorch ships its own libamdhip64/libhsa-runtime64; loading a second copy beside it breaks
    device discovery and makes streams / RCCL unshareable, so torch's copy goes in first, globally."""
    candidates = []
    try:
        import torch  # noqa: F401  (plumbing: device memory, streams, torch.distributed)
        candidates.append(Path(torch.__file__).resolve().parent / "lib" / "libamdhip64.so")
    except Exception:  # torch absent: a plain ROCm install is fine for C-ABI-only use
        pass
    candidates += [Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "lib" / "libamdhip64.so"]
    for cand in candidates:
        if cand.exists():
            C.CDLL(str(cand), mode=C.RTLD_GLOBAL)
            return
    raise NativeError(E_NODEVICE, "no libamdhip64.so found (neither PyTorch-ROCm nor $ROCM_PATH/lib)")


def lib() -> C.CDLL:
    """Load the native library once; raise loudly when it has not been built."""
    global _lib
    if _lib is None:
        _lib = _bind(LIB_PATH, debug=False)
    return _lib


def debug_lib() -> C.CDLL:
    """``libcoderag_hip_debug.so``: the product's sources + the ``crh_debug_*`` entry points.  For tools/ and kernel tests
    only -- nothing in the package calls this.  It is a separate library instance (its own handles and error slot)."""
    global _debug_lib
    if _debug_lib is None:
        _debug_lib = _bind(DEBUG_LIB_PATH, debug=True)
    return _debug_lib


def _bind(path: Path, debug: bool) -> C.CDLL:
    if not path.exists():
        raise NativeError(E_INTERNAL, f"{path} is missing -- build it with "
                          "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc)")
    _preload_hip_runtime()
    L = C.CDLL(str(path))
    vp, i32, i64, f32p = C.c_void_p, C.c_int, C.c_int64, C.c_void_p
    L.crh_abi_version.restype = i32
    L.crh_last_error.restype = C.c_char_p
    L.crh_device_count.argtypes = [C.POINTER(i32)]
    L.crh_device_info.argtypes = [i32, C.c_char_p, i32, C.c_char_p, i32, C.POINTER(i64), C.POINTER(i32)]
    L.crh_index_create.argtypes = [i32, i32, i64, i32, i32, C.POINTER(vp)]
    L.crh_index_destroy.argtypes = [vp]
    L.crh_index_append.argtypes = [vp, i64, f32p, i32, vp, C.POINTER(i64), vp]
    L.crh_index_append_preprocessed.argtypes = [vp, i64, f32p, i32, vp, C.POINTER(i64), vp]
    L.crh_index_tombstone.argtypes = [vp, i64, vp]
    L.crh_index_tombstone_filter.argtypes = [vp, C.POINTER(Filter), i32, C.POINTER(i64)]
    L.crh_index_compact.argtypes = [vp, vp, C.POINTER(i64)]
    L.crh_index_export.argtypes = [vp, i64, i64, vp, vp, vp, vp]
    L.crh_index_import.argtypes = [vp, i64, i64, i64, vp, vp, vp, vp]
    L.crh_index_count.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.crh_index_clear.argtypes = [vp]
    L.crh_index_reserve.argtypes = [vp, i64]
    L.crh_index_read_rows.argtypes = [vp, i64, i64, vp]
    L.crh_search.argtypes = [vp, i32, vp, i32, i32, C.POINTER(Filter), i32, i64, vp, vp, i32, vp]
    L.crh_search_finish.argtypes = [vp, vp]
    L.crh_search_get_stats.argtypes = [vp, C.POINTER(SearchStats)]
    L.crh_index_set_tuning.argtypes = [vp, i32, i32, i32, i32]
    L.crh_index_set_nomination.argtypes = [vp, i32]
    L.crh_index_get_nomination.argtypes = [vp, C.POINTER(i32)]
    L.crh_index_set_profiling.argtypes = [vp, i32]
    L.crh_index_get_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(i64)]
    L.crh_merge_topk.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp]
    L.crh_merge_topk_strided.argtypes = [i32, i32, i32, vp, vp, i64, i64, vp, vp, vp]
    L.crh_index_match_rows.argtypes = [vp, C.POINTER(Filter), i32, i64, vp, C.POINTER(i64)]
    L.crh_search_cond.argtypes = [vp, i32, vp, i32, i32, C.POINTER(Condition), i32, i64, vp, vp, i32, vp]
    L.crh_search_multi.argtypes = [vp, i32, vp, i32, i32, C.POINTER(Condition), vp, i32, vp, i64, vp, vp, i32, vp]
    L.crh_search_range.argtypes = [vp, i32, vp, i32, i32, vp, C.POINTER(Condition), i32, i64, vp, vp, vp, i32, vp]
    L.crh_index_match_rows_cond.argtypes = [vp, C.POINTER(Condition), i32, i64, vp, C.POINTER(i64)]
    L.crh_index_tombstone_cond.argtypes = [vp, C.POINTER(Condition), i32, C.POINTER(i64)]
    L.crh_index_set_sparse_route.argtypes = [vp, i32, i32]
    L.crh_gemm_bf16_bias.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp]
    L.crh_gemm_bf16_bias_res_ln.argtypes = [vp, vp, vp, vp, vp, vp, C.c_float, vp, i32, i32, i32, vp]
    L.crh_gemm_bf16_res_lnstats.argtypes = [vp, vp, vp, vp, vp, vp, C.c_float, vp, vp, vp, i32, i32, i32, vp]
    L.crh_gemm_bf16_lnin.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    L.crh_layernorm_apply.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp]
    L.crh_gemm_bf16_bias_res32_ln.argtypes = [vp, vp, vp, vp, vp, vp, C.c_float, vp, i32, i32, i32, vp]
    L.crh_attn_fwd_varlen.argtypes = [vp, vp, vp, i32, i32, i32, vp]
    L.crh_embed_ln.argtypes = [vp, vp, vp, vp, vp, vp, C.c_float, i32, vp, vp, i32, i32, i32, vp]
    L.crh_masked_mean_pool.argtypes = [vp, vp, vp, i32, i32, i32, vp]
    L.crh_embed_ln_packed.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_float, i32, vp, vp, i32, i32, i32, i32, vp]
    L.crh_attn_fwd_packed.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp]
    L.crh_masked_mean_pool_packed.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp]
    L.crh_encoder_finish.argtypes = [vp]
    L.crh_gather_rows_i32.argtypes = [i64, vp, i64, i64, vp, i32, vp, vp]
    L.crh_gather_rows_bytes.argtypes = [i64, vp, i64, i64, vp, i32, vp, vp]
    L.crh_gather_rerank_columns.argtypes = [i64, vp, i64, i64, vp, vp, vp]
    L.crh_rerank_vector.argtypes = [i32, i32, vp, vp, C.POINTER(RerankColumns), vp, C.c_double, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    L.crh_index_gather_vectors.argtypes = [vp, i64, vp, i64, vp, vp]
    L.crh_mmr_select.argtypes = [i32, i32, i32, i32, vp, vp, vp, C.c_float, vp, vp, vp, vp, vp]
    L.crh_index_gather_codes.argtypes = [vp, i32, i64, vp, i64, vp, vp]
    L.crh_group_select.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.crh_span_select.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.crh_fuse_select.argtypes = [i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.crh_recommend_query.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp]
    L.crh_recommend_select.argtypes = [i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.crh_index_row_mask.argtypes = [vp, C.POINTER(Condition), i32, vp, i64, vp]
    L.crh_lex_create.argtypes = [i32, i64, C.POINTER(vp)]
    L.crh_lex_destroy.argtypes = [vp]
    L.crh_lex_clear.argtypes = [vp]
    L.crh_lex_count.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.crh_lex_append.argtypes = [vp, i64, vp, vp, vp, vp]
    L.crh_lex_stats.argtypes = [vp, vp, i64, vp, vp, C.POINTER(i64), C.POINTER(i64)]
    L.crh_lex_search.argtypes = [vp, i32, vp, vp, vp, C.c_float, C.c_float, C.c_float, i32, vp, i64, vp, vp, vp, vp]
    L.crh_text_create.argtypes = [i32, i64, i64, C.POINTER(vp)]
    L.crh_text_destroy.argtypes = [vp]
    L.crh_text_clear.argtypes = [vp]
    L.crh_text_count.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.crh_text_append.argtypes = [vp, i64, vp, vp]
    L.crh_text_match.argtypes = [vp, i32, vp, vp, i32, i32, vp, vp, C.POINTER(i64), vp]
    L.crh_text_regex.argtypes = [vp, i32, i32, vp, i32, vp, i32, vp, vp, C.POINTER(i64), vp]
    L.crh_text_fuzzy.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp]
    L.crh_index_facet.argtypes = [vp, i32, C.POINTER(Condition), i32, i32, vp, vp, vp]
    L.crh_search_range_facet.argtypes = [vp, i32, vp, i32, vp, C.POINTER(Condition), i32, i32, i32, vp, vp, vp]
    L.crh_facet_select.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp]
    L.crh_graph_create.argtypes = [i32, i64, C.POINTER(vp)]
    L.crh_graph_destroy.argtypes = [vp]
    L.crh_graph_count.argtypes = [vp, i32, C.POINTER(i64), C.POINTER(i64)]
    L.crh_graph_set_relation.argtypes = [vp, i32, i64, vp, vp, vp, vp]
    L.crh_graph_bfs.argtypes = [vp, i32, i32, i32, vp, vp, i32, i32, i32, vp, vp, vp, vp]
    L.crh_graph_list.argtypes = [vp, i32, vp, i32, i32, i32, vp, vp, vp, vp]
    L.crh_graph_row_words.argtypes = [vp, i64, vp, i64, i32, vp, i64, vp]
    L.crh_graph_path.argtypes = [vp, i32, i32, vp, i32, i64, i32, vp, C.POINTER(i32), vp]
    L.crh_graph_node_rows.argtypes = [i64, vp, vp, i64, i64, vp, vp]
    L.crh_graph_ppr.argtypes = [vp, i32, i32, i32, i32, vp, vp, i32, C.c_float, i32, vp, vp, vp]
    L.crh_graph_ppr_bins.argtypes = [i64, i32, vp, i32, vp, vp, vp]
    L.crh_graph_ppr_order.argtypes = [i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.crh_graph_scc.argtypes = [vp, i32, vp, vp, vp, vp]
    L.crh_graph_scc_bins.argtypes = [i64, vp, vp, i64, vp, vp]
    L.crh_graph_layers.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp]
    L.crh_graph_node_words.argtypes = [i64, i32, vp, vp, i64, i64, i32, vp, vp]
    L.crh_graph_sigma.argtypes = [vp, i32, i32, i32, vp, vp, i32, vp, vp]
    L.crh_graph_chains.argtypes = [vp, i32, i32, i32, vp, vp, i32, vp, i32, i32, vp, vp, vp, vp]
    L.crh_graph_between.argtypes = [i64, i32, vp, vp, i32, i32, vp, vp, vp, vp]
    L.crh_graph_bfs_avoiding.argtypes = [vp, i32, i32, i32, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]
    L.crh_graph_candidates.argtypes = [i32, i32, i32, vp, vp, vp, i32, i32, vp, i64, vp, vp, vp, vp, vp, vp, vp]
    L.crh_rerank_hybrid.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_double, i32, i32, i32, i32, i32,
                                    vp, vp, vp, vp, vp, vp, vp]
    if debug or hasattr(L, "crh_debug_gemm_variant"):   # (CODERAG_HIP_LIB may point a tool's whole run at the debug build)
        debug = True
        L.crh_debug_gemm_variant.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp]
        L.crh_debug_read_ceiling.argtypes = [vp, vp]
        L.crh_debug_i8_move.argtypes = [vp]
        L.crh_debug_i8_intervals.argtypes = [vp, i32, vp, i32, C.POINTER(Filter), i32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.crh_debug_kth_largest.argtypes = [i32, vp, C.c_uint, C.c_uint, vp, C.c_uint, C.c_uint, vp]
        L.crh_debug_select_tail.argtypes = [i32, vp, C.c_uint, i32, i64, vp, vp]
        L.crh_debug_tile_list.argtypes = [vp, i64, vp, vp]
    for name in EXPORTS + (DEBUG_EXPORTS if debug else ()):
        if name != "crh_last_error":
            getattr(L, name).restype = i32
    if L.crh_abi_version() != ABI_VERSION:
        raise NativeError(E_INTERNAL, f"ABI version mismatch between ffi.py and {path.name}")
    return L


def check(rc: int, L: C.CDLL | None = None) -> None:
    if rc != OK:
        raise NativeError(rc, ((L or lib()).crh_last_error() or b"").decode("utf-8", "replace"))


def use_device(device: int) -> None:
    """Make ``device`` the calling thread's current HIP device.  The stateless entry points (GEMMs, attention, merge, gather,
    re-rank) launch on the CURRENT device, and a worker thread (the provider's and the store's executors) starts on device 0
    whatever the thread that created the tensors had selected."""
    import torch
    if torch.cuda.is_available() and torch.cuda.current_device() != int(device):   # (no device: the native call that follows reports it)
        torch.cuda.set_device(int(device))


def current_stream(device) -> int:
    """torch's current stream on ``device`` as a raw hipStream_t."""
    import torch
    return int(torch.cuda.current_stream(device).cuda_stream)


def device_count() -> int:
    n = C.c_int(0)
    rc = lib().crh_device_count(C.byref(n))
    return int(n.value) if rc == OK else 0


def device_info(device: int = 0) -> dict:
    name, arch = C.create_string_buffer(256), C.create_string_buffer(256)
    hbm, cus = C.c_int64(0), C.c_int(0)
    check(lib().crh_device_info(device, name, 256, arch, 256, C.byref(hbm), C.byref(cus)))
    return {"name": name.value.decode(), "arch": arch.value.decode(), "hbm_bytes": int(hbm.value),
            "cu_count": int(cus.value)}


def _filters(filters) -> tuple:
    filters = list(filters or [])
    if len(filters) > MAX_FILTERS:
        raise NativeError(E_INVALID, f"at most {MAX_FILTERS} filters are supported")
    arr = (Filter * max(1, len(filters)))()
    for i, (col, code) in enumerate(filters):
        arr[i].col, arr[i].code = int(col), int(code)
    return arr, len(filters)


class RowWords:
    """A ROW-BITMAP condition (``CRH_COND_WORDS`` / ``CRH_COND_NOT_WORDS``): the row passes iff its bit is set (``negate``: clear)
    in validity words somebody else computed (:meth:`Text.match`).  ``words`` maps ``id(index)`` to that index's int32 device
    tensor of at least ``ceil(rows / 32)`` words -- one filter serves every shard of a collection, each :class:`Index` takes
    its own words -- or is ONE tensor for whichever index is asked.  The library cannot look into the buffer: conditions are
    equal iff pointer, length, mode and ``tag`` are, so whoever rewrites a buffer takes a new tag (:func:`next_words_tag`).
    Travels with the set conditions (``crh_condition``); ``len()`` is 5, unlike every tuple form."""
    __slots__ = ("tag", "words", "negate")

    def __init__(self, tag: int, words, negate: bool = False):
        self.tag, self.words, self.negate = int(tag), words, bool(negate)

    def __len__(self) -> int:
        return 5

    def words_of(self, owner):
        w = self.words.get(id(owner)) if isinstance(self.words, dict) else self.words
        if w is None:
            raise NativeError(E_INVALID, "row-bitmap condition: no words for this index")
        _typed(w, "int32", "row bitmap")
        if not _is_dev(w):
            raise NativeError(E_INVALID, "row-bitmap condition: the words must be a device tensor")
        return w


_words_tag = 0


def next_words_tag() -> int:
    """A tag no earlier :class:`RowWords` of this process carries (positive, wraps far beyond any cache's memory)."""
    global _words_tag
    _words_tag = _words_tag % (2 ** 31 - 2) + 1
    return _words_tag


def is_set_condition(item) -> bool:
    """A filter item is ``(column, code)`` -- the equality of ``crh_filter`` -- or a SET condition ``(column, codes, negate)``:
    the column's code is (``negate`` false) / is not (true) one of ``codes`` (any iterable of ints; ``negate`` may be left out)
    -- or a RANGE condition ``(column, lo, hi, "between" | "not_between")`` (:func:`is_range_condition`), which travels with the
    set conditions (``crh_condition``)."""
    return isinstance(item, RowWords) or len(item) in (3, 4) or not isinstance(item[1], (int, np.integer))


def is_range_condition(item) -> bool:
    """``(column, lo, hi, "between" | "not_between")``: the column's VALUE (a numeric column stores the value itself, -1 for
    "absent") lies / does not lie in ``lo .. hi``, both ends inclusive; ``lo > hi`` is an empty range.  A row without the value
    fails every "between" and passes every "not_between"."""
    return not isinstance(item, RowWords) and len(item) == 4


def _range_parts(item) -> tuple[int, int, int, int]:
    """(column, mode, lo, hi) of a range condition, the bounds clipped to what an int32 column can hold."""
    col, lo, hi, mode = item
    if not isinstance(mode, str) or mode not in RANGE_MODES:
        raise NativeError(E_INVALID, f"range condition mode {mode!r} is not one of {sorted(RANGE_MODES)}")
    return int(col), RANGE_MODES[mode], max(int(lo), 0), min(int(hi), VALUE_MAX)


def _conditions(filters, owner=None) -> tuple:
    """Any mix of the item forms as ``crh_condition``s: (array, n, the numpy sets the array points into -- keep them alive
    for the call).  ``owner``: the :class:`Index` asking, whose words a :class:`RowWords` hands over."""
    filters = list(filters or [])
    if len(filters) > MAX_FILTERS:
        raise NativeError(E_INVALID, f"at most {MAX_FILTERS} filter conditions are supported")
    arr, keep = (Condition * max(1, len(filters)))(), []
    for i, item in enumerate(filters):
        if isinstance(item, RowWords):
            w = item.words_of(owner)
            keep.append(w)
            arr[i].col, arr[i].negate, arr[i].n, arr[i].codes = item.tag, COND_NOT_WORDS if item.negate else COND_WORDS, int(w.numel()), int(w.data_ptr())
            continue
        if is_range_condition(item):
            col, negate, lo, hi = _range_parts(item)
            if hi < lo:
                lo, hi = 1, 0                      # (an empty range, whichever bound was clipped)
            codes = np.asarray([lo, hi], np.int32)
        elif is_set_condition(item):
            col, codes, negate = item[0], item[1], (bool(item[2]) if len(item) == 3 else False)
            codes = np.ascontiguousarray(sorted(int(c) for c in codes) if not isinstance(codes, np.ndarray) else codes, dtype=np.int32).reshape(-1)
        else:
            col, codes, negate = item[0], np.asarray([int(item[1])], np.int32), False
        keep.append(codes)
        arr[i].col, arr[i].negate, arr[i].n, arr[i].codes = int(col), int(negate), int(codes.size), codes.ctypes.data if codes.size else None
    return arr, len(filters), keep


def filter_key(filters) -> tuple:
    """A filter (list of conditions in either item form) as a hashable key: two filters with the same key select the same rows.
    Conditions are ordered, a set's codes sorted without repeats; ``(col, code)`` and ``(col, [code])`` are the same condition."""
    out = []
    for item in filters or []:
        if isinstance(item, RowWords):
            out.append((item.tag, COND_NOT_WORDS if item.negate else COND_WORDS, ()))
        elif is_range_condition(item):
            col, mode, lo, hi = _range_parts(item)
            out.append((col, mode, (lo, hi) if lo <= hi else (1, 0)))
        elif is_set_condition(item):
            out.append((int(item[0]), bool(item[2]) if len(item) == 3 else False, tuple(sorted({int(c) for c in item[1]}))))
        else:
            out.append((int(item[0]), False, (int(item[1]),)))
    return tuple(sorted(out))


def multi_plan(class_filters, query_class) -> tuple[list, np.ndarray, list[np.ndarray]]:
    """How a mixed-filter batch is issued: ``(classes, qclass, calls)``.  ``classes`` are the DISTINCT filters the queries use
    (:func:`filter_key`; first use first), ``qclass`` every query's index into them, ``calls`` the query positions of each
    ``crh_search_multi`` call: all of them, in caller order, while there are at most ``MAX_CLASSES`` classes; otherwise the
    queries ordered by class and cut so that no call sees more than ``MAX_CLASSES`` of them."""
    query_class = np.asarray(query_class, dtype=np.int64).reshape(-1)
    if query_class.size and (query_class.min() < 0 or query_class.max() >= len(class_filters)):
        raise NativeError(E_INVALID, f"query_class outside 0..{len(class_filters) - 1}")
    seen: dict[tuple, int] = {}
    classes, remap = [], {}
    for c in query_class.tolist():
        if c not in remap:
            key = filter_key(class_filters[c])
            if key not in seen:
                seen[key] = len(classes)
                classes.append(list(class_filters[c] or []))
            remap[c] = seen[key]
    qclass = np.asarray([remap[c] for c in query_class.tolist()], dtype=np.int32)
    if len(classes) <= MAX_CLASSES:
        return classes, qclass, [np.arange(qclass.size)]
    order = np.argsort(qclass, kind="stable")
    group = qclass[order] // MAX_CLASSES
    return classes, qclass, [order[group == g] for g in range((len(classes) + MAX_CLASSES - 1) // MAX_CLASSES)]


def multi_passes(class_filters, query_class, batch_q: int = 64) -> int:
    """Corpus passes a mixed-filter batch costs: every call of :func:`multi_plan` is cut into ``batch_q``-query passes."""
    return sum((len(c) + batch_q - 1) // batch_q for c in multi_plan(class_filters, query_class)[2])


def debug_i8_intervals(handle, rows: int, dim: int, queries, k: int, filters=None) -> dict:
    """``crh_debug_i8_intervals`` (debug library only): the int8 scan's intervals, quantisation parameters and thresholds for up to
    64 raw queries, from the product's own launches.  ``handle`` is a ``crh_index`` created by :func:`debug_lib` -- the two
    libraries do not share handles."""
    q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, dim)
    nq = q.shape[0]
    out = {"hi_rec": np.empty((nq, rows), np.float32), "hi": np.empty((nq, rows), np.float32), "lo": np.empty((nq, rows), np.float32),
           "srow": np.empty((rows,), np.float32), "qpar": np.empty((64, 4), np.float32), "dn": np.empty((1,), np.float32),
           "c_abs": np.empty((1,), np.float32), "tau": np.empty((nq,), np.float32)}
    farr, nf = _filters(filters)
    L = debug_lib()
    check(L.crh_debug_i8_intervals(handle, nq, q.ctypes.data, int(k), farr, nf, *(out[n].ctypes.data for n in
                                   ("hi_rec", "hi", "lo", "srow", "qpar", "dn", "c_abs", "tau"))), L)
    out["dn"], out["c_abs"] = np.float32(out["dn"][0]), np.float32(out["c_abs"][0])
    return out


# ``variant`` of crh_debug_kth_largest (coderag_hip.h): the product's instantiations of the selection helpers
DEBUG_SEL_FAST = {1024: 0, 512: 1, 256: 2}      # wg_kth_largest_fast<NT, NT, 256>
DEBUG_SEL_RADIX = {1024: 3, 512: 4, 256: 5}     # wg_kth_largest<u32, NT>; | DEBUG_SEL_U64: wg_kth_largest<u64, NT> (1024, 256)
DEBUG_SEL_U64 = 8
DEBUG_TAIL = {1024: 0, 256: 1}                  # select_tail<NT>


def debug_kth_largest(variant: int, keys, k, floor_key: int = 0, nblocks: int | None = None) -> np.ndarray:
    """``crh_debug_kth_largest`` (debug library only): the ``k[s]``-th largest key of each row of ``keys`` [nsets, n] (uint32, or
    uint64 for the ``DEBUG_SEL_U64`` variants) as the product's selection helper of that ``variant`` returns it, uint64 [nsets].
    ``nblocks`` workgroups share the sets (default: one each)."""
    keys = np.asarray(keys)
    if keys.dtype not in (np.uint32, np.uint64) or keys.ndim != 2:
        raise NativeError(E_INVALID, "keys must be a uint32 or uint64 array [nsets, n]")
    keys = np.ascontiguousarray(keys)
    nsets, n = keys.shape
    ks = np.ascontiguousarray(np.broadcast_to(np.asarray(k, dtype=np.uint32), (nsets,)))
    out = np.zeros((nsets,), np.uint64)
    L = debug_lib()
    wide = variant | DEBUG_SEL_U64 if keys.dtype == np.uint64 else variant
    check(L.crh_debug_kth_largest(int(wide), keys.ctypes.data, nsets, n, ks.ctypes.data, int(floor_key),
                                  nsets if nblocks is None else int(nblocks), out.ctypes.data), L)
    return out


def debug_select_tail(variant: int, keys, k: int, row_base: int = 0):
    """``crh_debug_select_tail`` (debug library only): (scores float32 [k], rows int64 [k]) that ``select_tail`` of that ``variant``
    writes for the uint64 ``keys``."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
    scores, rows = np.empty((max(int(k), 0),), np.float32), np.empty((max(int(k), 0),), np.int64)
    L = debug_lib()
    check(L.crh_debug_select_tail(int(variant), keys.ctypes.data, keys.size, int(k), int(row_base), scores.ctypes.data, rows.ctypes.data), L)
    return scores, rows


def debug_tile_list(mask_words, sentinel: int = 0xffffffff):
    """``crh_debug_tile_list`` (debug library only): (list uint32 [ntiles], len) of the two tile-list launches for the uint32
    ``mask_words``; the list buffer holds ``sentinel`` everywhere before them."""
    words = np.ascontiguousarray(mask_words, dtype=np.uint32).reshape(-1)
    lst, ln = np.full((words.size,), sentinel, np.uint32), np.zeros((1,), np.uint32)
    L = debug_lib()
    check(L.crh_debug_tile_list(words.ctypes.data, words.size, lst.ctypes.data, ln.ctypes.data), L)
    return lst, int(ln[0])


def range_thresholds(thresholds, nq: int) -> np.ndarray:
    """The thresholds of a range search as float32 ``[nq]``: a scalar stands for every query; NaN and infinities are refused."""
    thr = np.asarray(thresholds, dtype=np.float32)
    thr = np.full((nq,), thr, np.float32) if thr.ndim == 0 else np.ascontiguousarray(thr.reshape(-1))
    if thr.shape[0] != nq:
        raise NativeError(E_INVALID, f"{thr.shape[0]} thresholds for {nq} queries")
    if not np.isfinite(thr).all():
        raise NativeError(E_INVALID, "a score threshold must be a finite number")
    return thr


def _has_sets(filters) -> bool:
    return any(is_set_condition(item) for item in (filters or []))


def _ptr(x) -> int:
    """Raw address of a numpy array / torch tensor / int."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    return int(x.data_ptr())  # torch tensor


def _is_dev(x) -> int:
    return int(not isinstance(x, np.ndarray) and getattr(x, "is_cuda", False))


_NP_NAMES = {"float32": np.float32, "int32": np.int32, "int64": np.int64}


def _typed(x, want: str, what: str):
    """The C side sees a bare pointer: refuse anything whose element type or layout it would misread.
    numpy inputs are converted (a copy is fine on the host); device tensors must already be right."""
    if x is None or isinstance(x, int):
        return x
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(x, dtype=_NP_NAMES[want])
    if str(x.dtype).rsplit(".", 1)[-1] != want:
        raise NativeError(E_INVALID, f"{what} must be {want}, got {x.dtype}")
    if not x.is_contiguous():
        raise NativeError(E_INVALID, f"{what} must be contiguous")
    return x


def _out(x, want: str, what: str, shape):
    if isinstance(x, np.ndarray):
        if x.dtype != _NP_NAMES[want] or not x.flags.c_contiguous:
            raise NativeError(E_INVALID, f"{what} must be a C-contiguous {want} array")
    else:
        _typed(x, want, what)
    if tuple(x.shape) != tuple(shape):
        raise NativeError(E_INVALID, f"{what} has shape {tuple(x.shape)}, expected {tuple(shape)}")
    return x


class Index:
    """Owning wrapper of one ``crh_index`` handle (one collection shard on one GPU)."""

    def __init__(self, dim: int = 768, dtype: int = DTYPE_F32, capacity_rows: int = 65536,
                 n_code_cols: int = 0, device: int = 0):
        self.dim, self.dtype, self.n_code_cols, self.device = dim, dtype, n_code_cols, device
        h = C.c_void_p()
        check(lib().crh_index_create(dim, dtype, capacity_rows, n_code_cols, device, C.byref(h)))
        self._h = h
        self.capacity_rows = (capacity_rows + 31) // 32 * 32

    def close(self) -> None:
        if getattr(self, "_h", None) and _lib is not None:   # (module globals are gone at interpreter shutdown)
            _lib.crh_index_destroy(self._h)
            self._h = None

    __del__ = close

    def _handle(self):
        if not self._h:
            raise NativeError(E_INVALID, "index handle is closed")
        return self._h

    def reserve(self, capacity_rows: int) -> None:
        check(lib().crh_index_reserve(self._handle(), capacity_rows))
        self.capacity_rows = max(self.capacity_rows, (capacity_rows + 31) // 32 * 32)

    def append(self, vecs, codes=None, stream: int = 0, preprocessed: bool = False) -> int:
        """vecs: float32 [n, dim] numpy array (host) or CUDA torch tensor.  Returns the first new row.
        ``preprocessed=True`` stores the rows verbatim (restoring a snapshot made with :meth:`read_rows`)."""
        vecs = _typed(vecs, "float32", "vecs")
        codes = _typed(codes, "int32", "codes")
        n = int(vecs.shape[0])
        if n and int(vecs.shape[1]) != self.dim:
            raise NativeError(E_INVALID, f"vector dim {vecs.shape[1]} != index dim {self.dim}")
        if codes is not None and tuple(codes.shape) != (n, self.n_code_cols):
            raise NativeError(E_INVALID, f"codes shape {tuple(codes.shape)} != ({n}, {self.n_code_cols})")
        if codes is not None and _is_dev(codes) != _is_dev(vecs):
            raise NativeError(E_INVALID, "vecs and codes must live in the same memory space")
        first = C.c_int64(-1)
        fn = lib().crh_index_append_preprocessed if preprocessed else lib().crh_index_append
        check(fn(self._handle(), n, _ptr(vecs), _is_dev(vecs), _ptr(codes), C.byref(first), stream))
        return int(first.value)

    def tombstone(self, rows) -> None:
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        check(lib().crh_index_tombstone(self._handle(), rows.shape[0], rows.ctypes.data))

    SET_CONDITIONS = True  # filters may hold (column, codes, negate) set conditions (an injected stand-in may know equalities only)
    device_calls = 0      # filtered deletes / matches issued to the library by all handles (tests count the calls of a job)

    def tombstone_filter(self, filters) -> int:
        """Delete every alive row matching all conditions -- ``(column, code)`` equalities and ``(column, codes, negate)`` sets
        (:func:`is_set_condition`) -- on the device, in ONE call; returns how many."""
        n = C.c_int64(0)
        Index.device_calls += 1
        if _has_sets(filters):
            carr, nc, keep = _conditions(filters, self)
            check(lib().crh_index_tombstone_cond(self._handle(), carr, nc, C.byref(n)))
            del keep
        else:
            farr, nf = _filters(filters)
            check(lib().crh_index_tombstone_filter(self._handle(), farr, nf, C.byref(n)))
        return int(n.value)

    def set_sparse_route(self, enable: bool | None = None, max_fraction_den: int = 0) -> None:
        """The route of filtered searches whose mask leaves at most 1 tile in ``max_fraction_den`` populated (``crh_index_set_sparse_route``;
        None / 0 = keep).  ``enable=False`` is the A/B switch: every search takes the dense scans."""
        check(lib().crh_index_set_sparse_route(self._handle(), -1 if enable is None else int(bool(enable)), int(max_fraction_den)))

    def compact(self) -> np.ndarray:
        """Reclaim the rows of deleted points (``crh_index_compact``): the alive rows move down in their old order.  Returns
        ``old_to_new`` (int64 per old row: its new row number, -1 for a deleted one)."""
        rows, _ = self.count()
        o2n = np.empty((rows,), dtype=np.int64)
        after = C.c_int64(0)
        check(lib().crh_index_compact(self._handle(), o2n.ctypes.data if rows else None, C.byref(after)))
        return o2n

    # ------------------------------------------------------------------ snapshot
    SNAPSHOT_FORMAT = 3                     # 3: inside a 1-KiB piece the 16-byte chunks are ordered [row][half]; 2 (rounds 2-3): [half][row]
    SNAPSHOT_CHUNK_TILES = 1 << 15          # 32768 tiles = 1M rows per transfer (1.5 GiB of tiles at dim 768)

    def save(self, directory: str) -> dict:
        """Write the stored image VERBATIM into ``directory``: ``tiles.bin`` (the tiled bf16 image, raw and mmap-able:
        rows/32 tiles of dim/16 KiB), ``master.f32`` ([rows padded to 32, dim] f32; f32 store only), ``alive.u32`` (one word
        per tile, tombstones included), ``codes.i32`` ([n_code_cols][rows padded to 32] int32, columnar) and ``index.json``.
        No pickle, no compression, no f32 inflation of a bf16 store: 10M x 768 bf16 is 15.36 GB on disk."""
        import json
        rows, alive = self.count()
        ntiles = (rows + 31) // 32
        tile_bytes = self.dim // 16 * 1024
        os.makedirs(directory, exist_ok=True)
        # index.json is what makes a directory a snapshot: it goes away first and comes back last (os.replace), carrying the size
        # of every data file, so a save that died half way leaves no directory load() would accept
        try:
            os.remove(os.path.join(directory, "index.json"))
        except FileNotFoundError:
            pass
        meta = {"format": self.SNAPSHOT_FORMAT, "dim": self.dim, "dtype": "bf16" if self.dtype == DTYPE_BF16 else "f32",
                "rows": rows, "alive": alive, "tiles": ntiles, "n_code_cols": self.n_code_cols, "tile_bytes": tile_bytes,
                "files": {"tiles": "tiles.bin", "alive": "alive.u32", "codes": "codes.i32" if self.n_code_cols else None,
                          "master": "master.f32" if self.dtype == DTYPE_F32 else None}}

        def mm(name, dtype, shape):
            if 0 in shape:
                open(os.path.join(directory, name), "wb").close()
                return None
            return np.memmap(os.path.join(directory, name), dtype=dtype, mode="w+", shape=shape)
        tiles = mm("tiles.bin", np.uint8, (ntiles, tile_bytes))
        al = mm("alive.u32", np.uint32, (ntiles,))
        master = mm("master.f32", np.float32, (ntiles * 32, self.dim)) if self.dtype == DTYPE_F32 else None
        codes = mm("codes.i32", np.int32, (self.n_code_cols, ntiles * 32)) if self.n_code_cols else None
        for t0 in range(0, ntiles, self.SNAPSHOT_CHUNK_TILES):
            nt = min(self.SNAPSHOT_CHUNK_TILES, ntiles - t0)
            cbuf = np.empty((self.n_code_cols, nt * 32), np.int32) if self.n_code_cols else None
            check(lib().crh_index_export(self._handle(), t0, nt, tiles[t0:t0 + nt].ctypes.data,
                                         master[t0 * 32:(t0 + nt) * 32].ctypes.data if master is not None else None,
                                         al[t0:t0 + nt].ctypes.data, cbuf.ctypes.data if cbuf is not None else None))
            if cbuf is not None:
                codes[:, t0 * 32:(t0 + nt) * 32] = cbuf
        for m in (tiles, al, master, codes):
            if m is not None:
                m.flush()
        del tiles, al, master, codes
        meta["sizes"] = {name: os.path.getsize(os.path.join(directory, name)) for name in meta["files"].values() if name}
        with open(os.path.join(directory, "index.json.tmp"), "w") as f:
            json.dump(meta, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(os.path.join(directory, "index.json.tmp"), os.path.join(directory, "index.json"))
        return meta

    def load(self, directory: str, widen=None) -> dict:
        """Fill this EMPTY index from a directory written by :meth:`save` (same dim / dtype / code columns): the files are
        memory-mapped and moved to HBM chunk by chunk; searches answer with the same ids and identical score bits.
        ``widen(first_row, rows)`` -> int32 ``[extra, rows]``: the snapshot may hold FEWER code columns than this index; its
        columns come first and every imported chunk is completed with the ``extra`` missing ones (a collection snapshot written
        before the store kept line numbers on the device)."""
        import json
        with open(os.path.join(directory, "index.json")) as f:
            meta = json.load(f)
        want = {"dim": self.dim, "dtype": "bf16" if self.dtype == DTYPE_BF16 else "f32", "n_code_cols": self.n_code_cols}
        have_cols = meta.get("n_code_cols")
        for key, val in want.items():
            if meta.get(key) != val and not (key == "n_code_cols" and widen is not None and isinstance(have_cols, int) and 0 <= have_cols < val):
                raise NativeError(E_INVALID, f"snapshot {directory} has {key}={meta.get(key)!r}, this index {val!r}")
        if meta.get("format") not in (2, self.SNAPSHOT_FORMAT):
            raise NativeError(E_INVALID, f"snapshot {directory} has format={meta.get('format')!r}, this library reads 2 and {self.SNAPSHOT_FORMAT}")
        old_piece_order = meta.get("format") == 2        # [half][row] chunks inside a piece: reordered chunk by chunk below
        if self.count()[0] != 0:
            raise NativeError(E_INVALID, "load() needs an empty index")
        rows, ntiles, tile_bytes = int(meta["rows"]), int(meta["tiles"]), int(meta["tile_bytes"])
        if ntiles != (rows + 31) // 32 or tile_bytes != self.dim // 16 * 1024:
            raise NativeError(E_INVALID, f"snapshot {directory}: inconsistent index.json")
        for name, size in (meta.get("sizes") or {}).items():
            if os.path.getsize(os.path.join(directory, name)) != int(size):
                raise NativeError(E_INVALID, f"snapshot file {os.path.join(directory, name)} is not the size index.json recorded")
        if rows == 0:
            return meta
        self.reserve(rows)

        def mm(name, dtype, shape):
            path = os.path.join(directory, name)
            if os.path.getsize(path) != int(np.prod(shape)) * np.dtype(dtype).itemsize:
                raise NativeError(E_INVALID, f"snapshot file {path} has the wrong size")
            return np.memmap(path, dtype=dtype, mode="r", shape=shape)
        tiles = mm("tiles.bin", np.uint8, (ntiles, tile_bytes))
        al = mm("alive.u32", np.uint32, (ntiles,))
        master = mm("master.f32", np.float32, (ntiles * 32, self.dim)) if self.dtype == DTYPE_F32 else None
        codes = mm("codes.i32", np.int32, (have_cols, ntiles * 32)) if have_cols else None
        for t0 in range(0, ntiles, self.SNAPSHOT_CHUNK_TILES):
            nt = min(self.SNAPSHOT_CHUNK_TILES, ntiles - t0)
            cbuf = np.ascontiguousarray(codes[:, t0 * 32:(t0 + nt) * 32]) if codes is not None else None
            if have_cols < self.n_code_cols:             # the missing columns of this chunk's rows (-1 behind the last row)
                real = min(rows, (t0 + nt) * 32) - t0 * 32
                extra = np.full((self.n_code_cols - have_cols, nt * 32), -1, np.int32)
                extra[:, :real] = np.asarray(widen(t0 * 32, real), np.int32).reshape(self.n_code_cols - have_cols, real)
                cbuf = np.ascontiguousarray(extra if cbuf is None else np.concatenate([cbuf, extra]))
            abuf = np.ascontiguousarray(al[t0:t0 + nt])
            tbuf = tiles[t0:t0 + nt]
            if old_piece_order:
                tbuf = np.ascontiguousarray(tbuf.reshape(nt, self.dim // 16, 2, 32, 16).transpose(0, 1, 3, 2, 4))
            check(lib().crh_index_import(self._handle(), t0, nt, min(rows, (t0 + nt) * 32), tbuf.ctypes.data,
                                         master[t0 * 32:(t0 + nt) * 32].ctypes.data if master is not None else None,
                                         abuf.ctypes.data, cbuf.ctypes.data if cbuf is not None else None))
        got_rows, got_alive = self.count()
        if got_rows != rows or got_alive != int(meta["alive"]):
            raise NativeError(E_INTERNAL, f"snapshot {directory}: restored {got_rows} rows / {got_alive} alive, index.json says {rows} / {meta['alive']}")
        return meta

    def alive_words(self) -> np.ndarray:
        """One validity word per 32-row tile (bit b of word t = row 32t+b is alive)."""
        ntiles = (self.count()[0] + 31) // 32
        out = np.zeros((ntiles,), np.uint32)
        if ntiles:
            check(lib().crh_index_export(self._handle(), 0, ntiles, None, None, out.ctypes.data, None))
        return out

    def count(self) -> tuple[int, int]:
        r, a = C.c_int64(0), C.c_int64(0)
        check(lib().crh_index_count(self._handle(), C.byref(r), C.byref(a)))
        return int(r.value), int(a.value)

    def clear(self) -> None:
        check(lib().crh_index_clear(self._handle()))

    def read_rows(self, first: int, n: int) -> np.ndarray:
        out = np.empty((n, self.dim), dtype=np.float32)
        check(lib().crh_index_read_rows(self._handle(), first, n, out.ctypes.data))
        return out

    def gather_vectors(self, rows, row_base: int = 0, out=None, stream: int = 0):
        """Stored vectors of a candidate table (``crh_index_gather_vectors``): ``rows`` is a CUDA int64 tensor of GLOBAL rows
        (any shape); returns / fills ``out``, a CUDA float32 tensor ``rows.shape + (dim,)`` -- the stored row where this index
        owns it (``row_base <= row < row_base + count``), zeros elsewhere (padding -1 included).  Enqueues only."""
        import torch
        if not _is_dev(rows):
            raise NativeError(E_INVALID, "rows must be a device tensor")
        rows = _typed(rows, "int64", "rows")
        shape = tuple(rows.shape) + (self.dim,)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=rows.device)
        else:
            _out(out, "float32", "out", shape)
            if not _is_dev(out):
                raise NativeError(E_INVALID, "out must be a device tensor")
        check(lib().crh_index_gather_vectors(self._handle(), int(rows.numel()), _ptr(rows), int(row_base), _ptr(out), stream))
        return out

    def gather_codes(self, rows, col: int, row_base: int = 0, out=None, stream: int = 0):
        """Codes of payload column ``col`` for a candidate table (``crh_index_gather_codes``): ``rows`` is a CUDA int64 tensor
        of GLOBAL rows (any shape); fills ``out``, a CUDA int32 tensor of the same shape, where this index owns the row
        (``row_base <= row < row_base + count``) and leaves every other position as it was -- ``out`` is allocated full of -1
        when not given, and several shards may be handed the same buffer.  Enqueues only."""
        import torch
        if not _is_dev(rows):
            raise NativeError(E_INVALID, "rows must be a device tensor")
        rows = _typed(rows, "int64", "rows")
        if out is None:
            out = torch.full(tuple(rows.shape), -1, dtype=torch.int32, device=rows.device)
        else:
            _out(out, "int32", "out", tuple(rows.shape))
            if not _is_dev(out):
                raise NativeError(E_INVALID, "out must be a device tensor")
        check(lib().crh_index_gather_codes(self._handle(), int(col), int(rows.numel()), _ptr(rows), int(row_base), _ptr(out), stream))
        return out

    def set_tuning(self, seed_tiles: int = 0, wave_cand_cap: int = 0, query_cand_cap: int = 0,
                   force_fallback: int = -1) -> None:
        check(lib().crh_index_set_tuning(self._handle(), seed_tiles, wave_cand_cap, query_cand_cap, force_fallback))

    def set_nomination(self, mode: int) -> None:
        """The most advanced way the index may nominate a <= 64-query batch: NOMINATE_BF16_3 / NOMINATE_BF16 / NOMINATE_INT8."""
        check(lib().crh_index_set_nomination(self._handle(), mode))

    def nomination(self) -> int:
        """The mode the next <= 64-query batch would use (the index may have fallen back by itself)."""
        out = C.c_int32(0)
        check(lib().crh_index_get_nomination(self._handle(), C.byref(out)))
        return int(out.value)

    def search(self, queries, k: int, filters=None, row_base: int = 0, out_scores=None, out_rows=None,
               stream: int = 0):
        """queries: [nq, dim] float32 numpy (host) or CUDA tensor.  With ``out_*`` CUDA tensors the call is
        asynchronous (finish with :meth:`search_finish`); otherwise numpy results are returned."""
        queries = _typed(queries, "float32", "queries")
        if queries.ndim == 1:
            queries = queries[None, :]
        nq = int(queries.shape[0])
        if nq and int(queries.shape[1]) != self.dim:
            raise NativeError(E_INVALID, f"query dim {queries.shape[1]} != index dim {self.dim}")
        if not 0 < k <= MAX_K:
            raise NativeError(E_CAPACITY, f"k={k} outside 1..{MAX_K}")
        if out_scores is None:
            out_scores = np.empty((nq, k), dtype=np.float32)
            out_rows = np.empty((nq, k), dtype=np.int64)
        else:
            _out(out_scores, "float32", "out_scores", (nq, k))
            _out(out_rows, "int64", "out_rows", (nq, k))
            if _is_dev(out_scores) != _is_dev(out_rows):
                raise NativeError(E_INVALID, "out_scores and out_rows must live in the same memory space")
        if _has_sets(filters):
            carr, nc, keep = _conditions(filters, self)
            check(lib().crh_search_cond(self._handle(), nq, _ptr(queries), _is_dev(queries), k, carr, nc, row_base,
                                        _ptr(out_scores), _ptr(out_rows), _is_dev(out_scores), stream))
            del keep
        else:
            farr, nf = _filters(filters)
            check(lib().crh_search(self._handle(), nq, _ptr(queries), _is_dev(queries), k, farr, nf, row_base,
                                   _ptr(out_scores), _ptr(out_rows), _is_dev(out_scores), stream))
        return out_scores, out_rows

    def search_multi(self, queries, k: int, class_filters, query_class, row_base: int = 0, out_scores=None, out_rows=None,
                     stream: int = 0):
        """:meth:`search` for a batch whose queries carry DIFFERENT filters: query ``i`` is answered under
        ``class_filters[query_class[i]]`` (each a filter as :meth:`search` takes it, None / empty = every alive row), and row
        ``i`` of the result is what :meth:`search` returns for query ``i`` alone under that filter -- ids and score bits.  Up to
        ``MAX_CLASSES`` distinct filters share each 64-query corpus pass (``crh_search_multi``; always the three-launch bf16 scan).
        Equal filters are one class however often they are listed.  With more than ``MAX_CLASSES`` distinct filters the queries
        are ordered by class and issued in several calls, results in caller order (device outputs are then complete on return:
        the calls are finished here).  A batch that uses ONE distinct filter takes :meth:`search` itself -- the code it runs today."""
        queries = _typed(queries, "float32", "queries")
        if queries.ndim == 1:
            queries = queries[None, :]
        nq = int(queries.shape[0])
        if len(query_class) != nq:
            raise NativeError(E_INVALID, f"query_class has {len(query_class)} entries for {nq} queries")
        classes, qclass, calls = multi_plan(class_filters, query_class)
        if len(classes) <= 1:
            return self.search(queries, k, filters=classes[0] if classes else None, row_base=row_base, out_scores=out_scores, out_rows=out_rows,
                               stream=stream)
        if nq and int(queries.shape[1]) != self.dim:
            raise NativeError(E_INVALID, f"query dim {queries.shape[1]} != index dim {self.dim}")
        if not 0 < k <= MAX_K:
            raise NativeError(E_CAPACITY, f"k={k} outside 1..{MAX_K}")
        if out_scores is None:
            out_scores = np.empty((nq, k), dtype=np.float32)
            out_rows = np.empty((nq, k), dtype=np.int64)
        else:
            _out(out_scores, "float32", "out_scores", (nq, k))
            _out(out_rows, "int64", "out_rows", (nq, k))
            if _is_dev(out_scores) != _is_dev(out_rows):
                raise NativeError(E_INVALID, "out_scores and out_rows must live in the same memory space")
        if len(calls) == 1:
            self._search_multi_native(queries, k, classes, qclass, row_base, out_scores, out_rows, stream)
            return out_scores, out_rows
        for sel in calls:
            used = sorted(set(qclass[sel].tolist()))
            local = np.asarray([used.index(c) for c in qclass[sel].tolist()], dtype=np.int32)
            if isinstance(queries, np.ndarray):
                q = np.ascontiguousarray(queries[sel])
            else:
                import torch
                q = queries[torch.as_tensor(sel, device=queries.device)].contiguous()
            if _is_dev(out_scores):
                import torch
                idx = torch.as_tensor(sel, device=out_scores.device)
                ps = torch.empty((len(sel), k), dtype=torch.float32, device=out_scores.device)
                pr = torch.empty((len(sel), k), dtype=torch.int64, device=out_scores.device)
                self._search_multi_native(q, k, [classes[c] for c in used], local, row_base, ps, pr, stream)
                self.search_finish(stream)
                out_scores[idx], out_rows[idx] = ps, pr
            else:
                ps, pr = np.empty((len(sel), k), np.float32), np.empty((len(sel), k), np.int64)
                self._search_multi_native(q, k, [classes[c] for c in used], local, row_base, ps, pr, stream)
                out_scores[sel], out_rows[sel] = ps, pr
        return out_scores, out_rows

    def _search_multi_native(self, queries, k: int, classes, qclass, row_base, out_scores, out_rows, stream) -> None:
        """One ``crh_search_multi`` call: at most ``MAX_CLASSES`` filters, ``qclass`` int32 per query."""
        flat, off = [], [0]
        for f in classes:
            f = list(f or [])
            if len(f) > MAX_FILTERS:
                raise NativeError(E_INVALID, f"at most {MAX_FILTERS} filter conditions are supported")
            flat += f
            off.append(len(flat))
        carr, keep = (Condition * max(1, len(flat)))(), []
        for i, item in enumerate(flat):
            one, _, kp = _conditions([item], self)
            carr[i] = one[0]
            keep.append(kp)
        off = np.asarray(off, dtype=np.int32)
        qclass = np.ascontiguousarray(qclass, dtype=np.int32)
        check(lib().crh_search_multi(self._handle(), int(queries.shape[0]), _ptr(queries), _is_dev(queries), k, carr, off.ctypes.data, len(classes),
                                     qclass.ctypes.data, row_base, _ptr(out_scores), _ptr(out_rows), _is_dev(out_scores), stream))
        del keep

    def search_range(self, queries, k: int, thresholds, filters=None, row_base: int = 0, counts: bool = True, out_scores=None, out_rows=None,
                     out_counts=None, stream: int = 0):
        """:meth:`search` with a score threshold per query (``crh_search_range``): ``thresholds`` is a scalar or ``[nq]``, finite.
        A row is IN RANGE iff it is alive, passes ``filters`` and its score is ``>=`` the query's threshold as f32 values
        (inclusive).  Returns ``(scores, rows, counts)``: the exact top-``k`` cut after its last in-range entry, padded with
        ``(-inf, -1)``, and -- with ``counts`` -- int64 ``[nq]``, the number of in-range rows however many there are (not clipped
        at ``k``); ``counts=False`` is the list-only mode and returns ``None`` there.  With ``out_*`` CUDA tensors (``out_counts``
        as well when counts are wanted) the call is asynchronous: finish with :meth:`search_finish`."""
        queries = _typed(queries, "float32", "queries")
        if queries.ndim == 1:
            queries = queries[None, :]
        nq = int(queries.shape[0])
        if nq and int(queries.shape[1]) != self.dim:
            raise NativeError(E_INVALID, f"query dim {queries.shape[1]} != index dim {self.dim}")
        if not 0 < k <= MAX_K:
            raise NativeError(E_INVALID, f"k={k} outside 1..{MAX_K}")
        thr = range_thresholds(thresholds, nq)
        if out_scores is None:
            if out_rows is not None or out_counts is not None:
                raise NativeError(E_INVALID, "out_rows / out_counts without out_scores")
            out_scores = np.empty((nq, k), dtype=np.float32)
            out_rows = np.empty((nq, k), dtype=np.int64)
            out_counts = np.empty((nq,), dtype=np.int64) if counts else None
        else:
            _out(out_scores, "float32", "out_scores", (nq, k))
            _out(out_rows, "int64", "out_rows", (nq, k))
            if counts:
                if out_counts is None:
                    raise NativeError(E_INVALID, "counts are wanted: out_counts must be given with out_scores / out_rows")
                _out(out_counts, "int64", "out_counts", (nq,))
            elif out_counts is not None:
                raise NativeError(E_INVALID, "out_counts given with counts=False")
            if _is_dev(out_scores) != _is_dev(out_rows) or (counts and _is_dev(out_counts) != _is_dev(out_scores)):
                raise NativeError(E_INVALID, "out_scores, out_rows and out_counts must live in the same memory space")
        carr, nc, keep = _conditions(filters, self)
        check(lib().crh_search_range(self._handle(), nq, _ptr(queries), _is_dev(queries), k, thr.ctypes.data, carr, nc, row_base,
                                     _ptr(out_scores), _ptr(out_rows), _ptr(out_counts) if counts else None, _is_dev(out_scores), stream))
        del keep
        return out_scores, out_rows, (out_counts if counts else None)

    def search_finish(self, stream: int = 0) -> None:
        check(lib().crh_search_finish(self._handle(), stream))

    def stats(self) -> dict:
        s = SearchStats()
        check(lib().crh_search_get_stats(self._handle(), C.byref(s)))
        return s.as_dict()

    def set_profiling(self, enable) -> None:
        """True / 1: HIP events around the dominant kernel of every batch; 2: around all three launches of the int8 scan."""
        check(lib().crh_index_set_profiling(self._handle(), int(enable)))

    def profile(self) -> tuple[float, int]:
        """(total ms, launches) of the scan kernel since profiling was enabled (HIP events on its stream)."""
        ms, n = C.c_double(0.0), C.c_int64(0)
        check(lib().crh_index_get_profile(self._handle(), C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def count_matching(self, filters=None) -> int:
        """Number of alive rows matching the filters (resolved on the device)."""
        return self._match(filters, 1 << 62, None)

    def _match(self, filters, limit: int, out) -> int:
        n = C.c_int64(0)
        Index.device_calls += 1
        if _has_sets(filters):
            carr, nc, keep = _conditions(filters, self)
            check(lib().crh_index_match_rows_cond(self._handle(), carr, nc, limit, out, C.byref(n)))
            del keep
        else:
            farr, nf = _filters(filters)
            check(lib().crh_index_match_rows(self._handle(), farr, nf, limit, out, C.byref(n)))
        return int(n.value)

    def match_rows(self, filters=None, limit: int = 1) -> np.ndarray:
        out = np.empty((max(limit, 1),), dtype=np.int64)
        return out[: self._match(filters, limit, out.ctypes.data)].copy()

    def row_mask(self, filters=None, out=None, stream: int = 0):
        """The validity words a search under ``filters`` uses (``crh_index_row_mask``): alive AND filter, one uint32 per 32-row
        tile -- an int32 CUDA tensor of ``ceil(rows / 32)`` words (given or allocated).  This is how tombstones and filters
        reach a :class:`Lex`.  Enqueues on ``stream``."""
        import torch
        words = (self.count()[0] + 31) // 32
        if out is None:
            out = torch.empty((words,), dtype=torch.int32, device=f"cuda:{self.device}")
        _typed(out, "int32", "out")
        if not _is_dev(out) or out.ndim != 1 or int(out.shape[0]) < words:
            raise NativeError(E_INVALID, f"out must be a device tensor of at least {words} words")
        carr, nc, keep = _conditions(filters, self)
        check(lib().crh_index_row_mask(self._handle(), carr, nc, _ptr(out), int(out.shape[0]), stream))
        del keep
        return out

    @staticmethod
    def _facet_out(out, lead: tuple, n_bins: int):
        """``out = (bins, info)`` checked: int64 CUDA tensors ``lead + (n_bins,)`` and ``lead + (3,)``."""
        bins, info = out
        for x, what, shape in ((bins, "out bins", lead + (n_bins,)), (info, "out info", lead + (3,))):
            _out(x, "int64", what, shape)
            if not _is_dev(x):
                raise NativeError(E_INVALID, f"{what} must be a device tensor")
        return bins, info

    def facet(self, col: int, n_bins: int, filters=None, out=None, stream: int = 0):
        """Exact per-code counts of dictionary column ``col`` over the rows a search under ``filters`` sees
        (``crh_index_facet``; any item form of :func:`_conditions`, :class:`RowWords` included).  Returns / fills ``out =
        (bins, info)``: int64 CUDA tensors ``[n_bins]`` and ``[3]`` = (counted, missing: code -1, out_of_range: code >=
        ``n_bins``).  ``n_bins`` up to ``FACET_LDS_BINS`` is counted in LDS, more by runs of equal codes: the bins are the same.
        Every slot is overwritten.  Enqueues on ``stream``."""
        import torch
        n_bins = int(n_bins)
        if n_bins < 1:
            raise NativeError(E_INVALID, f"n_bins={n_bins} must be >= 1")
        if out is None:
            dev = f"cuda:{self.device}"
            out = (torch.empty((n_bins,), dtype=torch.int64, device=dev), torch.empty((3,), dtype=torch.int64, device=dev))
        bins, info = self._facet_out(out, (), n_bins)
        carr, nc, keep = _conditions(filters, self)
        check(lib().crh_index_facet(self._handle(), int(col), carr, nc, n_bins, _ptr(bins), _ptr(info), stream))
        del keep
        return bins, info

    def search_range_facet(self, queries, thresholds, col: int, n_bins: int, filters=None, out=None, stream: int = 0):
        """The semantic facet (``crh_search_range_facet``): per query the counts of column ``col`` over the rows IN RANGE as
        :meth:`search_range` defines it (alive, passes ``filters``, score ``>=`` the query's threshold, inclusive).  Returns /
        fills ``out = (bins, info)``: int64 CUDA tensors ``[nq, n_bins]`` and ``[nq, 3]`` = (counted -- :meth:`search_range`'s
        count --, missing, out_of_range).  Overwrites; the batches are finished when the call returns."""
        import torch
        queries = _typed(queries, "float32", "queries")
        if queries.ndim == 1:
            queries = queries[None, :]
        nq = int(queries.shape[0])
        if nq and int(queries.shape[1]) != self.dim:
            raise NativeError(E_INVALID, f"query dim {queries.shape[1]} != index dim {self.dim}")
        n_bins = int(n_bins)
        if n_bins < 1:
            raise NativeError(E_INVALID, f"n_bins={n_bins} must be >= 1")
        thr = range_thresholds(thresholds, nq)
        if out is None:
            dev = f"cuda:{self.device}"
            out = (torch.empty((nq, n_bins), dtype=torch.int64, device=dev), torch.empty((nq, 3), dtype=torch.int64, device=dev))
        bins, info = self._facet_out(out, (nq,), n_bins)
        carr, nc, keep = _conditions(filters, self)
        check(lib().crh_search_range_facet(self._handle(), nq, _ptr(queries), _is_dev(queries), thr.ctypes.data, carr, nc, int(col), n_bins,
                                           _ptr(bins), _ptr(info), stream))
        del keep
        return bins, info


def lex_queries(queries, idf) -> tuple:
    """Per-query ascending distinct term ids and their idf as the CSR ``crh_lex_search`` takes: (q_off int64, terms uint32, idf
    float32).  More than ``LEX_MAX_QUERY_TERMS`` ids in a query, ids that do not ascend strictly, or an idf list of another
    length are refused here, before anything reaches the library."""
    if len(queries) != len(idf):
        raise NativeError(E_INVALID, f"{len(queries)} queries but {len(idf)} idf lists")
    off, ts, ws = [0], [], []
    for q, (t, w) in enumerate(zip(queries, idf)):
        t, w = np.asarray(t, dtype=np.uint32).reshape(-1), np.asarray(w, dtype=np.float32).reshape(-1)
        if t.size > LEX_MAX_QUERY_TERMS:
            raise NativeError(E_INVALID, f"query {q} has {t.size} terms, at most {LEX_MAX_QUERY_TERMS} are searched")
        if t.size != w.size:
            raise NativeError(E_INVALID, f"query {q} has {t.size} terms but {w.size} idf values")
        if t.size > 1 and not (t[1:] > t[:-1]).all():
            raise NativeError(E_INVALID, f"the term ids of query {q} are not strictly ascending")
        ts.append(t)
        ws.append(w)
        off.append(off[-1] + t.size)
    cat = lambda parts, dt: np.ascontiguousarray(np.concatenate(parts), dtype=dt) if parts else np.zeros(0, dt)   # noqa: E731
    return np.asarray(off, np.int64), cat(ts, np.uint32), cat(ws, np.float32)


class Lex:
    """Owning wrapper of one ``crh_lex`` handle: the forward index of term ids beside one :class:`Index` (same rows, same
    numbering), searched with exact BM25 on the device."""

    def __init__(self, capacity_rows: int = 0, device: int = 0):
        self.device = device
        h = C.c_void_p()
        check(lib().crh_lex_create(device, int(capacity_rows), C.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None) and _lib is not None:
            _lib.crh_lex_destroy(self._h)
            self._h = None

    __del__ = close

    def _handle(self):
        if not self._h:
            raise NativeError(E_INVALID, "lex handle is closed")
        return self._h

    def clear(self) -> None:
        check(lib().crh_lex_clear(self._handle()))

    def count(self) -> tuple[int, int]:
        """(rows, entries)."""
        r, e = C.c_int64(0), C.c_int64(0)
        check(lib().crh_lex_count(self._handle(), C.byref(r), C.byref(e)))
        return int(r.value), int(e.value)

    def append(self, row_off, terms, tf, dl) -> None:
        """``n`` rows behind the existing ones: CSR ``row_off`` int64 [n + 1] from 0, ``terms`` uint32 / ``tf`` uint8 per entry
        (a row's ids strictly ascending, tf >= 1), ``dl`` int32 per row (>= the sum of the row's tf).  All or nothing."""
        row_off = np.ascontiguousarray(row_off, dtype=np.int64).reshape(-1)
        terms = np.ascontiguousarray(terms, dtype=np.uint32).reshape(-1)
        tf = np.ascontiguousarray(tf, dtype=np.uint8).reshape(-1)
        dl = np.ascontiguousarray(dl, dtype=np.int32).reshape(-1)
        n = int(dl.size)
        if row_off.size != n + 1 or terms.size != tf.size or (n and int(row_off[-1]) != terms.size):
            raise NativeError(E_INVALID, f"append: row_off {row_off.size}, terms {terms.size}, tf {tf.size}, dl {n} do not make a CSR")
        check(lib().crh_lex_append(self._handle(), n, row_off.ctypes.data, terms.ctypes.data, tf.ctypes.data, dl.ctypes.data))

    def stats(self, terms, mask=None) -> tuple:
        """``(df int64 per term, rows, sum_dl)`` over the rows whose bit is set in ``mask`` (a device tensor of validity words as
        :meth:`Index.row_mask` returns it, complete on its stream; None: every row).  Synchronous."""
        terms = np.ascontiguousarray(terms, dtype=np.uint32).reshape(-1)
        df = np.zeros(terms.size, np.int64)
        rows, total = C.c_int64(0), C.c_int64(0)
        self._check_mask(mask)
        check(lib().crh_lex_stats(self._handle(), _ptr(mask), terms.size, terms.ctypes.data, df.ctypes.data, C.byref(rows), C.byref(total)))
        return df, int(rows.value), int(total.value)

    def _check_mask(self, mask) -> None:
        if mask is None:
            return
        _typed(mask, "int32", "mask")
        if not _is_dev(mask) or int(mask.numel()) < (self.count()[0] + 31) // 32:
            raise NativeError(E_INVALID, "mask must be a device tensor of one word per 32-row tile")

    def search(self, queries, idf, k: int, k1: float = 1.2, b: float = 0.75, avgdl: float = 1.0, mask=None, row_base: int = 0,
               out_scores=None, out_rows=None, out_count=None, stream: int = 0):
        """Exact BM25 top-``k`` (``crh_lex_search``): ``queries`` per query its distinct term ids ascending, ``idf`` the f32 idf
        of each.  Returns CUDA tensors ``(scores f32 [nq, k], rows i64 [nq, k], count i64 [nq])``; tail (-inf, -1); ``count``
        is the number of qualifying rows, never clipped.  Waits on ``stream``."""
        import torch
        q_off, terms, w = lex_queries(queries, idf)
        nq, k = len(queries), int(k)
        if not 1 <= k <= MAX_K:
            raise NativeError(E_INVALID, f"k={k} outside 1..{MAX_K}")
        self._check_mask(mask)
        dev = f"cuda:{self.device}"
        out_scores = torch.empty((nq, k), dtype=torch.float32, device=dev) if out_scores is None else _out(out_scores, "float32", "out_scores", (nq, k))
        out_rows = torch.empty((nq, k), dtype=torch.int64, device=dev) if out_rows is None else _out(out_rows, "int64", "out_rows", (nq, k))
        out_count = torch.empty((nq,), dtype=torch.int64, device=dev) if out_count is None else _out(out_count, "int64", "out_count", (nq,))
        check(lib().crh_lex_search(self._handle(), nq, q_off.ctypes.data, terms.ctypes.data, w.ctypes.data, float(k1), float(b), float(avgdl), k,
                                   _ptr(mask), int(row_base), _ptr(out_scores), _ptr(out_rows), _ptr(out_count), stream))
        return out_scores, out_rows, out_count


def text_patterns(patterns) -> tuple:
    """Byte patterns as the CSR ``crh_text_match`` takes: (n, pat_off int64, bytes uint8).  1..``TEXT_MAX_PATTERNS`` patterns of
    1..``TEXT_MAX_PATTERN_BYTES`` bytes each are the library's limits; it is the library that refuses what breaks them."""
    pats = [bytes(p) for p in patterns]
    off = np.zeros(len(pats) + 1, np.int64)
    np.cumsum([len(p) for p in pats], out=off[1:])
    return len(pats), off, np.frombuffer(b"".join(pats) or b"\0", dtype=np.uint8).copy()


class Text:
    """Owning wrapper of one ``crh_text`` handle: the text arena beside one :class:`Index` (same rows, same numbering), matched
    against literal byte patterns on the device."""
    match_calls = 0       # crh_text_match calls issued by all handles (tests count the greps of a job)
    regex_calls = 0       # crh_text_regex calls issued by all handles
    fuzzy_calls = 0       # crh_text_fuzzy calls issued by all handles

    def __init__(self, capacity_rows: int = 0, capacity_bytes: int = 0, device: int = 0):
        self.device = device
        h = C.c_void_p()
        check(lib().crh_text_create(device, int(capacity_rows), int(capacity_bytes), C.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None) and _lib is not None:
            _lib.crh_text_destroy(self._h)
            self._h = None

    __del__ = close

    def _handle(self):
        if not self._h:
            raise NativeError(E_INVALID, "text handle is closed")
        return self._h

    def clear(self) -> None:
        check(lib().crh_text_clear(self._handle()))

    def count(self) -> tuple[int, int]:
        """(rows, bytes)."""
        r, b = C.c_int64(0), C.c_int64(0)
        check(lib().crh_text_count(self._handle(), C.byref(r), C.byref(b)))
        return int(r.value), int(b.value)

    def append(self, row_off, data) -> None:
        """``n`` rows behind the existing ones: ``row_off`` int64 [n + 1] from 0, ``data`` their bytes (bytes-like or uint8
        array of ``row_off[n]`` bytes).  All or nothing."""
        row_off = np.ascontiguousarray(row_off, dtype=np.int64).reshape(-1)
        data = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        n = int(row_off.size) - 1
        if n < 0 or (n and int(row_off[-1]) != data.size):
            raise NativeError(E_INVALID, f"append: row_off {row_off.size} entries ending at {int(row_off[-1]) if n >= 0 else None}, {data.size} bytes")
        check(lib().crh_text_append(self._handle(), n, row_off.ctypes.data, data.ctypes.data if data.size else None))

    def match(self, patterns, fold_case: bool = False, any_of: bool = False, mask=None, out=None, count: bool = True, stream: int = 0):
        """Which rows hold the byte ``patterns`` (``crh_text_match``): all of them, or -- ``any_of`` -- at least one; ``fold_case``
        folds ASCII letters only.  ``mask``: device validity words as :meth:`Index.row_mask` returns them, complete on
        ``stream`` (None: every row).  Returns ``(words int32 device tensor [ceil(rows / 32)], count or None)``; with ``count``
        the call waits on ``stream``."""
        import torch
        n, off, data = text_patterns(patterns)
        words = (self.count()[0] + 31) // 32
        if mask is not None:
            _typed(mask, "int32", "mask")
            if not _is_dev(mask) or int(mask.numel()) < words:
                raise NativeError(E_INVALID, "mask must be a device tensor of one word per 32-row tile")
        if out is None:
            out = torch.empty((words,), dtype=torch.int32, device=f"cuda:{self.device}")
        _typed(out, "int32", "out")
        if not _is_dev(out) or out.ndim != 1 or int(out.shape[0]) < words:
            raise NativeError(E_INVALID, f"out must be a device tensor of at least {words} words")
        c = C.c_int64(0)
        Text.match_calls += 1
        check(lib().crh_text_match(self._handle(), n, off.ctypes.data, data.ctypes.data, int(bool(fold_case)), TEXT_ANY if any_of else TEXT_ALL,
                                   _ptr(mask), _ptr(out), C.byref(c) if count else None, stream))
        return out, (int(c.value) if count else None)

    def regex(self, dfa, mask=None, out=None, count: bool = True, stream: int = 0):
        """Which rows the byte DFA ``dfa`` matches (``crh_text_regex``): anything with ``n_states``,
        ``n_classes``, ``class_of`` (256 entries), ``end_class``, ``trans`` (``n_states * n_classes`` entries) and ``accept`` --
        a ``regex_dfa.RegexDFA``.  It is the library that refuses a table that breaks its limits.  ``mask``, ``out``, ``count``
        and ``stream`` as in :meth:`match`."""
        import torch
        n_states, n_classes = int(dfa.n_states), int(dfa.n_classes)
        class_of = np.ascontiguousarray(dfa.class_of, dtype=np.uint8).reshape(-1)
        trans = np.ascontiguousarray(dfa.trans, dtype=np.uint8).reshape(-1)
        if class_of.size != 256 or n_states < 0 or n_classes < 0 or trans.size != n_states * n_classes:
            raise NativeError(E_INVALID, f"regex: class_of has {class_of.size} entries (256), trans {trans.size} ({n_states} states x {n_classes} classes)")
        words = (self.count()[0] + 31) // 32
        if mask is not None:
            _typed(mask, "int32", "mask")
            if not _is_dev(mask) or int(mask.numel()) < words:
                raise NativeError(E_INVALID, "mask must be a device tensor of one word per 32-row tile")
        if out is None:
            out = torch.empty((words,), dtype=torch.int32, device=f"cuda:{self.device}")
        _typed(out, "int32", "out")
        if not _is_dev(out) or out.ndim != 1 or int(out.shape[0]) < words:
            raise NativeError(E_INVALID, f"out must be a device tensor of at least {words} words")
        c = C.c_int64(0)
        Text.regex_calls += 1
        check(lib().crh_text_regex(self._handle(), n_states, n_classes, class_of.ctypes.data, int(dfa.end_class), trans.ctypes.data if trans.size else None,
                                   int(dfa.accept), _ptr(mask), _ptr(out), C.byref(c) if count else None, stream))
        return out, (int(c.value) if count else None)

    def fuzzy(self, pattern, edits: int, fold_case: bool = False, mask=None, out=None, count: bool = True, stream: int = 0):
        """Which rows hold the byte ``pattern`` within ``edits`` edits (``crh_text_fuzzy``): a row's distance is
        the least Levenshtein distance between the pattern and any substring of the row, counted in BYTES (insertion, deletion
        and substitution of one byte cost 1 each), and level ``d`` of the result holds the rows whose distance is at most
        ``d``.  ``fold_case`` folds ASCII letters only.  ``mask`` and ``stream`` as in :meth:`match`.  Returns ``(levels int32
        device tensor [edits + 1, ceil(rows / 32)], per-level counts as a list or None)``: the levels are nested, the last one
        is the filter's bitmap; with ``count`` the call waits on ``stream``.  It is the library that refuses a length outside
        1..64, ``edits`` outside 0..3 and a pattern not longer than ``edits``."""
        import torch
        data = np.frombuffer(bytes(pattern), dtype=np.uint8)
        edits = int(edits)
        words = (self.count()[0] + 31) // 32
        levels = edits + 1 if 0 <= edits <= FUZZY_MAX_EDITS else 1           # (an edits the library refuses allocates one level)
        if mask is not None:
            _typed(mask, "int32", "mask")
            if not _is_dev(mask) or int(mask.numel()) < words:
                raise NativeError(E_INVALID, "mask must be a device tensor of one word per 32-row tile")
        if out is None:
            out = torch.empty((levels, words), dtype=torch.int32, device=f"cuda:{self.device}")
        _typed(out, "int32", "out")
        if not _is_dev(out) or tuple(out.shape) != (levels, words) or not out.is_contiguous():
            raise NativeError(E_INVALID, f"out must be a contiguous device tensor of {levels} levels x {words} words")
        c = (C.c_int64 * (FUZZY_MAX_EDITS + 1))()
        Text.fuzzy_calls += 1
        check(lib().crh_text_fuzzy(self._handle(), data.ctypes.data if data.size else None, int(data.size), edits, int(bool(fold_case)),
                                   _ptr(mask), _ptr(out), c if count else None, stream))
        return out, ([int(v) for v in c[:levels]] if count else None)


def gather_rows_i32(rows, row_base: int, col, fill: int = 0, stream: int = 0):
    """``crh_gather_rows_i32``: ``out[i] = col[rows[i] - row_base]`` where this shard owns the row, ``fill`` elsewhere (padding
    too); ``rows`` an int64 device tensor of GLOBAL rows, ``col`` the shard's int32 device column.  int32, the shape of ``rows``."""
    import torch
    _typed(rows, "int64", "rows")
    _typed(col, "int32", "col")
    if not _is_dev(rows) or not _is_dev(col):
        raise NativeError(E_INVALID, "gather_rows_i32 takes device tensors")
    out = torch.empty(tuple(rows.shape), dtype=torch.int32, device=rows.device)
    use_device(rows.device.index)
    check(lib().crh_gather_rows_i32(int(rows.numel()), _ptr(rows), int(row_base), int(col.numel()), _ptr(col) if col.numel() else None, int(fill),
                                    _ptr(out), stream))
    return out


def graph_direction(direction) -> int:
    """``"callees"`` / ``"callers"`` / ``"both"`` (or the CRH_GRAPH_* number) as ``crh_graph_bfs`` takes it."""
    if isinstance(direction, str) and direction in GRAPH_DIRECTIONS:
        return GRAPH_DIRECTIONS[direction]
    if isinstance(direction, (int, np.integer)) and not isinstance(direction, bool) and int(direction) in GRAPH_DIRECTIONS.values():
        return int(direction)
    raise NativeError(E_INVALID, f"graph direction {direction!r} is not one of {sorted(GRAPH_DIRECTIONS)}")


def graph_sources(sources) -> tuple[np.ndarray, np.ndarray]:
    """Host source sets (an iterable of iterables of node ids) as the CSR ``crh_graph_bfs`` takes: (src_off int64 [nq + 1],
    src_nodes int32)."""
    sets = [np.asarray(list(s), np.int64).reshape(-1) for s in sources]
    off = np.zeros(len(sets) + 1, np.int64)
    np.cumsum([s.size for s in sets], out=off[1:])
    nodes = np.concatenate(sets).astype(np.int32) if sets and off[-1] else np.zeros((0,), np.int32)
    return off, nodes


class _GraphWorkspace:
    """What one BFS writes: levels u64 [hops + 1, n_nodes], seen [n_nodes], active [GRAPH_MAX_HOPS + 1] as int64 device tensors,
    and ``last``, the (nq, max_hops) of the bfs that wrote them."""

    def __init__(self):
        self.levels = self.seen = self.active = self.last = None


def _workspace_attr(back: bool, name: str):
    return property(lambda self: getattr(self._ws[back], name))


class Graph:
    """Owning wrapper of one ``crh_graph`` handle: up to ``GRAPH_MAX_RELATIONS`` relations over ``n_nodes``
    nodes, and the workspace of its traversals -- levels u64 [hops + 1, n_nodes], seen [n_nodes], active [GRAPH_MAX_HOPS + 1],
    held as int64 device tensors, sized by the first BFS that needs them.  A BFS overwrites the workspace: list, row_words and
    path read what the LAST bfs left unless they are handed tensors of their own."""
    bfs_calls = 0         # crh_graph_bfs calls issued by all handles (tests count the traversals of a job)
    scc_calls = 0         # crh_graph_scc calls likewise

    def __init__(self, n_nodes: int, device: int = 0):
        self.device, self.n_nodes = device, int(n_nodes)
        h = C.c_void_p()
        check(lib().crh_graph_create(device, int(n_nodes), C.byref(h)))
        self._h = h
        self._ws = (_GraphWorkspace(), _GraphWorkspace())   # [False]: the first workspace, [True]: the second, bfs(..., back=True)
        self.ppr_work = None  # f32 [4, n_nodes, QS]: p0, two contribution planes, the scores of the last ppr
        self.ppr_last = None  # (nq, QS) of the last ppr
        self.sigma_buf = None   # u64 [n_nodes, QS] as int64: the chain counts of the last sigma
        self.sigma_last = None  # (nq, max_hops, the tensor it wrote)

    levels, seen, active, last = (_workspace_attr(False, name) for name in ("levels", "seen", "active", "last"))
    levels_back, seen_back, active_back, last_back = (_workspace_attr(True, name) for name in ("levels", "seen", "active", "last"))

    def close(self) -> None:
        if getattr(self, "_h", None) and _lib is not None:
            _lib.crh_graph_destroy(self._h)
            self._h = None
            for ws in self._ws:
                ws.levels = ws.seen = ws.active = None
            self.ppr_work = self.sigma_buf = self.sigma_last = None

    __del__ = close

    def _handle(self):
        if not self._h:
            raise NativeError(E_INVALID, "graph handle is closed")
        return self._h

    def count(self, rel: int = 0) -> tuple[int, int]:
        """(nodes, edges of relation ``rel``; -1: not set)."""
        n, e = C.c_int64(0), C.c_int64(0)
        check(lib().crh_graph_count(self._handle(), int(rel), C.byref(n), C.byref(e)))
        return int(n.value), int(e.value)

    def set_relation(self, rel: int, off_fwd, adj_fwd, off_rev, adj_rev) -> None:
        """Relation ``rel`` from two host CSRs over the node ids (``graph.build_csr`` makes them); replaces what was there."""
        of, orv = (np.ascontiguousarray(o, dtype=np.int64).reshape(-1) for o in (off_fwd, off_rev))
        af, ar = (np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (adj_fwd, adj_rev))
        if of.size != self.n_nodes + 1 or orv.size != self.n_nodes + 1 or af.size != ar.size:
            raise NativeError(E_INVALID, f"set_relation: offsets of {of.size} / {orv.size} entries for {self.n_nodes} nodes, {af.size} / {ar.size} edges")
        check(lib().crh_graph_set_relation(self._handle(), int(rel), int(af.size), of.ctypes.data, af.ctypes.data if af.size else None,
                                           orv.ctypes.data, ar.ctypes.data if ar.size else None))

    def _grow(self, holder, name: str, rows: int, dtype, cols: tuple = ()):
        """The grow-only buffer ``holder.name``: kept while it has ``rows`` rows, else replaced by one of [rows, *cols]."""
        import torch
        have = getattr(holder, name)
        have = -1 if have is None else int(have.shape[0])
        if have < rows:
            setattr(holder, name, None)                                # (released before the larger one is taken: the peak is one buffer)
            setattr(holder, name, torch.empty((max(rows, 1),) + cols, dtype=dtype, device=f"cuda:{self.device}"))
        return getattr(holder, name)

    def _workspace(self, max_hops: int, back: bool = False) -> _GraphWorkspace:
        """The workspace a bfs writes, with ``max_hops + 1`` levels at least.  ``back``: the second one, for the
        search from the other end, which ``between`` reads beside the first."""
        import torch
        ws = self._ws[bool(back)]
        self._grow(ws, "levels", max_hops + 1, torch.int64, (self.n_nodes,))
        if ws.seen is None:
            ws.seen = torch.empty((self.n_nodes,), dtype=torch.int64, device=f"cuda:{self.device}")
            ws.active = torch.zeros((GRAPH_MAX_HOPS + 1,), dtype=torch.int64, device=f"cuda:{self.device}")
        return ws

    def bfs(self, rel: int, direction, sources, max_hops: int, include_self: bool = False, stream: int = 0, back: bool = False, avoid=None):
        """``crh_graph_bfs`` from up to ``GRAPH_MAX_QUERIES`` source sets: ``sources`` is an iterable of iterables of node ids
        (host), or an int32 device tensor [nq, k] whose rows are the sets (-1: padding), complete on ``stream``.  Returns
        ``(levels [max_hops + 1, n_nodes], seen [n_nodes], active [max_hops + 1])``: int64 device tensors holding the u64
        words, views of the handle's workspace.  Only enqueues.  ``back``: the search runs in the SECOND workspace and leaves
        the first (and what ``list`` / ``path`` / ``sigma`` read by default) alone.  ``avoid`` (:meth:`bfs_avoiding`): an
        int64 device tensor [n_nodes], bit q at v = query q never enters v."""
        max_hops = int(max_hops)
        on_dev = _is_dev(sources)
        if on_dev:
            _typed(sources, "int32", "sources")
            if sources.ndim != 2:
                raise NativeError(E_INVALID, "device sources must be an int32 tensor [nq, k]")
            nq, k = int(sources.shape[0]), int(sources.shape[1])
            off, nodes = np.arange(nq + 1, dtype=np.int64) * k, sources
        else:
            off, nodes = graph_sources(sources)
            nq = off.size - 1
        hops = max_hops if 1 <= max_hops <= GRAPH_MAX_HOPS else 1           # (a max_hops the library refuses allocates one level)
        ws = self._workspace(hops, back)
        levels, seen, active = ws.levels, ws.seen, ws.active
        Graph.bfs_calls += 1
        head = (self._handle(), int(rel), graph_direction(direction), nq, off.ctypes.data, _ptr(nodes) if int(off[-1]) else None, on_dev, max_hops,
                int(bool(include_self)))
        if avoid is None:
            check(lib().crh_graph_bfs(*head, _ptr(levels), _ptr(seen), _ptr(active), stream))
        else:
            self._node_array(avoid, "int64", "avoid")
            check(lib().crh_graph_bfs_avoiding(*head, _ptr(avoid), _ptr(levels), _ptr(seen), _ptr(active), stream))
        ws.last = (nq, max_hops)
        return levels[: max_hops + 1], seen, active[: max_hops + 1]

    # -- chains in full
    def _query_nodes(self, nodes) -> tuple[np.ndarray, bool]:
        """A host list of one node per query (-1: none) as int64 [len(nodes)], and whether it is at most ``GRAPH_MAX_QUERIES``
        nodes of this graph."""
        nodes = np.asarray(list(nodes), np.int64).reshape(-1)
        return nodes, nodes.size <= GRAPH_MAX_QUERIES and not (nodes.size and (nodes.min() < -1 or nodes.max() >= self.n_nodes))

    def avoid_words(self, nodes):
        """The ``avoid`` words of :meth:`bfs_avoiding` from one node per query (a host sequence, -1: the query avoids nothing):
        an int64 device tensor [n_nodes] with bit q set at ``nodes[q]``."""
        import torch
        nodes, ok = self._query_nodes(nodes)
        if not ok:
            raise NativeError(E_INVALID, f"avoid: at most {GRAPH_MAX_QUERIES} nodes of 0..{self.n_nodes - 1} (or -1)")
        dev = f"cuda:{self.device}"
        out = torch.zeros((self.n_nodes,), dtype=torch.int64, device=dev)
        keep = np.flatnonzero(nodes >= 0)
        if keep.size:
            bits = (np.uint64(1) << keep.astype(np.uint64)).view(np.int64)
            out.index_add_(0, torch.from_numpy(nodes[keep]).to(dev), torch.from_numpy(bits).to(dev))   # (distinct bits: the sum is the OR)
        return out

    def bfs_avoiding(self, rel: int, direction, sources, max_hops: int, avoid, include_self: bool = False, stream: int = 0, back: bool = False):
        """``crh_graph_bfs_avoiding``: :meth:`bfs` in which query q never enters the nodes whose ``avoid`` word carries bit q
        (an avoided source is no source).  ``avoid``: an int64 device tensor [n_nodes], or one node per query as
        :meth:`avoid_words` takes them."""
        if not _is_dev(avoid):
            avoid = self.avoid_words(avoid)
        return self.bfs(rel, direction, sources, max_hops, include_self=include_self, stream=stream, back=back, avoid=avoid)

    def seen_bits(self, nodes, seen=None) -> np.ndarray:
        """Bit q of ``seen[nodes[q]]`` per query q (host bool [len(nodes)]; False for -1): gathered on the device, so the host
        sees the finished bits only.  ``seen``: default the last :meth:`bfs`'s.  Waits for the device."""
        import torch
        nodes, ok = self._query_nodes(nodes)
        seen = self.seen if seen is None else seen
        if seen is None or not ok:
            raise NativeError(E_INVALID, f"seen_bits: a bfs first, then at most {GRAPH_MAX_QUERIES} nodes of 0..{self.n_nodes - 1} (or -1)")
        if not nodes.size or not self.n_nodes:
            return np.zeros((nodes.size,), bool)
        at = torch.from_numpy(np.maximum(nodes, 0)).to(seen.device)
        got = (seen.index_select(0, at) >> torch.arange(nodes.size, device=seen.device)) & 1
        return (got.cpu().numpy() != 0) & (nodes >= 0)

    def _levels_arg(self, levels, nq, max_hops, what: str, back: bool = False):
        """The levels a call reads, with their nq and max_hops: what the last bfs left in the workspace (``back``: the second),
        or ``levels`` of the caller's own, checked."""
        if levels is None:
            ws = self._ws[bool(back)]
            if ws.last is None:
                raise NativeError(E_INVALID, f"{what}: no bfs has run on this graph")
            levels = ws.levels
            nq = ws.last[0] if nq is None else nq
            max_hops = ws.last[1] if max_hops is None else max_hops
        if nq is None or max_hops is None:
            raise NativeError(E_INVALID, f"{what}: levels of its own need nq and max_hops")
        _typed(levels, "int64", "levels")
        hops = int(max_hops) if 1 <= int(max_hops) <= GRAPH_MAX_HOPS else 1   # (a max_hops the library refuses needs one level)
        if not _is_dev(levels) or levels.ndim != 2 or int(levels.shape[0]) < hops + 1 or int(levels.shape[1]) != self.n_nodes:
            raise NativeError(E_INVALID, f"levels must be a device tensor of at least {hops + 1} levels x {self.n_nodes} nodes")
        return levels, int(nq), int(max_hops)

    @staticmethod
    def _qs(nq: int) -> int:
        qs = 1
        while qs < min(max(nq, 1), GRAPH_MAX_QUERIES):
            qs *= 2
        return qs

    def sigma(self, rel: int, direction, nq: int | None = None, max_hops: int | None = None, levels=None, active=None, out=None, stream: int = 0):
        """``crh_graph_sigma`` over the last BFS (same ``rel`` and ``direction``, ``include_self=True``; or ``levels`` and
        ``active`` with ``nq`` and ``max_hops``): the number of SHORTEST chains from source set q to every node, saturating at
        ``GRAPH_SATURATED``.  Returns an int64 device tensor [n_nodes, QS] holding the u64 words (QS: the power of two >= nq;
        the columns from nq on are 0), the handle's own unless ``out`` is given.  Only enqueues."""
        import torch
        if (levels is None) != (active is None):
            raise NativeError(E_INVALID, "sigma: levels and active come together")
        active = self.active if active is None else active
        levels, nq, max_hops = self._levels_arg(levels, nq, max_hops, "sigma")
        _typed(active, "int64", "active")
        if not _is_dev(active) or int(active.numel()) < min(max(max_hops, 1), GRAPH_MAX_HOPS) + 1:
            raise NativeError(E_INVALID, "active must be a device tensor of max_hops + 1 words")
        qs = self._qs(nq)
        if out is None:
            out = self._grow(self, "sigma_buf", self.n_nodes * qs, torch.int64)[: self.n_nodes * qs].view(self.n_nodes, qs)
        _out(out, "int64", "out", (self.n_nodes, qs))
        check(lib().crh_graph_sigma(self._handle(), int(rel), graph_direction(direction), nq, _ptr(levels), _ptr(active), max_hops, _ptr(out), stream))
        self.sigma_last = (nq, max_hops, out)
        return out

    def chains(self, rel: int, direction, targets, k: int, nq: int | None = None, max_hops: int | None = None, levels=None, sigma=None, out=None,
               stream: int = 0):
        """``crh_graph_chains``: the ``k`` (1..``GRAPH_MAX_CHAINS``) first shortest chains of every query to its target, in the
        order of the node ids read backwards from the target.  ``targets``: one node per query, a host sequence (-1: none) or
        an int32 device tensor [nq].  ``sigma``: default the last :meth:`sigma`'s.  Returns device tensors ``(nodes int32 [nq,
        k, max_hops + 1]`` from a source to the target, padding -1, ``length int32 [nq]`` (0: not reached), ``count int64
        [nq])`` -- the u64 words: ``count.cpu().numpy().view(np.uint64)``; ``out``: three tensors to write instead."""
        import torch
        levels, nq, max_hops = self._levels_arg(levels, nq, max_hops, "chains")
        if sigma is None:
            if self.sigma_last is None:
                raise NativeError(E_INVALID, "chains: no sigma has run on this graph")
            sigma = self.sigma_last[2]
        _out(sigma, "int64", "sigma", (self.n_nodes, self._qs(nq)))
        on_dev = _is_dev(targets)
        if on_dev:
            _out(targets, "int32", "targets", (nq,))
        else:
            targets = np.ascontiguousarray(np.asarray(list(targets), np.int64).reshape(-1).astype(np.int32))
            if targets.size != nq:
                raise NativeError(E_INVALID, f"chains: {targets.size} targets for {nq} queries")
        kk = int(k) if 1 <= int(k) <= GRAPH_MAX_CHAINS else 1               # (a k the library refuses allocates one chain)
        hops = max_hops if 1 <= max_hops <= GRAPH_MAX_HOPS else 1
        dev = f"cuda:{self.device}"
        if out is None:
            out = (torch.empty((nq, kk, hops + 1), dtype=torch.int32, device=dev), torch.empty((nq,), dtype=torch.int32, device=dev),
                   torch.empty((nq,), dtype=torch.int64, device=dev))
            if self.n_nodes == 0:
                out[0].fill_(-1), out[1].zero_(), out[2].zero_()
        nodes, length, count = out
        _out(nodes, "int32", "out nodes", (nq, kk, hops + 1))
        _out(length, "int32", "out length", (nq,))
        _out(count, "int64", "out count", (nq,))
        for t in out:
            if not _is_dev(t):
                raise NativeError(E_INVALID, "chains: out takes device tensors")
        check(lib().crh_graph_chains(self._handle(), int(rel), graph_direction(direction), nq, _ptr(levels), _ptr(sigma), max_hops, _ptr(targets),
                                     on_dev, int(k), _ptr(nodes), _ptr(length), _ptr(count), stream))
        return nodes, length, count

    def between(self, levels_back=None, mode="any", nq: int | None = None, max_hops: int | None = None, levels=None, out=None, dist=None,
                stream: int = 0):
        """``crh_graph_between``: the nodes between the source sets of the last :meth:`bfs` and the target sets of the last
        ``bfs(..., back=True)`` in the opposite direction (both ``include_self=True``, the same ``max_hops``; or ``levels`` /
        ``levels_back`` with ``nq`` and ``max_hops``).  ``mode`` ``"any"``: on a WALK of at most ``max_hops`` edges from the one
        set to the other; ``"shortest"``: on a shortest chain.  Returns ``(words, dist)``: int64 ``seen``-style words [n_nodes]
        (bit q; :meth:`row_words` takes them as ``seen=``) and int32 [nq] = the distance of the sets, -1 where they do not
        meet.  Both are tensors of the call's own (``out`` / ``dist``: tensors to write): no level is overwritten."""
        import torch
        if mode not in GRAPH_BETWEEN and mode not in GRAPH_BETWEEN.values():
            raise NativeError(E_INVALID, f"between mode {mode!r} is not one of {sorted(GRAPH_BETWEEN)}")
        mode = GRAPH_BETWEEN.get(mode, mode)
        if levels is None and levels_back is None and self.last is not None and self.last_back is not None and self.last != self.last_back:
            raise NativeError(E_INVALID, f"between: the two searches ran with (nq, max_hops) = {self.last} and {self.last_back}")
        levels, nq, max_hops = self._levels_arg(levels, nq, max_hops, "between")
        levels_back, _, _ = self._levels_arg(levels_back, nq, max_hops, "between", back=True)
        dev = f"cuda:{self.device}"
        if out is None:
            out = torch.empty((self.n_nodes,), dtype=torch.int64, device=dev)
        self._node_array(out, "int64", "out")
        if dist is None:
            dist = torch.full((nq,), -1, dtype=torch.int32, device=dev)
        _out(dist, "int32", "dist", (nq,))
        if not _is_dev(dist):
            raise NativeError(E_INVALID, "between: dist takes a device tensor")
        meet = torch.empty((GRAPH_MAX_HOPS + 1,), dtype=torch.int64, device=dev)
        use_device(self.device)
        check(lib().crh_graph_between(self.n_nodes, nq, _ptr(levels), _ptr(levels_back), max_hops, int(mode), _ptr(meet), _ptr(out), _ptr(dist), stream))
        return out, dist

    def list(self, limit: int, first_level: int = 1, nq: int | None = None, max_hops: int | None = None, levels=None, stream: int = 0):
        """``crh_graph_list`` over the last BFS's levels (or ``levels``, with ``nq`` and ``max_hops``): ``(nodes int32 [nq, limit],
        depth int32 [nq, limit], count int64 [nq])`` device tensors; (depth, node id) order, padding -1, exact counts."""
        import torch
        levels, nq, max_hops = self._levels_arg(levels, nq, max_hops, "list")
        dev = f"cuda:{self.device}"
        lim = max(int(limit), 0)
        nodes = torch.empty((max(int(nq), 0), lim), dtype=torch.int32, device=dev)
        depth = torch.empty((max(int(nq), 0), lim), dtype=torch.int32, device=dev)
        count = torch.zeros((max(int(nq), 0),), dtype=torch.int64, device=dev)
        check(lib().crh_graph_list(self._handle(), int(nq), _ptr(levels), int(max_hops), int(first_level), int(limit), _ptr(nodes), _ptr(depth),
                                   _ptr(count), stream))
        return nodes, depth, count

    def row_words(self, row_node, q: int = 0, n_words: int | None = None, out=None, seen=None, stream: int = 0):
        """``crh_graph_row_words``: the rows whose node (``row_node`` int32 device tensor, -1: none) query ``q`` of the last BFS
        reached (``seen``: another seen tensor), as int32 validity words [``n_words``, default ceil(rows / 32)]."""
        import torch
        _typed(row_node, "int32", "row_node")
        if not _is_dev(row_node) or row_node.ndim != 1:
            raise NativeError(E_INVALID, "row_node must be a one-dimensional int32 device tensor")
        seen = self.seen if seen is None else seen
        if seen is None:
            raise NativeError(E_INVALID, "row_words: no bfs has run on this graph")
        _typed(seen, "int64", "seen")
        if not _is_dev(seen) or int(seen.numel()) < self.n_nodes:
            raise NativeError(E_INVALID, f"seen must be a device tensor of {self.n_nodes} words")
        rows = int(row_node.shape[0])
        words = (rows + 31) // 32 if n_words is None else int(n_words)
        if out is None:
            out = torch.empty((words,), dtype=torch.int32, device=f"cuda:{self.device}")
        _typed(out, "int32", "out")
        if not _is_dev(out) or out.ndim != 1 or int(out.shape[0]) < words:
            raise NativeError(E_INVALID, f"out must be a device tensor of at least {words} words")
        use_device(self.device)
        check(lib().crh_graph_row_words(_ptr(row_node) if rows else None, rows, _ptr(seen), self.n_nodes, int(q), _ptr(out), words, stream))
        return out

    def path(self, rel: int, direction, q: int, target: int, max_hops: int | None = None, levels=None, stream: int = 0) -> np.ndarray:
        """``crh_graph_path``: the nodes of one shortest path of query ``q`` of the last BFS (same ``rel`` and ``direction``) from
        a source to ``target``, int32; empty when the target was not reached.  Waits on ``stream``."""
        levels, _, max_hops = self._levels_arg(levels, None if levels is None else 0, max_hops, "path")   # (a path has no nq: 0 stands in beside levels of its own)
        out = np.full((GRAPH_MAX_HOPS + 1,), -1, np.int32)
        n = C.c_int(0)
        check(lib().crh_graph_path(self._handle(), int(rel), graph_direction(direction), _ptr(levels), int(q), int(target), int(max_hops),
                                   out.ctypes.data, C.byref(n), stream))
        return out[: int(n.value)].copy()

    # -- personalised PageRank
    def _ppr_workspace(self, qs: int):
        import torch
        return self._grow(self, "ppr_work", 4 * self.n_nodes * qs, torch.float32)   # p0, two contribution planes, the scores

    def ppr(self, rel: int, direction, seeds, weights=None, restart: float = 0.15, steps: int = 16, stream: int = 0):
        """``crh_graph_ppr``: personalised PageRank from up to ``GRAPH_MAX_QUERIES`` seed lists.  ``seeds`` is an iterable of
        iterables of node ids with ``weights`` alike (host; ``None``: every weight 1), or an int32 device tensor [nq, c] with an
        f32 device tensor [nq, c] (-1 / 0: padding), complete on ``stream``.  Returns the scores, f32 [n_nodes, nq]: a view of
        the handle's workspace that the next ``ppr`` overwrites.  Only enqueues."""
        on_dev = _is_dev(seeds)
        if on_dev:
            _typed(seeds, "int32", "seeds")
            if seeds.ndim != 2:
                raise NativeError(E_INVALID, "device seeds must be an int32 tensor [nq, c]")
            nq, c = int(seeds.shape[0]), int(seeds.shape[1])
            if weights is not None:
                if not _is_dev(weights):
                    raise NativeError(E_INVALID, "device seeds take device weights")
                _out(weights, "float32", "weights", (nq, c))
            nodes, w = seeds, weights
        else:
            sets = [np.asarray(list(s), np.int64).reshape(-1) for s in seeds]
            nq, c = len(sets), max([int(s.size) for s in sets] + [1])
            nodes = np.full((nq, c), -1, np.int32)
            for q, s in enumerate(sets):
                nodes[q, : s.size] = s
            w = None
            if weights is not None:
                w = np.zeros((nq, c), np.float32)
                given = [np.asarray(list(x), np.float32).reshape(-1) for x in weights]
                if [int(x.size) for x in given] != [int(s.size) for s in sets]:
                    raise NativeError(E_INVALID, "ppr: weights must have the shape of seeds")
                for q, x in enumerate(given):
                    w[q, : x.size] = x
        qs = self._qs(nq)
        work = self._ppr_workspace(qs)
        plane = self.n_nodes * qs
        check(lib().crh_graph_ppr(self._handle(), int(rel), graph_direction(direction), nq, c, _ptr(nodes), _ptr(w), on_dev, float(restart),
                                  int(steps), _ptr(work), _ptr(work) + 12 * plane, stream))
        self.ppr_last = (nq, qs)
        return work[3 * plane: 4 * plane].view(self.n_nodes, qs)[:, :nq]

    def _ppr_state(self, what: str):
        if self.ppr_last is None:
            raise NativeError(E_INVALID, f"{what}: no ppr has run on this graph")
        nq, qs = self.ppr_last
        plane = self.n_nodes * qs
        return nq, self.ppr_work[3 * plane: 4 * plane]

    def ppr_top(self, k: int, exclude=None, stream: int = 0):
        """The top ``k`` nodes of the last ``ppr`` per query: ``crh_graph_ppr_bins`` (``exclude``: an int32 device tensor [nq, c]
        of nodes to leave out, -1: padding) and ``crh_facet_select``.  Returns device tensors ``(nodes int32 [nq, k], scores f32
        [nq, k])`` by descending score, ties to the lower node id, a zero score never returned; the tail is ``(-1, 0)``."""
        import torch
        nq, scores = self._ppr_state("ppr_top")
        c = 0
        if exclude is not None:
            _typed(exclude, "int32", "exclude")
            if not _is_dev(exclude) or exclude.ndim != 2 or int(exclude.shape[0]) != nq:
                raise NativeError(E_INVALID, f"exclude must be an int32 device tensor [{nq}, c]")
            c = int(exclude.shape[1])
        bins = torch.empty((nq, max(self.n_nodes, 1)), dtype=torch.int64, device=f"cuda:{self.device}")
        if self.n_nodes == 0:
            bins.zero_()
        use_device(self.device)
        check(lib().crh_graph_ppr_bins(self.n_nodes, nq, _ptr(scores), c, _ptr(exclude) if c else None, _ptr(bins), stream))
        codes, counts, _ = facet_select(bins, k, stream)
        return codes, counts.to(torch.int32).view(torch.float32)

    def ppr_order(self, rows, cosine, nodes, stream: int = 0):
        """``crh_graph_ppr_order`` over the last ``ppr``: a candidate table (``rows`` int64, ``cosine`` f32, ``nodes`` int32, each
        a device tensor [nq, c]) as ``(scores f32 [nq, 2, c], rows int64 [nq, 2, c], graph_score f32 [nq, c])`` -- the two lists
        ``fuse_select(scores, rows, 2, k)`` takes (the table itself; its candidates with a positive graph score by descending
        graph score, ties to the earlier position) and every candidate's graph score."""
        import torch
        nq, scores = self._ppr_state("ppr_order")
        for x, what in ((rows, "rows"), (cosine, "cosine"), (nodes, "nodes")):
            if not _is_dev(x):
                raise NativeError(E_INVALID, f"{what} must be a device tensor")
        if rows.ndim != 2 or int(rows.shape[0]) != nq:
            raise NativeError(E_INVALID, f"rows must be [{nq}, c]")
        c = int(rows.shape[1])
        _typed(rows, "int64", "rows")
        _out(cosine, "float32", "cosine", (nq, c))
        _out(nodes, "int32", "nodes", (nq, c))
        dev = f"cuda:{self.device}"
        fs = torch.empty((nq, 2, c), dtype=torch.float32, device=dev)
        fr = torch.empty((nq, 2, c), dtype=torch.int64, device=dev)
        gs = torch.empty((nq, c), dtype=torch.float32, device=dev)
        use_device(self.device)
        check(lib().crh_graph_ppr_order(self.n_nodes, nq, c, _ptr(scores), _ptr(rows), _ptr(cosine), _ptr(nodes), _ptr(fs), _ptr(fr), _ptr(gs), stream))
        return fs, fr, gs

    # -- components and layers
    def _node_array(self, x, want: str, what: str):
        _typed(x, want, what)
        if not _is_dev(x) or x.ndim != 1 or int(x.shape[0]) != self.n_nodes:
            raise NativeError(E_INVALID, f"{what} must be a {want} device tensor of {self.n_nodes} entries")
        return x

    def scc(self, rel: int, stream: int = 0):
        """``crh_graph_scc``: ``(comp, info)`` -- ``comp`` an int32 device tensor [n_nodes] of its own, ``comp[v]`` = the smallest
        node id of v's strongly connected component in relation ``rel``; ``info`` a host int64 [4] = (components, components of
        two nodes or more, nodes in those, sweeps launched).  Waits on ``stream``."""
        import torch
        dev = f"cuda:{self.device}"
        comp = torch.empty((self.n_nodes,), dtype=torch.int32, device=dev)
        work = torch.empty((self.n_nodes + GRAPH_SCC_WORK_EXTRA,), dtype=torch.int32, device=dev)
        info = np.zeros((4,), np.int64)
        Graph.scc_calls += 1
        check(lib().crh_graph_scc(self._handle(), int(rel), _ptr(comp), _ptr(work), info.ctypes.data, stream))
        return comp, info

    def scc_bins(self, comp, self_nodes=None, stream: int = 0):
        """``crh_graph_scc_bins``: int64 device tensor [n_nodes], ``bins[c]`` = the size of component ``c`` when it is cyclic (two
        nodes or more, or one node that is in ``self_nodes``: a sorted, distinct int32 host array or device tensor of the nodes
        with a self-loop), 0 otherwise.  ``facet_select(bins, k)`` then lists the largest cyclic components."""
        import torch
        self._node_array(comp, "int32", "comp")
        dev = f"cuda:{self.device}"
        n_self = 0
        if self_nodes is not None:
            if not _is_dev(self_nodes):
                self_nodes = torch.from_numpy(np.ascontiguousarray(self_nodes, dtype=np.int32).reshape(-1)).to(dev)
            _typed(self_nodes, "int32", "self_nodes")
            n_self = int(self_nodes.numel())
        bins = torch.empty((self.n_nodes,), dtype=torch.int64, device=dev)
        use_device(self.device)
        check(lib().crh_graph_scc_bins(self.n_nodes, _ptr(comp), _ptr(self_nodes) if n_self else None, n_self, _ptr(bins), stream))
        return bins

    def layers(self, rel: int, direction, comp, stream: int = 0):
        """``crh_graph_layers``: ``(layer, info)`` -- ``layer`` an int32 device tensor [n_nodes], the longest-path layer of every
        node's component in the condensation, travelling ``"callees"`` (along the edges: the DEPTH below the entry points) or
        ``"callers"`` (against them: the HEIGHT above the leaves); ``info`` a host int64 [2] = (layers, sweeps launched).  Waits
        on ``stream``."""
        import torch
        self._node_array(comp, "int32", "comp")
        dev = f"cuda:{self.device}"
        out = torch.empty((self.n_nodes,), dtype=torch.int32, device=dev)
        work = torch.empty((GRAPH_SCC_WORK_EXTRA,), dtype=torch.int32, device=dev)
        info = np.zeros((2,), np.int64)
        check(lib().crh_graph_layers(self._handle(), int(rel), graph_direction(direction), _ptr(comp), _ptr(out), _ptr(work), info.ctypes.data, stream))
        return out, info

    def node_words(self, mode, values, bins=None, lo: int = 0, hi: int = 0, q: int = 0, out=None, stream: int = 0):
        """``crh_graph_node_words``: a condition on every node as int64 ``seen`` words [n_nodes] (bit ``q`` where it holds), which
        :meth:`row_words` takes as ``seen=``.  ``mode`` ``"in_cycle"`` (``values`` = components, ``bins`` = :meth:`scc_bins`),
        ``"same_component"`` (``values`` = components, ``lo`` = a label) or ``"range"`` (``lo <= values[v] <= hi``)."""
        import torch
        if mode not in GRAPH_WORDS and mode not in GRAPH_WORDS.values():
            raise NativeError(E_INVALID, f"node_words mode {mode!r} is not one of {sorted(GRAPH_WORDS)}")
        mode = GRAPH_WORDS.get(mode, mode)
        self._node_array(values, "int32", "values")
        if bins is not None:
            self._node_array(bins, "int64", "bins")
        if out is None:
            out = torch.empty((self.n_nodes,), dtype=torch.int64, device=f"cuda:{self.device}")
        self._node_array(out, "int64", "out")
        use_device(self.device)
        check(lib().crh_graph_node_words(self.n_nodes, int(mode), _ptr(values), _ptr(bins), int(lo), int(hi), int(q), _ptr(out), stream))
        return out


def _list_stride(x, want: str, what: str, nl: int, nq: int, k: int) -> int:
    """[nl, nq, k] device tensor whose lists are contiguous but may lie apart (views into one gathered buffer)."""
    if str(x.dtype).rsplit(".", 1)[-1] != want:
        raise NativeError(E_INVALID, f"{what} must be {want}, got {x.dtype}")
    if tuple(x.shape) != (nl, nq, k) or (nq * k > 1 and (x.stride(2) != 1 or (nq > 1 and x.stride(1) != k))):
        raise NativeError(E_INVALID, f"{what} must be [nlists, nq, k] with contiguous lists, got shape {tuple(x.shape)} strides {tuple(x.stride())}")
    return int(x.stride(0)) if nl > 1 else nq * k


def merge_topk(scores, rows, out_scores, out_rows, stream: int = 0) -> None:
    """scores/rows: CUDA tensors [nlists, nq, k] (f32 / i64), each list contiguous; out_*: [nq, k]."""
    nl, nq, k = (int(v) for v in scores.shape)
    use_device(scores.device.index)
    ss = _list_stride(scores, "float32", "scores", nl, nq, k)
    rs = _list_stride(rows, "int64", "rows", nl, nq, k)
    _out(out_scores, "float32", "out_scores", (nq, k))
    _out(out_rows, "int64", "out_rows", (nq, k))
    check(lib().crh_merge_topk_strided(nl, nq, k, _ptr(scores), _ptr(rows), ss, rs, _ptr(out_scores), _ptr(out_rows), stream))


def mmr_select(scores, rows, vecs, k: int, diversity: float, out_pos=None, out_rows=None, out_scores=None, out_obj=None, stream: int = 0):
    """Greedy maximal-marginal-relevance picks (``crh_mmr_select``) over candidate lists left on the device: ``scores`` f32 /
    ``rows`` i64 [nq, c] as a search or merge returns them, ``vecs`` f32 [nq, c, dim] the candidates' stored vectors.  Returns
    ``(pos i32, rows i64, scores f32, obj f32)``, each [nq, k], CUDA tensors (given or allocated); enqueues only."""
    import torch
    for x, what in ((scores, "scores"), (rows, "rows"), (vecs, "vecs")):
        if not _is_dev(x):
            raise NativeError(E_INVALID, f"{what} must be a device tensor")
    if scores.ndim != 2 or vecs.ndim != 3:
        raise NativeError(E_INVALID, "scores must be [nq, c] and vecs [nq, c, dim]")
    nq, c = (int(v) for v in scores.shape)
    dim = int(vecs.shape[2])
    _typed(scores, "float32", "scores")
    _out(rows, "int64", "rows", (nq, c))
    _out(vecs, "float32", "vecs", (nq, c, dim))
    k = int(k)
    outs = []
    for x, want, what in ((out_pos, "int32", "out_pos"), (out_rows, "int64", "out_rows"), (out_scores, "float32", "out_scores"),
                          (out_obj, "float32", "out_obj")):
        if x is None:
            x = torch.empty((nq, max(k, 0)), dtype=getattr(torch, want), device=scores.device)
        else:
            _out(x, want, what, (nq, k))
            if not _is_dev(x):
                raise NativeError(E_INVALID, f"{what} must be a device tensor")
        outs.append(x)
    use_device(scores.device.index)
    check(lib().crh_mmr_select(nq, c, k, dim, _ptr(scores), _ptr(rows), _ptr(vecs), float(diversity), *(_ptr(x) for x in outs), stream))
    return tuple(outs)


def group_select(scores, rows, codes, k: int, group_size: int, stream: int = 0):
    """The capped walk (``crh_group_select``) over candidate lists left on the device: ``scores`` f32 / ``rows`` i64 [nq, c]
    as a search or merge returns them, ``codes`` i32 [nq, c] the candidates' codes in the group_by column
    (:meth:`Index.gather_codes`).  Returns CUDA tensors ``(pos i32, rows i64, scores f32, codes i32)``, each [nq, k] -- the
    first ``k`` candidates whose rank in their group is below ``group_size``, in list order, tail ``(-1, -1, -inf, -1)`` -- and
    ``info`` i32 [nq, 2] = (kept in the whole list, real candidates).  Enqueues only."""
    import torch
    for x, what in ((scores, "scores"), (rows, "rows"), (codes, "codes")):
        if not _is_dev(x):
            raise NativeError(E_INVALID, f"{what} must be a device tensor")
    if scores.ndim != 2:
        raise NativeError(E_INVALID, "scores must be [nq, c]")
    nq, c = (int(v) for v in scores.shape)
    _typed(scores, "float32", "scores")
    _out(rows, "int64", "rows", (nq, c))
    _out(codes, "int32", "codes", (nq, c))
    k = int(k)
    dev = scores.device
    outs = tuple(torch.empty((nq, max(k, 0)), dtype=dt, device=dev) for dt in (torch.int32, torch.int64, torch.float32, torch.int32))
    info = torch.empty((nq, 2), dtype=torch.int32, device=dev)
    use_device(dev.index)
    check(lib().crh_group_select(nq, c, k, int(group_size), _ptr(scores), _ptr(rows), _ptr(codes), *(_ptr(x) for x in outs), _ptr(info), stream))
    return outs + (info,)


def facet_select(bins, k: int, stream: int = 0):
    """The facet list (``crh_facet_select``) of histograms left on the device: ``bins`` int64 ``[nq, n_bins]`` (or ``[n_bins]``:
    one list), counts ``>= 0``.  Returns CUDA tensors ``(codes i32, counts i64)``, each ``[nq, k]`` -- the bins with count > 0 by
    count descending, ties to the lower code, tail ``(-1, 0)`` -- and ``info`` i64 ``[nq, 2]`` = (bins with count > 0, sum of
    the bins).  Enqueues only."""
    import torch
    if not _is_dev(bins):
        raise NativeError(E_INVALID, "bins must be a device tensor")
    _typed(bins, "int64", "bins")
    if bins.ndim == 1:
        bins = bins[None, :]
    if bins.ndim != 2:
        raise NativeError(E_INVALID, "bins must be [nq, n_bins]")
    nq, n_bins = (int(v) for v in bins.shape)
    k = int(k)
    dev = bins.device
    codes = torch.empty((nq, max(k, 0)), dtype=torch.int32, device=dev)
    counts = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=dev)
    info = torch.empty((nq, 2), dtype=torch.int64, device=dev)
    use_device(dev.index)
    check(lib().crh_facet_select(nq, n_bins, k, _ptr(bins), _ptr(codes), _ptr(counts), _ptr(info), stream))
    return codes, counts, info


def span_select(scores, rows, file_codes, lo, hi, k: int, max_overlap_permille: int, stream: int = 0):
    """The overlap-free walk (``crh_span_select``) over candidate lists left on the device: ``scores`` f32 /
    ``rows`` i64 [nq, c] as a search or merge returns them, ``file_codes`` / ``lo`` / ``hi`` i32 [nq, c] the candidates' file
    code, first and last line (:meth:`Index.gather_codes` over buffers full of -1).  Returns CUDA tensors ``(pos i32, rows i64,
    scores f32, file i32, lo i32, hi i32)``, each [nq, k] -- the first ``k`` candidates that repeat at most
    ``max_overlap_permille`` thousandths of the shorter span of any better kept hit of their file, in list order, tail
    ``(-1, -1, -inf, -1, -1, -1)`` -- and ``info`` i32 [nq, 2] = (kept in the whole list, real candidates).  Enqueues only."""
    import torch
    for x, what in ((scores, "scores"), (rows, "rows"), (file_codes, "file_codes"), (lo, "lo"), (hi, "hi")):
        if not _is_dev(x):
            raise NativeError(E_INVALID, f"{what} must be a device tensor")
    if scores.ndim != 2:
        raise NativeError(E_INVALID, "scores must be [nq, c]")
    nq, c = (int(v) for v in scores.shape)
    _typed(scores, "float32", "scores")
    _out(rows, "int64", "rows", (nq, c))
    for x, what in ((file_codes, "file_codes"), (lo, "lo"), (hi, "hi")):
        _out(x, "int32", what, (nq, c))
    k = int(k)
    dev = scores.device
    outs = tuple(torch.empty((nq, max(k, 0)), dtype=dt, device=dev)
                 for dt in (torch.int32, torch.int64, torch.float32, torch.int32, torch.int32, torch.int32))
    info = torch.empty((nq, 2), dtype=torch.int32, device=dev)
    use_device(dev.index)
    check(lib().crh_span_select(nq, c, k, int(max_overlap_permille), _ptr(scores), _ptr(rows), _ptr(file_codes), _ptr(lo), _ptr(hi),
                                *(_ptr(x) for x in outs), _ptr(info), stream))
    return outs + (info,)


def fuse_method(method) -> int:
    """``"rrf"`` / ``"max"`` -> CRH_FUSE_*; ``ValueError`` for anything else."""
    if not isinstance(method, str) or method.lower() not in FUSE_METHODS:
        raise ValueError(f"unknown fusion {method!r} (one of {sorted(FUSE_METHODS)})")
    return FUSE_METHODS[method.lower()]


def fuse_weights(weights, m: int, method: int):
    """Checked f32 [m] weights of one fused call (``None`` stays ``None``: every list weighs 1); ``ValueError`` otherwise."""
    if weights is None:
        return None
    if method != FUSE_RRF:
        raise ValueError("weights are only meaningful with fusion 'rrf'")
    w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    if w.size != m or not np.isfinite(w).all() or (w < 0).any():
        raise ValueError(f"weights must be {m} finite values >= 0, got {np.asarray(weights).tolist()}")
    return w


def fuse_select(scores, rows, m: int, k: int, method: str = "rrf", rrf_k: int = 60, weights=None, stream: int = 0):
    """Multi-query fusion (``crh_fuse_select``) over candidate lists left on the device: ``scores`` f32 /
    ``rows`` i64 ``[nq * m, c]`` or ``[nq, m, c]`` as a search or merge returns them -- the ``m`` lists of one logical query
    next to each other.  Returns CUDA tensors ``(rows i64, fused f32, cos f32, lists i32, first i32)``, each [nq, k] -- the
    first ``k`` distinct rows by descending fused score, ties to the lower row, tail ``(-1, -inf, -inf, 0, -1)`` -- and
    ``info`` i32 [nq, 2] = (distinct rows, real entries).  Enqueues only."""
    import torch
    for x, what in ((scores, "scores"), (rows, "rows")):
        if not _is_dev(x):
            raise NativeError(E_INVALID, f"{what} must be a device tensor")
    m = int(m)
    if scores.ndim == 3:
        if int(scores.shape[1]) != m:
            raise NativeError(E_INVALID, f"scores is [nq, {int(scores.shape[1])}, c] but m = {m}")
        flat = (int(scores.shape[0]) * m, int(scores.shape[2]))
    elif scores.ndim == 2:
        flat = tuple(int(v) for v in scores.shape)
    else:
        raise NativeError(E_INVALID, "scores must be [nq * m, c] or [nq, m, c]")
    if m < 1 or flat[0] % m:
        raise NativeError(E_INVALID, f"{flat[0]} lists are not whole sets of m = {m}")
    nq, c = flat[0] // m, flat[1]
    _typed(scores, "float32", "scores")
    _out(rows, "int64", "rows", tuple(scores.shape))
    k = int(k)
    code = fuse_method(method)
    w = fuse_weights(weights, m, code)
    dev = scores.device
    outs = tuple(torch.empty((nq, max(k, 0)), dtype=dt, device=dev) for dt in (torch.int64, torch.float32, torch.float32, torch.int32, torch.int32))
    info = torch.empty((nq, 2), dtype=torch.int32, device=dev)
    use_device(dev.index)
    check(lib().crh_fuse_select(nq, m, c, k, code, int(rrf_k), _ptr(w), _ptr(scores), _ptr(rows), *(_ptr(x) for x in outs), _ptr(info), stream))
    return outs + (info,)


def recommend_strategy(strategy) -> int:
    """``"average"`` / ``"best"`` -> CRH_RECOMMEND_*; ``ValueError`` for anything else."""
    if not isinstance(strategy, str) or strategy.lower() not in RECOMMEND_STRATEGIES:
        raise ValueError(f"unknown strategy {strategy!r} (one of {sorted(RECOMMEND_STRATEGIES)})")
    return RECOMMEND_STRATEGIES[strategy.lower()]


def _recommend_counts(n_pos, n_neg, nq: int):
    """The ragged sets' live counts as host int32 [nq] arrays (``None`` stays ``None``: every slot is live)."""
    out = []
    for x, what in ((n_pos, "n_pos"), (n_neg, "n_neg")):
        if x is not None:
            x = np.ascontiguousarray(x, dtype=np.int32).reshape(-1)
            if x.size != nq:
                raise NativeError(E_INVALID, f"{what} has {x.size} entries for {nq} queries")
        out.append(x)
    return out


def recommend_query(examples, P: int, N: int, n_pos=None, n_neg=None, stream: int = 0):
    """The "average" query of every example set (``crh_recommend_query``): ``examples`` f32 CUDA tensor
    ``[nq, P + N, dim]`` -- stored rows as :meth:`Index.gather_vectors` returns them, positives first; ``n_pos`` / ``n_neg``
    (host int [nq] or ``None``) the live counts of ragged sets.  Returns a CUDA tensor f32 ``[nq, dim]``; enqueues only."""
    import torch
    if not _is_dev(examples):
        raise NativeError(E_INVALID, "examples must be a device tensor")
    P, N = int(P), int(N)
    if examples.ndim != 3 or int(examples.shape[1]) != P + N:
        raise NativeError(E_INVALID, f"examples must be [nq, P + N = {P + N}, dim], got shape {tuple(examples.shape)}")
    _typed(examples, "float32", "examples")
    nq, dim = int(examples.shape[0]), int(examples.shape[2])
    n_pos, n_neg = _recommend_counts(n_pos, n_neg, nq)
    out = torch.empty((nq, dim), dtype=torch.float32, device=examples.device)
    use_device(examples.device.index)
    check(lib().crh_recommend_query(nq, P, N, dim, _ptr(examples), _ptr(n_pos), _ptr(n_neg), _ptr(out), stream))
    return out


def recommend_select(scores, rows, cand_vecs, examples, example_rows, P: int, N: int, k: int, strategy: str = "best", bf16: bool = False,
                     n_pos=None, n_neg=None, stream: int = 0):
    """The recommend selection (``crh_recommend_select``) over candidate lists left on the device.  ``"best"``:
    ``scores`` f32 / ``rows`` i64 ``[nq, P, c]`` the exact top-``c`` lists of the positives, ``cand_vecs`` f32 ``[nq, P * c, dim]``
    the candidates' stored vectors, ``examples`` f32 ``[nq, P + N, dim]`` the raw examples, ``example_rows`` i64 ``[nq, P + N]``
    their rows (-1: unused slot), ``bf16`` whether the store rounds its queries to bf16.  ``"average"``: ``[nq, 1, c]`` lists of
    the average query; ``cand_vecs`` / ``examples`` may be ``None``.  Returns CUDA tensors ``(rows i64, score f32, neg f32, best
    i32)``, each [nq, k] -- the first ``k`` kept rows by descending score, ties to the lower row, tail ``(-1, -inf, -inf, -1)``
    -- and ``info`` i32 [nq, 4] = (kept, settled, distinct, vetoed).  Enqueues only."""
    import torch
    code = recommend_strategy(strategy)
    for x, what in ((scores, "scores"), (rows, "rows"), (example_rows, "example_rows")) + (((cand_vecs, "cand_vecs"), (examples, "examples")) if code else ()):
        if not _is_dev(x):
            raise NativeError(E_INVALID, f"{what} must be a device tensor")
    P, N, k = int(P), int(N), int(k)
    m = P if code == RECOMMEND_BEST else 1
    if scores.ndim != 3 or int(scores.shape[1]) != m:
        raise NativeError(E_INVALID, f"scores must be [nq, {m}, c], got shape {tuple(scores.shape)}")
    nq, c = int(scores.shape[0]), int(scores.shape[2])
    _typed(scores, "float32", "scores")
    _out(rows, "int64", "rows", (nq, m, c))
    _out(example_rows, "int64", "example_rows", (nq, P + N))
    if code == RECOMMEND_BEST:
        if examples.ndim != 3:
            raise NativeError(E_INVALID, "examples must be [nq, P + N, dim]")
        dim = int(examples.shape[2])
        _out(examples, "float32", "examples", (nq, P + N, dim))
        _out(cand_vecs, "float32", "cand_vecs", (nq, m * c, dim))
    else:
        dim, cand_vecs, examples = 384, None, None        # (not read)
    n_pos, n_neg = _recommend_counts(n_pos, n_neg, nq)
    dev = scores.device
    outs = tuple(torch.empty((nq, max(k, 0)), dtype=dt, device=dev) for dt in (torch.int64, torch.float32, torch.float32, torch.int32))
    info = torch.empty((nq, 4), dtype=torch.int32, device=dev)
    use_device(dev.index)
    check(lib().crh_recommend_select(nq, P, N, c, k, dim, code, int(bool(bf16)), _ptr(scores), _ptr(rows), _ptr(cand_vecs), _ptr(examples),
                                     _ptr(example_rows), _ptr(n_pos), _ptr(n_neg), *(_ptr(x) for x in outs), _ptr(info), stream))
    return outs + (info,)


def topk_exchange_buffers(torch, world: int, nq: int, k: int, device):
    """Buffers for the cross-shard exchange with ONE collective: every rank's record is [scores f32 nq*k | rows i64 nq*k]
    (the score block padded to 8 bytes), so a single all-gather of ``local`` into ``gathered`` moves both, and the views
    ``all_scores`` / ``all_rows`` ([world, nq, k], lists contiguous, ranks one record apart) feed merge_topk as they are.
    Returns (local, loc_scores, loc_rows, gathered, all_scores, all_rows)."""
    nb_s = (nq * k * 4 + 7) // 8 * 8
    nb = nb_s + nq * k * 8
    local = torch.empty((nb,), dtype=torch.uint8, device=device)
    gathered = torch.empty((world, nb), dtype=torch.uint8, device=device)
    loc_s = local[: nq * k * 4].view(torch.float32).view(nq, k)
    loc_r = local[nb_s:].view(torch.int64).view(nq, k)
    all_s = gathered[:, : nq * k * 4].view(torch.float32).unflatten(1, (nq, k))
    all_r = gathered[:, nb_s:].view(torch.int64).unflatten(1, (nq, k))
    return local, loc_s, loc_r, gathered, all_s, all_r
