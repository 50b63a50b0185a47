"""HipVectorStore -- the reference's ``QdrantManager`` surface on an HBM-resident HIP index.

Drop-in for ``src/lattice/embeddings/client.py:18-228`` (and the ``VectorStore`` protocol of
``src/lattice/core/protocols.py:34-53``): same method names, argument meaning, return shapes and
error behaviour, but the vectors live in this process's GPU instead of a Qdrant server and the
cosine top-k runs in ``libcoderag_hip.so`` (``crh_search``).  Payload dictionaries, point ids and
the value<->code dictionaries of the filterable payload keys stay on the host; the device only
sees int32 codes.

There is no CPU fallback: without the native library or a gfx950 device ``connect()`` raises
``VectorStoreError``.
"""

from __future__ import annotations

import asyncio
import math
import os
import re
import logging
import threading
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from enum import Enum
from collections.abc import Mapping
from typing import Any, NamedTuple

import numpy as np

from . import ffi, graph as graph_mod, lexical, regex_dfa
from .errors import VectorStoreError
from .settings import get_settings
from .shards import STRIDE as SHARD_STRIDE, AppendFailed, ShardSet, split_global
from .tables import DICT_KEYS, NONE as NONE_CODE, TEXT_KEYS as _TEXT_COLUMNS, IdTable, PayloadTable

logger = logging.getLogger(__name__)


class CollectionName(str, Enum):
    """embeddings/client.py:13-15"""

    CODE_CHUNKS = "code_chunks"
    SUMMARIES = "summaries"


# Payload keys that can appear in a filter, per collection.  The first group mirrors the keyword payload
# indexes the reference creates (client.py:77-89); the rest are keys its callers filter on without an index
# (entity_name: query/context/builder.py:111-119; project_name on summaries: query/vector_search.py:144-146).
FILTER_KEYS: dict[str, tuple[str, ...]] = {
    CollectionName.CODE_CHUNKS.value: ("file_path", "entity_type", "language", "content_hash", "project_name",
                                       "entity_name"),
    CollectionName.SUMMARIES.value: ("file_path", "entity_type", "entity_name", "project_name"),
}

# Payload keys whose VALUE (a line number) the device holds beside the dictionary codes: range conditions compare them, the
# overlap-free walk (``max_overlap``) reads them.  Stored behind the columns of FILTER_KEYS, -1 = no usable value.
NUMERIC_KEYS: dict[str, tuple[str, ...]] = {
    CollectionName.CODE_CHUNKS.value: ("start_line", "end_line"),
    CollectionName.SUMMARIES.value: (),
}
_RANGE_WORDS = ("gte", "gt", "lte", "lt")
# Payload keys whose TEXT can be filtered by literal substring (``{"contains": ...}``): Qdrant's
# ``FieldCondition(key, match=MatchText(text))`` on a field without a full-text index.  Matched on the device by ``crh_text_match``
# over an arena derived from the payload tables on first use; never a device column, never part of a snapshot.
TEXT_KEYS: dict[str, tuple[str, ...]] = {
    CollectionName.CODE_CHUNKS.value: ("content",),
    CollectionName.SUMMARIES.value: ("summary",),
}
# "matches": a regular expression; "fuzzy" / "edits": a string within so many byte edits
_TEXT_WORDS = ("contains", "matches", "fuzzy", "edits", "any", "case")
_TEXT_KINDS = ("contains", "matches", "fuzzy")            # a text filter carries at least one of these
_ASCII_LOWER = bytes(c + 32 if 65 <= c <= 90 else c for c in range(256))   # the device's folding: ASCII letters only
_FUZZY_MIN_PIECE = 3     # the pigeonhole prefilter of an approximate match runs when its shortest piece has at least so many bytes
_TEXT_CACHE = 8          # match results a collection keeps (a repeated query under the same text filter does not grep again)


def range_bounds(key: str, spec) -> tuple[int, int]:
    """Qdrant's ``Range(gte, gt, lte, lt)`` -- a mapping or an object with those attributes -- as inclusive integer bounds
    ``(lo, hi)`` over non-negative ints: ``gt v`` is ``floor(v) + 1``, ``gte v`` ``ceil(v)``, ``lt v`` ``ceil(v) - 1``, ``lte v``
    ``floor(v)``; a missing (or None) end is open (0 below, ``ffi.VALUE_MAX`` above); ``lo > hi`` is an empty range.
    ``ValueError`` naming ``key`` for an unknown word or a bound that is no finite-or-infinite number."""
    if isinstance(spec, Mapping):
        unknown = [w for w in spec if w not in _RANGE_WORDS]
        if unknown:
            raise ValueError(f"range on {key!r}: unknown bound {unknown[0]!r} (use {', '.join(_RANGE_WORDS)})")
        get = spec.get
    else:
        get = lambda w: getattr(spec, w, None)   # noqa: E731
    lo, hi = 0, ffi.VALUE_MAX
    for word in _RANGE_WORDS:
        v = get(word)
        if v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or v != v:
            raise ValueError(f"range on {key!r}: {word}={v!r} is not a number")
        if v in (math.inf, -math.inf):
            down = up = (1 << 62) if v > 0 else -(1 << 62)
        else:
            down, up = math.floor(v), math.ceil(v)
        if word == "gte":
            lo = max(lo, up)
        elif word == "gt":
            lo = max(lo, down + 1)
        elif word == "lte":
            hi = min(hi, down)
        else:
            hi = min(hi, up - 1)
    return int(lo), int(hi)


def _is_text(value) -> bool:
    """A filter value that asks for a text match: a mapping with the key ``"contains"`` (substrings), ``"matches"`` (a
    regular expression) or ``"fuzzy"`` (a string within a bounded number of edits)."""
    return isinstance(value, Mapping) and any(w in value for w in _TEXT_KINDS)


def _is_range(value) -> bool:
    return isinstance(value, Mapping) and not _is_text(value)


class TextSpec(NamedTuple):
    """A ``{"contains": ..., "matches": ...}`` filter value, checked: the distinct patterns as sorted UTF-8 bytes (none when only
    ``matches`` is given), any-of / all-of, whether case matters (``case=False`` folds ASCII letters only, for both), and the
    regular expression as UTF-8 bytes (None: none); the approximate pattern as UTF-8 bytes (None: none; folded like the
    patterns) and the byte edits it allows.  Equal specs select the same rows."""
    patterns: tuple
    any_of: bool
    case: bool
    regex: bytes | None = None
    fuzzy: bytes | None = None
    edits: int = 0


def default_edits(nbytes: int) -> int:
    """The edits a ``fuzzy`` pattern of ``nbytes`` bytes allows when none are given: 1 up to 5 bytes, 2 above -- and 0 for a
    single byte, since a pattern must be longer than its edits (one that is not matches every row)."""
    return min(1 if nbytes <= 5 else 2, max(nbytes - 1, 0))


def text_spec(key: str, spec) -> TextSpec:
    """``{"contains": str | [str, ...], "matches": str, "fuzzy": str, "edits": int, "any": bool = False, "case": bool = True}``
    -- at least one of ``contains``, ``matches`` and ``fuzzy``; all that are given must hold -- as a :class:`TextSpec`.  ``any``
    concerns ``contains`` only, ``case`` all of them.  ``fuzzy`` keeps the rows in which some substring is
    within ``edits`` insertions, deletions or substitutions of one BYTE of the string (0..3; :func:`default_edits` when left
    out); the string has 1..64 bytes of UTF-8 and more bytes than ``edits``.  ``ValueError`` naming ``key`` for an unknown
    word, a pattern that is no ``str``, an empty pattern, one over 64 bytes of UTF-8, no pattern at all or more than 8, flags
    that are not bools, a regular expression that is no ``str`` or that ``regex_dfa.compile_regex`` refuses (the construct is
    named), ``edits`` without ``fuzzy``, ``edits`` that is no int or outside 0..3, and a ``fuzzy`` not longer than its edits."""
    unknown = [w for w in spec if w not in _TEXT_WORDS]
    if unknown:
        raise ValueError(f"text filter on {key!r}: unknown word {unknown[0]!r} (use {', '.join(_TEXT_WORDS)})")
    if not any(w in spec for w in _TEXT_KINDS):
        raise ValueError(f"text filter on {key!r}: needs 'contains' (strings), 'matches' (a regular expression), 'fuzzy' (a string "
                         f"within 'edits' edits) or several of them")
    pats = spec.get("contains", [])
    pats = [pats] if isinstance(pats, str) else list(pats) if isinstance(pats, (list, tuple)) else None
    if pats is None or not all(isinstance(p, str) for p in pats):
        raise ValueError(f"text filter on {key!r}: 'contains' takes a str or a list of str, not {spec['contains']!r}")
    if not (1 if "contains" in spec else 0) <= len(pats) <= ffi.TEXT_MAX_PATTERNS:
        raise ValueError(f"text filter on {key!r}: {len(pats)} patterns (1..{ffi.TEXT_MAX_PATTERNS} are matched in one pass)")
    raw = [p.encode("utf-8", "surrogatepass") for p in pats]
    for p, b in zip(pats, raw):
        if not 1 <= len(b) <= ffi.TEXT_MAX_PATTERN_BYTES:
            raise ValueError(f"text filter on {key!r}: the pattern {p[:80]!r} has {len(b)} bytes of UTF-8 (1..{ffi.TEXT_MAX_PATTERN_BYTES})")
    flags = []
    for word, default in (("any", False), ("case", True)):
        v = spec.get(word, default)
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"text filter on {key!r}: {word}={v!r} is not a bool")
        flags.append(bool(v))
    if not flags[1]:
        raw = [b.translate(_ASCII_LOWER) for b in raw]     # (what the device compares: folded patterns are equal patterns)
    regex = None
    if "matches" in spec:
        if not isinstance(spec["matches"], str):
            raise ValueError(f"text filter on {key!r}: 'matches' takes a str (a regular expression), not {spec['matches']!r}")
        regex = spec["matches"].encode("utf-8", "surrogatepass")
        regex_dfa.compile_regex(regex, flags[1], key)              # (refuses with the key named; the DFA stays in its cache)
    if "fuzzy" not in spec:
        if "edits" in spec:
            raise ValueError(f"text filter on {key!r}: 'edits' stands beside 'fuzzy' only")
        return TextSpec(tuple(sorted(set(raw))), flags[0], flags[1], regex)
    if not isinstance(spec["fuzzy"], str):
        raise ValueError(f"text filter on {key!r}: 'fuzzy' takes a str, not {spec['fuzzy']!r}")
    fuzzy = spec["fuzzy"].encode("utf-8", "surrogatepass")
    if not 1 <= len(fuzzy) <= ffi.TEXT_MAX_PATTERN_BYTES:
        raise ValueError(f"text filter on {key!r}: the 'fuzzy' pattern {spec['fuzzy'][:80]!r} has {len(fuzzy)} bytes of UTF-8 (1..{ffi.TEXT_MAX_PATTERN_BYTES})")
    edits = spec.get("edits")
    if edits is None:
        edits = default_edits(len(fuzzy))
    if isinstance(edits, (bool, np.bool_)) or not isinstance(edits, (int, np.integer)) or not 0 <= edits <= ffi.FUZZY_MAX_EDITS:
        raise ValueError(f"text filter on {key!r}: edits={edits!r} is not an int in 0..{ffi.FUZZY_MAX_EDITS}")
    if len(fuzzy) <= edits:
        raise ValueError(f"text filter on {key!r}: the 'fuzzy' pattern {spec['fuzzy']!r} has {len(fuzzy)} bytes, not more than "
                         f"edits={int(edits)} (every text would match)")
    return TextSpec(tuple(sorted(set(raw))), flags[0], flags[1], regex, fuzzy if flags[1] else fuzzy.translate(_ASCII_LOWER), int(edits))


def fuzzy_distance(pattern: bytes, text: bytes) -> tuple[int, int]:
    """``(distance, last)`` of an approximate match by its definition, on the host: the least Levenshtein
    distance between ``pattern`` and any substring of ``text`` -- Sellers' table, ``D[0][j] = 0``, ``D[i][0] = i``, the minimum of
    its last row -- and the index of the last byte of the first substring that reaches it (-1: the empty substring at the text's
    start does, which takes ``len(pattern)`` edits).  Neither side is folded here.  For the hits a text search returns, not
    for filtering: that is the device's work."""
    m = len(pattern)
    pat = np.frombuffer(pattern, np.uint8)
    col = np.arange(m + 1, dtype=np.int64)
    best, last = m, -1
    steps = np.arange(m + 1, dtype=np.int64)
    for j, c in enumerate(text):
        diag = col[:-1] + (pat != c)
        new = np.empty_like(col)
        new[0] = 0
        new[1:] = np.minimum(diag, col[1:] + 1)
        new = np.minimum.accumulate(new - steps) + steps                 # (the deletions down the column: new[i] = min(new[i], new[i-1] + 1))
        col = new
        if col[m] < best:
            best, last = int(col[m]), j
            if best == 0:
                break
    return best, last


def fuzzy_pieces(pattern: bytes, edits: int) -> tuple:
    """The exact prefilter of an approximate match (pigeonhole): ``pattern`` cut into ``edits + 1`` contiguous
    pieces of nearly equal length.  ``edits`` edits touch at most ``edits`` of them, so every occurrence within ``edits`` edits
    holds one piece verbatim, and only the rows that hold ANY piece need the walk.  ``()`` when the cut cannot help: no edits
    (the walk is then the grep), or a shortest piece under ``_FUZZY_MIN_PIECE`` bytes -- a piece of one or two bytes occurs in
    almost every chunk of code, so its grep costs a pass and removes next to nothing."""
    n = edits + 1
    if edits == 0 or len(pattern) // n < _FUZZY_MIN_PIECE:
        return ()
    cuts = [len(pattern) * i // n for i in range(n + 1)]
    return tuple(sorted({pattern[a:b] for a, b in zip(cuts, cuts[1:])}))


def has_text_condition(filters, must_not=None) -> bool:
    """Does a filter (a dict, None, or a per-query sequence of them) carry a ``{"contains": ...}`` / ``{"matches": ...}`` /
    ``{"fuzzy": ...}`` value?"""
    for f in (filters, must_not):
        for d in (f if isinstance(f, (list, tuple)) else [f]):
            if isinstance(d, Mapping) and any(_is_text(v) for v in d.values()):
                return True
    return False


# -- reachability in the call graph as a filter condition
GRAPH_KEY = "graph"      # filters={"graph": {"callers_of": "pkg.mod.f", "hops": 3}}: not a payload key, a condition on the row's node
_GRAPH_WORDS = tuple(graph_mod.FILTER_WORDS) + ("hops", "relation", "include_self", "match")
_GRAPH_CACHE = 8         # reachability results a collection keeps (a repeated query under the same graph filter runs no second BFS)


class GraphSpec(NamedTuple):
    """A ``{"callers_of" | "callees_of" | "connected_to": name or names, ...}`` filter value, checked: the direction of travel,
    the distinct names sorted, the hops, the relation, whether the named nodes' own rows pass, and how names resolve."""
    direction: str
    names: tuple
    hops: int
    relation: str
    include_self: bool
    match: str


class GraphStructureSpec(NamedTuple):
    """A ``{"in_cycle": True}`` / ``{"same_cycle_as": name}`` / ``{"depth" | "height": int or range}`` filter value, checked
    (DESIGN.md 3.31): the kind, its argument (True, the name, or inclusive ``(lo, hi)``), the relation and how a name resolves."""
    kind: str
    arg: Any
    relation: str
    match: str


class GraphBetweenSpec(NamedTuple):
    """A ``{"between": [source or names, target or names], "hops": 8, "shortest": False, ...}`` filter value, checked (DESIGN.md
    3.32): the distinct names of either end sorted, the hop budget, whether only shortest chains count, the relation and how
    names resolve."""
    sources: tuple
    targets: tuple
    hops: int
    shortest: bool
    relation: str
    match: str


def _graph_between_spec(spec) -> GraphBetweenSpec:
    word = graph_mod.BETWEEN_WORD
    unknown = [k for k in spec if k not in (word, "hops", "shortest", "relation", "match")]
    if unknown:
        raise ValueError(f"filter key {GRAPH_KEY!r}: {word} stands alone beside any of hops, shortest, relation, match (got {sorted(map(str, spec))})")
    ends = spec[word]
    if not isinstance(ends, (list, tuple)) or len(ends) != 2:
        raise ValueError(f"filter key {GRAPH_KEY!r}: {word} takes [source or names, target or names], not {ends!r}")
    sides = []
    for names in ends:
        names = [names] if isinstance(names, str) else list(names) if isinstance(names, _COLLECTIONS) else None
        if not names or not all(isinstance(n, str) for n in names):
            raise ValueError(f"filter key {GRAPH_KEY!r}: either end of {word} is a node name or a non-empty list of them, not {ends!r}")
        sides.append(tuple(sorted(set(names))))
    hops, shortest = spec.get("hops", 8), spec.get("shortest", False)
    if isinstance(hops, bool) or not isinstance(hops, (int, np.integer)) or not 1 <= int(hops) <= ffi.GRAPH_MAX_HOPS:
        raise ValueError(f"filter key {GRAPH_KEY!r}: hops must be an int in 1..{ffi.GRAPH_MAX_HOPS}, not {hops!r}")
    if not isinstance(shortest, bool):
        raise ValueError(f"filter key {GRAPH_KEY!r}: shortest is True or False, not {shortest!r}")
    relation, match = spec.get("relation", "calls"), spec.get("match", "exact")
    if not isinstance(relation, str) or match not in ("exact", "suffix"):
        raise ValueError(f"filter key {GRAPH_KEY!r}: relation is a string and match 'exact' or 'suffix' (got {relation!r}, {match!r})")
    return GraphBetweenSpec(sides[0], sides[1], int(hops), shortest, relation, match)


def _graph_structure_spec(spec) -> GraphStructureSpec:
    kinds = [k for k in spec if k in graph_mod.STRUCTURE_WORDS]
    allowed = ("relation", "match") if kinds == ["same_cycle_as"] else ("relation",)
    unknown = [k for k in spec if k not in kinds and k not in allowed]
    if unknown or len(kinds) != 1:
        raise ValueError(f"filter key {GRAPH_KEY!r}: exactly one of {', '.join(graph_mod.STRUCTURE_WORDS)} (or of {', '.join(graph_mod.FILTER_WORDS)}) "
                         f"and 'relation' (got {sorted(map(str, spec))})")
    kind, value = kinds[0], spec[kinds[0]]
    relation, match = spec.get("relation", "calls"), spec.get("match", "exact")
    if not isinstance(relation, str) or match not in ("exact", "suffix"):
        raise ValueError(f"filter key {GRAPH_KEY!r}: relation is a string and match 'exact' or 'suffix' (got {relation!r}, {match!r})")
    if kind == "in_cycle":
        if value is not True:
            raise ValueError(f"filter key {GRAPH_KEY!r}: in_cycle takes True (exclude the cycles with must_not), not {value!r}")
        arg = True
    elif kind == "same_cycle_as":
        if not isinstance(value, str) or not value:
            raise ValueError(f"filter key {GRAPH_KEY!r}: same_cycle_as takes one node name, not {value!r}")
        arg = value
    elif isinstance(value, (int, np.integer)) and not isinstance(value, bool):
        if value < 0:
            raise ValueError(f"filter key {GRAPH_KEY!r}: {kind} is a layer number >= 0, not {value!r}")
        arg = (int(value), int(value))
    elif isinstance(value, Mapping):
        if any(v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer))) for v in value.values()):
            raise ValueError(f"filter key {GRAPH_KEY!r}: the bounds of a {kind} range are ints, not {dict(value)!r}")
        try:
            arg = range_bounds(kind, value)
        except ValueError as e:
            raise ValueError(f"filter key {GRAPH_KEY!r}: {e}") from None
    else:
        raise ValueError(f"filter key {GRAPH_KEY!r}: {kind} takes an int or a range mapping ({', '.join(_RANGE_WORDS)}), not {value!r}")
    return GraphStructureSpec(kind, arg, relation, match)


def graph_spec(spec) -> "GraphSpec | GraphStructureSpec | GraphBetweenSpec":
    """The value of a ``"graph"`` filter entry as a :class:`GraphSpec`; ``ValueError`` naming the key for anything else."""
    if not isinstance(spec, Mapping):
        raise ValueError(f"filter key {GRAPH_KEY!r} takes a mapping {{'callers_of' | 'callees_of' | 'connected_to': name or list of names, 'hops': 1..{ffi.GRAPH_MAX_HOPS}}}, not {spec!r}")
    if graph_mod.BETWEEN_WORD in spec:
        return _graph_between_spec(spec)
    if any(k in graph_mod.STRUCTURE_WORDS for k in spec):
        return _graph_structure_spec(spec)
    unknown = [k for k in spec if k not in _GRAPH_WORDS]
    kinds = [k for k in spec if k in graph_mod.FILTER_WORDS]
    if unknown or len(kinds) != 1:
        raise ValueError(f"filter key {GRAPH_KEY!r}: exactly one of {', '.join(graph_mod.FILTER_WORDS)} and any of hops, relation, include_self, match "
                         f"(got {sorted(map(str, spec))})")
    names = spec[kinds[0]]
    names = [names] if isinstance(names, str) else list(names) if isinstance(names, _COLLECTIONS) else None
    if not names or not all(isinstance(n, str) for n in names):
        raise ValueError(f"filter key {GRAPH_KEY!r}: {kinds[0]} takes a node name or a non-empty list of them, not {spec[kinds[0]]!r}")
    hops = spec.get("hops", 3)
    if isinstance(hops, bool) or not isinstance(hops, (int, np.integer)) or not 1 <= int(hops) <= ffi.GRAPH_MAX_HOPS:
        raise ValueError(f"filter key {GRAPH_KEY!r}: hops must be an int in 1..{ffi.GRAPH_MAX_HOPS}, not {hops!r}")
    relation, match = spec.get("relation", "calls"), spec.get("match", "exact")
    if not isinstance(relation, str) or match not in ("exact", "suffix"):
        raise ValueError(f"filter key {GRAPH_KEY!r}: relation is a string and match 'exact' or 'suffix' (got {relation!r}, {match!r})")
    return GraphSpec(graph_mod.FILTER_WORDS[kinds[0]], tuple(sorted(set(names))), int(hops), relation, bool(spec.get("include_self", True)), match)


def has_graph_condition(filters, must_not=None) -> bool:
    """Does a filter (a dict, None, or a per-query sequence of them) carry a ``"graph"`` entry?"""
    for f in (filters, must_not):
        for d in (f if isinstance(f, (list, tuple)) else [f]):
            if isinstance(d, Mapping) and GRAPH_KEY in d:
                return True
    return False


def _host(x) -> np.ndarray:
    """A device tensor or a host array as a host array."""
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


_DTYPES = {"f32": ffi.DTYPE_F32, "fp32": ffi.DTYPE_F32, "float32": ffi.DTYPE_F32, "bf16": ffi.DTYPE_BF16,
           "bfloat16": ffi.DTYPE_BF16}


@dataclass
class CollectionInfo:
    """What ``get_collection_info`` hands back; callers read ``points_count`` (query/engine.py:299-302)."""

    name: str
    points_count: int
    vectors_count: int
    indexed_vectors_count: int
    status: str = "green"
    config: dict = field(default_factory=dict)


class _Collection:
    """One collection: row shards on the device(s) + the host-side id / payload tables.

    What lives where: vectors, validity bits and the dictionary CODES of the filterable payload keys are on the device
    (columnar int32, one column per key; ``shards.ShardSet`` spreads the rows over one or more ``crh_index`` handles).  The
    host keeps what a hit has to carry back -- ids and payloads, by SLOT (insertion order), columnar (``tables.IdTable`` /
    ``tables.PayloadTable``: no Python object per row) -- and the map slot <-> (shard, local row).  Filters, deletes and the
    update check are resolved on the device from the code columns.  A deleted row keeps its slot until ``compact()``
    (``crh_index_compact``) moves the survivors together on the device and in the tables; the store compacts by itself once
    the dead rows pass a fraction of the collection (the reference deletes and re-inserts every chunk of a file on every
    indexing run, embeddings/indexer.py:61-64)."""

    regex_prefilter = True     # a regex condition first greps for the strings every match holds (tests switch it off to compare)
    fuzzy_prefilter = True     # an approximate condition first greps for the pieces one of which every match holds (likewise)

    def __init__(self, name: str, dim: int, dtype: int, capacity: int, device: int, nshards: int = 1, backend: str = "local",
                 group=None, merge_fn=None, compact_dead_fraction: float = 0.25, compact_min_dead: int = 1024):
        self.name = name
        self.keys = FILTER_KEYS.get(name, ())
        self.numeric_keys = NUMERIC_KEYS.get(name, ())
        self.text_keys = TEXT_KEYS.get(name, ())
        ncols = len(self.keys) + len(self.numeric_keys)          # the numeric columns last
        self.shards = ShardSet(nshards, lambda s: ffi.Index(dim, dtype, capacity_rows=capacity, n_code_cols=ncols, device=device),
                               device=device, backend=backend, group=group, merge_fn=merge_fn)
        self.ids = IdTable()
        self.payloads = PayloadTable(tuple(DICT_KEYS) + tuple(self.keys))
        # slot <-> row.  With ONE shard a slot IS its row (rows are appended and compacted in slot order): no map is kept.
        self.row_shard = np.zeros((0,), np.int32)
        self.row_local = np.zeros((0,), np.int64)
        self.slot_of: list[np.ndarray] = [np.zeros((0,), np.int64) for _ in range(self.shards.ns)]
        self._side: dict[int, Any] = {}      # shard -> ranking.device.SideColumns of its rows (built on first use)
        self._side_books = None
        self._degrees: dict[str, int] | None = None
        self._device = device
        # keyword side, DERIVED like the side columns: shard -> ffi.Lex of its rows, built from the payload
        # tables on the first lexical call, extended lazily, dropped by compact() and load(); never part of a snapshot
        self._lex: dict[int, Any] = {}
        self._lex_df: tuple | None = None    # (mutation state, {term id: df}, N, sum_dl) of the alive rows of the whole collection
        self.lex_stats_calls = 0             # crh_lex_stats rounds run so far (repeated queries reuse the counts)
        # substring side, DERIVED the same way: text key -> shard -> ffi.Text of its rows, built from the payload
        # tables on the first text filter, extended lazily, dropped by compact() and load(); never part of a snapshot
        self._text: dict[str, dict[int, Any]] = {}
        self._text_cache: dict[tuple, tuple] = {}    # (key, spec, other conditions, collection state) -> (tag, words per index, count, the levels of an approximate match or None)
        self.text_match_calls = 0            # text conditions resolved by a grep so far (repeated filters reuse the words)
        # call graph: the node names in order of first appearance (ids only grow), every relation's edges as
        # node-id pairs -- the part a snapshot keeps --, and, DERIVED on first use: the device graph and, per owned shard, the
        # row -> node column (the host array, its device copy)
        self._graph_names: list[str] = []
        self._graph_code: dict[str, int] = {}
        self._graph_rel: dict[str, np.ndarray] = {}
        self._graph_self: dict[str, np.ndarray] = {}   # relation -> the nodes that carried a self-loop (the CSRs keep none): sorted int32
        self._graph_struct: dict[str, dict] = {}       # relation -> components, cyclic bins, layers on the device: DERIVED
        self._graph = None
        self._graph_version = 0              # bumped by every set_graph_edges: what the derived parts and the cache are keyed by
        self._graph_rows: dict[int, tuple] = {}
        self._graph_rows_state = None
        self._graph_cache: dict[tuple, tuple] = {}   # (spec, graph version, collection state) -> (tag, words per index)
        self.graph_bfs_calls = 0             # graph conditions resolved by a BFS so far (repeated filters reuse the words)
        self.graph_ppr_calls = 0             # personalised PageRank passes run so far (64 queries or name sets each)
        self.graph_scc_calls = 0             # component computations run so far (one per relation and graph version)
        self.compact_dead_fraction, self.compact_min_dead = compact_dead_fraction, compact_min_dead
        self.compactions = 0
        self.group_rounds = {"queries": 0, "round2": 0, "exclusion": 0}    # search_grouped: queries asked / sent to round 2 / exclusion rounds run
        self.recommend_rounds = {"queries": 0, "round2": 0, "short": 0}    # recommend: queries asked / sent to round 2 / answered short
        self.span_rounds = {"queries": 0, "round2": 0, "short": 0}         # search_spans: queries asked / sent to round 2 / answered short
        # One process per shard (backend "dist"): a rank keeps the payload TEXT (content, summary: 4.2 of the 5.2 GB of host
        # tables per 10M chunks) of its OWN rows only -- everybody else stores an empty string there -- and a hit's payload comes
        # from the rank that owns the row (payloads_of: one byte exchange per search, shards.ShardSet.exchange_bytes).
        self.partial = backend == "dist" and nshards > 1

    @property
    def index(self):
        """The one ``crh_index`` of an unsharded collection (tools and tests look at it)."""
        if self.shards.ns != 1:
            raise AttributeError("a sharded collection has no single index (use .shards)")
        return self.shards.index[0]

    # -- slots and rows
    def rows_of(self, slots: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        slots = np.asarray(slots, np.int64)
        if self.shards.ns == 1:
            return np.zeros(slots.shape, np.int32), slots
        return self.row_shard[slots], self.row_local[slots]

    def slots_of(self, shard: np.ndarray, local: np.ndarray) -> np.ndarray:
        """Slots of rows (shard, local); -1 stays -1."""
        local = np.asarray(local, np.int64)
        if self.shards.ns == 1:
            return local
        out = np.full(local.shape, -1, np.int64)
        for s in range(self.shards.ns):
            m = (np.asarray(shard) == s) & (local >= 0)
            if m.any():
                out[m] = self.slot_of[s][local[m]]
        return out

    def _global_slots(self, rows: np.ndarray) -> np.ndarray:
        """Slots of a table of GLOBAL rows (``shard * SHARD_STRIDE + local row``, as the shards' candidate lists carry them)."""
        return self.slots_of(*split_global(rows))

    def side_columns(self) -> dict[int, Any]:
        """Per-shard side data for the device re-rank (ranking/device.py), extended lazily as rows are appended; the
        dictionaries behind the file / merge-key / node codes are shared by the shards (candidates of different shards are
        compared by code)."""
        from .ranking.device import SideColumns
        if self._side_books is None:
            self._side_books = {"file": {}, "key": {}, "node": {}}
        for s in self.shards.owned:
            side = self._side.get(s)
            if side is None:
                side = self._side[s] = SideColumns(self._device, books=self._side_books)
            have, want = side.rows, self.shards.rows[s]
            if have < want:
                slots = np.arange(have, want) if self.shards.ns == 1 else self.slot_of[s][have:want]
                side.append([self.payloads.get(int(t)) if t >= 0 else {} for t in slots])      # (-1: a dead row without a slot)
                if self._degrees is not None:
                    side.set_degrees(self._degrees)
        return self._side

    def gather_side(self, rows_dev):
        """Side columns of a candidate table of GLOBAL rows (CUDA int64 [nq, k]), complete over all shards."""
        sides = self.side_columns()
        total = None
        for s in self.shards.owned:
            cols = sides[s].gather(rows_dev, row_base=s * SHARD_STRIDE)
            if total is None:
                total = cols
            else:
                total.packed += cols.packed
        self.shards.reduce(total.packed, "SUM")
        return total

    def set_degrees(self, total_degree: dict[str, int]) -> None:
        self._degrees = dict(total_degree)
        for side in self._side.values():
            side.set_degrees(self._degrees)

    # -- filters
    def _column(self, key: str) -> int:
        if key not in self.keys:
            raise ValueError(f"collection {self.name!r} cannot filter on payload key {key!r} "
                             f"(filterable: {', '.join(self.keys)})")
        return self.keys.index(key)

    def _numeric_column(self, key: str) -> int:
        return len(self.keys) + self.numeric_keys.index(key)

    def _range_condition(self, key: str, value, negate: bool) -> tuple:
        """A filter entry on a numeric key as ``(column, lo, hi, "between" | "not_between")``: a ``Range`` mapping, or a plain
        int (``lo == hi``).  ``ValueError`` naming the key for anything else (a set of values, a string, a float, a bool)."""
        if _is_range(value):
            lo, hi = range_bounds(key, value)
        elif isinstance(value, (int, np.integer)) and not isinstance(value, bool):
            lo = hi = int(value)
        else:
            raise ValueError(f"payload key {key!r} holds numbers: filter it with an int or a range mapping "
                             f"({', '.join(_RANGE_WORDS)}), not {value!r}")
        return (self._numeric_column(key), lo, hi, "not_between" if negate else "between")

    def _codes_of(self, key: str, values) -> list[int]:
        """Codes of the values the column's dictionary knows (a value that was never stored contributes none)."""
        book = self.payloads.cols[key]
        return sorted({c for c in (book.code_of(v) for v in values) if c is not None})

    def device_filters(self, filters: dict[str, Any] | None, must_not: dict[str, Any] | None = None) -> list[tuple] | None:
        """dict(s) -> the conditions of ``ffi.Index``: ``(column, code)`` for a plain value, ``(column, codes, False)`` for a
        list / tuple / set of values (any of them), ``(column, codes, True)`` for a ``must_not`` entry (none of them; one
        value or a collection); on a numeric key (``numeric_keys``) ``(column, lo, hi, "between")`` for a range mapping or a
        plain int and ``(column, lo, hi, "not_between")`` under ``must_not``.  None when a plain value or a whole any-of
        collection was never stored (nothing can match); a ``must_not`` entry whose values were never stored excludes nothing
        and is dropped."""
        out: list[tuple] = []
        texts: list[tuple] = []                                          # (key, TextSpec, negate): resolved once the others are known
        graphs: list[tuple] = []                                         # (GraphSpec, negate): resolved before the text conditions
        for key, value in (filters or {}).items():
            if key == GRAPH_KEY:
                graphs.append((graph_spec(value), False))
                continue
            if self._text_entry(key, value, False, texts):
                continue
            if key in self.numeric_keys:
                out.append(self._range_condition(key, value, False))
                continue
            if _is_range(value):
                raise ValueError(f"payload key {key!r} is dictionary-coded: a range needs one of the numeric keys "
                                 f"({', '.join(self.numeric_keys) or 'this collection has none'})")
            col = self._column(key)
            if isinstance(value, _COLLECTIONS):
                codes = self._codes_of(key, value)
                if not codes:
                    return None
                out.append((col, codes, False))
            else:
                code = self.payloads.cols[key].code_of(value)
                if code is None:
                    return None
                out.append((col, code))
        for key, value in (must_not or {}).items():
            if key == GRAPH_KEY:
                graphs.append((graph_spec(value), True))
                continue
            if self._text_entry(key, value, True, texts):
                continue
            if key in self.numeric_keys:
                out.append(self._range_condition(key, value, True))      # (rows without the value pass, as under Qdrant's must_not)
                continue
            if _is_range(value):
                raise ValueError(f"payload key {key!r} is dictionary-coded: a range needs one of the numeric keys "
                                 f"({', '.join(self.numeric_keys) or 'this collection has none'})")
            col = self._column(key)
            codes = self._codes_of(key, value if isinstance(value, _COLLECTIONS) else [value])
            if codes:
                out.append((col, codes, True))
        if len(out) + len(graphs) > ffi.MAX_FILTERS:
            raise ValueError(f"{len(out) + len(graphs)} filter conditions, the device takes {ffi.MAX_FILTERS} (a graph condition is one)")
        for spec, negate in graphs:                                      # (before the text conditions: a grep skips the tiles they empty)
            cond = self._graph_condition(spec, negate)
            if cond is None and not negate:
                return None                                              # (no name is a node: nothing is reachable)
            if cond is not None:
                out.append(cond)
        if texts:
            if len(out) + len(texts) > ffi.MAX_FILTERS:
                raise ValueError(f"{len(out) + len(texts)} filter conditions, the device takes {ffi.MAX_FILTERS} (a text condition is one)")
            others = list(out)                                           # every text condition greps under the OTHER kinds' rows
            out += [self._text_condition(key, spec, negate, others) for key, spec, negate in texts]
        return out

    # -- substring filters
    def _text_entry(self, key: str, value, negate: bool, texts: list) -> bool:
        """Files a filter entry that concerns a text key under ``texts`` and says so; ``ValueError`` naming the key for
        ``contains`` on another key and for anything but ``contains`` on a text key."""
        if key not in self.text_keys:
            if _is_text(value):
                raise ValueError(f"collection {self.name!r} cannot match text in payload key {key!r} "
                                 f"(text keys: {', '.join(self.text_keys) or 'none'})")
            return False
        if not _is_text(value):
            raise ValueError(f"payload key {key!r} holds text: filter it with a mapping {{'contains': str or list of str}}, "
                             f"{{'matches': regular expression}} or {{'fuzzy': str, 'edits': 0..{ffi.FUZZY_MAX_EDITS}}}, not {value!r}")
        texts.append((key, text_spec(key, value), negate))
        return True

    def _text_ready(self, key: str) -> dict[int, Any]:
        """The text arenas of ``key`` for the owned shards, brought up to date: the UTF-8 of the rows appended since the last
        text filter is appended.  A value that is absent or no ``str`` is empty text.  A collection that is never filtered by
        text never comes here."""
        if self.shards.backend == "dist":
            raise VectorStoreError("text filters are not available with shard_backend='dist' yet (a rank holds the text of its own rows only)")
        arenas = self._text.setdefault(key, {})
        for s in self.shards.owned:
            arena = arenas.get(s)
            if arena is None:
                arena = arenas[s] = ffi.Text(capacity_rows=self.shards.rows[s], device=self._device)
            have, want = arena.count()[0], self.shards.rows[s]
            for a in range(have, want, 65536):
                b = min(want, a + 65536)
                slots = np.arange(a, b) if self.shards.ns == 1 else self.slot_of[s][a:b]
                vals = [self.payloads.value(int(t), key) if t >= 0 else None for t in slots]                  # (-1: a dead row without a slot)
                raw = [v.encode("utf-8", "surrogatepass") if isinstance(v, str) else b"" for v in vals]
                off = np.zeros(len(raw) + 1, np.int64)
                np.cumsum([len(r) for r in raw], out=off[1:])
                arena.append(off, b"".join(raw))
        return arenas

    def _text_drop(self) -> None:
        for arenas in self._text.values():
            for arena in arenas.values():
                arena.close()
        self._text, self._text_cache = {}, {}

    def _text_condition(self, key: str, spec: TextSpec, negate: bool, others: list) -> "ffi.RowWords":
        """A text condition as the row-bitmap condition of the device filter.  Per owned shard: the words of the OTHER
        conditions (``crh_index_row_mask``; none: the alive words), ``crh_text_match`` under them -- a tile they leave empty
        costs no read of its text -- and the result as ``CRH_COND_WORDS`` (``negate``: ``_NOT_WORDS``).  With a regular
        expression the literal match runs for ``contains`` if given, otherwise for the strings every match of
        the expression holds (``regex_prefilter``; none: no literal pass), and ``crh_text_regex`` walks the rows that are left.
        With an approximate pattern ``crh_text_fuzzy`` goes last, under the words of the passes before it and
        -- ``fuzzy_prefilter``, when :func:`fuzzy_pieces` cuts any -- under a grep for the pieces one of which every match
        holds; its last level is the condition, and all its levels stay with the result (:meth:`_text_levels`).  The last few
        results are kept, keyed by what they were computed from; every result lives in buffers of its own under a tag of its
        own."""
        hit = self._text_result(key, spec, others)
        return ffi.RowWords(hit[0], hit[1], negate)

    def _text_levels(self, key: str, spec: TextSpec, others: list) -> tuple[list, list]:
        """The levels of an approximate condition as ``([RowWords of level 0 .. edits], [rows at distance 0 .. edits])``: level
        ``d`` holds the rows (under ``others`` and the spec's other words) whose distance is at most ``d``; from the result
        :meth:`_text_condition` computed or kept, so it costs no second walk."""
        hit = self._text_result(key, spec, others)
        tags, levels, counts = hit[3]
        return ([ffi.RowWords(tags[d], {i: lv[d] for i, lv in levels.items()}) for d in range(spec.edits + 1)],
                [counts[0]] + [counts[d] - counts[d - 1] for d in range(1, spec.edits + 1)])

    def _text_result(self, key: str, spec: TextSpec, others: list) -> tuple:
        """``(tag, {id(index): words}, rows, fuzzy)`` of a text condition, computed or taken from the cache; ``fuzzy`` is None
        or ``(tags, {id(index): levels [edits + 1, words]}, cumulative counts)``, the last level being ``words`` under ``tag``."""
        arenas = self._text_ready(key)
        state = (tuple(self.shards.rows), self.shards.count()[1], self.compactions)
        ck = (key, spec, ffi.filter_key(others), state)
        hit = self._text_cache.pop(ck, None)
        if hit is None:
            words, total, levels, counts = {}, 0, {}, [0] * (spec.edits + 1)
            stream = self.shards._stream()
            for s in self.shards.owned:
                ix = self.shards.index[s]
                mask = ix.row_mask(others, stream=stream)
                if spec.fuzzy is not None:
                    if spec.patterns:
                        mask, _ = arenas[s].match(spec.patterns, fold_case=not spec.case, any_of=spec.any_of, mask=mask, count=False, stream=stream)
                    if spec.regex is not None:
                        mask, _ = arenas[s].regex(regex_dfa.compile_regex(spec.regex, spec.case, key), mask=mask, count=False, stream=stream)
                    pieces = fuzzy_pieces(spec.fuzzy, spec.edits) if self.fuzzy_prefilter else ()
                    if pieces:
                        mask, _ = arenas[s].match(pieces, fold_case=not spec.case, any_of=True, mask=mask, count=False, stream=stream)
                    lv, cs = arenas[s].fuzzy(spec.fuzzy, spec.edits, fold_case=not spec.case, mask=mask, stream=stream)
                    levels[id(ix)] = lv
                    counts = [a + b for a, b in zip(counts, cs)]
                    w, n = lv[spec.edits], cs[spec.edits]
                elif spec.regex is None:
                    w, n = arenas[s].match(spec.patterns, fold_case=not spec.case, any_of=spec.any_of, mask=mask, stream=stream)
                else:
                    dfa = regex_dfa.compile_regex(spec.regex, spec.case, key)
                    if spec.patterns:
                        mask, _ = arenas[s].match(spec.patterns, fold_case=not spec.case, any_of=spec.any_of, mask=mask, count=False, stream=stream)
                    elif self.regex_prefilter and dfa.literals:
                        mask, _ = arenas[s].match(dfa.literals, fold_case=not spec.case, mask=mask, count=False, stream=stream)
                    w, n = arenas[s].regex(dfa, mask=mask, stream=stream)
                words[id(ix)] = w
                total += n
            self.text_match_calls += 1
            fuzzy = None
            if spec.fuzzy is not None:                                    # (the last level IS the condition: one tag for both)
                tags = [ffi.next_words_tag() for _ in range(spec.edits + 1)]
                fuzzy = (tags, levels, counts)
            hit = (fuzzy[0][-1] if fuzzy else ffi.next_words_tag(), words, total, fuzzy)
            while len(self._text_cache) >= _TEXT_CACHE:
                self._text_cache.pop(next(iter(self._text_cache)))       # (the least recently used: hits are re-inserted below)
        self._text_cache[ck] = hit
        return hit

    # -- call graph
    def set_graph_edges(self, edges, relation: str = "calls", derive_degrees: bool = False) -> dict[str, Any]:
        """Sets or replaces the edges of ``relation``: ``edges`` is an iterable of ``(source_name, target_name)``.  Nodes are
        numbered in order of first appearance, over all relations of the collection; self-loops and repeats are dropped from
        the edges, the nodes that carried a self-loop are kept beside them (sorted int32, ``_graph_self``).
        ``derive_degrees``: the re-rank's centrality table becomes the distinct in-degree + out-degree of this relation."""
        if not isinstance(relation, str) or not relation:
            raise ValueError(f"a graph relation is named by a non-empty string, not {relation!r}")
        if relation not in self._graph_rel and len(self._graph_rel) >= graph_mod.MAX_RELATIONS:
            raise ValueError(f"a collection holds at most {graph_mod.MAX_RELATIONS} graph relations ({', '.join(self._graph_rel)})")
        n0 = len(self._graph_names)
        try:
            pairs = graph_mod.number_edges(edges, self._graph_code, self._graph_names)
        except Exception:
            for name in self._graph_names[n0:]:                          # all or nothing: the names of a refused list leave again
                del self._graph_code[name]
            del self._graph_names[n0:]
            raise
        self._graph_rel[relation] = graph_mod.unique_edges(pairs, len(self._graph_names))
        self._graph_self[relation] = graph_mod.self_loops(pairs, len(self._graph_names))
        self._graph_changed()
        if derive_degrees:
            deg = graph_mod.total_degrees(self._graph_rel[relation], len(self._graph_names))
            self.set_degrees({self._graph_names[i]: int(d) for i, d in enumerate(deg) if d})
        return self.graph_info()

    def graph_info(self) -> dict[str, Any]:
        return {"nodes": len(self._graph_names), "relations": {r: int(len(e)) for r, e in self._graph_rel.items()}}

    def _graph_changed(self) -> None:
        self._graph_version += 1
        self._graph_drop()

    def _graph_drop(self) -> None:
        """Forgets what is derived (the device graph, the row -> node columns, the kept results); names and edges stay."""
        if self._graph is not None:
            self._graph.close()
        self._graph, self._graph_rows, self._graph_rows_state, self._graph_cache, self._graph_struct = None, {}, None, {}, {}

    def _graph_ready(self, relation: str) -> tuple[Any, int]:
        """(the device graph, built from the kept edges on first use; the number of ``relation`` in it)."""
        if self.shards.backend == "dist":
            raise VectorStoreError(f"the call graph ({GRAPH_KEY!r} filters, graph_neighbors, call_chain) is not available with shard_backend='dist' yet")
        if relation not in self._graph_rel:
            raise ValueError(f"collection {self.name!r} has no graph relation {relation!r} (set_graph_edges; known: {', '.join(self._graph_rel) or 'none'})")
        if self._graph is None:
            n = len(self._graph_names)
            g = ffi.Graph(n, device=self._device)
            try:
                for r, pairs in enumerate(self._graph_rel.values()):
                    g.set_relation(r, *graph_mod.build_csr(pairs, n))
            except Exception:
                g.close()
                raise
            self._graph = g
        return self._graph, list(self._graph_rel).index(relation)

    def _graph_row_nodes(self) -> dict[int, Any]:
        """shard -> the row -> node column where the indexes live (int32, -1: the row's key is no node), by the re-rank's key
        rule ``graph_node_id or entity_name``; derived from the payload table on first use, extended as rows are appended,
        rebuilt after a compaction and after the graph's names changed."""
        state = (self._graph_version, self.compactions)
        if self._graph_rows_state != state:
            self._graph_rows, self._graph_rows_state = {}, state
        code, value = self._graph_code, self.payloads.value
        for s in self.shards.owned:
            host, dev = self._graph_rows.get(s, (np.zeros((0,), np.int32), None))
            have, want = int(host.size), self.shards.rows[s]
            if have < want or dev is None:
                slots = np.arange(have, want) if self.shards.ns == 1 else self.slot_of[s][have:want]
                new = np.fromiter((code.get(value(int(t), "graph_node_id") or value(int(t), "entity_name", "") or "", -1) if t >= 0 else -1
                                   for t in slots), np.int32, want - have)
                host = np.concatenate([host, new])
                self._graph_rows[s] = (host, self.shards._local(host))
        return {s: self._graph_rows[s][1] for s in self.shards.owned}

    def _graph_condition(self, spec: GraphSpec, negate: bool) -> "ffi.RowWords | None":
        """A graph condition as the row-bitmap condition of the device filter: ONE BFS with one query bit from the named nodes,
        then per owned shard the reached nodes' rows (``crh_graph_row_words`` over the row -> node column) as
        ``CRH_COND_WORDS`` (``negate``: ``_NOT_WORDS``).  None when no name is a node.  The last few results are kept, keyed by
        what they were computed from; every result lives in buffers of its own under a tag of its own."""
        if isinstance(spec, GraphStructureSpec):
            return self._graph_structure_condition(spec, negate)
        if isinstance(spec, GraphBetweenSpec):
            return self._graph_between_condition(spec, negate)
        graph, rel = self._graph_ready(spec.relation)
        ids, _ = graph_mod.resolve(spec.names, self._graph_code, self._graph_names, spec.match)
        if not ids:
            return None
        def reached(stream):
            self.graph_bfs_calls += 1
            return graph.bfs(rel, spec.direction, [ids], spec.hops, include_self=spec.include_self, stream=stream)[1]
        return self._graph_row_words(spec, negate, graph, reached)

    def _graph_row_words(self, spec, negate: bool, graph, node_words) -> "ffi.RowWords":
        """The rows of the nodes whose word ``node_words(stream)`` (the ``seen`` words of a BFS, or ``crh_graph_node_words``')
        carries bit 0, per owned shard, kept in the LRU under ``spec`` and what the rows were computed from."""
        ck = (spec, self._graph_version, tuple(self.shards.rows), self.shards.count()[1], self.compactions)
        hit = self._graph_cache.pop(ck, None)
        if hit is None:
            stream = self.shards._stream()
            columns = self._graph_row_nodes()
            seen = node_words(stream)
            words = {id(self.shards.index[s]): graph.row_words(columns[s], 0, seen=seen, stream=stream) for s in self.shards.owned}
            hit = (ffi.next_words_tag(), words)
            while len(self._graph_cache) >= _GRAPH_CACHE:
                self._graph_cache.pop(next(iter(self._graph_cache)))     # (the least recently used: hits are re-inserted below)
        self._graph_cache[ck] = hit
        return ffi.RowWords(hit[0], hit[1], negate)

    def _graph_between_condition(self, spec: GraphBetweenSpec, negate: bool) -> "ffi.RowWords | None":
        """The rows of the nodes that lie on a way of at most ``hops`` edges from the one named set to the other:
        a BFS along the edges from the sources, one against them from the targets in the second workspace, and
        ``crh_graph_between`` over the two, then :meth:`_graph_row_words`.  None when either end names no node."""
        graph, rel = self._graph_ready(spec.relation)
        src, _ = graph_mod.resolve(spec.sources, self._graph_code, self._graph_names, spec.match)
        dst, _ = graph_mod.resolve(spec.targets, self._graph_code, self._graph_names, spec.match)
        if not src or not dst:
            return None
        def between(stream):
            self.graph_bfs_calls += 2
            graph.bfs(rel, "callees", [src], spec.hops, include_self=True, stream=stream)
            graph.bfs(rel, "callers", [dst], spec.hops, include_self=True, stream=stream, back=True)
            return graph.between(mode="shortest" if spec.shortest else "any", stream=stream)[0]
        return self._graph_row_words(spec, negate, graph, between)

    # -- the graph as a whole: cycles, components, layers
    def _graph_structure(self, relation: str, layers: bool = False) -> tuple[Any, dict]:
        """(the device graph, the derived state of ``relation``): ``comp`` int32 / ``bins`` int64 [nodes] on the device and
        ``info``; with ``layers`` also ``depth`` / ``height`` int32 [nodes] and ``layers``.  Computed on first use, once per
        relation and graph version; :meth:`_graph_drop` forgets it."""
        graph, rel = self._graph_ready(relation)
        st = self._graph_struct.get(relation)
        stream = self.shards._stream()
        if st is None:
            comp, info = graph.scc(rel, stream=stream)
            self.graph_scc_calls += 1
            loops = self._graph_self.get(relation)
            bins = graph.scc_bins(comp, loops if loops is not None and loops.size else None, stream=stream)
            st = self._graph_struct[relation] = {"comp": comp, "bins": bins, "info": [int(v) for v in info]}
        if layers and "depth" not in st:
            depth, info = graph.layers(rel, "callees", st["comp"], stream=stream)
            st["height"], _ = graph.layers(rel, "callers", st["comp"], stream=stream)
            st["depth"], st["layers"] = depth, int(info[0])
        return graph, st

    def _graph_structure_host(self, st: dict, what: str) -> np.ndarray:
        """A derived array on the host (4 or 8 bytes per node: the listings' output formatting), copied once."""
        host = st.setdefault("host", {})
        if what not in host:
            host[what] = _host(st[what])
        return host[what]

    def _graph_structure_condition(self, spec: GraphStructureSpec, negate: bool) -> "ffi.RowWords | None":
        """A condition on the node's place in the whole graph as the row-bitmap condition of the device filter:
        ``crh_graph_node_words`` over the kept components or layers, then :meth:`_graph_row_words` (the LRU of the walk
        conditions).  None when ``same_cycle_as`` names no node."""
        graph, st = self._graph_structure(spec.relation, layers=spec.kind in ("depth", "height"))
        if spec.kind == "in_cycle":
            args = ("in_cycle", st["comp"], st["bins"], 0, 0)
        elif spec.kind == "same_cycle_as":
            ids, _ = graph_mod.resolve([spec.arg], self._graph_code, self._graph_names, spec.match)
            if not ids:
                return None
            if len(ids) > 1:
                raise ValueError(f"filter key {GRAPH_KEY!r}: same_cycle_as={spec.arg!r} names {len(ids)} nodes ({', '.join(self._graph_names[i] for i in ids[:4])}, ...): name one")
            args = ("same_component", st["comp"], None, int(self._graph_structure_host(st, "comp")[ids[0]]), 0)
        else:
            args = ("range", st[spec.kind], None, spec.arg[0], spec.arg[1])
        return self._graph_row_words(spec, negate, graph, lambda stream: graph.node_words(args[0], args[1], bins=args[2], lo=args[3], hi=args[4], q=0, stream=stream))

    def graph_cycles(self, relation: str, limit: int, members: int) -> dict[str, Any]:
        """The cyclic components of ``relation``, largest first (ties to the node seen first): see ``HipVectorStore.graph_cycles``."""
        if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)) or not 1 <= limit <= ffi.MAX_K:
            raise ValueError(f"graph_cycles: limit must be an int in 1..{ffi.MAX_K}, not {limit!r}")
        if isinstance(members, bool) or not isinstance(members, (int, np.integer)) or members < 0:
            raise ValueError(f"graph_cycles: members must be a non-negative int, not {members!r}")
        graph, st = self._graph_structure(relation)
        names, n = self._graph_names, len(self._graph_names)
        if n == 0:
            return {"components": [], "count": 0, "nodes": 0, "self_recursive": []}
        codes, counts, info = (_host(t) for t in ffi.facet_select(st["bins"], int(limit), self.shards._stream()))
        comp = self._graph_structure_host(st, "comp")
        loops = self._graph_self.get(relation, np.zeros((0,), np.int32))
        looped = set(loops.tolist())
        out = []
        for c, size in zip(codes.reshape(-1).tolist(), counts.reshape(-1).tolist()):
            if c < 0:
                break
            nodes = np.flatnonzero(comp == c)
            out.append({"id": names[c], "size": int(size), "nodes": [names[v] for v in nodes[:members].tolist()],
                        "self_recursive": [names[v] for v in nodes.tolist() if v in looped][:members]})
        bins = self._graph_structure_host(st, "bins")
        alone = [names[v] for v in loops.tolist() if bins[comp[v]] == 1]
        return {"components": out, "count": int(info.reshape(-1)[0]), "nodes": int(info.reshape(-1)[1]),
                "self_recursive": alone if len(alone) <= members else len(alone)}

    def graph_layers(self, relation: str, names, match: str) -> dict[str, Any]:
        """The layers of the condensation of ``relation``: see ``HipVectorStore.graph_layers``."""
        graph, st = self._graph_structure(relation, layers=True)
        n = len(self._graph_names)
        depth, height = self._graph_structure_host(st, "depth"), self._graph_structure_host(st, "height")
        layers = st["layers"] if n else 0
        out = {"layers": layers, "histogram": {"depth": np.bincount(depth, minlength=layers).tolist() if n else [],
                                               "height": np.bincount(height, minlength=layers).tolist() if n else []}, "nodes": []}
        if names is not None:
            ids, missing = graph_mod.resolve(names, self._graph_code, self._graph_names, match)
            comp, bins = self._graph_structure_host(st, "comp"), self._graph_structure_host(st, "bins")
            out["nodes"] = [{"name": self._graph_names[v], "depth": int(depth[v]), "height": int(height[v]), "component": self._graph_names[int(comp[v])],
                             "cyclic": bool(bins[comp[v]] > 0)} for v in ids]
            out["unresolved"] = missing
        return out

    def graph_nodes_of(self, rows_dev, stream: int = 0):
        """The nodes of a table of GLOBAL rows (CUDA int64, -1: padding) as an int32 CUDA tensor of the same shape, -1 where the
        row's key is no node: ``crh_gather_rows_i32`` over every owned shard's row -> node column (a shard answers 0 for the
        rows of the others, so the gathers add up)."""
        columns = self._graph_row_nodes()
        if not self.shards._native():                                    # injected indexes: host arrays all the way
            shard, local = split_global(np.asarray(rows_dev, np.int64))
            out = np.full(local.shape, -1, np.int32)
            for s in self.shards.owned:
                mine = (local >= 0) & (shard == s)
                out[mine] = columns[s][local[mine]]
            return out
        import torch
        total = None
        for s in self.shards.owned:
            part = ffi.gather_rows_i32(rows_dev, s * SHARD_STRIDE, columns[s], 0, stream)
            total = part if total is None else total + part
        return torch.where(rows_dev >= 0, total, torch.full_like(total, -1))

    def search_expanded(self, queries: np.ndarray, limit: int, dfilt, direction: str, hops: int, related_limit: int, relation: str):
        """Per 64 queries: the search, its hit rows gathered to nodes, those nodes as the source sets of ONE BFS, and the list of
        what it reached beyond them -- all on the device; the host sees the finished tables.  Returns ``(scores [nq, limit],
        slots [nq, limit], related nodes [nq, related_limit], their depths, related counts [nq])`` host arrays."""
        import torch
        graph, rel = self._graph_ready(relation)
        stream = self.shards._stream()
        out = []
        for a in range(0, len(queries), ffi.GRAPH_MAX_QUERIES):
            part = np.ascontiguousarray(queries[a:a + ffi.GRAPH_MAX_QUERIES])
            s, r = self.shards.search_device(torch.from_numpy(part).to(torch.device("cuda", self._device)), limit, dfilt)
            graph.bfs(rel, direction, self.graph_nodes_of(r, stream), hops, include_self=True, stream=stream)
            nodes, depth, count = graph.list(related_limit, first_level=1, stream=stream)
            out.append((_host(s), self._global_slots(_host(r)), _host(nodes), _host(depth), _host(count)))
        return tuple(np.concatenate([o[i] for o in out]) for i in range(5))

    # -- graph-propagated relevance (personalised PageRank)
    def _node_slots(self, nodes: np.ndarray) -> np.ndarray:
        """The slots of the representative rows of a host table of nodes (-1: padding), -1 for a node without an alive row."""
        rows_host = self.graph_node_rows()[1]
        nodes = np.asarray(nodes, np.int64)
        rows = np.where(nodes >= 0, rows_host[np.maximum(nodes, 0)], -1) if rows_host.size else np.full(nodes.shape, -1, np.int64)
        return self._global_slots(rows)

    def search_propagated(self, queries: np.ndarray, limit: int, candidates: int, dfilt, prop: dict[str, Any], related_limit: int):
        """Per 64 queries, all on the device: the exact top-``candidates``, their rows gathered to nodes, those nodes as the
        seeds of ONE personalised PageRank (weights ``max(cos, +0)``, or 1), the candidates ordered by graph score and fused
        with the cosine list (``crh_graph_ppr_order`` + ``crh_fuse_select``, m = 2), and the best nodes that are no candidate's
        node (``crh_graph_ppr_bins`` + ``crh_facet_select``).  Returns host arrays ``(slots [nq, limit], fused, cosine,
        graph_score, related nodes [nq, related_limit], their scores, their representative slots)``; -1 is padding."""
        graph, rel = self._graph_ready(prop["relation"])
        stream = self.shards._stream()
        out = []
        for a in range(0, len(queries), ffi.GRAPH_MAX_QUERIES):
            part = np.ascontiguousarray(queries[a:a + ffi.GRAPH_MAX_QUERIES])
            cs, cr = self.shards._candidates(part, candidates, dfilt)
            nodes = self.graph_nodes_of(cr, stream)
            weights = cs.clip(min=0) if prop["seed_weight"] == "cosine" else None
            graph.ppr(rel, prop["direction"], nodes, weights, prop["restart"], prop["steps"], stream=stream)
            self.graph_ppr_calls += 1
            fs, fr, gs = graph.ppr_order(cr, cs, nodes, stream=stream)
            fused = ffi.fuse_select(fs, fr, 2, limit, "rrf", prop["rrf_k"], stream=stream)
            rows, score, first = _host(fused[0]), _host(fused[1]), _host(fused[4])
            at = np.maximum(first, 0)                                    # (a row's first entry lies in list 0: its position there)
            cos = np.where(rows >= 0, np.take_along_axis(_host(cs), at, 1), -np.inf).astype(np.float32)
            gsc = np.where(rows >= 0, np.take_along_axis(_host(gs), at, 1), 0).astype(np.float32)
            if related_limit:
                top, top_scores = (_host(t) for t in graph.ppr_top(related_limit, exclude=nodes, stream=stream))
            else:
                top, top_scores = np.zeros((len(part), 0), np.int32), np.zeros((len(part), 0), np.float32)
            out.append((self._global_slots(rows), score, cos, gsc, top, top_scores, self._node_slots(top)))
        return tuple(np.concatenate([o[i] for o in out]) for i in range(7))

    def graph_rank(self, name_sets, weight_sets, relation: str, direction: str, restart: float, steps: int, limit: int, match: str,
                   include_seeds: bool):
        """Per name set: personalised PageRank seeded by the named nodes (a name's weight goes to every node it stands for), 64
        sets per pass, and its ``limit`` best nodes.  Returns ``[(nodes, scores, slots, unresolved)]``: host arrays of the nodes
        with a positive score, best first, and the slots of their representative rows (-1: none)."""
        graph, rel = self._graph_ready(relation)
        stream = self.shards._stream()
        resolved = []
        for names, ws in zip(name_sets, weight_sets):
            ids, w, missing = [], [], []
            for j, name in enumerate(names):
                got, miss = graph_mod.resolve([name], self._graph_code, self._graph_names, match)
                missing += miss
                ids += got
                w += [1.0 if ws is None else float(ws[j])] * len(got)
            if len(ids) > ffi.MAX_K:
                raise ValueError(f"a seed set of {len(ids)} nodes exceeds the maximum of {ffi.MAX_K}")
            resolved.append((ids, w, missing))
        out = []
        for a in range(0, len(resolved), ffi.GRAPH_MAX_QUERIES):
            part = resolved[a:a + ffi.GRAPH_MAX_QUERIES]
            graph.ppr(rel, direction, [ids for ids, _, _ in part], [w for _, w, _ in part], restart, steps, stream=stream)
            self.graph_ppr_calls += 1
            exclude = None
            if not include_seeds:
                c = max(max(len(ids) for ids, _, _ in part), 1)
                exclude = self.shards._local(np.asarray([ids + [-1] * (c - len(ids)) for ids, _, _ in part], np.int32).reshape(len(part), c))
            nodes, scores = (_host(t) for t in graph.ppr_top(limit, exclude=exclude, stream=stream))
            slots = self._node_slots(nodes)
            out += [(nodes[q][nodes[q] >= 0], scores[q][nodes[q] >= 0], slots[q][nodes[q] >= 0], missing) for q, (_, _, missing) in enumerate(part)]
        return out

    # -- the hybrid re-rank with graph results
    def richness_columns(self) -> dict[int, Any]:
        """Per-shard richness bits (``ranking.device.RichnessColumn``) beside the side columns: derived from the payload table,
        extended as rows are appended, rebuilt after a compaction."""
        from .ranking.device import RichnessColumn
        state = getattr(self, "_rich_state", None)
        if state != self.compactions:
            self._rich, self._rich_state = {}, self.compactions
        for s in self.shards.owned:
            col = self._rich.get(s)
            if col is None:
                col = self._rich[s] = RichnessColumn(self._device)
            have, want = col.rows, self.shards.rows[s]
            if have < want:
                slots = np.arange(have, want) if self.shards.ns == 1 else self.slot_of[s][have:want]
                col.append([self.payloads.get(int(t)) if t >= 0 else {} for t in slots])
        return self._rich

    def graph_node_rows(self):
        """``(device int64 [nodes], host copy)``: every node's representative row -- the lowest alive GLOBAL row whose row -> node
        entry is the node, -1 without one (``crh_graph_node_rows`` over every owned shard's column and alive words, into one
        array).  Kept until rows are appended, deleted or compacted or the graph changes."""
        from .ranking.device import graph_node_rows
        key = (self._graph_version, tuple(self.shards.rows), self.shards.count()[1], self.compactions)
        kept = getattr(self, "_node_rows", None)
        if kept is None or kept[0] != key:
            stream = self.shards._stream()
            columns = self._graph_row_nodes()
            out = None
            for s in self.shards.owned if self.shards._native() else ():
                alive = self.shards.index[s].row_mask(None, stream=stream)
                out = graph_node_rows(columns[s], len(self._graph_names), alive, row_base=s * SHARD_STRIDE, out=out, stream=stream)
            if out is None:                                              # injected indexes: the same minimum on the host
                out = np.full((len(self._graph_names),), -1, np.int64)
                for s in sorted(self.shards.owned, reverse=True):
                    alive = np.unpackbits(np.asarray(self.shards.index[s].row_mask(None)).view(np.uint8), bitorder="little").astype(bool)
                    for r in range(len(columns[s]) - 1, -1, -1):
                        if alive[r] and columns[s][r] >= 0:
                            out[columns[s][r]] = s * SHARD_STRIDE + r
            kept = self._node_rows = (key, out, _host(out))
            self.graph_node_rows_builds = getattr(self, "graph_node_rows_builds", 0) + 1
        return kept[1], kept[2]

    def _graph_role_info(self):
        """What ``engine_helpers.plan_graph_roles`` asks of this collection's graph."""
        col, (_, rows_host) = self, self.graph_node_rows()

        class Info:
            relations = set(col._graph_rel)

            @staticmethod
            def resolve(name, match):
                return graph_mod.resolve(name, col._graph_code, col._graph_names, match)[0]

            @staticmethod
            def is_class(node):
                row = int(rows_host[node])
                if row < 0:
                    return False
                slot = int(col._global_slots(np.asarray([row], np.int64))[0])
                return str(col.payloads.value(slot, "entity_type", "") or "").lower() == "class"
        return Info

    def search_rerank_hybrid(self, queries: np.ndarray, plans, reranker, limit: int, dfilt, relation: str):
        """Per 64 queries: the search (left on the device), the primaries of every query as one-node source sets of one BFS per
        (relation, direction, hops) on the one stream, ``crh_graph_list``, the kept representative rows, ``crh_graph_candidates``,
        the gathers and ``crh_rerank_hybrid`` -- the host sees the finished tables.  Returns per batch ``(output, slots [nq, k],
        scores, graph slots [nq, G], graph nodes [nq, G], declined)``; ``declined[q]`` (count -1, or a graph list that does not fit
        CRH_RR_MAX_HYBRID beside the hits) holds the query's graph lists ``[(role, node, depth)]`` for the host ranker."""
        import torch
        from .engine_helpers import plan_graph_roles
        from .ranking.device import graph_candidates, segment_table
        graph, _ = self._graph_ready(relation)
        stream = self.shards._stream()
        dev = torch.device("cuda", self._device)
        node_rows, node_rows_host = self.graph_node_rows()
        info = self._graph_role_info()
        width = 50                                                       # MAX_RESULTS_PER_QUERY: the widest list a walk asks for
        out = []
        for a in range(0, len(plans), ffi.GRAPH_MAX_QUERIES):
            part_plans = plans[a:a + ffi.GRAPH_MAX_QUERIES]
            nq = len(part_plans)
            if dfilt is not None and limit > 0:
                s, r = self.shards.search_device(torch.from_numpy(np.ascontiguousarray(queries[a:a + nq])).to(dev), limit, dfilt)
            else:
                s = torch.full((nq, max(limit, 0)), float("-inf"), dtype=torch.float32, device=dev)
                r = torch.full((nq, max(limit, 0)), -1, dtype=torch.int64, device=dev)
            k = int(r.shape[1])
            roles = [plan_graph_roles(p, info) for p in part_plans]
            groups: dict[tuple, list] = {}                               # (relation, direction, hops) -> [(query, walk)]
            for q, rp in enumerate(roles):
                for w in rp.walks:
                    groups.setdefault((w.relation, w.direction, w.hops), []).append((q, w))
            per_query = [[(ffi.ROLE_PRIMARY, v, -1, 0) for v in rp.primaries] for rp in roles]
            lists_n, lists_d, n_lists = [], [], 0
            for (rel_name, direction, hops), members in groups.items():
                rel = list(self._graph_rel).index(rel_name)
                for b in range(0, len(members), ffi.GRAPH_MAX_QUERIES):   # one bit per (query, primary), 64 bits per BFS
                    chunk = members[b:b + ffi.GRAPH_MAX_QUERIES]
                    graph.bfs(rel, direction, [[w.source] for _, w in chunk], hops, include_self=False, stream=stream)
                    nodes, depth, _ = graph.list(width, first_level=1, stream=stream)
                    lists_n.append(nodes.clone())
                    lists_d.append(depth.clone())
                    for i, (q, w) in enumerate(chunk):
                        per_query[q].append((w.role, -1, n_lists + i, min(w.limit, width)))
                    n_lists += len(chunk)
            segs, G_all = segment_table(per_query)
            G = max(0, min(G_all, ffi.RR_MAX_HYBRID - k))
            ln = torch.cat(lists_n) if lists_n else None
            ld = torch.cat(lists_d) if lists_d else None
            table = graph_candidates(segs, nq, G, node_rows, ln, ld, stream=stream) if G else None
            g_cols = self.gather_side(table.row) if G else None
            g_rich = None
            if G:
                rich = self.richness_columns()
                for sh in self.shards.owned:
                    part = rich[sh].gather(table.row, row_base=sh * SHARD_STRIDE, stream=stream)
                    g_rich = part if g_rich is None else g_rich + part
            res = reranker.rank(table, g_cols, g_rich, s if k else None, r if k else None, self.gather_side(r) if k else None, part_plans,
                                stream=stream)
            g_rows = _host(table.row) if G else np.zeros((nq, 0), np.int64)
            g_nodes = _host(table.node) if G else np.zeros((nq, 0), np.int32)
            declined = {}
            too_long = [q for q in range(nq) if sum(1 if n >= 0 else t for _, n, _, t in per_query[q]) > G]
            for q in sorted(set(too_long) | {q for q in range(nq) if res.count[q] < 0}):
                res.count[q] = -1
                ln_h, ld_h = (_host(ln), _host(ld)) if ln is not None else (None, None)
                entries = []
                for _, role, node, list_row, take in (sg for sg in segs if sg[0] == q):
                    found = [(node, 0)] if node >= 0 else list(zip(ln_h[list_row][:take], ld_h[list_row][:take]))
                    entries += [(role, int(v), int(d)) for v, d in found if v >= 0 and node_rows_host[int(v)] >= 0]
                declined[q] = entries
            out.append((res, self._global_slots(_host(r)) if k else np.zeros((nq, 0), np.int64), _host(s), self._global_slots(g_rows), g_nodes, declined))
        return out

    def _graph_names_of(self, nodes, depth) -> list[dict[str, Any]]:
        return [{"name": self._graph_names[int(v)], "depth": int(d)} for v, d in zip(nodes, depth) if v >= 0]

    def graph_neighbors(self, name_sets, direction: str, relation: str, max_hops: int, limit: int, include_self: bool, match: str) -> list[dict[str, Any]]:
        """Per name set: the nodes reached within ``max_hops`` as ``{"hits": [{"name", "depth"}], "count", "unresolved"}``, in
        (depth, node id) order; 64 sets per BFS."""
        if direction not in graph_mod.DIRECTIONS:
            raise ValueError(f"graph direction {direction!r} is not one of {', '.join(graph_mod.DIRECTIONS)}")
        if isinstance(max_hops, bool) or not isinstance(max_hops, (int, np.integer)) or not 1 <= int(max_hops) <= ffi.GRAPH_MAX_HOPS:
            raise ValueError(f"max_hops must be an int in 1..{ffi.GRAPH_MAX_HOPS}, not {max_hops!r}")
        if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)) or limit < 0:
            raise ValueError(f"limit must be a non-negative int, not {limit!r}")
        graph, rel = self._graph_ready(relation)
        resolved = [graph_mod.resolve(names, self._graph_code, self._graph_names, match) for names in name_sets]
        stream = self.shards._stream()
        out = []
        for a in range(0, len(resolved), ffi.GRAPH_MAX_QUERIES):
            part = resolved[a:a + ffi.GRAPH_MAX_QUERIES]
            graph.bfs(rel, direction, [ids for ids, _ in part], int(max_hops), include_self=include_self, stream=stream)
            nodes, depth, count = (_host(t) for t in graph.list(int(limit), first_level=0 if include_self else 1, stream=stream))
            out += [{"hits": self._graph_names_of(nodes[q], depth[q]), "count": int(count[q]), "unresolved": missing}
                    for q, (_, missing) in enumerate(part)]
        return out

    def call_chain(self, source: str, target: str, relation: str, max_hops: int) -> list[str] | None:
        """One shortest chain ``source -> ... -> target`` along ``relation`` of at most ``max_hops`` edges, as names; None when
        there is none or a name is no node.  Among equally short chains, every step back from the target takes the node that
        ``set_graph_edges`` saw first."""
        if isinstance(max_hops, bool) or not isinstance(max_hops, (int, np.integer)) or not 1 <= int(max_hops) <= ffi.GRAPH_MAX_HOPS:
            raise ValueError(f"max_hops must be an int in 1..{ffi.GRAPH_MAX_HOPS}, not {max_hops!r}")
        graph, rel = self._graph_ready(relation)
        a, b = self._graph_code.get(source), self._graph_code.get(target)
        if a is None or b is None:
            return None
        stream = self.shards._stream()
        graph.bfs(rel, "callees", [[a]], int(max_hops), include_self=True, stream=stream)
        nodes = _host(graph.path(rel, "callees", 0, b, stream=stream))
        return [self._graph_names[int(v)] for v in nodes] or None

    def call_chains(self, pairs, relation: str, max_hops: int, limit: int, must_pass: bool, match: str) -> list[dict[str, Any]]:
        """Per ``(source or names, target)`` pair: how many shortest chains lead from the source set to the target, the first
        ``limit`` of them and the nodes no chain of at most ``max_hops`` edges can avoid -- see ``HipVectorStore.call_chains``.
        64 pairs per pass: one BFS, ``crh_graph_sigma``, ``crh_graph_chains``; then the (pair, interior node of chain 0)
        candidates, 64 per ``crh_graph_bfs_avoiding``, of which the host reads the targets' finished bits only."""
        if isinstance(max_hops, bool) or not isinstance(max_hops, (int, np.integer)) or not 1 <= int(max_hops) <= ffi.GRAPH_MAX_HOPS:
            raise ValueError(f"max_hops must be an int in 1..{ffi.GRAPH_MAX_HOPS}, not {max_hops!r}")
        if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)) or not 0 <= int(limit) <= ffi.GRAPH_MAX_CHAINS:
            raise ValueError(f"limit must be an int in 0..{ffi.GRAPH_MAX_CHAINS}, not {limit!r}")
        graph, rel = self._graph_ready(relation)
        names, hops = self._graph_names, int(max_hops)
        resolved = []
        for pair in pairs:
            if not isinstance(pair, (tuple, list)) or len(pair) != 2 or not isinstance(pair[1], str):
                raise ValueError(f"a chain is asked for by a (source or names, target) pair, not {pair!r}")
            src, missing = graph_mod.resolve(pair[0], self._graph_code, names, match)
            dst, gone = graph_mod.resolve([pair[1]], self._graph_code, names, match)
            if len(dst) > 1:
                raise ValueError(f"target {pair[1]!r} names {len(dst)} nodes ({', '.join(names[i] for i in dst[:4])}, ...): name one")
            resolved.append((src, dst[0] if dst else -1, missing + gone))
        stream = self.shards._stream()
        out = []
        for a in range(0, len(resolved), ffi.GRAPH_MAX_QUERIES):
            part = resolved[a:a + ffi.GRAPH_MAX_QUERIES]
            graph.bfs(rel, "callees", [src for src, _, _ in part], hops, include_self=True, stream=stream)
            graph.sigma(rel, "callees", stream=stream)
            nodes, length, count = (_host(t) for t in graph.chains(rel, "callees", [t for _, t, _ in part], max(int(limit), 1), stream=stream))
            count = count.view(np.uint64)
            found = [[] for _ in part]
            if must_pass:
                cand = [(q, int(v)) for q in range(len(part)) for v in nodes[q, 0, 1:max(int(length[q]) - 1, 1)]]
                for b in range(0, len(cand), ffi.GRAPH_MAX_QUERIES):
                    some = cand[b:b + ffi.GRAPH_MAX_QUERIES]
                    graph.bfs_avoiding(rel, "callees", [part[q][0] for q, _ in some], hops, [v for _, v in some], include_self=True, stream=stream)
                    reached = graph.seen_bits([part[q][1] for q, _ in some])
                    for (q, v), still in zip(some, reached):
                        if not still:
                            found[q].append(v)
            for q, (_, _, missing) in enumerate(part):
                n, c = int(length[q]), int(count[q])
                out.append({"count": c, "saturated": c == ffi.GRAPH_SATURATED, "length": n - 1 if n else None,
                            "chains": [[names[int(v)] for v in nodes[q, r, :n]] for r in range(min(c, int(limit)))],
                            "must_pass": [names[v] for v in found[q]], "unresolved": missing})
        return out

    def matching_slots(self, filters: dict[str, Any] | None, limit: int | None = None, must_not: dict[str, Any] | None = None) -> np.ndarray:
        """Alive slots matching every condition, in insertion order -- resolved on the device from the code columns."""
        dfilt = self.device_filters(filters, must_not)
        if dfilt is None:
            return np.zeros((0,), np.int64)
        sh, lo = self.shards.match_rows(dfilt, sum(self.shards.rows) if limit is None else limit)
        slots = np.sort(self.slots_of(sh, lo))
        return slots if limit is None else slots[:limit]

    # -- mutation
    def remove_slots(self, slots) -> None:
        slots = np.asarray(slots, dtype=np.int64)
        if slots.size:
            self.shards.tombstone(*self.rows_of(slots))

    def delete(self, filters: dict[str, Any], must_not: dict[str, Any] | None = None) -> int:
        """client.py:159-169: every point matching the AND of the conditions.  An empty filter matches every point, as
        ``Filter(must=[])`` does."""
        if has_graph_condition(filters, must_not):
            raise ValueError(f"delete takes no {GRAPH_KEY!r} condition: fetch the matching points (search with query_vector=None) and delete by id or file")
        if has_text_condition(filters, must_not):
            raise ValueError("delete takes no text condition ({'contains': ...} / {'matches': ...} / {'fuzzy': ...}): fetch the matching points (search_text) and delete by id or file")
        dfilt = self.device_filters(filters, must_not)
        if dfilt is None:
            return 0
        if not dfilt:
            slots = self.matching_slots(None)
            self.remove_slots(slots)
            n = int(slots.size)
        else:
            n = self.shards.tombstone_filter(dfilt)
        self.maybe_compact()
        return n

    def upsert(self, ids, vectors, payloads, preprocessed: bool = False, texts=None, embed=None) -> None:
        """``vectors``: list of float lists (what the reference passes), a float32 ndarray [n, dim], or a CUDA tensor [n, dim]
        on this collection's device (no host round trip) -- or None with ``texts`` and ``embed`` (``embed(list[str])`` -> ndarray /
        CUDA tensor [m, dim]): the rows are routed first and every process embeds only the texts of the shards it owns, straight
        into them (embeddings/indexer.py:66-85 with the embedding work sharded like the rows: SURVEY 8(e), embed row)."""
        n = len(ids)
        if n == 0:
            return
        lazy = vectors is None
        if lazy:
            if texts is None or embed is None or len(texts) != n:
                raise ValueError("upsert without vectors needs one text per id and an embed callable")
            vecs, on_dev = None, False
        else:
            on_dev = not isinstance(vectors, (list, tuple, np.ndarray)) and bool(getattr(vectors, "is_cuda", False))
            vecs = vectors if on_dev else np.asarray(vectors, dtype=np.float32)
            if vecs.ndim != 2 or int(vecs.shape[0]) != n:
                raise ValueError(f"upsert needs equally many ids, vectors and payloads (got {n}, {tuple(vecs.shape)}, {len(payloads)})")
            if int(vecs.shape[1]) != self.shards.dim:
                raise ValueError(f"vector dimension {vecs.shape[1]} does not match the collection's {self.shards.dim}")
        if len(payloads) != n:
            raise ValueError(f"upsert needs equally many ids, vectors and payloads (got {n} ids, {len(payloads)} payloads)")
        ids = [str(i) for i in ids]
        last = dict(zip(ids, range(n)))                       # a repeated id inside one call: last one wins
        if len(last) != n:
            keep = sorted(last.values())
            ids, payloads = [ids[i] for i in keep], [payloads[i] for i in keep]
            if lazy:
                texts = [texts[i] for i in keep]
            else:
                vecs = vecs[keep] if not on_dev else vecs[ffi_index_tensor(vecs, keep)]
            n = len(keep)
        n0 = self.payloads.n
        saved_next = self.shards._next_block
        shard = self.shards.route(n)
        if self.partial:                                      # the text of rows other ranks own stays with them
            owned = np.isin(shard, self.shards.owned)
            stored = [p if o else {k: ("" if k in _TEXT_COLUMNS and isinstance(v, str) else v) for k, v in p.items()} for p, o in zip(payloads, owned)]
        else:
            stored = payloads
        self.payloads.extend(stored)
        orphans: dict[int, tuple[int, int]] = {}
        try:
            codes = self.device_codes(n0, n0 + n)
            if lazy:
                per_shard = {}
                embed_failure = None
                try:
                    for sh in self.shards.owned:
                        sel = np.flatnonzero(shard == sh)
                        if sel.size:
                            v = embed([texts[i] for i in sel])
                            v = v if bool(getattr(v, "is_cuda", False)) else np.asarray(v, dtype=np.float32)
                            if v.ndim != 2 or int(v.shape[0]) != sel.size or int(v.shape[1]) != self.shards.dim:
                                raise ValueError(f"embed returned {tuple(v.shape)} for {sel.size} texts of dimension {self.shards.dim}")
                            per_shard[sh] = v
                except Exception as e:  # noqa: BLE001 -- carried into the append's agreement (below), re-raised from there
                    embed_failure = e
                dev_rows = [v for v in per_shard.values() if not isinstance(v, np.ndarray)]
                if embed_failure is not None:
                    # one rank's encoder failed (a bad text, out of memory): the others are already on their way into the append's
                    # agreement collective -- this rank joins it with its failure, so that everyone rolls back and raises together
                    self.shards.append({}, codes, preprocessed, shard=shard, failure=embed_failure)
                    raise embed_failure          # (not reached: append re-raises it)
                if dev_rows:
                    import torch
                    per_shard = {sh: (v.contiguous() if v.dtype == torch.float32 else v.float().contiguous()) if not isinstance(v, np.ndarray) else v
                                 for sh, v in per_shard.items()}
                    _, local = self.shards.append(per_shard, codes, preprocessed, stream=ffi.current_stream(dev_rows[0].device), shard=shard)
                    torch.cuda.current_stream(dev_rows[0].device).synchronize()
                else:
                    _, local = self.shards.append(per_shard, codes, preprocessed, shard=shard)
            elif on_dev:
                import torch
                # (the caller's tensor comes from the device's default stream -- the encoder's --, this job may run on the store's own)
                torch.cuda.current_stream(vecs.device).wait_stream(torch.cuda.default_stream(vecs.device))
                vecs = vecs.contiguous() if vecs.dtype == torch.float32 else vecs.float().contiguous()
                _, local = self.shards.append(vecs, codes, preprocessed, stream=ffi.current_stream(vecs.device), shard=shard)
                torch.cuda.current_stream(vecs.device).synchronize()      # the caller may free / reuse its tensor right away
            else:
                _, local = self.shards.append(vecs, codes, preprocessed, shard=shard)
        except AppendFailed as e:
            # some shards took their rows before another refused: those rows are dead on the device and have no slot -- the
            # maps step over them (-1), the tables go back
            self.payloads.truncate(n0)
            if self.shards.ns > 1:
                for sh, (_, m) in e.done.items():
                    self.slot_of[sh] = np.concatenate([self.slot_of[sh], np.full((m,), -1, np.int64)])
            else:
                raise RuntimeError("a one-shard collection cannot lose an append half-way") from e
            # the orphans are dead on the device already: reclaim them now, so that no later state (a snapshot, the side columns of
            # the re-rank) ever holds a row without a slot.  Every rank is here (the append agreed on the failure), so the
            # compaction's collectives line up.  Should the compaction itself fail, the maps above keep the collection usable
            # and save() tries again.
            try:
                self.compact()
            except Exception as ce:  # noqa: BLE001
                raise e.cause from ce
            self.shards._next_block = saved_next              # nothing of the call is left: the next rows are routed as if it had not been made
            raise e.cause
        except Exception:
            self.payloads.truncate(n0)                        # nothing was stored: the tables go back to where they were
            self.shards._next_block = saved_next
            raise
        replaced = self.ids.extend(ids)                       # slots these ids occupied before (-1: new)
        if self.shards.ns > 1:
            self.row_shard = np.concatenate([self.row_shard, shard])
            self.row_local = np.concatenate([self.row_local, local])
            for s in range(self.shards.ns):
                m = shard == s
                if m.any():
                    self.slot_of[s] = np.concatenate([self.slot_of[s], n0 + np.flatnonzero(m)])
        stale = replaced[replaced >= 0]
        if stale.size:
            self.remove_slots(stale)                          # (a slot that is already dead is tombstoned again: the device ignores it)
            self.maybe_compact()

    def device_codes(self, lo: int, hi: int):
        """[hi - lo, columns] int32 of the slots [lo, hi) as the index stores them: the dictionary codes of ``keys``, then the
        values of ``numeric_keys`` (None for a collection without columns)."""
        if not self.keys and not self.numeric_keys:
            return None
        codes = self.payloads.device_codes(self.keys, lo, hi)
        if not self.numeric_keys:
            return codes
        return np.ascontiguousarray(np.concatenate([codes, self.payloads.numeric_codes(self.numeric_keys, lo, hi)], axis=1))

    def hit(self, slot: int, score: float) -> dict[str, Any]:
        return {"id": self.ids.get(slot), "score": score, "payload": self.payloads_of([slot])[0]}

    def payloads_of(self, slots) -> list[dict[str, Any]]:
        """The stored payload dictionaries of ``slots`` (every process passes the same list).  With one process per shard only a
        row's OWNER holds its text: each rank serialises the payloads of the slots it owns and ONE byte exchange completes the
        list everywhere (``ShardSet.exchange_bytes``: two tensor all-reduces)."""
        slots = [int(t) for t in slots]
        if not self.partial:
            return [self.payloads.get(t) for t in slots]
        import json
        mine = set(self.shards.owned)
        # only the TEXT fields travel (everything else is replicated and keeps its Python type: tuples, None, numbers)
        local = [self.payloads.get(t) for t in slots]
        parts = [json.dumps({k: p[k] for k in _TEXT_COLUMNS if isinstance(p.get(k), str)}, ensure_ascii=False).encode("utf-8", "surrogatepass")
                 if int(self.row_shard[t]) in mine else None for t, p in zip(slots, local)]
        out = []
        for p, b in zip(local, self.shards.exchange_bytes(parts)):
            p = dict(p)
            p.update(json.loads(b.decode("utf-8", "surrogatepass")))
            out.append(p)
        return out

    def hits(self, slots, scores) -> list[dict[str, Any]]:
        """Hit dictionaries of a flat list of (slot, score) pairs, payloads fetched together."""
        slots = [int(t) for t in slots]
        pays = self.payloads_of(slots)
        return [{"id": self.ids.get(t), "score": float(sc), "payload": p} for t, sc, p in zip(slots, scores, pays)]

    def search(self, queries: np.ndarray, limit: int, dfilt) -> tuple[np.ndarray, np.ndarray]:
        """(scores [nq, limit], slots [nq, limit]); -1 slots are padding."""
        scores, shard, local = self.shards.search(queries, limit, dfilt)
        return scores, self.slots_of(shard, local)

    def search_range(self, queries: np.ndarray, limit: int, thresholds, dfilt, counts: bool = True):
        """The same under a score threshold per query (``ShardSet.search_range``): the lists cut after their last in-range hit,
        and ``counts`` int64 [nq] -- how many rows are in range, however many -- or None."""
        scores, shard, local, totals = self.shards.search_range(queries, limit, thresholds, dfilt, counts)
        return scores, self.slots_of(shard, local), totals

    def facet_column(self, key: str) -> int:
        """The device column of a key whose values can be counted: one of the dictionary keys.  ``ValueError`` naming them for a
        numeric key (its column holds the values themselves, not codes: no histogram of lines in this version) and for any other."""
        if key in self.numeric_keys:
            raise ValueError(f"payload key {key!r} holds numbers: a facet counts the values of a dictionary key "
                             f"(filterable: {', '.join(self.keys)})")
        return self._column(key)

    def facet(self, key: str, limit: int, dfilt, queries: np.ndarray | None = None, thresholds=None) -> list[dict[str, Any]]:
        """Per query -- one without ``queries`` -- the values of ``key`` among the rows that count (``ShardSet.facet``; DESIGN.md
        3.23): ``{"hits": [{"value", "count"}], "values", "total", "missing"}``.  The device keeps ONE code (0) for "the key is
        absent" and "its value is None", as the filters do: those rows are counted under the value None -- the rows a filter
        ``{key: None}`` selects.  ``missing`` counts rows whose column holds -1, which no upsert of this store writes."""
        book = self.payloads.cols[key]
        n_bins = len(book.values) + 1                                       # code = position in `values` + 1; 0: no value
        codes, counts, sel, info = self.shards.facet(dfilt, self.facet_column(key), n_bins, limit, queries, thresholds)
        if info[:, 2].any():
            raise RuntimeError(f"facet of {key!r}: {int(info[:, 2].sum())} rows carry a code beyond the dictionary's {n_bins} entries")
        return [{"hits": [{"value": None if c == 0 else book.values[c - 1], "count": int(n)} for c, n in zip(codes[q].tolist(), counts[q].tolist()) if c >= 0],
                 "values": int(sel[q, 0]), "total": int(sel[q, 1]), "missing": int(info[q, 1])} for q in range(codes.shape[0])]

    def search_multi(self, queries: np.ndarray, limit: int, class_dfilts, query_class) -> tuple[np.ndarray, np.ndarray]:
        """The same for a batch whose queries carry different filters: query ``i`` under ``class_dfilts[query_class[i]]``."""
        scores, shard, local = self.shards.search_multi(queries, limit, class_dfilts, query_class)
        return scores, self.slots_of(shard, local)

    def search_mmr(self, queries: np.ndarray, limit: int, candidates: int, diversity: float, dfilt) -> tuple[np.ndarray, np.ndarray]:
        """The same for the diversity-aware top-k: the ``limit`` MMR picks among the ``candidates`` best hits of every query
        (``ShardSet.search_mmr``); scores are the picks' cosines."""
        scores, shard, local = self.shards.search_mmr(queries, limit, candidates, diversity, dfilt)
        return scores, self.slots_of(shard, local)

    @staticmethod
    def _exclude_codes(dfilt: list[tuple], col: int, codes) -> list[tuple]:
        """``dfilt`` + "column ``col`` is none of ``codes``": merged into the filter's own negated set on that column when it
        has one, a new condition otherwise (``ValueError`` when that would be one more than the device takes)."""
        out = list(dfilt)
        for i, cond in enumerate(out):
            if ffi.is_set_condition(cond) and len(cond) == 3 and cond[2] and cond[0] == col:
                out[i] = (col, sorted(set(int(c) for c in cond[1]) | set(codes)), True)
                return out
        if len(out) >= ffi.MAX_FILTERS:
            raise ValueError(f"the grouped search needs one more filter condition than the {ffi.MAX_FILTERS} the device takes "
                             f"(exclude the saturated groups of {col!r}): use fewer conditions")
        out.append((col, sorted(set(codes)), True))
        return out

    def search_grouped(self, queries: np.ndarray, limit: int, candidates: int, group_by: str, group_size: int, dfilt) -> tuple[np.ndarray, np.ndarray]:
        """(scores [nq, limit], slots [nq, limit]) of the EXACT grouped top-``limit``: the first ``limit`` rows,
        in the order of the plain search, whose rank in their ``group_by`` group is below ``group_size``; rows without the key
        (or with the value None: the device column holds code 0 for both) belong to no group and are never capped.  One round of ``ShardSet.search_grouped`` answers a query whose capped walk reached ``limit`` inside
        the candidate list or whose list came back short (the filter has no more rows).  The others go on, together, at
        ``MAX_K`` candidates; what is still incomplete then takes exclusion rounds, one query at a time: the groups that
        reached ``group_size`` keep those rows (a group's best ones) and are excluded from the next search by a negated set
        condition, until the remembered rows and the new list's walk hold ``limit`` rows or the new list is short.  Every such
        round with a full list saturates at least one more group, so it ends -- after one round per group at the worst.
        ``self.group_rounds`` counts the queries asked, those that needed the second round, and the exclusion rounds run."""
        col = self._column(group_by)
        nq = int(queries.shape[0])
        out_s, out_r = np.full((nq, limit), -np.inf, np.float32), np.full((nq, limit), -1, np.int64)
        stats = self.group_rounds
        stats["queries"] += nq
        todo = np.arange(nq)
        last: dict[int, tuple] = {}                 # query -> (scores, rows, codes) of its incomplete MAX_K-candidate round
        for rnd, c in enumerate((candidates, ffi.MAX_K)):
            if rnd == 1:
                if candidates >= ffi.MAX_K:          # (round 1 already ran at MAX_K)
                    break
                stats["round2"] += int(todo.size)
            s, r, g, info = self.shards.search_grouped(queries[todo], limit, c, col, group_size, dfilt, ungrouped=NONE_CODE)
            done = (info[:, 0] >= limit) | (info[:, 1] < c)
            out_s[todo[done]], out_r[todo[done]] = s[done], r[done]
            if c >= ffi.MAX_K:
                last = {int(qi): (s[i], r[i], g[i]) for i, qi in enumerate(todo) if not done[i]}
            todo = todo[~done]
            if not todo.size:
                break
        for qi in todo:
            s, r, g = last[int(qi)]
            held: list[tuple[float, int]] = []      # the rows of the excluded groups: (score, global row)
            excluded: set[int] = set()
            while True:
                real = r >= 0                       # (an incomplete list kept fewer than limit rows: all of them are here)
                codes, counts = np.unique(g[real & (g >= 0)], return_counts=True)
                full = set(int(v) for v in codes[counts >= group_size]) - excluded
                if not full:                        # cannot happen (see the docstring); never loop on it
                    raise RuntimeError("grouped search: a full candidate list saturated no group")
                sat = real & np.isin(g, sorted(full))
                held += list(zip(s[sat].tolist(), r[sat].tolist()))
                excluded |= full
                stats["exclusion"] += 1
                s, r, g, info = (a[0] for a in self.shards.search_grouped(queries[qi:qi + 1], limit, ffi.MAX_K, col, group_size,
                                                                          self._exclude_codes(dfilt, col, excluded), ungrouped=NONE_CODE))
                if int(info[1]) < ffi.MAX_K or len(held) + int(info[0]) >= limit:
                    break
            real = r >= 0
            both = sorted(held + list(zip(s[real].tolist(), r[real].tolist())), key=lambda t: (-t[0], t[1]))[:limit]
            out_s[qi, :len(both)] = np.asarray([t[0] for t in both], np.float32)       # (a Python float holds an f32 exactly)
            out_r[qi, :len(both)] = [t[1] for t in both]
        return out_s, self._global_slots(out_r)

    def search_spans(self, queries: np.ndarray, limit: int, candidates: int, permille: int, dfilt) -> tuple[np.ndarray, np.ndarray]:
        """(scores [nq, limit], slots [nq, limit]) of the EXACT overlap-free top-``limit``: the first ``limit``
        rows, in the order of the plain search, that repeat at most ``permille`` thousandths of the shorter span of any better
        KEPT row of their file; rows without a file, a start line or an end line are always kept.  Whether a row is kept
        depends on the rows before it only, so the walk over an exact top-c list is a prefix of the corpus-wide walk.  Round 1
        runs at ``candidates``; a query is done when its walk kept ``limit`` rows or its list came back short (the filter has
        no more rows); the others go on together at ``MAX_K``; what is still short then is returned SHORT -- its kept hits are
        exactly the first kept hits of the corpus-wide walk, only fewer than ``limit``.  ``self.span_rounds`` counts the queries
        asked, those sent to round 2 and those answered short."""
        if not self.numeric_keys:
            raise ValueError(f"collection {self.name!r} keeps no line numbers on the device: max_overlap needs them")
        cols = (self._column("file_path"), self._numeric_column("start_line"), self._numeric_column("end_line"))
        nq = int(queries.shape[0])
        out_s, out_r = np.full((nq, limit), -np.inf, np.float32), np.full((nq, limit), -1, np.int64)
        stats = self.span_rounds
        stats["queries"] += nq
        todo = np.arange(nq)
        for rnd, c in enumerate((candidates, ffi.MAX_K)):
            if rnd == 1:
                stats["round2"] += int(todo.size)
            s, r, info = self.shards.search_spans(queries[todo], limit, c, cols, permille, dfilt, no_file=NONE_CODE)
            done = (info[:, 0] >= limit) | (info[:, 1] < c)
            last = c >= ffi.MAX_K                    # (no deeper round: what is not done comes back short)
            take = done | last
            out_s[todo[take]], out_r[todo[take]] = s[take], r[take]
            if last:
                stats["short"] += int((~done).sum())
            todo = todo[~take]
            if not todo.size:
                break
        return out_s, self._global_slots(out_r)

    def search_fused(self, queries: np.ndarray, limit: int, candidates: int, dfilt, method: str, rrf_k: int, weights, live=None):
        """The fused top-``limit`` of every logical query of ``queries`` [nq, m, dim] (``ShardSet.search_fused``):
        (slots i64, fused f32, cos f32, lists i32), each [nq, limit]; -1 slots are padding."""
        rows, fused, cos, lists, _, _ = self.shards.search_fused(queries, limit, candidates, dfilt, method, rrf_k, weights, live)
        return self._global_slots(rows), fused, cos, lists

    def example_rows(self, slots: np.ndarray) -> np.ndarray:
        """GLOBAL rows of a table of example slots (-1 stays -1)."""
        slots = np.asarray(slots, np.int64)
        shard, local = self.rows_of(np.maximum(slots, 0))
        return np.where(slots >= 0, np.asarray(shard, np.int64) * SHARD_STRIDE + np.asarray(local, np.int64), -1)

    def recommend(self, slots: np.ndarray, P: int, N: int, limit: int, candidates: int, dfilt, strategy: str, n_pos=None, n_neg=None):
        """Recommend by example for ``nq`` logical queries whose examples are the slots ``slots`` [nq, P + N]
        (positives first, -1 for an unused slot): (slots i64, score f32, neg f32, best i32), each [nq, limit]; -1 slots are
        padding.  ``"average"`` is one round at ``limit + P + N`` candidates.  ``"best"`` holds the rounds: round 1 runs at
        ``candidates`` per positive; a query whose settled prefix reaches ``limit``, or none of whose lists came back full (the
        filter has no more rows), is done; the others go on together at ``MAX_K // P``; what is still unsettled then comes back
        SHORT -- its settled prefix only, every returned hit the exact hit of its position.  ``self.recommend_rounds`` counts
        the queries asked, those sent to round 2 and those answered short."""
        ex = self.example_rows(slots)
        nq = int(ex.shape[0])
        stats = self.recommend_rounds
        stats["queries"] += nq
        out = (np.full((nq, limit), -1, np.int64), np.full((nq, limit), -np.inf, np.float32), np.full((nq, limit), -np.inf, np.float32),
               np.full((nq, limit), -1, np.int32))
        if strategy == "average":
            c = limit + P + N
            rows, score, neg, best, _, _ = self.shards.recommend(ex, P, N, min(limit, c), c, dfilt, strategy, n_pos, n_neg)
            for o, v in zip(out, (rows, score, neg, best)):
                o[:, :v.shape[1]] = v
        else:
            todo = np.arange(nq)
            deep = ffi.MAX_K // P
            for rnd, c in enumerate((candidates, deep)):
                if rnd == 1:
                    if candidates >= deep:            # (round 1 already ran as deep as a round can)
                        stats["short"] += int(todo.size)
                        break
                    stats["round2"] += int(todo.size)
                k = min(limit, P * c)
                sub = lambda a: None if a is None else np.asarray(a)[todo]   # noqa: E731
                rows, score, neg, best, info, full = self.shards.recommend(ex[todo], P, N, k, c, dfilt, strategy, sub(n_pos), sub(n_neg))
                settled = np.minimum(info[:, 1], k)
                done = (info[:, 1] >= limit) | ~full
                take = done if rnd == 0 and candidates < deep else np.ones_like(done)
                for i in np.flatnonzero(take):
                    w = int(settled[i])
                    for o, v in zip(out, (rows, score, neg, best)):
                        o[todo[i], :w] = v[i, :w]
                if rnd == 1:
                    stats["short"] += int((~done).sum())
                todo = todo[~done]
                if not todo.size:
                    break
        return (self._global_slots(out[0]),) + out[1:]

    # -- keyword search
    def _lex_ready(self) -> dict[int, Any]:
        """The forward indexes of the owned shards, brought up to date: rows appended since the last lexical call are cut into
        terms (``lexical.terms_batch``) and appended.  A collection that is never searched lexically never comes here."""
        if self.shards.backend == "dist":
            raise VectorStoreError("lexical search is not available with shard_backend='dist' yet (its collection statistics need "
                                   "an all-reduce)")
        for s in self.shards.owned:
            lex = self._lex.get(s)
            if lex is None:
                lex = self._lex[s] = ffi.Lex(capacity_rows=self.shards.rows[s], device=self._device)
            have, want = lex.count()[0], self.shards.rows[s]
            for a in range(have, want, 65536):
                b = min(want, a + 65536)
                slots = np.arange(a, b) if self.shards.ns == 1 else self.slot_of[s][a:b]
                texts = [lexical.point_text(self.payloads.get(int(t))) if t >= 0 else b"" for t in slots]   # (-1: a dead row without a slot)
                lex.append(*lexical.terms_batch(texts))
        return self._lex

    def _lex_drop(self) -> None:
        for lex in self._lex.values():
            lex.close()
        self._lex, self._lex_df = {}, None

    def _lex_weights(self, lex: dict, term_lists) -> tuple[list, list, np.float32]:
        """Per query ``(term ids, idf)`` and ``avgdl``: the statistics are those of the ALIVE rows of the whole collection
        (Lucene's and Qdrant's convention: not of the filtered subset), kept until the next upsert, delete or compaction --
        only terms not counted yet go to ``crh_lex_stats``.  A text with more than 32 distinct terms keeps the 32 with the
        smallest df, ties to the lower id."""
        state = (tuple(self.shards.rows), self.shards.count()[1], self.compactions)
        if self._lex_df is None or self._lex_df[0] != state:
            self._lex_df = (state, {}, None, None)
        _, known, n_rows, sum_dl = self._lex_df
        every = np.unique(np.concatenate([np.zeros(0, np.uint32)] + [np.asarray(t, np.uint32) for t in term_lists]))
        new = np.asarray([t for t in every.tolist() if t not in known], np.uint32)
        if new.size or n_rows is None:
            df, n_rows, sum_dl = self.shards.lex_stats(lex, new)
            self.lex_stats_calls += 1
            known.update(zip(new.tolist(), df.tolist()))
            self._lex_df = (state, known, n_rows, sum_dl)
        queries, weights = [], []
        avgdl = np.float32(1.0)
        for t in term_lists:
            t = np.asarray(t, np.uint32)
            t, _ = lexical.rarest(t, [known[v] for v in t.tolist()])
            idf, avgdl = lexical.bm25_weights([known[v] for v in t.tolist()], n_rows, sum_dl)
            queries.append(t)
            weights.append(idf)
        return queries, weights, avgdl

    def search_lexical(self, texts, limit: int, dfilt, k1: float = 1.2, b: float = 0.75):
        """Exact BM25 top-``limit`` of every text: (scores f32 [nq, limit], slots i64 [nq, limit], counts i64 [nq]); -1 slots
        are padding, ``counts`` the rows that hold at least one of the text's terms under the filter, however many."""
        lex = self._lex_ready()
        queries, idf, avgdl = self._lex_weights(lex, [lexical.query_terms(t) for t in texts])
        scores, rows, counts = self.shards.lex_search(lex, queries, idf, limit, k1, b, float(avgdl), dfilt)
        return scores, self._global_slots(rows), counts

    def search_hybrid(self, vectors: np.ndarray, texts, limit: int, candidates: int, dfilt, rrf_k: int, weights, k1: float = 1.2, b: float = 0.75):
        """Dense + keyword under one filter, fused by reciprocal rank on the device (``ShardSet.search_hybrid``): per query the
        fused ``(slots, fused score, cosine or nan, lexical score or nan, lists bits)``, each [nq, limit].  The cosine and the
        BM25 score of a hit are looked up in the two candidate lists -- nan when that list did not hold the row."""
        lex = self._lex_ready()
        queries, idf, avgdl = self._lex_weights(lex, [lexical.query_terms(t) for t in texts])
        (rows, fused, _, lists, _, _), (ds, dr, ls, lr) = self.shards.search_hybrid(lex, vectors, queries, idf, limit, candidates, k1, b,
                                                                                     float(avgdl), dfilt, rrf_k, weights)
        def looked_up(cs, cr):
            out = np.full(rows.shape, np.nan, np.float32)
            for q in range(rows.shape[0]):
                where = {int(r): float(v) for r, v in zip(cr[q], cs[q]) if r >= 0}
                for j, r in enumerate(rows[q].tolist()):
                    if r in where:
                        out[q, j] = where[r]
            return out
        return self._global_slots(rows), fused, looked_up(ds, dr), looked_up(ls, lr), lists

    # -- compaction
    def maybe_compact(self) -> bool:
        rows, alive = self.shards.count()
        dead = rows - alive
        if self.compact_dead_fraction > 0 and dead >= self.compact_min_dead and dead >= self.compact_dead_fraction * rows:
            self.compact()
            return True
        return False

    def compact(self) -> int:
        """Reclaim the rows of deleted points on the device (``crh_index_compact``) and drop their ids / payloads from the host
        tables; returns the number of rows reclaimed.  Slots and rows are renumbered; ids, payloads, filters and search
        results are unchanged."""
        before = self.payloads.n
        maps = self.shards.compact()
        if self.shards.ns == 1:
            o2n = maps[0]
            keep = np.flatnonzero(o2n >= 0)
        else:
            new_local = np.full((before,), -1, np.int64)
            for s, o2n in maps.items():
                m = self.row_shard == s
                new_local[m] = o2n[self.row_local[m]]
            keep = np.flatnonzero(new_local >= 0)
            self.row_shard, self.row_local = self.row_shard[keep], new_local[keep]
            for s in range(self.shards.ns):
                m = np.flatnonzero(self.row_shard == s)
                so = np.empty((m.size,), np.int64)
                so[self.row_local[m]] = m
                self.slot_of[s] = so
        if keep.size != before:
            self.ids.compact(keep)
            self.payloads.compact(keep)
        moved = any(bool((o2n < 0).any()) for o2n in maps.values())      # (rows without a slot -- a half-way append -- count as well)
        if moved:
            for s, side in self._side.items():
                side.select(np.flatnonzero(maps[s][: side.rows] >= 0))
            self.compactions += 1
        self._lex_drop()                      # (derived: rebuilt from the payload tables on the next lexical call)
        self._text_drop()                     # (likewise: on the next text filter)
        self._graph_rows, self._graph_rows_state, self._graph_cache = {}, None, {}    # (the row -> node columns: on the next graph filter)
        return int(before - keep.size)

    # -- persistence
    def save(self, directory: str) -> None:
        """``directory``: the index image of every shard (``ffi.Index.save``: raw, mmap-able, verbatim) + the id and payload
        tables as raw arrays (``tables``) + ``collection.json`` (keys, shard layout, graph degrees).  Written next to the
        target and renamed over it, so a crash mid-save leaves the previous snapshot intact."""
        import json
        import shutil
        if any(bool((so < 0).any()) for so in self.slot_of):      # rows without a slot (a half-way append whose clean-up failed) never reach a snapshot
            self.compact()
        tmp = directory.rstrip("/") + ".tmp"
        primary = self.shards.rank in (None, 0)
        if primary:
            shutil.rmtree(tmp, ignore_errors=True)
            os.makedirs(tmp, exist_ok=True)
        self.shards.barrier()                                     # (every rank sees the directory before writing into it)
        self.shards.save(tmp)
        if self.partial:                                          # a rank's payload table holds the text of its own rows only: one table per rank
            sub = os.path.join(tmp, f"tables{self.shards.rank}")
            os.makedirs(sub, exist_ok=True)
            self.payloads.save(sub)
        if primary:
            self.ids.save(tmp)
            if not self.partial:
                self.payloads.save(tmp)
            self.row_shard.tofile(os.path.join(tmp, "rows.shard.i32"))
            self.row_local.tofile(os.path.join(tmp, "rows.local.i64"))
            # the call graph is not derivable from the payloads: its node names (a JSON list, in id order) and every relation's
            # edges (raw int32 [edges, 2] node ids) lie beside the tables, named by an optional "graph" entry of collection.json
            graph_meta = None
            if self._graph_rel:
                with open(os.path.join(tmp, "graph.names.json"), "w") as f:
                    json.dump(self._graph_names, f)
                graph_meta = {"names": "graph.names.json", "nodes": len(self._graph_names), "relations": []}
                for r, (rel, pairs) in enumerate(self._graph_rel.items()):
                    np.ascontiguousarray(pairs, dtype=np.int32).tofile(os.path.join(tmp, f"graph.{r}.edges.i32"))
                    graph_meta["relations"].append({"name": rel, "file": f"graph.{r}.edges.i32", "edges": int(len(pairs))})
                    loops = self._graph_self.get(rel)
                    if loops is not None and loops.size:                  # optional: the nodes that carried a self-loop (sorted int32)
                        np.ascontiguousarray(loops, dtype=np.int32).tofile(os.path.join(tmp, f"graph.{r}.self.i32"))
                        graph_meta["relations"][-1]["self"] = f"graph.{r}.self.i32"
            with open(os.path.join(tmp, "collection.json"), "w") as f:
                # format 4: says where the payload tables are ("text_tables": "per_rank" = tables{rank}/ hold the text of that
                # rank's rows only, written by one process per shard; "root" = one complete table)
                # format 5: "numeric_keys" -- the shards' codes.i32 hold len(keys) + len(numeric_keys) columns, the numeric ones last
                json.dump({"name": self.name, "keys": list(self.keys), "numeric_keys": list(self.numeric_keys), "format": 5,
                           "slots": self.payloads.n, "shards": self.shards.ns,
                           "shard_rows": list(self.shards.rows), "degrees": self._degrees,
                           "text_tables": "per_rank" if self.partial else "root", **({"graph": graph_meta} if graph_meta else {})}, f, default=repr)
        self.shards.barrier()
        if primary:
            shutil.rmtree(directory, ignore_errors=True)
            os.replace(tmp, directory)
        self.shards.barrier()

    def load(self, directory: str) -> None:
        import json
        with open(os.path.join(directory, "collection.json")) as f:
            meta = json.load(f)
        if list(meta["keys"]) != list(self.keys):
            raise ValueError(f"snapshot of {self.name} codes the payload keys {meta['keys']}, this store {list(self.keys)}")
        if int(meta.get("shards", 1)) != self.shards.ns:
            raise ValueError(f"snapshot of {self.name} has {meta.get('shards', 1)} shards, this store {self.shards.ns}")
        # format <= 4 knows no numeric columns: its codes.i32 hold len(keys) columns, and every imported chunk is widened with
        # the numeric ones, rebuilt from the payload table's int columns of the same rows (the tables are read first for that)
        snap_numeric = tuple(meta.get("numeric_keys", ())) if int(meta.get("format", 0)) >= 5 else ()
        if snap_numeric not in ((), self.numeric_keys):
            raise ValueError(f"snapshot of {self.name} stores the numeric keys {list(snap_numeric)}, this store {list(self.numeric_keys)}")
        widen = snap_numeric != self.numeric_keys
        if not widen:
            self.shards.load(directory)
        n = int(meta["slots"])
        self.ids.load(directory, n)
        per_rank = os.path.join(directory, f"tables{self.shards.rank}") if self.partial else None
        layout = meta.get("text_tables") or ("per_rank" if per_rank and os.path.isdir(per_rank) else "root")
        if layout == "per_rank" and not self.partial:
            raise ValueError(f"snapshot of {self.name} was written by one process per shard (payload text split over tables0..{int(meta.get('shards', 1)) - 1}/): "
                             "load it with shard_backend='dist' on as many ranks")
        # a complete table at the root (format <= 3 of a 'dist' store, or a snapshot of in-process shards) serves a per-rank
        # store as well: it merely holds more text than this rank needs
        self.payloads.load(per_rank if layout == "per_rank" else directory)
        self.row_shard = np.fromfile(os.path.join(directory, "rows.shard.i32"), np.int32)
        self.row_local = np.fromfile(os.path.join(directory, "rows.local.i64"), np.int64)
        if widen:
            values = self.payloads.numeric_codes(self.numeric_keys, 0, self.payloads.n)          # [slots, numeric columns]
            slot_of = {}
            for s in self.shards.owned if self.shards.ns > 1 else ():
                m = np.flatnonzero(self.row_shard == s)
                slot_of[s] = np.empty((m.size,), np.int64)
                slot_of[s][self.row_local[m]] = m

            def columns(s: int, first: int, rows: int) -> np.ndarray:
                """int32 [numeric columns, rows]: the values of shard ``s``'s local rows first .. first + rows."""
                slots = np.arange(first, first + rows) if self.shards.ns == 1 else slot_of[s][first:first + rows]
                return np.ascontiguousarray(values[slots].T)
            self.shards.load(directory, widen=columns)
        if self.payloads.n != n or sum(self.shards.rows) != n or list(self.shards.rows) != [int(v) for v in meta["shard_rows"]]:
            raise ValueError(f"snapshot of {self.name}: {self.shards.rows} rows in the shards, {n} ids, {self.payloads.n} payloads")
        self.slot_of = [np.zeros((0,), np.int64) for _ in range(self.shards.ns)]
        if self.shards.ns > 1:
            for s in range(self.shards.ns):
                m = np.flatnonzero(self.row_shard == s)
                so = np.empty((m.size,), np.int64)
                so[self.row_local[m]] = m
                self.slot_of[s] = so
        self._side = {}
        self._lex_drop()
        self._text_drop()
        self._degrees = meta.get("degrees")
        self._graph_names, self._graph_code, self._graph_rel, self._graph_self = [], {}, {}, {}
        graph_meta = meta.get("graph")
        if graph_meta:
            with open(os.path.join(directory, graph_meta["names"])) as f:
                self._graph_names = [str(v) for v in json.load(f)]
            self._graph_code = {v: i for i, v in enumerate(self._graph_names)}
            if len(self._graph_names) != int(graph_meta["nodes"]) or len(self._graph_code) != len(self._graph_names):
                raise ValueError(f"snapshot of {self.name}: {len(self._graph_names)} graph node names ({len(self._graph_code)} distinct), collection.json says {graph_meta['nodes']}")
            for r in graph_meta["relations"]:
                pairs = np.fromfile(os.path.join(directory, r["file"]), np.int32).reshape(-1, 2)
                if len(pairs) != int(r["edges"]):
                    raise ValueError(f"snapshot of {self.name}: relation {r['name']!r} holds {len(pairs)} edges, collection.json says {r['edges']}")
                self._graph_rel[str(r["name"])] = graph_mod.unique_edges(pairs, len(self._graph_names))
                loops = np.fromfile(os.path.join(directory, r["self"]), np.int32) if r.get("self") else np.zeros((0,), np.int32)
                self._graph_self[str(r["name"])] = graph_mod.self_loops(np.stack([loops, loops], axis=1), len(self._graph_names))
        self._graph_changed()

    def close(self) -> None:
        self._lex_drop()
        self._text_drop()
        self._graph_drop()
        self.shards.close()


class RerankHits:
    """Ids and payloads of the slots a ``search_rerank_batch`` output refers to, read while the slots still meant them."""

    def __init__(self, by_slot: dict[int, tuple[Any, dict[str, Any]]], degrees: dict[str, int] | None):
        self._by_slot = by_slot
        self._degrees = degrees

    def hit(self, slot: int, score: float) -> dict[str, Any]:
        pid, payload = self._by_slot[int(slot)]
        return {"id": pid, "score": score, "payload": payload}


def ffi_index_tensor(vecs, keep):
    import torch
    return torch.as_tensor(keep, device=vecs.device, dtype=torch.int64)


_COLLECTIONS = (list, tuple, set, frozenset)


class SpanCut(NamedTuple):
    """What travels in the ``group`` slot of a search pass for ``max_overlap``: the overlap a hit may share with a better one,
    in thousandths (the coalescer keys passes by it, as it does by ``(group_by, group_size)``)."""
    permille: int


def _value_key(v) -> str:
    """A filter value as part of a coalescing key: collections compare as sets of their members, range mappings as the
    inclusive bounds they stand for (``{"gt": 3}`` and ``{"gte": 4}`` select the same points) -- and as nothing else does."""
    if _is_text(v):
        try:
            return "text" + repr(tuple(text_spec("", v)))
        except (ValueError, TypeError):        # (a malformed text filter: its own key; the call fails where the filter is built)
            return "text?" + repr(sorted((str(k), repr(x)) for k, x in v.items()))
    if _is_range(v):
        try:
            return "range" + repr(range_bounds("", v))
        except ValueError:                     # (a malformed range: its own key; the call fails where the filter is built)
            return "range?" + repr(sorted((str(k), repr(x)) for k, x in v.items()))
    return repr(sorted(repr(x) for x in v)) if isinstance(v, _COLLECTIONS) else "=" + repr(v)


def _filter_key(filters, must_not) -> tuple:
    """A (filters, must_not) pair as a key: equal keys select the same points (what the coalescer groups calls by, and what
    makes two queries of a per-query batch members of one class)."""
    return (tuple(sorted((k, _value_key(v)) for k, v in (filters or {}).items())),
            tuple(sorted((k, _value_key(v)) for k, v in (must_not or {}).items())))


def _per_query(filters, must_not, nq: int):
    """``filters`` / ``must_not`` of a batch call as per-query lists -- or None when both are the single dict (or None) that
    holds for the whole batch.  A sequence must have one entry (a dict or None) per query."""
    seqs = [isinstance(v, (list, tuple)) for v in (filters, must_not)]
    if not any(seqs):
        return None
    out = []
    for v, is_seq, what in ((filters, seqs[0], "filters"), (must_not, seqs[1], "must_not")):
        if is_seq:
            if len(v) != nq:
                raise ValueError(f"per-query {what} has {len(v)} entries for {nq} queries")
            if not all(e is None or isinstance(e, dict) for e in v):
                raise ValueError(f"per-query {what} entries must be dicts or None")
            out.append(list(v))
        else:
            out.append([v] * nq)
    return out[0], out[1]


class _RawClient:
    """The slice of ``AsyncQdrantClient`` that callers reach through ``QdrantManager.client``
    (health check: client.py:66; admin cleanup: projects/cleanup.py:41-61)."""

    def __init__(self, store: "HipVectorStore"):
        self._store = store

    async def get_collections(self):
        names = list(self._store._collections)
        return type("CollectionsResponse", (), {"collections": [type("CollectionDescription", (), {"name": n})() for n in names]})()

    async def get_collection(self, collection_name: str) -> CollectionInfo:
        return await self._store.get_collection_info(collection_name)

    @staticmethod
    def _conditions(flt) -> list[tuple[str, str, Any, bool]]:
        """Duck-typed qdrant ``Filter(must=[...], must_not=[...])`` of ``FieldCondition(key, match=MatchValue | MatchText |
        MatchAny | MatchExcept)`` or ``FieldCondition(key, range=Range(gte, gt, lte, lt))`` -> (key, kind, value, negate); kind:
        "value", "text", "any" (value: the list), "range" (value: the inclusive ``(lo, hi)`` of :func:`range_bounds`)."""
        out = []
        for negate, conds in ((False, getattr(flt, "must", None)), (True, getattr(flt, "must_not", None))):
            if conds is not None and not isinstance(conds, (list, tuple)):
                conds = [conds]                      # (qdrant accepts a single condition in place of a list)
            for cond in (conds or []):
                m = getattr(cond, "match", None)
                if m is None and getattr(cond, "range", None) is not None:
                    out.append((cond.key, "range", range_bounds(cond.key, cond.range), negate))
                elif getattr(m, "text", None) is not None:
                    out.append((cond.key, "text", m.text, negate))
                elif getattr(m, "any", None) is not None:
                    out.append((cond.key, "any", list(m.any), negate))
                elif getattr(m, "except_", None) is not None:   # MatchExcept(**{"except": [...]}): anything but these
                    out.append((cond.key, "any", list(m.except_), not negate))
                else:
                    out.append((cond.key, "value", getattr(m, "value", None), negate))
        return out

    def _device_filter(self, col: _Collection, conds) -> list[tuple] | None:
        """The conditions as ONE device filter (``(column, codes, negate)`` per condition), or None when some condition is on a
        key the device does not code (then the payloads are walked on the host).  MatchValue on a coded key is one code,
        MatchAny its values' codes, MatchText every code whose VALUE contains the text -- the dictionaries are small (distinct
        files, not rows), and however many codes that is, the device takes them as one set."""
        out: list[tuple] = []
        for key, kind, value, negate in conds:
            if key in col.numeric_keys:
                if kind == "range":
                    out.append((col._numeric_column(key), value[0], value[1], "not_between" if negate else "between"))
                elif kind == "value" and isinstance(value, (int, np.integer)) and not isinstance(value, bool):
                    out.append(col._range_condition(key, value, negate))
                else:
                    return None                      # (MatchValue(None), MatchAny, MatchText on a line number: the host walk, as before)
                continue
            if kind == "range":
                raise ValueError(f"payload key {key!r} is not numeric: a Range needs one of {', '.join(col.numeric_keys) or '(none)'}")
            if key not in col.keys:
                return None
            book = col.payloads.cols[key]
            if kind == "text":
                codes = [i + 1 for i, v in enumerate(book.values) if isinstance(v, str) and str(value) in v]
            else:
                codes = col._codes_of(key, value if kind == "any" else [value])
            out.append((col.keys.index(key), codes, negate))
        if len(out) > ffi.MAX_FILTERS:
            return None
        return out

    def _host_select(self, col: _Collection, conds) -> np.ndarray:
        """Slots whose payload meets conditions on keys the device does not code: a walk over the alive slots' columns."""
        slots = []
        mine = set(col.shards.owned)
        for t in col.matching_slots(None):
            if col.partial and int(col.row_shard[t]) not in mine:
                continue                                  # (one process per shard: a row's text is with its owner, who answers for it)
            ok = True
            for key, kind, value, negate in conds:
                have = col.payloads.value(int(t), key)
                hit = ((isinstance(have, str) and str(value) in have) if kind == "text" else
                       (have in value) if kind == "any" else
                       (type(have) is int and max(value[0], 0) <= have <= min(value[1], ffi.VALUE_MAX)) if kind == "range" else have == value)
                ok = ok and (hit != negate)
            if ok:
                slots.append(int(t))
        if col.partial:
            parts = col.shards._arrays_everyone({col.shards.rank: np.asarray(slots, np.int64)})
            slots = sorted(int(t) for part in parts.values() for t in part)
        return np.asarray(slots, dtype=np.int64)

    async def count(self, collection_name: str, count_filter=None, exact: bool = True):
        def work():
            col = self._store._col(collection_name)
            conds = self._conditions(count_filter)
            dfilt = self._device_filter(col, conds)
            if dfilt is None:
                return int(self._host_select(col, conds).size)
            return col.shards.count_matching(dfilt)
        n = await self._store._run(work)
        return type("CountResult", (), {"count": n})()

    async def facet(self, collection_name: str, key: str, facet_filter=None, limit: int = 10, exact: bool = True):
        """Qdrant's ``client.facet``: an object with ``.hits[i].value`` / ``.hits[i].count`` (``FacetResponse``), the ``limit``
        most frequent values of ``key`` among the points ``facet_filter`` keeps -- always exact, whatever ``exact`` says; ties
        go to the value stored first (Qdrant: to the value itself).  The filter's keys must be coded on the device."""
        def work():
            col = self._store._col(collection_name)
            col.facet_column(key)
            if not 1 <= int(limit) <= ffi.MAX_K:
                raise ValueError(f"facet: limit {limit} outside 1..{ffi.MAX_K}")
            dfilt = self._device_filter(col, self._conditions(facet_filter))
            if dfilt is None:
                raise ValueError(f"facet_filter holds a condition the device cannot evaluate (filterable: {', '.join(col.keys + col.numeric_keys)})")
            return col.facet(key, int(limit), dfilt)[0]
        res = await self._store._run(work)
        hits = [type("FacetValueHit", (), {"value": h["value"], "count": h["count"]})() for h in res["hits"]]
        return type("FacetResponse", (), {"hits": hits})()

    async def delete(self, collection_name: str, points_selector=None):
        flt = getattr(points_selector, "filter", points_selector)

        def work():
            col = self._store._col(collection_name)
            conds = self._conditions(flt)
            dfilt = self._device_filter(col, conds)
            if dfilt is None:
                col.remove_slots(self._host_select(col, conds))
            elif dfilt:
                col.shards.tombstone_filter(dfilt)      # ONE device call per shard, however many codes a MatchText resolves to
            else:                                       # no condition at all: every point
                col.remove_slots(col.matching_slots(None))
            col.maybe_compact()
        await self._store._run(work)


class HipVectorStore:
    """``QdrantManager`` replacement.  Constructor keeps the reference's positional arguments
    (client.py:19-30: host, port, grpc_port) and ignores them; GPU options are keyword-only."""

    def __init__(self, host: str | None = None, port: int | None = None, grpc_port: int | None = None, *,
                 device: int | None = None, dim: int | None = None, dtype: str | None = None,
                 initial_capacity: int | None = None, search_window_ms: float | None = None, shards: int | None = None,
                 shard_backend: str | None = None, process_group=None, compact_dead_fraction: float | None = None,
                 compact_min_dead: int | None = None, stream: str | None = None, coalesce_filters: bool | None = None, _merge_fn=None):
        s = get_settings()
        self._host, self._port, self._grpc_port = host, port, grpc_port
        self._device = s.hip_device if device is None else device
        # quirk Q3: the reference sizes collections from EMBEDDING_DIMENSIONS (default 1536) although UniXcoder
        # emits 768; here an explicit dim wins, a UniXcoder provider implies 768, else the env value is used.
        if dim is None:
            dim = 768 if s.embedding_provider.startswith("unixcoder") else s.embedding_dimensions
        self._dimensions = dim
        name = (dtype or s.hip_store_dtype).lower()
        if name not in _DTYPES:
            raise VectorStoreError(f"Unknown store dtype {name!r} (use 'f32' or 'bf16')")
        self._dtype = _DTYPES[name]
        self._capacity = initial_capacity or s.hip_initial_capacity
        # Row shards (BASELINE configs[3]: the corpus row-sharded over the GPUs): `shards` handles per collection.  Backend
        # "local": all of them in this process (what a one-GPU box can run); "dist": one process per GPU under
        # torch.distributed -- every rank constructs the same store and makes the same calls, the vectors of a collection are
        # spread over the ranks and every search ends with ONE all-gather + merge (shards.ShardSet).  Default: "dist" when a
        # process group with as many ranks as shards is up, "local" otherwise.
        self._shards = int(shards if shards is not None else s.hip_shards)
        if shard_backend is None:
            shard_backend = s.hip_shard_backend
        if shard_backend == "auto":
            shard_backend = "local"
            if self._shards > 1:
                try:
                    import torch.distributed as dist
                    if dist.is_available() and dist.is_initialized() and dist.get_world_size(process_group) == self._shards:
                        shard_backend = "dist"
                except ImportError:
                    pass
        self._shard_backend, self._group, self._merge_fn = shard_backend, process_group, _merge_fn
        self._compact = (s.hip_compact_dead_fraction if compact_dead_fraction is None else compact_dead_fraction,
                         s.hip_compact_min_dead if compact_min_dead is None else compact_min_dead)
        # The stream the store's device work runs on.  "priority" (default): its own HIGH-PRIORITY stream -- the reference's query
        # path runs beside its indexing path in one process (providers/unixcoder_provider.py:260: the encoder on a worker thread),
        # and on the default stream a search queues behind every launch of a forward that is under way (13 ms for a 65 k-token
        # batch; on an equal-priority side stream the device was still seen to leave it there); with priority its kernels get
        # the CUs at the forward's next kernel boundary (~1 ms).  "default": torch's default stream, as in rounds 1-3.  Every
        # job of the store completes on the host before the next starts, so mutations (host-synchronous in the library) and
        # searches stay ordered whichever stream each used.
        self._stream_mode = (stream or s.hip_store_stream).lower()
        self._stream = None                        # torch.cuda.Stream, created by connect()
        self._collections: dict[str, _Collection] = {}
        self._client: _RawClient | None = None
        self._executor: ThreadPoolExecutor | None = None
        self._lock = threading.Lock()
        # Concurrent search() calls (many users, one query each -- how the reference's query path arrives) are coalesced: the
        # calls that queue up while a pass over the corpus is running, for the same collection and filter, share the NEXT pass
        # (up to 64 queries cost what one costs); an idle store serves a lone call at once.  search_window_ms > 0 additionally
        # waits that long before each pass; < 0 (or CODERAG_HIP_SEARCH_WINDOW_MS=-1) turns coalescing off.
        if search_window_ms is None:
            search_window_ms = float(os.environ.get("CODERAG_HIP_SEARCH_WINDOW_MS", "0"))
        # (one process per shard: every search ends in collectives, so all ranks must cut their calls into the SAME passes; how
        # many concurrent calls a pass picks up depends on each rank's own timing -- there, every call is its own pass)
        self._search_coalesce = search_window_ms >= 0 and self._shard_backend != "dist"
        self._search_window_s = max(0.0, search_window_ms) / 1e3
        self._search_pending: dict[tuple, list] = {}
        self._search_drainers: dict[tuple, asyncio.Task] = {}
        self.search_passes = 0                      # corpus passes issued by search() (observability / tests)
        # coalesce_filters (CODERAG_HIP_COALESCE_FILTERS=1; default off): plain concurrent calls for one collection share passes
        # WHATEVER their filters -- a pass serves up to 8 distinct filters (crh_search_multi), every caller keeps its own filter
        # and its own limit prefix.  Off: a pass is shared by the calls of one filter only, as before.
        if coalesce_filters is None:
            coalesce_filters = os.environ.get("CODERAG_HIP_COALESCE_FILTERS", "0").lower() in ("1", "true", "yes", "on")
        self._coalesce_filters = bool(coalesce_filters)

    # ------------------------------------------------------------------ plumbing
    async def _run(self, fn, *args):
        """All native work goes through one worker thread: one handle, one thread at a time."""
        if self._executor is None:
            raise VectorStoreError("Client not connected. Call connect() first.")
        loop = asyncio.get_running_loop()

        def guarded():
            with self._lock:
                ffi.use_device(self._device)      # the worker thread starts on device 0 whatever CODERAG_HIP_DEVICE says
                if self._stream is None:
                    return fn(*args)
                import torch
                with torch.cuda.stream(self._stream):      # torch-side work and ffi.current_stream() of the job resolve to the store's stream
                    try:
                        return fn(*args)
                    finally:
                        self._stream.synchronize()           # (a job is complete when it returns: the next one may use another stream)
        return await loop.run_in_executor(self._executor, guarded)

    def _col(self, collection: str) -> _Collection:
        name = collection.value if isinstance(collection, CollectionName) else collection
        if name not in self._collections:
            raise KeyError(f"collection {name!r} does not exist (call create_collections())")
        return self._collections[name]

    # ------------------------------------------------------------------ lifecycle (client.py:32-70)
    async def connect(self) -> None:
        if self._client is not None:
            return
        try:
            ffi.lib()
            if ffi.device_count() <= self._device:
                raise ffi.NativeError(ffi.E_NODEVICE, f"HIP device {self._device} is not visible")
            info = ffi.device_info(self._device)
            self._executor = ThreadPoolExecutor(max_workers=1, thread_name_prefix="hip-store")
            self._client = _RawClient(self)
            if self._stream_mode == "priority":
                try:
                    import torch
                    if torch.cuda.is_available():
                        self._stream = torch.cuda.Stream(device=self._device, priority=-1)
                except ImportError:
                    self._stream = None
            logger.info("Connected to HIP vector store on device %d (%s, %s)", self._device, info["name"], info["arch"])
        except Exception as e:
            self._client = None
            raise VectorStoreError("Failed to connect to Qdrant", cause=e)

    async def close(self) -> None:
        if self._client is None:
            return
        try:
            await self._run(lambda: [c.close() for c in self._collections.values()])
            logger.info("Closed HIP vector store")
        except Exception as e:  # same leniency as client.py:52-55
            logger.warning(f"Error closing HIP vector store: {e}")
        finally:
            self._collections = {}
            self._client = None
            self._stream = None
            if self._executor:
                self._executor.shutdown(wait=True)
                self._executor = None

    @property
    def client(self) -> _RawClient:
        if self._client is None:
            raise VectorStoreError("Client not connected. Call connect() first.")
        return self._client

    async def health_check(self) -> bool:
        try:
            await self.client.get_collections()
            await self._run(ffi.device_info, self._device)
            return True
        except Exception as e:
            logger.warning(f"HIP vector store health check failed: {e}")
            return False

    # ------------------------------------------------------------------ collections (client.py:72-113)
    async def create_collections(self) -> None:
        try:
            _ = self.client

            def work():
                for name in (CollectionName.CODE_CHUNKS.value, CollectionName.SUMMARIES.value):
                    if name not in self._collections:
                        self._collections[name] = _Collection(name, self._dimensions, self._dtype, self._capacity, self._device,
                                                              nshards=self._shards, backend=self._shard_backend, group=self._group,
                                                              merge_fn=self._merge_fn, compact_dead_fraction=self._compact[0],
                                                              compact_min_dead=self._compact[1])
                        self._collections[name].shards.stream = int(self._stream.cuda_stream) if self._stream is not None else 0
                        logger.info(f"Created collection: {name}")
            await self._run(work)
        except Exception as e:
            raise VectorStoreError("Failed to create collections", cause=e)

    async def clear_collections(self) -> None:
        def drop():
            for name in (CollectionName.CODE_CHUNKS.value, CollectionName.SUMMARIES.value):
                col = self._collections.pop(name, None)
                if col is not None:
                    col.close()
        _ = self.client
        await self._run(drop)
        await self.create_collections()

    async def get_collection_info(self, collection: str) -> CollectionInfo:
        try:
            def work():
                col = self._col(collection)
                rows, alive = col.shards.count()
                return CollectionInfo(name=col.name, points_count=alive, vectors_count=alive, indexed_vectors_count=alive,
                                      config={"size": col.shards.dim, "distance": "Cosine", "rows_appended": rows,
                                              "capacity_rows": col.shards.capacity_rows, "shards": col.shards.ns,
                                              "shard_rows": list(col.shards.rows), "shard_backend": col.shards.backend,
                                              "compactions": col.compactions,
                                              "dtype": "bf16" if col.shards.dtype == ffi.DTYPE_BF16 else "f32"})
            return await self._run(work)
        except Exception as e:
            raise VectorStoreError(f"Failed to get collection info for {collection}", cause=e)

    # ------------------------------------------------------------------ data path
    async def upsert(self, collection: str, ids: list[str], vectors, payloads: list[dict[str, Any]], *, texts=None, embed=None) -> None:
        """client.py:115-130.  Same id again replaces the point (Qdrant upsert semantics).  ``vectors``: the reference's
        list of float lists, or -- without the list round trip -- a float32 ndarray / a CUDA tensor [n, dim].
        ``vectors=None`` with ``texts`` and ``embed`` (a callable ``list[str] -> [m, dim]``, e.g. ``provider.embed_texts_sync``):
        the store routes the rows first and THIS process embeds only the texts of the shards it owns -- with one process per GPU
        (``shards=N``, backend "dist") rank g embeds and stores exactly its share, no vector ever crosses ranks."""
        try:
            await self._run(lambda: self._col(collection).upsert(ids, vectors, payloads, texts=texts, embed=embed))
            logger.debug(f"Upserted {len(ids)} vectors to {collection}")
        except Exception as e:
            raise VectorStoreError(f"Failed to upsert vectors to {collection}", cause=e)

    def _search_sync(self, collection: str, queries: np.ndarray, limit: int, filters: dict[str, Any] | None, must_not: dict[str, Any] | None = None,
                     diversity: float | None = None, candidates: int | None = None, group: tuple | None = None):
        col = self._col(collection)
        nq = queries.shape[0]
        per = _per_query(filters, must_not, nq)
        if per is not None:
            if has_graph_condition(filters, must_not):
                raise ValueError(f"a per-query filter list cannot carry a {GRAPH_KEY!r} condition: it is one BFS and one row bitmap for the whole batch -- pass ONE filter dict")
            if has_text_condition(filters, must_not):
                raise ValueError("a per-query filter list cannot carry a text condition ({'contains': ...} / {'matches': ...} / {'fuzzy': ...}): a text condition is "
                                 "one grep for the whole batch -- pass ONE filter dict")
            if diversity is not None or group is not None:
                raise ValueError("per-query filters cannot be combined with diversity, group_by or max_overlap (a follow-up: the "
                                 "candidate lists behind them are per filter)")
            classes: dict[tuple, int] = {}
            pairs, qclass = [], []
            for f, m in zip(*per):                                       # distinct filters -> classes, by the coalescer's normalisation
                key = _filter_key(f, m)
                if key not in classes:
                    classes[key] = len(pairs)
                    pairs.append((f, m))
                qclass.append(classes[key])
            if len(pairs) > 1:
                return (col,) + self._search_classes(col, queries, limit, pairs, np.asarray(qclass, np.int32))
            filters, must_not = pairs[0] if pairs else (None, None)      # ONE distinct filter: the batch runs the code it runs today
        dfilt = col.device_filters(filters, must_not)
        if dfilt is None or limit <= 0 or ((diversity is not None or group is not None) and nq == 0):
            return col, np.full((nq, max(limit, 0)), -np.inf, np.float32), np.full((nq, max(limit, 0)), -1, np.int64)
        if isinstance(group, SpanCut):
            scores, slots = col.search_spans(queries, limit, candidates, group.permille, dfilt)
        elif group is not None:
            scores, slots = col.search_grouped(queries, limit, candidates, group[0], group[1], dfilt)
        elif diversity is None:
            scores, slots = col.search(queries, limit, dfilt)
        else:
            scores, slots = col.search_mmr(queries, limit, candidates, diversity, dfilt)
        return col, scores, slots

    @staticmethod
    def _search_classes(col, queries: np.ndarray, limit: int, pairs, qclass: np.ndarray):
        """The mixed-filter pass: ``pairs`` are the distinct (filters, must_not) of the batch, ``qclass`` every query's index
        into them.  A class naming a value the collection never stored answers its own queries with nothing; the others share
        corpus passes (``ffi.Index.search_multi``)."""
        nq = queries.shape[0]
        scores, slots = np.full((nq, max(limit, 0)), -np.inf, np.float32), np.full((nq, max(limit, 0)), -1, np.int64)
        dfilts = [col.device_filters(f, m) for f, m in pairs]
        live = np.flatnonzero(np.asarray([dfilts[c] is not None for c in qclass.tolist()], bool))
        if limit > 0 and live.size:
            used = sorted(set(qclass[live].tolist()))
            s, r = col.search_multi(np.ascontiguousarray(queries[live]), limit, [dfilts[c] for c in used],
                                    np.asarray([used.index(c) for c in qclass[live].tolist()], np.int32))
            scores[live], slots[live] = s, r
        return scores, slots

    def _search_hits_sync(self, collection: str, queries: np.ndarray, limits, filters: dict[str, Any] | None,
                          must_not: dict[str, Any] | None = None, diversity: float | None = None,
                          candidates: int | None = None, group: tuple | None = None) -> list[list[dict[str, Any]]]:
        """One pass + the hit dictionaries of every query, built HERE -- inside the worker job, under the store's lock.  Slots
        are positions in the host tables and a compaction renumbers them (the store compacts by itself after deletes and
        replacing upserts): a slot handed back to the event loop could name another point, or none, by the time its payload is
        read.  ``limits``: one int for all queries, or one per query (coalesced callers keep their own prefix).  ``diversity``
        (with its resolved ``candidates``): the pass is the diversity-aware one; greedy picks over one candidate list are
        prefix-stable, so the prefixes hold there too.  ``group`` = ``(group_by, group_size)``: the pass is the grouped one
        (``_Collection.search_grouped``); the first j rows of its answer are the j-row answer, so the prefixes hold again."""
        per = [int(limits)] * queries.shape[0] if isinstance(limits, (int, np.integer)) else [int(v) for v in limits]
        col, scores, slots = self._search_sync(collection, queries, max(per, default=0), filters, must_not, diversity, candidates, group)
        return self._hit_lists(col, slots, scores, per)

    @staticmethod
    def _hit_lists(col: _Collection, slots: np.ndarray, scores: np.ndarray, limit=None, decorate=None) -> list[list[dict[str, Any]]]:
        """The hit dictionaries of every query of a ``[nq, k]`` table of slots (-1: padding) and its scores: ONE flat
        ``col.hits`` call (payloads fetched together), split by the queries' own counts.  ``limit``: how much of its row a
        query keeps -- one int, or one per query; ``decorate(hits, keep)`` adds a feature's own fields to the flat list, ``keep``
        being the bool ``[nq, k]`` mask of the entries that became hits, in order.  Like its callers it runs inside the worker
        job, under the store's lock (:meth:`_search_hits_sync`)."""
        keep = slots >= 0
        if limit is not None:
            keep &= np.arange(slots.shape[1])[None, :] < np.asarray(limit).reshape(-1, 1)
        flat = col.hits(slots[keep].tolist(), scores[keep].tolist())
        if decorate is not None:
            decorate(flat, keep)
        out, at = [], 0
        for n in keep.sum(1).tolist():
            out.append(flat[at:at + n])
            at += n
        return out

    @staticmethod
    def _range_args(score_threshold, nq: int, **others) -> np.ndarray:
        """Checked thresholds of one thresholded call, float32 [nq] (a scalar stands for every query).  ``others``: the arguments
        a score threshold cannot be combined with in this version, by name; any that is set raises.  ``ValueError`` for the
        caller alone, before anything is searched."""
        used = [name for name, v in others.items() if v]
        if used:
            raise ValueError(f"score_threshold cannot be combined with {', '.join(used)} (a follow-up: those select from finished "
                             "top-c lists, the threshold works at the scan)")
        try:
            thr = np.asarray(score_threshold, dtype=np.float32)
        except (TypeError, ValueError):
            raise ValueError(f"score_threshold {score_threshold!r} is not a number or one number per query") from None
        thr = np.full((nq,), thr, np.float32) if thr.ndim == 0 else thr.reshape(-1)
        if thr.shape[0] != nq:
            raise ValueError(f"{thr.shape[0]} score thresholds for {nq} queries")
        if not np.isfinite(thr).all():
            raise ValueError("score_threshold must be a finite number")
        return thr

    def _search_range_sync(self, collection: str, queries: np.ndarray, limit: int, thresholds: np.ndarray, filters, must_not,
                           counts: bool) -> tuple[list[list[dict[str, Any]]], list[int] | None]:
        """One thresholded pass + the hit dictionaries of every query, built inside the worker job as in
        :meth:`_search_hits_sync`: ``(hits per query, in-range count per query or None)``.  ``limit`` 0 asks for the counts
        alone (the device still selects one row per query: its k is at least 1)."""
        col = self._col(collection)
        nq = queries.shape[0]
        dfilt = col.device_filters(filters, must_not)
        if dfilt is None or nq == 0 or (limit <= 0 and not counts):       # (a value the collection never stored: nothing is in range)
            return [[] for _ in range(nq)], ([0] * nq if counts else None)
        scores, slots, totals = col.search_range(queries, max(int(limit), 1), thresholds, dfilt, counts)
        return self._hit_lists(col, slots, scores, limit), ([int(c) for c in totals] if counts else None)

    async def _range_call(self, collection: str, query_vectors, score_threshold, limit: int, filters, must_not, counts: bool, **others):
        """The common path of every thresholded entry point: argument checks for the caller alone, then a pass of its own --
        thresholded calls never join the coalescer (their pass differs from a plain one: the threshold moves the scan's cut)."""
        q = np.asarray(query_vectors, dtype=np.float32)
        dim = self._col(collection).shards.dim
        if q.ndim != 2 or (q.shape[0] and q.shape[1] != dim):
            raise ValueError(f"query dim {q.shape[-1] if q.ndim else 0} != index dim {dim}")
        if isinstance(filters, (list, tuple)) or isinstance(must_not, (list, tuple)):
            others["per-query filters"] = True
        thr = self._range_args(score_threshold, q.shape[0], **others)
        if limit > ffi.MAX_K:
            raise ValueError(f"limit {limit} exceeds the index's maximum k of {ffi.MAX_K}")
        self.search_passes += (q.shape[0] + 63) // 64
        return await self._run(self._search_range_sync, collection, q, int(limit), thr, filters, must_not, counts)

    async def search_range_batch(self, collection: str, query_vectors, score_threshold, limit: int = 10,
                                 filters: dict[str, Any] | None = None, must_not: dict[str, Any] | None = None) -> list[dict[str, Any]]:
        """Batched :meth:`search_range`: ``score_threshold`` is one number or one per query; one ``{"hits", "count"}`` per query."""
        try:
            hits, totals = await self._range_call(collection, query_vectors, score_threshold, limit, filters, must_not, True)
            return [{"hits": h, "count": c} for h, c in zip(hits, totals)]
        except Exception as e:
            raise VectorStoreError(f"Failed to search {collection}", cause=e)

    async def search_range(self, collection: str, query_vector: list[float], score_threshold: float, limit: int = 10,
                           filters: dict[str, Any] | None = None, must_not: dict[str, Any] | None = None) -> dict[str, Any]:
        """The hits whose cosine is at least ``score_threshold`` (Qdrant's ``query_points(score_threshold=...)``) AND how many
        such points there are: ``{"hits": [...], "count": int}``.  A point is in range iff it is alive, passes the filter and
        its score -- the f32 value :meth:`search` reports -- is ``>= score_threshold`` (inclusive).  ``hits`` are the first
        ``min(limit, count)`` of them in :meth:`search`'s order; ``count`` is exact and not clipped at ``limit`` or at the
        index's maximum k: "is the top-``limit`` the whole story or the tip of it".  A very low threshold makes
        every in-range row a candidate on the device; one beyond the candidate workspace's budget fails with the count it met,
        it never returns a clipped number."""
        return (await self.search_range_batch(collection, [query_vector], score_threshold, limit, filters, must_not))[0]

    async def count_similar(self, collection: str, query_vector: list[float], score_threshold: float,
                            filters: dict[str, Any] | None = None, must_not: dict[str, Any] | None = None) -> int:
        """How many points are at least ``score_threshold`` similar to ``query_vector`` (:meth:`search_range`'s ``count``
        without the hits): clone pressure before a refactor, "a one-off or a pattern"."""
        try:
            return (await self._range_call(collection, [query_vector], score_threshold, 0, filters, must_not, True))[1][0]
        except Exception as e:
            raise VectorStoreError(f"Failed to search {collection}", cause=e)

    # ------------------------------------------------------------------ facets
    def _facet_sync(self, collection: str, key: str, limit: int, filters, must_not, queries, thresholds) -> list[dict[str, Any]]:
        """One facet job on the worker: the filter's conditions (text conditions grep here, through the collection's cache), the
        histogram, its list, and the codes mapped back to values -- all under the store's lock, so the dictionaries are the ones
        the codes were counted with."""
        col = self._col(collection)
        nq = 1 if queries is None else queries.shape[0]
        dfilt = col.device_filters(filters, must_not)
        if dfilt is None or nq == 0:                                        # (a value the collection never stored: nothing counts)
            return [{"hits": [], "values": 0, "total": 0, "missing": 0} for _ in range(nq)]
        return col.facet(key, limit, dfilt, queries, thresholds)

    async def _facet_call(self, collection: str, key: str, limit, filters, must_not, query_vectors, score_threshold) -> list[dict[str, Any]]:
        """Argument checks for the caller alone, then one job."""
        col = self._col(collection)
        col.facet_column(key)
        limit = int(limit)
        if not 1 <= limit <= ffi.MAX_K:
            raise ValueError(f"facet: limit {limit} outside 1..{ffi.MAX_K}")
        if isinstance(filters, (list, tuple)) or isinstance(must_not, (list, tuple)):
            raise ValueError("a facet takes one filter, not per-query filters")
        q = thr = None
        if (query_vectors is None) != (score_threshold is None):
            raise ValueError("facet: query_vector and score_threshold come together (the rows at least that similar count) or not at all")
        if query_vectors is not None:
            q = np.asarray(query_vectors, dtype=np.float32)
            if q.ndim != 2 or (q.shape[0] and q.shape[1] != col.shards.dim):
                raise ValueError(f"query dim {q.shape[-1] if q.ndim else 0} != index dim {col.shards.dim}")
            thr = self._range_args(score_threshold, q.shape[0])
            self.search_passes += (q.shape[0] + 63) // 64
        return await self._run(self._facet_sync, collection, key, limit, filters, must_not, q, thr)

    async def facet(self, collection: str, key: str, limit: int = 10, filters: dict[str, Any] | None = None,
                    must_not: dict[str, Any] | None = None, *, query_vector: list[float] | None = None,
                    score_threshold: float | None = None) -> dict[str, Any]:
        """Qdrant's ``client.facet(collection_name, key, facet_filter, limit, exact=True)``: the values of payload key ``key``
        among the points that COUNT, with how many points carry each -- "how many chunks per file hold ``TODO(``", "which
        languages make up this project".  A point counts iff it is alive and passes ``filters`` / ``must_not`` (everything
        :meth:`search` takes, ``{"content": {"contains": ...}}`` / ``{"matches": ...}`` / ``{"fuzzy": ...}`` included); with ``query_vector`` and
        ``score_threshold`` -- both or neither -- its score must also be ``>= score_threshold``, exactly :meth:`count_similar`'s
        rule: "in which files does this concept live".  Returns ``{"hits": [{"value", "count"}, ...], "values", "total",
        "missing"}``: ``hits`` are the ``limit`` (1..1024) most frequent values, count descending, ties to the value STORED
        FIRST (Qdrant breaks ties by the value itself); ``values`` how many distinct values were counted and ``total`` how many
        points carry one, neither clipped at ``limit``; ``total + missing`` is what :meth:`count` / :meth:`count_similar` return
        for the same arguments.  ``key`` is one of the collection's dictionary-coded keys.  A point without the key is counted
        under the value None, as a filter ``{key: None}`` selects it.  Counted, selected and sorted on the device, exact
        (DESIGN.md 3.23)."""
        try:
            return (await self._facet_call(collection, key, limit, filters, must_not, None if query_vector is None else [query_vector],
                                           score_threshold))[0]
        except VectorStoreError:
            raise
        except Exception as e:
            raise VectorStoreError(f"Failed to facet {collection}", cause=e)

    async def facet_batch(self, collection: str, key: str, query_vectors, score_threshold, limit: int = 10,
                          filters: dict[str, Any] | None = None, must_not: dict[str, Any] | None = None) -> list[dict[str, Any]]:
        """:meth:`facet` for several queries in one pass per 64: ``score_threshold`` is one number or one per query; one result
        per query."""
        try:
            if query_vectors is None or score_threshold is None:
                raise ValueError("facet_batch needs query vectors and a score threshold")
            return await self._facet_call(collection, key, limit, filters, must_not, query_vectors, score_threshold)
        except VectorStoreError:
            raise
        except Exception as e:
            raise VectorStoreError(f"Failed to facet {collection}", cause=e)

    @staticmethod
    def _mmr_args(limit: int, diversity: float | None, candidates: int | None) -> tuple[float | None, int | None]:
        """Checked ``(diversity, candidates)`` of one call -- ``(None, None)`` for a plain search.  ``candidates`` defaults to
        ``min(MAX_K, 4 * limit)``.  Raises ``ValueError`` for the caller alone, before the call joins any pass."""
        if diversity is None:
            if candidates is not None:
                raise ValueError("candidates is only meaningful together with diversity")
            return None, None
        diversity = float(diversity)
        if not 0.0 <= diversity <= 1.0:                                    # (NaN fails both comparisons)
            raise ValueError(f"diversity {diversity} outside [0, 1]")
        if candidates is None:
            candidates = min(ffi.MAX_K, 4 * max(int(limit), 1))
        candidates = int(candidates)
        if candidates < limit or candidates < 1 or candidates > ffi.MAX_K:
            raise ValueError(f"candidates {candidates} must be >= limit ({limit}) and <= {ffi.MAX_K}")
        return diversity, candidates

    def _group_args(self, collection: str, limit: int, group_by: str | None, group_size: int, diversity: float | None,
                    candidates: int | None, has_vector: bool = True) -> tuple[tuple | None, int | None]:
        """Checked ``((group_by, group_size), candidates)`` of one grouped call -- ``(None, candidates)`` untouched for a call
        without ``group_by``.  ``candidates`` defaults to ``min(MAX_K, 4 * limit)``, bounds as for the diversity-aware search.
        Raises ``ValueError`` for the caller alone, before the call joins any pass."""
        if int(group_size) < 1:
            raise ValueError(f"group_size {group_size} must be >= 1")
        if group_by is None:
            return None, candidates
        if diversity is not None:
            raise ValueError("group_by and diversity cannot be combined")
        if not has_vector:
            raise ValueError("group_by needs a query vector (the filter-only fetch has no order to cap)")
        self._col(collection)._column(group_by)                             # (ValueError: not a filterable key of the collection)
        if candidates is None:
            candidates = min(ffi.MAX_K, 4 * max(int(limit), 1))
        candidates = int(candidates)
        if candidates < limit or candidates < 1 or candidates > ffi.MAX_K:
            raise ValueError(f"candidates {candidates} must be >= limit ({limit}) and <= {ffi.MAX_K}")
        return (group_by, int(group_size)), candidates

    def _span_args(self, collection: str, limit: int, max_overlap, candidates: int | None, diversity: float | None, group: tuple | None,
                   has_vector: bool = True, per_query: bool = False) -> tuple[SpanCut, int]:
        """Checked ``(SpanCut(permille), candidates)`` of one ``max_overlap`` call: a float in [0, 1] becomes
        ``round(max_overlap * 1000)``; ``candidates`` defaults to ``min(MAX_K, 4 * limit)``, bounds as for the grouped search.
        Raises ``ValueError`` for the caller alone, before the call joins any pass."""
        try:
            share = float(max_overlap)
        except (TypeError, ValueError):
            raise ValueError(f"max_overlap {max_overlap!r} is not a number") from None
        if isinstance(max_overlap, bool) or not 0.0 <= share <= 1.0:          # (NaN fails both comparisons)
            raise ValueError(f"max_overlap {max_overlap!r} outside [0, 1]")
        used = [name for name, v in (("diversity", diversity is not None), ("group_by", group is not None), ("per-query filters", per_query)) if v]
        if used:
            raise ValueError(f"max_overlap cannot be combined with {', '.join(used)}")
        if not has_vector:
            raise ValueError("max_overlap needs a query vector (the filter-only fetch has no order to walk)")
        if not self._col(collection).numeric_keys:
            raise ValueError(f"collection {collection!r} keeps no line numbers on the device: max_overlap needs them")
        if candidates is None:
            candidates = min(ffi.MAX_K, 4 * max(int(limit), 1))
        candidates = int(candidates)
        if candidates < limit or candidates < 1 or candidates > ffi.MAX_K:
            raise ValueError(f"candidates {candidates} must be >= limit ({limit}) and <= {ffi.MAX_K}")
        return SpanCut(int(round(share * 1000))), candidates

    async def chunks_at(self, collection: str, file_path: str, line: int, last_line: int | None = None, limit: int = 64) -> list[dict[str, Any]]:
        """The payloads of the alive points of ``file_path`` whose span meets the lines ``line .. last_line`` (``last_line``
        None: the one line) -- ``start_line <= last`` and ``end_line >= first`` -- in insertion order, at most ``limit``: "which
        chunk covers line 120 of this file", the chunks under a stack frame or an editor selection.  One filter-only device call
        (two range conditions and the file's code); no vector is involved.  Points without line numbers never match."""
        try:
            first = int(line)
            last = first if last_line is None else int(last_line)
            if isinstance(line, bool) or isinstance(last_line, bool) or first < 0 or last < first:
                raise ValueError(f"chunks_at needs 0 <= line <= last_line, got {line!r} .. {last_line!r}")

            def fetch():
                col = self._col(collection)
                if not col.numeric_keys:
                    raise ValueError(f"collection {collection!r} keeps no line numbers on the device")
                slots = col.matching_slots({"file_path": file_path, "start_line": {"lte": last}, "end_line": {"gte": first}}, limit=int(limit))
                return col.payloads_of(slots)
            return await self._run(fetch)
        except Exception as e:
            raise VectorStoreError(f"Failed to fetch the chunks at {file_path}:{line}", cause=e)

    async def search(self, collection: str, query_vector: list[float] | None, limit: int = 10,
                     filters: dict[str, Any] | None = None, must_not: dict[str, Any] | None = None, *,
                     diversity: float | None = None, candidates: int | None = None,
                     group_by: str | None = None, group_size: int = 1, score_threshold: float | None = None,
                     max_overlap: float | None = None) -> list[dict[str, Any]]:
        """client.py:132-157: descending cosine, ``[{"id", "score", "payload"}]``.  ``query_vector=None`` is the
        filter-only fetch the context builder issues (quirk Q7): first ``limit`` matching points, score 0.0.
        A ``filters`` value may be a list / tuple / set (any of them: Qdrant's ``MatchAny``); ``must_not`` (not in the
        reference's signature) names values a hit must NOT have, one or a collection per key (``Filter(must_not=...)``).
        Values the collection has never stored contribute nothing and never raise.
        ``diversity`` in [0, 1] (not in the reference either; Qdrant's ``Mmr(diversity, candidates_limit)``) asks for the
        diversity-aware top-k: the ``limit`` greedy maximal-marginal-relevance picks among the ``candidates`` best hits
        (default ``min(MAX_K, 4 * limit)``; ``limit <= candidates <= MAX_K``), selected on the device.  A hit's
        ``score`` stays its cosine to the query, so the list is no longer sorted by it.  ``diversity=None`` is the plain search.
        ``group_by`` (one of the collection's filterable keys; Qdrant's ``query_points_groups``, the reference's
        ``max_per_file`` done before the cut instead of after it) caps the hits per value of that key at ``group_size``: the
        answer is EXACTLY the first ``limit`` rows of the plain order whose rank among the rows of their own value is below
        ``group_size``, still sorted by score, scores and ids unchanged.  Rows without the key (or with None)
        are never capped.  ``candidates`` (default ``min(MAX_K, 4 * limit)``) is how many hits the first round looks at; the
        store goes on by itself when that does not settle the answer.  Not combinable with ``diversity``.
        ``score_threshold`` (Qdrant's parameter of that name; the reference never sends it): only hits whose score is ``>=`` it
        are returned -- possibly fewer than ``limit``, possibly none.  Exactly the plain list cut after its last such hit
        (:meth:`search_range` also says how many there are).  Not combinable with ``diversity`` or ``group_by``;
        a thresholded call takes a pass of its own.
        A ``filters`` / ``must_not`` value on ``start_line`` / ``end_line`` may be an int or a mapping with any of ``gte``, ``gt``,
        ``lte``, ``lt`` (Qdrant's ``Range``): a numeric range, evaluated on the device; under ``must_not`` points without the
        value pass.
        ``max_overlap`` in [0, 1] (no counterpart in the reference or in Qdrant): the exact top-``limit`` in which no hit repeats
        more than that share of a better hit's lines -- a method next to its class, a ``_part2`` next to ``_part1`` (DESIGN.md
        3.19).  A hit is dropped iff a better KEPT hit of the same file shares more than ``max_overlap`` of the SHORTER of the
        two spans with it; hits without a file or line numbers are never dropped; scores, ids and order are unchanged.
        ``candidates`` as for ``group_by``; a list that 1024 candidates cannot complete comes back short, never wrong.  Not
        combinable with ``diversity``, ``group_by``, ``score_threshold`` or per-query filters.  ``None`` is the plain search.
        A ``filters`` / ``must_not`` value on a TEXT key (``TEXT_KEYS``: ``content`` of the code chunks, ``summary`` of the
        summaries) is a mapping ``{"contains": str | [str, ...], "any": False, "case": True}``: the points whose text holds the
        literal string(s) -- all of them, or with ``any`` at least one; ``case=False`` folds ASCII letters only; under
        ``must_not`` the points that do not (a point without the text passes).  Exact substring match on the device (Qdrant's
        ``MatchText`` on a field without a full-text index), combinable with everything a filter combines with
        except per-query filter lists.  1..8 patterns of 1..64 bytes of UTF-8 each.  ``{"matches": regular expression}`` -- alone
        or beside ``contains``, then both must hold -- keeps the points in whose text Python's ``re`` on bytes (``re.MULTILINE``;
        ``case=False``: ``re.IGNORECASE``) finds the expression, matched on the device by a DFA.
        ``{"fuzzy": string, "edits": 0..3}`` -- alone or beside the other two, then all must hold -- keeps the points whose text
        holds the string within that many insertions, deletions or substitutions of one BYTE (``edits`` left out: 1 up to 5
        bytes, 2 above), matched on the device by a bit-parallel edit-distance walk.
        ``filters`` / ``must_not`` may also carry the key ``"graph"`` (no payload key: a condition on the point's node,
        ``graph_node_id or entity_name``): ``{"callers_of" | "callees_of" | "connected_to": name or list of names, "hops": 3,
        "relation": "calls", "include_self": True, "match": "exact" | "suffix"}`` keeps the points whose node calls / is called
        from / is connected to the named nodes within ``hops`` (1..16) edges given to :meth:`set_graph_edges` -- one BFS on the
        device, the result a row bitmap like a text condition's, combinable with everything a filter combines
        with except per-query filter lists; under ``must_not`` those points are excluded.  Names that are no node match nothing.
        Instead of a walk the entry may ask about the node's place in the WHOLE graph, with ``"relation"``
        beside it: ``{"in_cycle": True}`` -- the node lies in a cycle of the relation (it calls itself, or is one of several
        nodes that all reach each other) --, ``{"same_cycle_as": name}``, or ``{"depth" | "height": int or range mapping}`` --
        its layer below the entry points / above the leaves (:meth:`graph_layers`).  Components and layers are found on the
        device once per relation and graph version.  Or it asks for the code BETWEEN two node sets:
        ``{"between": [source or names, target or names], "hops": 8, "shortest": False, "relation": "calls", "match":
        "exact"}`` keeps the points whose node lies on a WALK of at most ``hops`` edges from a source to a target, both ends
        included (a walk, not a simple path: its two halves may share a node); ``"shortest": True`` keeps the nodes of the
        shortest chains only."""
        try:
            if score_threshold is not None:
                if query_vector is None:
                    raise ValueError("score_threshold needs a query vector (the filter-only fetch has no scores)")
                return (await self._range_call(collection, [query_vector], score_threshold, limit, filters, must_not, False,
                                               diversity=diversity is not None, group_by=group_by is not None, candidates=candidates is not None,
                                               max_overlap=max_overlap is not None))[0][0]
            group, candidates = self._group_args(collection, limit, group_by, group_size, diversity, candidates, query_vector is not None)
            if max_overlap is not None:
                group, candidates = self._span_args(collection, limit, max_overlap, candidates, diversity, group, query_vector is not None)
            if query_vector is not None and group is None:
                diversity, candidates = self._mmr_args(limit, diversity, candidates)
            if query_vector is None:
                def fetch():
                    col = self._col(collection)
                    slots = col.matching_slots(filters, limit=limit, must_not=must_not)
                    return col.hits(slots, [0.0] * len(slots))
                results = await self._run(fetch)
            elif len(query_vector) != self._col(collection).shards.dim:   # (must not fail the pass it would have joined)
                raise ValueError(f"query dim {len(query_vector)} != index dim {self._col(collection).shards.dim}")
            elif limit > ffi.MAX_K:                                      # (likewise: only THIS caller is refused)
                raise ValueError(f"limit {limit} exceeds the index's maximum k of {ffi.MAX_K}")
            elif self._search_coalesce:
                results = await self._search_coalesced(collection, query_vector, limit, filters, must_not, diversity, candidates, group)
            else:
                q = np.asarray(query_vector, dtype=np.float32).reshape(1, -1)
                self.search_passes += 1
                results = (await self._run(self._search_hits_sync, collection, q, limit, filters, must_not, diversity, candidates, group))[0]
            logger.debug(f"Found {len(results)} results in {collection}")
            return results
        except Exception as e:
            raise VectorStoreError(f"Failed to search {collection}", cause=e)

    async def _search_coalesced(self, collection: str, query_vector, limit: int, filters: dict[str, Any] | None,
                                must_not: dict[str, Any] | None = None, diversity: float | None = None, candidates: int | None = None,
                                group: tuple | None = None):
        """One entry of a coalesced pass: queue the query, let the key's drainer run the batch, return this call's slice.
        Calls are grouped by (collection, filter); the pass asks for the largest limit of the group and each caller keeps
        its own prefix (an exact top-k list is a prefix of every longer one).  Diversified calls are grouped by their
        (diversity, candidates) as well -- one candidate list, one greedy order, each caller its prefix of it -- and never
        share a pass with plain ones (whose key carries (None, None)).  Grouped calls likewise: their key carries
        (group_by, group_size, candidates), and the first j rows of a grouped answer are the j-row answer."""
        loop = asyncio.get_running_loop()
        name = collection.value if isinstance(collection, CollectionName) else collection
        vec = np.asarray(query_vector, dtype=np.float32).reshape(-1)
        fut: asyncio.Future = loop.create_future()
        if self._coalesce_filters and diversity is None and group is None and not has_text_condition(filters, must_not) and not has_graph_condition(filters, must_not):
            # (a text condition is one grep per pass, not one per query: such calls are keyed by their filter below)
            # plain calls of one collection travel together whatever their filters: each entry carries its own
            key = (name, "any filter")
            self._search_pending.setdefault(key, []).append((vec, int(limit), fut, filters, must_not))
            task = self._search_drainers.get(key)
            if task is None or task.done():
                self._search_drainers[key] = loop.create_task(self._drain_searches_mixed(key, name))
            return await fut
        key = (name, tuple(sorted((k, _value_key(v)) for k, v in (filters or {}).items())),
               tuple(sorted((k, _value_key(v)) for k, v in (must_not or {}).items())), (diversity, candidates), group)
        self._search_pending.setdefault(key, []).append((vec, int(limit), fut))
        task = self._search_drainers.get(key)
        if task is None or task.done():
            self._search_drainers[key] = loop.create_task(self._drain_searches(key, name, filters, must_not, diversity, candidates, group))
        return await fut

    async def _drain_searches_mixed(self, key, name: str) -> None:
        """The drainer of ``coalesce_filters``: like :meth:`_drain_searches`, with every entry's own filter handed on per query.
        ``search_passes`` counts the corpus passes the batch really costs: 64 queries of up to 8 distinct filters each."""
        while self._search_pending.get(key):
            await asyncio.sleep(self._search_window_s)
            batch = self._search_pending.pop(key, [])
            if not batch:
                break
            for start in range(0, len(batch), 256):
                part = batch[start:start + 256]
                try:
                    q = np.stack([b[0] for b in part])
                    keys = [_filter_key(b[3], b[4]) for b in part]
                    distinct = {k: i for i, k in enumerate(dict.fromkeys(keys))}
                    if len(distinct) == 1:                               # (one filter: the pass of _drain_searches, counted its way)
                        self.search_passes += (len(part) + 63) // 64
                        per_query = await self._run(self._search_hits_sync, name, q, [b[1] for b in part], part[0][3], part[0][4])
                    else:
                        self.search_passes += ffi.multi_passes([[(0, i)] for i in range(len(distinct))], [distinct[k] for k in keys])
                        per_query = await self._run(self._search_hits_sync, name, q, [b[1] for b in part], [b[3] for b in part], [b[4] for b in part])
                    for b, hits in zip(part, per_query):
                        if not b[2].done():
                            b[2].set_result(hits)
                except Exception as e:  # noqa: BLE001 -- every caller of the pass sees the failure (wrapped by search())
                    for b in part:
                        if not b[2].done():
                            b[2].set_exception(e)

    async def _drain_searches(self, key, name: str, filters, must_not=None, diversity=None, candidates=None, group=None) -> None:
        while self._search_pending.get(key):
            await asyncio.sleep(self._search_window_s)       # (0: one turn of the loop, so calls issued together travel together)
            batch = self._search_pending.pop(key, [])
            if not batch:
                break
            for start in range(0, len(batch), 256):
                part = batch[start:start + 256]
                try:
                    q = np.stack([b[0] for b in part])
                    self.search_passes += (len(part) + 63) // 64
                    per_query = await self._run(self._search_hits_sync, name, q, [b[1] for b in part], filters, must_not, diversity, candidates, group)
                    for (_, _, fut), hits in zip(part, per_query):
                        if not fut.done():
                            fut.set_result(hits)
                except Exception as e:  # noqa: BLE001 -- every caller of the pass sees the failure (wrapped by search())
                    for _, _, fut in part:
                        if not fut.done():
                            fut.set_exception(e)

    async def search_batch(self, collection: str, query_vectors, limit: int = 10,
                           filters=None, must_not=None, *,
                           diversity: float | None = None, candidates: int | None = None,
                           group_by: str | None = None, group_size: int = 1, score_threshold=None,
                           max_overlap: float | None = None) -> list[list[dict[str, Any]]]:
        """Batched form of :meth:`search` (not in the reference, which sends one query per RPC): one corpus scan
        serves up to 64 queries.  ``diversity`` / ``candidates`` / ``group_by`` / ``group_size`` as in :meth:`search`.
        ``filters`` and ``must_not`` may each be a dict for the whole batch, as in :meth:`search`, or a SEQUENCE with one dict
        (or None) per query: every query is then answered under its own filter, exactly as a lone :meth:`search` with that
        filter would answer it, and up to 8 distinct filters share each 64-query pass.  A filter naming a
        value the collection never stored yields an empty list for its own queries only.  Per-query filters cannot be combined
        with ``diversity`` or ``group_by`` (``ValueError``; a follow-up).  ``score_threshold`` as in :meth:`search`, one number or
        one per query; not combinable with ``diversity``, ``group_by`` or per-query filters.  ``max_overlap`` as in :meth:`search`;
        not combinable with ``diversity``, ``group_by``, ``score_threshold`` or per-query filters."""
        try:
            if score_threshold is not None:
                return (await self._range_call(collection, query_vectors, score_threshold, limit, filters, must_not, False,
                                               diversity=diversity is not None, group_by=group_by is not None, candidates=candidates is not None,
                                               max_overlap=max_overlap is not None))[0]
            per_query = isinstance(filters, (list, tuple)) or isinstance(must_not, (list, tuple))
            if per_query and (diversity is not None or group_by is not None):
                raise ValueError("per-query filters cannot be combined with diversity or group_by")
            group, candidates = self._group_args(collection, limit, group_by, group_size, diversity, candidates)
            if max_overlap is not None:
                group, candidates = self._span_args(collection, limit, max_overlap, candidates, diversity, group, per_query=per_query)
            if group is None:
                diversity, candidates = self._mmr_args(limit, diversity, candidates)
            elif limit > ffi.MAX_K:
                raise ValueError(f"limit {limit} exceeds the index's maximum k of {ffi.MAX_K}")
            q = np.asarray(query_vectors, dtype=np.float32)
            return await self._run(self._search_hits_sync, collection, q, limit, filters, must_not, diversity, candidates, group)
        except Exception as e:
            raise VectorStoreError(f"Failed to search {collection}", cause=e)

    def _fused_args(self, collection: str, sets, limit: int, fusion, rrf_k: int, weights, candidates: int | None):
        """Checked ``(queries [nq, m, dim], live [nq, m] or None, method, rrf_k, weights, candidates)`` of one fused call; raises
        ``ValueError`` for the caller alone.  ``candidates`` -- the depth of every sub-query's list -- defaults to
        ``min(MAX_K // m, 4 * limit)``."""
        method = ffi.fuse_method(fusion)
        dim = self._col(collection).shards.dim
        sets = [np.asarray(one, dtype=np.float32) for one in sets]
        sets = [one.reshape(0, dim) if one.size == 0 else one for one in sets]
        for one in sets:
            if one.ndim != 2 or one.shape[1] != dim:
                raise ValueError(f"a fused query is a set of vectors [m, {dim}], got shape {tuple(one.shape)}")
        m = max((len(one) for one in sets), default=1)
        if m < 1 or any(len(one) < 1 for one in sets):
            raise ValueError("a fused query needs at least one query vector")
        if m > ffi.MAX_LISTS:
            raise ValueError(f"{m} query vectors exceed the {ffi.MAX_LISTS} lists one fusion takes")
        limit, rrf_k = int(limit), int(rrf_k)
        if limit > ffi.MAX_K:
            raise ValueError(f"limit {limit} exceeds the index's maximum k of {ffi.MAX_K}")
        if rrf_k < 0 or rrf_k > 2**31 - 1:
            raise ValueError(f"rrf_k {rrf_k} must be >= 0")
        weights = ffi.fuse_weights(weights, m, method)
        if candidates is None:
            candidates = min(ffi.MAX_K // m, 4 * max(limit, 1))
        candidates = int(candidates)
        if candidates < limit or candidates < 1 or m * candidates > ffi.MAX_K:
            raise ValueError(f"candidates {candidates} must be >= limit ({limit}) and {m} lists x candidates <= {ffi.MAX_K}")
        queries = np.zeros((len(sets), m, dim), np.float32)
        live = np.zeros((len(sets), m), bool)
        for i, one in enumerate(sets):
            queries[i, :len(one)] = one
            live[i, :len(one)] = True
        return queries, (None if live.all() else live), fusion.lower(), rrf_k, weights, candidates

    def _search_fused_sync(self, collection: str, queries: np.ndarray, live, limit: int, filters, must_not, method: str, rrf_k: int,
                           weights, candidates: int) -> list[list[dict[str, Any]]]:
        """One fused pass + the hit dictionaries of every logical query, built inside the worker job, under the store's lock
        (slots are only good until the next compaction: :meth:`_search_hits_sync`)."""
        col = self._col(collection)
        nq = queries.shape[0]
        dfilt = col.device_filters(filters, must_not)
        if dfilt is None or limit <= 0 or nq == 0:
            return [[] for _ in range(nq)]
        slots, fused, cos, lists = col.search_fused(queries, limit, candidates, dfilt, method, rrf_k, weights, live)

        def decorate(hits, keep):
            for h, cv, bits in zip(hits, cos[keep].tolist(), lists[keep].tolist()):
                h["cosine"] = cv
                h["matched"] = [j for j in range(ffi.MAX_LISTS) if bits >> j & 1]
        return self._hit_lists(col, slots, fused, decorate=decorate)

    async def search_fused_batch(self, collection: str, query_vector_sets, limit: int = 10,
                                 filters: dict[str, Any] | None = None, must_not: dict[str, Any] | None = None, *,
                                 fusion: str = "rrf", rrf_k: int = 60, weights=None, candidates: int | None = None,
                                 score_threshold=None) -> list[list[dict[str, Any]]]:
        """Batched :meth:`search_fused`: ``query_vector_sets`` is a list of sets of query vectors, one set per logical query;
        the sets may differ in size (a shorter one fuses its own lists only, and ``weights`` / the default ``candidates`` go by
        the largest).  All sub-queries of the batch share corpus passes of 64, under ONE filter.  The batch is searched as
        ``len(sets) * m`` queries with ``m`` the largest set: the absent members of shorter sets are searched as zero vectors
        and their lists discarded -- wasted slots of the pass, so sets of very different sizes are better sent apart.
        ``search_passes`` counts ``ceil(len(sets) * m / 64)`` for every call that passes its argument checks, also when the
        filter names a value the collection never stored and nothing is searched.  ``score_threshold`` is accepted to be
        refused: a fused score is not a cosine, and a threshold on the sub-queries' lists is a follow-up (``ValueError``)."""
        try:
            if score_threshold is not None:
                self._range_args(score_threshold, 1, fusion=True)
            q, live, method, rrf_k, weights, candidates = self._fused_args(collection, list(query_vector_sets), limit, fusion, rrf_k, weights, candidates)
            self.search_passes += (q.shape[0] * q.shape[1] + 63) // 64
            return await self._run(self._search_fused_sync, collection, q, live, int(limit), filters, must_not, method, rrf_k, weights, candidates)
        except Exception as e:
            raise VectorStoreError(f"Failed to search {collection}", cause=e)

    async def search_fused(self, collection: str, query_vectors, limit: int = 10,
                           filters: dict[str, Any] | None = None, must_not: dict[str, Any] | None = None, *,
                           fusion: str = "rrf", rrf_k: int = 60, weights=None, candidates: int | None = None,
                           score_threshold=None) -> list[dict[str, Any]]:
        """ONE logical query asked in ``m`` ways (``query_vectors`` [m, dim], m <= 16: the original text and its reformulations,
        a HyDE answer, ...): every vector's ``candidates`` best hits, fused on the device into one list of ``limit`` (DESIGN.md
        3.16; Qdrant's ``prefetch=[...]`` + ``FusionQuery``; not in the reference, whose engine searches the original text only).
        ``fusion="rrf"``: reciprocal-rank fusion, a hit's ``score`` is the sum over the lists that hold it of ``weights[j] /
        (rrf_k + rank + 1)`` (rank 0 = best; ``weights`` default to 1).  ``fusion="max"``: ``score`` is the hit's best cosine over
        the ``m`` vectors -- exactly the top-``limit`` of the corpus under that maximum.  Hits are ``{"id", "score", "payload",
        "cosine", "matched"}``: ``cosine`` the best cosine among the lists that hold the hit, ``matched`` the ascending indexes
        of those lists.  ``candidates`` (default ``min(MAX_K // m, 4 * limit)``; ``limit <= candidates``, ``m * candidates <=
        MAX_K``) is the depth of every list.  ``filters`` / ``must_not`` as in :meth:`search`, one filter for all ``m`` vectors.
        A fused call takes a pass of its own (it never joins the coalescer)."""
        return (await self.search_fused_batch(collection, [query_vectors], limit, filters, must_not, fusion=fusion, rrf_k=rrf_k,
                                              weights=weights, candidates=candidates, score_threshold=score_threshold))[0]

    # ------------------------------------------------------------------ keyword and hybrid search
    @staticmethod
    def _lexical_args(texts, limit: int, filters, must_not, k1: float, b: float) -> tuple[list, int, float, float]:
        """Checked ``(texts, limit, k1, b)`` of a lexical call; ``ValueError`` for the caller alone, before anything runs."""
        texts = list(texts)
        if not all(isinstance(t, (str, bytes)) for t in texts):
            raise ValueError("a lexical query is a text (str or bytes)")
        if isinstance(filters, (list, tuple)) or isinstance(must_not, (list, tuple)):
            raise ValueError("lexical and hybrid searches take one filter for the whole batch, not per-query filters")
        limit, k1, b = int(limit), float(k1), float(b)
        if limit > ffi.MAX_K:
            raise ValueError(f"limit {limit} exceeds the index's maximum k of {ffi.MAX_K}")
        if not (math.isfinite(k1) and k1 >= 0.0 and 0.0 <= b <= 1.0):
            raise ValueError(f"BM25 needs k1 >= 0 and 0 <= b <= 1, got k1={k1} b={b}")
        return texts, limit, k1, b

    def _search_lexical_sync(self, collection: str, texts: list, limit: int, filters, must_not, k1: float, b: float):
        """One lexical pass + the hit dictionaries of every text, built inside the worker job (:meth:`_search_hits_sync`):
        ``(hits per text, qualifying rows per text)``.  ``limit`` 0 asks for the counts alone."""
        col = self._col(collection)
        dfilt = col.device_filters(filters, must_not)
        if col.shards.backend == "dist":
            col._lex_ready()                                             # (raises: not available there yet)
        if dfilt is None or not texts:
            return [[] for _ in texts], [0] * len(texts)
        scores, slots, counts = col.search_lexical(texts, max(limit, 1), dfilt, k1, b)
        return self._hit_lists(col, slots, scores, limit), [int(c) for c in counts]

    async def search_lexical_batch(self, collection: str, texts, limit: int = 10, filters: dict[str, Any] | None = None,
                                   must_not: dict[str, Any] | None = None, *, k1: float = 1.2, b: float = 0.75) -> list[list[dict[str, Any]]]:
        """Batched :meth:`search_lexical`: one list of hits per text, all texts under ONE filter, 64 texts per pass over the
        forward index."""
        try:
            texts, limit, k1, b = self._lexical_args(texts, limit, filters, must_not, k1, b)
            return (await self._run(self._search_lexical_sync, collection, texts, limit, filters, must_not, k1, b))[0]
        except Exception as e:
            raise VectorStoreError(f"Failed to search {collection}", cause=e)

    async def search_lexical(self, collection: str, text: str, limit: int = 10, filters: dict[str, Any] | None = None,
                             must_not: dict[str, Any] | None = None, *, k1: float = 1.2, b: float = 0.75) -> list[dict[str, Any]]:
        """Exact keyword search (BM25) over the points' ``entity_name`` / ``content`` / ``summary``: where is
        ``parse_retry_after``, who mentions ``HTTPServerError`` (Qdrant's sparse BM25 vectors).  ``text`` is cut
        like the stored text -- identifiers into their sub-words AND kept whole -- and a point qualifies iff it is alive,
        passes the filter and holds at least one of the terms.  Hits ``{"id", "score", "payload"}`` by descending BM25 score
        (idf and average length those of the whole collection's alive points), ties to the earlier row.  A text with more than
        32 distinct terms is searched by its 32 rarest.  The keyword index is built from the payloads on the first such call
        and kept up to date lazily; not available with ``shard_backend="dist"`` yet."""
        return (await self.search_lexical_batch(collection, [text], limit, filters, must_not, k1=k1, b=b))[0]

    async def lexical_count(self, collection: str, text: str, filters: dict[str, Any] | None = None,
                            must_not: dict[str, Any] | None = None) -> int:
        """How many alive points under the filter hold at least one term of ``text``: exact, not clipped at any ``limit``."""
        try:
            texts, _, k1, b = self._lexical_args([text], 0, filters, must_not, 1.2, 0.75)
            return (await self._run(self._search_lexical_sync, collection, texts, 0, filters, must_not, k1, b))[1][0]
        except Exception as e:
            raise VectorStoreError(f"Failed to count in {collection}", cause=e)

    # ------------------------------------------------------------------ literal text search
    def _search_text_sync(self, collection: str, contains, limit: int, filters, must_not, any_of: bool, case: bool, matches=None,
                          fuzzy=None, edits=None) -> dict[str, Any]:
        """The text condition joined to the filter, the exact count and the first ``limit`` matching points in insertion order
        (``crh_index_match_rows_cond``), with their ``match_line``; ``limit`` 0 asks for the count alone.  With ``fuzzy`` the
        points come by ``(distance, insertion order)``: level by level, the rows of level ``d`` that are not of level ``d - 1``."""
        col = self._col(collection)
        if not col.text_keys:
            raise ValueError(f"collection {col.name!r} has no text key to search")
        key = col.text_keys[0]
        if isinstance(filters, (list, tuple)) or isinstance(must_not, (list, tuple)):
            raise ValueError("a text search takes one filter, not per-query filters")
        if key in (filters or {}):
            raise ValueError(f"the filter already holds a condition on {key!r}: give the strings in `contains`, the expression in `matches`, "
                             f"the approximate string in `fuzzy`")
        if contains is None and matches is None and fuzzy is None:
            raise ValueError("a text search needs `contains` (strings), `matches` (a regular expression), `fuzzy` (a string within `edits` edits) or several of them")
        spec = {"any": any_of, "case": case}
        if contains is not None:
            spec["contains"] = contains
        if matches is not None:
            spec["matches"] = matches
        if fuzzy is not None:
            spec["fuzzy"] = fuzzy
        if edits is not None:
            spec["edits"] = edits
        if fuzzy is not None:
            return self._search_fuzzy_sync(col, key, spec, limit, filters, must_not)
        dfilt = col.device_filters({**(filters or {}), key: spec}, must_not)
        if dfilt is None:
            return {"hits": [], "count": 0}
        count = int(col.shards.count_matching(dfilt))
        if limit <= 0 or count == 0:
            return {"hits": [], "count": count}
        sh, lo = col.shards.match_rows(dfilt, int(limit))
        slots = np.sort(col.slots_of(sh, lo))[: int(limit)]
        hits = col.hits(slots, [0.0] * len(slots))
        checked = text_spec(key, spec)
        pats = checked.patterns
        rx = None if checked.regex is None else re.compile(checked.regex, re.MULTILINE | (0 if case else re.IGNORECASE))
        for hit in hits:
            text, start = hit["payload"].get(key), hit["payload"].get("start_line")
            raw = text.encode("utf-8", "surrogatepass") if isinstance(text, str) else b""
            where = [p for p in ((raw if case else raw.translate(_ASCII_LOWER)).find(pat) for pat in pats) if p >= 0]
            found = rx.search(raw) if rx is not None else None
            if found is not None:
                where.append(found.start())
            first = type(start) is int and where
            hit["match_line"] = start + raw.count(b"\n", 0, min(where)) if first else None
        return {"hits": hits, "count": count}

    def _search_fuzzy_sync(self, col: "_Collection", key: str, spec: dict, limit: int, filters, must_not) -> dict[str, Any]:
        """:meth:`_search_text_sync` with an approximate pattern: one resolution of the filter (which walks the text once, every
        level at a time), then per level ``d`` the first rows of level ``d`` (``CRH_COND_WORDS``) that are not of level ``d - 1``
        (``CRH_COND_NOT_WORDS``), until ``limit`` points are fetched.  The levels hold every condition that is no text condition
        already (the walk ran under their words), so the two row bitmaps are the whole filter of a fetch -- unless ``must_not``
        carries a text condition of its own: text conditions are resolved beside each other, never under each other, so its row
        bitmap joins every fetch, and the rows at each distance are then counted under it (``count_matching``) instead of taken
        from the walk.  ``distance`` and ``match_line`` of the returned points are computed on the host, by the definition."""
        checked = text_spec(key, spec)
        none = {"hits": [], "count": 0, "counts_by_distance": [0] * (checked.edits + 1)}
        dfilt = col.device_filters({**(filters or {}), key: spec}, must_not)
        if dfilt is None:
            return none
        levels, by_distance = col._text_levels(key, checked, [c for c in dfilt if not isinstance(c, ffi.RowWords)])
        # the other text conditions (must_not's): every row bitmap of the filter but the fuzzy condition's own, which is the last level
        beside = [c for c in dfilt if isinstance(c, ffi.RowWords) and (c.negate or c.tag != levels[-1].tag)]

        def exactly(d: int) -> list:
            return [levels[d]] + ([ffi.RowWords(levels[d - 1].tag, levels[d - 1].words, True)] if d else []) + beside

        if beside:
            by_distance = [int(col.shards.count_matching(exactly(d))) for d in range(len(levels))]
        out = {"hits": [], "count": int(sum(by_distance)), "counts_by_distance": [int(c) for c in by_distance]}
        for d in range(len(levels)):
            want = int(limit) - len(out["hits"])
            if want <= 0:
                break
            if by_distance[d] == 0:
                continue
            sh, lo = col.shards.match_rows(exactly(d), want)
            slots = np.sort(col.slots_of(sh, lo))[:want]
            for hit in col.hits(slots, [0.0] * len(slots)):
                text, start = hit["payload"].get(key), hit["payload"].get("start_line")
                raw = text.encode("utf-8", "surrogatepass") if isinstance(text, str) else b""
                dist, last = fuzzy_distance(checked.fuzzy, raw if checked.case else raw.translate(_ASCII_LOWER))
                hit["distance"] = dist
                hit["match_line"] = start + raw.count(b"\n", 0, max(last, 0)) if type(start) is int else None
                out["hits"].append(hit)
        return out

    async def search_text(self, collection: str, contains=None, limit: int = 10, filters: dict[str, Any] | None = None,
                          must_not: dict[str, Any] | None = None, *, matches: str | None = None, any: bool = False,   # noqa: A002
                          case: bool = True, fuzzy: str | None = None, edits: int | None = None) -> dict[str, Any]:
        """Literal text search -- grep over the stored chunks: the points whose text (``content`` of the code chunks, ``summary``
        of the summaries) holds the string ``contains``, or every string of a list (``any``: at least one), under ``filters`` /
        ``must_not`` as in :meth:`search`.  ``case=False`` folds ASCII letters only.  Returns ``{"hits": [...], "count": int}``:
        ``hits`` are the first ``limit`` matching points in insertion order (``{"id", "score": 0.0, "payload", "match_line"}``),
        ``count`` how many points match, exact and not clipped at ``limit``.  ``match_line`` is ``start_line`` plus the number of
        newlines before the first occurrence of any of the strings (None for a point without an int ``start_line``).  Matched
        on the device; 1..8 strings of 1..64 bytes of UTF-8 each.

        ``matches`` is a regular expression in the syntax of Python's ``re`` ON BYTES, with ``re.MULTILINE``:
        the points in whose text ``re.search`` finds it; beside ``contains`` both must hold (``any`` concerns the strings
        only, ``case`` both).  At least one of ``contains`` and ``matches`` is required.  ``match_line`` counts the newlines
        before the earliest place where one of the strings occurs or the expression's first match starts.

        ``fuzzy`` is a string the text must hold within ``edits`` edits: some substring of the text is at most
        ``edits`` insertions, deletions or substitutions of one BYTE away from it (a transposition is two; a multi-byte
        character counts per byte; ``case=False`` folds ASCII letters on both sides).  ``edits`` is 0..3 and less than the
        string's bytes; left out it is 1 for up to 5 bytes and 2 above.  Beside ``contains`` / ``matches`` all must hold.  The
        hits then come ordered by ``(distance, insertion order)`` and carry ``distance`` -- the least edit distance between the
        string and any substring of the text -- and ``match_line``: ``start_line`` plus the newlines before the LAST byte of the
        first substring that reaches that distance.  The result also carries ``counts_by_distance``, the exact number of
        matching points at each distance ``0 .. edits`` (``count`` is their sum)."""
        try:
            return await self._run(self._search_text_sync, collection, contains, int(limit), filters, must_not, any, case, matches, fuzzy, edits)
        except Exception as e:
            raise VectorStoreError(f"Failed to search {collection}", cause=e)

    async def count_text(self, collection: str, contains=None, filters: dict[str, Any] | None = None, must_not: dict[str, Any] | None = None, *,
                         matches: str | None = None, any: bool = False, case: bool = True, fuzzy: str | None = None,   # noqa: A002
                         edits: int | None = None) -> int:
        """How many points :meth:`search_text` matches: exact."""
        try:
            return (await self._run(self._search_text_sync, collection, contains, 0, filters, must_not, any, case, matches, fuzzy, edits))["count"]
        except Exception as e:
            raise VectorStoreError(f"Failed to count in {collection}", cause=e)

    def _search_hybrid_sync(self, collection: str, queries: np.ndarray, texts: list, limit: int, candidates: int, rrf_k: int, weights,
                            filters, must_not, k1: float, b: float) -> list[list[dict[str, Any]]]:
        col = self._col(collection)
        dfilt = col.device_filters(filters, must_not)
        if col.shards.backend == "dist":
            col._lex_ready()
        if dfilt is None or limit <= 0 or not texts:
            return [[] for _ in texts]
        slots, fused, cos, lexs, lists = col.search_hybrid(queries, texts, limit, candidates, dfilt, rrf_k, weights, k1, b)

        def decorate(hits, keep):
            for h, cv, lv, bits in zip(hits, cos[keep].tolist(), lexs[keep].tolist(), lists[keep].tolist()):
                h["cosine"] = None if math.isnan(cv) else cv
                h["lexical_score"] = None if math.isnan(lv) else lv
                h["matched"] = tuple(name for j, name in enumerate(("vector", "lexical")) if bits >> j & 1)
        return self._hit_lists(col, slots, fused, decorate=decorate)

    async def search_hybrid_batch(self, collection: str, query_vectors, texts, limit: int = 10, candidates: int | None = None,
                                  rrf_k: int = 60, weights=None, filters: dict[str, Any] | None = None,
                                  must_not: dict[str, Any] | None = None, *, fusion: str = "rrf", k1: float = 1.2, b: float = 0.75,
                                  diversity=None, group_by=None, max_overlap=None, score_threshold=None) -> list[list[dict[str, Any]]]:
        """Batched :meth:`search_hybrid`: query ``i`` is ``(query_vectors[i], texts[i])``; all under ONE filter."""
        try:
            used = [name for name, v in (("diversity", diversity), ("group_by", group_by), ("max_overlap", max_overlap),
                                         ("score_threshold", score_threshold)) if v is not None]
            if used:
                raise ValueError(f"a hybrid search cannot be combined with {', '.join(used)} (a follow-up: those select from one "
                                 "candidate list, the fusion from two)")
            if ffi.fuse_method(fusion) != ffi.FUSE_RRF:
                raise ValueError("a hybrid search fuses by rank (fusion='rrf'): a cosine and a BM25 score are on different scales")
            texts, limit, k1, b = self._lexical_args(texts, limit, filters, must_not, k1, b)
            q = np.asarray(query_vectors, dtype=np.float32)
            dim = self._col(collection).shards.dim
            q = q.reshape(0, dim) if q.size == 0 else q
            if q.ndim != 2 or q.shape[1] != dim or q.shape[0] != len(texts):
                raise ValueError(f"{len(texts)} texts need query vectors [{len(texts)}, {dim}], got shape {tuple(q.shape)}")
            rrf_k = int(rrf_k)
            if rrf_k < 0 or rrf_k > 2**31 - 1:
                raise ValueError(f"rrf_k {rrf_k} must be >= 0")
            weights = ffi.fuse_weights(weights, 2, ffi.FUSE_RRF)
            candidates = min(ffi.MAX_K // 2, 4 * max(limit, 1)) if candidates is None else int(candidates)
            if candidates < limit or candidates < 1 or 2 * candidates > ffi.MAX_K:
                raise ValueError(f"candidates {candidates} must be >= limit ({limit}) and 2 lists x candidates <= {ffi.MAX_K}")
            self.search_passes += (q.shape[0] + 63) // 64
            return await self._run(self._search_hybrid_sync, collection, q, texts, limit, candidates, rrf_k, weights, filters, must_not, k1, b)
        except Exception as e:
            raise VectorStoreError(f"Failed to search {collection}", cause=e)

    async def search_hybrid(self, collection: str, query_vector, text: str, limit: int = 10, candidates: int | None = None,
                            rrf_k: int = 60, weights=None, filters: dict[str, Any] | None = None,
                            must_not: dict[str, Any] | None = None, **kw) -> list[dict[str, Any]]:
        """Dense and keyword search fused (Qdrant's ``query_points(prefetch=[dense, sparse], query=FusionQuery(RRF))``): the
        ``candidates`` best hits of ``query_vector`` and the ``candidates`` best BM25 hits of ``text`` (default ``4 * limit``;
        ``2 * candidates <= MAX_K``) under the same filter, fused on the device by reciprocal rank (``rrf_k``, ``weights`` =
        ``(vector, lexical)``, default 1 each) into ``limit`` hits.  A hit carries ``score`` (fused), ``cosine`` and
        ``lexical_score`` -- each None when that list did not hold the point -- and ``matched``, a subset of ``("vector",
        "lexical")``.  ``fusion="max"`` is refused (the scales differ); not combinable with ``diversity``, ``group_by``,
        ``max_overlap``, ``score_threshold`` or per-query filter lists."""
        return (await self.search_hybrid_batch(collection, [query_vector], [text], limit, candidates, rrf_k, weights, filters, must_not, **kw))[0]

    def _recommend_args(self, collection: str, sets, limit: int, strategy, candidates: int | None):
        """Checked ``(positive ids, negative ids, P, N, strategy, candidates)`` of one recommend call; raises ``ValueError`` for
        the caller alone.  ``candidates`` -- the depth of every positive's list in round 1 of ``"best"`` -- defaults to
        ``4 * limit``, clipped so that ``P * candidates <= MAX_K``."""
        ffi.recommend_strategy(strategy)
        strategy = strategy.lower()
        self._col(collection)
        pos, neg = [], []
        for one in sets:
            if isinstance(one, (str, bytes)) or len(one) != 2:
                raise ValueError("a recommend query is a pair (positive ids, negative ids)")
            p_ids, n_ids = ([one[0]] if isinstance(one[0], str) else list(one[0])), ([one[1]] if isinstance(one[1], str) else list(one[1] or ()))
            if not 1 <= len(p_ids) <= ffi.MAX_POS or len(n_ids) > ffi.MAX_NEG:
                raise ValueError(f"a recommend query takes 1..{ffi.MAX_POS} positive and 0..{ffi.MAX_NEG} negative ids, got {len(p_ids)} and {len(n_ids)}")
            pos.append([str(i) for i in p_ids])
            neg.append([str(i) for i in n_ids])
        P, N = max((len(p) for p in pos), default=1), max((len(n) for n in neg), default=0)
        limit = int(limit)
        if limit > ffi.MAX_K or (strategy == "average" and limit + P + N > ffi.MAX_K):
            raise ValueError(f"limit {limit} (plus the examples under 'average') exceeds the index's maximum k of {ffi.MAX_K}")
        if candidates is None:
            candidates = max(1, min(ffi.MAX_K // P, 4 * max(limit, 1)))
        candidates = int(candidates)
        if candidates < 1 or P * candidates > ffi.MAX_K:
            raise ValueError(f"candidates {candidates} must be >= 1 and {P} lists x candidates <= {ffi.MAX_K}")
        return pos, neg, P, N, strategy, candidates

    def _recommend_sync(self, collection: str, pos, neg, P: int, N: int, limit: int, filters, must_not, strategy: str,
                        candidates: int) -> list[list[dict[str, Any]]]:
        """The ids resolved, one recommend call and the hit dictionaries of every logical query, built inside the worker job,
        under the store's lock (slots are only good until the next compaction: :meth:`_search_hits_sync`)."""
        col = self._col(collection)
        nq = len(pos)
        slots = np.full((nq, P + N), -1, np.int64)
        flat = [i for p, n in zip(pos, neg) for i in p + n]
        found = col.ids.lookup(flat) if flat else np.zeros((0,), np.int64)
        alive = np.zeros(found.shape, bool)
        if (found >= 0).any():
            alive[found >= 0] = col.shards.rows_alive(*col.rows_of(found[found >= 0]))
        missing = [i for i, ok in zip(flat, alive) if not ok]
        if missing:
            raise ValueError(f"unknown or deleted point id {missing[0]!r}")
        at = 0
        for q, (p, n) in enumerate(zip(pos, neg)):
            slots[q, :len(p)] = found[at:at + len(p)]
            slots[q, P:P + len(n)] = found[at + len(p):at + len(p) + len(n)]
            at += len(p) + len(n)
        dfilt = col.device_filters(filters, must_not)
        if dfilt is None or limit <= 0 or nq == 0:
            return [[] for _ in range(nq)]
        n_pos, n_neg = np.asarray([len(p) for p in pos], np.int32), np.asarray([len(n) for n in neg], np.int32)
        ragged = bool((n_pos != P).any() or (n_neg != N).any())
        got, score, nscore, best = col.recommend(slots, P, N, limit, candidates, dfilt, strategy, n_pos if ragged else None, n_neg if ragged else None)

        def decorate(hits, keep):
            for h, q, nv, b in zip(hits, np.nonzero(keep)[0].tolist(), nscore[keep].tolist(), best[keep].tolist()):
                h["negative_score"] = nv
                h["matched_positive"] = pos[q][b]
        return self._hit_lists(col, got, score, decorate=decorate if strategy == "best" else None)

    async def recommend_batch(self, collection: str, example_sets, limit: int = 10, strategy: str = "average",
                              filters: dict[str, Any] | None = None, must_not: dict[str, Any] | None = None,
                              candidates: int | None = None) -> list[list[dict[str, Any]]]:
        """Batched :meth:`recommend`: ``example_sets`` is a list of ``(positive ids, negative ids)`` pairs, one per logical
        query; the sets may differ in size (the batch runs at the largest ``P`` and ``N``; under ``"best"`` the absent positives
        are searched as zero vectors and their lists discarded).  All queries of the batch share corpus passes of 64, under ONE
        filter.  ``search_passes`` counts the passes of round 1."""
        try:
            pos, neg, P, N, strategy, candidates = self._recommend_args(collection, list(example_sets), limit, strategy, candidates)
            self.search_passes += (len(pos) * (P if strategy == "best" else 1) + 63) // 64
            return await self._run(self._recommend_sync, collection, pos, neg, P, N, int(limit), filters, must_not, strategy, candidates)
        except Exception as e:
            raise VectorStoreError(f"Failed to recommend in {collection}", cause=e)

    async def recommend(self, collection: str, positive, negative=(), limit: int = 10, strategy: str = "average",
                        filters: dict[str, Any] | None = None, must_not: dict[str, Any] | None = None,
                        candidates: int | None = None) -> list[dict[str, Any]]:
        """"More like these, not like those" (Qdrant's ``RecommendQuery(positive, negative, strategy)``; the
        reference's ``find_similar`` intent can only embed a snippet): ``positive`` (1..8) and ``negative`` (0..8) are ids of
        stored points -- no text is embedded again; an unknown or deleted id raises ``VectorStoreError`` naming it.  The example
        points themselves never appear in the answer; ``filters`` / ``must_not`` as in :meth:`search`.
        ``strategy="average"``: the exact top-``limit`` for the vector ``2 * mean(positive) - mean(negative)`` (the mean of the
        positives without negatives), computed on the device from the stored rows.  Hits are ``{"id", "score", "payload"}``.
        ``strategy="best"``: a point's ``score`` is its best cosine to a positive; it is dropped (not ranked last, as Qdrant
        does) when a negative is at least as close.  Hits also carry ``negative_score`` (the best cosine to a negative, -inf
        without negatives) and ``matched_positive`` (the id of the positive that gave ``score``).  The answer is exact: every
        returned hit is the hit of its position over the whole filtered collection; when two rounds of candidates (``candidates``
        per positive, default ``4 * limit``, then ``MAX_K // P``) cannot settle ``limit`` hits -- negatives that veto most of the
        positives' neighbourhood -- the list comes back shorter than ``limit``.  A recommend call takes passes of its own."""
        return (await self.recommend_batch(collection, [(positive, negative)], limit, strategy, filters, must_not, candidates))[0]

    async def search_groups(self, collection: str, query_vector: list[float], group_by: str, limit: int = 5, group_size: int = 3,
                            filters: dict[str, Any] | None = None, must_not: dict[str, Any] | None = None) -> list[dict[str, Any]]:
        """Qdrant's ``query_points_groups(group_by, limit, group_size)``, exact: ``[{"id": value, "hits": [...]}]`` -- the
        ``limit`` values of ``group_by`` whose best hit scores highest, in that order, each with its best ``group_size`` hits
        (``limit * group_size <= MAX_K``).  Rows without the key (or with None) are left out.  Two grouped searches: one hit
        per group names the groups; a second one, filtered to those values (a short any-of list: the sparse-mask route),
        fills them.  The caller's own ``filters`` / ``must_not`` hold in both (the groups found already satisfy them)."""
        try:
            limit, group_size = int(limit), int(group_size)
            if limit < 1 or group_size < 1 or limit * group_size > ffi.MAX_K:
                raise ValueError(f"search_groups: limit {limit} x group_size {group_size} must be within 1..{ffi.MAX_K}")
            if query_vector is None:
                raise ValueError("search_groups needs a query vector")
            self._col(collection)._column(group_by)
            banned = dict(must_not or {})
            mine = banned.get(group_by, [])
            banned[group_by] = [None] + list(mine if isinstance(mine, _COLLECTIONS) else [mine])       # (no value, no group)
            first = await self.search(collection, query_vector, limit=limit, filters=filters, must_not=banned, group_by=group_by, group_size=1)
            values = [h["payload"].get(group_by) for h in first]
            if not values:
                return []
            inside = dict(filters or {})
            inside[group_by] = values
            flat = await self.search(collection, query_vector, limit=len(values) * group_size, filters=inside, must_not=must_not,
                                     group_by=group_by, group_size=group_size)
            groups: dict[Any, dict[str, Any]] = {}
            for h in flat:                                                   # (first appearance = the group's best hit: the order asked for)
                v = h["payload"].get(group_by)
                groups.setdefault(_value_key(v), {"id": v, "hits": []})["hits"].append(h)
            return list(groups.values())
        except VectorStoreError:
            raise
        except Exception as e:
            raise VectorStoreError(f"Failed to search {collection}", cause=e)

    async def set_graph_degrees(self, collection: str, total_degree: dict[str, int]) -> None:
        """``{graph_node_id or entity_name: total_degree}`` for the device re-rank's centrality signal (the reference asks
        Memgraph per query, query/engine.py:348-377; a store that keeps the degrees beside the vectors answers on the device)."""
        await self._run(lambda: self._col(collection).set_degrees(total_degree))

    # ------------------------------------------------------------------ the call graph on the device
    async def set_graph_edges(self, collection: str, edges, relation: str = "calls", derive_degrees: bool = False) -> dict[str, Any]:
        """The edges of one named relation of the collection's graph (the reference keeps them in Memgraph): ``edges`` is an
        iterable of ``(source_name, target_name)``; a node is named like the chunks' key ``graph_node_id or entity_name``.  A
        call REPLACES that relation; up to 8 relations share one node numbering, in order of first appearance; repeats and
        self-loops are dropped from the edges (WHICH nodes carried a self-loop is kept: :meth:`graph_cycles` reports a function
        that calls itself).  ``derive_degrees``: the re-rank's centrality table (:meth:`set_graph_degrees`) is filled
        with every node's distinct in-degree + out-degree in this relation (GET_ENTITY_CENTRALITY's ``total_degree``).
        Returns :meth:`graph_info`."""
        try:
            edges = list(edges)
            return await self._run(lambda: self._col(collection).set_graph_edges(edges, relation, derive_degrees))
        except Exception as e:
            raise VectorStoreError(f"Failed to set the graph edges of {collection}", cause=e)

    async def graph_info(self, collection: str) -> dict[str, Any]:
        """``{"nodes": n, "relations": {name: edges}}``."""
        return await self._run(lambda: self._col(collection).graph_info())

    async def graph_neighbors_batch(self, collection: str, name_sets, direction: str = "callers", relation: str = "calls", max_hops: int = 3,
                                    limit: int = 50, include_self: bool = False, match: str = "exact") -> list[dict[str, Any]]:
        """:meth:`graph_neighbors` for a list of name sets (each a name or a list of names): one device BFS per 64 sets."""
        try:
            sets = [[s] if isinstance(s, str) else list(s) for s in name_sets]
            return await self._run(lambda: self._col(collection).graph_neighbors(sets, direction, relation, max_hops, limit, include_self, match))
        except Exception as e:
            raise VectorStoreError(f"Failed to walk the graph of {collection}", cause=e)

    async def graph_neighbors(self, collection: str, names, direction: str = "callers", relation: str = "calls", max_hops: int = 3,
                              limit: int = 50, include_self: bool = False, match: str = "exact") -> dict[str, Any]:
        """What reaches (``direction="callers"``), is reached from (``"callees"``) or is connected to (``"both"``) the named
        nodes within ``max_hops`` (1..16) edges of ``relation``: FIND_TRANSITIVE_CALLERS / _CALLEES of the reference's
        query/graph_reasoning/queries.py, as a bit-parallel BFS on the device.  Returns ``{"hits": [{"name", "depth"}], "count",
        "unresolved"}``: every reached node ONCE, at its minimum depth (the Cypher's DISTINCT over (node, depth) lists a node
        once per path length), ordered by (depth, order of first appearance in :meth:`set_graph_edges`), the first ``limit``
        of them; ``count`` is how many there are, never clipped; ``unresolved`` the names that are no node.  ``names``: one
        name or several (their union is the source set).  ``match="suffix"``: a name also stands for every node whose name ends
        in ``"." + name``.  ``include_self``: the sources themselves lead the list at depth 0."""
        return (await self.graph_neighbors_batch(collection, [names], direction, relation, max_hops, limit, include_self, match))[0]

    async def call_chain(self, collection: str, source: str, target: str, relation: str = "calls", max_hops: int = 8) -> list[str] | None:
        """One shortest chain of ``relation`` edges from ``source`` to ``target`` (FIND_CALL_CHAIN; at most ``max_hops`` edges,
        1..16) as the list of node names, both ends included -- or None.  ONE chain per pair: where several are equally short,
        each step back from the target takes the node :meth:`set_graph_edges` saw first."""
        try:
            return await self._run(lambda: self._col(collection).call_chain(source, target, relation, max_hops))
        except Exception as e:
            raise VectorStoreError(f"Failed to walk the graph of {collection}", cause=e)

    async def call_chains_batch(self, collection: str, pairs, relation: str = "calls", max_hops: int = 8, limit: int = 10, must_pass: bool = True,
                                match: str = "exact") -> list[dict[str, Any]]:
        """:meth:`call_chains` for a list of ``(source or names, target)`` pairs: 64 pairs per pass over the graph."""
        try:
            pairs = list(pairs)
            return await self._run(lambda: self._col(collection).call_chains(pairs, relation, max_hops, limit, must_pass, match))
        except Exception as e:
            raise VectorStoreError(f"Failed to walk the graph of {collection}", cause=e)

    async def call_chains(self, collection: str, source, target: str, relation: str = "calls", max_hops: int = 8, limit: int = 10,
                          must_pass: bool = True, match: str = "exact") -> dict[str, Any]:
        """How ``source`` reaches ``target`` over ``relation``, in full (:meth:`call_chain` returns one chain):
        ``{"count", "saturated", "length", "chains", "must_pass", "unresolved"}``.  ``count`` is the number of SHORTEST chains
        of at most ``max_hops`` (1..16) edges, exact up to 2^64 - 1 (``saturated``: at least that many); ``length`` their number
        of edges, None when there is no chain; ``chains`` the first ``limit`` (0..64) of them as lists of names from a source
        to the target, ordered by the nodes read BACKWARDS from the target in the order :meth:`set_graph_edges` saw them --
        ``chains[0]`` is :meth:`call_chain`'s; longer chains than the shortest are not listed (the reference's FIND_ALL_PATHS
        lists every path up to its bound).  ``must_pass`` (``must_pass=False`` skips it): the nodes other than the ends that
        EVERY way of at most ``max_hops`` edges passes, in chain order -- the bound is part of the statement: a detour longer
        than ``max_hops`` does not count.  ``source``: a name or several (together the source set); ``target`` must name
        exactly one node (``match="suffix"`` may find several: a ValueError lists them).  ``unresolved``: the names that are
        no node."""
        return (await self.call_chains_batch(collection, [(source, target)], relation, max_hops, limit, must_pass, match))[0]

    # ------------------------------------------------------------------ the graph as a whole
    async def graph_cycles(self, collection: str, relation: str = "calls", limit: int = 10, members: int = 50) -> dict[str, Any]:
        """Which functions are (mutually) recursive, which modules import each other in a circle: the CYCLIC strongly connected
        components of ``relation`` -- two nodes or more that all reach each other, or one node with an edge to itself -- found on
        the device (trim, colouring, back-mark; the ``limit`` largest chosen by ``crh_facet_select``).  Returns ``{"components":
        [{"id", "size", "nodes", "self_recursive"}], "count", "nodes", "self_recursive"}``: the components largest first, ties
        to the one whose first node :meth:`set_graph_edges` saw first; ``id`` is that first node's name, ``nodes`` the members in
        order of first appearance (at most ``members``), ``self_recursive`` those of them that also call themselves; ``count``
        and ``nodes`` are the number of cyclic components and of nodes in them, never clipped; the outer ``self_recursive``
        names the nodes that are cyclic ONLY by their own self-loop (their number when there are more than ``members``)."""
        try:
            return await self._run(lambda: self._col(collection).graph_cycles(relation, limit, members))
        except Exception as e:
            raise VectorStoreError(f"Failed to list the cycles of {collection}", cause=e)

    async def graph_layers(self, collection: str, relation: str = "calls", names=None, match: str = "exact") -> dict[str, Any]:
        """Entry points, leaf utilities and a reading or build order: the longest-path layers of the CONDENSATION of ``relation``
        (every cycle shrunk to one node), both ways.  ``depth`` is 0 for a node nobody outside its own cycle calls, ``height`` 0
        for one that calls nothing outside its own cycle.  Returns ``{"layers": n, "histogram": {"depth": [nodes per layer],
        "height": [...]}, "nodes": [{"name", "depth", "height", "component", "cyclic"}]}`` -- ``nodes`` for the named ones
        (``names``: a name or a list, resolved as in :meth:`graph_neighbors`; ``"unresolved"`` lists the rest)."""
        try:
            return await self._run(lambda: self._col(collection).graph_layers(relation, names, match))
        except Exception as e:
            raise VectorStoreError(f"Failed to layer the graph of {collection}", cause=e)

    async def search_expanded_batch(self, collection: str, query_vectors, limit: int = 10, graph_expand: dict[str, Any] | None = None,
                                    filters: dict[str, Any] | None = None, must_not: dict[str, Any] | None = None) -> list[dict[str, Any]]:
        """:meth:`search_batch` plus, per query, the graph neighbourhood of its hits: ``[{"hits": [...], "related": [{"name",
        "depth"}], "related_count": n}]``.  ``graph_expand`` = ``{"direction": "both", "hops": 1, "limit": 10, "relation":
        "calls"}`` (any key may be left out): ``related`` holds the nodes reached within ``hops`` edges from the nodes of the
        query's hits (a hit's node is its ``graph_node_id or entity_name``), the hits' own nodes left out, in (depth, order of
        first appearance) order, the first ``limit`` of them; ``related_count`` is how many there are.  The hit rows become BFS
        sources on the device, 64 queries per BFS: nothing returns to the host between the search and the list."""
        try:
            ex = dict(graph_expand or {})
            unknown = [k for k in ex if k not in ("direction", "hops", "limit", "relation")]
            direction, hops, rlimit, relation = ex.get("direction", "both"), ex.get("hops", 1), ex.get("limit", 10), ex.get("relation", "calls")
            if unknown or direction not in graph_mod.DIRECTIONS or not isinstance(relation, str):
                raise ValueError(f"graph_expand takes direction (one of {', '.join(graph_mod.DIRECTIONS)}), hops, limit and relation, not {graph_expand!r}")
            for what, v, lo, hi in (("hops", hops, 1, ffi.GRAPH_MAX_HOPS), ("limit", rlimit, 0, 2 ** 20)):
                if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
                    raise ValueError(f"graph_expand: {what} must be an int in {lo}..{hi}, not {v!r}")
            if has_graph_condition(filters, must_not) and (isinstance(filters, (list, tuple)) or isinstance(must_not, (list, tuple))):
                raise ValueError(f"a per-query filter list cannot carry a {GRAPH_KEY!r} condition -- pass ONE filter dict")
            if isinstance(filters, (list, tuple)) or isinstance(must_not, (list, tuple)):
                raise ValueError("search_expanded takes ONE filter dict for the whole batch")
            q = np.ascontiguousarray(np.asarray(query_vectors, dtype=np.float32))
            if q.size == 0:
                return []
            q = q.reshape(-1, q.shape[-1]) if q.ndim != 2 else q
            if limit > ffi.MAX_K:
                raise ValueError(f"limit {limit} exceeds the index's maximum k of {ffi.MAX_K}")

            def work():
                col = self._col(collection)
                if q.shape[1] != col.shards.dim:
                    raise ValueError(f"query dim {q.shape[1]} != index dim {col.shards.dim}")
                col._graph_ready(relation)
                dfilt = col.device_filters(filters, must_not)
                if dfilt is None or limit <= 0 or not len(q):
                    return [{"hits": [], "related": [], "related_count": 0} for _ in range(len(q))]
                self.search_passes += 1
                scores, slots, nodes, depth, count = col.search_expanded(q, int(limit), dfilt, direction, int(hops), int(rlimit), relation)
                return [{"hits": h, "related": col._graph_names_of(nodes[i], depth[i]), "related_count": int(count[i])}
                        for i, h in enumerate(self._hit_lists(col, slots, scores))]
            return await self._run(work)
        except Exception as e:
            raise VectorStoreError(f"Failed to search {collection}", cause=e)

    async def search_expanded(self, collection: str, query_vector, limit: int = 10, graph_expand: dict[str, Any] | None = None,
                              filters: dict[str, Any] | None = None, must_not: dict[str, Any] | None = None) -> dict[str, Any]:
        """:meth:`search_expanded_batch` for one query: ``{"hits", "related", "related_count"}``."""
        return (await self.search_expanded_batch(collection, [query_vector], limit, graph_expand, filters, must_not))[0]

    # ------------------------------------------------------------------ graph-propagated relevance
    PROPAGATE_DEFAULTS = {"relation": "calls", "direction": "both", "restart": 0.15, "steps": 16, "seed_weight": "cosine", "rrf_k": 60}

    @classmethod
    def _propagate_args(cls, propagate, what: str = "propagate") -> dict[str, Any]:
        """The checked settings of one personalised PageRank: the defaults with the caller's keys over them; ``ValueError`` for
        the caller alone, before anything runs."""
        given = {} if propagate is None or propagate is True else propagate
        if not isinstance(given, dict) or any(k not in cls.PROPAGATE_DEFAULTS for k in given):
            raise ValueError(f"{what} takes {', '.join(cls.PROPAGATE_DEFAULTS)}, not {propagate!r}")
        p = {**cls.PROPAGATE_DEFAULTS, **given}
        if not isinstance(p["relation"], str) or not p["relation"]:
            raise ValueError(f"{what}: relation must be a non-empty string, not {p['relation']!r}")
        if p["direction"] not in graph_mod.DIRECTIONS:
            raise ValueError(f"{what}: direction must be one of {', '.join(graph_mod.DIRECTIONS)}, not {p['direction']!r}")
        if p["seed_weight"] not in ("cosine", "uniform"):
            raise ValueError(f"{what}: seed_weight must be 'cosine' or 'uniform', not {p['seed_weight']!r}")
        for key, lo, hi in (("steps", 1, ffi.GRAPH_PPR_MAX_STEPS), ("rrf_k", 0, 2 ** 31 - 1)):
            if isinstance(p[key], bool) or not isinstance(p[key], (int, np.integer)) or not lo <= int(p[key]) <= hi:
                raise ValueError(f"{what}: {key} must be an int in {lo}..{hi}, not {p[key]!r}")
            p[key] = int(p[key])
        r = p["restart"]
        if isinstance(r, bool) or not isinstance(r, (int, float, np.floating)) or not 0.0 < float(np.float32(r)) < 1.0:
            raise ValueError(f"{what}: restart must be a number inside (0, 1), not {r!r}")
        p["restart"] = float(r)
        return p

    async def search_propagated_batch(self, collection: str, query_vectors, limit: int = 10, candidates: int | None = None,
                                      propagate: dict[str, Any] | None = None, related_limit: int = 10,
                                      filters: dict[str, Any] | None = None, must_not: dict[str, Any] | None = None, **others) -> list[dict[str, Any]]:
        """Vector search re-ranked and extended by graph-propagated relevance: ``[{"hits": [...], "related": [...]}]``.  Per
        query the exact top-``candidates`` (default ``4 * limit``, at most 512) seed a personalised PageRank over the
        collection's graph -- a random walk with restart from the candidates' nodes, weighted ``max(cosine, 0)`` -- and

        * ``hits`` are the first ``limit`` candidates under reciprocal-rank fusion of the cosine order and the graph-score
          order (a candidate without a node, or with graph score 0, stands in the cosine list only); each carries ``score``
          (fused), ``cosine`` and ``graph_score``;
        * ``related`` are the ``related_limit`` nodes with the highest graph score that are NO candidate's node -- what the
          query is about beyond what the embedding found -- as ``{"node", "graph_score", "payload"}``, ``payload`` being that of
          the node's representative chunk (its first alive one) or None.

        ``propagate`` = ``{"relation": "calls", "direction": "both", "restart": 0.15, "steps": 16, "seed_weight": "cosine" |
        "uniform", "rrf_k": 60}`` (any key may be left out).  64 queries per pass; nothing returns to the host between the
        search and the finished tables.  The definition is exact and deterministic."""
        try:
            used = [name for name in ("diversity", "group_by", "max_overlap", "score_threshold") if others.get(name) is not None]
            unknown = [name for name in others if name not in ("diversity", "group_by", "max_overlap", "score_threshold")]
            if unknown:
                raise TypeError(f"search_propagated got unexpected arguments: {', '.join(unknown)}")
            if isinstance(filters, (list, tuple)) or isinstance(must_not, (list, tuple)):
                used.append("per-query filter lists")
            if used:
                raise ValueError(f"search_propagated cannot be combined with {', '.join(used)} (it takes ONE filter dict, and fuses two "
                                 "orders of one candidate list)")
            if self._shard_backend == "dist":
                raise ValueError("search_propagated is not available with shard_backend='dist' yet")
            prop = self._propagate_args(propagate)
            for what, v, lo, hi in (("limit", limit, 0, ffi.MAX_K // 2), ("related_limit", related_limit, 0, ffi.MAX_K)):
                if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
                    raise ValueError(f"search_propagated: {what} must be an int in {lo}..{hi}, not {v!r}")
            limit, related_limit = int(limit), int(related_limit)
            if candidates is None:
                candidates = min(ffi.MAX_K // 2, 4 * max(limit, 1))
            if isinstance(candidates, bool) or not isinstance(candidates, (int, np.integer)) or not max(limit, 1) <= int(candidates) <= ffi.MAX_K // 2:
                raise ValueError(f"search_propagated: candidates must be an int in {max(limit, 1)}..{ffi.MAX_K // 2} (>= limit), not {candidates!r}")
            candidates = int(candidates)
            q = np.ascontiguousarray(np.asarray(query_vectors, dtype=np.float32))
            if q.size == 0:
                return []
            q = q.reshape(-1, q.shape[-1]) if q.ndim != 2 else q

            def work():
                col = self._col(collection)
                if q.shape[1] != col.shards.dim:
                    raise ValueError(f"query dim {q.shape[1]} != index dim {col.shards.dim}")
                col._graph_ready(prop["relation"])
                dfilt = col.device_filters(filters, must_not)
                if dfilt is None or limit <= 0:
                    return [{"hits": [], "related": []} for _ in range(len(q))]
                self.search_passes += (len(q) + 63) // 64
                slots, fused, cos, gsc, top, top_scores, top_slots = col.search_propagated(q, limit, candidates, dfilt, prop, related_limit)

                def decorate(hits, keep):
                    for h, cv, gv in zip(hits, cos[keep].tolist(), gsc[keep].tolist()):
                        h["cosine"], h["graph_score"] = cv, gv
                return [{"hits": h, "related": self._node_list(col, top[i], top_scores[i], top_slots[i])}
                        for i, h in enumerate(self._hit_lists(col, slots, fused, decorate=decorate))]
            return await self._run(work)
        except Exception as e:
            raise VectorStoreError(f"Failed to search {collection}", cause=e)

    @staticmethod
    def _node_list(col: _Collection, nodes, scores, slots) -> list[dict[str, Any]]:
        """``[{"node", "graph_score", "payload"}]`` of one query's ranked nodes (-1: padding); a node without an alive chunk has
        payload None.  Runs inside the worker job, like :meth:`_hit_lists`."""
        keep = np.asarray(nodes) >= 0
        have = [int(t) for t in np.asarray(slots)[keep] if t >= 0]
        pays = iter(col.payloads_of(have)) if have else iter(())
        return [{"node": col._graph_names[int(v)], "graph_score": float(g), "payload": next(pays) if t >= 0 else None}
                for v, g, t in zip(np.asarray(nodes)[keep], np.asarray(scores)[keep], np.asarray(slots)[keep])]

    async def search_propagated(self, collection: str, query_vector, limit: int = 10, candidates: int | None = None,
                                propagate: dict[str, Any] | None = None, related_limit: int = 10,
                                filters: dict[str, Any] | None = None, must_not: dict[str, Any] | None = None, **others) -> dict[str, Any]:
        """:meth:`search_propagated_batch` for one query: ``{"hits", "related"}``."""
        return (await self.search_propagated_batch(collection, [query_vector], limit, candidates, propagate, related_limit, filters, must_not,
                                                   **others))[0]

    async def graph_rank_batch(self, collection: str, name_sets, weights=None, direction: str = "both", relation: str = "calls",
                               restart: float = 0.15, steps: int = 16, limit: int = 10, match: str = "exact",
                               include_seeds: bool = True) -> list[dict[str, Any]]:
        """:meth:`graph_rank` for a list of name sets (each a name or a list of names; ``weights``: None, or per set None or one
        number per name): one personalised PageRank per 64 sets."""
        try:
            sets = [[s] if isinstance(s, str) else list(s) for s in name_sets]
            wsets = [None] * len(sets) if weights is None else list(weights)
            if len(wsets) != len(sets):
                raise ValueError(f"{len(wsets)} weight lists for {len(sets)} name sets")
            checked = []
            for names, ws in zip(sets, wsets):
                if ws is not None:
                    ws = [ws] if isinstance(ws, (int, float)) else list(ws)
                    if len(ws) != len(names) or any(isinstance(w, bool) or not isinstance(w, (int, float, np.floating, np.integer))
                                                     or not np.isfinite(np.float32(w)) or w < 0 for w in ws):
                        raise ValueError(f"weights must be one finite number >= 0 per name, not {ws!r} for {names!r}")
                checked.append(ws)
            prop = self._propagate_args({"relation": relation, "direction": direction, "restart": restart, "steps": steps}, "graph_rank")
            if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)) or not 1 <= int(limit) <= ffi.MAX_K:
                raise ValueError(f"graph_rank: limit must be an int in 1..{ffi.MAX_K}, not {limit!r}")
            if self._shard_backend == "dist":
                raise ValueError("graph_rank is not available with shard_backend='dist' yet")

            def work():
                col = self._col(collection)
                ranked = col.graph_rank(sets, checked, prop["relation"], prop["direction"], prop["restart"], prop["steps"], int(limit), match,
                                        bool(include_seeds))
                return [{"hits": self._node_list(col, nodes, scores, slots), "unresolved": missing} for nodes, scores, slots, missing in ranked]
            return await self._run(work)
        except Exception as e:
            raise VectorStoreError(f"Failed to rank the graph of {collection}", cause=e)

    async def graph_rank(self, collection: str, names, weights=None, direction: str = "both", relation: str = "calls",
                         restart: float = 0.15, steps: int = 16, limit: int = 10, match: str = "exact",
                         include_seeds: bool = True) -> dict[str, Any]:
        """What matters around the named nodes: personalised PageRank over ``relation`` seeded by them (``weights``: one number
        >= 0 per name, default 1; ``match="suffix"``: a name also stands for every node whose name ends in ``"." + name``, each
        with the name's weight), ``steps`` (1..64) steps with restart probability ``restart``.  ``direction``: the way the walk
        travels -- ``"callees"`` follows the calls, ``"callers"`` goes against them, ``"both"`` either way.  Returns ``{"hits":
        [{"node", "graph_score", "payload"}], "unresolved"}``: the ``limit`` nodes with the highest score (> 0), ties to the
        node :meth:`set_graph_edges` saw first; ``include_seeds=False`` leaves the named nodes out; ``payload`` is that of the
        node's first alive chunk, or None.  Exact and deterministic."""
        return (await self.graph_rank_batch(collection, [names], None if weights is None else [weights], direction, relation, restart, steps,
                                            limit, match, include_seeds))[0]

    async def search_rerank_batch(self, collection: str, query_vectors, plans, reranker, limit: int = 20,
                                  filters: dict[str, Any] | None = None, must_not: dict[str, Any] | None = None):
        """One corpus scan for all queries, then the hybrid re-rank of every candidate list on the device
        (``ranking.device.DeviceReranker``): returns ``(hits, output, slots, scores)`` -- the :class:`RerankOutput`, the host
        copies of the [nq, limit] candidate slots / scores it indexes, and ``hits``: a :class:`RerankHits` whose
        ``hit(slot, score)`` answers for every slot the output refers to (the survivors of each query; the whole list of a query
        the device declined).  Their ids and payloads are read inside this job, under the store's lock: a compaction that runs
        after it renumbers the slots (see ``_search_hits_sync``).  Payloads are still read only for the survivors."""
        import torch
        try:
            def work():
                col = self._col(collection)
                dfilt = col.device_filters(filters, must_not)
                q = np.ascontiguousarray(np.asarray(query_vectors, dtype=np.float32))
                nq = q.shape[0]
                dev = torch.device("cuda", self._device)
                if dfilt is not None and limit > 0 and nq > 0:
                    s, r = col.shards.search_device(torch.from_numpy(q).to(dev), limit, dfilt)       # r: GLOBAL rows
                else:
                    s = torch.full((nq, limit), float("-inf"), dtype=torch.float32, device=dev)
                    r = torch.full((nq, limit), -1, dtype=torch.int64, device=dev)
                out = reranker.rank(s, r, col.gather_side(r), plans)
                slots = col._global_slots(r.cpu().numpy())
                wanted = set()
                for qi in range(nq):
                    c = int(out.count[qi])
                    pos = out.index[qi, :c] if c >= 0 else np.flatnonzero(slots[qi] >= 0)
                    wanted.update(int(t) for t in slots[qi, pos] if t >= 0)
                wanted = sorted(wanted)
                return RerankHits({t: (col.ids.get(t), p) for t, p in zip(wanted, col.payloads_of(wanted))}, col._degrees), out, slots, s.cpu().numpy()
            return await self._run(work)
        except Exception as e:
            raise VectorStoreError(f"Failed to search {collection}", cause=e)

    async def search_rerank_hybrid_batch(self, collection: str, query_vectors, plans, reranker, limit: int = 20,
                                         filters: dict[str, Any] | None = None, must_not: dict[str, Any] | None = None, relation: str = "calls"):
        """:meth:`search_rerank_batch` with the GRAPH branch of the ranker on the device as well (DESIGN.md 3.28;
        ``ranking.device.HybridDeviceReranker``): per 64 queries the search, one BFS per direction from the plans' primary
        entities (``engine_helpers.plan_graph_roles``), ``crh_graph_list``, the kept representative rows, ``crh_graph_candidates``,
        the gathers and ``crh_rerank_hybrid`` -- nothing travels to the host before the finished tables.  Returns ``(hits, parts,
        names)``: ``parts`` holds per batch of 64 ``(HybridRerankOutput, hit slots [nq, k], scores, graph slots [nq, G], graph nodes
        [nq, G], declined)``, ``hits`` a :class:`RerankHits` answering for every slot a survivor, something it absorbed or a
        declined query refers to, ``names`` the node id -> ``(name, slot of its representative row)`` table of those nodes.  ``declined[q]`` lists a declined
        query's graph results ``[(role, node, depth)]`` for the host ranker.  One and several local shards; not available with
        ``shard_backend="dist"``."""
        try:
            q = np.ascontiguousarray(np.asarray(query_vectors, dtype=np.float32))
            q = q.reshape(-1, q.shape[-1]) if q.ndim != 2 else q
            if len(plans) != len(q):
                raise ValueError(f"{len(plans)} plans for {len(q)} query vectors")
            if limit > ffi.RR_MAX_HYBRID:
                raise ValueError(f"limit {limit} exceeds the {ffi.RR_MAX_HYBRID} candidates one hybrid re-rank takes")
            if isinstance(filters, (list, tuple)) or isinstance(must_not, (list, tuple)):
                raise ValueError("search_rerank_hybrid_batch takes ONE filter dict for the whole batch")

            def work():
                col = self._col(collection)
                if len(q) and q.shape[1] != col.shards.dim:
                    raise ValueError(f"query dim {q.shape[1]} != index dim {col.shards.dim}")
                col._graph_ready(relation)
                dfilt = col.device_filters(filters, must_not)
                self.search_passes += 1
                parts = col.search_rerank_hybrid(q, list(plans), reranker, int(limit), dfilt, relation)
                wanted, nodes = set(), set()
                for res, slots, _, g_slots, g_nodes, declined in parts:
                    both = np.concatenate([g_slots, slots], axis=1)
                    for qi in range(len(res.count)):
                        c = int(res.count[qi])
                        if c < 0:
                            pos = np.flatnonzero(both[qi] >= 0)
                            nodes.update(v for _, v, _ in declined[qi])
                        else:
                            pos = set(int(i) for i in res.index[qi, :c])
                            for i, merged in zip(res.index[qi, :c], res.hybrid[qi, :c]):
                                if merged:                                # what a survivor absorbed fills its missing fields
                                    pos.update(int(j) for j in np.flatnonzero(res.key[qi] == res.key[qi, i]))
                            pos = np.asarray(sorted(pos), np.int64)
                        wanted.update(int(t) for t in both[qi, pos] if t >= 0)
                        nodes.update(int(g_nodes[qi, i]) for i in pos if i < g_nodes.shape[1] and g_nodes[qi, i] >= 0)
                order = sorted(nodes)
                node_slots = col._global_slots(col.graph_node_rows()[1][order]) if order else []
                wanted.update(int(t) for t in node_slots if t >= 0)      # (a declined query's lists may hold nodes beyond the table)
                wanted = sorted(wanted)
                hits = RerankHits({t: (col.ids.get(t), p) for t, p in zip(wanted, col.payloads_of(wanted))}, col._degrees)
                return hits, parts, {v: (col._graph_names[v], int(t)) for v, t in zip(order, node_slots)}
            return await self._run(work)
        except VectorStoreError:
            raise
        except Exception as e:
            raise VectorStoreError(f"Failed to search {collection}", cause=e)

    async def delete(self, collection: str, filters: dict[str, Any], must_not: dict[str, Any] | None = None) -> None:
        """client.py:159-169: delete every point matching the AND of the conditions (values and ``must_not`` as in :meth:`search`)."""
        try:
            await self._run(lambda: self._col(collection).delete(filters, must_not))
            logger.debug(f"Deleted vectors from {collection} with filters: {filters}")
        except Exception as e:
            raise VectorStoreError(f"Failed to delete from {collection}", cause=e)

    async def file_needs_update(self, collection: str, file_path: str, content_hash: str) -> bool:
        """client.py:178-202: True on a miss, on a different stored hash, and on ANY error."""
        try:
            def work():
                col = self._col(collection)
                slots = col.matching_slots({"file_path": file_path}, limit=1)
                if not len(slots):
                    return True
                return col.payloads.value(int(slots[0]), "content_hash") != content_hash
            return bool(await self._run(work))
        except Exception as e:
            logger.warning(f"Error checking file update status: {e}")
            return True

    async def files_need_update(self, collection: str, files: list[tuple[str, str]]) -> list[bool]:
        """:meth:`file_needs_update` for many ``(file_path, content_hash)`` pairs in ONE job (a batched indexer asks once for a
        whole project instead of once per file); True on a miss, on a different stored hash, and for every file on ANY error."""
        try:
            def work():
                col = self._col(collection)
                out = []
                for file_path, content_hash in files:
                    slots = col.matching_slots({"file_path": file_path}, limit=1)
                    out.append(True if not len(slots) else col.payloads.value(int(slots[0]), "content_hash") != content_hash)
                return out
            return [bool(v) for v in await self._run(work)]
        except Exception as e:
            logger.warning(f"Error checking file update status: {e}")
            return [True] * len(files)

    async def delete_files(self, collection: str, file_paths: list[str]) -> None:
        """``delete(collection, {"file_path": p})`` for many files in ONE job and ONE device call per shard: the paths the
        collection has stored become one set condition (a path it has never stored costs a dictionary look-up); the collection
        compacts at most once, at the end."""
        try:
            def work():
                col = self._col(collection)
                dfilt = col.device_filters({"file_path": list(file_paths)})
                if dfilt:
                    col.shards.tombstone_filter(dfilt)
                col.maybe_compact()
            await self._run(work)
        except Exception as e:
            raise VectorStoreError(f"Failed to delete from {collection}", cause=e)

    async def compact(self, collection: str | None = None) -> int:
        """Reclaim the rows of deleted points (``crh_index_compact`` + the host tables): what Qdrant's optimizer does in the
        background.  The store also does it by itself once dead rows exceed ``compact_dead_fraction`` of a collection
        (``CODERAG_HIP_COMPACT_DEAD_FRACTION``, 0 = never).  Returns the number of rows reclaimed."""
        try:
            names = [collection.value if isinstance(collection, CollectionName) else collection] if collection else list(self._collections)
            return int(await self._run(lambda: sum(self._col(n).compact() for n in names)))
        except Exception as e:
            raise VectorStoreError("Failed to compact", cause=e)

    # ------------------------------------------------------------------ persistence
    async def save(self, directory: str) -> None:
        """Write every collection to ``directory/<name>/``: the index image verbatim (raw ``tiles.bin`` the scan's layout,
        mmap-able; ``alive.u32``; columnar ``codes.i32``; ``master.f32`` for the f32 store; one sub-directory per shard) + the id
        and payload tables as raw arrays + ``collection.json``.  No pickle, no per-row JSON.  Stands in for the Qdrant volume the reference relies on
        for restarts (docker-compose.yml:42-43): an indexed project can be reloaded without re-embedding."""
        try:
            def work():
                os.makedirs(directory, exist_ok=True)
                for name, col in self._collections.items():
                    col.save(os.path.join(directory, name))
            await self._run(work)
        except Exception as e:
            raise VectorStoreError(f"Failed to save collections to {directory}", cause=e)

    async def load(self, directory: str) -> None:
        """Replace the collections' contents with a snapshot written by :meth:`save`.  The stored image goes back verbatim
        (``crh_index_import``): searches return bit-identical scores and the same ids as before, deleted rows stay deleted."""
        try:
            await self.clear_collections()

            def work():
                for name, col in self._collections.items():
                    sub = os.path.join(directory, name)
                    if os.path.isdir(sub):
                        col.load(sub)
            await self._run(work)
        except Exception as e:
            raise VectorStoreError(f"Failed to load collections from {directory}", cause=e)

    async def __aenter__(self):
        await self.connect()
        return self

    async def __aexit__(self, exc_type, exc_val, exc_tb):
        await self.close()


# the name the reference's call sites import
QdrantManager = HipVectorStore
