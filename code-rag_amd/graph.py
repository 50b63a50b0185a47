"""Host side of the device call graph: numbering the nodes of an edge list, the two CSRs ``crh_graph_set_relation``
takes, degrees, and the resolution of names to nodes.  numpy only; nothing here touches the device."""

from __future__ import annotations

from typing import Iterable

import numpy as np

MAX_RELATIONS = 8          # CRH_GRAPH_MAX_RELATIONS: named relations one collection holds
DIRECTIONS = ("callers", "callees", "both")
FILTER_WORDS = {"callers_of": "callers", "callees_of": "callees", "connected_to": "both"}    # the filter's key -> the direction of travel
STRUCTURE_WORDS = ("in_cycle", "same_cycle_as", "depth", "height")    # filter keys on the graph as a whole
BETWEEN_WORD = "between"   # the filter key of the nodes on a way from one node set to another


def number_edges(edges: Iterable, code: dict, names: list) -> np.ndarray:
    """``edges`` (an iterable of ``(source_name, target_name)``) as int32 [m, 2] node ids.  A name the dictionary ``code`` does
    not know yet gets the next id, in order of first appearance (the source of an edge before its target), and is appended to
    ``names``; ids never change afterwards."""
    out = []
    for e in edges:
        if not isinstance(e, (tuple, list)) or len(e) != 2 or not all(isinstance(v, str) for v in e):
            raise ValueError(f"a graph edge is a (source_name, target_name) pair of strings, not {e!r}")
        for v in e:
            if v not in code:
                code[v] = len(names)
                names.append(v)
        out.append((code[e[0]], code[e[1]]))
    return np.asarray(out, np.int32).reshape(-1, 2)


def unique_edges(pairs: np.ndarray, n_nodes: int) -> np.ndarray:
    """The edges without self-loops and repeats, int32 [m, 2] ordered by (source, target)."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    if pairs.size and (pairs.min() < 0 or pairs.max() >= n_nodes):
        raise ValueError(f"an edge names a node outside 0..{n_nodes - 1}")
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    keys = np.unique(pairs[:, 0] * max(n_nodes, 1) + pairs[:, 1])
    return np.stack([keys // max(n_nodes, 1), keys % max(n_nodes, 1)], axis=1).astype(np.int32)


def self_loops(pairs: np.ndarray, n_nodes: int) -> np.ndarray:
    """The nodes that carry a self-loop, int32, ascending without repeats: what :func:`unique_edges` drops and a listing of the
    recursive functions needs (a function that calls itself is a cycle of one node)."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    if pairs.size and (pairs.min() < 0 or pairs.max() >= n_nodes):
        raise ValueError(f"an edge names a node outside 0..{n_nodes - 1}")
    return np.unique(pairs[pairs[:, 0] == pairs[:, 1], 0]).astype(np.int32)


def build_csr(pairs: np.ndarray, n_nodes: int) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """``(off_fwd, adj_fwd, off_rev, adj_rev)`` of an edge list: offsets int64 [n_nodes + 1], adjacency int32; the forward CSR
    lists a node's targets, the reverse one its sources; self-loops and repeats dropped, every list ascending."""
    e = unique_edges(pairs, n_nodes)
    out = []
    for a, b in ((0, 1), (1, 0)):
        order = np.lexsort((e[:, b], e[:, a]))
        off = np.zeros(n_nodes + 1, np.int64)
        np.cumsum(np.bincount(e[:, a], minlength=n_nodes), out=off[1:])
        out += [off, np.ascontiguousarray(e[order, b], dtype=np.int32)]
    return tuple(out)


def total_degrees(pairs: np.ndarray, n_nodes: int) -> np.ndarray:
    """Distinct in-degree + distinct out-degree per node (what the reference's GET_ENTITY_CENTRALITY returns as total_degree),
    int64 [n_nodes]; self-loops and repeated edges do not count."""
    e = unique_edges(pairs, n_nodes)
    return np.bincount(e[:, 0], minlength=n_nodes) + np.bincount(e[:, 1], minlength=n_nodes)


def resolve(wanted, code: dict, names: list, match: str = "exact") -> tuple[list[int], list[str]]:
    """Names -> node ids, ascending without repeats, and the names that resolved to nothing.  ``match="exact"``: the node of
    that very name; ``"suffix"``: also every node whose name ends in ``"." + name`` (``parse`` finds ``pkg.mod.parse``)."""
    if match not in ("exact", "suffix"):
        raise ValueError(f"match {match!r} is neither 'exact' nor 'suffix'")
    wanted = [wanted] if isinstance(wanted, str) else list(wanted)
    ids, missing = set(), []
    for name in wanted:
        if not isinstance(name, str):
            raise ValueError(f"a graph node is named by a string, not {name!r}")
        got = [code[name]] if name in code else []
        if match == "suffix":
            tail = "." + name
            got += [i for i, full in enumerate(names) if full.endswith(tail)]
        if not got:
            missing.append(name)
        ids.update(got)
    return sorted(ids), missing
