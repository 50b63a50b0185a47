"""Facets: the CPU restatement, the code generators, and the fake index / fake text arena of the CPU tier.
Test infrastructure only.

The restatement is the definition read aloud: ``numpy.bincount`` over the codes of the rows the mask (and, in the semantic form,
``oracle.search.scores >= thr`` as f32, inclusive) lets through; the list is ``lexsort((code, -count))`` over the non-zero bins,
cut at ``k``."""
import numpy as np

from oracle import search as orc
from tests import span_cases
from tests.range_cases import RangeFakeIndex

_LOWER = bytes(c + 32 if 65 <= c <= 90 else c for c in range(256))     # ASCII letters only, as the device folds them


def histogram(codes, passing, n_bins: int):
    """``codes`` int [n] (one column), ``passing`` bool [n]: ``(bins i64 [n_bins], info i64 [3] = counted, missing, out_of_range)``."""
    c = np.asarray(codes, np.int64)[np.asarray(passing, bool)]
    inside = c[(c >= 0) & (c < n_bins)]
    bins = np.bincount(inside, minlength=n_bins).astype(np.int64)
    return bins, np.asarray([c.size, int((c < 0).sum()), int((c >= n_bins).sum())], np.int64)


def histograms(codes, all_scores, thr, passing, n_bins: int):
    """The semantic form: per query the histogram of the passing rows whose score is ``>= thr[q]``: ``(bins [nq, n_bins], info [nq, 3])``."""
    all_scores = np.asarray(all_scores, np.float32)
    thr = np.broadcast_to(np.asarray(thr, np.float32), (all_scores.shape[0],))
    ok = np.ones((all_scores.shape[1],), bool) if passing is None else np.asarray(passing, bool)
    got = [histogram(codes, ok & (all_scores[q] >= thr[q]), n_bins) for q in range(all_scores.shape[0])]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def facet_list(bins, k: int):
    """``bins`` i64 [nq, n_bins] (or [n_bins]): ``(codes i32 [nq, k], counts i64 [nq, k], info i64 [nq, 2] = values, total)`` --
    the non-zero bins by count descending, ties to the lower code, tail (-1, 0)."""
    bins = np.asarray(bins, np.int64)
    bins = bins[None, :] if bins.ndim == 1 else bins
    nq = bins.shape[0]
    codes, counts = np.full((nq, k), -1, np.int32), np.zeros((nq, k), np.int64)
    info = np.zeros((nq, 2), np.int64)
    for q in range(nq):
        nz = np.flatnonzero(bins[q] > 0)
        order = nz[np.lexsort((nz, -bins[q, nz]))][:k]
        codes[q, :order.size], counts[q, :order.size] = order, bins[q, order]
        info[q] = (nz.size, int(bins[q].sum()))
    return codes, counts, info


def np_facet_select(bins, k: int, stream: int = 0):
    """``ffi.facet_select`` on host arrays."""
    return facet_list(bins, int(k))


# ---------------------------------------------------------------------------------------------------- code generators
def _runs(n, rng):
    """Runs of equal codes, one boundary near every multiple of 32 rows: one row before it, on it and one row after it in turn,
    so the lane-63/64 edges (every second multiple), the 32-row tile edges and the 256-row workgroup edges (every eighth) each meet
    all three; run i carries code i % 97 (codes repeat far apart: no order is promised)."""
    cuts = [m + (-1, 0, 1)[i % 3] for i, m in enumerate(range(32, n, 32))] + [n]
    out, first = np.empty((n,), np.int32), 0
    for i, c in enumerate(cuts):
        out[first:c] = i % 97
        first = c
    return out


GENERATORS = {
    "one": lambda n, rng: np.full((n,), 3, np.int32),                                  # every row the same code
    "distinct": lambda n, rng: np.arange(n, dtype=np.int32),                           # no two rows share one
    "alternating": lambda n, rng: (np.arange(n) % 2 * 5 + 1).astype(np.int32),         # no two neighbours share one
    "runs": _runs,
    "random10": lambda n, rng: rng.integers(0, 10, n).astype(np.int32),
    "files": lambda n, rng: np.sort(rng.integers(0, max(n // 6, 1), n)).astype(np.int32),   # chunks of a file next to each other
}


def codes_for(name: str, n: int, seed: int = 0, sprinkle: bool = True):
    """The column of generator ``name`` with -1 sprinkled in (every 13th row from row 4, and a whole tile's worth at the end of a
    corpus long enough to have one): int32 [n]."""
    rng = np.random.default_rng(100 + seed + n)
    c = GENERATORS[name](n, rng).astype(np.int32)
    if sprinkle:
        c[4::13] = -1
        if n >= 96:
            c[n - 40:n - 8] = -1
    return c


# ---------------------------------------------------------------------------------------------------- the CPU tier's fakes
def _row_words(item, owner):
    """The bool rows of a ``ffi.RowWords`` made by :class:`FakeText` for ``owner``."""
    w = item.words.get(id(owner)) if isinstance(item.words, dict) else item.words
    bits = np.unpackbits(np.asarray(w, np.int32).view(np.uint8), bitorder="little").astype(bool)[: len(owner.alive)]
    return ~bits if item.negate else bits


class FacetFakeIndex(RangeFakeIndex):
    """``FakeIndex`` with set, range and row-bitmap conditions, ``search_range``, ``row_mask`` and the two facet calls as numpy
    restatements over the rows it holds."""
    facet_calls: list = []

    def _mask(self, filters=None):
        from coderag_amd import ffi
        plain = [c for c in (filters or []) if not isinstance(c, ffi.RowWords)]
        ok = span_cases.np_mask(self.codes, self.alive, plain) if len(self.alive) else np.zeros((0,), bool)
        for c in filters or []:
            if isinstance(c, ffi.RowWords):
                ok &= _row_words(c, self)
        return ok

    def row_mask(self, filters=None, out=None, stream=0):
        bits = np.zeros(((len(self.alive) + 31) // 32) * 32, np.uint8)
        bits[: len(self.alive)] = self._mask(filters)
        return np.packbits(bits, bitorder="little").view(np.int32).copy()

    def facet(self, col, n_bins, filters=None, out=None, stream=0):
        FacetFakeIndex.facet_calls.append(("facet", int(col), int(n_bins)))
        assert 0 <= col < self.n_code_cols and n_bins >= 1
        return histogram(self.codes[:, col], self._mask(filters), n_bins)

    def search_range_facet(self, queries, thresholds, col, n_bins, filters=None, out=None, stream=0):
        q = orc.preprocess(np.asarray(queries, np.float32).reshape(-1, self.dim), to_bf16=(self.dtype == 1))
        FacetFakeIndex.facet_calls.append(("range", int(col), int(n_bins), len(q)))
        assert 0 <= col < self.n_code_cols and n_bins >= 1
        if len(self.x) == 0:
            return np.zeros((len(q), n_bins), np.int64), np.zeros((len(q), 3), np.int64)
        return histograms(self.codes[:, col], orc.scores(self.x, q), thresholds, self._mask(filters), n_bins)


class FakeText:
    """``ffi.Text`` on the host: the rows' bytes, ``match`` by ``bytes.find`` and ``regex`` by the compiled table's own walk, under the
    mask words they are handed; results are int32 validity words like the device's."""

    def __init__(self, capacity_rows=0, capacity_bytes=0, device=0):
        self.rows: list[bytes] = []

    def close(self):
        self.rows = []

    def clear(self):
        self.rows = []

    def count(self):
        return len(self.rows), sum(len(r) for r in self.rows)

    def append(self, row_off, data):
        off = np.asarray(row_off, np.int64)
        self.rows += [bytes(data[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]

    def _under(self, mask, hit):
        n = len(self.rows)
        ok = np.ones((n,), bool) if mask is None else np.unpackbits(np.asarray(mask, np.int32).view(np.uint8), bitorder="little").astype(bool)[:n]
        ok = ok & np.asarray([bool(hit(r)) for r in self.rows], bool) if n else ok
        bits = np.zeros(((n + 31) // 32) * 32, np.uint8)
        bits[:n] = ok
        return np.packbits(bits, bitorder="little").view(np.int32).copy(), int(ok.sum())

    def match(self, patterns, fold_case=False, any_of=False, mask=None, out=None, count=True, stream=0):
        pats = [p.encode("utf-8") if isinstance(p, str) else bytes(p) for p in patterns]
        pats = [p.translate(_LOWER) for p in pats] if fold_case else pats
        how = any if any_of else all
        return self._under(mask, lambda r: how((r.translate(_LOWER) if fold_case else r).find(p) >= 0 for p in pats))

    def regex(self, dfa, mask=None, out=None, count=True, stream=0):
        return self._under(mask, dfa.search)                                       # (RegexDFA.search: the device's table walk on the host)


# ---------------------------------------------------------------------------------------------------- the store script
SCRIPT_DIM = 384
FACET_KEYS = ("file_path", "language", "entity_type", "project_name")
_LANGS = ("python", "go", "typescript", "rust")


def point(i: int, rev: int = 0):
    """Point ``i`` of the script (``rev`` > 0: its replacement): chunks of a file lie next to each other (8 per file), a few
    payloads carry no ``language`` and a few ``None``; every 7th text holds ``TODO(``, every 11th ``todo(``."""
    f = i // 8
    pay = {"file_path": f"/proj/{'new/' if rev else ''}f{f}.py", "entity_type": ("function", "class", "method")[i % 3], "entity_name": f"ent{i}",
           "language": "zig" if rev else _LANGS[f % 4 if f % 9 else 0], "start_line": i, "end_line": i + 3,
           "content": f"def ent{i}(): pass" + ("  # TODO(me): tidy\n" if i % 7 == 0 else "") + ("  # todo(you)\n" if i % 11 == 0 else ""),
           "graph_node_id": f"mod.ent{i}", "content_hash": "h", "project_name": "p1" if i < 250 else ("p2" if i < 450 else "p3")}
    if i % 29 == 3:
        del pay["language"]
    elif i % 31 == 5:
        pay["language"] = None
    return f"00000000-0000-4000-8000-{i:012d}", pay


def script_vectors(n: int = 600):
    rng = np.random.default_rng(23)
    vecs = rng.standard_normal((n, SCRIPT_DIM)).astype(np.float32)
    vecs[290:330] = vecs[290]                                                       # 40 identical rows: five files, inclusive at their own score
    q = (vecs[290] + 0.3 * rng.standard_normal(SCRIPT_DIM)).astype(np.float32)
    return vecs, q, rng.standard_normal(SCRIPT_DIM).astype(np.float32)


class FacetModel:
    """What the store must answer, from the points alone: never reads the store."""

    def __init__(self):
        self.rows: dict = {}                                                        # id -> (vector, payload), in upsert order
        self.first: dict = {k: {} for k in FACET_KEYS}                              # value -> when it was first stored (never forgotten)

    def upsert(self, ids, vecs, pays):
        for i, v, p in zip(ids, vecs, pays):
            self.rows.pop(i, None)
            self.rows[i] = (np.asarray(v, np.float32), p)
            for k in FACET_KEYS:
                if p.get(k) is not None:
                    self.first[k].setdefault(p[k], len(self.first[k]))

    def delete(self, pred):
        self.rows = {i: r for i, r in self.rows.items() if not pred(r[1])}

    def counting(self, pred=None, q=None, thr=None):
        rows = list(self.rows.values())
        ok = np.asarray([pred is None or bool(pred(p)) for _, p in rows], bool)
        if q is not None:
            s = orc.scores(orc.preprocess(np.stack([v for v, _ in rows])), orc.preprocess(np.asarray(q, np.float32)[None]))[0]
            ok &= s >= np.float32(thr)
        return [p for (_, p), keep in zip(rows, ok) if keep]

    def facet(self, key, limit, pred=None, q=None, thr=None):
        from collections import Counter
        pays = self.counting(pred, q, thr)
        c = Counter(p.get(key) for p in pays)
        order = sorted(c, key=lambda v: (-c[v], -1 if v is None else self.first[key][v]))
        return {"hits": [{"value": v, "count": c[v]} for v in order[:limit]], "values": len(c), "total": sum(c.values()), "missing": 0}, len(pays)


def _finds(text, pat, case=True):
    raw = text.encode() if isinstance(text, str) else b""
    return (raw if case else raw.translate(_LOWER)).find(pat.encode() if case else pat.encode().translate(_LOWER)) >= 0


async def store_script(make_store, model: FacetModel | None, tmp_dir: str | None = None) -> dict:
    """The facet life-cycle on one store: upserts, every kind of facet, delete, upsert-replace, ``compact()`` and -- with
    ``tmp_dir`` -- ``save()`` / ``load()``; the same facets after each step.  Returns {name: result}; with ``model`` every result
    is compared with the model's, and the sum invariant with the store's own counts, on the way."""
    import re
    vecs, q, q2 = script_vectors()
    out: dict = {}
    thr_box: list = []

    async def facets(s, stage):
        if not thr_box:                                                             # the block's own score, as the store reports it
            top = await s.search("code_chunks", q.tolist(), limit=100)
            thr_box.append(float(next(h["score"] for h in top if h["id"] == point(290)[0])))
        thr = thr_box[0]
        rx = r"def ent\d*7\("
        cases = {
            "language": (("language", 10, None, None), {}, None),
            "files top 10": (("file_path", 10, None, None), {}, None),
            "files top 3": (("file_path", 3, None, None), {}, None),
            "files all": (("file_path", 1024, None, None), {}, None),
            "types under sets": (("entity_type", 10, {"language": ["python", "go"]}, {"project_name": "p2"}), {},
                                 lambda p: p.get("language") in ("python", "go") and p.get("project_name") != "p2"),
            "files in a line range": (("file_path", 5, {"start_line": {"gte": 100, "lt": 300}}, None), {}, lambda p: 100 <= p["start_line"] < 300),
            "files without a language": (("file_path", 10, {"language": None}, None), {}, lambda p: p.get("language") is None),
            "files holding TODO(": (("file_path", 7, {"content": {"contains": "TODO("}}, None), {}, lambda p: _finds(p["content"], "TODO(")),
            "languages holding todo( in any case": (("language", 10, {"content": {"contains": "todo(", "case": False}, "project_name": ["p1", "p3"]}, None), {},
                                                    lambda p: _finds(p["content"], "todo(", False) and p["project_name"] in ("p1", "p3")),
            "files matching a regex": (("file_path", 10, {"content": {"matches": rx}}, None), {}, lambda p: re.search(rx.encode(), p["content"].encode(), re.M) is not None),
            "files near the block": (("file_path", 10, None, None), {"query_vector": q.tolist(), "score_threshold": thr}, None),
            "languages near the block, one project": (("language", 10, {"project_name": "p2"}, None), {"query_vector": q.tolist(), "score_threshold": thr},
                                                      lambda p: p["project_name"] == "p2"),
            "never stored": (("file_path", 10, {"language": "cobol"}, None), {}, lambda p: False),
        }
        for name, (args, kw, pred) in cases.items():
            key, limit, flt, mn = args
            got = await s.facet("code_chunks", key, limit, flt, mn, **kw)
            out[f"{stage}: {name}"] = got
            if model is not None:
                want, counted = model.facet(key, limit, pred, kw.get("query_vector"), kw.get("score_threshold"))
                assert got == want, f"{stage}: {name}: {got} vs {want}"
                assert got["total"] + got["missing"] == counted, name                               # the sum invariant, against the model ...
                if flt is None and mn is None and not kw:                                           # ... and against the store's own counts
                    assert counted == (await s.get_collection_info("code_chunks")).points_count, name
                if kw:
                    assert got["total"] + got["missing"] == counted == await s.count_similar("code_chunks", q.tolist(), thr, filters=flt, must_not=mn), name
                elif flt and "content" in flt and len(flt) == 1:
                    spec = flt["content"]
                    assert got["total"] == counted == await s.count_text("code_chunks", spec.get("contains"), matches=spec.get("matches"), case=spec.get("case", True))
        a, b, c = (out[f"{stage}: files {w}"]["hits"] for w in ("top 3", "top 10", "all"))
        assert a == b[:3] and b == c[:10] and len(c) == out[f"{stage}: files all"]["values"]          # the prefix property; nothing clipped below 1024
        both = await s.facet_batch("code_chunks", "file_path", np.stack([q, q2]), [thr, -2.0], limit=4, filters={"language": ["python", "rust"]})
        out[f"{stage}: batch"] = both
        if model is not None:
            pred = lambda p: p.get("language") in ("python", "rust")               # noqa: E731
            assert both == [model.facet("file_path", 4, pred, q, thr)[0], model.facet("file_path", 4, pred, q2, -2.0)[0]], stage
            assert both[1]["total"] == len(model.counting(pred)) > both[0]["total"] > 0

    def put(ids):
        return [point(i)[0] for i in ids], vecs[list(ids)], [point(i)[1] for i in ids]

    s = make_store()
    async with s:
        await s.create_collections()
        for a in range(0, 600, 100):
            batch = put(range(a, a + 100))
            await s.upsert("code_chunks", *batch)
            if model is not None:
                model.upsert(*batch)
        await facets(s, "filled")
        await s.delete("code_chunks", {"language": "go"})
        await s.delete_files("code_chunks", [point(8 * f)[1]["file_path"] for f in (36, 50)])          # one file of the block among them
        ids = list(range(40, 60)) + [291, 292]
        redo = ([point(i, 1)[0] for i in ids], vecs[ids], [point(i, 1)[1] for i in ids])
        await s.upsert("code_chunks", *redo)                                                          # replaced: new files, a new language
        if model is not None:
            model.delete(lambda p: p.get("language") == "go")
            model.delete(lambda p: p.get("file_path") in (point(8 * 36)[1]["file_path"], point(8 * 50)[1]["file_path"]))
            model.upsert(*redo)
        await facets(s, "after deletes and replacements")
        assert await s.compact("code_chunks") > 0
        await facets(s, "compacted")
        if tmp_dir is not None:
            await s.save(tmp_dir)
    if tmp_dir is not None:
        s = make_store()
        async with s:
            await s.create_collections()
            await s.load(tmp_dir)
            await facets(s, "loaded")
    return out
