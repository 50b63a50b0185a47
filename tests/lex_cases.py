"""CPU restatement of the keyword search: the term cutter, the forward index of a list of texts, the
collection statistics, the idf and the exact BM25 top-k -- plain Python and numpy float32, one operation per line so that
nothing is fused -- and the synthetic corpus the GPU tests score.  Test infrastructure only; the checker of
code-rag_amd/csrc_host/lex_terms.cpp and code-rag_amd/csrc/crh_lex.hip."""
import math

import numpy as np

LEXICAL_KEYS = ("entity_name", "content", "summary")
MAX_QUERY_TERMS = 32
f32 = np.float32


# ------------------------------------------------------------------ terms

def point_text(payload) -> bytes:
    """The text of a point: its string values under LEXICAL_KEYS, in that order, joined by a newline."""
    vals = [payload[k] for k in LEXICAL_KEYS if isinstance((payload or {}).get(k), str)]
    return "\n".join(vals).encode("utf-8", "surrogatepass")


def _is_word(c: int) -> bool:
    return c >= 0x80 or c == 0x5F or 0x30 <= c <= 0x39 or 0x41 <= c <= 0x5A or 0x61 <= c <= 0x7A


def _cls(c: int) -> str:
    if 0x30 <= c <= 0x39:
        return "D"
    if 0x41 <= c <= 0x5A:
        return "U"
    return "L"          # a-z and every byte >= 0x80


def _lower(bs: bytes) -> bytes:
    return bytes(c + 32 if 0x41 <= c <= 0x5A else c for c in bs)


def _sub_words(piece: bytes) -> list:
    out, start = [], 0
    for i in range(1, len(piece)):
        a, b = _cls(piece[i - 1]), _cls(piece[i])
        cut = (a == "L" and b == "U") or ((a == "D") != (b == "D"))
        if not cut and a == "U" and b == "U" and i + 1 < len(piece) and _cls(piece[i + 1]) == "L":
            cut = True
        if cut:
            out.append(piece[start:i])
            start = i
    out.append(piece[start:])
    return out


def terms_of(text) -> list:
    """The emitted terms of a text (bytes, or a str encoded like the store encodes it), in emission order."""
    data = text.encode("utf-8", "surrogatepass") if isinstance(text, str) else bytes(text)
    out, i, n = [], 0, len(data)
    while i < n:
        if not _is_word(data[i]):
            i += 1
            continue
        j = i
        while j < n and _is_word(data[j]):
            j += 1
        word = data[i:j]
        i = j
        subs = []
        for piece in word.split(b"_"):
            if piece:
                subs.extend(_sub_words(piece))
        emitted = [_lower(s) for s in subs]
        if len(subs) > 1:
            emitted.append(_lower(word))
        out.extend(t for t in emitted if 2 <= len(t) <= 64)
    return out


def fnv1a(term: bytes) -> int:
    h = 2166136261
    for c in term:
        h = ((h ^ c) * 16777619) & 0xFFFFFFFF
    return h


_rows_seen: dict = {}       # short texts already cut (the store tests cut the same payloads after every mutation)


def row_of(text):
    """(distinct ids ascending u32, tf u8 saturated at 255, dl) of one text."""
    key = text if isinstance(text, (str, bytes)) and len(text) < 4096 else None
    if key is not None and key in _rows_seen:
        return _rows_seen[key]
    ids = [fnv1a(t) for t in terms_of(text)]
    uniq, cnt = np.unique(np.asarray(ids, np.uint32), return_counts=True)
    out = uniq.astype(np.uint32), np.minimum(cnt, 255).astype(np.uint8), len(ids)
    if key is not None:
        _rows_seen[key] = out
    return out


def query_terms(text) -> np.ndarray:
    return row_of(text)[0]


def rows_from_texts(texts):
    """CSR forward index of a list of texts: (row_off int64 [n+1], terms u32, tf u8, dl int32)."""
    off, terms, tfs, dls = [0], [], [], []
    for t in texts:
        ids, tf, dl = row_of(t)
        terms.append(ids)
        tfs.append(tf)
        dls.append(dl)
        off.append(off[-1] + len(ids))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)   # noqa: E731
    return np.asarray(off, np.int64), cat(terms, np.uint32), cat(tfs, np.uint8), np.asarray(dls, np.int32)


# ------------------------------------------------------------------ statistics, idf

def row_ids(row_off) -> np.ndarray:
    """The row of every entry."""
    return np.repeat(np.arange(len(row_off) - 1, dtype=np.int64), np.diff(row_off))


def mask_from_words(words, n: int) -> np.ndarray:
    """Validity words (one u32 per 32-row tile, bit i = row 32 t + i) as a bool per row."""
    bits = np.unpackbits(np.asarray(words, np.uint32).view(np.uint8), bitorder="little")
    return bits[:n].astype(bool)


def words_from_mask(mask) -> np.ndarray:
    bits = np.zeros(((len(mask) + 31) // 32) * 32, np.uint8)
    bits[: len(mask)] = np.asarray(mask, bool)
    return np.packbits(bits, bitorder="little").view(np.uint32).copy()


def stats(row_off, terms, dl, mask, query_ids):
    """(df int64 per id, rows, sum_dl) over the rows whose mask is set (None: all)."""
    n = len(row_off) - 1
    ok = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    er = row_ids(row_off)
    df = np.asarray([int(np.count_nonzero(ok[er[terms == np.uint32(t)]])) for t in query_ids], np.int64)
    return df, int(ok.sum()), int(np.asarray(dl, np.int64)[ok].sum())


def idf(df, n_rows: int, sum_dl: int):
    """Lucene's idf per term, computed in f64 and rounded once to f32, and avgdl = (float)(sum_dl / N) (1 for an empty collection)."""
    out = np.asarray([f32(math.log(1.0 + (n_rows - int(d) + 0.5) / (int(d) + 0.5))) for d in df], f32)
    avgdl = f32(sum_dl / n_rows) if n_rows > 0 and sum_dl > 0 else f32(1.0)
    return out, avgdl


# ------------------------------------------------------------------ BM25

def _postings(terms):
    order = np.argsort(terms, kind="stable")
    st = terms[order]
    uniq, first = np.unique(st, return_index=True)
    ends = np.append(first[1:], len(st))
    return {int(u): order[a:b] for u, a, b in zip(uniq, first, ends)}


def bm25_search(row_off, terms, tf, dl, mask, queries, idf, k1, b, avgdl, k, row_base=0, postings=None):
    """Exact BM25 top-k.  queries: per query its distinct ids ascending; idf: per query the f32 idf of each of them.
    Returns (scores f32 [nq, k], rows int64 [nq, k], counts int64 [nq]); tail (-inf, -1)."""
    n, nq = len(row_off) - 1, len(queries)
    ok = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    er = row_ids(row_off)
    post = _postings(np.asarray(terms, np.uint32)) if postings is None else postings
    k1, b, avgdl = f32(k1), f32(b), f32(avgdl)
    ln = np.asarray(dl).astype(f32)
    ratio = ln / avgdl
    scaled = b * ratio
    one_minus_b = f32(1.0) - b
    inner = one_minus_b + scaled
    norm = k1 * inner
    k1p = k1 + f32(1.0)
    scores = np.full((nq, k), -np.inf, f32)
    rows = np.full((nq, k), -1, np.int64)
    counts = np.zeros(nq, np.int64)
    for q in range(nq):
        acc = np.zeros(n, f32)
        hit = np.zeros(n, bool)
        ids = np.asarray(queries[q], np.uint32)
        assert ids.size <= MAX_QUERY_TERMS and (np.diff(ids.astype(np.int64)) > 0).all()
        for t, w in zip(ids.tolist(), np.asarray(idf[q], f32)):        # ascending term id
            e = post.get(int(t))
            if e is None:
                continue
            r = er[e]
            c = np.asarray(tf)[e].astype(f32)
            num = c * k1p
            den = c + norm[r]
            frac = num / den
            contrib = f32(w) * frac
            acc[r] = acc[r] + contrib
            hit[r] = True
        q_rows = np.flatnonzero(hit & ok)
        counts[q] = q_rows.size
        order = q_rows[np.lexsort((q_rows, -acc[q_rows].astype(np.float64)))][:k]
        scores[q, : order.size] = acc[order]
        rows[q, : order.size] = order + row_base
    return scores, rows, counts


# ------------------------------------------------------------------ the synthetic corpus

VOCAB = 300
SPECIAL_LENGTHS = (0, 1, 2, 63, 64, 65, 300)


def vocabulary():
    """(ids of the 300 words, the id every row with entries holds, an id no row holds) -- distinct u32."""
    words = np.asarray([fnv1a(b"word%d" % i) for i in range(VOCAB)], np.uint32)
    every, nowhere = np.uint32(fnv1a(b"everywhere")), np.uint32(fnv1a(b"nowhere"))
    assert len(set(words.tolist()) | {int(every), int(nowhere)}) == VOCAB + 2
    return words, every, nowhere


def corpus(n: int, seed: int = 0):
    """n rows over a 300-word vocabulary with Zipf weights.  A row's entries are its distinct words (ascending id) plus the
    everywhere-term; rows of exactly 0, 1, 2, 63, 64, 65 and 300 entries are mixed with lognormal ones around 40 tokens, so rows
    start and end inside a 64-entry step and span several; rows 640..735 are empty (three whole tiles); rows 5..8 and 100..139
    are identical (ties); row 10 holds one word 300 times (tf 255, dl 300).  The first n rows of corpus(m) are corpus(n)."""
    words, every, _ = vocabulary()
    rng = np.random.default_rng(seed)
    zipf = 1.0 / np.arange(1, VOCAB + 1)
    zipf /= zipf.sum()
    rows = []
    for i in range(n):
        r = np.random.default_rng([seed, i])
        if 640 <= i < 736:
            rows.append({})
        elif i == 10:
            rows.append({int(words[7]): 300})
        elif i % 9 == 4:
            L = SPECIAL_LENGTHS[(i // 9) % len(SPECIAL_LENGTHS)]
            if L == 0:
                rows.append({})
                continue
            pick = r.choice(VOCAB, size=min(L, VOCAB) - 1, replace=False) if L > 1 else []
            d = {int(words[w]): int(r.integers(1, 4)) for w in pick}
            d[int(every)] = 1
            rows.append(d)
        else:
            toks = r.choice(VOCAB, size=max(1, int(r.lognormal(math.log(40.0), 0.6))), p=zipf)
            d = {}
            for w in toks:
                d[int(words[w])] = d.get(int(words[w]), 0) + 1
            d[int(every)] = 1
            rows.append(d)
    for lo, hi in ((5, 9), (100, 140)):
        for i in range(lo + 1, min(hi, n)):
            rows[i] = dict(rows[lo])
    del rng
    off, terms, tfs, dls = [0], [], [], []
    for d in rows:
        ids = sorted(d)
        terms.extend(ids)
        tfs.extend(min(d[t], 255) for t in ids)
        dls.append(sum(d.values()))
        off.append(len(terms))
    return np.asarray(off, np.int64), np.asarray(terms, np.uint32), np.asarray(tfs, np.uint8), np.asarray(dls, np.int32)


# ------------------------------------------------------------------ synthetic code chunks and the store's expected answers

_VERBS = ("parse", "load", "fetch", "merge", "retry", "build", "flush", "encode", "resolve", "compact", "render", "validate")
_NOUNS = ("request", "Header", "backoff", "Index", "token", "Payload", "shard", "Cursor", "snapshot", "Filter", "buffer", "HTTPServer")
RARE = "zyxwvutQuuxHandler"          # the identifier ONE chunk holds (chunk RARE_AT)
RARE_AT = 1234


def chunks(n: int, seed: int = 5):
    """n synthetic code chunks (payload dictionaries as the indexer writes them): snake_case and camelCase identifiers drawn
    from small vocabularies, a few files and two languages to filter on; chunk RARE_AT alone holds the identifier RARE --
    among chunks that share every other word of its content."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        v, w = rng.choice(_VERBS, 2)
        a, b = rng.choice(_NOUNS, 2)
        name = f"{v}_{a.lower()}_{w}" if i % 2 else f"{v}{a[0].upper()}{a[1:]}{b[0].upper()}{b[1:]}"
        body = " ".join(f"{rng.choice(_VERBS)}_{rng.choice(_NOUNS)}(x{int(rng.integers(0, 40))})" for _ in range(int(rng.integers(2, 12))))
        if i % 97 == 3:
            body = "return MAX_BACKOFF_MS  # raise HTTPServerError"          # identical texts: ties
            name = "retry_after"
        if i == RARE_AT:
            body = body + f" {RARE}(request)"
        p = {"file_path": f"/proj/f{i % 23}.py", "language": "python" if i % 3 else "go", "entity_type": "function" if i % 4 else "class",
             "entity_name": name, "content": f"def {name}(x):\n    {body}\n", "start_line": i % 500, "end_line": i % 500 + 9,
             "project_name": "demo"}
        if i % 5 == 0:
            p["summary"] = f"{v}s the {a} and then {w}s it"
        out.append(p)
    return out


def store_rows(col):
    """Per shard of a store collection, in local row order: (slots, alive bool) -- the rows a lexical index beside it holds."""
    out = {}
    for s, ix in col.shards.index.items():
        n = col.shards.rows[s]
        slots = np.arange(n) if col.shards.ns == 1 else np.asarray(col.slot_of[s][:n], np.int64)
        out[s] = (slots, mask_from_words(ix.alive_words(), n))
    return out


def lists_expected(row_texts, alive, passing, texts, limit, k1=1.2, b=0.75, grow=None):
    """The expected lexical answer from PLAIN LISTS -- nothing of a store is read: ``row_texts`` the rows' texts (bytes),
    ``alive`` / ``passing`` a bool per row (``passing``: alive and under the filter), ``grow`` the rows' GLOBAL rows, ascending
    (None: their positions in the lists).  Statistics over the alive rows, the exact BM25 top-``limit`` over the passing ones,
    ties to the lower global row.  Returns ``(scores f32 [nq, limit], global rows i64 [nq, limit] (-1: padding), counts i64 [nq],
    the queries' term ids)``."""
    off, terms, tf, dl = rows_from_texts(list(row_texts))
    alive, ok = np.asarray(alive, bool).reshape(-1), np.asarray(passing, bool).reshape(-1)
    term_lists = [query_terms(t) for t in texts]
    ids = np.unique(np.concatenate([np.zeros(0, np.uint32)] + term_lists))
    df, n_rows, sum_dl = stats(off, terms, dl, alive, ids)
    known = dict(zip(ids.tolist(), df.tolist()))
    queries, weights = [], []
    avgdl = f32(1.0)
    for t in term_lists:
        if t.size > MAX_QUERY_TERMS:
            keep = np.sort(np.lexsort((t, np.asarray([known[v] for v in t.tolist()], np.int64)))[:MAX_QUERY_TERMS])
            t = t[keep]
        w, avgdl = idf([known[v] for v in t.tolist()], n_rows, sum_dl)
        queries.append(t)
        weights.append(w)
    sc, ix, counts = bm25_search(off, terms, tf, dl, ok, queries, weights, k1, b, avgdl, limit)
    if grow is not None:
        grow = np.asarray(grow, np.int64).reshape(-1)
        assert (np.diff(grow) > 0).all(), "the lists are in ascending global-row order"
        ix = np.append(grow, -1)[ix]                             # (-1 picks the padding entry)
    return sc, ix, counts, queries


def hybrid_expected(stored, q_pre, row_texts, alive, passing, texts, limit, c, grow=None):
    """The expected hybrid answer from plain lists: ``stored`` [n, dim] the preprocessed rows and ``q_pre`` [nq, dim] the
    preprocessed queries; the other arguments as for :func:`lists_expected`.  The dense top-``c`` by ``oracle.search`` and the
    lexical top-``c`` by the restatement under the same mask, fused by tests/fuse_cases.py's restatement.  Per query ``[(global
    row, fused score bits, cosine or None, lexical score or None, matched)]``."""
    from oracle import search as orc
    from tests import fuse_cases
    n = len(row_texts)
    grow = np.arange(n, dtype=np.int64) if grow is None else np.asarray(grow, np.int64).reshape(-1)
    ls, lr, _, _ = lists_expected(row_texts, alive, passing, texts, c, grow=grow)
    if n:
        es, er = orc.search(np.asarray(stored, f32), np.asarray(q_pre, f32), c, alive=np.asarray(passing, np.uint8))
    else:
        es, er = np.full((len(texts), c), -np.inf, f32), np.full((len(texts), c), -1, np.int64)
    dr = np.append(grow, -1)[er]
    fused = fuse_cases.fuse_select(np.stack([es, ls], axis=1), np.stack([dr, lr], axis=1), 2, limit, "rrf", 60, None)
    out = []
    for q in range(len(texts)):
        hits = []
        for j, r in enumerate(fused[0][q].tolist()):
            if r < 0:
                continue
            in_d, in_l = np.flatnonzero(dr[q] == r), np.flatnonzero(lr[q] == r)
            hits.append((r, int(fused[1][q, j].view(np.uint32)), float(es[q, in_d[0]]) if in_d.size else None,
                         float(ls[q, in_l[0]]) if in_l.size else None, tuple(n for n, on in (("vector", in_d.size), ("lexical", in_l.size)) if on)))
        out.append(hits)
    return out


def store_lists(col, passes=None, stride=1 << 32):
    """A store collection as the plain lists of :func:`lists_expected`, every shard's rows one behind the other: ``(texts, alive,
    passing, global rows, slots)``."""
    row_texts, alive, ok, grow, slots = [], [], [], [], []
    for s, (sl, al) in sorted(store_rows(col).items()):
        pays = [col.payloads.get(int(t)) if t >= 0 else {} for t in sl]
        row_texts += [point_text(p) for p in pays]
        alive += al.tolist()
        ok += [bool(a) and (passes is None or bool(passes(p))) for a, p in zip(al.tolist(), pays)]
        grow += (np.arange(len(sl), dtype=np.int64) + s * stride).tolist()
        slots += np.asarray(sl, np.int64).tolist()
    return row_texts, alive, ok, grow, slots


def store_expected(col, texts, limit, passes=None, k1=1.2, b=0.75, stride=1 << 32):
    """What ``search_lexical`` must answer: per text ``[(id, score bits), ...]`` and the count -- :func:`lists_expected` on the
    texts of the stored payloads of every shard (:func:`store_lists`), statistics over the ALIVE rows of all shards.
    ``passes(payload) -> bool``: the filter.  Also returns the per-text GLOBAL-row lists ``(scores, rows)`` for the fusion."""
    row_texts, alive, ok, grow, slots = store_lists(col, passes, stride)
    out_s, out_r, counts, queries = lists_expected(row_texts, alive, ok, texts, limit, k1, b, grow=grow)
    slot_of = dict(zip(grow, slots))
    pairs = [[(col.ids.get(slot_of[int(r)]), int(v.view(np.uint32))) for v, r in zip(out_s[q], out_r[q]) if r >= 0] for q in range(len(texts))]
    return pairs, counts.tolist(), (out_s, out_r), queries
