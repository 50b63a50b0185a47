"""Keyword side of the store: the terms of a text and the BM25 weights.

The term cutter is native (``csrc_host/lex_terms.cpp`` in ``lib/libcoderag_tok.so``): words of letters, digits, ``_`` and
non-ASCII bytes, cut into sub-words at underscores, camel-case humps and letter/digit borders, lower-cased, hashed to 32-bit
FNV-1a ids.  The scoring is ``crh_lex_search`` (``ffi.Lex``); :func:`bm25_weights` is the one place the idf and the average
length are computed -- the store and the tests both call it, so the device and its checker never disagree about a logarithm.
"""

from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import tokenizer_native

LEXICAL_KEYS = ("entity_name", "content", "summary")   # the payload's string values that make a point's text, in this order
MAX_QUERY_TERMS = 32                                    # CRH_LEX_MAX_QUERY_TERMS
DEFAULT_THREADS = max(1, min(16, os.cpu_count() or 1))

_bound = False


def _lib() -> C.CDLL:
    global _bound
    L = tokenizer_native.lib()
    if not _bound:
        L.crl_terms_batch.argtypes = [C.c_int64, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_int]
        L.crl_terms_batch.restype = C.c_void_p
        L.crl_terms_entries.argtypes = [C.c_void_p]
        L.crl_terms_entries.restype = C.c_int64
        L.crl_terms_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.crl_terms_copy.restype = None
        L.crl_terms_free.argtypes = [C.c_void_p]
        L.crl_terms_free.restype = None
        _bound = True
    return L


def point_text(payload) -> bytes:
    """The text of a point: its string values under ``LEXICAL_KEYS``, in that order, joined by a newline; absent or
    non-string values are skipped.  Encoded like the store encodes text (UTF-8, lone surrogates passed through)."""
    vals = [payload[k] for k in LEXICAL_KEYS if isinstance((payload or {}).get(k), str)]
    return "\n".join(vals).encode("utf-8", "surrogatepass")


def _bytes(text) -> bytes:
    return text.encode("utf-8", "surrogatepass") if isinstance(text, str) else bytes(text)


def terms_batch(texts, threads: int = 0):
    """The forward index of a list of texts (str or bytes) as CSR: ``(row_off int64 [n + 1], terms uint32, tf uint8, dl
    int32)`` -- per text its distinct term ids ascending, their occurrences saturated at 255, and the number of emitted terms."""
    L = _lib()
    raw = [_bytes(t) for t in texts]
    n = len(raw)
    ptrs = (C.c_char_p * max(n, 1))(*raw)
    lens = (C.c_int64 * max(n, 1))(*[len(r) for r in raw])
    res = L.crl_terms_batch(n, ptrs, lens, int(threads) if threads and threads > 0 else DEFAULT_THREADS)
    try:
        ne = int(L.crl_terms_entries(res))
        row_off, terms = np.zeros(n + 1, np.int64), np.zeros(ne, np.uint32)
        tf, dl = np.zeros(ne, np.uint8), np.zeros(n, np.int32)
        L.crl_terms_copy(res, row_off.ctypes.data, terms.ctypes.data, tf.ctypes.data, dl.ctypes.data)
    finally:
        L.crl_terms_free(res)
    return row_off, terms, tf, dl


def query_terms(text) -> np.ndarray:
    """The distinct term ids of a query text, ascending; its own term frequencies are ignored."""
    return terms_batch([text], threads=1)[1]


def bm25_weights(df, n_rows: int, sum_dl: int):
    """``(idf float32 per term, avgdl float32)`` from the integer statistics of the collection's alive rows: Lucene's
    ``idf = log(1 + (N - df + 0.5) / (df + 0.5))`` computed in float64 and rounded once, always > 0, and ``avgdl = sum_dl / N``
    (1 for a collection without terms: nothing is scored then)."""
    idf = np.asarray([np.float32(math.log(1.0 + (n_rows - int(d) + 0.5) / (int(d) + 0.5))) for d in df], np.float32)
    avgdl = np.float32(sum_dl / n_rows) if n_rows > 0 and sum_dl > 0 else np.float32(1.0)
    return idf, avgdl


def rarest(terms, df, limit: int = MAX_QUERY_TERMS):
    """At most ``limit`` of a query's terms: those with the smallest ``df``, ties to the lower id; returned ascending by id
    with their positions in ``terms``."""
    terms = np.asarray(terms, np.uint32)
    if terms.size <= limit:
        keep = np.arange(terms.size)
    else:
        keep = np.sort(np.lexsort((terms, np.asarray(df, np.int64)))[:limit])
    return terms[keep], keep
