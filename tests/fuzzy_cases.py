"""The approximate substring match restated on the CPU (include/coderag_hip.h, crh_text_fuzzy) and what the fuzzy
tests share.  The restatement is Sellers' dynamic programme, row of the table by row of the table in numpy -- nothing of the
kernel's bit vectors is repeated, and nothing of the store's host helper (which walks the table column by column).

Definition (this repository's own):
  * pattern P of m bytes, 1 <= m <= 64; edits k, 0 <= k <= 3, m > k; the text is the row's own BYTES;
  * folding maps ASCII A..Z to a..z only, on text and pattern; every other byte (>= 0x80 among them) is itself;
  * the row's DISTANCE is min over all substrings S of the row of Levenshtein(P, S), where the insertion, the deletion and the
    substitution of one byte cost 1 each (a transposition therefore costs 2):
        D[0][j] = 0, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + (P[i-1] != T[j-1]), D[i-1][j] + 1, D[i][j-1] + 1),
        distance = min over j = 0 .. n of D[m][j];
  * the row matches iff distance <= k; a match never spans two rows; the empty row has distance m and never matches;
  * level d (0 .. k) of the result: bit r is set iff the mask bit is set (no mask: every row) and row r's distance is <= d;
  * the END of a row's match is the least j with D[m][j] = distance: T[j-1] is the last byte of the first substring that reaches
    the distance (j = 0, the empty substring at the row's start, only where distance = m: such a row never matches).
"""
import numpy as np

from tests.text_cases import csr, filler, fold, mask_from_words, pattern_of, words_from_mask  # noqa: F401  (re-exported: the fuzzy tests take them from here)

MAX_EDITS, MAX_PATTERN_BYTES = 3, 64


def encode(s) -> bytes:
    return s.encode("utf-8", "surrogatepass") if isinstance(s, str) else bytes(s)


def last_row(pattern: bytes, text: bytes) -> np.ndarray:
    """D[m][0 .. n] of Sellers' table, computed one pattern byte (one ROW of the table) at a time."""
    t = np.frombuffer(bytes(text), np.uint8)
    n = t.size
    ramp = np.arange(n + 1, dtype=np.int64)
    prev = np.zeros(n + 1, np.int64)                                     # D[0][j] = 0: a match may start anywhere
    for i, c in enumerate(bytes(pattern), 1):
        cur = np.empty(n + 1, np.int64)
        cur[0] = i                                                       # D[i][0] = i
        cur[1:] = np.minimum(prev[:-1] + (t != c), prev[1:] + 1)         # substitution / match, deletion of P[i-1]
        cur = np.minimum.accumulate(cur - ramp) + ramp                   # insertions: D[i][j] = min(D[i][j], D[i][j-1] + 1), left to right
        prev = cur
    return prev


def distance_end(row: bytes, pattern, fold_case: bool = False) -> tuple:
    """(distance, end) of one row by the definition above."""
    row, pattern = bytes(row), encode(pattern)
    if fold_case:
        row, pattern = fold(row), fold(pattern)
    d = last_row(pattern, row)
    best = int(d.min())
    return best, int(np.flatnonzero(d == best)[0])


def distances(rows, pattern, fold_case: bool = False) -> np.ndarray:
    return np.asarray([distance_end(r, pattern, fold_case)[0] for r in rows], np.int64).reshape(len(rows))


def levels(rows, pattern, edits: int, fold_case: bool = False, mask=None, dist=None) -> np.ndarray:
    """bool [edits + 1, rows]: level d = mask bit (None: every row) AND distance <= d."""
    dist = distances(rows, pattern, fold_case) if dist is None else np.asarray(dist)
    out = np.stack([dist <= d for d in range(edits + 1)])
    return out if mask is None else out & np.asarray(mask, bool)[None, :]


def level_words(lv) -> np.ndarray:
    """bool [levels, rows] -> uint32 [levels, ceil(rows / 32)]."""
    return np.stack([words_from_mask(m) for m in lv])


def match_line(payload_text: str, start_line: int, pattern, fold_case: bool = False) -> int:
    """``start_line`` plus the newlines before the last byte of the first substring that reaches the row's distance."""
    raw = encode(payload_text)
    _, end = distance_end(raw, pattern, fold_case)
    return start_line + raw.count(b"\n", 0, max(end - 1, 0))


# ---------------------------------------------------------------------------------------------------- brute force (tiny strings)

def levenshtein(a: bytes, b: bytes) -> int:
    """The textbook distance between two whole strings, in plain Python."""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j - 1] + (x != y), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[-1]


def brute_distance_end(row: bytes, pattern: bytes) -> tuple:
    """min over ALL substrings row[a:b] of levenshtein(pattern, row[a:b]), and the least b at which some substring reaches it."""
    per_end = [min(levenshtein(pattern, row[a:b]) for a in range(b + 1)) for b in range(len(row) + 1)]
    best = min(per_end)
    return best, per_end.index(best)


# ---------------------------------------------------------------------------------------------------- edits

def substitute(p: bytes, i: int, by: int = 0x7E) -> bytes:
    """p with byte i replaced (by '~', or by '|' where p[i] is '~')."""
    return p[:i] + bytes([by if p[i] != by else 0x7C]) + p[i + 1:]


def insert(p: bytes, i: int, byte: int = 0x7E) -> bytes:
    """p with one byte put in front of byte i."""
    return p[:i] + bytes([byte]) + p[i:]


def delete(p: bytes, i: int) -> bytes:
    return p[:i] + p[i + 1:]


def transpose(p: bytes, i: int) -> bytes:
    """p with bytes i and i + 1 swapped (they differ in every pattern the tests use it on)."""
    assert p[i] != p[i + 1]
    return p[:i] + p[i + 1:i + 2] + p[i:i + 1] + p[i + 2:]


def distinct_pattern(length: int, seed: int = 0) -> bytes:
    """``length`` bytes of digits, upper case and punctuation, no filler byte among them and -- up to 62 bytes -- no byte twice:
    one edit of it is exactly one edit away, two edits exactly two."""
    pool = b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ#@_=" + b"!$%&()*+,-./:;<>?[]^{}"
    assert length <= MAX_PATTERN_BYTES
    rng = np.random.default_rng(1000 + seed)
    order = rng.permutation(len(pool))
    return bytes(pool[int(order[i % len(pool)])] for i in range(length))


def random_rows(rng, n: int, max_len: int, alphabet: bytes = b"abAB_1 \n") -> list:
    """n rows of 0..max_len bytes over a small alphabet (approximate matches are then frequent at every level)."""
    a = np.frombuffer(alphabet, np.uint8)
    return [bytes(rng.choice(a, size=int(rng.integers(0, max_len + 1)))) for _ in range(n)]
