"""The literal-substring match restated on the CPU (include/coderag_hip.h, crh_text_match), and the corpora the
text tests share.  The restatement is ``bytes.find`` on each row's own bytes -- nothing of the kernel's streaming is repeated.

Definitions (this repository's own):
  * a row matches pattern p iff p occurs contiguously inside the row's own bytes; a match never spans two rows;
  * folding maps ASCII A..Z to a..z only, on text and pattern; every other byte ('@', '[', '`', '{', NUL, >= 0x80) is itself;
  * ALL: every pattern; ANY: at least one;
  * bit r of the result is set iff the mask bit is set (no mask: every row) and the row matches.
"""
import numpy as np

U32 = np.uint32

# The kernel's streaming geometry (code-rag_amd/csrc/crh_text.hip: kTextLane, kTextStep, kTextWindow), MIRRORED here so that
# the boundary cases can be placed: a lane loads 16 bytes per step, a wave covers 64 lanes = 1024 bytes per step, and keeps 4 steps
# = 4096 bytes in flight; the stream of a 32-row tile starts at the 16-byte boundary at or below the tile's first byte.
LANE, STEP, WINDOW = 16, 1024, 4096
MAX_PATTERNS, MAX_PATTERN_BYTES = 8, 64

_FOLD = bytes(c + 32 if 65 <= c <= 90 else c for c in range(256))


def fold(b: bytes) -> bytes:
    """ASCII A..Z -> a..z; every other byte unchanged."""
    return bytes(b).translate(_FOLD)


def row_matches(row: bytes, patterns, fold_case: bool = False, any_of: bool = False) -> bool:
    if fold_case:
        row, patterns = fold(row), [fold(p) for p in patterns]
    found = [bytes(row).find(bytes(p)) >= 0 for p in patterns]
    return any(found) if any_of else all(found)


def match_rows(rows, patterns, fold_case: bool = False, any_of: bool = False, mask=None) -> np.ndarray:
    """bool per row: mask bit (None: every row) AND the row matches."""
    out = np.asarray([row_matches(r, patterns, fold_case, any_of) for r in rows], bool).reshape(len(rows))
    return out if mask is None else out & np.asarray(mask, bool)


def words_from_mask(mask) -> np.ndarray:
    """bool per row -> one uint32 per 32-row tile, bit i of word t = row 32 t + i (the bits past the last row are 0)."""
    mask = np.asarray(mask, bool)
    n = mask.size
    padded = np.zeros(((n + 31) // 32) * 32, bool)
    padded[:n] = mask
    return np.packbits(padded.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).astype(U32)


def mask_from_words(words, n: int) -> np.ndarray:
    bits = np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")
    return bits[:n].astype(bool)


def csr(rows) -> tuple:
    """(row_off int64 [n + 1], the rows' bytes one behind the other)."""
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    return off, b"".join(bytes(r) for r in rows)


def filler(n: int, seed: int = 0) -> bytes:
    """n bytes of lower-case letters and blanks that hold none of the planted strings (no digit, no upper case, no punctuation)."""
    rng = np.random.default_rng(seed)
    return bytes(rng.choice(np.frombuffer(b"abcdefghijklmnopqrstuvwxyz  \n", np.uint8), size=n))


def pattern_of(length: int) -> bytes:
    """A pattern of `length` bytes no filler holds: digits, upper case and punctuation, no byte repeated inside the first 4."""
    base = b"X9#Q_7@Z" + bytes(48 + (i * 7) % 10 for i in range(MAX_PATTERN_BYTES))
    return base[:length]


def planted_rows(n_rows: int, row_len: int, plants, seed: int = 0) -> list:
    """n_rows filler rows of row_len bytes; plants = [(absolute byte position in the arena, pattern bytes)]: the pattern is
    written over the filler there (the caller keeps it inside one row unless it WANTS it to straddle a row end)."""
    blob = bytearray(filler(n_rows * row_len, seed))
    for pos, pat in plants:
        blob[pos:pos + len(pat)] = pat
    return [bytes(blob[i * row_len:(i + 1) * row_len]) for i in range(n_rows)]
