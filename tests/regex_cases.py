"""The regular-expression match restated on the CPU (include/coderag_hip.h, crh_text_regex) and what the regex
tests share: a seeded random pattern generator and random rows.  The restatement is Python's ``re`` on each row's own BYTES --
nothing of the compiler or of the kernel is repeated.

Definition: a row matches iff ``re.compile(pattern_bytes, re.MULTILINE | (re.IGNORECASE if not case else 0)).search(row)`` finds
something; bit r of the result is set iff the mask bit is set (no mask: every row) and the row matches.
"""
import re
import warnings

import numpy as np

from tests.text_cases import csr, filler, words_from_mask  # noqa: F401  (re-exported: the regex tests take them from here)

ALPHABET = b"abAB_1 \n"          # what the random rows are made of: both cases, a word byte that is no letter, a digit, blank, newline


def encode(pattern) -> bytes:
    return pattern.encode("utf-8", "surrogatepass") if isinstance(pattern, str) else bytes(pattern)


def re_compile(pattern, case: bool = True):
    """The oracle, or None for a pattern ``re`` rejects."""
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return re.compile(encode(pattern), re.MULTILINE | (0 if case else re.IGNORECASE))
    except (re.error, RecursionError, OverflowError):
        return None


def row_matches(row: bytes, pattern, case: bool = True) -> bool:
    return re_compile(pattern, case).search(bytes(row)) is not None


def match_rows(rows, pattern, case: bool = True, mask=None) -> np.ndarray:
    """bool per row: mask bit (None: every row) AND the row matches."""
    rx = re_compile(pattern, case)
    out = np.asarray([rx.search(bytes(r)) is not None for r in rows], bool).reshape(len(rows))
    return out if mask is None else out & np.asarray(mask, bool)


def random_rows(rng, n: int, max_len: int) -> list:
    """n rows of 0..max_len bytes over ALPHABET."""
    alphabet = np.frombuffer(ALPHABET, np.uint8)
    return [bytes(rng.choice(alphabet, size=int(rng.integers(0, max_len + 1)))) for _ in range(n)]


_ATOMS = ("a", "b", "A", "B", "_", "1", " ", r"\n", ".", r"\w", r"\s", r"\d", "[ab]", r"[^a\n]", r"\b", r"\B", "^", "$")
_QUANTIFIERS = ("*", "+", "?", "{2}", "{1,3}", "*?")


def random_pattern(rng, depth: int = 0) -> str:
    """A pattern over literals, ``\\n . \\w \\s \\d [ab] [^a\\n] \\b \\B ^ $``, groups and alternation, with the quantifiers
    ``* + ? {2} {1,3} *?``.  ``re`` rejects some (a quantifier behind an assertion, ...): those are no cases."""
    parts = []
    for _ in range(int(rng.integers(1, 5))):
        roll = rng.random()
        if depth < 2 and roll < 0.15:
            atom = "(" + random_pattern(rng, depth + 1) + ")"
        elif depth < 2 and roll < 0.25:
            atom = "(?:" + random_pattern(rng, depth + 1) + "|" + random_pattern(rng, depth + 1) + ")"
        else:
            atom = _ATOMS[int(rng.integers(0, len(_ATOMS)))]
        if rng.random() < 0.3:
            atom += _QUANTIFIERS[int(rng.integers(0, len(_QUANTIFIERS)))]
        parts.append(atom)
    return "".join(parts)


def random_cases(seed: int, n: int) -> list:
    """n (pattern, case) pairs ``re`` accepts; 30 % ignore case."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        pattern, case = random_pattern(rng), bool(rng.random() >= 0.3)
        if re_compile(pattern, case) is not None:
            out.append((pattern, case))
    return out
