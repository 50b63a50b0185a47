"""Regular expressions as byte DFAs for ``crh_text_regex``.

The definition is Python's ``re`` on BYTES: a row matches iff
``re.compile(pattern_bytes, re.MULTILINE | (re.IGNORECASE if not case else 0)).search(row_bytes)`` finds something.  The pattern is
parsed by the stdlib's own parser (``re._parser`` / ``sre_parse``), so what a construct means cannot drift from ``re``; this module
turns the parse tree into a Thompson NFA whose epsilon edges may carry an assertion (``^ $ \\A \\Z \\b \\B``), and the NFA into a DFA
by subset construction over 256 byte symbols plus END.  A DFA state is (NFA set, kind of the previous byte); assertions are resolved
when the NEXT symbol is known.  Reaching the NFA's final state goes to one absorbing ACCEPT state, and the NFA's start is re-added
after every byte (an unanchored search), so the table is total and needs no dead state.  Not minimised.

Consequences of "``re`` on bytes": ``\\w \\d \\s \\b`` are ASCII, ``.`` is any byte but ``\\n``, case folding touches ASCII letters only,
and a non-ASCII character is its UTF-8 byte sequence -- ``é+`` repeats the LAST byte of ``é``.

Refused (``ValueError`` naming the key and the construct): back-references, look-ahead / look-behind, conditionals, inline flags,
repeat bounds over 64, an empty pattern, one over 256 bytes, what ``re`` rejects, and a DFA over 256 states or 32768 table bytes.
"""
from __future__ import annotations

import functools
import re
import warnings
from typing import NamedTuple

import numpy as np

try:                                    # Python >= 3.11
    from re import _constants as _sc, _parser as _sp
except ImportError:                     # Python <= 3.10
    import sre_constants as _sc
    import sre_parse as _sp

MAX_PATTERN_BYTES = 256
MAX_REPEAT = 64
MAX_STATES = 256                        # CRH_REGEX_MAX_STATES
MAX_TABLE_BYTES = 32768                 # CRH_REGEX_MAX_TABLE_BYTES
MAX_LITERALS, MAX_LITERAL_BYTES, MIN_LITERAL_BYTES = 8, 64, 3
_MAX_NFA = 20000                        # NFA states built before a pattern is called too large (nested counted repeats)

_EDGE, _NEWLINE, _WORD, _OTHER = 0, 1, 2, 3      # the kind of a byte (EDGE: no byte -- before the first, behind the last)
_WORD_BYTES = frozenset(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_")
_KIND = np.full(256, _OTHER, np.int64)
_KIND[list(_WORD_BYTES)] = _WORD
_KIND[10] = _NEWLINE
_DIGIT = frozenset(b"0123456789")
_SPACE = frozenset(b" \t\n\r\f\v")
_ALL = frozenset(range(256))


def _lower(c: int) -> int:
    return c + 32 if 65 <= c <= 90 else c


class _Refused(Exception):
    """Why a pattern is not compiled; the public function names the key in front of it."""


class RegexDFA(NamedTuple):
    """A compiled pattern in the format of ``crh_text_regex``: ``s = 0``; for each byte ``b``:
    ``s = trans[s * n_classes + class_of[b]]``; then ``s = trans[s * n_classes + end_class]``; a match iff ``s == accept``.
    ``literals``: byte strings every matching row holds (folded to lower case when the pattern ignores case)."""
    n_states: int
    n_classes: int
    class_of: np.ndarray       # uint8 [256]
    end_class: int
    trans: np.ndarray          # uint8 [n_states * n_classes]
    accept: int
    literals: tuple

    def search(self, row: bytes) -> bool:
        """The table walk the device does, on the host."""
        t, nc, s = self.trans.tolist(), self.n_classes, 0
        for c in self.class_of[np.frombuffer(bytes(row), np.uint8)].tolist():
            s = t[s * nc + c]
        return t[s * nc + self.end_class] == self.accept


# ---------------------------------------------------------------------------------------------------------------- parse tree -> NFA
class _NFA:
    def __init__(self):
        self.eps: list[list] = []        # state -> [(target, assertion or None)]
        self.edge: list = []             # state -> (frozenset of bytes, target) or None

    def new(self) -> int:
        if len(self.eps) >= _MAX_NFA:
            raise _Refused("the pattern is too large (its counted repeats expand to too many states)")
        self.eps.append([])
        self.edge.append(None)
        return len(self.eps) - 1


def _category(cat) -> frozenset:
    table = {_sc.CATEGORY_DIGIT: _DIGIT, _sc.CATEGORY_SPACE: _SPACE, _sc.CATEGORY_WORD: _WORD_BYTES}
    neg = {_sc.CATEGORY_NOT_DIGIT: _DIGIT, _sc.CATEGORY_NOT_SPACE: _SPACE, _sc.CATEGORY_NOT_WORD: _WORD_BYTES}
    if cat in table:
        return table[cat]
    if cat in neg:
        return _ALL - neg[cat]
    raise _Refused(f"the character category {cat} is not supported")


def _byte_set(op, av, fold: bool) -> frozenset:
    """The bytes an atom consumes.  Folding is ``re``'s on bytes: a byte is tested by its ASCII lower case against the lowered
    members (a negation applies to the result)."""
    if op is _sc.ANY:
        return _ALL - {10}
    negate = op is _sc.NOT_LITERAL
    if op in (_sc.LITERAL, _sc.NOT_LITERAL):
        members = {av}
    else:
        members = set()
        for o, a in av:
            if o is _sc.NEGATE:
                negate = True
            elif o is _sc.LITERAL:
                members.add(a)
            elif o is _sc.RANGE:
                members.update(range(a[0], a[1] + 1))
            elif o is _sc.CATEGORY:
                members |= _category(a)
            else:
                raise _Refused(f"the set item {o} is not supported")
    members = {c for c in members if c < 256}
    if fold:
        low = {_lower(c) for c in members}
        hit = {b for b in range(256) if _lower(b) in low}
    else:
        hit = members
    return frozenset(_ALL - hit if negate else hit)


_ASSERTIONS = {_sc.AT_BEGINNING: "^", _sc.AT_BEGINNING_LINE: "^", _sc.AT_END: "$", _sc.AT_END_LINE: "$",
               _sc.AT_BEGINNING_STRING: "A", _sc.AT_END_STRING: "Z", _sc.AT_BOUNDARY: "b", _sc.AT_NON_BOUNDARY: "B"}


def _build(nfa: _NFA, items, start: int, fold: bool) -> int:
    """Threads ``items`` (a parsed sequence) behind ``start``; returns the state the sequence ends in."""
    cur = start
    for op, av in items:
        if op in (_sc.LITERAL, _sc.NOT_LITERAL, _sc.ANY, _sc.IN):
            nxt = nfa.new()
            nfa.edge[cur] = (_byte_set(op, av, fold), nxt)
            cur = nfa.new()                      # (a state holds one byte edge: the next atom starts on a fresh one)
            nfa.eps[nxt].append((cur, None))
        elif op is _sc.AT:
            if av not in _ASSERTIONS:
                raise _Refused(f"the assertion {av} is not supported")
            nxt = nfa.new()
            nfa.eps[cur].append((nxt, _ASSERTIONS[av]))
            cur = nxt
        elif op is _sc.SUBPATTERN:
            _, add_flags, del_flags, sub = av
            if add_flags or del_flags:
                raise _Refused("inline flags ((?i:...), (?s:...), ...) are not supported: `case` is the only switch")
            cur = _build(nfa, sub, cur, fold)
        elif op is _sc.BRANCH:
            end = nfa.new()
            for alt in av[1]:
                a = nfa.new()
                nfa.eps[cur].append((a, None))
                nfa.eps[_build(nfa, alt, a, fold)].append((end, None))
            cur = end
        elif op in (_sc.MAX_REPEAT, _sc.MIN_REPEAT):
            lo, hi, sub = av
            if lo > MAX_REPEAT or (hi is not _sc.MAXREPEAT and hi > MAX_REPEAT):
                raise _Refused(f"a repeat bound over {MAX_REPEAT} ({{{lo},{'' if hi is _sc.MAXREPEAT else hi}}})")
            for _ in range(lo):
                cur = _build(nfa, sub, _nfa_fresh(nfa, cur), fold)
            if hi is _sc.MAXREPEAT:              # zero or more: a loop through a fresh pair of states
                a, end = _nfa_fresh(nfa, cur), nfa.new()
                nfa.eps[a].append((end, None))
                b = _nfa_fresh(nfa, a)
                nfa.eps[_build(nfa, sub, b, fold)].append((a, None))
                cur = end
            else:
                end = nfa.new()
                for _ in range(hi - lo):         # each optional copy may be skipped to the end
                    nfa.eps[cur].append((end, None))
                    cur = _build(nfa, sub, _nfa_fresh(nfa, cur), fold)
                nfa.eps[cur].append((end, None))
                cur = end
        elif op is _sc.GROUPREF:
            raise _Refused("a back-reference is not supported")
        elif op in (_sc.ASSERT, _sc.ASSERT_NOT):
            raise _Refused("look-ahead / look-behind is not supported")
        elif op is _sc.GROUPREF_EXISTS:
            raise _Refused("a conditional ((?(1)...)) is not supported")
        else:
            raise _Refused(f"the construct {op} is not supported")
    return cur


def _nfa_fresh(nfa: _NFA, cur: int) -> int:
    """A new state one epsilon edge behind ``cur``."""
    s = nfa.new()
    nfa.eps[cur].append((s, None))
    return s


# ------------------------------------------------------------------------------------------------------------------------ NFA -> DFA
def _holds(a: str, pk: int, nk: int) -> bool:
    """Does assertion ``a`` hold between a byte of kind ``pk`` and a symbol of kind ``nk`` (EDGE: none)?"""
    if a == "^":
        return pk in (_EDGE, _NEWLINE)
    if a == "$":
        return nk in (_EDGE, _NEWLINE)
    if a == "A":
        return pk == _EDGE
    if a == "Z":
        return nk == _EDGE
    if pk == _EDGE and nk == _EDGE:                 # (re's quirk: neither \b nor \B matches on a zero-byte subject)
        return False
    return ((pk == _WORD) != (nk == _WORD)) == (a == "b")


def _closure(nfa: _NFA, states, pk: int, nk: int) -> set:
    seen, stack = set(states), list(states)
    while stack:
        for t, a in nfa.eps[stack.pop()]:
            if t not in seen and (a is None or _holds(a, pk, nk)):
                seen.add(t)
                stack.append(t)
    return seen


def _to_dfa(nfa: _NFA, start: int, final: int):
    # bytes that no edge and no assertion tells apart walk the same way: construct over those groups
    sets = sorted({e[0] for e in nfa.edge if e is not None}, key=sorted)
    sig = np.zeros((len(sets) + 1, 256), np.int64)
    sig[0] = _KIND
    for i, bs in enumerate(sets):
        sig[i + 1, list(bs)] = 1
    _, rep, group_of = np.unique(sig, axis=1, return_index=True, return_inverse=True)
    group_of = group_of.reshape(-1)
    reps = [int(r) for r in rep]                       # one byte per group
    kinds = [int(_KIND[r]) for r in reps]
    ng = len(reps)

    first = (frozenset([start]), _EDGE)
    ids = {first: 0}
    order = [first]
    rows: list[list] = []                              # per state: ng targets, then END's (-1: ACCEPT)
    i = 0
    while i < len(order):
        kernel, pk = order[i]
        i += 1
        closed = {nk: _closure(nfa, kernel, pk, nk) for nk in set(kinds) | {_EDGE}}
        row = []
        for g in range(ng):
            cl = closed[kinds[g]]
            if final in cl:
                row.append(-1)
                continue
            b = reps[g]
            nxt = {start}
            for s in cl:
                e = nfa.edge[s]
                if e is not None and b in e[0]:
                    nxt.add(e[1])
            key = (frozenset(nxt), kinds[g])
            if key not in ids:
                if len(order) + 1 >= MAX_STATES:       # (one id is ACCEPT's)
                    raise _Refused(f"its DFA has more than {MAX_STATES} states")
                ids[key] = len(order)
                order.append(key)
            row.append(ids[key])
        row.append(-1 if final in closed[_EDGE] else ids[(kernel, pk)])   # END: ACCEPT, or anywhere else (here: stay)
        rows.append(row)
    n_states = len(order) + 1
    accept = n_states - 1
    table = np.array(rows + [[-1] * (ng + 1)], np.int64)
    table[table < 0] = accept
    # bytes with identical columns share a class; END keeps a class of its own, the last one
    cols, cls = np.unique(table[:, :ng], axis=1, return_inverse=True)
    cls = cls.reshape(-1)
    n_classes = cols.shape[1] + 1
    if n_states * n_classes > MAX_TABLE_BYTES:
        raise _Refused(f"its DFA table has {n_states * n_classes} bytes (at most {MAX_TABLE_BYTES})")
    trans = np.concatenate([cols, table[:, ng:]], axis=1).astype(np.uint8)
    class_of = cls[group_of].astype(np.uint8)
    return n_states, n_classes, class_of, n_classes - 1, np.ascontiguousarray(trans).reshape(-1), accept


# -------------------------------------------------------------------------------------------------------------- required literals
def _literals(items, fold: bool) -> tuple:
    """Byte strings every match holds: maximal runs of LITERAL in the mandatory top-level sequence, seen through plain groups
    and through the first copy of a repeat with minimum >= 1.  Nothing comes from an alternation, an optional part or a class."""
    runs, run = [], bytearray()

    def flush():
        if len(run) >= MIN_LITERAL_BYTES:
            runs.append(bytes(run[:MAX_LITERAL_BYTES]))
        run.clear()

    def walk(seq):
        for op, av in seq:
            if op is _sc.LITERAL and av < 256:
                run.append(_lower(av) if fold else av)
            elif op is _sc.SUBPATTERN and not av[1] and not av[2]:
                walk(av[3])
            elif op in (_sc.MAX_REPEAT, _sc.MIN_REPEAT) and av[0] >= 1:
                walk(av[2])                  # the first copy continues the run; what follows it may be another copy
                flush()
            else:
                flush()

    walk(items)
    flush()
    out: list = []
    for r in sorted(set(runs), key=lambda r: (-len(r), r)):
        if len(out) < MAX_LITERALS:
            out.append(r)
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------------- public
@functools.lru_cache(maxsize=64)
def _compile(pattern: bytes, case: bool) -> RegexDFA:
    if not pattern:
        raise _Refused("an empty pattern")
    if len(pattern) > MAX_PATTERN_BYTES:
        raise _Refused(f"the pattern has {len(pattern)} bytes of UTF-8 (1..{MAX_PATTERN_BYTES})")
    flags = re.MULTILINE | (0 if case else re.IGNORECASE)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            re.compile(pattern, flags)
            tree = _sp.parse(pattern, flags)
    except re.error as e:
        raise _Refused(f"re rejects the pattern: {e}") from None
    except (RecursionError, OverflowError) as e:
        raise _Refused(f"re rejects the pattern: {type(e).__name__}") from None
    state = getattr(tree, "state", None) or tree.pattern
    if int(state.flags) & ~int(flags):
        raise _Refused("inline flags ((?i), (?s), (?x), ...) are not supported: `case` is the only switch")
    nfa = _NFA()
    start = nfa.new()
    final = _build(nfa, tree, start, not case)
    return RegexDFA(*_to_dfa(nfa, start, final), _literals(tree, not case))


def compile_regex(pattern, case: bool = True, key: str = "") -> RegexDFA:
    """``pattern`` (a ``str``, encoded as UTF-8 with ``surrogatepass``, or bytes) as a :class:`RegexDFA`; ``case=False`` ignores
    the case of ASCII letters.  ``ValueError`` naming ``key`` and the construct for what is refused.  The last 64 distinct
    patterns are kept."""
    if isinstance(pattern, str):
        pattern = pattern.encode("utf-8", "surrogatepass")
    if not isinstance(pattern, (bytes, bytearray)):
        raise ValueError(f"regex on {key!r}: the pattern must be a str, not {pattern!r}")
    try:
        return _compile(bytes(pattern), bool(case))
    except _Refused as e:
        raise ValueError(f"regex on {key!r}: {e} (pattern {bytes(pattern)[:80]!r})") from None
