"""Guided decoding: token-level deterministic automata.

A `TokenGuide` says, state by state, which tokens a request may draw next and
where each one leads.  The last stage keeps the tables of the guides in flight
on the device (parallel/draw.py `_guide_tab`), masks a guided row's logits with
its current state ahead of every draw and advances the state behind the draw,
inside the captured decode graphs: the host never sees the state
(csrc/kernels/guide.hip; ops/reference.py `guide_mask` / `guide_advance` are
the exact definitions).

`compile_regex` and `compile_choice` build a guide from a byte-level regular
expression or a set of strings and a tokenizer's `token_bytes`:

    regex -> Thompson NFA over bytes -> subset construction -> trim the states
    that cannot reach an accepting one -> lift to tokens (walk every token's
    bytes from every state, vectorised over the vocabulary) -> group tokens
    with identical columns into classes

The whole output must match.  EOS, when the vocabulary has one, is a class of
its own: drawable exactly in accepting states, leading to a final state in
which only EOS is drawable.
"""
from __future__ import annotations

import hashlib
import threading
from typing import List, Optional, Sequence

import numpy as np

MAX_STATES = 32767       # a state is an int16
_MAX_NFA = 1 << 16       # NFA states a pattern may expand to ({m,n} copies its operand)
_MAX_REPEAT = 1000


class TokenGuide:
    """A deterministic automaton over tokens.

    cls  int16 [vocab]: token -> class in [0, C)
    next int16 [S, C]:  the state after a token of that class from that state,
                        or -1 (dead); row-major, cell s * C + c; state 0 starts
    Token t may be drawn in state s iff next[s, cls[t]] >= 0.  EOS is an
    ordinary token: a builder that wants "EOS only where the match is
    complete" gives it a class of its own whose cells are -1 except in
    accepting states.  `eos` only records which token the builder meant (the
    engine checks it against the model's)."""

    def __init__(self, cls, next, vocab: int, eos: Optional[int] = None):
        self.cls, self.next, self.vocab, self.eos = cls, next, vocab, eos
        self._digest = None
        self._rows = None
        self._valid = None  # the caps validate() last passed with

    @property
    def S(self) -> int:
        return int(self.next.shape[0])

    @property
    def C(self) -> int:
        return int(self.next.shape[1])

    def validate(self, max_classes: int = 4096, max_cells: int = 1 << 20) -> None:
        if self._valid == (max_classes, max_cells):
            return
        cls, nxt, V = self.cls, self.next, self.vocab
        if isinstance(V, bool) or not isinstance(V, (int, np.integer)) or V < 1:
            raise ValueError("guide: vocab must be a positive integer")
        if self.eos is not None and (isinstance(self.eos, bool) or not isinstance(self.eos, (int, np.integer))):
            raise ValueError("guide: eos must be None or a token id")
        if not isinstance(cls, np.ndarray) or cls.dtype != np.int16 or cls.shape != (V,):
            raise ValueError(f"guide: cls must be an int16 numpy array [vocab = {V}]")
        if not isinstance(nxt, np.ndarray) or nxt.dtype != np.int16 or nxt.ndim != 2 or nxt.shape[0] < 1:
            raise ValueError("guide: next must be an int16 numpy array [S, C] with S >= 1")
        S, C = nxt.shape
        if not 1 <= C <= max_classes:
            raise ValueError(f"guide: {C} classes; at least 1 and at most {max_classes} (max_guide_classes)")
        if S * C > max_cells:
            raise ValueError(f"guide: {S} states x {C} classes = {S * C} cells; at most {max_cells} "
                             "(max_guide_cells)")
        if S > MAX_STATES:
            raise ValueError(f"guide: {S} states; at most {MAX_STATES}")
        if int(cls.min()) < 0 or int(cls.max()) >= C:
            raise ValueError(f"guide: every class must lie in [0, {C})")
        if int(nxt.min()) < -1 or int(nxt.max()) >= S:
            raise ValueError(f"guide: every cell of next must lie in [-1, {S})")
        # every state reachable from 0 through classes some token has keeps a
        # token to draw: the guarantee the other logit edits give
        used = np.zeros(C, dtype=bool)
        used[cls] = True
        live = np.where(used[None, :], nxt, -1)
        seen = np.zeros(S, dtype=bool)
        seen[0] = True
        front = np.array([0])
        while front.size:
            rows = live[front]
            if (rows.max(axis=1) < 0).any():
                s = int(front[int(np.argmax(rows.max(axis=1) < 0))])
                raise ValueError(f"guide: state {s} is reachable and leaves no token to draw")
            nx = np.unique(rows[rows >= 0])
            front = nx[~seen[nx]]
            seen[front] = True
        self._valid = (max_classes, max_cells)

    @property
    def digest(self) -> str:
        """Stable over equal (vocab, eos, cls, next): equal guides share one
        row of the last stage's table."""
        if self._digest is None:
            h = hashlib.sha256()
            h.update(repr((int(self.vocab), None if self.eos is None else int(self.eos),
                           tuple(self.next.shape))).encode())
            h.update(np.ascontiguousarray(self.cls).tobytes())
            h.update(np.ascontiguousarray(self.next).tobytes())
            self._digest = h.hexdigest()
        return self._digest

    def walk(self, tokens: Sequence[int]) -> int:
        """The state after `tokens` from the start, -1 once dead."""
        if self._rows is None:
            self._rows = (self.cls.tolist(), self.next.tolist())
        cls, nxt = self._rows
        s = 0
        for t in tokens:
            if not 0 <= t < self.vocab:
                return -1
            s = nxt[s][cls[t]]
            if s < 0:
                return -1
        return s

    def drawable(self, state: int) -> np.ndarray:
        """bool [vocab]: the tokens that may be drawn in `state`."""
        return self.next[state][self.cls] >= 0

    def __eq__(self, other) -> bool:
        return isinstance(other, TokenGuide) and self.digest == other.digest

    def __hash__(self) -> int:
        return hash(self.digest)

    def __repr__(self) -> str:
        return f"TokenGuide(S={self.S}, C={self.C}, vocab={self.vocab}, eos={self.eos})"


class GuideRows:
    """Which guide each row of the last stage's guide table holds: the engine's
    host-side book.  Guides are interned by digest, so equal guides share a
    row; a row is pinned once per request that follows it, from submit until
    the request's KV slot is released, and only a row without pins is given
    to another guide -- a free one first, else the least recently used.  The
    caller holds `lock` around acquire and the upload that follows a fresh
    row, so no second request can be planned on a row that is still being
    written."""

    def __init__(self, rows: int):
        self.lock = threading.Lock()
        self.digest: List[Optional[str]] = [None] * rows
        self.pins = [0] * rows
        self.used = [0] * rows
        self._tick = 0

    def acquire(self, guide: TokenGuide) -> tuple:
        """-> (row, fresh): the row that holds `guide`, pinned once more;
        fresh when the caller has to write the guide into it first.  A
        ValueError when every row is pinned by another guide."""
        self._tick += 1
        d = guide.digest
        if d in self.digest:
            row, fresh = self.digest.index(d), False
        else:
            idle = [r for r, n in enumerate(self.pins) if n == 0]
            if not idle:
                raise ValueError(f"guide: all {len(self.pins)} rows of the guide table are held by other guides in "
                                 "flight (max_guides)")
            row = min(idle, key=lambda r: (self.digest[r] is not None, self.used[r]))
            self.digest[row], fresh = d, True
        self.pins[row] += 1
        self.used[row] = self._tick
        return row, fresh

    def forget(self, row: int) -> None:
        """The upload into a fresh row failed: the row holds nothing."""
        self.pins[row] = 0
        self.digest[row] = None

    def release(self, row: int) -> None:
        with self.lock:
            if 0 <= row < len(self.pins) and self.pins[row] > 0:
                self.pins[row] -= 1

    def reset(self) -> None:
        """Every request failed: no pins are left."""
        with self.lock:
            self.pins = [0] * len(self.pins)


# ---------------------------------------------------------------------------
# regular expressions over bytes
# ---------------------------------------------------------------------------
# AST: ("set", 256-bit int) | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, m, n or None)

_DIGIT = sum(1 << b for b in range(0x30, 0x3A))
_WORD = _DIGIT | sum(1 << b for b in range(0x41, 0x5B)) | sum(1 << b for b in range(0x61, 0x7B)) | 1 << 0x5F
_SPACE = sum(1 << b for b in b" \t\n\r\f\v")
_ALL = (1 << 256) - 1
_SHORT = {"d": _DIGIT, "w": _WORD, "s": _SPACE, "D": _ALL ^ _DIGIT, "W": _ALL ^ _WORD, "S": _ALL ^ _SPACE}
_CTRL = {"n": 10, "t": 9, "r": 13, "f": 12, "v": 11, "0": 0, "a": 7}


class _Parser:
    def __init__(self, pattern: str):
        if not isinstance(pattern, str):
            raise ValueError("the pattern must be a string")
        self.p, self.i = pattern, 0

    def fail(self, what: str, at: Optional[int] = None):
        raise ValueError(f"regex: {what} at position {self.i if at is None else at}")

    def peek(self) -> str:
        return self.p[self.i] if self.i < len(self.p) else ""

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        arms = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            arms.append(self.cat())
        return arms[0] if len(arms) == 1 else ("alt", arms)

    def cat(self):
        items = []
        while self.peek() not in ("", "|", ")"):
            items.append(self.repeat())
        return ("cat", items)

    def repeat(self):
        at = self.i
        node = self.atom()
        while True:
            c = self.peek()
            if c == "*":
                m, n = 0, None
            elif c == "+":
                m, n = 1, None
            elif c == "?":
                m, n = 0, 1
            elif c == "{":
                m, n = self.bounds()
            else:
                return node
            if c != "{":
                self.i += 1
            if self.peek() in ("?", "+"):
                self.fail("lazy and possessive quantifiers are not supported")
            if self.peek() in ("*", "{"):
                self.fail("a quantifier cannot follow a quantifier")
            if n is not None and (n < m or n > _MAX_REPEAT) or m > _MAX_REPEAT:
                self.fail(f"repeat bounds must satisfy m <= n <= {_MAX_REPEAT}", at)
            node = ("rep", node, m, n)

    def bounds(self) -> tuple:
        j = self.p.find("}", self.i)
        body = self.p[self.i + 1: j] if j >= 0 else ""
        lo, comma, hi = body.partition(",")
        if j < 0 or not lo.isdigit() or not lo.isascii() or (hi and (not hi.isdigit() or not hi.isascii())):
            self.fail("malformed {m}, {m,} or {m,n}")
        self.i = j + 1
        m = int(lo)
        return m, (m if not comma else (int(hi) if hi else None))

    def atom(self):
        c = self.peek()
        if c == "(":
            at = self.i
            self.i += 1
            if self.peek() == "?":
                if self.p[self.i: self.i + 2] != "?:":
                    self.fail("only (?: ) groups are supported, no lookaround, flags or named groups", at)
                self.i += 2
            node = self.alt()
            if self.peek() != ")":
                self.fail("unbalanced '('", at)
            self.i += 1
            return node
        if c in ("^", "$"):
            self.fail("anchors are not supported (the whole output is matched)")
        if c in ("*", "+", "?", "{"):
            self.fail("nothing to repeat")
        if c in ("}", "]"):
            self.fail(f"unescaped {c!r}")
        if c == ".":
            self.i += 1
            return ("set", _ALL ^ (1 << 10))
        if c == "[":
            return self.klass()
        if c == "\\":
            v = self.escape(False)
            return ("set", v[0] if isinstance(v, tuple) else 1 << v)
        self.i += 1
        b = c.encode("utf-8")
        if len(b) == 1:
            return ("set", 1 << b[0])
        return ("cat", [("set", 1 << x) for x in b])

    def escape(self, in_class: bool):
        """At a backslash: -> a byte value, or (set,) for \\d \\w \\s and their negations."""
        at = self.i
        self.i += 1
        c = self.peek()
        if c == "":
            self.fail("a trailing backslash", at)
        self.i += 1
        if c in _SHORT:
            return (_SHORT[c],)
        if c == "x":
            h = self.p[self.i: self.i + 2]
            if len(h) != 2 or any(x not in "0123456789abcdefABCDEF" for x in h):
                self.fail("\\x needs two hex digits", at)
            self.i += 2
            return int(h, 16)
        if c in _CTRL:
            return _CTRL[c]
        if c == "b" and in_class:
            return 8
        if c.isascii() and not c.isalnum():
            return ord(c)
        self.fail(f"unsupported escape \\{c} (no backreferences, word boundaries or anchors)", at)

    def klass(self):
        at = self.i
        self.i += 1
        neg = self.peek() == "^"
        if neg:
            self.i += 1
        bits, first = 0, True
        while True:
            c = self.peek()
            if c == "":
                self.fail("unbalanced '['", at)
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            lo = self.class_item()
            if isinstance(lo, tuple):
                bits |= lo[0]
                continue
            if self.peek() == "-" and self.p[self.i + 1: self.i + 2] not in ("]", ""):
                self.i += 1
                hi = self.class_item()
                if isinstance(hi, tuple) or hi < lo:
                    self.fail("bad character range", at)
                bits |= sum(1 << b for b in range(lo, hi + 1))
            else:
                bits |= 1 << lo
        return ("set", (_ALL ^ bits) if neg else bits)

    def class_item(self):
        c = self.peek()
        if c == "\\":
            return self.escape(True)
        if not c.isascii():
            self.fail("a class holds bytes: write a non-ASCII character as \\xHH escapes")
        self.i += 1
        return ord(c)


def _parse(pattern: str):
    ps = _Parser(pattern)
    node = ps.parse()
    return node


class _NFA:
    def __init__(self):
        self.eps: List[list] = []
        self.edge: List[Optional[tuple]] = []  # (256-bit set, target) or None

    def new(self) -> int:
        if len(self.eps) >= _MAX_NFA:
            raise ValueError(f"regex: the pattern expands to more than {_MAX_NFA} NFA states")
        self.eps.append([])
        self.edge.append(None)
        return len(self.eps) - 1

    def build(self, node) -> tuple:
        """-> (entry, exit) of the fragment for `node`."""
        kind = node[0]
        if kind == "set":
            a, b = self.new(), self.new()
            self.edge[a] = (node[1], b)
            return a, b
        if kind == "cat":
            a = b = self.new()
            for it in node[1]:
                x, y = self.build(it)
                self.eps[b].append(x)
                b = y
            return a, b
        if kind == "alt":
            a, b = self.new(), self.new()
            for it in node[1]:
                x, y = self.build(it)
                self.eps[a].append(x)
                self.eps[y].append(b)
            return a, b
        _, sub, m, n = node
        a = b = self.new()
        for _ in range(m):
            x, y = self.build(sub)
            self.eps[b].append(x)
            b = y
        if n is None:
            x, y = self.build(sub)
            h = self.new()
            self.eps[b].append(h)
            self.eps[h].append(x)
            self.eps[y].append(h)
            return a, h
        end = self.new()
        for _ in range(n - m):
            x, y = self.build(sub)
            self.eps[b] += [x, end]
            b = y
        self.eps[b].append(end)
        return a, end


def _byte_dfa(node) -> tuple:
    """The trimmed DFA of `node` over bytes: (D int32 [S, 256] with -1 for no
    transition, accepting bool [S]); state 0 starts.  An empty language is a
    ValueError."""
    nfa = _NFA()
    start, final = nfa.build(node)

    def closure(states) -> frozenset:
        seen, todo = set(states), list(states)
        while todo:
            for y in nfa.eps[todo.pop()]:
                if y not in seen:
                    seen.add(y)
                    todo.append(y)
        return frozenset(seen)

    first = closure([start])
    index, order, rows = {first: 0}, [first], []
    while len(rows) < len(order):
        cur = order[len(rows)]
        by_byte: dict = {}
        for x in cur:
            e = nfa.edge[x]
            if e is None:
                continue
            bits, tgt = e
            b = 0
            while bits:
                low = bits & -bits
                b = low.bit_length() - 1
                by_byte.setdefault(b, set()).add(tgt)
                bits ^= low
        row = np.full(256, -1, dtype=np.int32)
        memo: dict = {}
        for b, tg in by_byte.items():
            key = frozenset(tg)
            to = memo.get(key)
            if to is None:
                cl = closure(key)
                to = index.get(cl)
                if to is None:
                    if len(order) >= MAX_STATES:
                        raise ValueError(f"regex: more than {MAX_STATES} DFA states")
                    to = index[cl] = len(order)
                    order.append(cl)
                memo[key] = to
            row[b] = to
        rows.append(row)
    D = np.stack(rows)
    acc = np.array([final in st for st in order], dtype=bool)
    # trim: keep the states that reach an accepting one
    S = len(order)
    good = acc.copy()
    while True:
        reach = np.zeros(S + 1, dtype=bool)
        reach[:S] = good
        more = good | reach[D].any(axis=1)  # D == -1 indexes the last entry: False
        if (more == good).all():
            break
        good = more
    if not good[0]:
        raise ValueError("regex: the pattern matches nothing")
    new = np.full(S + 1, -1, dtype=np.int32)
    new[:S][good] = np.arange(int(good.sum()), dtype=np.int32)
    return new[D[good]], acc[good]


def _lift(D: np.ndarray, acc: np.ndarray, token_bytes: Sequence[bytes], eos: Optional[int]) -> TokenGuide:
    V, S = len(token_bytes), D.shape[0]
    if V < 1:
        raise ValueError("token_bytes is empty")
    if eos is not None and not 0 <= eos < V:
        eos = None
    if eos is None and ((D < 0).all(axis=1) & acc).any():
        raise ValueError("regex: without an EOS token in the vocabulary an accepting state with no continuation "
                         "leaves no token to draw")
    lens = np.fromiter((len(b) for b in token_bytes), dtype=np.int64, count=V)
    if eos is not None:
        lens[eos] = 0  # not walked: its column is written below
    Lmax = int(lens.max()) if V else 0
    mat = np.zeros((V, max(Lmax, 1)), dtype=np.uint8)
    for n in set(lens.tolist()) - {0}:  # one numpy copy per token length
        at = np.nonzero(lens == n)[0]
        mat[at, :n] = np.frombuffer(b"".join(token_bytes[i] for i in at.tolist()), dtype=np.uint8).reshape(-1, n)
    # dead is state S here; the final state (after EOS) S + 1 has no byte transitions
    dead = S
    D2 = np.full((S + 1, 256), dead, dtype=np.int32)
    D2[:S] = np.where(D >= 0, D, dead)
    order = np.argsort(-lens, kind="stable")  # longest first: position p concerns a prefix of `order`
    T = np.empty((S, V), dtype=np.int32)
    step = max(1, (1 << 24) // max(V, 1))  # states per trip: 64 MB of int32
    for s0 in range(0, S, step):
        cur = np.repeat(np.arange(s0, min(S, s0 + step), dtype=np.int32)[:, None], V, axis=1)
        for p in range(Lmax):
            k = int(np.searchsorted(-lens[order], -p, side="left"))  # tokens longer than p
            at = order[:k]
            cur[:, at] = D2[cur[:, at], mat[at, p][None, :]]
        T[s0: s0 + step] = cur
    T[:, lens == 0] = dead
    nstates = S
    if eos is not None:
        fin = S + 1
        T = np.concatenate([T, np.full((2, V), dead, dtype=np.int32)])  # rows: dead (unused), final
        T[:S, eos] = np.where(acc, fin, dead)
        T[fin, eos] = fin
        nstates = S + 2
    # token-level reachability from 0, renumbered in discovery order (0 stays 0)
    seen = np.zeros(nstates + 1, dtype=bool)
    seen[dead] = True
    seen[0] = True
    keep, front = [0], np.array([0])
    while front.size:
        nx = np.unique(T[front])
        nx = nx[~seen[nx]]
        seen[nx] = True
        keep += nx.tolist()
        front = nx
    if len(keep) > MAX_STATES:
        raise ValueError(f"regex: {len(keep)} token-level states; at most {MAX_STATES}")
    new = np.full(nstates + 1, -1, dtype=np.int32)
    new[keep] = np.arange(len(keep), dtype=np.int32)
    T = new[T[keep]].astype(np.int16)  # [S', V]
    cls, nxt = _classes(T)
    # merge the states no token sequence tells apart (Moore's refinement over the
    # classes), so that equal languages give equal guides; then the classes again
    blk = np.zeros(nxt.shape[0], dtype=np.int64)
    while True:
        sig = np.concatenate([blk[:, None], np.where(nxt >= 0, blk[np.maximum(nxt, 0)], -1)], axis=1)
        _, new = np.unique(sig, axis=0, return_inverse=True)
        new = new.reshape(-1)
        if new.max() == blk.max():
            break
        blk = new
    first = np.full(int(blk.max()) + 1, nxt.shape[0], dtype=np.int64)
    np.minimum.at(first, blk, np.arange(nxt.shape[0]))
    rank = np.empty_like(first)
    rank[np.argsort(first)] = np.arange(first.size)  # blocks in the order of their first state: 0 stays 0
    blk, reps = rank[blk], np.sort(first)
    merged = np.where(nxt[reps] >= 0, blk[np.maximum(nxt[reps], 0)], -1).astype(np.int16)
    again, nxt = _classes(merged)
    cls = again[cls]
    if nxt.shape[1] > MAX_STATES:
        raise ValueError(f"regex: {nxt.shape[1]} token classes; at most {MAX_STATES}")
    return TokenGuide(cls.astype(np.int16), np.ascontiguousarray(nxt), V, eos)


def _classes(T: np.ndarray) -> tuple:
    """Group the identical columns of T [S, n] int16: -> (class of every column
    int64 [n], T's distinct columns [S, C] in the order np.unique gives)."""
    cols = np.ascontiguousarray(T.T)
    _, firsts, inv = np.unique(cols.view(np.dtype((np.void, cols.shape[1] * 2))).ravel(),
                               return_index=True, return_inverse=True)
    return inv.reshape(-1).astype(np.int64), np.ascontiguousarray(T[:, firsts])


def compile_regex(pattern: str, token_bytes: Sequence[bytes], eos: Optional[int] = None) -> TokenGuide:
    """The guide whose outputs, decoded to bytes, match `pattern` as a whole.

    Byte-level syntax: literals (a non-ASCII character is its UTF-8 bytes) and
    escapes (\\\\ \\. \\n \\t \\r \\f \\v \\0 \\xHH, any escaped punctuation),
    `.` (any byte but \\n), classes [a-z0-9_] and [^...], \\d \\w \\s and
    their negations (ASCII), groups ( ) and (?: ), alternation |, the
    quantifiers * + ? {m} {m,} {m,n}.  Anything else -- anchors,
    backreferences, lookaround, lazy quantifiers -- is a ValueError naming the
    position.  token_bytes[t] is the bytes token t decodes to; an empty entry
    is never drawable.  EOS, when `eos` names a token of the vocabulary, is
    drawable exactly where the match is complete and only EOS follows it;
    otherwise a pattern with an accepting state that has no continuation is a
    ValueError."""
    D, acc = _byte_dfa(_parse(pattern))
    return _lift(D, acc, token_bytes, eos)


def compile_choice(strings: Sequence, token_bytes: Sequence[bytes], eos: Optional[int] = None) -> TokenGuide:
    """The guide whose outputs are exactly one of `strings` (str, as UTF-8, or
    bytes): an alternation of literals through compile_regex's path."""
    if isinstance(strings, (str, bytes)) or not hasattr(strings, "__iter__"):
        raise ValueError("guided choice: a list of strings")
    arms = []
    for s in strings:
        if not isinstance(s, (str, bytes)):
            raise ValueError("guided choice: every choice is a string")
        b = s.encode("utf-8") if isinstance(s, str) else s
        arms.append(("cat", [("set", 1 << x) for x in b]))
    if not arms:
        raise ValueError("guided choice: at least one string")
    D, acc = _byte_dfa(("alt", arms))
    return _lift(D, acc, token_bytes, eos)
