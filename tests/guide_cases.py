"""Shared case builders of tests/test_guide.py and tests/test_guide_gpu.py:
the synthetic vocabulary and the patterns the regex compiler is checked on,
and the hand-built guide tables the mask and advance passes are checked on
(CPU tensors, built once and left unchanged)."""
import itertools
import re

import numpy as np
import torch

from llm_sharding_demo_amd.guide import TokenGuide

# ---------------------------------------------------------------------------
# the regex compiler's vocabulary and patterns


def synthetic_vocab():
    """(token_bytes, eos): the 256 bytes, multi-byte strings that straddle the
    patterns' boundaries, empty entries, one duplicated string, and an EOS."""
    toks = [bytes([b]) for b in range(256)]
    multi = [b"ab", b"b1", b"12", b'":', b"abc", b"tr", b"ue", b"true", b"fal", b"se", b"false", b"als", b"rue",
             b'"a', b'a"', b": ", b" -", b"-1", b"1.", b".1", b"\\.", b".\n", b"\n\t", b"[x", b"x]", b"_-", b"1 ",
             b"x?", b"?A", b"xA", b"1x", b"a a", b"1a ", b" a1", b"9-", b"\tx", b"_!", b'":1', b'b1"', b"1.2"]
    multi += [bytes(p) for p in itertools.product(b"ab12c", repeat=2)]
    multi += [bytes(p) for p in itertools.product(b"ab1", repeat=3)]
    rng = np.random.default_rng(7)
    multi += [bytes(rng.integers(32, 127, size=2).tolist()) for _ in range(50)]
    seen = set()
    for m in multi:
        if m not in seen:
            seen.add(m)
            toks.append(m)
    toks += [b"", b"", b"ab", b""]  # never drawable; and a second id for b"ab"
    eos = len(toks)
    toks.append(b"")
    return toks, eos


def _over(alphabet: bytes, upto: int):
    return [bytes(p) for n in range(upto + 1) for p in itertools.product(alphabet, repeat=n)]


# (pattern, the candidate strings its sub-language is enumerated from)
PATTERNS = [
    (r"ab+c", _over(b"abc", 6)),
    (r"(true|false)", [b"true", b"false", b"tru", b"truefalse", b""]),
    (r"[a-c]{2,4}\d?", _over(b"ab12", 5)),
    (r'"\w+":\s*-?\d+(\.\d+)?', [b'"a":1', b'"ab": 12', b'"b1":-1.2', b'"a_":  12.12', b'"a":', b'"":1', b'"a":1.']),
    (r"(?:ab|b1)*12", _over(b"ab12", 6)),
    (r"[^a-z]x.\x41", [b"1x?A", b"Ax\x00A", b"\nxbA", b"\xffx\xffA", b"ax?A", b"1x\nA", b"1x?a"]),
    (r"a{3}", _over(b"a", 5)),
    (r"a{2,}b", _over(b"ab", 6)),
    (r"\d\D\s\S\w\W", [b"1a a1 ", b"9-\tx_!", b"11 a1 ", b"1a a11", b"1aaa1 "]),
    (r"\\\.\n\t", [b"\\.\n\t", b"\\a\n\t", b".\n\t"]),
    (r"(a|b1?)+c?", _over(b"ab1c", 5)),
    (r"[\d_-]+|\[x\]", _over(b"1_-[x]", 4)),
]


def language(pattern: str, candidates) -> list:
    """The candidates the pattern matches as a whole, by Python's re on bytes."""
    rx = re.compile(pattern.encode())
    return [s for s in candidates if rx.fullmatch(s)]


def tokenisations(s: bytes, token_bytes, skip=()) -> list:
    """Every token sequence over the vocabulary that decodes to `s`."""
    by = {}
    for t, b in enumerate(token_bytes):
        if b and t not in skip:
            by.setdefault(b, []).append(t)
    lens = sorted({len(b) for b in by})

    def go(at):
        if at == len(s):
            yield ()
            return
        for n in lens:
            for t in by.get(s[at: at + n], ()) if at + n <= len(s) else ():
                for rest in go(at + n):
                    yield (t,) + rest
    return list(go(0))


# ---------------------------------------------------------------------------
# the mask / advance passes' table

SLOTS, SCRATCH, G = 16, 15, 5
B = 12
MAX_CLASSES = 4096
CELLS = 2 * MAX_CLASSES + 300
ROW_A, ROW_B, ROW_C = 1, 3, 4  # guide rows in use: C = 1, C = 7, C = MAX_CLASSES; rows 0 and 2 hold garbage
# rows: off slot (3), scratch slot, out of range (16), one token (7), everything (0), every other token (12),
# one whole segment (5), both ends (9), a random half (1), a state at S (4), out of range (-1), slot 9 again
ROW_SLOTS = torch.tensor([3, SCRATCH, 16, 7, 0, 12, 5, 9, 1, 4, -1, 9], dtype=torch.int32)
UNTOUCHED = (0, 1, 2, 4, 9, 10)

_CASES = {}


def mask_case(V: int, Vp: int) -> dict:
    """CPU tensors of a 12-row case on 16 slots and three guides, built once
    per shape and left unchanged.  Random garbage fills whatever must not be
    read: the unused guide rows (classes, cells and dimensions), the cells
    past S * C, the classes of columns at or past V, the entries of unused
    slots.  keep[r]: the tokens row r may draw (None: the row is untouched)."""
    if (V, Vp) in _CASES:
        return _CASES[V, Vp]
    g = torch.Generator().manual_seed(V)
    i16 = lambda *shape: torch.randint(-2 ** 15, 2 ** 15, shape, generator=g, dtype=torch.int64).to(torch.int16)  # noqa: E731
    lg = torch.randn(B, Vp, generator=g) * 3
    gcls, gnext = i16(G, Vp), i16(G, CELLS)
    gdim = torch.randint(-5, 2 ** 20, (G, 2), generator=g, dtype=torch.int64).to(torch.int32)
    gsl = torch.randint(0, 2 ** 20, (SLOTS, 2), generator=g, dtype=torch.int64).to(torch.int32)
    gsl[:, 0] = -1
    gsl[SCRATCH] = torch.tensor([-1, 0], dtype=torch.int32)
    gsl[8] = torch.tensor([G, 0], dtype=torch.int32)  # unused slots: rows past the table, never looked at
    gsl[10] = torch.tensor([G + 7, 1], dtype=torch.int32)
    am = lg[:, :V].argmax(dim=1)
    seg = (V // 8) // 3
    one = (int(am[3]) + 1237) % V
    while one in (0, V - 1) or one // 8 == seg:
        one = (one + 1) % V
    tok = torch.arange(V)

    def cells(row, S, C, allowed):
        """next[S, C] of a guide row: a random state where allowed, -1 elsewhere."""
        nx = torch.randint(0, S, (S, C), generator=g, dtype=torch.int64).to(torch.int16)
        nx[~allowed] = -1
        gnext[row, : S * C] = nx.reshape(-1)
        gdim[row] = torch.tensor([S, C], dtype=torch.int32)
        return nx

    # guide A, C = 1: one class, drawable in state 0
    gcls[ROW_A, :V] = 0
    cells(ROW_A, 2, 1, torch.tensor([[True], [False]]))
    # guide B, C = 7: class 1 = one token, 2 = one whole segment, 3 = both ends, the rest spread over 0, 4, 5, 6;
    # state 0 allows class 1, state 1 class 2, state 2 class 3, state 3 everything
    cb = torch.tensor([0, 4, 5, 6])[torch.randint(0, 4, (V,), generator=g)]
    cb[8 * seg: 8 * seg + 8] = 2
    cb[0] = cb[V - 1] = 3
    cb[one] = 1
    gcls[ROW_B, :V] = cb.to(torch.int16)
    ab = torch.zeros(4, 7, dtype=torch.bool)
    ab[0, 1] = ab[1, 2] = ab[2, 3] = True
    ab[3] = True
    cells(ROW_B, 4, 7, ab)
    # guide C, C = MAX_CLASSES: class t mod C; state 0 allows the even classes -- every other token, every
    # segment mixed -- state 1 a random half of the classes
    cc = tok % MAX_CLASSES
    gcls[ROW_C, :V] = cc.to(torch.int16)
    ac = torch.zeros(2, MAX_CLASSES, dtype=torch.bool)
    ac[0, 0::2] = True
    ac[1] = torch.rand(MAX_CLASSES, generator=g) < 0.5
    cells(ROW_C, 2, MAX_CLASSES, ac)
    for slot, row, state in ((7, ROW_B, 0), (0, ROW_A, 0), (12, ROW_C, 0), (5, ROW_B, 1), (9, ROW_B, 2),
                             (1, ROW_C, 1), (4, ROW_B, 4)):  # slot 4: a state at S
        gsl[slot] = torch.tensor([row, state], dtype=torch.int32)
    keep = {3: cb == 1, 4: torch.ones(V, dtype=torch.bool), 5: tok % 2 == 0, 6: cb == 2, 7: cb == 3,
            8: ac[1][cc], 11: cb == 3}
    c = dict(lg=lg, tab=(gcls, gnext, gdim, gsl), slots=ROW_SLOTS, V=V, Vp=Vp, am=am, one=one, seg=seg, keep=keep)
    _CASES[V, Vp] = c
    return c


def counting_guide(V: int, counts=(1, 2, 5), seed: int = 0) -> tuple:
    """A guide whose state i allows exactly counts[i] tokens (class i + 1; the
    rest of the vocabulary is class 0, never drawable) and stays there.
    -> (TokenGuide, the allowed token lists)."""
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(V, generator=g).tolist()
    cls = np.zeros(V, dtype=np.int16)
    lists, at = [], 0
    for i, n in enumerate(counts):
        lists.append(sorted(perm[at: at + n]))
        cls[lists[-1]] = i + 1
        at += n
    nxt = np.full((len(counts), len(counts) + 1), -1, dtype=np.int16)
    for i in range(len(counts)):
        nxt[i, i + 1] = i
    return TokenGuide(cls, nxt, V), lists


def table_of(guides, Vp: int, slots: int, cells: int = 0) -> tuple:
    """The last stage's table holding `guides` in rows 0.., every slot off."""
    cells = cells or max(gd.S * gd.C for gd in guides)
    gcls = torch.zeros(len(guides), Vp, dtype=torch.int16)
    gnext = torch.zeros(len(guides), cells, dtype=torch.int16)
    gdim = torch.zeros(len(guides), 2, dtype=torch.int32)
    for r, gd in enumerate(guides):
        gcls[r, : gd.vocab] = torch.from_numpy(gd.cls)
        gnext[r, : gd.S * gd.C] = torch.from_numpy(np.ascontiguousarray(gd.next).reshape(-1))
        gdim[r] = torch.tensor([gd.S, gd.C], dtype=torch.int32)
    gsl = torch.zeros(slots, 2, dtype=torch.int32)
    gsl[:, 0] = -1
    return gcls, gnext, gdim, gsl
