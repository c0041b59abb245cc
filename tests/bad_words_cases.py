"""Cases of the bad-words pass shared by the CPU and the GPU tests: CPU tensors,
built once per shape and left unchanged, and the brute-force rule.

Tables are full of random junk wherever the pass must not look -- the end
offsets and tokens past a slot's count, the slots with cnt == 0, the context
past n -- so reading the wrong place changes the result.
"""
import numpy as np
import torch

INF = float("inf")
SLOTS, SCRATCH = 16, 15
L, N, T = 1024, 256, 2048


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def segmax_of(logits):
    """What linear_f32 writes beside these logits (padding columns included)."""
    n, Vp = logits.shape
    return logits.view(n, Vp // 8, 8).amax(-1).contiguous()


def brute_row(row, x, words, V):
    """The rule, literally: `row` a list of floats, `x` the context (prompt +
    generated tokens), `words` the sequences -> (the row, the banned tokens)."""
    row, banned = list(row), set()
    for w in words:
        m = len(w)
        if len(x) >= m - 1 and list(x[len(x) - m + 1:]) == list(w[:-1]) and 0 <= w[-1] < V:
            row[w[-1]] = -INF
            banned.add(w[-1])
    return row, banned


def brute(c, step="step"):
    """(logits, segmax) of the case by brute_row, row by row."""
    lg = c["lg"].clone()
    sm = segmax_of(c["lg"])
    cnt, end, tok = c["tab"]
    plen, ctok = c["ctx"][0], c["ctx"][3]
    Lc = ctok.shape[1]
    st = c[step] if step is not None else None
    for r, s in enumerate(c["slots"].tolist()):
        if not 0 <= s < cnt.shape[0]:
            continue
        n = max(0, min(int(plen[s]) + (int(st[r]) if st is not None else 0), Lc))
        ends = [0] + end[s, : int(cnt[s])].tolist()
        words = [tok[s, a:b].tolist() for a, b in zip(ends, ends[1:])]
        row, banned = brute_row(lg[r].tolist(), ctok[s, :n].tolist(), words, c["V"])
        lg[r] = torch.tensor(np.array(row, dtype=np.float32))
        for t in banned:
            sm[r, t // 8] = lg[r, t // 8 * 8: t // 8 * 8 + 8].max()
    return lg, sm


def _tables(g, V, slots=SLOTS, Lc=L, n=N, t=T):
    cnt = torch.zeros(slots, dtype=torch.int32)
    end = torch.randint(0, t, (slots, n), generator=g).to(torch.int32)
    tok = torch.randint(0, V, (slots, t), generator=g).to(torch.int32)
    plen = torch.randint(0, Lc, (slots,), generator=g).to(torch.int32)  # junk on slots nobody sets
    ctok = torch.randint(0, V, (slots, Lc), generator=g).to(torch.int32)
    ctx = (plen, torch.ones(slots), torch.zeros(slots, dtype=torch.int32), ctok)
    return (cnt, end, tok), ctx


def _put(tab, slot, words):
    cnt, end, tok = tab
    flat = [t for w in words for t in w]
    cnt[slot] = len(words)
    end[slot, : len(words)] = torch.tensor(np.cumsum([len(w) for w in words]), dtype=torch.int32)
    tok[slot, : len(flat)] = torch.tensor(flat, dtype=torch.int32)


_CASES = {}


def case(V, Vp):
    """14 rows on 16 slots; what each row is for stands beside it.  c["ban"]:
    row -> the tokens the pass bans there with the steps of c["step"]."""
    if (V, Vp) in _CASES:
        return _CASES[V, Vp]
    g = torch.Generator().manual_seed(V + 7)
    B = 14
    lg = torch.randn(B, Vp, generator=g) * 3
    tab, ctx = _tables(g, V)
    plen, ctok = ctx[0], ctx[3]
    am = lg[:, :V].argmax(dim=1).tolist()
    slots = torch.tensor([3, SCRATCH, 7, 0, 12, 5, 9, 1, 14, 14, 16, -1, 2, 4], dtype=torch.int32)
    step = torch.tensor([4, 0, 10, 0, 100, 3, 1, 2, 6, 9, 1, 1, 5, 3], dtype=torch.int64)
    ban = {}

    def x(slot, r):  # the context of the row
        return ctok[slot, : min(int(plen[slot]) + int(step[r]), L)].tolist()

    # rows 0, 1: cnt == 0 (the junk of their slots untouched), the second on the scratch slot
    plen[3], plen[SCRATCH] = 50, 0
    # row 2: lengths 1, 2 and 32, all matching; a 32-token sequence that differs in its first token
    plen[7] = 30
    c2 = x(7, 2)
    a, b, cc = (am[2] + 11) % V, (am[2] + 500) % V, (am[2] + 901) % V
    _put(tab, 7, [[a], [c2[-1], b], c2[-31:] + [cc], [(c2[-31] + 1) % V] + c2[-30:] + [(cc + 1) % V]])
    ban[2] = {a, b, cc}
    # row 3: a context of 2 tokens: shorter than a prefix of 4 (no ban, although the prefix ends with it), exactly
    # m - 2 (no ban, although the prefix starts with it), exactly m - 1 (ban)
    plen[0] = 2
    c3 = x(0, 3)
    _put(tab, 0, [[5, 6] + c3 + [41], c3 + [7, 42], c3 + [43], [c3[1], 44], [c3[0], 45]])
    ban[3] = {43, 44}
    # row 4: n = L: 1000 + 100 is clipped to the table's 1024 tokens
    plen[12] = 1000
    _put(tab, 12, [ctok[12, L - 2:].tolist() + [77], ctok[12, L - 3: L - 1].tolist() + [78]])
    ban[4] = {77}
    # row 5: two sequences banning one token; two banned tokens in one segment
    plen[5] = 9
    c5 = x(5, 5)
    d, e = (am[5] + 300) % V, 8 * ((am[5] // 8 + 9) % (V // 8))
    _put(tab, 5, [[d], [c5[-1], d], [e], c5[-2:] + [e + 3]])
    ban[5] = {d, e, e + 3}
    # row 6: the last token of the vocabulary, in the last, partly padded segment
    plen[9] = 4
    _put(tab, 9, [[x(9, 6)[-1], V - 1]])
    ban[6] = {V - 1}
    # row 7: a token whose logit is -inf already, and the row's argmax
    plen[1] = 20
    f = (am[7] + 77) % V
    lg[7, f] = -INF
    _put(tab, 1, [[f], [x(1, 7)[-1], am[7]]])
    ban[7] = {f, am[7]}
    # rows 8, 9: cnt == N on one slot, two rows at different steps; sequences of 1 to 3 tokens, every fourth planted
    # on the context of row 8, the next on that of row 9
    plen[14] = 100
    c8, c9 = x(14, 8), x(14, 9)
    words, ban[8], ban[9] = [], set(), set()
    for i in range(N):
        m = 1 + i % 3
        last = int(torch.randint(0, V, (1,), generator=g))
        if i % 4 == 0:
            words.append(c8[len(c8) - m + 1:] + [last])
            ban[8].add(last)
            if m == 1:
                ban[9].add(last)
        elif i % 4 == 1:
            words.append(c9[len(c9) - m + 1:] + [last])
            ban[9].add(last)
            if m == 1:
                ban[8].add(last)
        else:
            words.append([(c8[-1] + 1 + i) % V] * (m - 1) + [last] if m > 1 else [c8[-1], last])
    _put(tab, 14, words)
    for r, cx in ((8, c8), (9, c9)):  # random tokens can match by accident: the rule decides
        ban[r] = brute_row([0.0] * Vp, cx, words, V)[1]
    # rows 10, 11: slots outside the table
    # row 12: asking, nothing banned: prefixes that do not match, a matching one whose last token is a padding column
    # or negative
    plen[2] = 12
    c12 = x(2, 12)
    _put(tab, 2, [[(c12[-1] + 1) % V, 9], [c12[-2], (c12[-1] + 1) % V, 10], [c12[-1], Vp - 1 if Vp > V else V],
                  [c12[-1], -3], [c12[-1], V]])
    ban[12] = set()
    # row 13: one sequence matches at its step (n = 8), another at draw 0 (n = 5) only
    plen[4] = 5
    _put(tab, 4, [ctok[4, 6:8].tolist() + [90], ctok[4, 3:5].tolist() + [91]])
    ban[13] = {90} if ctok[4, 6:8].tolist() != ctok[4, 3:5].tolist() else {90, 91}
    c = dict(lg=lg, tab=tab, ctx=ctx, slots=slots, step=step, V=V, Vp=Vp, am=am, ban=ban, B=B)
    _CASES[V, Vp] = c
    return c


def random_case(V, Vp, B, seed=0):
    """B rows on B + 2 slots, a slot per row in random order: counts 1, 0, 3 or
    5; every second sequence planted on its row's context."""
    key = (V, Vp, B, seed)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(1000 * seed + B + V)
    Lc, n, t = 64, 8, 64
    lg = torch.randn(B, Vp, generator=g) * 3
    tab, ctx = _tables(g, V, B + 2, Lc, n, t)
    plen, ctok = ctx[0], ctx[3]
    slots = torch.randperm(B + 2, generator=g)[:B].to(torch.int32)
    step = torch.randint(0, 40, (B,), generator=g)
    for r, s in enumerate(slots.tolist()):
        k = (1, 0, 3, 5)[(r + seed) % 4]
        x = ctok[s, : min(int(plen[s]) + int(step[r]), Lc)].tolist()
        words = []
        for i in range(k):
            m = 1 + int(torch.randint(0, 6, (1,), generator=g))
            last = int(torch.randint(0, V, (1,), generator=g))
            pre = x[len(x) - m + 1:] if i % 2 == 0 and len(x) >= m - 1 else torch.randint(0, V, (m - 1,), generator=g).tolist()
            words.append(pre + [last])
        if words:
            _put(tab, s, words)
    c = dict(lg=lg, tab=tab, ctx=ctx, slots=slots, step=step, V=V, Vp=Vp, B=B)
    _CASES[key] = c
    return c


def big_case():
    """One row whose context fills the largest table, L = n = 8192, and a
    neighbour with cnt == 0."""
    if "big" in _CASES:
        return _CASES["big"]
    V, Vp, Lc = 1000, 1024, 8192
    g = torch.Generator().manual_seed(5)
    lg = torch.randn(2, Vp, generator=g) * 3
    tab, ctx = _tables(g, V, 4, Lc, 4, 64)
    ctx[0][2], ctx[0][1] = 8000, 10
    tail = ctx[3][2, Lc - 31:].tolist()
    am = int(lg[0, :V].argmax())
    _put(tab, 2, [tail + [am], tail[-1:] + [3], [(tail[-1] + 1) % V, 4]])
    c = dict(lg=lg, tab=tab, ctx=ctx, slots=torch.tensor([2, 1], dtype=torch.int32),
             step=torch.tensor([200, 0], dtype=torch.int64), V=V, Vp=Vp, am=am, B=2)
    _CASES["big"] = c
    return c
