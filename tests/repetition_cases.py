"""Shared by tests/test_repetition.py (CPU) and tests/test_repetition_gpu.py:
the 12-row case the repetition pass is checked on, and a brute-force
implementation of the two rules on Python lists -- HF's formulas, written
without torch indexing, independent of ops/reference.py.
"""
import numpy as np
import torch

SLOTS, SCRATCH = 16, 15
INF = float("inf")


def brute_row(logits, ctx, r, G, V):
    """One row: `logits` a list of np.float32, `ctx` the list of context ids
    (prompt + generated).  -> (new list, set of rewritten tokens)."""
    out = list(logits)
    touched = set()
    r32 = np.float32(r)
    if r32 != np.float32(1.0):
        for t in set(ctx):
            if 0 <= t < V:
                l = np.float32(out[t])
                out[t] = l * r32 if l < 0 else l / r32  # np.float32 op np.float32: one rounding
                touched.add(t)
    n = len(ctx)
    if G > 0 and n >= G - 1:
        tail = ctx[n - G + 1:]
        for i in range(0, n - G + 1):
            if ctx[i: i + G - 1] == tail:
                t = ctx[i + G - 1]
                if 0 <= t < V:
                    out[t] = np.float32(-INF)
                    touched.add(t)
    return out, touched


def brute(logits, table, slots, step, V, segmax=None):
    """ops/reference.py repetition's contract on lists -> (logits, segmax or
    None) as new tensors."""
    plen, rpen, ngram, tok = (t.tolist() for t in table)
    L = len(tok[0])
    rows, segs = [], []
    with np.errstate(all="ignore"):
        for i, s in enumerate(slots.tolist()):
            row = [np.float32(v) for v in logits[i].tolist()]
            sm = None if segmax is None else [np.float32(v) for v in segmax[i].tolist()]
            if 0 <= s < len(plen) and (np.float32(rpen[s]) != 1 or ngram[s] > 0):
                c = int(step[i]) if step is not None else 0
                n = max(0, min(plen[s] + c, L))
                row, touched = brute_row(row, tok[s][:n], rpen[s], ngram[s], V)
                if sm is not None:
                    for g in {t // 8 for t in touched}:
                        sm[g] = max(row[8 * g: 8 * g + 8])
            rows.append(row)
            segs.append(sm)
    out = torch.tensor(np.array(rows, dtype=np.float32))
    return out, None if segmax is None else torch.tensor(np.array(segs, dtype=np.float32))


def segmax_of(logits):
    """What linear_f32 writes beside these logits (padding columns included)."""
    B, Vp = logits.shape
    return logits.view(B, Vp // 8, 8).amax(-1).contiguous()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def case(V, Vp, L=1024):
    """CPU tensors of a 12-row case on 16 slots.  The table is full of valid
    tokens everywhere (other slots, positions at or past each n) and of live
    knobs on the slots no row uses, so reading anything but the row's own
    context changes the result."""
    g = torch.Generator().manual_seed(V + L)
    B = 12
    lg = torch.randn(B, Vp, generator=g) * 3
    plen = torch.zeros(SLOTS, dtype=torch.int32)
    rpen = torch.full((SLOTS,), 1.7)
    ngram = torch.full((SLOTS,), 2, dtype=torch.int32)
    tok = torch.randint(0, V, (SLOTS, L), generator=g, dtype=torch.int32)
    slots = torch.tensor([3, SCRATCH, 7, 0, 12, 9, 5, 1, 14, 11, 6, 2], dtype=torch.int32)
    step = torch.zeros(B, dtype=torch.int64)
    am = lg[:, :V].argmax(dim=1)

    def put(row, n, c, r, G, ctx=None):
        """Row `row`: n context tokens of which c generated, knobs r / G."""
        s = int(slots[row])
        plen[s], rpen[s], ngram[s], step[row] = n - c, r, G, c
        if ctx is not None:
            tok[s, : len(ctx)] = torch.as_tensor(ctx, dtype=torch.int32)

    def rand(n, hi=None):
        return torch.randint(0, hi or V, (n,), generator=g).tolist()

    put(0, 200, 4, 1.0, 0)                          # row 0: both knobs off
    put(1, 0, 0, 1.0, 0)                            # row 1: a pad row on the scratch slot
    step[1] = 9
    put(2, 1, 0, 1.3, 0)                            # row 2: r only, n = 1
    put(3, 300, 37, 1.2, 0, rand(300, 120))         # row 3: r only, n = 300 with duplicates (120 distinct at most)
    put(4, L, 5, 0.8, 0)                            # row 4: r only, n = L
    seg5 = 77  # row 5: r < 1 lifts the segment's smallest (negative) logit over its maximum
    lg[5, seg5 * 8: seg5 * 8 + 8] = -1.0 - 4.0 * torch.rand(8, generator=g)
    tok5 = seg5 * 8 + int(lg[5, seg5 * 8: seg5 * 8 + 8].argmin())
    put(5, 3, 1, 0.01, 0, [tok5, 0, tok5])
    ctx6 = rand(40)                                 # row 6: G = 1, and ids outside [0, V)
    ctx6[3], ctx6[17], ctx6[30], ctx6[39] = -1, V, V + 7, 2 ** 31 - 1
    put(6, 40, 11, 1.0, 1, ctx6)
    ctx7 = rand(200)                                # row 7: G = 2, the argmax banned: its segment maximum falls
    ctx7[50], ctx7[51] = ctx7[-1], int(am[7])
    put(7, 200, 60, 1.0, 2, ctx7)
    ctx8 = rand(150, 40)                            # row 8: G = 3 and r: tokens both penalised and banned
    ctx8[10:13] = [ctx8[-2], ctx8[-1], 33]
    put(8, 150, 149, 1.3, 3, ctx8)
    ctx9 = rand(500)                                # row 9: G = 32, one earlier occurrence of the 31-token tail
    ctx9[100:131] = ctx9[-31:]
    ctx9[131] = V - 1
    put(9, 500, 250, 1.0, 32, ctx9)
    put(10, 3, 2, 1.0, 5)                           # row 10: n = G - 2: no tail, nothing banned
    ctx11 = [16, 17, 18]                            # row 11: n = G - 1: a tail, no start position; 0.0, -0.0, -inf
    lg[11, 16], lg[11, 17], lg[11, 18] = 0.0, -0.0, -INF
    put(11, 3, 0, 2.5, 4, ctx11)
    return dict(lg=lg, tab=(plen, rpen, ngram, tok), slots=slots, step=step, V=V, L=L, am=am, seg5=seg5, tok5=tok5,
                ctx={6: ctx6, 7: ctx7, 8: ctx8, 9: ctx9})


def big_case(V=50257, Vp=50304, L=8192):
    """The largest LDS key set: one slot whose context fills L = 8192, both
    rules on (mostly distinct tokens: the set is half full), beside a default
    row."""
    g = torch.Generator().manual_seed(L)
    lg = torch.randn(2, Vp, generator=g) * 3
    tok = torch.randint(0, V, (2, L), generator=g, dtype=torch.int32)
    tok[0, 4000:4002] = tok[0, -2:]
    tok[0, 4002] = int(lg[0, :V].argmax())
    tab = (torch.tensor([L - 100, 50], dtype=torch.int32), torch.tensor([1.25, 1.0]),
           torch.tensor([3, 0], dtype=torch.int32), tok)
    return dict(lg=lg, tab=tab, slots=torch.tensor([0, 1], dtype=torch.int32),
                step=torch.tensor([100, 7], dtype=torch.int64), V=V, L=L)
