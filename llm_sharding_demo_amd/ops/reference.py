"""Pure-PyTorch reference implementations of every op the engine uses.

These are the *semantics* the hand-written HIP kernels in `csrc/kernels/`
must reproduce; they also run the whole engine on CPU (tests, golden
numerics).  They compute in fp32 regardless of input dtype.

Op semantics follow HF GPT-2, which the reference delegates to
(`/root/reference/server.py:79-102`; [tf5.15] models/gpt2/modeling_gpt2.py):
  * LayerNorm eps 1e-5, affine (K4)
  * Conv1D = x @ W + b, with W stored [in, out] by HF; we store W^T [out, in]
  * gelu_new = tanh-approximation GELU (K11, [tf5.15] activations.py:59-66)
  * causal softmax(QK^T / sqrt(hd)) V (K7) -- the causal mask is explicit here
    (the reference gets causality only implicitly through SDPA, quirk Q3).
Llama ops (RMSNorm, RoPE, SwiGLU, GQA) follow [tf5.15] models/llama.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F

_GELU_C = math.sqrt(2.0 / math.pi)


def gelu_new(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * (1.0 + torch.tanh(_GELU_C * (x + 0.044715 * torch.pow(x, 3.0))))


def embed(ids: torch.Tensor, pos: torch.Tensor, wte: torch.Tensor,
          wpe: Optional[torch.Tensor]) -> torch.Tensor:
    """x[t] = wte[ids[t]] + wpe[pos[t]]  -> fp32 [T, H]."""
    x = wte.index_select(0, ids.long()).float()
    if wpe is not None:
        x = x + wpe.index_select(0, pos.long()).float()
    return x


def layernorm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float) -> torch.Tensor:
    return F.layer_norm(x.float(), (x.shape[-1],), w.float(), b.float(), eps)


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    var = xf.pow(2).mean(-1, keepdim=True)
    return xf * torch.rsqrt(var + eps) * w.float()


def linear(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a [T, K] @ w[N, K]^T (+ bias) in fp32."""
    out = a.float() @ w.float().t()
    if bias is not None:
        out = out + bias.float()
    return out


def silu_mul(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    g = gate.float()
    return g * torch.sigmoid(g) * up.float()


def rope_cos_sin(pos: torch.Tensor, head_dim: int, theta: float):
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    ang = pos.double()[:, None] * inv[None, :]
    return ang.cos().float(), ang.sin().float()  # [T, hd/2]


def apply_rope(x: torch.Tensor, pos: torch.Tensor, theta: float) -> torch.Tensor:
    """HF rotate_half convention: pairs (i, i + hd/2).  x: [T, nh, hd]."""
    hd = x.shape[-1]
    cos, sin = rope_cos_sin(pos.to(torch.float64), hd, theta)
    cos = cos.to(x.device)[:, None, :]
    sin = sin.to(x.device)[:, None, :]
    x1, x2 = x[..., : hd // 2].float(), x[..., hd // 2:].float()
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


def kv_append(k_cache: torch.Tensor, v_cache: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
              slots: torch.Tensor, pos: torch.Tensor) -> None:
    """Cache layout [slots, n_kv, max_seq, hd]; k, v: [T, n_kv, hd]."""
    s, p = slots.long(), pos.long()
    k_cache[s, :, p, :] = k.to(k_cache.dtype)
    v_cache[s, :, p, :] = v.to(v_cache.dtype)


def attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
              seq_slots: torch.Tensor, q_start: torch.Tensor, cu_q: torch.Tensor) -> torch.Tensor:
    """Causal attention of packed queries over the KV cache.

    q: [T, nh, hd] packed; sequence i owns rows cu_q[i]:cu_q[i+1], whose
    positions are q_start[i] + j.  Keys/values for sequence i live at
    k_cache[seq_slots[i], :, 0:q_start[i]+len_i].  GQA: nh % n_kv == 0.
    Returns fp32 [T, nh, hd]; fp64 when q is fp64 (the tests' high-precision
    reference).
    """
    nh, hd = q.shape[1], q.shape[2]
    n_kv = k_cache.shape[1]
    grp = nh // n_kv
    dt = torch.float64 if q.dtype == torch.float64 else torch.float32
    out = torch.empty(q.shape, dtype=dt, device=q.device)
    scale = 1.0 / math.sqrt(hd)
    for i in range(seq_slots.numel()):
        a, b = int(cu_q[i]), int(cu_q[i + 1])
        if b == a:
            continue
        st = int(q_start[i])
        L = st + (b - a)
        s = int(seq_slots[i])
        kk = k_cache[s, :, :L].to(dt).repeat_interleave(grp, dim=0)  # [nh, L, hd]
        vv = v_cache[s, :, :L].to(dt).repeat_interleave(grp, dim=0)
        qq = q[a:b].to(dt).transpose(0, 1)  # [nh, Lq, hd]
        sc = torch.matmul(qq, kk.transpose(1, 2)) * scale  # [nh, Lq, L]
        qpos = torch.arange(st, L, device=q.device)[:, None]
        kpos = torch.arange(L, device=q.device)[None, :]
        sc = sc.masked_fill(kpos > qpos, float("-inf"))
        p = torch.softmax(sc, dim=-1)
        out[a:b] = torch.matmul(p, vv).transpose(0, 1)
    return out


def penalize(logits: torch.Tensor, hist: torch.Tensor, slots: torch.Tensor, counts: torch.Tensor,
             presence: torch.Tensor, frequency: torch.Tensor, vocab: int,
             segmax: Optional[torch.Tensor] = None):
    """Presence / frequency penalties over the tokens a row has generated
    (OpenAI / vLLM rule; the prompt does not count), ahead of `sample`.

    hist [slots, L] int: hist[s, j] = the j-th generated token of the sequence
    on KV slot s; row r reads hist[slots[r], 0 .. counts[r]).  With c(t) the
    occurrences of token t in there, every t with c(t) > 0 gets
        logit[t] <- logit[t] - (presence[r] + frequency[r] * float(c(t)))
    in fp32, three roundings (product, sum, difference).  Rows whose two
    penalties are both 0, or whose history is empty, are untouched; history
    entries outside [0, vocab) are ignored.

    fp32 `logits` [B, >= vocab] are rewritten in place and returned.  With
    `segmax` [B, width / 8] (linear_f32's 8-logit segment maxima, padding
    columns included) the maxima of the touched segments are recomputed in
    place too, and (logits, segmax) is returned.
    """
    assert logits.dtype == torch.float32, "penalize rewrites fp32 logits in place"
    B, L = logits.shape[0], hist.shape[1]
    for r in range(B):
        p, f = presence[r].float(), frequency[r].float()
        n = min(int(counts[r]), L)
        if (float(p) == 0.0 and float(f) == 0.0) or n <= 0:
            continue
        h = hist[int(slots[r]), :n].long()
        toks, cnt = torch.unique(h[(h >= 0) & (h < vocab)], return_counts=True)
        if toks.numel() == 0:
            continue
        pen = p + f * cnt.to(torch.float32)  # two roundings: the product, then the sum
        logits[r, toks] = logits[r, toks] - pen
        if segmax is not None:
            segs = torch.unique(toks // 8)
            idx = segs[:, None] * 8 + torch.arange(8)
            segmax[r, segs] = logits[r][idx].max(dim=1).values
    return logits if segmax is None else (logits, segmax)


def logit_edits(logits: torch.Tensor, table, slots: torch.Tensor, step: Optional[torch.Tensor], vocab: int,
                segmax: Optional[torch.Tensor] = None):
    """Per-request logit edits (logit_bias, banned tokens, min_new_tokens),
    after `penalize` and ahead of `sample`.

    table = (cnt [slots] int, tok [slots, E] int, val [slots, E] fp32, until
    [slots, E] int): row r reads entries [0, cnt[s]) of its KV slot s =
    slots[r], sorted by token.  With c = step[r], the row's sampler counter
    before the draw (step None: c = 0, the prefill draw), every entry with
    c < until is active and does
        logit[tok] <- logit[tok] + val
    in fp32, one rounding per addition, the entries of one token in table
    order (a ban is val = -inf; a permanent entry has until = INT32_MAX).
    Rows whose slot has no entry are untouched, as is a token none of whose
    entries is active; entries with a token outside [0, vocab) are ignored.

    fp32 `logits` [B, >= vocab] are rewritten in place and returned.  With
    `segmax` [B, width / 8] (linear_f32's 8-logit segment maxima, padding
    columns included) the maximum of every segment holding an edited token is
    recomputed from its 8 stored logits in place too, and (logits, segmax) is
    returned.
    """
    assert logits.dtype == torch.float32, "logit_edits rewrites fp32 logits in place"
    cnt, tok, val, until = table
    E = tok.shape[1]
    for r in range(logits.shape[0]):
        s = int(slots[r])
        if not 0 <= s < cnt.shape[0]:
            continue
        n = min(int(cnt[s]), E)
        c = int(step[r]) if step is not None else 0
        touched = []
        for e in range(n):
            t = int(tok[s, e])
            if not (0 <= t < vocab and c < int(until[s, e])):
                continue
            logits[r, t] = logits[r, t] + val[s, e].float()  # fp32 + fp32: one rounding
            touched.append(t // 8)
        if segmax is not None and touched:
            segs = torch.unique(torch.tensor(touched))
            idx = segs[:, None] * 8 + torch.arange(8)
            segmax[r, segs] = logits[r][idx].max(dim=1).values
    return logits if segmax is None else (logits, segmax)


def allow_mask(logits: torch.Tensor, table, slots: torch.Tensor, vocab: int,
               segmax: Optional[torch.Tensor] = None):
    """Per-request allowed_token_ids: a vocabulary bitmask, after `repetition`,
    `penalize` and `logit_edits` and ahead of `sample` and `logprobs`.

    table = (on [slots] int32, bits [slots, W] int32), W >= ceil(width / 32)
    for logits of `width` columns: token t is allowed when bit t & 31 of word
    t >> 5 is set.  Row r reads its KV slot s = slots[r]: a slot outside
    [0, slots) or with on[s] == 0 leaves the row untouched, whatever its bits
    hold; otherwise every t in [0, vocab) with a clear bit gets
        logit[t] <- -inf
    a pure select: every other logit keeps its bits.  Columns at or past
    `vocab` are never written, whatever their bits.

    fp32 `logits` [B, >= vocab] are rewritten in place and returned.  With
    `segmax` [B, width / 8] (linear_f32's 8-logit segment maxima, padding
    columns included) every segment that holds a cleared t < vocab is
    recomputed as the maximum of its 8 stored logits, in place too -- every
    other segment is left as it is -- and (logits, segmax) is returned.
    """
    assert logits.dtype == torch.float32, "allow_mask rewrites fp32 logits in place"
    on, bits = table
    width, dev = logits.shape[1], logits.device
    assert bits.shape[1] * 32 >= width and vocab <= width
    t = torch.arange(vocab, device=dev)
    for r in range(logits.shape[0]):
        s = int(slots[r])
        if not 0 <= s < on.shape[0] or int(on[s]) == 0:
            continue
        clear = ((bits[s].to(dev)[t >> 5] >> (t & 31)) & 1) == 0
        logits[r, :vocab] = torch.where(clear, torch.full_like(logits[r, :vocab], -math.inf), logits[r, :vocab])
        if segmax is not None:
            segs = torch.unique(t[clear] >> 3)
            if segs.numel():
                idx = segs[:, None] * 8 + torch.arange(8, device=dev)
                segmax[r, segs] = logits[r][idx].max(dim=1).values
    return logits if segmax is None else (logits, segmax)


def repetition(logits: torch.Tensor, table, slots: torch.Tensor, step: Optional[torch.Tensor], vocab: int,
               segmax: Optional[torch.Tensor] = None):
    """HF-style repetition_penalty and no_repeat_ngram_size over prompt +
    generated tokens, ahead of `penalize`, `logit_edits` and `sample`.

    table = (plen [slots] int, rpen [slots] fp32, ngram [slots] int, tok
    [slots, L] int): the context of the sequence on KV slot s is x =
    tok[s, 0 .. n), its prompt followed by its generated tokens, with n =
    min(plen[s] + c, L) and c = step[r], the row's sampler counter before the
    draw (step None: c = 0, the prefill draw).  With r = rpen[s], G = ngram[s]:

      1. r != 1: every distinct token t of x in [0, vocab) is rewritten once,
         logit[t] <- logit[t] * r if logit[t] < 0 else logit[t] / r, in fp32
         with one rounding (IEEE division; -0.0 and -inf stay what they are);
      2. G > 0 and n >= G - 1: with tail = x[n - G + 1 .. n), every i in
         [0, n - G] with x[i .. i + G - 1) == tail (raw ids) bans the token
         that followed, logit[x[i + G - 1]] <- -inf when it is in [0, vocab);
         G = 1 bans every context token.  Bans come after the penalty.

    Rows whose slot has r == 1 and G == 0 are untouched.  fp32 `logits`
    [B, >= vocab] are rewritten in place and returned.  With `segmax`
    [B, width / 8] (linear_f32's 8-logit segment maxima, padding columns
    included) the maximum of every segment holding a rewritten token is
    recomputed from its 8 stored logits in place too, and (logits, segmax) is
    returned.
    """
    assert logits.dtype == torch.float32, "repetition rewrites fp32 logits in place"
    plen, rpen, ngram, tok = table
    L = tok.shape[1]
    for r in range(logits.shape[0]):
        s = int(slots[r])
        if not 0 <= s < plen.shape[0]:
            continue
        rp, G = rpen[s].float(), min(int(ngram[s]), 32)  # 32: the largest n-gram (SamplingParams.validate)
        if float(rp) == 1.0 and G <= 0:
            continue
        c = int(step[r]) if step is not None else 0
        n = max(0, min(int(plen[s]) + c, L))
        x = tok[s, :n].long()
        touched = []
        if float(rp) != 1.0:
            toks = torch.unique(x[(x >= 0) & (x < vocab)])
            if toks.numel():
                l = logits[r, toks]
                logits[r, toks] = torch.where(l < 0, l * rp, l / rp)  # fp32 op fp32: one rounding
                touched.append(toks)
        if G > 0 and n >= G:
            win = x.unfold(0, G, 1)  # [n - G + 1, G]: x[i .. i + G)
            hit = (win[:, :G - 1] == x[n - G + 1:]).all(dim=1)
            ban = torch.unique(win[hit, G - 1])
            ban = ban[(ban >= 0) & (ban < vocab)]
            if ban.numel():
                logits[r, ban] = float("-inf")
                touched.append(ban)
        if segmax is not None and touched:
            segs = torch.unique(torch.cat(touched) // 8)
            idx = segs[:, None] * 8 + torch.arange(8)
            segmax[r, segs] = logits[r][idx].max(dim=1).values
    return logits if segmax is None else (logits, segmax)


def bad_words(logits: torch.Tensor, table, ctx_table, slots: torch.Tensor, step: Optional[torch.Tensor], vocab: int,
              segmax: Optional[torch.Tensor] = None):
    """Per-request bad_words (HF bad_words_ids): token sequences that may never
    be completed, right after `repetition` and ahead of `penalize`,
    `logit_edits`, `allow_mask` and `sample`.

    table = (cnt [slots] int, end [slots, N] int, tok [slots, T] int): the
    sequence e < min(cnt[s], N) of KV slot s is w = tok[s, end[s, e - 1] ..
    end[s, e]) (end[s, -1] = 0), m = len(w) tokens.  ctx_table is `repetition`'s
    table, of which plen and tok are read: the context of row r on slot s =
    slots[r] is x = tok[s, 0 .. n), n = min(plen[s] + c, L), c = step[r], the
    row's sampler counter before the draw (step None: c = 0, the prefill
    draw).  Every sequence with m - 1 <= n and x[n - m + 1 .. n) == w[: m - 1]
    (raw ids; m = 1: always) does
        logit[w[m - 1]] <- -inf
    when that token is in [0, vocab): a pure store, every other logit keeps its
    bits.  A sequence whose offsets do not describe 1 to 32 tokens inside the
    row is skipped.  Rows whose slot is outside the table or has cnt == 0 are
    untouched.

    fp32 `logits` [B, >= vocab] are rewritten in place and returned.  With
    `segmax` [B, width / 8] (linear_f32's 8-logit segment maxima, padding
    columns included) the maximum of every segment holding a banned token is
    recomputed from its 8 stored logits in place too, and (logits, segmax) is
    returned.
    """
    assert logits.dtype == torch.float32, "bad_words rewrites fp32 logits in place"
    cnt, end, tok = table
    plen, ctok = ctx_table[0], ctx_table[3]
    N, T, L = end.shape[1], tok.shape[1], ctok.shape[1]
    for r in range(logits.shape[0]):
        s = int(slots[r])
        if not 0 <= s < cnt.shape[0] or int(cnt[s]) <= 0:
            continue
        c = int(step[r]) if step is not None else 0
        n = max(0, min(int(plen[s]) + c, L))
        x = ctok[s, max(0, n - 31): n].tolist()
        ends, banned = [0] + end[s, : min(int(cnt[s]), N)].tolist(), []
        for b, e in zip(ends, ends[1:]):
            m = e - b
            if b < 0 or e > T or not 1 <= m <= 32 or m - 1 > n:
                continue
            w = tok[s, b:e].tolist()
            if x[len(x) - (m - 1):] == w[:-1] and 0 <= w[-1] < vocab:
                banned.append(w[-1])
        if banned:
            ban = torch.unique(torch.tensor(banned))
            logits[r, ban] = float("-inf")
            if segmax is not None:
                segs = torch.unique(ban // 8)
                idx = segs[:, None] * 8 + torch.arange(8)
                segmax[r, segs] = logits[r][idx].max(dim=1).values
    return logits if segmax is None else (logits, segmax)


def record_context(table, slots: torch.Tensor, step: Optional[torch.Tensor], tokens: torch.Tensor,
                   active: Optional[torch.Tensor] = None, back: int = 0) -> None:
    """tok[slots[i], plen[slots[i]] + step[i] - back] = tokens[i] for active
    rows (all rows when `active` is None), table as in `repetition`; step
    None = the prefill draw, right behind the prompt.  back = 1 when the
    sampler counters were already advanced past the draw.  Positions outside
    [0, L) and slots outside the table are dropped."""
    plen, _, _, tok = table
    for i in range(tokens.shape[0]):
        if active is not None and int(active[i]) == 0:
            continue
        s = int(slots[i])
        if not 0 <= s < tok.shape[0]:
            continue
        j = int(plen[s]) + (int(step[i]) - back if step is not None else 0)
        if 0 <= j < tok.shape[1]:
            tok[s, j] = int(tokens[i])


def _guide_state(table, s: int) -> Optional[tuple]:
    """(guide row g, state, S, C) of KV slot `s` when the guide passes act on
    it: the slot lies in the table, g in [0, G), the state in [0, S) and its
    row of C cells, 1 <= C <= 4096 (the classes the mask kernel's LDS flags
    hold), within the row's max_cells; None otherwise."""
    gcls, gnext, gdim, gsl = table
    if not 0 <= s < gsl.shape[0]:
        return None
    g, st = int(gsl[s, 0]), int(gsl[s, 1])
    if not 0 <= g < gcls.shape[0]:
        return None
    S, C = int(gdim[g, 0]), int(gdim[g, 1])
    if st < 0 or st >= S or not 1 <= C <= 4096 or (st + 1) * C > gnext.shape[1]:
        return None
    return g, st, S, C


def guide_mask(logits: torch.Tensor, table, slots: torch.Tensor, vocab: int,
               segmax: Optional[torch.Tensor] = None):
    """Per-request guided decoding, the mask: after `allow_mask`, the last edit
    ahead of `sample` and `logprobs`.

    table = (gcls [G, Vp] int16, gnext [G, max_cells] int16, gdim [G, 2] int32,
    gsl [slots, 2] int32): guide row g holds a TokenGuide -- the class of every
    logits column, its next[S, C] row-major, (S, C) -- and gsl[s] = (the guide
    row of KV slot s or -1, its current state).  Row r reads (g, state) of its
    slot s = slots[r]; a slot outside the table, g outside [0, G), a state
    outside [0, S) or a state row that does not fit max_cells leaves the row
    untouched, whatever the tables hold.  Otherwise every t in [0, vocab)
    whose class c = gcls[g, t] is outside [0, C) or has gnext[g, state * C +
    c] < 0 gets
        logit[t] <- -inf
    a pure select: every other logit keeps its bits.  Columns at or past
    `vocab` are never written and their classes never matter.  The tables are
    only read.

    fp32 `logits` [B, >= vocab] are rewritten in place and returned; `segmax`
    as in `allow_mask`: every 8-logit segment that holds a cleared t < vocab is
    recomputed as the maximum of its 8 stored logits, padding columns included.
    """
    assert logits.dtype == torch.float32, "guide_mask rewrites fp32 logits in place"
    gcls, gnext, gdim, gsl = table
    width, dev = logits.shape[1], logits.device
    assert vocab <= width <= gcls.shape[1]
    t = torch.arange(vocab, device=dev)
    for r in range(logits.shape[0]):
        st = _guide_state(table, int(slots[r]))
        if st is None:
            continue
        g, s, _, C = st
        c = gcls[g, :vocab].to(dev).long()
        inside = (c >= 0) & (c < C)
        cell = gnext[g].to(dev)[(s * C + c.clamp(0, C - 1)).clamp(0, gnext.shape[1] - 1)]
        clear = ~(inside & (cell >= 0))
        logits[r, :vocab] = torch.where(clear, torch.full_like(logits[r, :vocab], -math.inf), logits[r, :vocab])
        if segmax is not None:
            segs = torch.unique(t[clear] >> 3)
            if segs.numel():
                idx = segs[:, None] * 8 + torch.arange(8, device=dev)
                segmax[r, segs] = logits[r][idx].max(dim=1).values
    return logits if segmax is None else (logits, segmax)


def guide_advance(table, slots: torch.Tensor, tokens: torch.Tensor, vocab: int,
                  active: Optional[torch.Tensor] = None) -> None:
    """Guided decoding, the step behind the draw: for every active row (all
    rows when `active` is None) whose slot holds a valid (g, state) -- as
    `guide_mask` decides -- and whose token lies in [0, vocab), with a class c
    = gcls[g, token] in [0, C):
        gsl[slot].state <- gnext[g, state * C + c]
    (-1 once the guide is dead: the mask pass then leaves the row alone).
    Everything else is left as it is.  Each row owns its slot."""
    gcls, gnext, _, gsl = table
    new = []
    for i in range(tokens.shape[0]):
        if active is not None and int(active[i]) == 0:
            continue
        s, tok = int(slots[i]), int(tokens[i])
        st = _guide_state(table, s)
        if st is None or not 0 <= tok < vocab:
            continue
        g, cur, _, C = st
        c = int(gcls[g, tok])
        if 0 <= c < C:
            new.append((s, int(gnext[g, cur * C + c])))
    for s, v in new:
        gsl[s, 1] = v


def record_tokens(hist: torch.Tensor, slots: torch.Tensor, step: Optional[torch.Tensor], tokens: torch.Tensor,
                  active: Optional[torch.Tensor] = None, back: int = 0) -> None:
    """hist[slots[i], step[i] - back] = tokens[i] for active rows (all rows
    when `active` is None); step None = entry 0, the prefill draw.  back = 1
    when the sampler counters were already advanced past the draw."""
    for i in range(tokens.shape[0]):
        if active is not None and int(active[i]) == 0:
            continue
        j = int(step[i]) - back if step is not None else 0
        if 0 <= j < hist.shape[1]:
            hist[int(slots[i]), j] = int(tokens[i])


def lse64(row: torch.Tensor) -> torch.Tensor:
    """m + log(sum exp(x - m)) of one row in float64, m its maximum (-inf for
    a row of -inf)."""
    x = row.double()
    m = x.max()
    if float(m) == float("-inf"):
        return m
    return m + torch.log(torch.exp(x - m).sum())


def logprobs(logits: torch.Tensor, tokens: torch.Tensor, nlp, vocab: int, W: int):
    """Token logprobs and top-N alternatives of fp32 logit rows [B, >= vocab].

    Over [0, vocab) of each row: lse = m + log(sum exp(x - m)) with m the row
    maximum, the sum taken in float64 and lse rounded once to fp32; the
    logprob of x is fl32(x - lse), -inf for x = -inf (-inf entries add 0 to
    the sum).  Row r with n = min(nlp[r], W) >= 0 gets its n most likely ids
    and their logprobs in the sampler's contract order -- logit descending by
    numeric comparison (-0.0 == +0.0), index ascending: a stable sort -- and
    entries [n, W), or past the vocabulary, hold id -1 and -inf.  Rows with
    nlp < 0 did not ask: logprob -inf and a padded record.

    -> (tok_lp [B] fp32, top_id [B, W] int32, top_lp [B, W] fp32), tok_lp the
    logprob of tokens[r]: bit-equal to its entry among the alternatives.
    """
    B = logits.shape[0]
    tok_lp = torch.full((B,), float("-inf"), dtype=torch.float32)
    top_id = torch.full((B, W), -1, dtype=torch.int32)
    top_lp = torch.full((B, W), float("-inf"), dtype=torch.float32)
    neg = torch.tensor(float("-inf"))
    for r in range(B):
        n = int(nlp[r])
        if n < 0:
            continue
        n = min(n, W)
        row = logits[r, :vocab].detach().float().cpu()
        lse = lse64(row).float()
        lp = torch.where(row == neg, neg, row - lse)
        t = int(tokens[r])
        if 0 <= t < vocab:
            tok_lp[r] = lp[t]
        if n:
            _, idx = torch.sort(row, descending=True, stable=True)
            idx = idx[:n]
            top_id[r, : idx.numel()] = idx.to(torch.int32)
            top_lp[r, : idx.numel()] = lp[idx]
    return tok_lp, top_id, top_lp


def record_logprobs(rec, slots: torch.Tensor, step: Optional[torch.Tensor], nlp, tok_lp, top_id, top_lp,
                    active: Optional[torch.Tensor] = None, back: int = 0) -> None:
    """Store `logprobs` results of the rows with nlp >= 0 as record
    step[i] - back (step None = 0, the prefill draw) of KV slot slots[i] in
    rec = (lp_tok [slots, L], lp_top_id [slots, L, W], lp_top [slots, L, W]);
    inactive rows, and records outside [0, L), are skipped."""
    lt, li, lv = rec
    for i in range(tok_lp.shape[0]):
        if int(nlp[i]) < 0 or (active is not None and int(active[i]) == 0):
            continue
        j = int(step[i]) - back if step is not None else 0
        s = int(slots[i])
        if 0 <= j < lt.shape[1] and 0 <= s < lt.shape[0]:
            lt[s, j] = tok_lp[i]
            li[s, j] = top_id[i]
            lv[s, j] = top_lp[i]


def sample(logits: torch.Tensor, temperature: torch.Tensor, top_k: torch.Tensor,
           greedy: torch.Tensor, uniforms: torch.Tensor, vocab: int,
           top_p: Optional[torch.Tensor] = None, min_p: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-row sampler.  Reference semantics (server.py:187-206):
    logits/T -> topk(k) -> softmax over the k values -> draw -> map to vocab id.
    `uniforms` [B] in [0,1) drive the draw (inverse CDF over the top-k sorted
    descending), so the result is a deterministic function of its inputs.
    greedy rows return argmax (lowest index on ties).

    top_p / min_p [B] (optional) cut the sorted candidates to a prefix before
    the draw.  With e_i = exp(v_i - v_0) and c their running sum: min_p keeps
    the n_m entries with e_i >= min_p (p_i / p_max), top_p the shortest prefix
    n_p with c >= top_p * total (of the top-k-renormalised distribution; all k
    when top_p >= 1); the draw is the inverse CDF over the first
    n = max(1, min(n_p, n_m)) entries.  A row with top_p >= 1 and min_p <= 0
    (or None) takes the uncut path unchanged.
    """
    B = logits.shape[0]
    lg = logits[:, :vocab].float()
    out = torch.empty(B, dtype=torch.int32, device=logits.device)
    for r in range(B):
        row = lg[r]
        if bool(greedy[r]):
            out[r] = int(torch.argmax(row))
            continue
        k = int(top_k[r])
        # logit desc (numeric: -0.0 == +0.0), index asc, through a stable sort of
        # the whole row: torch.topk leaves open which of several equal values at
        # the k boundary it returns (not the lowest index).  The order is that
        # of the logits themselves, as on the device (two logits an ulp apart
        # can round to one quotient)
        vals, idx = torch.sort(row, descending=True, stable=True)
        vals, idx = vals[:k] / float(temperature[r]), idx[:k]
        tp = float(top_p[r]) if top_p is not None else 1.0
        mp = float(min_p[r]) if min_p is not None else 0.0
        if tp < 1.0 or mp > 0.0:
            e = torch.exp(vals - vals[0])
            c = torch.cumsum(e, 0)
            n_m = int((e >= mp).sum())
            n_p = k
            if tp < 1.0:
                hit = torch.nonzero(c >= tp * float(e.sum()))
                n_p = int(hit[0]) + 1 if hit.numel() else k
            n = max(1, min(n_p, n_m))
            c = c[:n]
            u = float(uniforms[r]) * float(c[-1])
            j = int(torch.searchsorted(c, torch.tensor([u], dtype=c.dtype)).clamp(max=n - 1))
            out[r] = int(idx[j])
            continue
        p = torch.softmax(vals, dim=-1)
        c = torch.cumsum(p, 0)
        u = float(uniforms[r]) * float(c[-1])
        j = int(torch.searchsorted(c, torch.tensor([u], dtype=c.dtype)).clamp(max=k - 1))
        out[r] = int(idx[j])
    return out


def check_forks(buf: torch.Tensor, src, dst, lens) -> tuple:
    """The host-side contract of kv_fork, for both backends: buf is a stage's
    whole KV allocation [layers, 2, slots, kv_heads, max_seq, head_dim]; src,
    dst and lens hold one entry per fork; slots lie in [0, slots) and lengths in
    [0, max_seq]; destinations are distinct and no destination is a source (a
    source may repeat).  -> (src, dst, lens) as lists of ints."""
    src, dst, lens = [int(s) for s in src], [int(d) for d in dst], [int(n) for n in lens]
    if buf.dim() != 6 or buf.shape[1] != 2 or not buf.is_contiguous():
        raise ValueError("kv_fork: buf is a contiguous [layers, 2, slots, kv_heads, max_seq, head_dim]")
    if not len(src) == len(dst) == len(lens):
        raise ValueError("kv_fork: src, dst and lens hold one entry per fork")
    S, L = buf.shape[2], buf.shape[4]
    if any(not 0 <= s < S for s in src + dst) or any(not 0 <= n <= L for n in lens):
        raise ValueError(f"kv_fork: a slot lies outside [0, {S}) or a length outside [0, {L}]")
    if len(set(dst)) != len(dst) or set(dst) & set(src):
        raise ValueError("kv_fork: destinations must be distinct and must not be sources")
    return src, dst, lens


def kv_fork(buf: torch.Tensor, src, dst, lens) -> None:
    """Fork prompts' KV: for fork f and every (layer, K|V, head), positions
    [0, lens[f]) of slot src[f] are copied to slot dst[f] of buf [layers, 2,
    slots, kv_heads, max_seq, head_dim].  Nothing else is written.  The twin
    of csrc/kernels/kv_fork.hip: what the CPU engine runs and what the GPU
    tests compare the kernel with, bit for bit."""
    for s, d, n in zip(*check_forks(buf, src, dst, lens)):
        if n:
            buf[:, :, d, :, :n] = buf[:, :, s, :, :n]
