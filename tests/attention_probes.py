"""Exact-arithmetic probes for the attention kernels (pure torch, CPU or GPU).

Random q / K / V with a 2e-2 tolerance cannot see a fault that touches one key
of a long context: it moves the output by p_j * |v_j - o|, a few 1e-3.  The
inputs built here have answers that are exact, so one dropped, doubled,
mis-paired or stale key is a large, deterministic error.

count probe   q = 0: every score is 0, every p is exactly 1, l = ctx exactly.
              V[slot, kvh, j, :] is the one-hot row of (j + kvh + 3 slot) % hd,
              so o[d] = #{j < ctx : (j + kvh + 3 slot) % hd == d} / ctx in
              closed form.  All partial sums are small integers (exact in
              fp32, and P = 1.0 is exact in bf16); the only roundings are
              1 / l, one multiply and the output store.
needle probe  K[j] = 2 s_j with s_j a random +-1 vector, V[j] random integers
              in +-{1..8}, q = 4 s_{j*}: the needle scores 8 sqrt(hd) nats, all
              other keys like 8 N(0, 1), so their total weight is far below
              the rounding of the output and o must be BIT-equal to V[j*].
              `needle_rest` computes that weight from fp64 scores; every user
              asserts it (NEEDLE_REST_BF16 / NEEDLE_REST_FP32) before it
              trusts the probe.
attention_bound  elementwise error bound for random data, from the number
              formats alone: 2^-8 (|ref| + A) + 2^-20 A with A the attention of
              |V| -- the bf16 output rounding, P rounded to bf16 against an
              fp32 l (the MFMA kernels), fp32 accumulation.
emulate       fp32 attention with fault knobs; tests/test_attention_probes.py
              shows that each checker accepts the fault-free emulation (plain
              and with P rounded to bf16) and rejects the faults meant for it.

Layouts as in ops/reference.py: caches [slots, n_kv, S, hd], q [rows, nh, hd],
one context length (position + 1) per row; head h reads kv head h // G.
"""
from __future__ import annotations

import math

import torch

from llm_sharding_demo_amd.ops import reference as ref

# contexts on both sides of every round / tile size of the kernels (32-key MFMA
# tiles, 64-key prefill tiles, rounds of 128 / 256 / 512 keys), plus 1, 2 and a
# tail past two rounds of the widest variant
EDGE_CTX = (1, 2, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1024, 1100)
S_PROBE = 1100

COUNT_REL_BF16 = 2.0 ** -8   # bf16 store (half an ulp); the fp32 terms are 2^-15 of it
COUNT_REL_FP32 = 2.0 ** -20  # fp32 output: a handful of fp32 roundings
NEEDLE_REST_BF16 = 2.0 ** -12  # rest weight * max|V| that cannot move a bf16 output
# fp32 output: l = fl(1 + rest) = 1 needs rest < 2^-24, o = fl(V + e) = V needs
# |e| < 2^-25 for |V| >= 1; 2^-26 leaves a factor 2 for the partial sums' own rounding
NEEDLE_REST_FP32 = 2.0 ** -26


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------
# count probe
# ---------------------------------------------------------------------------
def count_cache(slots: int, n_kv: int, S: int, hd: int, seed: int = 5):
    """(K, V) bf16 [slots, n_kv, S, hd]: K arbitrary finite, V one-hot rows."""
    kc = torch.randn(slots, n_kv, S, hd, generator=_gen(seed)).to(torch.bfloat16)
    j = torch.arange(S)[None, None, :]
    kvh = torch.arange(n_kv)[None, :, None]
    sl = torch.arange(slots)[:, None, None]
    hot = (j + kvh + 3 * sl) % hd
    vc = torch.zeros(slots, n_kv, S, hd)
    vc.scatter_(3, hot[..., None], 1.0)
    return kc, vc.to(torch.bfloat16)


def count_expected(seq_slots, ctx, nh: int, n_kv: int, hd: int) -> torch.Tensor:
    """fp64 [rows, nh, hd]: #{j < ctx : (j + kvh + 3 slot) % hd == d} / ctx."""
    sl = torch.as_tensor(seq_slots).long().cpu()[:, None, None]
    c = torch.as_tensor(ctx).long().cpu()[:, None, None]
    kvh = (torch.arange(nh) // (nh // n_kv))[None, :, None]
    d = torch.arange(hd)[None, None, :]
    first = (d - kvh - 3 * sl) % hd  # smallest j >= 0 that lands on d
    cnt = torch.div(c + hd - 1 - first, hd, rounding_mode="floor")
    return cnt.double() / c.double()


def count_ratio(out: torch.Tensor, exp: torch.Tensor, rel: float = COUNT_REL_BF16) -> float:
    """max |out - e| / (rel e) over the non-zero expectations; inf when a zero
    expectation did not come out as exactly 0 (or anything is not finite).
    The probe passes iff the result is <= 1."""
    o, e = out.double().reshape(exp.shape), exp.to(out.device)
    if not bool(torch.isfinite(o).all()):
        return math.inf
    zero = e == 0
    if bool((o[zero] != 0).any()):
        return math.inf
    if bool(zero.all()):
        return 0.0
    return float(((o - e).abs()[~zero] / (rel * e[~zero])).max())


# ---------------------------------------------------------------------------
# needle probe
# ---------------------------------------------------------------------------
def needle_cache(slots: int, n_kv: int, S: int, hd: int, seed=None):
    """(K, V) bf16 [slots, n_kv, S, hd]: K = 2 s_j (s_j random +-1), V random
    integers in +-{1..8}; the seed defaults to the head dim."""
    g = _gen(hd if seed is None else seed)
    sign = torch.randint(0, 2, (slots, n_kv, S, hd), generator=g) * 2 - 1
    mag = torch.randint(1, 9, (slots, n_kv, S, hd), generator=g)
    sgn = torch.randint(0, 2, (slots, n_kv, S, hd), generator=g) * 2 - 1
    return (2 * sign).to(torch.bfloat16), (mag * sgn).to(torch.bfloat16)


def needle_q(kc: torch.Tensor, seq_slots, needles: torch.Tensor) -> torch.Tensor:
    """bf16 [rows, nh, hd]: q of (row, head) = 4 s_{j*} = 2 K[slot, kvh, j*];
    needles is int [rows, nh]."""
    n_kv, nh = kc.shape[1], needles.shape[1]
    sl = torch.as_tensor(seq_slots).long().to(kc.device)[:, None]
    kvh = (torch.arange(nh, device=kc.device) // (nh // n_kv))[None, :]
    return (kc[sl, kvh, needles.long().to(kc.device)].float() * 2).to(torch.bfloat16)


def needle_expected(vc: torch.Tensor, seq_slots, needles: torch.Tensor) -> torch.Tensor:
    """bf16 [rows, nh, hd]: V[slot, kvh, j*]."""
    n_kv, nh = vc.shape[1], needles.shape[1]
    sl = torch.as_tensor(seq_slots).long().to(vc.device)[:, None]
    kvh = (torch.arange(nh, device=vc.device) // (nh // n_kv))[None, :]
    return vc[sl, kvh, needles.long().to(vc.device)]


def sweep_needles(ctxs=EDGE_CTX, nh: int = 1):
    """Rows = every (ctx, j*) with j* < ctx; head h of a row uses
    (j* + 7 h) % ctx.  Returns (ctx [rows], needles [rows, nh]) int64."""
    c = torch.cat([torch.full((n,), n) for n in ctxs])
    j = torch.cat([torch.arange(n) for n in ctxs])
    return c, (j[:, None] + 7 * torch.arange(nh)[None, :]) % c[:, None]


def needle_rest(kc: torch.Tensor, vc: torch.Tensor, seq_slots, needles: torch.Tensor, n_keys=None) -> float:
    """The probe's precondition, from fp64 scores: the largest, over the given
    (row, head) needles, of  sum_{j != j*} exp(s_j - s_{j*}) * max|V|  with j
    over the first n_keys positions (default: the whole cache, an upper bound
    for every context)."""
    kc, vc = kc.cpu(), vc.cpu()
    n_kv, hd = kc.shape[1], kc.shape[3]
    nh = needles.shape[1]
    n = kc.shape[2] if n_keys is None else n_keys
    sl = torch.as_tensor(seq_slots).long().cpu()[:, None].expand(-1, nh)
    kvh = (torch.arange(nh) // (nh // n_kv))[None, :].expand_as(sl)
    trip = torch.unique(torch.stack([sl.reshape(-1), kvh.reshape(-1), needles.long().cpu().reshape(-1)], 1), dim=0)
    vmax = float(vc.float().abs().max())
    worst = 0.0
    for s in torch.unique(trip[:, 0]).tolist():
        for h in torch.unique(trip[trip[:, 0] == s, 1]).tolist():
            js = trip[(trip[:, 0] == s) & (trip[:, 1] == h), 2]
            K = kc[s, h, :n].double()
            for a in range(0, js.numel(), 512):
                jj = js[a:a + 512]
                sc = (2 * kc[s, h, jj].double()) @ K.t() / math.sqrt(hd)  # [needles, n]
                own = sc.gather(1, jj[:, None])
                w = torch.exp(sc - own)
                w.scatter_(1, jj[:, None], 0.0)
                worst = max(worst, float(w.sum(1).max()) * vmax)
    return worst


def stale_tail_case(n_kv: int, G: int, hd: int, ctxs, S: int = S_PROBE, seed=None):
    """One row per context, each on its own slot, with poison behind its end:
    cache positions >= ctx hold K = 3 s_{j*} (1.5x the needle's score) and
    V = -V[j*].  The G heads of a kv head share one needle (the poison is one
    key per kv head).  Returns q [rows, nh, hd], K, V, slots, ctx, needles
    [rows, nh], expected [rows, nh, hd] and the clean (un-poisoned) K for the
    precondition."""
    rows = len(ctxs)
    clean, vc = needle_cache(rows, n_kv, S, hd, seed)
    kc = clean.clone()
    slots = torch.arange(rows)
    ctx = torch.tensor(list(ctxs))
    per_kv = (3 * ctx[:, None] // 4 + 5 * torch.arange(n_kv)[None, :]) % ctx[:, None]  # [rows, n_kv]
    needles = per_kv.repeat_interleave(G, dim=1)
    q = needle_q(clean, slots, needles)
    exp = needle_expected(vc, slots, needles).clone()
    for r in range(rows):
        c = int(ctx[r])
        for h in range(n_kv):
            j = int(per_kv[r, h])
            kc[r, h, c:] = (clean[r, h, j].float() * 1.5).to(torch.bfloat16)
            vc[r, h, c:] = -vc[r, h, j]
    return q, kc, vc, slots, ctx, needles, exp, clean


# ---------------------------------------------------------------------------
# bounded error on random data
# ---------------------------------------------------------------------------
def attention_bound(o_ref: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    """2^-8 (|ref| + A) + 2^-20 A, elementwise; A = attention of |V|."""
    return 2.0 ** -8 * (o_ref.abs() + A) + 2.0 ** -20 * A


def reference_and_bound(q, kc, vc, seq_slots, q_start, cu_q):
    """(fp64 reference, attention_bound) of ref.attention's arguments."""
    args = (seq_slots.cpu(), q_start.cpu(), cu_q.cpu())
    q64, k64, v64 = q.cpu().double(), kc.cpu().double(), vc.cpu().double()
    o = ref.attention(q64, k64, v64, *args)
    A = ref.attention(q64, k64, v64.abs(), *args)
    assert o.dtype == torch.float64
    return o, attention_bound(o, A)


def bound_ratio(out: torch.Tensor, o_ref: torch.Tensor, bound: torch.Tensor) -> float:
    """max |out - ref| / bound; the check passes iff the result is <= 1."""
    o = out.detach().cpu().double().reshape(o_ref.shape)
    if not bool(torch.isfinite(o).all()):
        return math.inf
    return float(((o - o_ref).abs() / bound).max())


# ---------------------------------------------------------------------------
# fp32 emulation with fault knobs
# ---------------------------------------------------------------------------
def emulate(q, kc, vc, seq_slots, ctx, fault=None, out_dtype=torch.bfloat16) -> torch.Tensor:
    """fp32 attention of q [rows, nh, hd] over the first ctx[row] keys of slot
    seq_slots[row]; the result, rounded to out_dtype, as fp32 [rows, nh, hd].

    fault: None, a name, a (name, arg) pair, or a list of those --
      "drop_last"        the last key of the context is not counted
      ("drop_at", j)     key j is not counted (rows with ctx > j)
      ("dup_at", j)      key j is counted twice (rows with ctx > j)
      "extra_key"        the key at position ctx (one past the end) is counted
      "shift_v"          p_j is paired with V[(j + 1) % ctx]
      "wrong_kv_head"    K and V are read from kv head (kvh + 1) % n_kv
      ("scale", f)       scores multiplied by f
      "p_bf16"           P rounded to bf16 before P.V, l from the fp32 P
                         (the MFMA kernels' arithmetic; not a fault)
    """
    faults = fault if isinstance(fault, list) else ([] if fault is None else [fault])
    faults = [(f, None) if isinstance(f, str) else tuple(f) for f in faults]
    known = {"drop_last", "drop_at", "dup_at", "extra_key", "shift_v", "wrong_kv_head", "scale", "p_bf16"}
    assert all(f in known for f, _ in faults), faults
    names = dict(faults)
    rows, nh, hd = q.shape
    n_kv, S = kc.shape[1], kc.shape[2]
    G = nh // n_kv
    seq_slots = torch.as_tensor(seq_slots).long().cpu()
    ctx = torch.as_tensor(ctx).long().cpu()
    if "wrong_kv_head" in names:
        kc, vc = kc.roll(-1, dims=1), vc.roll(-1, dims=1)
    pos = torch.arange(S)[None, :]
    wgt = (pos < ctx[:, None]).float()  # multiplicity of every key, [rows, S]
    r = torch.arange(rows)
    if "drop_last" in names:
        wgt[r, ctx - 1] = 0.0
    if "drop_at" in names:
        j = names["drop_at"]
        wgt[ctx > j, j] = 0.0
    if "dup_at" in names:
        j = names["dup_at"]
        wgt[ctx > j, j] = 2.0
    if "extra_key" in names:
        ok = ctx < S
        wgt[r[ok], ctx[ok]] = 1.0
    scale = float(names.get("scale") or 1.0) / math.sqrt(hd)
    out = torch.zeros(rows, nh, hd)
    qf = q.float().cpu().reshape(rows, n_kv, G, hd)
    for s in torch.unique(seq_slots).tolist():
        sel = torch.nonzero(seq_slots == s).flatten()
        K, V = kc[s].float().cpu(), vc[s].float().cpu()  # [n_kv, S, hd]
        w = wgt[sel][:, None, None, :]
        sc = torch.einsum("rkgd,ksd->rkgs", qf[sel], K) * scale
        sc = sc.masked_fill(w == 0, float("-inf"))
        m = sc.amax(-1, keepdim=True)
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))  # nothing counted: l = 0
        p = torch.exp(sc - m) * w
        l = p.sum(-1, keepdim=True)
        if "p_bf16" in names:
            p = p.to(torch.bfloat16).float()
        if "shift_v" in names:  # P'[j] = P[(j - 1) % ctx]: weight of key j lands on V[j + 1]
            c = ctx[sel][:, None]
            src = torch.where(pos < c, (pos - 1) % c, pos)[:, None, None, :].expand_as(p)
            p = p.gather(-1, src)
        o = torch.einsum("rkgs,ksd->rkgd", p, V)
        o = torch.where(l > 0, o / l, torch.zeros_like(o))
        out[sel] = o.reshape(sel.numel(), nh, hd)
    return out.to(out_dtype).float()


# ---------------------------------------------------------------------------
# the cases of tests/test_attention_exact_gpu.py, shared with the CPU self-test
# ---------------------------------------------------------------------------
VALU_SHAPES = ((64, 4, 4), (64, 8, 4), (64, 8, 2), (128, 4, 4), (128, 8, 4), (128, 8, 2), (128, 16, 2))  # hd, nh, n_kv
MFMA_SHAPES = ((128, 8, 4), (128, 8, 2), (128, 16, 2))  # G = 2, 4, 8
PREFILL_SHAPES = ((64, 4, 4), (64, 8, 2), (128, 4, 4), (128, 8, 2))  # G = 1 and 4
OPROJ_SHAPES = ((64, 4, 4), (128, 2, 2), (128, 4, 2), (128, 8, 2), (128, 16, 2))  # G = 1; 1, 2, 4, 8
# (slot, cached tokens, new tokens): tiles of 64 + 64 + 2 queries; one token;
# exactly one tile; an unaligned start; many key tiles
PREFILL_SEQS = ((1, 0, 130), (0, 0, 1), (3, 0, 64), (2, 37, 200), (4, 1000, 70))
STALE_CTX = (1, 2, 33, 128, 257, 511, 513, 1024)
# (rows, nh, n_kv, hd, captured context bucket) of three launches of the engine
ROUTED = ((256, 25, 25, 64, 300), (1, 32, 8, 128, 300), (8, 32, 8, 128, 8128))


def count_sweep(hd: int, nh: int, n_kv: int, S: int = S_PROBE, ctxs=None):
    """One row per context 1..S (or per entry of ctxs), alternating over two
    shared slots.  Returns q (zeros), K, V, slots, ctx, expected (fp64)."""
    ctx = torch.arange(1, S + 1) if ctxs is None else torch.tensor(list(ctxs))
    slots = (ctx + ctx // 7) % 2
    kc, vc = count_cache(2, n_kv, S, hd)
    q = torch.zeros(ctx.numel(), nh, hd, dtype=torch.bfloat16)
    return q, kc, vc, slots, ctx, count_expected(slots, ctx, nh, n_kv, hd)


def needle_sweep(hd: int, nh: int, n_kv: int, S: int = S_PROBE, ctxs=EDGE_CTX):
    """Rows = every (ctx, j*) of the contexts, over two shared slots.  Returns
    q, K, V, slots, ctx, needles, expected (bf16)."""
    ctx, needles = sweep_needles(ctxs, nh)
    slots = torch.arange(ctx.numel()) % 2
    kc, vc = needle_cache(2, n_kv, S, hd)
    return needle_q(kc, slots, needles), kc, vc, slots, ctx, needles, needle_expected(vc, slots, needles)


def prefill_rows(seqs=PREFILL_SEQS):
    """(slot, position) of every packed query row of the sequences."""
    slots = torch.tensor([s for s, st, n in seqs for _ in range(n)])
    pos = torch.tensor([st + i for s, st, n in seqs for i in range(n)])
    return slots, pos


def prefill_count(hd: int, nh: int, n_kv: int, S: int = S_PROBE, seqs=PREFILL_SEQS):
    """Count probe over a packed prefill batch: query at position pos expects
    c(pos + 1) / (pos + 1).  Returns q, K, V, row slots, row ctx, expected."""
    slots, pos = prefill_rows(seqs)
    kc, vc = count_cache(1 + max(s for s, _, _ in seqs), n_kv, S, hd)
    q = torch.zeros(pos.numel(), nh, hd, dtype=torch.bfloat16)
    return q, kc, vc, slots, pos + 1, count_expected(slots, pos + 1, nh, n_kv, hd)


def prefill_needle(hd: int, nh: int, n_kv: int, S: int = S_PROBE, seqs=PREFILL_SEQS):
    """Needle probe over a packed prefill batch: one needle <= pos per (token,
    head) -- the token's own position for head 0 (the causal mask's edge),
    then positions spread over the context."""
    slots, pos = prefill_rows(seqs)
    h = torch.arange(nh)[None, :]
    needles = (pos[:, None] - h * (1 + 3 * pos[:, None] // 7)) % (pos[:, None] + 1)
    kc, vc = needle_cache(1 + max(s for s, _, _ in seqs), n_kv, S, hd)
    return needle_q(kc, slots, needles), kc, vc, slots, pos + 1, needles, needle_expected(vc, slots, needles)


def routed_rows(B: int, nh: int, bucket: int):
    """Rows of a launch captured for `bucket` keys: contexts 1, bucket / 2 and
    bucket (one launch each for a single row, rotated over the rows
    otherwise), two slots, needles at 3/4 of the context + 7 h.  Yields
    (slots, ctx, needles)."""
    mix = [1, bucket // 2, bucket]
    sets = [[c] for c in mix] if B == 1 else [[mix[(i + k) % 3] for i in range(B)] for k in range(3)]
    for ctxs in sets:
        ctx = torch.tensor(ctxs)
        needles = (3 * ctx[:, None] // 4 + 7 * torch.arange(nh)[None, :]) % ctx[:, None]
        yield torch.arange(B) % 2, ctx, needles
