"""Exact-arithmetic probes for the GEMM / GEMV kernels and their epilogues
(pure torch, CPU or GPU).

Random bf16 data with `close(..., 3e-2, rtol=2e-2)` cannot see a fault that is
limited to one row, one lane or one rounding: bf16 split-K partials, a bias
applied once per split or a RoPE position off by one all stay inside it
(tests/test_gemm_probes.py pins that).  The inputs built here have answers that
are one bit pattern, the same for every kernel variant, tile shape, split
count and ring depth.

Why they are exact.  A product of two bf16 integers of magnitude <= 2 is an
integer, exact in fp32; an fp32 sum of integers is exact in any order while
every partial sum stays below 2^24.  bf16 keeps 8 significant bits, so every
integer of magnitude <= 256 (BF16_INT) is a bf16 number and a bf16 store of it
is exact too.

integer probe  a in {-1, 0, 0, 1}, w in {-2 .. 2}, both uniform: one term has
              variance 1/2 * 2 = 1, a K-term sum a standard deviation sqrt(K)
              -- 40 at K = 1600, where 300 x 384 outputs reach about 5.2
              sigma = 209.  Bias is an integer in [-8, 8], so |y + bias| <=
              217 < 256 with room.  Above K = 2048 `a` is thinned with
              probability 1600 / K so the variance stays 1600.  Nothing is
              taken on trust: `exact_product` gives the int64 answer and
              `assert_bf16_exact` / `max_partial_range` assert |y + bias| <=
              256 (bf16 outputs) and that every partial sum over whole 32-k
              blocks is <= 256 in magnitude (bf16 split-K slabs: each
              partial is then a bf16 number, and the folded sum is exact).
              The residual x is an integer in [-64, 64] held in fp32.
wide probe    fp32 outputs need only 2^24, and that is what lets them see a
              double rounding: `wide_weights` gives w' = 16 w + w2 (w2 a second
              draw from {-2 .. 2}; |w'| <= 34 are bf16 integers), so partial
              sums are odd and even integers of a few thousand -- 12 bits, not
              bf16 numbers.  Partials rounded to bf16 before a split-K combine
              are invisible to the bf16 probe (its partials are bf16 numbers
              by construction) and a wrong integer here.  The fp32, segmax,
              residual and fp32-slab epilogues use it.
placement     one-hot rows a[m, k_m] = 1 give y[m, n] = w[n, k_m]; w holds
              the column code (n % 251) - 125 in one launch and the k code
              (k % 251) - 125 in another (251: the largest prime <= 256, codes
              in [-125, 125] are bf16 integers).  A wrong element is named by
              its code.  Blind spot, pinned in the CPU test: codes repeat
              every 251, two columns 251 apart may swap unseen (the integer
              probe sees that).
poison        operands are views into larger buffers (row stride K + 16,
              extra rows before and after, base 16 bytes in) whose other
              elements hold POISON = 64: any element read from outside
              [M, K] / [N, K] and used moves an integer result by a multiple
              of 64 times a weight.
guards        the residual and the KV caches are views into larger buffers
              filled with SENTINEL = -776 (a bf16 number no probe can
              produce: results are <= 256 + 64 in magnitude); the cache
              positions no (slot, position) addresses hold it too.  After a
              launch the whole buffer is compared with the expectation, so a
              write anywhere else is seen.
rope          a synthetic table whose (cos, sin) entries are the four exact
              quarter turns (1,0), (0,1), (-1,0), (0,-1), chosen by
              r(pos, pair) = (pos + 3 pair + 2 ((pos // 4 + pair // 4) % 2))
              % 4.  r(pos + 1, pair) - r(pos, pair) and r(pos, pair + 1) -
              r(pos, pair) are 1 or 3 mod 4 -- never 0 -- so a wrong position
              or pair is another rotation; a rotation by a quarter turn only
              permutes and negates integers, so the result is exact.
SiLU . up     up probe: column 0 of `a` is 1 and gate weights are 32 in
              column 0, 0 elsewhere, so gate = 32 exactly; silu(32) = 32 /
              (1 + 2^-46.2) and 1 + 2^-46 rounds to 1 in fp32, so the output
              is 32 * up bit-exactly (|up| <= 256: still 8 significant bits).
              gate probe: up pinned to 1 the same way, silu(gate) checked
              with the activation bound.
activations   gelu_new and silu (csrc/kernels/common.h) are
                  f(x) = x * rcp(1 + exp2(y)),
                  y = x * fma(k c, x^2, k)  (gelu, k = -2 sqrt(2/pi) log2 e)
                  y = -log2(e) * x          (silu)
              with v_exp_f32 and v_rcp_f32 (1 ulp = 2^-23 each), so they are
              not bit-defined.  Against the fp64 function of the exact
              pre-activation x:
                * y carries a relative error dy: gelu's k is a product of
                  three rounded constants (4 x 2^-24), k c one constant and
                  one product more (2 x 2^-24), the fma and the product with
                  x one rounding each, both fma terms of one sign: dy <=
                  2^-21; silu has one constant and one product: dy <= 2^-23;
                * e = exp2(y) has relative error |y| ln 2 dy + 2^-23 (the
                  argument error amplified through exp2, plus its ulp);
                * 1 + e: the error of e weighs e / (1 + e) = s, plus 2^-24;
                  rcp 2^-23; the product with x 2^-24.
              E(x) = s (|y| ln 2 dy + 2^-23) + 2^-22 relative for the fp32
              value, then the bf16 store 2^-8 on top:
                  |out - f(x)| <= (2^-8 + (1 + 2^-8) E(x)) |f(x)| + ACT_FLOOR.
              ACT_FLOOR = 2^-117: an intermediate below the smallest normal
              2^-126 may be flushed to zero (rcp of 1 + e > 2^126, or e =
              inf), and the result is that times |x| < 2^9.
              `act_emulate` evaluates the same formula in fp32 with
              torch.exp2 and reciprocal; the CPU test measures it against the
              bound for every integer and half-integer in [-300, 300].  The
              margin over the emulation is the two hardware ulps it lacks.
fused norm    residual rows are a balanced permutation of +-1 (K even): mean
              0 and variance 1 exactly, rstd = rsqrt(1 + eps) = 1 - 5e-6;
              gamma in {-1, 0, 1}, LayerNorm beta in {-2, 0, 2}, so the
              normalised values are +-rstd + {-2, 0, 2} or beta alone:
              within 2^-17 of an integer in {-3 .. 3} and never a small
              difference of large terms, so their bf16 rounding is exactly
              x gamma + beta.  `norm_case` asserts that from an fp32
              emulation with rstd moved by +-2e-4 before it trusts it.
emulate       an fp32 GEMM with every epilogue and fault knobs (one dropped
              k for one row, an 8-k chunk for one lane's 4 outputs, a
              repeated k-step, an omitted or repeated split, bf16 partials,
              bias per split, swapped columns, gate/up interleave off by a
              block, RoPE position / pair / sign, KV row at pos + 1 or in the
              wrong slot, an element read past K, a row written past M);
              tests/test_gemm_probes.py shows each checker accepts the
              fault-free emulation and rejects the faults meant for it.

Layouts as in the bindings: a [M, K], w [N, K] (K contiguous), caches
[slots, n_kv, S, hd]; SiLU weights through ops/hip.py interleave_gate_up; RoPE
weights through rope_pair_permutation, q and K then live in pair order.
"""
from __future__ import annotations

import math

import torch

BF16_INT = 256          # integers up to here are bf16 numbers
POISON = 64.0
SENTINEL = -776.0       # 97 * 8: a bf16 number, beyond every probe result
CODE_MOD, CODE_OFF = 251, 125
ACT_FLOOR = 2.0 ** -117
ACT_DY = {"gelu": 2.0 ** -21, "silu": 2.0 ** -23}
VAR_TARGET = 1600       # K x density of `a` (K > 2048 is thinned to this)
_LOG2E = 1.4426950408889634
_GELU_C = 0.7978845608028654


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------
# integer probe
# ---------------------------------------------------------------------------
def integer_operands(M: int, N: int, K: int, seed: int = 0, w_density: float = 1.0):
    """(a [M, K], w [N, K], bias [N], x [M, N]) as int64."""
    g = _gen(seed)
    a = torch.tensor([-1, 0, 0, 1])[torch.randint(0, 4, (M, K), generator=g)]
    if K > 2048:
        a = a * (torch.rand(M, K, generator=g) < VAR_TARGET / K)
    w = torch.randint(-2, 3, (N, K), generator=g)
    if w_density < 1.0:
        w = w * (torch.rand(N, K, generator=g) < w_density)
    bias = torch.randint(-8, 9, (N,), generator=g)
    x = torch.randint(-64, 65, (M, N), generator=g)
    return a, w, bias, x


def wide_weights(w: torch.Tensor, seed: int = 0) -> torch.Tensor:
    """16 w + w2 with w2 uniform in {-2 .. 2}: the fp32 epilogues' weights."""
    return 16 * w + torch.randint(-2, 3, tuple(w.shape), generator=_gen(seed + 991))


def exact_product(a: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """int64 a @ w^T through fp64 (exact: every sum is far below 2^53)."""
    y = a.detach().cpu().double() @ w.detach().cpu().double().t()
    assert float(y.abs().max()) < 2.0 ** 24 if y.numel() else True
    return y.round().long()


def assert_bf16_exact(y: torch.Tensor, bias=None) -> int:
    """Precondition of a bf16 output: max |y + bias| <= 256.  Returns it."""
    v = y if bias is None else y + bias.long().cpu()[None, :]
    m = int(v.abs().max()) if v.numel() else 0
    assert m <= BF16_INT, f"integer probe out of the bf16-exact range: {m}"
    return m


def max_partial_range(a: torch.Tensor, w: torch.Tensor, step: int = 32) -> int:
    """Largest |sum over k in [i step, j step)| over every output and every
    i < j: the bound on any split-K partial whose boundaries are multiples of
    `step`.  bf16 slabs are exact when this is <= 256."""
    a, w = a.detach().cpu().double(), w.detach().cpu().double()
    M, K = a.shape
    assert K % step == 0
    KB = K // step
    wb = w.reshape(w.shape[0], KB, step)
    worst = 0.0
    for r in range(0, M, 64):
        p = torch.einsum("mbk,nbk->mnb", a[r:r + 64].reshape(-1, KB, step), wb).cumsum(-1)
        hi = p.amax(-1).clamp_min(0.0)
        lo = p.amin(-1).clamp_max(0.0)
        worst = max(worst, float((hi - lo).max()))
    return int(worst)


def segmax_expected(y: torch.Tensor) -> torch.Tensor:
    """Exact maximum of every 8-column segment, [M, N / 8]."""
    M, N = y.shape
    return y.reshape(M, N // 8, 8).amax(-1)


def split_bounds(K: int, S: int, step: int):
    """k ranges of the S splits as the kernels cut them (whole `step`-k steps)."""
    assert K % step == 0, (K, step)
    KT = K // step
    return [(KT * s // S * step, KT * (s + 1) // S * step) for s in range(S)]


# ---------------------------------------------------------------------------
# placement probe
# ---------------------------------------------------------------------------
def code(i):
    return (i % CODE_MOD) - CODE_OFF


def placement_operands(M: int, N: int, K: int, which: str):
    """a one-hot [M, K] with a[m, k_m] = 1, k_m = (7 m + 3) % K; w [N, K] holds
    the column code (which = "n") or the k code ("k").  Returns a, w, k_m, y."""
    km = (7 * torch.arange(M) + 3) % K
    a = torch.zeros(M, K, dtype=torch.int64)
    a[torch.arange(M), km] = 1
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    w = (code(n) if which == "n" else code(k)).expand(N, K).contiguous()
    y = code(torch.arange(N))[None, :].expand(M, N) if which == "n" else code(km)[:, None].expand(M, N)
    return a, w, km, y.contiguous()


def placement_mismatch(out: torch.Tensor, y: torch.Tensor, which: str, km: torch.Tensor, N: int, K: int):
    """None, or a sentence naming the first wrong element and where its value
    came from."""
    o = out.detach().cpu().double().reshape(y.shape)
    bad = torch.nonzero(o != y.double())
    if bad.numel() == 0:
        return None
    m, n = (int(v) for v in bad[0])
    got = float(o[m, n])
    if got != round(got) or abs(got) > CODE_OFF:
        src = "no code"
    elif which == "n":
        src = "column(s) " + str([c for c in range(N) if int(code(c)) == int(got)][:4])
    else:
        src = "k " + str([c for c in range(K) if int(code(c)) == int(got)][:4])
    return (f"{int(bad.shape[0])} wrong; first y[{m}, {n}] = {got}, expected {int(y[m, n])} "
            f"(k_m = {int(km[m])}): value of {src}")


# ---------------------------------------------------------------------------
# poison and guards
# ---------------------------------------------------------------------------
def poisoned(t: torch.Tensor, value: float = POISON, rows: int = 2, pad: int = 8) -> torch.Tensor:
    """A view equal to the 2-D t inside a larger buffer full of `value`: `rows`
    extra rows on both sides, `pad` extra elements on both sides of every
    row (row stride = width + 2 pad; pad % 8 == 0 keeps 16-byte alignment)."""
    assert t.dim() == 2 and pad % 8 == 0 and t.shape[1] % 8 == 0
    R, W = t.shape
    buf = torch.full((R + 2 * rows, W + 2 * pad), value, dtype=t.dtype, device=t.device)
    v = buf[rows:rows + R, pad:pad + W]
    v.copy_(t)
    return v


def guarded(t: torch.Tensor, rows: int = 2, value: float = SENTINEL):
    """(buffer, view): a contiguous view equal to t with `rows` leading-dim
    entries of `value` on both sides."""
    buf = torch.full((t.shape[0] + 2 * rows,) + tuple(t.shape[1:]), value, dtype=t.dtype, device=t.device)
    v = buf[rows:rows + t.shape[0]]
    v.copy_(t)
    return buf, v


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit-for-bit equality (sentinels and -0.0 included)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return bool(torch.equal(a.contiguous().view(it), b.to(a.device).contiguous().view(it)))


def same_values(out: torch.Tensor, exp: torch.Tensor) -> bool:
    """Every element equal to the exact expectation (integers: +0 only)."""
    return bool(torch.equal(out.detach().double().reshape(exp.shape), exp.detach().double().to(out.device)))


# ---------------------------------------------------------------------------
# QKV epilogue: head split, KV-cache append, synthetic RoPE
# ---------------------------------------------------------------------------
def qkv_dims(N: int):
    """(q_size, kv_size, hd, n_heads, n_kv) for N output columns: 2 kv heads,
    the rest q heads; 32-dim heads when N allows, else 16 (8: GEMV only)."""
    hd = 32 if N % 32 == 0 else (16 if N % 16 == 0 else 8)
    heads = N // hd
    assert N % 8 == 0 and heads >= 5
    return (heads - 4) * hd, 2 * hd, hd, heads - 4, 2


def token_map(M: int, slots: int = 3):
    """Unique (slot, position) per row: row m -> slot m % slots, position
    2 (m // slots) + slot, so the rows of a slot leave every other position
    unaddressed.  Returns (tslot, tpos) int32 and the cache length S."""
    m = torch.arange(M)
    tslot = m % slots
    tpos = 2 * (m // slots) + tslot
    return tslot.int(), tpos.int(), int(tpos.max()) + 3


def rope_rotation(pos, pair):
    return (pos + 3 * pair + 2 * ((pos // 4 + pair // 4) % 2)) % 4


def rope_table_exact(S: int, hd: int) -> torch.Tensor:
    """fp32 [S, hd / 2, 2] of exact quarter turns (see the module docstring)."""
    r = rope_rotation(torch.arange(S)[:, None], torch.arange(hd // 2)[None, :])
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[r]
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[r]
    return torch.stack([cos, sin], -1).contiguous()


def rope_rotate(v: torch.Tensor, tpos: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """HF rotate_half convention (pairs (i, i + hd / 2)) with the table's
    (cos, sin): v [M, heads, hd] in the model's order."""
    half = v.shape[-1] // 2
    cs = table.to(v.dtype)[tpos.long()]  # [M, half, 2]
    c, s = cs[:, None, :, 0], cs[:, None, :, 1]
    x1, x2 = v[..., :half], v[..., half:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


def qkv_expected(y: torch.Tensor, N: int, tslot, tpos, slots: int, S: int, table=None, guard: int = 1, dims=None):
    """From the exact y + bias [M, N] in the model's column order: q fp64
    [M, q_size] and the two whole cache buffers (guard slots included,
    SENTINEL wherever nothing is written) as bf16.  With a table, q and K are
    rotated and returned in the kernel's pair order.  dims: (q_size, kv_size,
    hd, n_heads, n_kv) when they are not qkv_dims(N)."""
    from llm_sharding_demo_amd.ops.hip import rope_pair_permutation

    qs, kvs, hd, nh, nkv = dims or qkv_dims(N)
    M = y.shape[0]
    y = y.double()
    q = y[:, :qs].reshape(M, nh, hd)
    k = y[:, qs:qs + kvs].reshape(M, nkv, hd)
    v = y[:, qs + kvs:].reshape(M, nkv, hd)
    if table is not None:
        hp = rope_pair_permutation(1, hd)
        q = rope_rotate(q, tpos, table.double())[..., hp]
        k = rope_rotate(k, tpos, table.double())[..., hp]
    kc = torch.full((slots + 2 * guard, nkv, S, hd), SENTINEL, dtype=torch.float64)
    vc = kc.clone()
    kc[tslot.long() + guard, :, tpos.long()] = k
    vc[tslot.long() + guard, :, tpos.long()] = v
    assert float(kc.abs().max()) <= 776 and float(q.abs().max() if q.numel() else 0) <= BF16_INT
    return q.reshape(M, qs), kc.to(torch.bfloat16), vc.to(torch.bfloat16)


def qkv_weight_order(N: int) -> torch.Tensor:
    """Row permutation of the QKV weight and bias for the RoPE epilogue."""
    from llm_sharding_demo_amd.ops.hip import rope_pair_permutation

    qs, kvs, hd, nh, nkv = qkv_dims(N)
    return torch.cat([rope_pair_permutation(nh, hd), rope_pair_permutation(nkv, hd) + qs,
                      torch.arange(qs + kvs, N)])


# ---------------------------------------------------------------------------
# activations
# ---------------------------------------------------------------------------
def _act_y(name: str, x: torch.Tensor) -> torch.Tensor:
    x = x.double()
    if name == "gelu":
        return -2.0 * _GELU_C * _LOG2E * x * (1.0 + 0.044715 * x * x)
    return -_LOG2E * x


def act_ref(name: str, x: torch.Tensor) -> torch.Tensor:
    """fp64 gelu_new / silu of the exact pre-activation: x / (1 + 2^y)."""
    x = x.double()
    return x / (1.0 + torch.exp2(_act_y(name, x).clamp(max=1100.0)))


def act_bound(name: str, x: torch.Tensor) -> torch.Tensor:
    y = _act_y(name, x)
    s = 1.0 / (1.0 + torch.exp2((-y).clamp(max=1100.0)))  # e / (1 + e)
    E = s * (y.abs() * math.log(2.0) * ACT_DY[name] + 2.0 ** -23) + 2.0 ** -22
    return (2.0 ** -8 + (1.0 + 2.0 ** -8) * E) * act_ref(name, x).abs() + ACT_FLOOR


def act_ratio(out: torch.Tensor, name: str, pre: torch.Tensor, scale=None) -> float:
    """max |out - f(pre)| / bound (`scale`: an exact factor on f, the SiLU
    gate probe's up = 1); inf when anything is not finite.  Passes iff <= 1."""
    o = out.detach().double().reshape(pre.shape)
    pre = pre.to(o.device)
    if not bool(torch.isfinite(o).all()):
        return math.inf
    f, b = act_ref(name, pre), act_bound(name, pre)
    if scale is not None:
        f, b = f * scale, b * abs(scale)
    return float(((o - f).abs() / b).max()) if o.numel() else 0.0


def act_emulate(name: str, x: torch.Tensor) -> torch.Tensor:
    """common.h's formula in fp32 (torch.exp2 / reciprocal for v_exp_f32 /
    v_rcp_f32), the bf16 store included; returned as fp32."""
    x = x.float()
    if name == "gelu":
        k = torch.tensor(-2.0, dtype=torch.float32) * torch.tensor(_GELU_C, dtype=torch.float32)
        k = k * torch.tensor(_LOG2E, dtype=torch.float32)
        kc = k * torch.tensor(0.044715, dtype=torch.float32)
        y = x * torch.addcmul(k, kc, x * x)
    else:
        y = torch.tensor(-_LOG2E, dtype=torch.float32) * x
    return (x * torch.reciprocal(1.0 + torch.exp2(y))).to(torch.bfloat16).float()


# ---------------------------------------------------------------------------
# SiLU . up probes
# ---------------------------------------------------------------------------
def silu_operands(a: torch.Tensor, w: torch.Tensor, which: str):
    """From integer a [M, K] and w [2F, K] (rows [:F] gate, [F:] up in the
    model's order): copies with column 0 of `a` set to 1 and the pinned half
    of w replaced -- "up" probe: gate = 32; "gate" probe: up = 1.  Returns
    (a, w, exact gate [M, F], exact up [M, F])."""
    F = w.shape[0] // 2
    a, w = a.clone(), w.clone()
    a[:, 0] = 1
    pin = slice(0, F) if which == "up" else slice(F, 2 * F)
    w[pin] = 0
    w[pin, 0] = 32 if which == "up" else 1
    y = exact_product(a, w)
    return a, w, y[:, :F], y[:, F:]


# ---------------------------------------------------------------------------
# fused-norm GEMV probe
# ---------------------------------------------------------------------------
def norm_case(M: int, N: int, K: int, rms: bool, eps: float, seed: int = 0, bf16_out: bool = True):
    """x fp32 [M, K] (balanced +-1 rows), gamma, beta (None for RMSNorm), w
    [N, K], bias [N] as int64 / fp32, and the exact y = (x gamma + beta) w^T.
    w is thinned so a bf16 output stays <= 256 (asserted by the caller's
    assert_bf16_exact); the normalised row's exactness is asserted here."""
    assert K % 2 == 0
    g = _gen(seed + 17 * K + (1 if rms else 0))
    x = torch.stack([(torch.arange(K) % 2 * 2 - 1)[torch.randperm(K, generator=g)] for _ in range(M)])
    gamma = torch.randint(-1, 2, (K,), generator=g)
    beta = None if rms else 2 * torch.randint(-1, 2, (K,), generator=g)
    xn = x * gamma[None, :] + (0 if rms else beta[None, :])
    # E[xn^2] = 2/3 (+ 8/3 with beta), E[w^2] = 2 p: variance K 2 p E[xn^2] <= 1600
    dens = min(1.0, VAR_TARGET / (K * 2.0 * (2.0 / 3.0 if rms else 10.0 / 3.0))) if bf16_out else 1.0
    w = torch.randint(-2, 3, (N, K), generator=g)
    if dens < 1.0:
        w = w * (torch.rand(N, K, generator=g) < dens)
    bias = torch.randint(-8, 9, (N,), generator=g)
    for pert in (-2e-4, 0.0, 2e-4):  # the kernel's statistics may differ by a few ulps: far inside
        xf = x.float()
        mean = torch.zeros(M, 1) if rms else xf.mean(-1, keepdim=True)
        var = ((xf - mean) ** 2).mean(-1, keepdim=True)
        rstd = torch.rsqrt(var + eps) * (1.0 + pert)
        z = (xf - mean) * rstd * gamma.float()[None, :]
        if not rms:
            z = z + beta.float()[None, :]
        assert torch.equal(z.to(torch.bfloat16).double(), xn.double()), "normalised row is not exact"
    return x.float(), gamma, beta, w, bias, exact_product(xn, w)


# ---------------------------------------------------------------------------
# fp32 emulation with fault knobs
# ---------------------------------------------------------------------------
FAULTS = {"drop_k", "drop_chunk", "repeat_kstep", "omit_split", "repeat_split", "partials_bf16",
          "bias_per_split", "swap_cols", "interleave_shift", "rope_pos", "rope_pair", "rope_sign",
          "kv_pos", "kv_slot", "read_past_k", "write_past_m"}


def _bf(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).float()


def _wider(t: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    """t's storage seen `rows` rows / `cols` columns larger (a view into the
    buffer t was cut from)."""
    return t.as_strided((t.shape[0] + rows, t.shape[1] + cols), t.stride(), t.storage_offset())


def emulate(a, w, bias=None, *, epi: str = "bf16", splits: int = 1, step: int = 32, x=None, slab_dtype=None,
            qkv=None, fault=None):
    """fp32 GEMM a [M, K] . w [N, K]^T with the kernels' epilogues, on CPU.

    epi: "bf16", "gelu", "silu" (w interleaved by interleave_gate_up), "f32"
    (returns out and segmax), "resid" (x updated in place), "slab" (returns the
    [splits, M, N] slab of slab_dtype), "qkv" (qkv = dict(tslot, tpos, kc, vc,
    table or None); returns q, caches updated in place).
    fault: None, a name, a (name, arg) pair or a list of those --
      ("drop_k", (m, k))          one k not counted for row m
      ("drop_chunk", (m0, n, k0)) k0 .. k0 + 8 not counted for rows m0 .. m0 + 4 of column n
      ("repeat_kstep", k0)        k0 .. k0 + 32 counted twice
      ("omit_split", s) / ("repeat_split", s)
      "partials_bf16"             every split's partial rounded to bf16 before the sum
      "bias_per_split"            bias added once per split
      ("swap_cols", (n1, n2))     two output columns exchanged
      "interleave_shift"          SiLU: up taken from the next 32-row block
      "rope_pos" / "rope_pair" / "rope_sign"   table read at pos + 1 / pair + 1 / sin negated
      "kv_pos" / "kv_slot"        KV row written to pos + 1 / slot + 1
      ("read_past_k", m)          a[m, K] w[:, K] (one element past the row) counted
      "write_past_m"              row M - 1's result also written to row M
    Returns a dict of fp32 tensors."""
    faults = fault if isinstance(fault, list) else ([] if fault is None else [fault])
    f = dict((x_, None) if isinstance(x_, str) else tuple(x_) for x_ in faults)
    assert set(f) <= FAULTS, f
    af, wf = a.float(), w.float()
    M, K = af.shape
    N = wf.shape[0]
    parts = []
    for s, (k0, k1) in enumerate(split_bounds(K, splits, step)):
        p = af[:, k0:k1] @ wf[:, k0:k1].t()
        if "drop_k" in f and k0 <= f["drop_k"][1] < k1:
            m, k = f["drop_k"]
            p[m] -= af[m, k] * wf[:, k]
        if "drop_chunk" in f and k0 <= f["drop_chunk"][2] < k1:
            m0, n, kk = f["drop_chunk"]
            p[m0:m0 + 4, n] -= af[m0:m0 + 4, kk:kk + 8] @ wf[n, kk:kk + 8]
        if "repeat_kstep" in f and k0 <= f["repeat_kstep"] < k1:
            kk = f["repeat_kstep"]
            p += af[:, kk:kk + 32] @ wf[:, kk:kk + 32].t()
        if "read_past_k" in f and k1 == K:
            m = f["read_past_k"]
            p[m] += _wider(a, 0, 1)[m, K].float() * _wider(w, 0, 1)[:, K].float()
        parts.append(p)
    if "omit_split" in f:
        parts[f["omit_split"]] = torch.zeros(M, N)
    if "repeat_split" in f:
        parts.append(parts[f["repeat_split"]])
    if "partials_bf16" in f:
        parts = [_bf(p) for p in parts]
    if "swap_cols" in f:
        n1, n2 = f["swap_cols"]
        for p in parts:
            p[:, [n1, n2]] = p[:, [n2, n1]]
    if epi == "slab":
        if "repeat_split" in f:  # the split's partial lands in the next slab as well
            parts[(f["repeat_split"] + 1) % splits] = parts[f["repeat_split"]]
        slab = torch.stack(parts[:splits])
        return {"slab": slab.to(slab_dtype or torch.float32).float()}
    acc = torch.zeros(M, N)
    for p in parts:
        acc = acc + p
    b = torch.zeros(N) if bias is None else bias.float()
    y = acc + b * (len(parts) if "bias_per_split" in f else 1)
    if epi == "bf16":
        return {"out": _bf(y)}
    if epi == "gelu":
        return {"out": act_emulate("gelu", y)}
    if epi == "f32":
        return {"out": acc, "segmax": segmax_expected(acc)}
    if epi == "resid":
        xw = _wider(x, 1, 0) if "write_past_m" in f else x
        x += y
        if "write_past_m" in f:
            xw[M] = xw[M - 1]
        return {"x": x}
    if epi == "silu":
        blk = acc.reshape(M, N // 32, 2, 16)
        gate, up = blk[:, :, 0], blk[:, :, 1]
        if "interleave_shift" in f:
            up = up.roll(-1, 1)
        sg = gate * torch.reciprocal(1.0 + torch.exp2(torch.tensor(-_LOG2E, dtype=torch.float32) * gate))
        return {"out": _bf(sg * up).reshape(M, N // 2)}
    assert epi == "qkv"
    tslot, tpos, kc, vc, table = (qkv[k] for k in ("tslot", "tpos", "kc", "vc", "table"))
    qs, kvs, hd, nh, nkv = qkv["dims"] if "dims" in qkv else qkv_dims(N)
    tslot, tpos = tslot.long(), tpos.long()
    if table is not None:
        half = hd // 2
        n = torch.arange(qs + kvs)
        d = torch.where(n < qs, n, n - qs) % hd
        pair = ((d >> 1) + (1 if "rope_pair" in f else 0)) % half
        cs = table.float()[(tpos + (1 if "rope_pos" in f else 0))[:, None], pair[None, :]]  # [M, qk, 2]
        c, s = cs[..., 0], cs[..., 1] * (-1.0 if "rope_sign" in f else 1.0)
        v = y[:, :qs + kvs]
        partner = v.reshape(M, -1, 2).flip(-1).reshape(M, -1)
        odd = (d & 1).bool()[None, :]
        y = torch.cat([torch.where(odd, v * c + partner * s, v * c - partner * s), y[:, qs + kvs:]], 1)
    yb = _bf(y)
    ps = tpos + (1 if "kv_pos" in f else 0)
    sl = (tslot + 1) % kc.shape[0] if "kv_slot" in f else tslot
    kc[sl, :, ps] = yb[:, qs:qs + kvs].reshape(M, nkv, hd).to(kc.dtype)
    vc[sl, :, ps] = yb[:, qs + kvs:].reshape(M, nkv, hd).to(vc.dtype)
    return {"q": yb[:, :qs]}
