"""Exact-arithmetic probes for the norm kernels of csrc/kernels/norm.hip (the
split-K slab fold, the block-per-row and the wave-per-row LayerNorm / RMSNorm)
(pure torch, CPU or GPU).

Random rows of variance 1 with `close(..., 2e-2)` cannot see a missing `eps`,
a 16-byte chunk dropped from the statistics at H = 768, a divisor off by one
chunk, or (zero-mean rows at H = 8192) a mean that is never subtracted
(tests/test_norm_probes.py pins all four).  The inputs built here have answers
that are one bit pattern, or a closed form with a bound that comes from the
number formats.

What the kernels compute.  x[t] += pending bias + sum_s slab[s][t] (fp32,
written back), then y = (x - mean) rsqrt(var + eps) gamma + beta rounded to
bf16 (RMSNorm: mean = 0, var = sum x^2 / H, no beta).  LayerNorm statistics:
every thread takes the exact two-pass (count, mean, M2) of its own 4 MAXV (block
kernel: chunks thread + 256 i) or 4 MAXC (wave kernel: chunks lane + 64 i)
values, and the (n, m, M) triples are merged pairwise (Chan):
    n = na + nb,  m = (na ma + nb mb) / n,  M = Ma + Mb + (mb - ma)^2 na nb / n.
Lanes past the row load a clamped duplicate chunk (the last one) and a
separate guard keeps it out of the sums.

fold      x, the pending bias and bf16 slabs are integers code(.) in
          [-125, 125] (gemm_probes.code: (i % 251) - 125); fp32 slabs are
          1024 code(.) + code(.), 18 significant bits, so a slab rounded to
          bf16 on the way is a wrong integer.  The index coded is 131 split +
          29 row + column: a wrong split, row (or row stride) or column moves
          it by a non-multiple of 251.  |x| + 12 (1024 * 125 + 125) + 125 =
          1.54e6 < 2^24 (asserted), so every partial sum in any order is an
          exact fp32 integer and the folded residual has one bit pattern.
sign      rows are a balanced permutation of +-1 (another one per row): mean
          0, variance 1, rstd = rsqrt(1 + 1e-5) = 1 - 5e-6.  "wide": gamma =
          code(column) (so a gamma read from another column is another
          integer), beta = 0; y = +-rstd gamma lies within 125 * 5e-6 of an
          integer of magnitude <= 125, where bf16 numbers are >= 1/2 apart for
          |y| >= 64 and integers are bf16 numbers: it rounds to x gamma.
          "beta" (LayerNorm): gamma in {-1, 0, 1}, beta in {-2, 0, 2}, as the
          fused-norm GEMV probe of gemm_probes.  `sign_case` asserts the
          exactness from the fp32 emulation with rstd moved by +-2e-4.
offset    the same rows + 1024 (LayerNorm): 1023 and 1025 are fp32 numbers, a
          thread's sum of <= 32 of them is an exact integer, its mean is off
          by at most half an ulp of 1024 (6e-5) and its M2, taken about that
          mean, by count * 6e-5^2; the merges see means that differ by ~1 /
          sqrt(n) with that error, 1e-4 relative on M at the worst -- inside
          the 2e-3 that the bf16 rounding of 125 rstd leaves.  One-pass
          E[x^2] - m^2 subtracts 1048577 - 1048576 with an fp32 ulp of 1/8
          there: once a sum of squares passes 2^24 (more than 16 values in
          one sum: 1025^2 is odd) it is rounded and the variance is no
          longer 1.  Below that -- H = 8, or groups of 4 .. 12 whose partial
          sums happen to stay representable -- one-pass arithmetic is exact
          too and nothing can tell it apart (pinned in the CPU test); on
          the kernels that is MAXV 2 and 4 and MAXC 4.  A larger offset
          does not help: from 4096 on every merge rounds n m to 24 bits and
          the two-pass mean itself drifts by 2e-3, past what bf16 forgives.
          Asserted from the emulation at every group size like the sign probe.
eps       rows are a balanced +-2^-12: var = 2^-24 = 6e-8, so rstd =
          rsqrt(2^-24 + eps) is eps's doing (316 at 1e-5, 31.6 at 1e-3; 4096
          without eps, 13 times more; eps outside the root gives 4086).
          Expected x rstd gamma in fp64, tolerance 2^-8 relative: the bf16
          store is half a spacing of 2^-7 at the bottom of a binade, at most
          2^-8 / (1 + 2^-8) = 2^-8 - 2^-16 relative, and the fp32 terms
          (rsqrtf 2^-23, three products 2^-24 each, the variance through the
          merges < 2^-20) fit into the 2^-16 = 1.5e-5 that leaves.
energy    row r is zero except for chunk r and its partner chunk (r + nch / 2)
          % nch (nch = H / 4 chunks, one row per chunk, T = nch): (v, -v, v,
          -v) and (-v, v, -v, v) balanced; "unbalanced" (LayerNorm) all v in
          chunk r and all -v / 2 in the partner, mean v / (2 nch) (one chunk
          when nch = 1: (v, -v, v, -v) / (v, -v/2, v, -v/2)).  gamma =
          code(column), zeros replaced by 1.  Expected from the fp64 mean and
          variance of the row, 2^-8 relative.  A chunk dropped from the
          sums halves the balanced energy (rstd x sqrt 2 = +41 %), a
          duplicate counted adds a half (x sqrt(2/3) = -18 %); a divisor that
          counts loaded elements (H + 4) is sqrt(12 / 8) = +22 % at H = 8 and
          certain to show while 2 / H > 2^-8 (H < 512); the null probe takes
          over above.
null      (LayerNorm) every row is the same balanced +-1 pattern s, gamma =
          128, beta = -128 s.  With y = s rstd the kernel computes z = 128 y -
          128 s: 128 y is exact (a power of two), and the subtraction of two
          numbers within a factor of two is exact (Sterbenz), so z = 128 s
          (rstd' - 1) for whatever rstd' the kernel got -- -6.4e-4 s at eps =
          1e-5, where bf16 numbers are 2^-19 apart.  Error terms, relative to
          |y| ~ 1, u = 2^-25:
              rsqrtf, 1 ulp of the binade of 1                    4 u
              var + eps rounded in [1, 2): 2^-24, halved by the root   1 u
              x - mean, and its product with rstd, below 1: 2^-25 each  2 u
              statistics: |mean'| + |var' - 1| / 2                 <= 9 u
          and the sum is 2^-21: NULL_ABS = 128 * 2^-21 = 6.1e-5, plus the bf16
          store, 2^-9 of |z| (1.2e-6 at eps = 1e-5; 1.2e-4 at 1e-3, where z =
          -0.064 and the probe is that much coarser).  The statistics' share
          is not a worst case over all rows (ten merge levels of arbitrary
          data give ~40 u) but a property of these rows: sums of +-1 are
          exact integers, a group mean is an integer over its count -- exact
          for the power-of-two counts of every full thread -- and deviations
          and their squares are short dyadic fractions.  `null_case` asserts
          it on the CPU: in the emulation, at every group size 4 .. 32 and
          both kernels' own layouts, |mean'| + |var' - 1| / 2 stays within
          half the share, 4.5 u (3.1 u is the most seen: the variance 1.5 ulp
          from 1), before the probe is trusted.  What
          a relative rstd error of 5e-7 looks like: a divisor of H + 4 at H =
          8192 (2.4e-4), an eps 10 % off at 1e-5 (5.0e-7: 6.4e-5 against 6.2e-5,
          on the edge; 15 % is seen from both sides), a mean off by 5e-7.
isolation any probe's rows interleaved with rows of NaN (the slabs likewise):
          the clean rows must come out bit-equal to a launch without them.
guards    x is the first T rows of a larger buffer whose other rows hold
          SENTINEL; the whole buffer is compared after the launch.

Blind spot, pinned in the CPU test: RMSNorm has no beta, so its output is
rstd times something and an rstd error under 2^-9 relative can hide inside
the bf16 rounding for any input; no null probe exists for it.  The energy
probe at H = 8 and 12 is what bounds a wrong divisor there.

`emulate` is an fp32 CPU model of fold + norm with the statistics computed the
kernels' way and a knob per fault (FAULTS); tests/test_norm_probes.py shows
each checker accepts it fault-free at every group size and rejects the faults
meant for it.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

from .gemm_probes import SENTINEL, _gen, bits_equal, code, guarded  # noqa: F401  (re-exported for the tests)

BF = torch.bfloat16
REL_TOL = 2.0 ** -8            # eps and energy probes
NULL_ABS = 128.0 * 2.0 ** -21  # null probe, before the bf16 store's share
GROUPS = (4, 8, 12, 16, 20, 24, 28, 32, "block", "wave")


def _bf(t: torch.Tensor) -> torch.Tensor:
    return t.to(BF).float()


def balanced_rows(T: int, H: int, seed: int = 0, same: bool = False) -> torch.Tensor:
    """[T, H] fp32 rows, each a permutation of H/2 times +1 and H/2 times -1."""
    assert H % 2 == 0
    g = _gen(seed + 13 * H)
    base = (torch.arange(H) % 2 * 2 - 1).float()
    if same:
        return base[torch.randperm(H, generator=g)].expand(T, H).contiguous()
    return torch.stack([base[torch.randperm(H, generator=g)] for _ in range(T)])


def col_code(H: int, nonzero: bool = False) -> torch.Tensor:
    c = code(torch.arange(H)).float()
    return torch.where(c == 0, torch.ones(()), c) if nonzero else c


# ---------------------------------------------------------------------------
# input builders
# ---------------------------------------------------------------------------
def fold_case(T: int, H: int, S: int, slab_dtype=torch.float32, bias: bool = True):
    """x fp32 [T, H], slab [S, T, H] (None when S = 0), pbias bf16 [H] or None,
    and the exact folded residual `x_exp` (fp32)."""
    t, c = torch.arange(T)[:, None], torch.arange(H)[None, :]
    x = code(59 * t + c + 11)
    slab = pb = None
    total = x.clone()
    if S:
        s = torch.arange(S)[:, None, None]
        k = 131 * s + 29 * t[None] + c[None]
        slab = code(k) if slab_dtype == BF else 1024 * code(k) + code(7 * k + 3)
        assert slab_dtype != BF or int(slab.abs().max()) <= 256
        total = total + slab.sum(0)
        if bias:
            pb = code(3 * torch.arange(H) + 5)
            total = total + pb[None, :]
        worst = int(x.abs().max()) + int(slab.abs().sum(0).max()) + (125 if bias else 0)
        assert worst < 2 ** 24, worst  # every partial sum, in any order, is an exact fp32 integer
        slab = slab.to(slab_dtype)
        pb = None if pb is None else pb.to(BF)
    return SimpleNamespace(x=x.float(), slab=slab, pbias=pb, x_exp=total.float())


def _assert_exact(c, rms, eps, what):
    """The expected bf16 bits hold for the fp32 emulation at every group size
    and with rstd moved by +-2e-4 (the kernel's own few ulps are far inside)."""
    for group in GROUPS:
        for pert in (-2e-4, 0.0, 2e-4):
            out = emulate(c.x.clone(), c.w, c.b, rms=rms, eps=eps, group=group, fault=("rstd_scale", 1.0 + pert))["out"]
            assert bits_equal(out, c.out_exp), f"{what} probe is not exact (group {group}, rstd {pert:+g})"


def sign_case(T: int, H: int, rms: bool, kind: str = "wide", eps: float = 1e-5, seed: int = 0, check: bool = True):
    """Balanced +-1 rows; kind "wide": gamma = code(column), beta = 0; "beta"
    (LayerNorm): gamma in {-1, 0, 1}, beta in {-2, 0, 2}.  out_exp bf16."""
    x = balanced_rows(T, H, seed)
    g = _gen(seed + 7 * H + 1)
    if kind == "wide":
        w, b = col_code(H), torch.zeros(H)
    else:
        assert kind == "beta" and not rms
        w = torch.randint(-1, 2, (H,), generator=g).float()
        b = 2.0 * torch.randint(-1, 2, (H,), generator=g).float()
    c = SimpleNamespace(x=x, w=w.to(BF), b=None if rms else b.to(BF), out_exp=(x * w if rms else x * w + b).to(BF))  # RMSNorm: -1 * 0 = -0 stays
    if check:
        _assert_exact(c, rms, eps, "sign")
    return c


def offset_case(T: int, H: int, kind: str = "wide", eps: float = 1e-5, seed: int = 0, check: bool = True):
    """sign_case's LayerNorm rows + 1024; the same expected output."""
    c = sign_case(T, H, False, kind, eps, seed, check=False)
    c.x = c.x + 1024.0
    if check:
        _assert_exact(c, False, eps, "offset")
    return c


def eps_case(T: int, H: int, rms: bool, eps: float, seed: int = 0):
    """Balanced +-2^-12 rows, gamma = code(column), beta 0; `exp` fp64."""
    x = balanced_rows(T, H, seed + 1) * 2.0 ** -12
    w = col_code(H)
    exp = x.double() * w.double() / math.sqrt(2.0 ** -24 + eps)
    return SimpleNamespace(x=x, w=w.to(BF), b=None if rms else torch.zeros(H, dtype=BF), exp=exp)


def energy_case(H: int, rms: bool, unbalanced: bool = False, v: float = 3.0, eps: float = 1e-5, device="cpu"):
    """One row per 16-byte chunk (T = H / 4), see the module docstring; `exp`
    fp64 from the row's fp64 mean and variance (computed on `device`, where x
    and exp stay: 2048 rows at H = 8192)."""
    assert H % 4 == 0 and not (rms and unbalanced)
    nch = H // 4
    x = torch.zeros(nch, nch, 4)
    r = torch.arange(nch)
    alt = torch.tensor([1.0, -1.0, 1.0, -1.0])
    if nch == 1:
        x[0, 0] = v * (torch.tensor([1.0, -0.5, 1.0, -0.5]) if unbalanced else alt)
    else:
        x[r, r] = v * (torch.ones(4) if unbalanced else alt)
        x[r, (r + nch // 2) % nch] = v * (-0.5 * torch.ones(4) if unbalanced else -alt)
    x = x.reshape(nch, H).to(device)
    w = col_code(H, nonzero=True).to(device)
    xd = x.double()
    mean = torch.zeros(nch, 1, dtype=torch.float64, device=device) if rms else xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(-1, keepdim=True)
    exp = (xd - mean) / torch.sqrt(var + eps) * w.double()
    return SimpleNamespace(x=x, w=w.to(BF), b=None if rms else torch.zeros(H, dtype=BF, device=device), exp=exp)


def null_case(T: int, H: int, eps: float, seed: int = 0, check: bool = True):
    """(LayerNorm) identical balanced +-1 rows, gamma = 128, beta = -128 sign:
    `exp` = 128 (rstd - 1) sign in fp64 and the absolute `bound`."""
    x = balanced_rows(T, H, seed + 2, same=True)
    z = 128.0 * (1.0 / math.sqrt(1.0 + eps) - 1.0)
    c = SimpleNamespace(x=x, w=torch.full((H,), 128.0, dtype=BF), b=(-128.0 * x[0]).to(BF), exp=z * x.double(),
                        bound=NULL_ABS * (1.0 + 2.0 ** -9) + 2.0 ** -9 * abs(z))
    if check:  # the statistics' share of the bound (9 u, u = 2^-25) is a property of these rows
        for group in GROUPS:
            mean, var = _ln_stats(x[:1], _layout(H, group), H, {})
            assert abs(float(mean)) + abs(float(var) - 1.0) / 2 <= 4.5 * 2.0 ** -25, (group, mean, var)
    return c


def interleave_nan(t: torch.Tensor, dim: int = 0) -> torch.Tensor:
    """Rows 2 i of the result are t's rows i, rows 2 i + 1 are NaN."""
    out = torch.full_like(torch.cat([t, t], dim), float("nan"))
    out.index_copy_(dim, torch.arange(0, 2 * t.shape[dim], 2, device=t.device), t)
    return out


# ---------------------------------------------------------------------------
# checkers
# ---------------------------------------------------------------------------
def rel_err(out: torch.Tensor, exp: torch.Tensor) -> float:
    """max |out - exp| / |exp| (0 / 0 = 0, anything else over 0 or not finite
    = inf).  The eps and energy probes pass iff <= REL_TOL."""
    o = out.detach().double().reshape(exp.shape)
    e = exp.detach().double().to(o.device)
    if not bool(torch.isfinite(o).all()):
        return math.inf
    d = (o - e).abs()
    r = torch.where(e == 0, torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, math.inf)), d / e.abs())
    return float(r.max()) if r.numel() else 0.0


def null_ratio(out: torch.Tensor, c) -> float:
    """max |out - exp| / bound of the null probe; passes iff <= 1."""
    o = out.detach().double().reshape(c.exp.shape)
    if not bool(torch.isfinite(o).all()):
        return math.inf
    return float((o - c.exp.to(o.device)).abs().max()) / c.bound


# ---------------------------------------------------------------------------
# fp32 emulation with fault knobs
# ---------------------------------------------------------------------------
FAULTS = {"drop_chunk", "dup_chunk", "divisor", "eps_omit", "eps_outside", "no_mean", "one_pass", "gamma_shift",
          "beta_omit", "omit_split", "repeat_split", "pbias_omit", "pbias_per_split", "slab_stride", "slab_as_bf16",
          "no_writeback", "write_no_slab", "ignore_rows", "write_past_T", "rstd_scale", "eps_scale", "mean_bias"}


def _layout(H: int, group) -> torch.Tensor:
    """[P, G] column indices of P threads' values, -1 where a thread has none.
    group: an int (consecutive groups of that many columns), "block" (thread p
    of 256 holds chunks p + 256 i, i < MAXV) or "wave" (lane p of 64, chunks p
    + 64 i, i < MAXC)."""
    if group == "block" or group == "wave":
        nch = H // 4
        P = 256 if group == "block" else 64
        n = -(-max(nch, 1) // P)
        n = next(m for m in ((2, 4, 8) if group == "block" else (4, 8, 16, 32)) if m >= n)
        chunk = torch.arange(P)[:, None] + P * torch.arange(n)[None, :]
        idx = (4 * chunk[:, :, None] + torch.arange(4)[None, None, :]).reshape(P, 4 * n)
    else:
        P = -(-H // group)
        idx = torch.arange(P * group).reshape(P, group)
    return torch.where(idx < H, idx, torch.full_like(idx, -1))


def _gather(x, idx):
    mask = (idx >= 0)
    return x[:, idx.clamp(min=0)] * mask, mask


def _ln_stats(x, idx, H, f):
    """(mean [T, 1], var [T, 1]) in fp32 the kernels' way."""
    g, mask = _gather(x, idx)
    n = mask.sum(-1).float()                                    # [P]
    s1 = g.sum(-1)
    if "one_pass" in f:  # every add an fp32 add: sequential per thread, then a pairwise tree
        acc = torch.zeros_like(g[..., 0])
        for j in range(g.shape[-1]):
            acc = acc + g[..., j] * g[..., j]
        while acc.shape[1] > 1:
            if acc.shape[1] % 2:
                acc = torch.cat([acc, torch.zeros_like(acc[:, :1])], 1)
            acc = acc[:, 0::2] + acc[:, 1::2]
        mean = s1.sum(-1, keepdim=True) / H
        return mean, acc / H - mean * mean
    m = torch.where(n > 0, s1 / n.clamp(min=1.0), torch.zeros(()))
    d = (g - m[..., None]) * mask
    M = (d * d).sum(-1)
    P = 1 << max(0, (idx.shape[0] - 1).bit_length())
    pad = P - idx.shape[0]
    n = torch.cat([n, torch.zeros(pad)])[None, :].expand(x.shape[0], P)
    m, M = (torch.cat([t, torch.zeros(x.shape[0], pad)], 1) for t in (m, M))
    while n.shape[1] > 1:  # Chan merges, neighbours first
        na, nb, ma, mb, Ma, Mb = n[:, 0::2], n[:, 1::2], m[:, 0::2], m[:, 1::2], M[:, 0::2], M[:, 1::2]
        nn = na + nb
        rn = 1.0 / nn.clamp(min=1.0)
        dd = mb - ma
        keep = nn == 0
        m = torch.where(keep, ma, (na * ma + nb * mb) * rn)
        M = torch.where(keep, Ma, Ma + Mb + dd * dd * (na * nb) * rn)
        n = nn
    return m, M / float(H + f.get("divisor", 0))


def emulate(x, w=None, b=None, *, rms: bool, eps: float = 1e-5, group=8, slab=None, pbias=None, rows=None,
            want_out: bool = True, fault=None):
    """fp32 CPU model of lsd_norm: folds `slab` [S, T, H] and `pbias` into x
    IN PLACE (x fp32 [T, H], possibly a view of a larger buffer), then norms
    rows `rows` (all when None).  Returns {"out": bf16 [n, H] or None}.
    fault: None, a name, a (name, arg) pair or a list of those --
      ("drop_chunk", c)      chunk c (columns 4 c .. 4 c + 3) left out of the statistics
      "dup_chunk"            the clamped duplicate of the last chunk counted as well
      ("divisor", d)         variance divided by H + d ("divisor" alone: the loaded H + 4)
      "eps_omit" / "eps_outside"   rsqrt(var) / 1 / (sqrt(var) + eps)
      "no_mean"              the mean is not subtracted from the row
      "one_pass"             var = E[x^2] - mean^2
      "gamma_shift"          gamma read one chunk later
      "beta_omit"
      ("omit_split", s) / ("repeat_split", s)
      "pbias_omit" / "pbias_per_split"
      "slab_stride"          slab rows addressed with T - 1 rows per split
      "slab_as_bf16"         an fp32 slab's bytes read as bf16
      "no_writeback"         the folded row is normed but not stored
      "write_no_slab"        the slab-free path stores the row it loaded at x[t] (visible under a row gather)
      "ignore_rows"          t used for rows[t]
      "write_past_T"         row T - 1's folded residual also stored at row T
      ("rstd_scale", k) / ("eps_scale", k) / ("mean_bias", d)   sensitivity knobs"""
    faults = fault if isinstance(fault, list) else ([] if fault is None else [fault])
    f = dict((x_, None) if isinstance(x_, str) else tuple(x_) for x_ in faults)
    assert set(f) <= FAULTS, f
    if "divisor" in f and f["divisor"] is None:
        f["divisor"] = 4
    T, H = x.shape
    if slab is not None:
        S = slab.shape[0]
        if "slab_as_bf16" in f:
            assert slab.dtype == torch.float32
            parts = slab.contiguous().view(BF).flatten()[:S * T * H].reshape(S, T, H).float()
        elif "slab_stride" in f:
            flat = slab.float().flatten()
            k = ((torch.arange(S)[:, None, None] * (T - 1) + torch.arange(T)[None, :, None]) * H
                 + torch.arange(H)[None, None, :])
            parts = flat[k]
        else:
            parts = slab.float()
        a = x.clone()
        n_added = 0
        for s in list(range(S)) + ([f["repeat_split"]] if "repeat_split" in f else []):
            if f.get("omit_split", -1) == s and "omit_split" in f:
                continue
            a = a + parts[s]
            n_added += 1
        if pbias is not None and "pbias_omit" not in f:
            a = a + pbias.float()[None, :] * (n_added if "pbias_per_split" in f else 1)
        if "write_past_T" in f:
            x.as_strided((T + 1, H), x.stride(), x.storage_offset())[T] = a[T - 1]
        if "no_writeback" not in f:
            x.copy_(a)
    else:
        a = x
    if not want_out:
        return {"out": None}
    src = torch.arange(T) if rows is None else rows.long()
    if "ignore_rows" in f:
        src = torch.arange(src.numel())
    v = a[src].clone()
    if slab is None and "write_no_slab" in f:
        x[:src.numel()] = v
    idx = _layout(H, group)
    if "drop_chunk" in f:
        c = f["drop_chunk"]
        idx = torch.where((idx >= 4 * c) & (idx < 4 * c + 4), torch.full_like(idx, -1), idx)
    if "dup_chunk" in f:
        extra = torch.full((1, idx.shape[1]), -1)
        extra[0, :4] = torch.arange(H - 4, H)
        idx = torch.cat([idx, extra])
    if rms:
        g, _ = _gather(v, idx)
        mean = torch.zeros(v.shape[0], 1)
        var = (g * g).sum(-1).sum(-1, keepdim=True) / float(H + f.get("divisor", 0))
    else:
        mean, var = _ln_stats(v, idx, H, f)
        mean = mean + torch.tensor(f.get("mean_bias", 0.0), dtype=torch.float32)
    e = torch.tensor(eps * f.get("eps_scale", 1.0), dtype=torch.float32)
    if "eps_omit" in f:
        rstd = torch.rsqrt(var)
    elif "eps_outside" in f:
        rstd = 1.0 / (torch.sqrt(var) + e)
    else:
        rstd = torch.rsqrt(var + e)
    rstd = rstd * torch.tensor(f.get("rstd_scale", 1.0), dtype=torch.float32)
    y = (v if "no_mean" in f else v - mean) * rstd
    gamma = w.float()
    if "gamma_shift" in f:
        gamma = gamma.roll(-4)
    z = y * gamma[None, :]
    if not rms and "beta_omit" not in f:
        z = z + b.float()[None, :]
    return {"out": z.to(BF)}
