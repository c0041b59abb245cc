"""The attention probes test themselves (CPU): every checker of
tests/attention_probes.py accepts the fault-free fp32 emulation -- plain, and
with P rounded to bf16 as the MFMA kernels do -- at the shapes the GPU module
uses, and rejects the injected faults it is meant for.

One blind spot is inherent and asserted here rather than hidden: at a context
that is a multiple of the head dim the count probe's expectation is uniform
over d, so a wrong kv head (a rotation of V's one-hot pattern) is invisible to
it; the needle probe rejects that fault at every context.
"""
import functools

import pytest
import torch

from . import attention_probes as ap

STYLES = [None, "p_bf16"]


def _rows(n, step):
    """Every row of the small contexts, a stride over the rest: the CPU
    emulation of a whole needle sweep would take most of this file's time."""
    idx = torch.arange(n)
    return idx[(idx < 200) | (idx % step == 0)]


SWEEP_SHAPES = sorted(set(ap.VALU_SHAPES + ap.MFMA_SHAPES + ap.OPROJ_SHAPES))


@pytest.mark.parametrize("hd,nh,n_kv", SWEEP_SHAPES)
def test_count_sweep_accepts_emulation(hd, nh, n_kv):
    q, kc, vc, slots, ctx, exp = ap.count_sweep(hd, nh, n_kv)
    for style in STYLES:
        o32 = ap.emulate(q, kc, vc, slots, ctx, style, torch.float32)  # the fused kernel's output format
        r = ap.count_ratio(o32, exp, ap.COUNT_REL_FP32)
        assert r <= 1.0, (style, r)
        r = ap.count_ratio(o32.bfloat16().float(), exp)
        assert r <= 1.0, (style, r)


@pytest.mark.parametrize("hd,nh,n_kv", SWEEP_SHAPES)
def test_needle_sweep_accepts_emulation(hd, nh, n_kv):
    q, kc, vc, slots, ctx, needles, exp = ap.needle_sweep(hd, nh, n_kv)
    rest = ap.needle_rest(kc, vc, slots, needles)
    assert rest < ap.NEEDLE_REST_FP32 < ap.NEEDLE_REST_BF16, rest
    sel = _rows(ctx.numel(), 1 if (hd, nh) == (64, 4) else 29)
    for style in STYLES:
        out = ap.emulate(q[sel], kc, vc, slots[sel], ctx[sel], style)
        assert torch.equal(out, exp[sel].float()), style
    out = ap.emulate(q[sel], kc, vc, slots[sel], ctx[sel], None, torch.float32)
    assert torch.equal(out, exp[sel].float())  # the fused kernel's fp32 output


@pytest.mark.parametrize("hd,nh,n_kv", ap.PREFILL_SHAPES)
def test_prefill_cases_accept_emulation(hd, nh, n_kv):
    q, kc, vc, slots, ctx, exp = ap.prefill_count(hd, nh, n_kv)
    assert q.shape[0] == sum(n for _, _, n in ap.PREFILL_SEQS)
    for style in STYLES:
        assert ap.count_ratio(ap.emulate(q, kc, vc, slots, ctx, style), exp) <= 1.0
    q, kc, vc, slots, ctx, needles, exp = ap.prefill_needle(hd, nh, n_kv)
    assert bool((needles < ctx[:, None]).all()) and bool((needles[:, 0] == ctx - 1).all())
    assert ap.needle_rest(kc, vc, slots, needles) < ap.NEEDLE_REST_BF16
    for style in STYLES:
        assert torch.equal(ap.emulate(q, kc, vc, slots, ctx, style), exp.float())


@pytest.mark.parametrize("B,nh,n_kv,hd,bucket", ap.ROUTED)
def test_routed_cases_accept_emulation(B, nh, n_kv, hd, bucket):
    kc, vc = ap.count_cache(2, n_kv, bucket, hd)
    kn, vn = ap.needle_cache(2, n_kv, bucket, hd)
    for slots, ctx, needles in ap.routed_rows(B, nh, bucket):
        assert sorted(set(ctx.tolist())) == ([1, bucket // 2, bucket] if B > 1 else ctx.tolist())
        assert ap.needle_rest(kn, vn, slots, needles) < ap.NEEDLE_REST_BF16
        q, exp = ap.needle_q(kn, slots, needles), ap.needle_expected(vn, slots, needles).float()
        for style in (STYLES if B != 8 else ["p_bf16"]):  # 8 rows of 8128 keys: the MFMA kernel's launch
            out = ap.emulate(torch.zeros_like(q), kc, vc, slots, ctx, style)
            assert ap.count_ratio(out, ap.count_expected(slots, ctx, nh, n_kv, hd)) <= 1.0
            assert torch.equal(ap.emulate(q, kn, vn, slots, ctx, style), exp)


@pytest.mark.parametrize("hd,n_kv,G", [(64, 4, 1), (64, 2, 4), (128, 4, 1), (128, 2, 2), (128, 4, 4), (128, 2, 8)])
def test_stale_tail(hd, n_kv, G):
    """Poison behind the context: invisible to a correct kernel, and the
    answer flips to -V[j*] as soon as one key past the end is counted."""
    q, kc, vc, slots, ctx, needles, exp, clean = ap.stale_tail_case(n_kv, G, hd, ap.STALE_CTX)
    assert ap.needle_rest(clean, vc, slots, needles, n_keys=int(ctx.max())) < ap.NEEDLE_REST_FP32
    for style in STYLES:
        assert torch.equal(ap.emulate(q, kc, vc, slots, ctx, style), exp.float())
    bad = ap.emulate(q, kc, vc, slots, ctx, "extra_key")
    for r in range(len(ap.STALE_CTX)):
        assert torch.equal(bad[r], -exp[r].float()), ctx[r]


@functools.lru_cache(maxsize=None)
def _count_cache(hd, n_kv):
    return ap.count_cache(2, n_kv, ap.S_PROBE + 1, hd)  # one position past the longest context, for extra_key


def _count_row(c, hd, nh, n_kv, fault):
    kc, vc = _count_cache(hd, n_kv)
    slots, ctx = torch.tensor([c % 2]), torch.tensor([c])
    q = torch.zeros(1, nh, hd, dtype=torch.bfloat16)
    return ap.count_ratio(ap.emulate(q, kc, vc, slots, ctx, fault), ap.count_expected(slots, ctx, nh, n_kv, hd))


@pytest.mark.parametrize("hd,nh,n_kv", [(64, 4, 4), (128, 8, 2)])
def test_count_checker_rejects_faults(hd, nh, n_kv):
    for c in ap.EDGE_CTX:
        assert _count_row(c, hd, nh, n_kv, None) <= 1.0
        faults = ["drop_last", ("drop_at", 0), ("drop_at", c // 2), "extra_key"]
        if c >= 2:
            faults += [("dup_at", 0), ("dup_at", c // 2), ("dup_at", c - 1)]
        if c % hd:  # uniform expectation otherwise: see the module docstring
            faults.append("wrong_kv_head")
        for f in faults:
            assert _count_row(c, hd, nh, n_kv, f) > 1.0, (c, f)
    for c in (hd, 2 * hd):  # the blind spot, pinned
        assert _count_row(c, hd, nh, n_kv, "wrong_kv_head") <= 1.0


def test_count_fault_margin_at_long_context():
    """One key at 1100 keys, hd 64: a relative error of at least
    (ctx - c) / (c (ctx - 1)) = 0.054 with c = 18, 14x the tolerance."""
    assert _count_row(1100, 64, 4, 4, "drop_last") > 10.0
    assert _count_row(1100, 64, 4, 4, ("dup_at", 600)) > 10.0


@pytest.mark.parametrize("hd,nh,n_kv", [(64, 4, 4), (128, 8, 2)])
def test_needle_checker_rejects_faults(hd, nh, n_kv):
    kc, vc = ap.needle_cache(2, n_kv, ap.S_PROBE, hd)
    for c in ap.EDGE_CTX:
        for j in sorted({0, c // 2, c - 1}):
            slots, ctx = torch.tensor([1]), torch.tensor([c])
            needles = torch.full((1, nh), j)
            q, exp = ap.needle_q(kc, slots, needles), ap.needle_expected(vc, slots, needles).float()
            assert torch.equal(ap.emulate(q, kc, vc, slots, ctx), exp)
            faults = [("drop_at", j), "wrong_kv_head"] + (["shift_v"] if c >= 2 else [])
            if j == c - 1:
                faults.append("drop_last")
            for f in faults:
                assert not torch.equal(ap.emulate(q, kc, vc, slots, ctx, f), exp), (c, j, f)


def _random_case(hd, nh, n_kv, ctxs, seed):
    g = torch.Generator().manual_seed(seed)
    B, S = len(ctxs), max(ctxs)
    kc = torch.randn(B, n_kv, S, hd, generator=g).bfloat16()
    vc = torch.randn(B, n_kv, S, hd, generator=g).bfloat16()
    q = torch.randn(B, nh, hd, generator=g).bfloat16()
    slots, ctx = torch.randperm(B, generator=g), torch.tensor(ctxs)
    o_ref, bound = ap.reference_and_bound(q, kc, vc, slots.int(), (ctx - 1).int(), torch.arange(B + 1).int())
    return q, kc, vc, slots, ctx, o_ref, bound


@pytest.mark.parametrize("hd,nh,n_kv,ctxs", [(64, 12, 12, (1, 18, 64, 141, 300)), (128, 8, 2, (1, 18, 64, 141, 300)),
                                             (128, 32, 8, (1, 8, 518, 1024, 1100))])
def test_bound_accepts_emulation_and_rejects_scale(hd, nh, n_kv, ctxs):
    q, kc, vc, slots, ctx, o_ref, bound = _random_case(hd, nh, n_kv, ctxs, 16)
    for style in STYLES:
        r = ap.bound_ratio(ap.emulate(q, kc, vc, slots, ctx, style), o_ref, bound)
        assert r <= 1.0, (style, r)
    bad = ap.emulate(q, kc, vc, slots, ctx, ("scale", 1.03)).double()
    per_head = ((bad - o_ref).abs() / bound).amax(-1)  # [rows, nh]
    assert float(per_head.max()) > 1.0
    if hd == 64:  # every head of every context from 18 to 300 keys (a context of 1 has no scale)
        assert bool((per_head[1:] > 1.0).all()), per_head[1:].min(1).values


def test_reference_keeps_fp64():
    q, kc, vc, slots, ctx, o_ref, bound = _random_case(64, 2, 2, (5, 40), 3)
    assert o_ref.dtype == torch.float64 and bound.dtype == torch.float64 and bool((bound > 0).all())
    o32 = ap.ref.attention(q, kc, vc, slots.int(), (ctx - 1).int(), torch.arange(3).int())
    assert o32.dtype == torch.float32
    torch.testing.assert_close(o32.double(), o_ref, atol=1e-5, rtol=1e-5)
