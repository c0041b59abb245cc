"""Exact-arithmetic probes of every attention kernel's key coverage on an
MI355X (tests/attention_probes.py; self-tested on the CPU by
tests/test_attention_probes.py).

count probe   q = 0 and one-hot V: the output is a closed-form count / ctx,
              so a dropped, doubled, stale or wrong-head key is an error of at
              least (ctx - c) / (c (ctx - 1)) against a tolerance of 2^-8 (the
              bf16 store) or 2^-20 (the fused kernel's fp32 output).
needle probe  one key outweighs all others by > 2^26: the output is bit-equal
              to that key's V row; every (context, needle) pair of the edge
              contexts rides in one launch.

Covered: the VALU decode kernel (every block shape x splits 1 / 3 / 16, every
context 1..1100 in one launch), the MFMA decode kernel, the split combine, the
prefill kernel, the fused attention + out-projection kernel, poison behind
the context (stale keys of an earlier sequence), a strided q, and the
launches the engine's routing picks.

Measured on an MI355X (bounds are derived, not measured; recorded so the next
rewrite can see its margin) -- largest err / bound of the count probe:
  VALU decode    0.992 of 2^-8   (127 / 128: the bf16 store's worst half-ulp;
  MFMA decode    0.992 of 2^-8    the fp32 emulation on the CPU gives the same
  prefill        0.992 of 2^-8    figure, so nothing but that rounding is left)
  fused o-proj   0.104 of 2^-20
Largest err / attention_bound on the random cases of test_kernels_gpu.py:
  VALU decode 0.496, MFMA decode 0.674, prefill 0.783, fused o-proj about 5e-6
  (its bound is carried through the projection and the kernel keeps o in fp32;
  the residual it adds to is unseeded, so the figure moves from run to run)
Wall time of this module: 12.5 s for 512 tests, the slowest 0.7 s.

The probes were also run once against kernels rebuilt with an in-bounds
one-key fault each (the last key counted twice from the second round of loads
on in the VALU kernel and from the fifth tile on in the MFMA kernel, key 700
dropped in prefill, key 300 dropped in the fused kernel): 181 of the 512
tests failed, in every family, and only those whose launch reaches the fault.
"""
import contextlib
import functools
import time
from types import SimpleNamespace as NS

import pytest
import torch

from . import attention_probes as ap

pytestmark = pytest.mark.gpu

DEV = "cuda"
WORST = {}  # kernel family -> largest count-probe err / bound seen


@pytest.fixture(scope="module")
def C():
    from llm_sharding_demo_amd.ops.hip import _load

    return _load()


@pytest.fixture(scope="module")
def CNT():
    return torch.zeros(1 << 16, dtype=torch.int32, device=DEV)


@pytest.fixture(scope="module", autouse=True)
def _module_report():
    t0 = time.perf_counter()
    yield
    for f in (_count, _needle, _pf_count, _pf_needle, _stale, _eye):
        f.cache_clear()
    print(f"\ncount probe, largest err / bound: {WORST}; module wall time {time.perf_counter() - t0:.1f} s")


@contextlib.contextmanager
def knobs(C, max_wg=None, small=None, large=None, mfma_min=None):
    """Set the attention launch knobs (None: the engine's default) and restore
    the defaults afterwards."""
    from llm_sharding_demo_amd.ops.hip import HipBackend

    R = HipBackend.R

    def apply(wg, sw64, sw128, lw, mf):
        C.attn_set_max_wg(wg)
        C.attn_set_small_waves(sw64)
        C.attn_set_small_waves128(sw128)
        C.attn_set_large_waves(64, lw)
        C.attn_set_large_waves(128, lw)
        C.attn_set_mfma_min(mf)

    try:
        apply(R.attn_max_wg if max_wg is None else max_wg,
              R.attn_small_waves if small is None else small,
              R.attn_small_waves128 if small is None else small,
              R.attn_large_waves if large is None else large,
              256 if mfma_min is None else mfma_min)
        yield
    finally:
        apply(R.attn_max_wg, R.attn_small_waves, R.attn_small_waves128, R.attn_large_waves, 256)


# full batch: one block per (row, kv head), 4 / 8 / 4 (2 keys in flight) / 2
# waves; small batch (grid capped at 3 blocks, so gx * splits <= 128): 8 / 16 /
# 4 waves, 88 = 8 waves with 8 keys per wave in flight
BLOCKS = [("full", 4), ("full", 8), ("full", 42), ("full", 2), ("small", 8), ("small", 16), ("small", 4), ("small", 88)]
BLOCK_IDS = [f"{k}{w}" for k, w in BLOCKS]


def valu(C, block):
    kind, waves = block
    if kind == "full":
        return knobs(C, max_wg=0, large=waves, mfma_min=0)
    return knobs(C, max_wg=3, small=waves, mfma_min=0)


def _dev(q, kc, vc, slots, ctx, **kw):
    return NS(q=q.reshape(q.shape[0], -1).to(DEV), kc=kc.to(DEV), vc=vc.to(DEV), slots=slots.int().to(DEV),
              pos=(ctx - 1).int().to(DEV), ctx=ctx, nh=q.shape[1], hd=q.shape[2], **kw)


@functools.lru_cache(maxsize=None)
def _count(hd, nh, n_kv):
    q, kc, vc, slots, ctx, exp = ap.count_sweep(hd, nh, n_kv)
    return _dev(q, kc, vc, slots, ctx, exp=exp.to(DEV))


@functools.lru_cache(maxsize=None)
def _needle(hd, nh, n_kv):
    q, kc, vc, slots, ctx, needles, exp = ap.needle_sweep(hd, nh, n_kv)
    # every (slot, kv head, position) is some row's needle: one bound for all users of this cache
    return _dev(q, kc, vc, slots, ctx, exp=exp.to(DEV), rest=ap.needle_rest(kc, vc, slots, needles), n_kv=n_kv)


def check_count(family, out, d, rel=ap.COUNT_REL_BF16, rows=None):
    exp = d.exp if rows is None else d.exp[rows]
    ctx = d.ctx if rows is None else d.ctx[rows]
    o = out.reshape(exp.shape)
    r = ap.count_ratio(o, exp, rel)
    WORST[family] = max(WORST.get(family, 0.0), r)
    if r > 1.0:
        bad = ((o.double() - exp).abs() > rel * exp).flatten(1).any(1).cpu()
        pytest.fail(f"count probe: err / bound = {r:.3g}; contexts of the first wrong rows: {ctx[bad][:12].tolist()}")


def check_needle(out, d, rows=None):
    exp = d.exp if rows is None else d.exp[rows]
    ctx = d.ctx if rows is None else d.ctx[rows]
    o = out.reshape(exp.shape)
    if not torch.equal(o.float(), exp.float()):  # V[j*] is never 0: no -0 / +0 ambiguity
        bad = (o.float() != exp.float()).flatten(1).any(1).cpu()
        pytest.fail(f"needle probe: {int(bad.sum())} of {bad.numel()} rows differ from V[j*]; "
                    f"contexts of the first: {ctx[bad][:12].tolist()}")


def decode(C, d, splits, rows=None):
    """One launch; with splits, twice: the combine's order is fixed, so the
    bits must repeat."""
    q, sl, pos = (d.q, d.slots, d.pos) if rows is None else (d.q[rows], d.slots[rows], d.pos[rows])
    o = C.attn_decode(q, d.kc, d.vc, sl, pos, d.nh, splits)
    if splits > 1:
        assert torch.equal(C.attn_decode(q, d.kc, d.vc, sl, pos, d.nh, splits), o)
    return o


# ---------------------------------------------------------------------------
# VALU decode
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("hd,nh,n_kv", ap.VALU_SHAPES)
@pytest.mark.parametrize("block", BLOCKS, ids=BLOCK_IDS)
@pytest.mark.parametrize("splits", [1, 3, 16])
def test_valu_decode_count_sweep(C, hd, nh, n_kv, block, splits):
    """Every context 1..1100 in one launch; 16 splits of contexts 1..15 are
    the empty and one-key splits."""
    d = _count(hd, nh, n_kv)
    with valu(C, block):
        o = decode(C, d, splits)
    check_count("valu", o, d)


@pytest.mark.parametrize("hd,nh,n_kv", ap.VALU_SHAPES)
@pytest.mark.parametrize("block", BLOCKS, ids=BLOCK_IDS)
@pytest.mark.parametrize("splits", [1, 3, 16])
def test_valu_decode_needle_sweep(C, hd, nh, n_kv, block, splits):
    """Every (context, needle) of the edge contexts in one launch."""
    d = _needle(hd, nh, n_kv)
    assert d.rest < ap.NEEDLE_REST_BF16
    with valu(C, block):
        o = decode(C, d, splits)
    check_needle(o, d)


# ---------------------------------------------------------------------------
# MFMA decode
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("hd,nh,n_kv", ap.MFMA_SHAPES)
@pytest.mark.parametrize("splits", [1, 2, 5, 16])
def test_mfma_decode_sweeps(C, hd, nh, n_kv, splits):
    dc, dn = _count(hd, nh, n_kv), _needle(hd, nh, n_kv)
    assert dn.rest < ap.NEEDLE_REST_BF16
    with knobs(C, max_wg=0, mfma_min=1):
        oc = decode(C, dc, splits)
        on = decode(C, dn, splits)
    check_count("mfma", oc, dc)
    check_needle(on, dn)


@pytest.mark.parametrize("nh,n_kv", [(8, 2), (16, 2)])
@pytest.mark.parametrize("splits", [1, 5])
def test_mfma_decode_partial_last_block(C, nh, n_kv, splits):
    """A block serves four (row, kv head) items: item counts of 2198, 10 and 2
    (count) / 9818 and 14 (needle) leave a partial last block."""
    dc, dn = _count(128, nh, n_kv), _needle(128, nh, n_kv)
    with knobs(C, max_wg=0, mfma_min=1):
        for B in (1099, 5, 1):
            assert (B * n_kv) % 4
            rows = torch.arange(dc.q.shape[0] - B, dc.q.shape[0], device=DEV)  # the longest contexts
            check_count("mfma", decode(C, dc, splits, rows), dc, rows=rows.cpu())
        for B in (4909, 7):
            assert (B * n_kv) % 4
            rows = torch.arange(dn.q.shape[0] - B, dn.q.shape[0], device=DEV)
            check_needle(decode(C, dn, splits, rows), dn, rows=rows.cpu())


# ---------------------------------------------------------------------------
# prefill
# ---------------------------------------------------------------------------
def _prefill_meta():
    from llm_sharding_demo_amd.ops.hip import prefill_tiles
    from llm_sharding_demo_amd.runtime.batch import BatchMeta

    meta = BatchMeta.build([s for s, _, _ in ap.PREFILL_SEQS], [st for _, st, _ in ap.PREFILL_SEQS],
                           [n for _, _, n in ap.PREFILL_SEQS], DEV)
    return meta, prefill_tiles(meta).to(DEV)


@functools.lru_cache(maxsize=None)
def _pf_count(hd, nh, n_kv):
    q, kc, vc, slots, ctx, exp = ap.prefill_count(hd, nh, n_kv)
    return _dev(q, kc, vc, slots, ctx, exp=exp.to(DEV))


@functools.lru_cache(maxsize=None)
def _pf_needle(hd, nh, n_kv):
    q, kc, vc, slots, ctx, needles, exp = ap.prefill_needle(hd, nh, n_kv)
    return _dev(q, kc, vc, slots, ctx, exp=exp.to(DEV), rest=ap.needle_rest(kc, vc, slots, needles))


def prefill(C, d, meta, tiles, q=None):
    return C.attn_prefill(d.q if q is None else q, d.kc, d.vc, tiles, meta.seq_slots, meta.q_start, meta.cu_q, d.nh)


@pytest.mark.parametrize("hd,nh,n_kv", ap.PREFILL_SHAPES)
def test_prefill_probes(C, hd, nh, n_kv):
    """One packed batch: 130 fresh tokens (tiles of 64, 64 and 2 queries), one
    token, exactly one tile, 200 tokens after 37 cached, 70 after 1000 cached.
    Query pos expects c(pos + 1) / (pos + 1); head 0's needle is the query's
    own position, the causal mask's last admitted key."""
    meta, tiles = _prefill_meta()
    dc, dn = _pf_count(hd, nh, n_kv), _pf_needle(hd, nh, n_kv)
    assert dn.rest < ap.NEEDLE_REST_BF16
    check_count("prefill", prefill(C, dc, meta, tiles), dc)
    check_needle(prefill(C, dn, meta, tiles), dn)


# ---------------------------------------------------------------------------
# fused attention + out-projection
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _eye(n):
    return torch.eye(n, dtype=torch.bfloat16, device=DEV)


def oproj(C, CNT, d, rows, nc):
    """x of the fused kernel with W = I, no bias and x = 0 on entry: the
    attention output itself, in fp32 (the kernel keeps o in fp32 in LDS)."""
    N = d.nh * d.hd
    x = torch.zeros(len(rows), N, device=DEV)
    C.attn_oproj(d.q[rows], d.kc, d.vc, d.slots[rows], d.pos[rows], d.nh, _eye(N), None, x, nc, CNT)
    return x


def _nc_choices(N, n_kv):
    chunks = max(1, -(-256 // n_kv))
    return [16, 160, -(-(-(-N // chunks)) // 16) * 16]  # 16, 160, the engine's choice


@pytest.mark.parametrize("hd,nh,n_kv", ap.OPROJ_SHAPES)
@pytest.mark.parametrize("B", [1, 2, 3, 4])
@pytest.mark.parametrize("nci", [0, 1, 2])
def test_oproj_probes(C, CNT, hd, nh, n_kv, B, nci):
    """The edge contexts, four per launch (B = 4 covers all 16).  Count probe
    to 2^-20 relative; needles at the last, first and middle key, x == V[j*]."""
    nc = _nc_choices(nh * hd, n_kv)[nci]
    dc, dn = _count(hd, nh, n_kv), _needle(hd, nh, n_kv)
    assert dn.rest < ap.NEEDLE_REST_FP32
    for g in range(4):
        ctxs = ap.EDGE_CTX[g::4][:B]
        rows = torch.tensor([c - 1 for c in ctxs])  # the count sweep's row of context c
        check_count("fused", oproj(C, CNT, dc, rows.to(DEV), nc), dc, ap.COUNT_REL_FP32, rows=rows)
        first = {c: int((dn.ctx == c).nonzero()[0]) for c in ctxs}  # needle sweep: rows of context c are contiguous
        for pick in (lambda c: c - 1, lambda c: 0, lambda c: c // 2):
            rows = torch.tensor([first[c] + pick(c) for c in ctxs])
            check_needle(oproj(C, CNT, dn, rows.to(DEV), nc), dn, rows=rows)
    assert int(CNT.abs().sum()) == 0  # every ticket counter re-armed


# ---------------------------------------------------------------------------
# stale keys behind the context
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stale(hd, n_kv, G):
    q, kc, vc, slots, ctx, needles, exp, clean = ap.stale_tail_case(n_kv, G, hd, ap.STALE_CTX)
    rest = ap.needle_rest(clean, vc, slots, needles, n_keys=int(ctx.max()))
    return _dev(q, kc, vc, slots, ctx, exp=exp.to(DEV), rest=rest, needles=needles, n_kv=n_kv)


@pytest.mark.parametrize("hd,n_kv,G", [(64, 4, 1), (64, 2, 4), (128, 4, 1), (128, 2, 2), (128, 2, 8)])
@pytest.mark.parametrize("block", [None, ("small", 16), ("small", 4), ("small", 88)], ids=["routed", "small16", "small4", "small88"])
@pytest.mark.parametrize("splits", [1, 3, 16])
def test_stale_tail_valu_decode(C, hd, n_kv, G, block, splits):
    """Cache positions >= ctx hold a key that outscores the needle 1.5x, with
    V = -V[j*]: one read past the end flips the sign of the output."""
    d = _stale(hd, n_kv, G)
    assert d.rest < ap.NEEDLE_REST_BF16
    with (knobs(C, mfma_min=0) if block is None else valu(C, block)):
        o = decode(C, d, splits)
    check_needle(o, d)


@pytest.mark.parametrize("n_kv,G", [(2, 2), (4, 4), (2, 8)])
@pytest.mark.parametrize("splits", [1, 2, 5, 16])
def test_stale_tail_mfma_decode(C, n_kv, G, splits):
    d = _stale(128, n_kv, G)
    assert d.rest < ap.NEEDLE_REST_BF16
    with knobs(C, max_wg=0, mfma_min=1):
        o = decode(C, d, splits)
    check_needle(o, d)


@pytest.mark.parametrize("hd,n_kv,G", [(64, 4, 1), (128, 4, 1), (128, 2, 2), (128, 2, 4), (128, 2, 8)])
def test_stale_tail_oproj(C, CNT, hd, n_kv, G):
    d = _stale(hd, n_kv, G)
    assert d.rest < ap.NEEDLE_REST_FP32
    for rows in (torch.arange(0, 4), torch.arange(4, 8), torch.tensor([7, 0, 5])):
        check_needle(oproj(C, CNT, d, rows.to(DEV), 160), d, rows=rows)
    assert int(CNT.abs().sum()) == 0


@pytest.mark.parametrize("hd,n_kv,G", [(64, 4, 1), (64, 2, 4), (128, 4, 1), (128, 2, 4)])
def test_stale_tail_prefill(C, hd, n_kv, G):
    """The poison behind the last query: sequence r is the tokens from its
    largest needle to ctx - 1 (every needle <= every query), all asking for
    the row's needles."""
    from llm_sharding_demo_amd.ops.hip import prefill_tiles
    from llm_sharding_demo_amd.runtime.batch import BatchMeta

    d = _stale(hd, n_kv, G)
    assert d.rest < ap.NEEDLE_REST_BF16
    start = d.needles.max(1).values
    qlen = d.ctx - start
    meta = BatchMeta.build(list(range(len(qlen))), start.tolist(), qlen.tolist(), DEV)
    rep = torch.repeat_interleave(torch.arange(len(qlen)), qlen).to(DEV)
    o = C.attn_prefill(d.q[rep].contiguous(), d.kc, d.vc, prefill_tiles(meta).to(DEV), meta.seq_slots,
                       meta.q_start, meta.cu_q, d.nh)
    assert torch.equal(o.reshape(-1, d.nh, hd), d.exp[rep])


# ---------------------------------------------------------------------------
# strided q
# ---------------------------------------------------------------------------
def _qkv_view(q, nh, n_kv, hd):
    """q as the trailing columns of a [rows, (2 n_kv + nh) hd] tensor (a fused
    QKV output's shape): a row stride and a base offset."""
    big = torch.randn(q.shape[0], (2 * n_kv + nh) * hd, device=DEV).bfloat16()
    big[:, 2 * n_kv * hd:] = q
    v = big[:, 2 * n_kv * hd:]
    assert not v.is_contiguous() and torch.equal(v, q)
    return v


@pytest.mark.parametrize("hd,nh,n_kv,block,mfma", [(64, 8, 2, ("full", 4), 0), (64, 4, 4, ("small", 8), 0),
                                                   (128, 8, 4, ("small", 88), 0), (128, 16, 2, ("full", 4), 0),
                                                   (128, 8, 2, ("full", 4), 1)])
@pytest.mark.parametrize("splits", [1, 3])
def test_strided_q_decode(C, hd, nh, n_kv, block, mfma, splits):
    d = _needle(hd, nh, n_kv)
    qv = _qkv_view(d.q, nh, n_kv, hd)
    with (knobs(C, max_wg=0, mfma_min=1) if mfma else valu(C, block)):
        o = C.attn_decode(d.q, d.kc, d.vc, d.slots, d.pos, nh, splits)
        ov = C.attn_decode(qv, d.kc, d.vc, d.slots, d.pos, nh, splits)
    assert torch.equal(o, ov)
    check_needle(ov, d)


@pytest.mark.parametrize("hd,nh,n_kv", [(64, 8, 2), (128, 4, 4)])
def test_strided_q_prefill(C, hd, nh, n_kv):
    meta, tiles = _prefill_meta()
    d = _pf_needle(hd, nh, n_kv)
    ov = prefill(C, d, meta, tiles, _qkv_view(d.q, nh, n_kv, hd))
    assert torch.equal(prefill(C, d, meta, tiles), ov)
    check_needle(ov, d)


# ---------------------------------------------------------------------------
# the launches the engine's routing picks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,nh,n_kv,hd,bucket", ap.ROUTED)
def test_routed_splits(C, B, nh, n_kv, hd, bucket):
    """Splits come from the captured context bucket, so rows much shorter than
    the bucket run empty and one-key splits: row contexts 1, bucket / 2 and
    bucket under the engine's own knobs and split count."""
    from llm_sharding_demo_amd.ops.hip import HipBackend

    splits = HipBackend.decode_attn_splits(B, nh, n_kv, hd, bucket)
    assert splits == {256: 1, 1: 2, 8: 16}[B]
    kc, vc = (t.to(DEV) for t in ap.count_cache(2, n_kv, bucket, hd))
    kn, vn = (t.to(DEV) for t in ap.needle_cache(2, n_kv, bucket, hd))
    for slots, ctx, needles in ap.routed_rows(B, nh, bucket):
        sl, pos = slots.int().to(DEV), (ctx - 1).int().to(DEV)
        assert ap.needle_rest(kn, vn, slots, needles) < ap.NEEDLE_REST_BF16
        qn = ap.needle_q(kn, slots, needles).reshape(B, nh * hd)
        dc = NS(exp=ap.count_expected(slots, ctx, nh, n_kv, hd).to(DEV), ctx=ctx)
        dn = NS(exp=ap.needle_expected(vn, slots, needles), ctx=ctx)
        with knobs(C):
            oc = C.attn_decode(torch.zeros_like(qn), kc, vc, sl, pos, nh, splits)
            on = C.attn_decode(qn, kn, vn, sl, pos, nh, splits)
        check_count("mfma" if B == 8 else "valu", oc, dc)
        check_needle(on, dn)
