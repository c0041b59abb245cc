"""Exact-arithmetic probes for the embedding gather (csrc/kernels/norm.hip) and
the two stand-alone epilogue passes of csrc/kernels/elementwise.hip, silu_mul
and qkv_post, on an MI355X.  Both passes take their input tensor directly, so
they get integers with one right answer (tests/gemm_probes.py derives why each
is exact): no GEMM in front, a row stride larger than the row with POISON in
the other columns, a partly idle last workgroup, hd = 8, and caches pre-filled
with SENTINEL that must survive wherever nothing is written.
"""
import pytest
import torch

from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.ops.hip import rope_pair_permutation

from . import gemm_probes as gp

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture(scope="module")
def C():
    from llm_sharding_demo_amd.ops.hip import _load

    return _load()


# ---------------------------------------------------------------------------
# embed
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("H", [8, 2048, 2056])  # 2056: thread 0 takes a second trip
def test_embed_exact(C, H):
    """Integer tables: wte[id] + wpe[pos] is exact in fp32.  Ids below 0 and
    from `vocab` on gather rows 0 and vocab - 1."""
    V, P = 50, 40
    r, c = torch.arange(64)[:, None], torch.arange(H)[None, :]
    wte = gp.code(31 * r[:V] + c).to(BF).to(DEV)
    wpe = gp.code(17 * r[:P] + 3 * c + 7).to(BF).to(DEV)
    special = [-1, -2 ** 31, V, 2 ** 31 - 1, 0, V - 1]
    ids37 = (7 * torch.arange(37) + 3) % V
    ids37[[0, 5, 17, 30, 35, 36]] = torch.tensor(special)
    cases = [ids37] + [torch.tensor([i]) for i in special + [23]]
    for ids in cases:
        ids = ids.int().to(DEV)
        pos = ((5 * torch.arange(ids.numel()) + 11) % P).int().to(DEV)
        clamped = ids.clamp(0, V - 1)
        for pe in (wpe, None):
            out = C.embed(ids, pos, wte, pe)
            exp = ref.embed(clamped, pos, wte, pe)
            assert out.dtype == torch.float32 and torch.equal(out, exp), (ids.tolist()[:6], pe is None)
            assert float(out.abs().max()) <= 250


# ---------------------------------------------------------------------------
# silu_mul
# ---------------------------------------------------------------------------
def _gate_up_layout(gate, up):
    """[M, 2F] in the [gate 16 | up 16] block layout."""
    M, F = gate.shape
    return torch.stack([gate.reshape(M, F // 16, 16), up.reshape(M, F // 16, 16)], 2).reshape(M, 2 * F)


@pytest.mark.parametrize("M", [1, 33])
@pytest.mark.parametrize("F", [16, 48, 1024])  # M F / 8 = 2 .. 4224 threads: 16.5 workgroups at the largest
def test_silu_mul_exact(C, F, M):
    m, c = torch.arange(M)[:, None], torch.arange(F)[None, :]
    up = gp.code(31 * m + c).double()
    y = gp.poisoned(_gate_up_layout(torch.full((M, F), 32.0), up).to(BF).to(DEV))
    assert y.stride(0) == 2 * F + 16 and y.data_ptr() % 16 == 0
    out = C.silu_mul(y)
    assert out.shape == (M, F) and gp.same_values(out, 32 * up), "silu(32) * up"
    gate = (((7 * (m * F + c)) % 161) - 80).double() / 2  # integers and half-integers in [-40, 40]
    y = gp.poisoned(_gate_up_layout(gate, torch.ones(M, F, dtype=torch.float64)).to(BF).to(DEV))
    out = C.silu_mul(y)
    r = gp.act_ratio(out, "silu", gate)
    print(f"silu_mul F {F} M {M}: error / bound = {r:.3f}")
    assert r <= 1.0, f"silu: error / bound = {r}"


# ---------------------------------------------------------------------------
# qkv_post
# ---------------------------------------------------------------------------
def _qkv_perm(nh, nkv, hd):
    qs, kvs = nh * hd, nkv * hd
    return torch.cat([rope_pair_permutation(nh, hd), rope_pair_permutation(nkv, hd) + qs,
                      torch.arange(qs + kvs, qs + 2 * kvs)])


def _qkv_inputs(M, nh, nkv, hd, rope):
    """Integer y [M, N] in the model's column order, the token map (the last
    three of 33 rows parked on the scratch slot 3, position 0, with one and the
    same row of values: they race for one place) and the RoPE table."""
    N = (nh + 2 * nkv) * hd
    y = gp.code(37 * torch.arange(M)[:, None] + torch.arange(N)[None, :])
    tslot, tpos, S = gp.token_map(M)
    if M > 3:
        y[-3:] = y[-3]
        tslot[-3:], tpos[-3:] = 3, 0
    table = gp.rope_table_exact(S, hd) if rope else None
    return N, y, tslot, tpos, S, table


@pytest.mark.parametrize("M", [1, 33])
@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("nh,nkv,hd", [(1, 1, 8), (4, 2, 64), (8, 2, 128)])
def test_qkv_post_exact(C, nh, nkv, hd, bias, rope, M):
    N, y, tslot, tpos, S, table = _qkv_inputs(M, nh, nkv, hd, rope)
    dims = (nh * hd, nkv * hd, hd, nh, nkv)
    b = ((5 * torch.arange(N)) % 17 - 8) if bias else torch.zeros(N, dtype=torch.int64)
    q_exp, ek, ev = gp.qkv_expected(y + b[None, :], N, tslot, tpos, 4, S, table, dims=dims)
    perm = _qkv_perm(nh, nkv, hd) if rope else torch.arange(N)
    yk = gp.poisoned(y[:, perm].float().to(DEV))  # the kernel's column order, row stride N + 16
    assert yk.stride(0) == N + 16 and yk.data_ptr() % 16 == 0
    kb = torch.full((6, nkv, S, hd), gp.SENTINEL, dtype=BF, device=DEV)
    vb = kb.clone()
    q = C.qkv_post(yk, b[perm].to(BF).to(DEV) if bias else None, kb[1:-1], vb[1:-1], tslot.to(DEV), tpos.to(DEV),
                   dims[0], dims[1], hd, None if table is None else table.to(DEV))
    assert gp.same_values(q, q_exp), "q"
    assert gp.bits_equal(kb, ek), "K cache, the unwritten positions and the guard slots"
    assert gp.bits_equal(vb, ev), "V cache, the unwritten positions and the guard slots"
    assert int((kb == gp.SENTINEL).sum()) == kb.numel() - min(M, 31) * nkv * hd


@pytest.mark.parametrize("rope", [False, True])
def test_qkv_post_equals_fused_epilogue(C, rope):
    """The same integer product through linear_qkv's fused epilogue and
    through qkv_post: the same bits in q and both caches."""
    nh, nkv, hd, M, K = 4, 2, 64, 33, 256
    N = (nh + 2 * nkv) * hd
    a, w, bias, _ = gp.integer_operands(M, N, K, seed=11)
    y = gp.exact_product(a, w)
    gp.assert_bf16_exact(y, bias)
    tslot, tpos, S = gp.token_map(M)
    table = gp.rope_table_exact(S, hd) if rope else None
    perm = _qkv_perm(nh, nkv, hd) if rope else torch.arange(N)
    td = None if table is None else table.to(DEV)
    cnt = torch.zeros(1 << 16, dtype=torch.int32, device=DEV)
    caches = [torch.full((5, nkv, S, hd), gp.SENTINEL, dtype=BF, device=DEV) for _ in range(4)]
    bk = bias[perm].to(BF).to(DEV)
    q1 = C.qkv_post(y[:, perm].float().to(DEV), bk, caches[0][1:-1], caches[1][1:-1], tslot.to(DEV), tpos.to(DEV),
                    nh * hd, nkv * hd, hd, td)
    q2 = C.linear_qkv(a.to(BF).to(DEV), w[perm].to(BF).to(DEV).contiguous(), bk, caches[2][1:-1], caches[3][1:-1],
                      tslot.to(DEV), tpos.to(DEV), nh * hd, nkv * hd, hd, td, True, 1, cnt)
    assert gp.bits_equal(q1, q2) and gp.bits_equal(caches[0], caches[2]) and gp.bits_equal(caches[1], caches[3])
    q_exp, ek, ev = gp.qkv_expected(y + bias[None, :], N, tslot, tpos, 3, S, table, dims=(nh * hd, nkv * hd, hd, nh, nkv))
    assert gp.same_values(q1, q_exp) and gp.bits_equal(caches[0], ek) and gp.bits_equal(caches[1], ev)
    assert int(cnt.abs().sum()) == 0
