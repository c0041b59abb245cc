"""CPU self-test of tests/gemm_probes.py: every checker accepts the fault-free
fp32 emulation and rejects the faults meant for it; the faults the random-data
tolerances of tests/test_kernels_gpu.py let through are pinned as such."""
import math

import pytest
import torch

from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.ops.hip import interleave_gate_up, rope_pair_permutation, rope_table

from . import gemm_probes as gp

M, N, K = 40, 192, 576  # 2.5 row tiles of 16, 3 column tiles of 64, 18 k-steps of 32 (9 of 64)


def bf(t):
    return t.to(torch.bfloat16)


@pytest.fixture(scope="module")
def case():
    a, w, bias, x = gp.integer_operands(M, N, K, seed=1)
    y = gp.exact_product(a, w)
    gp.assert_bf16_exact(y, bias)
    assert gp.max_partial_range(a, w) <= gp.BF16_INT
    return a, w, bias, x, y


def test_density_stays_in_the_bf16_range():
    """The docstring's figures: K = 1600 at 300 x 384 stays below 256 - 8 for
    three seeds; thinned K = 4096 and 14336 likewise."""
    worst = 0
    for seed in range(3):
        a, w, bias, _ = gp.integer_operands(300, 384, 1600, seed)
        y = gp.exact_product(a, w)
        worst = max(worst, gp.assert_bf16_exact(y, bias))
        assert gp.max_partial_range(a, w) <= gp.BF16_INT
    assert 150 <= worst <= 240, worst
    for Kbig in (4096, 14336):
        a, w, bias, _ = gp.integer_operands(8, 1008, Kbig, 3)
        assert abs(float(a.abs().double().mean()) * Kbig - gp.VAR_TARGET / 2) < 40  # K x density x 1/2 non-zero
        gp.assert_bf16_exact(gp.exact_product(a, w), bias)


@pytest.mark.parametrize("name", ["gelu", "silu"])
def test_activation_bound_covers_the_fp32_formula(name):
    """The measurement behind the bound: common.h's formula in fp32 (exact
    exp2 / reciprocal) meets it at every integer and half-integer in
    [-300, 300]; one more bf16 ulp of error does not."""
    x = torch.arange(-600, 601).double() / 2
    out = gp.act_emulate(name, x)
    r = gp.act_ratio(out, name, x)
    print(f"{name}: emulation / bound = {r:.3f}")
    assert r <= 1.0
    assert 0.3 < r  # the bound is the bf16 store's size, not a loose multiple of it
    f = gp.act_ref(name, x)
    big = f.abs() > 1e-3
    wrong = out.double().clone()
    wrong[big] = (f[big] * (1 + 1.5 * 2.0 ** -7)).to(torch.bfloat16).double()  # 1.5 bf16 ulps off
    assert gp.act_ratio(wrong, name, x) > 1.0
    assert not math.isfinite(gp.act_ratio(torch.full_like(out, float("nan")), name, x))
    # negative saturation: exp2 overflows, the result is -0, the truth is below the floor
    assert float(gp.act_emulate(name, torch.tensor([-300.0]))) == 0.0
    assert float(gp.act_emulate("silu", torch.tensor([32.0]))) == 32.0  # the SiLU up probe's pin


def _run(case, epi, splits=1, fault=None, step=32, slab_dtype=None):
    a, w, bias, x, y = case
    xb, xv = gp.guarded(x.float())
    out = gp.emulate(gp.poisoned(bf(a)), gp.poisoned(bf(w)), None if epi in ("f32", "slab") else bf(bias),
                     epi=epi, splits=splits, step=step, x=xv, slab_dtype=slab_dtype, fault=fault)
    return out, xb, xv


def _ok(case, epi, out, xb, xv):
    a, w, bias, x, y = case
    yb = (y + bias[None, :]).double()
    if epi == "bf16":
        return gp.same_values(out["out"], yb)
    if epi == "gelu":
        return gp.act_ratio(out["out"], "gelu", yb) <= 1.0
    if epi == "f32":
        return gp.same_values(out["out"], y.double()) and gp.same_values(out["segmax"], gp.segmax_expected(y).double())
    if epi == "slab":
        return gp.same_values(out["slab"].sum(0), y.double())
    assert epi == "resid"
    eb, ev = gp.guarded((x + y + bias[None, :]).float())
    return gp.bits_equal(xb, eb)


GEMM_FAULTS = [("drop_k", (17, 333)), ("drop_chunk", (36, 100, 64)), ("repeat_kstep", 448), ("omit_split", 1),
               ("repeat_split", 2), ("swap_cols", (3, 150)), ("read_past_k", 5)]


@pytest.mark.parametrize("epi", ["bf16", "gelu", "f32", "resid", "slab"])
def test_integer_probe_accepts_and_rejects(case, epi):
    for splits, step in ((1, 32), (3, 32), (7, 32), (2, 64)):
        for sd in ((torch.float32, torch.bfloat16) if epi == "slab" else (None,)):
            assert _ok(case, epi, *_run(case, epi, splits, None, step, sd)), (splits, step, sd)
    for fault in GEMM_FAULTS + (["bias_per_split"] if epi in ("bf16", "gelu", "resid") else []) \
            + (["write_past_m"] if epi == "resid" else []):
        out, xb, xv = _run(case, epi, 3, fault)
        assert not _ok(case, epi, out, xb, xv), fault


def test_bf16_partials_are_seen_only_when_partials_leave_the_bf16_range():
    """Partials rounded to bf16 are exact while they are integers <= 256 (that
    is what makes bf16 slabs bit-exact); the probe that sees the double
    rounding is the one whose partials exceed 256 while the total stays an
    fp32 integer: the fp32 epilogues with gemm_probes.wide_weights."""
    a, w, bias, x = gp.integer_operands(M, N, 1600, seed=2)
    y = gp.exact_product(a, w)
    assert gp.same_values(gp.emulate(bf(a), bf(w), epi="f32", splits=3, fault="partials_bf16")["out"], y.double())
    w16 = gp.wide_weights(w)  # |w'| <= 34: still bf16 integers; partials of a few thousand are not
    y16 = gp.exact_product(a, w16)
    assert int(y16.abs().max()) > 4 * gp.BF16_INT
    assert gp.same_values(gp.emulate(bf(a), bf(w16), epi="f32", splits=3)["out"], y16.double())
    assert not gp.same_values(gp.emulate(bf(a), bf(w16), epi="f32", splits=3, fault="partials_bf16")["out"],
                              y16.double())


def test_placement_probe(case):
    for which in ("n", "k"):
        a, w, km, y = gp.placement_operands(M, N, K, which)
        out = gp.emulate(bf(a), bf(w), epi="bf16", splits=3)["out"]
        assert gp.placement_mismatch(out, y, which, km, N, K) is None
    a, w, km, y = gp.placement_operands(M, N, K, "n")
    msg = gp.placement_mismatch(gp.emulate(bf(a), bf(w), epi="bf16", fault=("swap_cols", (3, 150)))["out"],
                                y, "n", km, N, K)
    assert msg is not None and "y[0, 3]" in msg and "[150]" in msg  # names the source column
    a, w, km, y = gp.placement_operands(M, N, K, "k")
    shifted = gp.emulate(bf(a.roll(1, 1)), bf(w), epi="bf16")["out"]  # every row reads k_m + 1
    msg = gp.placement_mismatch(shifted, y, "k", km, N, K)
    assert msg is not None and f"value of k [{int(km[0]) + 1}," in msg  # names the k it read
    # the column code cannot see a row-limited fault; the k code can
    a, w, km, y = gp.placement_operands(M, N, K, "n")
    assert gp.placement_mismatch(gp.emulate(bf(a.roll(1, 1)), bf(w), epi="bf16")["out"], y, "n", km, N, K) is None


def test_placement_blind_spot_codes_repeat_every_251():
    """Columns 251 apart carry one code: their swap passes the placement probe
    and fails the integer probe."""
    Nw = 272
    a, w, km, y = gp.placement_operands(M, Nw, K, "n")
    out = gp.emulate(bf(a), bf(w), epi="bf16", fault=("swap_cols", (5, 256)))["out"]
    assert gp.placement_mismatch(out, y, "n", km, Nw, K) is None
    a, w, bias, x = gp.integer_operands(M, Nw, K, seed=4)
    out = gp.emulate(bf(a), bf(w), bf(bias), epi="bf16", fault=("swap_cols", (5, 256)))["out"]
    assert not gp.same_values(out, (gp.exact_product(a, w) + bias[None, :]).double())


def _qkv(case, rope, fault=None):
    a, w, bias, x, y = case
    qs, kvs, hd, nh, nkv = gp.qkv_dims(N)
    tslot, tpos, S = gp.token_map(M)
    table = gp.rope_table_exact(S, hd) if rope else None
    perm = gp.qkv_weight_order(N) if rope else torch.arange(N)
    kb, kc = gp.guarded(torch.full((3, nkv, S, hd), gp.SENTINEL, dtype=torch.bfloat16), 1)
    vb, vc = gp.guarded(torch.full((3, nkv, S, hd), gp.SENTINEL, dtype=torch.bfloat16), 1)
    out = gp.emulate(bf(a), bf(w[perm]), bf(bias[perm]), epi="qkv", splits=3, fault=fault,
                     qkv=dict(tslot=tslot, tpos=tpos, kc=kc, vc=vc, table=table))
    q, ek, ev = gp.qkv_expected(y + bias[None, :], N, tslot, tpos, 3, S, table)
    return gp.same_values(out["q"], q), gp.bits_equal(kb, ek), gp.bits_equal(vb, ev)


def test_qkv_probe(case):
    hd = gp.qkv_dims(N)[2]
    r = gp.rope_rotation(torch.arange(64)[:, None], torch.arange(hd // 2)[None, :])
    assert bool(((r[1:] - r[:-1]) % 4 != 0).all()) and bool(((r[:, 1:] - r[:, :-1]) % 4 != 0).all())
    for rope in (False, True):
        assert _qkv(case, rope) == (True, True, True)
        for fault in ("kv_pos", "kv_slot"):
            okq, okk, okv = _qkv(case, rope, fault)
            assert okq and not okk and not okv, fault
        okq, okk, okv = _qkv(case, rope, ("swap_cols", (1, 2)))  # two q columns of one head
        assert not okq and okk and okv
    for fault in ("rope_pos", "rope_pair", "rope_sign"):
        okq, okk, okv = _qkv(case, True, fault)
        assert not okq and not okk and okv, fault  # V is not rotated


def test_silu_probes(case):
    a, w, bias, x, y = case
    F = N // 2
    au, wu, gate, up = gp.silu_operands(a, w, "up")
    assert bool((gate == 32).all())
    gp.assert_bf16_exact(up)
    wi = interleave_gate_up(bf(wu), F)
    assert gp.same_values(gp.emulate(bf(au), wi, epi="silu", splits=2)["out"], (32 * up).double())
    k_up = int(torch.nonzero(au[17] * wu[F + 5] != 0)[-1])
    for fault in ("interleave_shift", ("drop_k", (17, k_up)), ("swap_cols", (16, 48))):
        assert not gp.same_values(gp.emulate(bf(au), wi, epi="silu", fault=fault)["out"], (32 * up).double()), fault
    ag, wg, gate, up = gp.silu_operands(a, w, "gate")
    assert bool((up == 1).all())
    wi = interleave_gate_up(bf(wg), F)
    assert gp.act_ratio(gp.emulate(bf(ag), wi, epi="silu", splits=2)["out"], "silu", gate.double()) <= 1.0
    # a gate column off by one block; a gate short of one k
    assert gp.act_ratio(gp.emulate(bf(ag), wi.roll(32, 0), epi="silu")["out"], "silu", gate.double()) > 1.0
    k_hit = int(torch.nonzero(ag[17] * wg[5] != 0)[-1])
    assert gp.act_ratio(gp.emulate(bf(ag), wi, epi="silu", fault=("drop_k", (17, k_hit)))["out"],
                        "silu", gate.double()) > 1.0


@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("Kn", [768, 2056, 14336])
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_fused_norm_probe_is_exact(rms, Kn, eps):
    x, gamma, beta, w, bias, y = gp.norm_case(2, 64, Kn, rms, eps)
    assert bool((x.sum(1) == 0).all()) and bool((x.abs() == 1).all())
    gp.assert_bf16_exact(y, bias)
    xn = (ref.rmsnorm(x, bf(gamma), eps) if rms else ref.layernorm(x, bf(gamma), bf(beta), eps)).to(torch.bfloat16)
    assert gp.same_values(gp.emulate(xn, bf(w), bf(bias), step=8)["out"], (y + bias[None, :]).double())
    # a tail chunk that is not masked: one extra element per row changes the integer
    assert not gp.same_values(gp.emulate(gp.poisoned(xn), gp.poisoned(bf(w)), bf(bias), step=8,
                                         fault=("read_past_k", 1))["out"],
                              (y + bias[None, :]).double())


def close_ok(a, b, atol, rtol=2e-2):
    try:
        torch.testing.assert_close(a.float(), b.float(), atol=atol, rtol=rtol)
        return True
    except AssertionError:
        return False


def rnd(*shape, scale=1.0, seed=0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(torch.bfloat16)


@pytest.mark.parametrize("Mr", [33, 100])
@pytest.mark.parametrize("splits", [3, 7])
def test_gap_bf16_partials_pass_the_random_data_tolerance(Mr, splits):
    """test_linear's data and shape (N, K = 384, 640): split-K partials rounded
    to bf16 before the combine pass close(3e-2), with and without GELU.  The
    wide integer probe sees them
    (test_bf16_partials_are_seen_only_when_partials_leave_the_bf16_range)."""
    a, w, bias = rnd(Mr, 640, seed=5), rnd(384, 640, scale=0.05, seed=6), rnd(384, scale=0.1, seed=7)
    y_ref = ref.linear(a, w, bias)
    assert close_ok(gp.emulate(a, w, bias, splits=splits)["out"], y_ref, 3e-2)
    assert close_ok(gp.emulate(a, w, bias, splits=splits, fault="partials_bf16")["out"], y_ref, 3e-2)
    assert close_ok(gp.emulate(a, w, bias, epi="gelu", splits=splits, fault="partials_bf16")["out"],
                    ref.gelu_new(y_ref), 3e-2)


@pytest.mark.parametrize("n0", [4, 100])
def test_gap_rope_position_off_by_one(n0):
    """test_qkv_kv_append's data and shape (4 heads of 64, H = 256, theta
    10000): with every RoPE position one too far, half or more of the 32 pairs
    of each head still pass close(3e-2) (16 of 32 with 100-token sequences, more
    with 4) -- the slow pairs' cos / sin move by less than 0.015 -- so that test
    only sees the fault through the fast pairs.  The synthetic table fails
    every pair."""
    nh, n_kv, hd, H = 4, 2, 64, 256
    qs, kvs = nh * hd, n_kv * hd
    T, S = n0 + n0 + 2, 320
    a, w, bias = rnd(T, H, seed=13), rnd(qs + 2 * kvs, H, scale=0.05, seed=14), rnd(qs + 2 * kvs, scale=0.1, seed=15)
    tslot = torch.tensor([0] * n0 + [2] * (n0 + 2), dtype=torch.int32)
    tpos = torch.tensor(list(range(n0)) + list(range(5, 7 + n0)), dtype=torch.int32)
    y = ref.linear(a, w, bias)
    q_ref = ref.apply_rope(y[:, :qs].reshape(T, nh, hd), tpos, 10000.0)
    perm = torch.cat([rope_pair_permutation(nh, hd), rope_pair_permutation(n_kv, hd) + qs,
                      torch.arange(qs + kvs, qs + 2 * kvs)])
    inv = torch.argsort(rope_pair_permutation(1, hd))
    dims = (qs, kvs, hd, nh, n_kv)

    def run(table, fault):
        kc = torch.zeros(3, n_kv, S, hd, dtype=torch.bfloat16)
        out = gp.emulate(a, w[perm], bias[perm], epi="qkv", fault=fault,
                         qkv=dict(tslot=tslot, tpos=tpos, kc=kc, vc=kc.clone(), table=table, dims=dims))
        return out["q"].reshape(T, nh, hd)[:, :, inv]

    table = rope_table(S, hd, 10000.0, "cpu")
    assert close_ok(run(table, None), q_ref, 3e-2)
    q_bad = run(table, "rope_pos")
    pairs_passing = sum(close_ok(q_bad[..., [i, i + hd // 2]], q_ref[..., [i, i + hd // 2]], 3e-2)
                        for i in range(hd // 2))
    print(f"pairs of 32 that pass with pos + 1: {pairs_passing}")
    assert pairs_passing >= hd // 4
    exact = gp.rope_table_exact(S, hd)
    good, bad = run(exact, None), run(exact, "rope_pos")
    assert all(not torch.equal(good[..., [i, i + hd // 2]], bad[..., [i, i + hd // 2]]) for i in range(hd // 2))


def test_gap_row_limited_drop_can_pass_random_data():
    """One dropped k for one row moves one row's outputs by |a w| ~ 0.05:
    inside close(3e-2, rtol 2e-2) for most draws of test_linear's data, a wrong
    integer in the probe."""
    a, w, bias = rnd(100, 640, seed=5), rnd(384, 640, scale=0.05, seed=6), rnd(384, scale=0.1, seed=7)
    y_ref = ref.linear(a, w, bias)
    k_small = int(a[17].float().abs().argmin())
    assert close_ok(gp.emulate(a, w, bias, fault=("drop_k", (17, k_small)))["out"], y_ref, 3e-2)
