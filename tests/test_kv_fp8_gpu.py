"""FP8 (E4M3) KV cache on an MI355X: the four QKV store sites against the
reference's saturating append, the three attention kernels against the fp64
reference over the dequantised cache (dequantisation is exact, so the
project's attention bound applies unchanged), and the engine end to end."""
import dataclasses

import pytest
import torch

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams, get_model_config
from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.runtime.engine import Engine
from llm_sharding_demo_amd.utils.golden import compare_with_golden

from . import attention_probes as ap
from .test_kernels_gpu import CNT, C, bf, close, within_attention_bound  # noqa: F401  (C, CNT: fixtures)
from .test_numerics_gpu import BOUNDS, _prompts

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn
# route -> (rows of sequence 0, rows of sequence 1): the GEMV, the per-accumulator
# epilogue (decode rows), the row-contiguous epilogue (tiled, 256-row kernel), qkv_post
ROUTES = {"gemv": (1, 2), "decode": (4, 6), "tiled": (150, 150), "d256": (100, 100), "post": (4, 6)}


def _qkv(C, CNT, route, a, w, bias, kc, vc, tslot, tpos, qs, kvs, hd, table):
    if route == "gemv":
        return C.gemv(a, w, bias, 6, 0, None, None, 0.0, None, kc, vc, tslot, tpos, qs, kvs, hd, table)
    if route == "post":
        return C.qkv_post(a.float() @ w.float().T, bias, kc, vc, tslot, tpos, qs, kvs, hd, table)
    tiled = {"decode": False, "tiled": True, "d256": 2}[route]
    return C.linear_qkv(a, w, bias, kc, vc, tslot, tpos, qs, kvs, hd, table, tiled, 1, CNT)


def _write_case(route, hd):
    nh, n_kv, H, slots, S = 4, 2, 256, 3, 320
    n0, n1 = ROUTES[route]
    tslot = torch.tensor([0] * n0 + [2] * n1, dtype=torch.int32, device=DEV)
    tpos = torch.tensor(list(range(n0)) + list(range(5, 5 + n1)), dtype=torch.int32, device=DEV)
    caches = [torch.zeros(slots, n_kv, S, hd, dtype=FP8, device=DEV) for _ in range(2)]
    return nh, n_kv, H, n0 + n1, tslot, tpos, caches


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("route", list(ROUTES))
def test_qkv_store_exact_bytes(C, CNT, route, hd):
    """Integer inputs whose K/V are integers of magnitude <= 16 (representable),
    and rows scaled by 128 whose K/V overflow and must saturate to +-448: the
    cache bytes equal ref.kv_append's on an FP8 cache."""
    nh, n_kv, H, T, tslot, tpos, (kc, vc) = _write_case(route, hd)
    qs, kvs = nh * hd, n_kv * hd
    g = torch.Generator().manual_seed(hd)
    w = torch.randint(-7, 8, (qs + 2 * kvs, H), generator=g).double()
    bias = torch.randint(-2, 3, (qs + 2 * kvs,), generator=g).double()
    a = torch.zeros(T, H, dtype=torch.float64)  # one non-zero per row: y = s w[:, k] + bias
    a[torch.arange(T), torch.arange(T) % H] = torch.where(torch.arange(T) % 3 == 1, 128.0, 2.0).double()
    y = a @ w.T + bias
    assert float(y[:, qs:].abs().max()) > 448 and float(y[a.sum(1) == 2.0, qs:].abs().max()) <= 16
    dev = lambda t: t.to(torch.bfloat16).to(DEV)  # noqa: E731
    _qkv(C, CNT, route, dev(a), dev(w), dev(bias), kc, vc, tslot, tpos, qs, kvs, hd, None)
    kr, vr = torch.zeros_like(kc, device="cpu"), torch.zeros_like(vc, device="cpu")
    ref.kv_append(kr, vr, y[:, qs:qs + kvs].reshape(T, n_kv, hd).float(), y[:, qs + kvs:].reshape(T, n_kv, hd).float(),
                  tslot.cpu(), tpos.cpu())
    assert torch.equal(kc.view(torch.uint8).cpu(), kr.view(torch.uint8))
    assert torch.equal(vc.view(torch.uint8).cpu(), vr.view(torch.uint8))
    assert int((kr.float().abs() == 448).sum()) > 0


@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("route", list(ROUTES))
def test_qkv_store_bounded_error(C, CNT, route, hd, rope):
    """Random bf16 inputs: |dequant(cache) - fp64 reference| <= 2^-3 |ref| + 2^-9,
    one E4M3 ulp (3 mantissa bits, subnormal step 2^-9) -- the fp32 sum may lie
    across a rounding boundary from the fp64 one; unwritten positions stay zero."""
    from llm_sharding_demo_amd.ops.hip import rope_pair_permutation, rope_table

    nh, n_kv, H, T, tslot, tpos, (kc, vc) = _write_case(route, hd)
    qs, kvs = nh * hd, n_kv * hd
    a, w, bias = bf(T, H, seed=13), bf(qs + 2 * kvs, H, scale=0.05, seed=14), bf(qs + 2 * kvs, scale=0.1, seed=15)
    y = (a.double() @ w.double().T + bias.double()).cpu()
    k_ref, v_ref = y[:, qs:qs + kvs].reshape(T, n_kv, hd), y[:, qs + kvs:].reshape(T, n_kv, hd)
    table = None
    if rope:
        k_ref = ref.apply_rope(k_ref, tpos.cpu(), 10000.0).double()
        perm = torch.cat([rope_pair_permutation(nh, hd), rope_pair_permutation(n_kv, hd) + qs,
                          torch.arange(qs + kvs, qs + 2 * kvs)]).to(DEV)
        w, bias = w[perm].contiguous(), bias[perm].contiguous()
        table = rope_table(kc.shape[2], hd, 10000.0, DEV)
    _qkv(C, CNT, route, a, w, bias, kc, vc, tslot, tpos, qs, kvs, hd, table)
    kd, vd = kc.cpu().double(), vc.cpu().double()
    if rope:  # un-permute the pair-interleaved head dims
        kd = kd[..., torch.argsort(rope_pair_permutation(1, hd))]
    s, p = tslot.cpu().long(), tpos.cpu().long()
    for name, got, want in (("k", kd, k_ref), ("v", vd, v_ref)):
        err = (got[s, :, p, :] - want).abs()
        ratio = float((err / (2.0 ** -3 * want.abs() + 2.0 ** -9)).max())
        print(f"{route} hd{hd} rope{int(rope)} {name}: err / bound = {ratio:.3g}")
        assert ratio <= 1.0
        got[s, :, p, :] = 0
        assert not bool(got.any())


def _fp8_cache(*shape, seed):
    # no value quantises to zero: a one-key context whose V element is exactly 0
    # has a zero bound and a zero error, and bound_ratio's 0 / 0 is not a verdict
    x = bf(*shape, seed=seed).cpu().float()
    return torch.where(x.abs() < 2.0 ** -6, torch.full_like(x, 2.0 ** -6), x).clamp(-448, 448).to(FP8).to(DEV)


def _check(family, o, q, kc, vc, seq_slots, q_start, cu_q, nh):
    o64, bound = ap.reference_and_bound(q.reshape(-1, nh, kc.shape[3]), kc, vc, seq_slots, q_start, cu_q)
    close(o.reshape(o64.shape), o64, 2e-2)
    within_attention_bound(family, o, o64, bound)


@pytest.mark.parametrize("hd,nh,n_kv", [(64, 4, 4), (64, 8, 2), (128, 8, 8), (128, 8, 2), (128, 32, 8)])
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("B", [5, 70])
def test_attention_decode_fp8(C, hd, nh, n_kv, splits, B):
    """B = 5: 8-wave blocks, one-key, KPI-edge (8 / 16) and S - 1 contexts;
    B = 70: 4-wave blocks (and, for (128, 32, 8) with 3 splits, the MFMA kernel)."""
    slots, S = max(6, B), 300
    kc, vc = _fp8_cache(slots, n_kv, S, hd, seed=16), _fp8_cache(slots, n_kv, S, hd, seed=17)
    q = bf(B, nh * hd, seed=18)
    if B == 5:
        seq_slots = torch.tensor([5, 0, 2, 3, 1], dtype=torch.int32, device=DEV)
        pos = torch.tensor([0, 17, 63, 140, 299], dtype=torch.int32, device=DEV)
    else:
        g = torch.Generator().manual_seed(B)
        seq_slots = torch.randperm(slots, generator=g)[:B].int().to(DEV)
        pos = torch.cat([torch.tensor([0, 7, 8, 15, 16, 299]), torch.randint(0, S, (B - 6,), generator=g)]).int().to(DEV)
    o = C.attn_decode(q, kc, vc, seq_slots, pos, nh, splits)
    _check("fp8", o, q, kc, vc, seq_slots, pos, torch.arange(B + 1, dtype=torch.int32), nh)
    if B == 5 and splits == 1:  # a capped grid: each block loops over (sequence, head) items
        C.attn_set_max_wg(3)
        try:
            assert torch.equal(C.attn_decode(q, kc, vc, seq_slots, pos, nh, splits), o)
        finally:
            C.attn_set_max_wg(0)


@pytest.mark.parametrize("nh,n_kv,B,splits", [(16, 8, 3, 1), (32, 8, 3, 1), (64, 8, 3, 1), (16, 8, 40, 1),
                                              (32, 8, 40, 1), (64, 8, 40, 1), (32, 8, 40, 3)])
def test_attention_decode_mfma_fp8(C, nh, n_kv, B, splits):
    """The two-deep prefetch over 1, 2 and 3 tiles: contexts at the 32- and 64-key edges."""
    hd, slots, S = 128, max(B, 8), 300
    kc, vc = _fp8_cache(slots, n_kv, S, hd, seed=26), _fp8_cache(slots, n_kv, S, hd, seed=27)
    q = bf(B, nh * hd, seed=28)
    g = torch.Generator().manual_seed(B + nh)
    seq_slots = torch.randperm(slots, generator=g)[:B].int().to(DEV)
    edge = [30, 31, 32, 62, 63, 64, 0, 95, 96, 299]  # positions: contexts 31 / 32 / 33, 63 / 64 / 65, ...
    pos = torch.tensor([edge[i] if i < len(edge) else int(torch.randint(0, S, (1,), generator=g))
                        for i in range(B)], dtype=torch.int32, device=DEV)
    C.attn_set_mfma_min(1)
    try:
        o = C.attn_decode(q, kc, vc, seq_slots, pos, nh, splits)
    finally:
        C.attn_set_mfma_min(256)
    _check("mfma-fp8", o, q, kc, vc, seq_slots, pos, torch.arange(B + 1, dtype=torch.int32), nh)


@pytest.mark.parametrize("hd,nh,n_kv", [(64, 4, 4), (128, 8, 2)])
def test_attention_prefill_fp8(C, hd, nh, n_kv):
    from llm_sharding_demo_amd.ops.hip import prefill_tiles
    from llm_sharding_demo_amd.runtime.batch import BatchMeta

    kc, vc = _fp8_cache(4, n_kv, 400, hd, seed=19), _fp8_cache(4, n_kv, 400, hd, seed=20)
    # seq 0: fresh 130 tokens; seq 1: 1 token; seq 2: chunk of 70 after 200 cached; seq 3: 64
    meta = BatchMeta.build([1, 0, 3, 2], [0, 0, 200, 5], [130, 1, 70, 64], DEV)
    q = bf(meta.num_tokens, nh * hd, seed=21)
    o = C.attn_prefill(q, kc, vc, prefill_tiles(meta).to(DEV), meta.seq_slots, meta.q_start, meta.cu_q, nh)
    _check("prefill-fp8", o, q, kc, vc, meta.seq_slots, meta.q_start, meta.cu_q, nh)


# ---- through the engine (greedy: exact equalities) ----
PROMPT = [(7 * i + 3) % 200 + 1 for i in range(40)]


def _engine(model="gpt2-test", **kw):
    cfg = EngineConfig(model_id=model, max_batch=8, device="cuda", max_seq_len=256, kv_dtype="fp8_e4m3", **kw)
    return Engine(cfg, devices=["cuda:0"])


@pytest.mark.parametrize("model", ["gpt2-test", "llama-test"])
def test_engine_graphs_equal_eager(model):
    sp = SamplingParams(greedy=True, max_new_tokens=8)
    prompts = [PROMPT, PROMPT[:3], PROMPT[5:30]]
    e = _engine(model, use_graphs=True)
    assert e.stages[0].kv.buf.dtype == FP8 and e.stages[0].backend.name == "hip"
    assert e.generate_ids(prompts, sp) == _engine(model, use_graphs=False).generate_ids(prompts, sp)


def test_engine_prefix_hit_equals_miss_and_forks_equal_lone_requests():
    on, off = _engine(prefix_cache=2), _engine()
    sp = SamplingParams(greedy=True, max_new_tokens=6)
    b = PROMPT[:32] + [5, 9, 11]
    on.generate_requests([PROMPT], [sp])
    hit = on.generate_requests([b], [sp])[0]
    assert hit.cached_tokens > 0 and hit.output == off.generate_requests([b], [sp])[0].output
    kw = dict(max_new_tokens=6, greedy=True)  # the forks read copies of the prompt's FP8 KV
    lone = [off.generate_ids([PROMPT], SamplingParams(seed=100 + i, **kw))[0] for i in range(2)]
    assert off.generate_samples([PROMPT], SamplingParams(n=2, seed=100, **kw)) == [lone]


@pytest.mark.parametrize("model,layers,lens", [("gpt2", None, [7, 33, 96]), ("llama-3-8b", 4, [9, 64])])
def test_numerics_within_the_formats_own_cost(model, layers, lens):
    """HIP/FP8 vs the fp32 golden stays within the cost of the format itself
    (golden ops over an FP8 cache vs the fp32 golden, same run) plus the
    compute-error budget the project already accepts for the model."""
    mc = get_model_config(model)
    if layers:
        mc = dataclasses.replace(mc, n_layers=layers)
    r = compare_with_golden(mc, _prompts(mc.vocab_size, lens), steps=8, kv_dtype=FP8)
    g, h = r["golden_kv"], r["hip_kv"]
    print(model, "golden-FP8 vs golden-fp32:", g, "HIP-FP8 vs golden-fp32:", h)
    top1, mx, mean = BOUNDS[model]
    assert h["max_rel_err"] <= g["max_rel_err"] + mx and h["mean_rel_err"] <= g["mean_rel_err"] + mean
    assert h["top1_agreement"] >= g["top1_agreement"] - (1 - top1)
