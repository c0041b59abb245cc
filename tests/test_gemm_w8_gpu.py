"""The FP8-weight decode GEMM (csrc/kernels/gemm_w8.hip): exact-arithmetic
cases bit for bit against float64, every fused epilogue against float64 over
the dequantised weights with the bf16 split-K kernel's tolerances, the
backend's route, refusals, and the model and the engine on it."""
import pytest
import torch

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams, get_model_config
from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.ops.hip import HipBackend, interleave_gate_up, rope_pair_permutation, rope_table
from llm_sharding_demo_amd.ops.routing import Routing
from llm_sharding_demo_amd.utils.golden import compare_with_golden

from .test_kernels_gpu import C, CNT, DEV, _fp32_slabs, bf, close  # noqa: F401  (fixtures)
from .test_numerics_gpu import BOUNDS, _prompts
from .test_weight_fp8_gpu import FP8, quant

pytestmark = pytest.mark.gpu


# K: one block; 3 blocks (3 splits of one); the first block of a second round for each round length the
# kernel instantiates (1024, 512, 256, 128 k: MT = 1, 2, 3-4, 6-8); >= 3 rounds for every MT
@pytest.mark.parametrize("K", [64, 192, 1088, 576, 320, 4160])
@pytest.mark.parametrize("M", [9, 16, 17, 40, 100, 129, 300])
def test_gemm_w8_exact(C, CNT, M, K):
    """Integer weights in [-7, 7] times 2^e per row (quantised without error),
    integer activations and bias: every partial sum is a multiple of 1/4 below
    2^24, so fp32 is exact in any order and the outputs equal float64's."""
    N = 1000  # the last 64-column tile is partial, its last 16-column sub-tile has 8 live columns
    C.gemm_set_sk_rows(128)  # row blocks of up to 128 rows: MT = 1, 1, 2, 3, 8, 6 + 3 (33-row tail), 8 + 8 + 3
    g = torch.Generator(device=DEV).manual_seed(K + M)
    wi = torch.randint(-7, 8, (N, K), device=DEV, generator=g).double()
    wi[:, K - 1] = 7
    w = wi * (2.0 ** torch.randint(-2, 3, (N, 1), device=DEV, generator=g).double())
    a = torch.randint(-3, 4, (M, K), device=DEV, generator=g).double()
    bias = torch.randint(-9, 10, (N,), device=DEV, generator=g).double()
    q, s = C.quantize_rows_fp8(w.bfloat16())
    assert torch.equal(q.float().double() * s.double()[:, None], w)
    y = a @ w.T + bias
    ab, bb = a.bfloat16(), bias.bfloat16()
    for splits in (1, 3) if K >= 192 else (1,):
        assert torch.equal(C.linear(ab, q, bb, 0, 0, splits, CNT, wscale=s), y.float().bfloat16())
        assert C.gemm_last_launch().startswith("w8<")
        assert torch.equal(C.linear_f32(ab, q, 0, splits, CNT, wscale=s).double(), y - bias)
        for defer in (False, True):
            x = torch.randint(-50, 50, (M, N), device=DEV, generator=g).float()
            want = x.double() + y
            slab = C.linear_residual(ab, q, bb, x, splits, 0, CNT, defer, wscale=s)
            assert (slab is not None) == (defer and splits > 1)
            if slab is not None:  # fp32 slabs: their sum is exact only if every partial was scaled
                assert slab.dtype == torch.float32 and torch.equal(slab.double().sum(0), y - bias)
                C.norm(x, slab, bb, None, None, 0.0, True, None, False)
            assert torch.equal(x.double(), want)
    C.gemm_set_sk_rows(64)
    assert int(CNT.abs().sum()) == 0  # every ticket counter re-armed


def exact_case(C, M, N, K, seed, e_lo, e_hi):
    """test_gemm_w8_exact's operands with row scales 2^e, e in [e_lo, e_hi]: (a, q, scale, bias, float64 a @ w^T,
    float64 bias).  The quantised bytes are the integers 64 wi, so every raw partial sum is an integer below
    3 * 448 * K (< 2^24 up to K = 3900) and the row scale 2^e / 64 multiplies it without error."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    wi = torch.randint(-7, 8, (N, K), device=DEV, generator=g).double()
    wi[:, K - 1] = 7
    w = wi * (2.0 ** torch.randint(e_lo, e_hi + 1, (N, 1), device=DEV, generator=g).double())
    a = torch.randint(-3, 4, (M, K), device=DEV, generator=g).double()
    bias = torch.randint(-9, 10, (N,), device=DEV, generator=g).double()
    q, s = C.quantize_rows_fp8(w.bfloat16())
    assert torch.equal(q.float().double() * s.double()[:, None], w)
    return a.bfloat16(), q, s, bias.bfloat16(), a @ w.T, bias


def stale_workspace_rounds(C, CNT, kind, big, small):
    """test_split_k_ignores_stale_workspace (test_gemm_exact_gpu.py) on the FP8-weight kernels: a larger problem of
    larger values first, then a smaller shape of smaller values on the same ticket counters.  The workspace comes
    from torch.empty (the allocator hands the freed block back), so a partial that is read before it is written, or
    a ticket left over, changes the second, exact result."""
    (M1, N1, K1, S1), (M2, N2, K2, S2) = big, small
    a1, q1, s1, _, y1, _ = exact_case(C, M1, N1, K1, 1, 2, 4)
    a2, q2, s2, b2, y2, bias2 = exact_case(C, M2, N2, K2, 2, -2, 2)
    for _ in range(2):
        out = C.linear_f32(a1, q1, kind, S1, CNT, wscale=s1)
        assert torch.equal(out.double(), y1)
        del out
        out = C.linear(a2, q2, b2, 0, kind, S2, CNT, wscale=s2)
        assert torch.equal(out, (y2 + bias2).float().bfloat16())
        out = C.linear_f32(a2, q2, kind, S2, CNT, wscale=s2)
        assert torch.equal(out.double(), y2)
        del out
    assert int(CNT.abs().sum()) == 0


def test_gemm_w8_split_k_ignores_stale_workspace(C, CNT):
    stale_workspace_rounds(C, CNT, 0, (64, 256, 1600, 7), (33, 192, 576, 3))
    assert C.gemm_last_launch().startswith("w8<")


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("K", [768, 1600])
@pytest.mark.parametrize("M", [16, 80])
@pytest.mark.parametrize("epi", ["gelu", "silu_mul", "f32_segmax", "slab_bf16"])
def test_gemm_w8_epilogues(C, CNT, epi, M, K, splits):
    N = 512 if epi == "silu_mul" else 1000
    a = bf(M, K, seed=1)
    w = bf(N, K, scale=0.05, seed=2)
    if epi == "silu_mul":
        w[:N // 2] *= 0.25  # gate and up rows get scales 16 times apart
        w[N // 2:] *= 4
    q, s, wd = quant(w)
    bias = bf(N, scale=0.1, seed=3)
    y = a.double() @ wd.T
    if epi == "gelu":  # test_linear: 3e-2
        close(C.linear(a, q, bias, 1, 0, splits, CNT, wscale=s), ref.gelu_new(y + bias.double()), 3e-2)
    elif epi == "silu_mul":  # test_linear: 3e-2
        qi = interleave_gate_up(q.view(torch.uint8), N // 2).contiguous().view(FP8)
        si = interleave_gate_up(s[:, None], N // 2).reshape(-1).contiguous()
        close(C.linear(a, qi, None, 2, 0, splits, CNT, wscale=si), ref.silu_mul(y[:, :N // 2], y[:, N // 2:]), 3e-2)
    elif epi == "f32_segmax":  # test_linear_residual_and_f32: 2e-3, 1e-3
        seg = torch.full((M, N // 8), float("nan"), device=DEV)
        out = C.linear_f32(a, q, 0, splits, CNT, seg, wscale=s)
        assert torch.equal(seg, out.view(M, N // 8, 8).amax(-1))
        close(out, y, 2e-3, 1e-3)
    else:  # test_linear_residual_bf16_slabs' bounds: S bf16 roundings of the partials
        C.gemm_set_slab_bf16(1)
        x = torch.randn(M, N, device=DEV)
        want = x.double() + y + bias.double()
        slab = C.linear_residual(a, q, bias, x, max(splits, 2), 0, CNT, True, wscale=s)
        assert slab.dtype == torch.bfloat16
        C.norm(x, slab, bias, None, None, 0.0, True, None, False)
        err = (x.double() - want).abs()
        assert float(err.max()) <= 2.0 ** -8 * float(y.abs().max()) * max(splits, 2)
        assert float(err.mean()) <= 2.0 ** -9 * float(y.abs().mean()) * 2
    assert int(CNT.abs().sum()) == 0


def _qkv_case(arch, M, kv):
    """(arguments of a QKV launch, float64 q / k / v) of test_gemv_fp8_qkv_kv_append's two shapes."""
    hd, nh, nkv, H = (64, 6, 6, 768) if arch == "gpt2" else (128, 8, 2, 1024)
    qs, kvs, slots, max_seq, rms = nh * hd, nkv * hd, 136, 96, arch == "llama"
    N = qs + 2 * kvs
    w, bias = bf(N, H, scale=0.05, seed=12), (None if rms else bf(N, scale=0.1, seed=13))
    xn = bf(M, H, seed=14)
    tslot = torch.randperm(slots, device=DEV)[:M].int()
    tpos = torch.randint(0, max_seq, (M,), device=DEV).int()
    rope = None
    if rms:  # quantise the permuted rows, as prepare_stage does; the reference un-permutes the result
        perm = torch.cat([rope_pair_permutation(nh, hd), rope_pair_permutation(nkv, hd) + qs,
                          torch.arange(qs + kvs, N)]).to(DEV)
        w = w.index_select(0, perm).contiguous()
        rope = rope_table(max_seq, hd, 500000.0, DEV)
    qw, s, wd = quant(w)
    if rms:
        wd = wd[torch.argsort(perm)]
    y = xn.double() @ wd.T + (bias.double() if bias is not None else 0)
    q, k, v = (t.reshape(M, -1, hd) for t in y.split([qs, kvs, kvs], 1))
    if rms:
        hp = rope_pair_permutation(1, hd).to(DEV)
        q = ref.apply_rope(q.cpu(), tpos.cpu(), 500000.0).to(DEV)[..., hp]
        k = ref.apply_rope(k.cpu(), tpos.cpu(), 500000.0).to(DEV)[..., hp]
    kc = torch.zeros(slots, nkv, max_seq, hd, dtype=torch.bfloat16, device=DEV).to(kv)
    return (xn, qw, bias, kc, torch.zeros_like(kc), tslot, tpos, qs, kvs, hd, rope), s, (q, k, v), nkv * hd


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("kv", [torch.bfloat16, FP8])
@pytest.mark.parametrize("arch", ["gpt2", "llama"])
@pytest.mark.parametrize("M", [16, 80])
def test_gemm_w8_qkv_kv_append(C, CNT, arch, M, kv, splits):
    """bf16 cache and q: test_qkv_kv_append's 3e-2; FP8 cache: one E4M3 ulp,
    2^-3 |ref| + 2^-9, as tests/test_kv_fp8_gpu.py bounds its stores."""
    args, s, (q, k, v), row = _qkv_case(arch, M, kv)
    kc, vc, tslot, tpos = args[3:7]
    out = C.linear_qkv(*args, 0, splits, CNT, wscale=s)
    assert C.gemm_last_launch().startswith("w8<")
    close(out, q.reshape(M, -1), 3e-2)
    for got, want in ((kc, k), (vc, v)):
        got = got.float()[tslot.long(), :, tpos.long()]
        if kv == FP8:
            assert bool(((got - want).abs() <= 2.0 ** -3 * want.abs() + 2.0 ** -9).all())
        else:
            close(got, want, 3e-2)
    assert int((kc.float() != 0).sum()) <= M * row and int((vc.float() != 0).sum()) <= M * row  # nothing else written


def _backend(N, K):
    be = HipBackend()
    be._counters = torch.zeros(8, 1 << 16, dtype=torch.int32, device=DEV)
    be._wscratch = torch.full((1, N * K), 7.0, dtype=torch.bfloat16, device=DEV)
    return be


@pytest.mark.parametrize("M,K,w8", [(16, 768, True), (Routing().w8_max_m + 1, 768, False), (16, 800, False)])
def test_backend_route(C, M, K, w8):
    """Up to w8_max_m rows at K % 64 == 0 the backend's three GEMMs run the
    FP8-weight kernel and leave the dequant scratch alone; otherwise they dequantise."""
    from llm_sharding_demo_amd.ops import Residual

    N = 768
    be = _backend(N, K)
    q, s, wd = quant(bf(N, K, scale=0.05, seed=4))
    q._lsd_scale = s
    a, bias = bf(M, K, seed=5), bf(N, scale=0.1, seed=6)
    y = a.double() @ wd.T + bias.double()
    tags = []
    close(be.linear(a, q, bias), y, 3e-2)
    tags.append(C.gemm_last_launch())
    r = Residual(torch.zeros(M, N, device=DEV))
    be.linear_residual(a, q, bias, r)
    tags.append(C.gemm_last_launch())
    close(be.flush(r), y, 3e-2)
    if K == 768:  # the GPT-2 QKV shape (N = 3 x 6 x 64); its epilogue is checked above
        args, s2, _, _ = _qkv_case("gpt2", M, torch.bfloat16)
        args[1]._lsd_scale = s2
        meta = type("Meta", (), {"token_slots": args[5], "token_pos": args[6]})
        mcfg = type("Cfg", (), {"q_size": args[7], "kv_size": args[8], "head_dim": args[9]})
        be._wscratch = torch.full((1, args[1].numel()), 7.0, dtype=torch.bfloat16, device=DEV)
        be.qkv_kv_append(args[0], args[1], args[2], args[3], args[4], meta, mcfg)
        tags.append(C.gemm_last_launch())
    assert all(t.startswith("w8<") == w8 for t in tags), tags
    assert bool((be._wscratch == 7).all()) == w8


def test_refusals(C, CNT):
    a, s = bf(16, 128), torch.ones(64, device=DEV)
    q = torch.zeros(64, 128, device=DEV).to(FP8)
    for bad, msg in [(lambda: C.linear(a[:, :96].contiguous(), q[:, :96].contiguous(), None, 0, 0, 1, CNT, wscale=s), "K % 64"),
                     (lambda: C.linear(a[:, :64], q[:, 8:72], None, 0, 0, 1, CNT, wscale=s), "16-byte aligned"),
                     (lambda: C.linear(a, q, None, 0, 0, 1, CNT, wscale=s[:63]), "wscale"),
                     (lambda: C.linear(a, q, None, 0, 0, 1, CNT, wscale=s.double()), "wscale"),
                     (lambda: C.linear(a, q, None, 0, 1, 1, CNT, wscale=s), "kind 0"),
                     (lambda: C.linear(a, q.to(torch.bfloat16), None, 0, 0, 1, CNT, wscale=s), "dtype")]:
        with pytest.raises(RuntimeError, match=msg):
            bad()


def test_engine_w8_equals_dequant_route(monkeypatch):
    """Greedy ids on gpt2-test, 12 prompts at max_batch 16: graphs equal eager,
    and both equal the dequant route (w8_max_m = 0)."""
    from llm_sharding_demo_amd.runtime.engine import Engine

    kw = dict(model_id="gpt2-test", max_batch=16, device="cuda", max_seq_len=256, weight_dtype="fp8_e4m3")
    sp = SamplingParams(greedy=True, max_new_tokens=8)
    prompts = _prompts(get_model_config("gpt2-test").vocab_size, [3 + 2 * i for i in range(12)])
    ids = [Engine(EngineConfig(use_graphs=g, **kw), devices=["cuda:0"]).generate_ids(prompts, sp) for g in (True, False)]
    monkeypatch.setattr(HipBackend, "R", Routing.from_env("w8_max_m=0"))
    ids.append(Engine(EngineConfig(use_graphs=True, **kw), devices=["cuda:0"]).generate_ids(prompts, sp))
    assert ids[0] == ids[1] == ids[2]


@pytest.mark.parametrize("model,bounds", [("gpt2", "gpt2"), ("llama-test", "llama-3-8b")])
def test_model_matches_golden_at_batch_32(model, bounds):
    prompts = _prompts(get_model_config(model).vocab_size, [7 + 3 * i for i in range(32)])
    r = compare_with_golden(model, prompts, steps=4, weight_dtype="fp8_e4m3")
    print(model, r)
    top1, mx, mean = BOUNDS[bounds]
    h = r["hip_w"]
    assert h["top1_agreement"] >= top1 and h["max_rel_err"] < mx and h["mean_rel_err"] < mean, r
