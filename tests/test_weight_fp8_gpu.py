"""Weight-only FP8 on the GPU: the row quantiser and dequantiser
(csrc/kernels/wquant.hip) bit for bit against ops/reference.py, the FP8-weight
GEMV (csrc/kernels/gemv.hip) against float64 over the dequantised weights with
the tolerances tests/test_gemv_gpu.py sets for the same epilogues, the dequant
route of the backend, and the model and the engine on FP8 weights."""
import pytest
import torch

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.runtime.engine import Engine
from llm_sharding_demo_amd.utils.golden import compare_with_golden

from .test_gemv_gpu import C, DEV, bf, close, norm_ref  # noqa: F401  (C: the fixture)
from .test_numerics_gpu import BOUNDS, _prompts

pytestmark = pytest.mark.gpu
FP8 = torch.float8_e4m3fn
NONE = (None,) * 5 + (0, 0, 0, None)  # gemv's resid .. rope arguments of a plain epilogue


def quant(w):
    """(q, scale) on the device from the CPU reference, and the float64 dequantised weight."""
    q, s = ref.quantize_rows(w.cpu())
    return q.to(DEV), s.to(DEV), ref.dequantize_rows(q, s).double().to(DEV)


def wcase(N, K):
    w = bf(N, K, seed=N + K)
    w[N // 2] = 0                 # a row of zeros: scale 1
    w[N - 1, K // 3] = 2.0 ** 15  # its row's other values land among the E4M3 subnormals
    return w


@pytest.mark.parametrize("N,K", [(5, 16), (130, 768), (64, 1600), (33, 14336)])
def test_quantizer_and_dequantizer_bit_equal(C, N, K):
    w = wcase(N, K)
    q_ref, s_ref = ref.quantize_rows(w.cpu())
    q, s = C.quantize_rows_fp8(w)
    assert torch.equal(s.cpu(), s_ref) and s_ref[N // 2] == 1.0
    assert torch.equal(q.cpu().view(torch.uint8), q_ref.view(torch.uint8))
    sub = q_ref[N - 1].float().abs()
    assert ((sub > 0) & (sub < 2.0 ** -6)).any()
    out = torch.full((N * K + 16,), 7.0, dtype=torch.bfloat16, device=DEV)
    d = C.dequant_rows_fp8(q, s, out)
    assert torch.equal(d.cpu(), (q_ref.float() * s_ref[:, None]).bfloat16()) and bool((out[N * K:] == 7).all())


# one chunk, a tail inside the second slot, and the first K past each K bucket (2048, 4096, 8192)
@pytest.mark.parametrize("K", [16, 1040, 2064, 4112, 8208])
@pytest.mark.parametrize("M", [1, 3, 8])
def test_gemv_fp8_exact(C, M, K):
    """Integer weights in [-7, 7] times a power of two per row (quantised
    without error: scale = 2^e / 64, q = 64 w), small integer activations and
    bias: every epilogue value is exact, so the outputs equal float64's."""
    if not C.gemv_ok(M, K, 0, 0, True):
        assert M > 1, "every K must run at M = 1"
        pytest.skip("shape not on the GEMV")
    N = 1000  # the last workgroup partial
    g = torch.Generator(device=DEV).manual_seed(K + M)
    wi = torch.randint(-7, 8, (N, K), device=DEV, generator=g).double()
    wi[:, K - 1] = 7
    w = wi * (2.0 ** torch.randint(-2, 3, (N, 1), device=DEV, generator=g).double())
    a = torch.randint(-3, 4, (M, K), device=DEV, generator=g).double()
    bias = torch.randint(-9, 10, (N,), device=DEV, generator=g).double()
    x = torch.randint(-50, 50, (M, N), device=DEV, generator=g).float()
    q, s = C.quantize_rows_fp8(w.bfloat16())
    assert torch.equal(q.float().double() * s.double()[:, None], w)
    y = a @ w.T + bias
    ab, bb = a.bfloat16(), bias.bfloat16()
    assert torch.equal(C.gemv(ab, q, bb, 0, 0, None, None, 0.0, *NONE, wscale=s), y.float().bfloat16())
    assert torch.equal(C.gemv(ab, q, bb, 3, 0, None, None, 0.0, *NONE, wscale=s).double(), y)
    want = x.double() + y
    C.gemv(ab, q, bb, 4, 0, None, None, 0.0, x, *NONE[1:], wscale=s)
    assert torch.equal(x.double(), want)


# every (epilogue, norm) pair lsd_gemv dispatches but QKV; (atol, rtol) of the matching test_gemv_gpu.py test
PAIRS = {(0, 0): (3e-2, 2e-2), (1, 0): (3e-2, 2e-2), (1, 1): (3e-2, 2e-2), (2, 0): (3e-2, 2e-2),
         (2, 2): (3e-2, 2e-2), (3, 0): (2e-3, 1e-3), (3, 1): (2e-2, 2e-2), (3, 2): (2e-2, 2e-2),
         (4, 0): (2e-3, 1e-3)}


@pytest.mark.parametrize("K", [768, 1600, 4096, 6400, 14336])
@pytest.mark.parametrize("M", [1, 2, 3, 8])
@pytest.mark.parametrize("epi,norm", list(PAIRS))
def test_gemv_fp8_epilogues(C, epi, norm, M, K):
    from llm_sharding_demo_amd.ops.hip import interleave_gate_up

    if not C.gemv_ok(M, K, epi, norm, True):
        # at M = 1 only the fused norm's own limit (4 rows x 2048 of K, as on bf16 weights) refuses a model K
        assert M > 1 or (norm and K > 8192)
        pytest.skip("shape not on the GEMV")
    N = 544 if epi == 2 else 1000
    q, s, wd = quant(bf(N, K, scale=0.03 if PAIRS[epi, norm][0] < 1e-2 else 0.05, seed=2))
    bias = None if epi == 2 else bf(N, scale=0.1, seed=3)
    gm = (1 + 0.1 * torch.randn(K, device=DEV)).bfloat16()
    bt = bf(K, scale=0.1, seed=7) if norm == 1 else None
    if norm:
        x = torch.randn(M, K, device=DEV) * 2 + 0.5
        a = norm_ref(x, gm, bt, norm == 2).bfloat16()
    else:
        x = a = bf(M, K, seed=1)
    y = a.double() @ wd.T + (bias.double() if bias is not None else 0)
    res = torch.randn(M, N, device=DEV)
    if epi == 1:
        y = ref.gelu_new(y)
    elif epi == 2:  # the kernel reads the 16-row interleaved layout: interleave q and its scales alike
        y = ref.silu_mul(y[:, :N // 2], y[:, N // 2:])
        q = interleave_gate_up(q.view(torch.uint8), N // 2).contiguous().view(FP8)
        s = interleave_gate_up(s[:, None], N // 2).reshape(-1).contiguous()
    elif epi == 4:
        y = y + res.double()
    out = C.gemv(x, q, bias, epi, norm, gm if norm else None, bt, 1e-5 if norm else 0.0,
                 res if epi == 4 else None, *NONE[1:], wscale=s)
    close(res if epi == 4 else out, y, *PAIRS[epi, norm])


@pytest.mark.parametrize("kv", [torch.bfloat16, FP8])
@pytest.mark.parametrize("arch", ["gpt2", "llama"])
@pytest.mark.parametrize("M", [1, 2, 5])
def test_gemv_fp8_qkv_kv_append(C, arch, M, kv):
    """test_gemv_qkv_kv_append's two cases (bias without RoPE, RoPE without
    bias) on FP8 weights, into a bf16 cache (its 3e-2) and an FP8 cache (one
    E4M3 ulp: 2^-3 |ref| + 2^-9, as tests/test_kv_fp8_gpu.py bounds its stores)."""
    from llm_sharding_demo_amd.ops.hip import rope_pair_permutation, rope_table

    hd, nh, nkv, H = (64, 6, 6, 768) if arch == "gpt2" else (128, 8, 2, 1024)
    qs, kvs, slots, max_seq, rms = nh * hd, nkv * hd, 6, 96, arch == "llama"
    N = qs + 2 * kvs
    w, bias = bf(N, H, scale=0.05, seed=12), (None if rms else bf(N, scale=0.1, seed=13))
    x = torch.randn(M, H, device=DEV)
    g, b = (1 + 0.1 * torch.randn(H, device=DEV)).bfloat16(), (None if rms else bf(H, scale=0.1, seed=14))
    xn = norm_ref(x, g, b, rms).bfloat16()
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
    for norm in ([0, 2 if rms else 1] if M <= 2 else [0]):
        kc = torch.zeros(slots, nkv, max_seq, hd, dtype=torch.bfloat16, device=DEV).to(kv)
        vc = torch.zeros_like(kc)
        out = C.gemv(x if norm else xn, qw, bias, 6, norm, g if norm else None, b if norm else None,
                     1e-5 if norm else 0.0, None, kc, vc, tslot, tpos, qs, kvs, hd, rope, wscale=s)
        close(out, q.reshape(M, -1), 3e-2)
        for got, want in ((kc, k), (vc, v)):
            got = got.float()[tslot.long(), :, tpos.long()]
            if kv == FP8:
                assert bool(((got - want).abs() <= 2.0 ** -3 * want.abs() + 2.0 ** -9).all())
            else:
                close(got, want, 3e-2)
        assert int((kc.float() != 0).sum()) <= M * nkv * hd  # nothing else written


@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("norm", [0, 1, 2])
@pytest.mark.parametrize("K,N", [(768, 1000), (4096, 2048)])
def test_gemv_fp8_logits_segmax(C, M, norm, K, N):
    if not C.gemv_ok(M, K, 3, norm, True):
        pytest.skip("shape not on the GEMV")
    x = torch.randn(M, K, device=DEV) * 2 + 0.3 if norm else bf(M, K, seed=2)
    gm, b = (1 + 0.1 * torch.randn(K, device=DEV)).bfloat16(), bf(K, scale=0.1, seed=3)
    args = (norm, gm, b if norm == 1 else None, 1e-5) if norm else (0, None, None, 0.0)
    q, s, wd = quant(bf(N, K, scale=0.05, seed=11))
    seg = torch.full((M, N // 8), float("nan"), device=DEV)
    y = C.gemv_logits(x, q, *args, seg, wscale=s)
    assert torch.equal(seg, y.view(M, N // 8, 8).amax(-1))
    a = norm_ref(x, gm, b, norm == 2).bfloat16() if norm else x
    close(y, a.double() @ wd.T, 2e-2, 2e-2)


def test_refused_shapes_take_the_dequant_route(C):
    """K % 16 != 0 and M = 9 are not the FP8 GEMV's; the backend then
    dequantises into its scratch and runs the GEMM it runs on bf16 weights."""
    from llm_sharding_demo_amd.ops.hip import HipBackend

    assert not C.gemv_ok(1, 776, 0, 0, True) and C.gemv_ok(1, 776, 0, 0)
    assert not C.gemv_ok(9, 768, 0, 0, True) and C.gemv_ok(8, 768, 0, 0, True)
    be = HipBackend()
    be._counters = torch.zeros(8, 1 << 16, dtype=torch.int32, device=DEV)
    N, K = 512, 768
    q, s, wd = quant(bf(N, K, scale=0.05, seed=4))
    q._lsd_scale = s
    be._wscratch = torch.empty(1, N * K, dtype=torch.bfloat16, device=DEV)
    a, bias = bf(9, K, seed=5), bf(N, scale=0.1, seed=6)
    close(be.linear(a, q, bias), a.double() @ wd.T + bias.double(), 3e-2)


@pytest.mark.parametrize("model,bounds", [("gpt2", "gpt2"), ("llama-test", "llama-3-8b")])
@pytest.mark.parametrize("batch", [1, 16])  # the GEMV route; the dequant route
def test_model_matches_golden_over_dequantised_weights(model, bounds, batch):
    from llm_sharding_demo_amd.config import get_model_config

    prompts = _prompts(get_model_config(model).vocab_size, [7 + 3 * i for i in range(batch)])
    r = compare_with_golden(model, prompts, steps=4, weight_dtype="fp8_e4m3")
    print(model, batch, r)
    top1, mx, mean = BOUNDS[bounds]  # llama-test: the Llama family's row
    h = r["hip_w"]
    assert h["top1_agreement"] >= top1 and h["max_rel_err"] < mx and h["mean_rel_err"] < mean, r


def test_engine_graphs_equal_eager_on_fp8_weights():
    kw = dict(model_id="gpt2-test", max_batch=8, device="cuda", max_seq_len=256)
    sp = SamplingParams(greedy=True, max_new_tokens=8)
    prompts = [[5, 9, 2, 77, 41], [100, 3]]
    e = Engine(EngineConfig(weight_dtype="fp8_e4m3", use_graphs=True, **kw), devices=["cuda:0"])
    assert e.kv_info()["weight_dtype"] == "fp8_e4m3" and e.stages[0].backend.name == "hip"
    assert e.stages[0].w["h.0.mlp.c_fc.weight"].dtype == FP8
    assert e._weight_bytes(0) < Engine(EngineConfig(**kw), devices=["cuda:0"])._weight_bytes(0)
    eager = Engine(EngineConfig(weight_dtype="fp8_e4m3", use_graphs=False, **kw), devices=["cuda:0"])
    assert e.generate_ids(prompts, sp) == eager.generate_ids(prompts, sp)
