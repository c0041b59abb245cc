"""Weight-only MXFP4 on the GPU: wquant.hip's block quantiser / dequantiser bit for bit against ops/reference.py,
gemv_mxfp4_kernel exactly on exact operands and against float64 over the dequantised weights (exact bf16, so the
tolerances are tests/test_weight_fp8_gpu.py's), the backend's dequant route, the model and the engine."""
import pytest
import torch

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams, get_model_config
from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.runtime.engine import Engine
from llm_sharding_demo_amd.utils.golden import compare_with_golden

from .test_gemv_gpu import C, DEV, bf, close, norm_ref  # noqa: F401  (C: the fixture)
from .test_numerics_gpu import BOUNDS, _prompts
from . import test_weight_fp8_gpu as fp8_tests
from .test_weight_fp8_gpu import FP8, NONE, PAIRS

pytestmark = pytest.mark.gpu
U8 = torch.uint8


def quant(w):
    """(q, e) on the device from the CPU reference, and the float64 dequantised weight."""
    q, e = ref.quantize_mx4(w.cpu())
    return q.view(U8).to(DEV).view(ref.FP4), e.view(U8).to(DEV).view(ref.E8M0), ref.dequantize_mx4(q, e).double().to(DEV)


@pytest.mark.parametrize("N,K", [(5, 32), (130, 768), (64, 1600), (33, 14336)])
def test_quantizer_and_dequantizer_bit_equal(C, N, K):
    w = bf(N, K, seed=N + K)
    w[N // 2] = 0                 # a row of zeros: scale bytes 127
    w[N - 1, K // 3] = 2.0 ** 15  # its block's other values land at 0 / 0.5
    ties = [.25, .75, 1.25, 1.75, 2.5, 3.5, 5]
    w[0, :32] = 0                 # a planted tie block under X = -3
    w[0, :15] = (torch.tensor([6] + ties + [-x for x in ties], device=DEV) / 8).bfloat16()
    q_ref, e_ref = ref.quantize_mx4(w.cpu())
    q, e = C.quantize_rows_mxfp4(w)
    assert q.dtype == ref.FP4 and e.dtype == ref.E8M0
    assert torch.equal(e.cpu().view(U8), e_ref.view(U8)) and bool((e_ref.view(U8)[N // 2] == 127).all())
    assert torch.equal(q.cpu().view(U8), q_ref.view(U8))
    d_ref, blk = ref.dequantize_mx4(q_ref, e_ref), (K // 3) // 32 * 32
    assert set(d_ref[N - 1, blk:blk + 32].abs().tolist()) <= {0.0, 2.0 ** 12, 2.0 ** 15}
    assert d_ref[0, :15].mul(8).tolist() == [6, 0, 1, 1, 2, 2, 4, 4, 0, -1, -1, -2, -2, -4, -4]
    out = torch.full((N * K + 16,), 7.0, dtype=torch.bfloat16, device=DEV)
    d = C.dequant_rows_mxfp4(q, e, out)
    assert torch.equal(d.cpu(), d_ref.bfloat16()) and bool((out[N * K:] == 7).all())


# one chunk, a tail inside the first slot, and the first block past each K bucket (2048, 4096, 8192)
@pytest.mark.parametrize("K", [32, 1056, 2080, 4128, 8224])
@pytest.mark.parametrize("M", [1, 3, 8])
def test_gemv_mxfp4_exact(C, M, K):
    """Weights on the E2M1 grid times a power of two per block (every block holds a 6: quantised without error),
    small integer activations and bias: every epilogue value is exact, so the outputs equal float64's."""
    if not C.gemv_ok(M, K, 0, 0, 2):
        assert M > 1, "every K must run at M = 1"
        pytest.skip("shape not on the GEMV")
    N = 1000  # the last workgroup partial at every CPW
    g = torch.Generator(device=DEV).manual_seed(K + M)
    rnd = lambda lo, hi, *s: torch.randint(lo, hi, s, device=DEV, generator=g)  # noqa: E731
    grid = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6], device=DEV, dtype=torch.float64)
    wi = grid[rnd(0, 8, N, K)] * (rnd(0, 2, N, K) * 2 - 1)
    wi[:, 31::32] = 6
    w = (wi.view(N, K // 32, 32) * 2.0 ** rnd(-2, 3, N, K // 32, 1).double()).view(N, K)
    a, bias, x = rnd(-3, 4, M, K).double(), rnd(-9, 10, N).double(), rnd(-50, 50, M, N).float()
    q, e = C.quantize_rows_mxfp4(w.bfloat16())
    assert torch.equal(ref.dequantize_mx4(q, e).double(), w)
    y = a @ w.T + bias
    ab, bb = a.bfloat16(), bias.bfloat16()
    assert torch.equal(C.gemv(ab, q, bb, 0, 0, None, None, 0.0, *NONE, wscale=e), y.float().bfloat16())
    assert torch.equal(C.gemv(ab, q, bb, 3, 0, None, None, 0.0, *NONE, wscale=e).double(), y)
    want = x.double() + y
    C.gemv(ab, q, bb, 4, 0, None, None, 0.0, x, *NONE[1:], wscale=e)
    assert torch.equal(x.double(), want)


@pytest.mark.parametrize("K", [768, 1600, 4096, 6400, 14336])
@pytest.mark.parametrize("M", [1, 2, 3, 8])
@pytest.mark.parametrize("epi,norm", list(PAIRS))
def test_gemv_mxfp4_epilogues(C, epi, norm, M, K):
    from llm_sharding_demo_amd.ops.hip import interleave_gate_up

    if not C.gemv_ok(M, K, epi, norm, 2):
        # at M = 1 only the fused norm's own limit (4 rows x 2048 of K, as on bf16 weights) refuses a model K
        assert M > 1 or (norm and K > 8192)
        pytest.skip("shape not on the GEMV")
    N = 544 if epi == 2 else 1000
    q, e, wd = quant(bf(N, K, scale=0.03 if PAIRS[epi, norm][0] < 1e-2 else 0.05, seed=2))
    bias = None if epi == 2 else bf(N, scale=0.1, seed=3)
    gm = (1 + 0.1 * torch.randn(K, device=DEV)).bfloat16()
    bt = bf(K, scale=0.1, seed=7) if norm == 1 else None
    x = torch.randn(M, K, device=DEV) * 2 + 0.5 if norm else bf(M, K, seed=1)
    a = norm_ref(x, gm, bt, norm == 2).bfloat16() if norm else x
    y = a.double() @ wd.T + (bias.double() if bias is not None else 0)
    res = torch.randn(M, N, device=DEV)
    if epi == 1:
        y = ref.gelu_new(y)
    elif epi == 2:  # the kernel reads the 16-row interleaved layout: interleave packed rows and scale rows alike
        y = ref.silu_mul(y[:, :N // 2], y[:, N // 2:])
        q = interleave_gate_up(q.view(U8), N // 2).contiguous().view(ref.FP4)
        e = interleave_gate_up(e.view(U8), N // 2).contiguous().view(ref.E8M0)
    elif epi == 4:
        y = y + res.double()
    out = C.gemv(x, q, bias, epi, norm, gm if norm else None, bt, 1e-5 if norm else 0.0,
                 res if epi == 4 else None, *NONE[1:], wscale=e)
    close(res if epi == 4 else out, y, *PAIRS[epi, norm])


@pytest.mark.parametrize("kv", [torch.bfloat16, FP8])
@pytest.mark.parametrize("arch", ["gpt2", "llama"])
@pytest.mark.parametrize("M", [1, 2, 5])
def test_gemv_mxfp4_qkv_kv_append(C, arch, M, kv, monkeypatch):
    """test_gemv_fp8_qkv_kv_append itself (bias without RoPE, RoPE without bias; 3e-2 into a bf16 cache, one E4M3 ulp
    into an FP8 cache; nothing else written) with its quant() replaced: the weight and wscale it passes are MXFP4."""
    monkeypatch.setattr(fp8_tests, "quant", quant)
    fp8_tests.test_gemv_fp8_qkv_kv_append(C, arch, M, kv)


@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("norm", [0, 1, 2])
@pytest.mark.parametrize("K,N", [(768, 1000), (4096, 2048)])
def test_gemv_mxfp4_logits_segmax(C, M, norm, K, N, monkeypatch):
    """test_gemv_fp8_logits_segmax the same way: maxima bit-equal to amax over the stored logits."""
    monkeypatch.setattr(fp8_tests, "quant", quant)
    fp8_tests.test_gemv_fp8_logits_segmax(C, M, norm, K, N)


def test_refused_shapes_take_the_dequant_route(C):
    """K % 32 != 0 is refused (prepare_stage keeps such a weight bf16); M = 9 dequantises into the backend's scratch."""
    from llm_sharding_demo_amd.ops.hip import HipBackend

    assert not C.gemv_ok(1, 784, 0, 0, 2) and C.gemv_ok(1, 784, 0, 0, True) and C.gemv_ok(1, 784, 0, 0)
    assert not C.gemv_ok(9, 768, 0, 0, 2) and C.gemv_ok(8, 768, 0, 0, 2)
    with pytest.raises(RuntimeError, match="K must be a multiple of 32"):
        C.quantize_rows_mxfp4(bf(8, 784))
    be = HipBackend()
    be._counters = torch.zeros(8, 1 << 16, dtype=torch.int32, device=DEV)
    N, K = 512, 768
    q, e, wd = quant(bf(N, K, scale=0.05, seed=4))
    q._lsd_scale = e
    a, bias = bf(9, K, seed=5), bf(N, scale=0.1, seed=6)
    with pytest.raises(RuntimeError, match="dequant_rows_mxfp4"):
        C.linear(a, q, bias, 0, 0, 1, be.counters)
    be._wscratch = torch.empty(1, N * K, dtype=torch.bfloat16, device=DEV)
    close(be.linear(a, q, bias), a.double() @ wd.T + bias.double(), 3e-2)


# batch 1: the GEMV route; batch 16: the dequant route
@pytest.mark.parametrize("model,bounds,batch", [("gpt2", "gpt2", 1), ("gpt2", "gpt2", 16), ("llama-test", "llama-3-8b", 1)])
def test_model_matches_golden_over_dequantised_weights(model, bounds, batch):
    prompts = _prompts(get_model_config(model).vocab_size, [7 + 3 * i for i in range(batch)])
    r = compare_with_golden(model, prompts, steps=4, weight_dtype="mxfp4")
    print(model, batch, r)
    top1, mx, mean = BOUNDS[bounds]  # llama-test: the Llama family's row
    h = r["hip_w"]
    assert h["top1_agreement"] >= top1 and h["max_rel_err"] < mx and h["mean_rel_err"] < mean, r


def test_engine_graphs_equal_eager_on_mxfp4_weights():
    kw = dict(model_id="gpt2-test", max_batch=8, device="cuda", max_seq_len=256)
    sp, prompts = SamplingParams(greedy=True, max_new_tokens=8), [[5, 9, 2, 77, 41], [100, 3]]
    e = Engine(EngineConfig(weight_dtype="mxfp4", use_graphs=True, **kw), devices=["cuda:0"])
    assert e.kv_info()["weight_dtype"] == "mxfp4" and e.stages[0].backend.name == "hip"
    assert e.stages[0].w["h.0.mlp.c_fc.weight"].dtype == ref.FP4
    eager = Engine(EngineConfig(weight_dtype="mxfp4", use_graphs=False, **kw), devices=["cuda:0"])
    assert e.generate_ids(prompts, sp) == eager.generate_ids(prompts, sp)
