"""gemm_w8_d256_kernel (launch kinds 2 / 3 with wscale): test_gemm_w8_gpu.py's cases and tolerances at 129-512 rows."""
import pytest
import torch

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams, get_model_config
from llm_sharding_demo_amd.ops import Residual, reference as ref
from llm_sharding_demo_amd.ops.hip import HipBackend, interleave_gate_up
from llm_sharding_demo_amd.ops.routing import Routing
from llm_sharding_demo_amd.runtime.engine import Engine
from llm_sharding_demo_amd.utils.golden import compare_with_golden

from .test_gemm_w8_gpu import _backend, _qkv_case, stale_workspace_rounds
from .test_kernels_gpu import C, CNT, DEV, _fp32_slabs, bf, close  # noqa: F401  (fixtures)
from .test_numerics_gpu import BOUNDS, _prompts
from .test_weight_fp8_gpu import FP8, quant

pytestmark = pytest.mark.gpu


def _qkv_rows(arch, M, kv):
    """_qkv_case past its 136 cache slots: cases of <= 136 rows (same seeded weight), each on 136 slots of its own."""
    parts = [_qkv_case(arch, m, kv) for m in [136] * (M // 136) + [M % 136]]
    a0, cat = parts[0][0], lambda i: torch.cat([p[0][i] for p in parts])
    kc = torch.zeros(136 * len(parts), *a0[3].shape[1:], dtype=torch.bfloat16, device=DEV).to(kv)
    tslot = torch.cat([p[0][5] + 136 * j for j, p in enumerate(parts)])
    args = (cat(0), a0[1], a0[2], kc, torch.zeros_like(kc), tslot, cat(6), *a0[7:])
    return args, parts[0][1], [torch.cat([p[2][i] for p in parts]) for i in range(3)], parts[0][3]


@pytest.mark.parametrize("slots,K", [(3, 64), (3, 192), (3, 1088), (3, 256), (2, 192), (4, 320)])
@pytest.mark.parametrize("M", [129, 256, 257, 300, 512])
def test_gemm_w8_rows_exact(C, CNT, M, K, slots):
    """test_gemm_w8_exact's integer construction (partial sums multiples of 1/4 below 2^24: float64's in any order).
    N = 1000 on kind 2 (partial last 64-column tile), N = 640 on kind 3 (128-column tiles: at most 3 slots).  M: one
    past w8_sk_max_m, a full block, one row / a ragged tail into a second, two blocks; K: 1, 3, 17 steps, refills."""
    C.gemm_set_d256_slots(slots)
    for N, kind in ((1000, 2), (640, 3)):
        g = torch.Generator(device=DEV).manual_seed(K + M + kind)
        wi = torch.randint(-7, 8, (N, K), device=DEV, generator=g).double()
        wi[:, K - 1] = 7
        w = wi * (2.0 ** torch.randint(-2, 3, (N, 1), device=DEV, generator=g).double())
        a = torch.randint(-3, 4, (M, K), device=DEV, generator=g).double()
        bias = torch.randint(-9, 10, (N,), device=DEV, generator=g).double()
        q, s = C.quantize_rows_fp8(w.bfloat16())
        assert torch.equal(q.float().double() * s.double()[:, None], w)
        y, ab, bb = a @ w.T + bias, a.bfloat16(), bias.bfloat16()
        for splits in (1, 3) if K >= 192 else (1,):
            assert torch.equal(C.linear(ab, q, bb, 0, kind, splits, CNT, wscale=s), y.float().bfloat16())
            assert C.gemm_last_launch() == f"w8d256<{64 * (kind - 1)},{min(slots, 6 - kind)}>"
            assert torch.equal(C.linear_f32(ab, q, kind, splits, CNT, wscale=s).double(), y - bias)
            for defer in (False, True):
                x = torch.randint(-50, 50, (M, N), device=DEV, generator=g).float()
                want = x.double() + y
                slab = C.linear_residual(ab, q, bb, x, splits, kind, CNT, defer, wscale=s)
                assert (slab is not None) == (defer or splits > 1)  # kinds 2 / 3 never combine a residual in-kernel
                if slab is not None:  # fp32 slabs: their sum is exact only if every partial was scaled
                    assert slab.dtype == torch.float32 and torch.equal(slab.double().sum(0), y - bias)
                    C.norm(x, slab, bb, None, None, 0.0, True, None, False)
                assert torch.equal(x.double(), want)
    C.gemm_set_d256_slots(3)
    assert int(CNT.abs().sum()) == 0  # every ticket counter re-armed


@pytest.mark.parametrize("kind", [2, 3])
def test_gemm_w8_rows_split_k_ignores_stale_workspace(C, CNT, kind):
    """Kind 3: 128-column tiles at N = 384, then 64-column tiles (N = 352 is no multiple of 128) on their counters."""
    stale_workspace_rounds(C, CNT, kind, (513, 384, 1600, 5), (255, 352, 320, 3))
    assert C.gemm_last_launch() == "w8d256<64,3>"


@pytest.mark.parametrize("kind,splits", [(2, 1), (2, 2), (3, 1), (3, 2)])
@pytest.mark.parametrize("M", [129, 300])
@pytest.mark.parametrize("epi", ["gelu", "silu_mul", "f32_segmax", "slab_bf16", "qkv_gpt2", "qkv_llama"])
def test_gemm_w8_rows_epilogues(C, CNT, epi, M, kind, splits):
    """test_gemm_w8_epilogues' and test_gemm_w8_qkv_kv_append's cases and tolerances on kinds 2 / 3."""
    N, K = 512 if epi == "silu_mul" else (1000 if kind == 2 else 640), 768
    a, w = bf(M, K, seed=1), bf(N, K, scale=0.05, seed=2)
    if epi == "silu_mul":  # gate and up rows get scales 16 times apart
        w[:N // 2], w[N // 2:] = w[:N // 2] * 0.25, w[N // 2:] * 4
    q, s, wd = quant(w)
    bias, y = bf(N, scale=0.1, seed=3), a.double() @ wd.T
    if epi == "gelu":  # test_linear: 3e-2
        close(C.linear(a, q, bias, 1, kind, splits, CNT, wscale=s), ref.gelu_new(y + bias.double()), 3e-2)
    elif epi == "silu_mul":  # test_linear: 3e-2
        qi = interleave_gate_up(q.view(torch.uint8), N // 2).contiguous().view(FP8)
        si = interleave_gate_up(s[:, None], N // 2).reshape(-1).contiguous()
        close(C.linear(a, qi, None, 2, kind, splits, CNT, wscale=si), ref.silu_mul(y[:, :N // 2], y[:, N // 2:]), 3e-2)
    elif epi == "f32_segmax":  # test_linear_residual_and_f32: 2e-3, 1e-3
        seg = torch.full((M, N // 8), float("nan"), device=DEV)
        out = C.linear_f32(a, q, kind, splits, CNT, seg, wscale=s)
        assert torch.equal(seg, out.view(M, N // 8, 8).amax(-1))
        close(out, y, 2e-3, 1e-3)
    elif epi == "slab_bf16":  # test_linear_residual_bf16_slabs' bounds: S bf16 roundings of the partials
        C.gemm_set_slab_bf16(1)
        x = torch.randn(M, N, device=DEV)
        want = x.double() + y + bias.double()
        slab = C.linear_residual(a, q, bias, x, max(splits, 2), kind, CNT, True, wscale=s)
        assert slab.dtype == torch.bfloat16
        C.norm(x, slab, bias, None, None, 0.0, True, None, False)
        err = (x.double() - want).abs()
        assert float(err.max()) <= 2.0 ** -8 * float(y.abs().max()) * max(splits, 2)
        assert float(err.mean()) <= 2.0 ** -9 * float(y.abs().mean()) * 2
    for kv in (torch.bfloat16, FP8) if epi.startswith("qkv") else ():
        args, s, (q, k, v), row = _qkv_rows(epi[4:], M, kv)
        kc, vc, tslot, tpos = args[3:7]
        close(C.linear_qkv(*args, kind, splits, CNT, wscale=s), q.reshape(M, -1), 3e-2)
        for got, want in ((kc, k), (vc, v)):
            got = got.float()[tslot.long(), :, tpos.long()]
            tol = 2.0 ** -3 * want.abs() + 2.0 ** -9 if kv == FP8 else 3e-2 + 2e-2 * want.abs()  # 1 ulp / close(3e-2)
            assert bool(((got - want).abs() <= tol).all())
        assert max(int((c.float() != 0).sum()) for c in (kc, vc)) <= M * row  # nothing else written
    assert C.gemm_last_launch().startswith("w8d256<")
    assert int(CNT.abs().sum()) == 0


@pytest.mark.parametrize("M,K,max_m,rows", [(129, 768, 512, True), (512, 768, 512, True), (129, 800, 512, False),
                                            (129, 768, 128, False)])
def test_backend_route_rows(C, M, K, max_m, rows):
    """w8_sk_max_m < M <= w8_max_m, K % 64 == 0: all three GEMMs on the all-rows kernel, scratch untouched."""
    N, be = 768, _backend(768, K)
    be.R = Routing().replace(w8_max_m=max_m)
    q, q._lsd_scale, _ = quant(bf(N, K, scale=0.05, seed=4))
    a, bias = bf(M, K, seed=5), bf(N, scale=0.1, seed=6)
    if K % 64:  # dequantised, and then no bf16 kernel takes K = 800 above 128 rows either
        with pytest.raises(RuntimeError, match="K % 64"):
            be.linear(a, q, bias)
        assert bool((be._wscratch != 7).any())
        return
    be.linear(a, q, bias)  # the numerics of all three are checked above
    tags = [C.gemm_last_launch()]
    r = Residual(torch.zeros(M, N, device=DEV))
    be.linear_residual(a, q, bias, r)
    tags.append(C.gemm_last_launch())
    args, s2, _, _ = _qkv_rows("gpt2", M, torch.bfloat16)  # the GPT-2 QKV shape; its epilogue is checked above
    args[1]._lsd_scale = s2
    meta = type("Meta", (), {"token_slots": args[5], "token_pos": args[6]})
    mcfg = type("Cfg", (), {"q_size": args[7], "kv_size": args[8], "head_dim": args[9]})
    scratch = be._wscratch
    be._wscratch = torch.full((1, args[1].numel()), 7.0, dtype=torch.bfloat16, device=DEV)
    be.qkv_kv_append(*args[:5], meta, mcfg)
    tags.append(C.gemm_last_launch())
    assert all(t.startswith("w8d256<") == rows for t in tags), tags
    assert bool((scratch == 7).all()) == bool((be._wscratch == 7).all()) == rows


@pytest.mark.parametrize("model,bounds", [("gpt2", "gpt2"), ("llama-test", "llama-3-8b")])
def test_model_matches_golden_at_batch_160(monkeypatch, model, bounds):
    """test_model_matches_golden_at_batch_32 with 160 prompts: decode steps of 160 rows, on the all-rows kernel."""
    kinds, kw = [], HipBackend._w8_kw
    monkeypatch.setattr(HipBackend, "_w8_kw", lambda *a, **k: kinds.append(kw(*a, **k)) or kinds[-1])
    monkeypatch.setattr(HipBackend, "R", Routing.from_env("w8_max_m=512"))
    prompts = _prompts(get_model_config(model).vocab_size, [3 + i % 9 for i in range(160)])
    r = compare_with_golden(model, prompts, steps=4, weight_dtype="fp8_e4m3")
    (top1, mx, mean), h = BOUNDS[bounds], r["hip_w"]
    assert h["top1_agreement"] >= top1 and h["max_rel_err"] < mx and h["mean_rel_err"] < mean, r
    assert kinds and all(kind >= 2 for kind, _ in kinds), kinds


def test_engine_w8_rows_graphs_equal_eager(monkeypatch):
    """Greedy ids on gpt2-test, 140 prompts in one decode batch: graphs equal eager (fixed-order combine)."""
    monkeypatch.setattr(HipBackend, "R", Routing.from_env("w8_max_m=512"))
    kw = dict(model_id="gpt2-test", max_batch=160, device="cuda", max_seq_len=64, weight_dtype="fp8_e4m3")
    sp = SamplingParams(greedy=True, max_new_tokens=8)
    prompts = _prompts(get_model_config("gpt2-test").vocab_size, [3 + i % 9 for i in range(140)])
    ids = [Engine(EngineConfig(use_graphs=g, **kw), devices=["cuda:0"]).generate_ids(prompts, sp) for g in (True, False)]
    assert ids[0] == ids[1]
