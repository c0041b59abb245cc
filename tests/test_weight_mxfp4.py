"""Weight-only MXFP4 (E2M1 nibbles, one E8M0 scale byte per 32 k) on the CPU
path: the reference quantiser against the format's rule, the config field, and
an engine that runs on MXFP4 weights."""
import pytest
import torch

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.runtime.engine import Engine

T = -3  # the planted block's values are these times 2^T
TIES, TIED = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]  # ties go to the even mantissa bit
# kind: (leading values of the block (the rest zeros), X - T, their dequantised values)
CASES = {"zeros": ([], -T, []),
         "six": ([6, -4, 3, 1.5, .5], 0, [6, -4, 3, 1.5, .5]),
         "four": ([4, -3, 2, 1, .5], 0, [4, -3, 2, 1, .5]),
         "three": ([3, -1.5, 1, .75, .25], -1, [3, -1.5, 1, .75, .25]),  # 3 2^t = 6 2^(t-1)
         "above_six": ([6 + 2.0 ** -5, 4], 1, [6, 4]),                   # the next bf16 above 6 2^t reads 3.01 2^(t+1)
         "ties": ([6] + TIES + [-x for x in TIES], 0, [6] + TIED + [-x for x in TIED]),
         "random": None}


@pytest.mark.parametrize("kind", list(CASES))
def test_quantize_mx4(kind):
    """Block 1 of row 1 is planted.  Everywhere |W' - w| <= amax_block / 4: with
    r = amax / 2^X in (3, 6], elements in [4, 6] err by at most 1, in [2, 4] by
    0.5, below by 0.25; that is amax / 4 at r >= 4 and below amax / 6 at r < 4."""
    w = (torch.randn(4, 96, generator=torch.Generator().manual_seed(5)) * 0.3).bfloat16()
    if CASES[kind]:
        vals, dx, want = CASES[kind]
        w[1, 32:64] = 0
        w[1, 32:32 + len(vals)] = (torch.tensor(vals) * 2.0 ** T).bfloat16()
    q, e = ref.quantize_mx4(w)
    assert q.dtype == ref.FP4 and q.shape == (4, 48) and e.dtype == ref.E8M0 and e.shape == (4, 3)
    eb, d = e.view(torch.uint8), ref.dequantize_mx4(q, e)
    assert eb.min() >= 1 and eb.max() <= 254 and torch.equal(d.bfloat16().float(), d)
    amax = w.float().reshape(4, 3, 32).abs().amax(2)
    assert ((d - w.float()).abs().reshape(4, 3, 32) <= amax[:, :, None] / 4).all()
    if CASES[kind]:
        assert int(eb[1, 1]) == T + dx + 127
        assert d[1, 32:64].tolist() == [x * 2.0 ** T for x in want] + [0.0] * (32 - len(want))
    if kind == "ties":  # element 2i in bits 3:0 of byte i, element 2i + 1 in bits 7:4, sign in bit 3 / 7
        assert q.view(torch.uint8)[1, 16:24].tolist() == [0x07, 0x22, 0x44, 0x66, 0xA8, 0xCA, 0xEC, 0x0E]


def test_weight_dtype_config(monkeypatch):
    assert EngineConfig(model_id="gpt2-test", weight_dtype="mxfp4").weight_dtype == "mxfp4"
    with pytest.raises(ValueError):
        EngineConfig(model_id="gpt2-test", weight_dtype="mxfp6")
    monkeypatch.setenv("WEIGHT_DTYPE", "mxfp4")
    assert EngineConfig.from_env().weight_dtype == "mxfp4"


@pytest.mark.parametrize("model", ["gpt2-test", "llama-test"])
def test_cpu_engine_runs_on_mxfp4_weights(model):
    """The tokens equal those of a bf16-config engine whose weights were
    replaced by the dequantised ones: both sides then do the same arithmetic."""
    kw = dict(model_id=model, max_batch=4, device="cpu")
    on, off = Engine(EngineConfig(weight_dtype="mxfp4", **kw)), Engine(EngineConfig(**kw))
    assert on.kv_info()["weight_dtype"] == "mxfp4"
    assert on._weight_bytes(0) < Engine(EngineConfig(weight_dtype="fp8_e4m3", **kw))._weight_bytes(0)
    w_on, w_off = on.stages[0].w, off.stages[0].w
    quantised = [k for k, v in w_on.items() if v.dtype == ref.FP4]
    assert len(quantised) == 4 * on.mcfg.n_layers
    assert all(k.endswith(tuple(on.mcfg.block_linears())) for k in quantised)
    for k in quantised:
        N, K = w_off[k].shape
        assert w_on[k].shape == (N, K // 2) and w_on[k]._lsd_scale.shape == (N, K // 32)
        w_off[k] = ref.dequantize_mx4(w_on[k], w_on[k]._lsd_scale)
    sp = SamplingParams(greedy=True, max_new_tokens=6)
    assert on.generate_ids([[5, 9, 2, 77], [100, 3]], sp) == off.generate_ids([[5, 9, 2, 77], [100, 3]], sp)
