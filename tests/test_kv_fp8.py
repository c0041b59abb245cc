"""FP8 (E4M3) KV cache without a GPU: the reference's saturating append, the
slot budget, the configuration switch and a CPU engine."""
import pytest
import torch

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.runtime.engine import Engine
from llm_sharding_demo_amd.runtime.kv_cache import plan_slots

FP8 = torch.float8_e4m3fn


def test_kv_append_saturates_and_round_trips():
    vals = torch.tensor([1000.0, -1000.0, 448.0, -448.0, 0.0, 2.0 ** -9, -0.875, 13.0, 30.0, 240.0])
    k = vals.reshape(1, 1, -1).repeat(2, 1, 1)
    kc, vc = (torch.zeros(3, 1, 4, vals.numel(), dtype=FP8) for _ in range(2))
    ref.kv_append(kc, vc, k, -k, torch.tensor([2, 0]), torch.tensor([1, 3]))
    want = vals.clamp(-448, 448)  # everything past the first two is representable
    for slot, pos in ((2, 1), (0, 3)):
        assert torch.equal(kc[slot, 0, pos].float(), want) and torch.equal(vc[slot, 0, pos].float(), -want)
    assert int((kc.float() != 0).sum()) == 2 * (vals != 0).sum()  # nothing else written


def test_plan_slots_fits_twice_the_bf16_count():
    kw = dict(fraction=1.0, mem_get_info=lambda dev: (1 << 30, 1 << 30))  # a whole number of slots
    n2 = plan_slots(10 ** 6, 4, 2, 256, 64, "cuda", elt=2, **kw)
    assert n2 == 2048 and plan_slots(10 ** 6, 4, 2, 256, 64, "cuda", elt=1, **kw) == 2 * n2


def test_unknown_kv_dtype_is_refused():
    with pytest.raises(ValueError):
        EngineConfig(model_id="gpt2-test", kv_dtype="fp8_e5m2")


def test_cpu_engine_same_tokens_with_and_without_a_prefix_hit():
    kw = dict(model_id="gpt2-test", max_batch=4, device="cpu", kv_dtype="fp8_e4m3")
    on, off = Engine(EngineConfig(prefix_cache=2, **kw)), Engine(EngineConfig(**kw))
    assert on.stages[0].kv.buf.dtype == FP8 and on.kv_info()["kv_dtype"] == "fp8_e4m3"
    a = [(7 * i + 3) % 200 + 1 for i in range(40)]
    b = a[:32] + [5, 9, 11]
    sp = SamplingParams(greedy=True, max_new_tokens=6)
    on.generate_requests([a], [sp])
    hit = on.generate_requests([b], [sp])[0]
    assert hit.cached_tokens > 0 and hit.output == off.generate_requests([b], [sp])[0].output
