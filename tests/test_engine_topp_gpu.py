"""Per-request top-p / min-p through the engine on an MI355X (gpt2-test, HIP
backend): the two per-row vectors live beside temperature / top-k in the last
stage's group state, are captured in the decode graphs and rewritten by
apply_rows when a group's composition changes."""
import pytest

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
from llm_sharding_demo_amd.runtime.engine import Engine

pytestmark = pytest.mark.gpu

PROMPTS = [[1, 2, 3, 4], [5, 6], list(range(10, 50)), [7] * 9, [3, 3]]


def _engine(graphs=True, **kw):
    cfg = EngineConfig(model_id="gpt2-test", num_stages=1, max_batch=16, device="cuda", use_graphs=graphs,
                       max_seq_len=512, **kw)
    e = Engine(cfg, devices=["cuda:0"])
    assert e.stages[0].backend.name == "hip"
    return e


def test_tiny_top_p_is_greedy():
    e = _engine()
    want = e.generate_ids(PROMPTS, SamplingParams(greedy=True, max_new_tokens=8))
    sps = [SamplingParams(temperature=1.3, top_k=k, top_p=1e-6, seed=i, max_new_tokens=8)
           for i, k in enumerate((40, 1000, 3, 200, 64))]
    assert e.generate_ids(PROMPTS, sps) == want
    assert e.generate_ids(PROMPTS, sps) == want  # replayed graphs


def test_cut_request_alone_in_a_changing_batch_and_without_graphs(monkeypatch):
    """A seeded top_p = 0.8 / min_p = 0.05 request draws the same ids alone and
    among default-parameter neighbours that leave at different steps (group
    compositions change; the native executor issues those items: packed row
    state with the two extra columns + the 14-word apply_rows record), with
    decode graphs on and off; the neighbours draw what they draw without it."""
    monkeypatch.setenv("LSD_NATIVE_EXEC", "1")
    cut = SamplingParams(temperature=1.0, top_k=40, top_p=0.8, min_p=0.05, seed=5, max_new_tokens=8)
    others = [SamplingParams(temperature=0.8, top_k=20, seed=11 + i, max_new_tokens=n)
              for i, n in enumerate((3, 6, 1, 5))]
    prompts, sps = PROMPTS, [others[0], others[1], cut, others[2], others[3]]
    e = _engine(num_microbatches=2)
    alone = e.generate_ids([PROMPTS[2]], [cut])[0]
    plain = e.generate_ids([PROMPTS[2]], [SamplingParams(temperature=1.0, top_k=40, seed=5, max_new_tokens=8)])[0]
    assert len(alone) == 8 and alone != plain  # the cut is live
    got = e.generate_ids(prompts, sps)
    assert got[2] == alone
    again = e.generate_ids(prompts, sps)  # graphs cached: native steps
    assert again == got
    assert sum(w.native_steps for w in e.workers) > 0
    assert sum(w.native_changes for w in e.workers) > 0
    without = e.generate_ids(prompts[:2] + prompts[3:], others)
    assert got[:2] + got[3:] == without
    assert _engine(graphs=False, num_microbatches=2).generate_ids(prompts, sps) == got
