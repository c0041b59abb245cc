"""Sequence scoring on the CPU (reference backend): Engine.score against a direct
log_softmax of the model's all-position logits, its validation, and POST /score."""
import pytest
import torch

from llm_sharding_demo_amd.config import EngineConfig
from llm_sharding_demo_amd.runtime.batch import BatchMeta
from llm_sharding_demo_amd.runtime.engine import Engine

SEQS = [[5, 9], [(7 * i + 3) % 1000 for i in range(33)], [(11 * i * i + 1) % 1000 for i in range(70)]]


@pytest.fixture(scope="module")
def engine():
    return Engine(EngineConfig(model_id="gpt2-test", max_batch=4, device="cpu", role="coordinator"))


def _direct(engine, seq):
    """float64 log_softmax of the single stage's logits at every position"""
    st = engine.stages[0]
    meta = BatchMeta.build([engine.kv_slots + 1], [0], [len(seq)], st.device)
    logits = st.forward(meta, torch.tensor(seq, dtype=torch.int32), all_logits=True)
    return torch.log_softmax(logits[:-1, : engine.mcfg.vocab_size].double(), dim=1)


def test_score_equals_direct_log_softmax(engine):
    for seq, sc in zip(SEQS, engine.score(SEQS)):
        lp = _direct(engine, seq)
        n = len(seq) - 1
        assert len(sc.token_logprobs) == len(sc.greedy_ids) == len(sc.greedy_logprobs) == n
        want = lp.gather(1, torch.tensor(seq[1:]).view(-1, 1))[:, 0]
        # fp32 logits shared; one fp32 rounding of lse and of the difference: |lp| < 16 -> 2 ulp = 2e-6
        assert (torch.tensor(sc.token_logprobs).double() - want).abs().max() < 2e-6
        assert sc.greedy_ids == lp.argmax(dim=1).tolist()
        assert (torch.tensor(sc.greedy_logprobs).double() - lp.max(dim=1).values).abs().max() < 2e-6
        for t, g, a, b in zip(seq[1:], sc.greedy_ids, sc.token_logprobs, sc.greedy_logprobs):
            assert t != g or a == b


BAD = [[], [[]], [[3]], [[1] * 5000], [[1, 1000]], [[-1, 4]]]


@pytest.mark.parametrize("seqs", BAD)
def test_score_validation(engine, seqs):
    with pytest.raises(ValueError):
        engine.score(seqs)


def test_http_score(engine):
    from fastapi.testclient import TestClient
    from llm_sharding_demo_amd.serving.server import create_app

    client = TestClient(create_app(engine.cfg, engine=engine))
    r = client.post("/score", json={"input_ids": SEQS[:2]})
    assert r.status_code == 200
    want = engine.score(SEQS[:2])
    for item, seq, sc in zip(r.json()["scores"], SEQS, want):
        assert set(item) == {"input_ids", "token_logprobs", "greedy_ids", "greedy_logprobs"}
        assert item["input_ids"] == seq and item["greedy_ids"] == sc.greedy_ids
        assert item["token_logprobs"] == sc.token_logprobs and item["greedy_logprobs"] == sc.greedy_logprobs
    t = client.post("/score", json={"texts": ["Hello there, world"]})
    assert t.status_code == 200 and len(t.json()["scores"][0]["token_logprobs"]) == len(t.json()["scores"][0]["input_ids"]) - 1
    for seqs in BAD:
        assert client.post("/score", json={"input_ids": seqs}).status_code == 422
    assert client.post("/score", json={}).status_code == 422
    assert client.post("/score", json={"texts": [""]}).status_code == 422
