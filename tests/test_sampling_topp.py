"""Per-request top-p / min-p sampling: host reference semantics, validation,
plan wire, the CPU engine and the HTTP API.

Semantics (ops/reference.py sample, csrc/kernels/sample.hip): after top-k, with
the candidates sorted by (value desc, index asc), e_i = exp(v_i/T - v_0/T) and
c their running sum, min-p keeps the n_m entries with e_i >= min_p, top-p the
shortest prefix n_p with c >= top_p * total, and the draw runs over the first
n = max(1, min(n_p, n_m)) entries.
"""
import collections
import pickle

import pytest
import torch

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.runtime.batch import counter_uniform
from llm_sharding_demo_amd.runtime.engine import Engine
from llm_sharding_demo_amd.runtime.plan import (MAGIC_PICKLE, Chunk, GroupPlan, PlanDecoder, PlanEncoder, Row,
                                                StepPlan)

PROBS = [0.5, 0.25, 0.15, 0.1]


def _draws(logits, T, k, top_p, min_p, steps, seed=1234):
    """Sampled id of a one-row batch at every step of one seed."""
    f = lambda v: None if v is None else torch.tensor([v], dtype=torch.float32)  # noqa: E731
    out = []
    for s in range(steps):
        u = counter_uniform(torch.tensor([seed]), torch.tensor([s]))
        out.append(int(ref.sample(logits, torch.tensor([T]), torch.tensor([k], dtype=torch.int32),
                                  torch.zeros(1, dtype=torch.int32), u, logits.shape[1], f(top_p), f(min_p))[0]))
    return out


@pytest.mark.parametrize("top_p,min_p,support", [(0.7, None, {0, 1}), (0.5, None, {0}), (None, 0.4, {0, 1}),
                                                 (0.4, 0.4, {0}), (1e-6, None, {0})])
def test_hand_made_rows(top_p, min_p, support):
    logits = torch.log(torch.tensor([PROBS]))
    assert set(_draws(logits, 1.0, 4, top_p, min_p, 400)) == support


def test_tiny_top_p_equals_greedy():
    torch.manual_seed(3)
    logits = torch.randn(6, 300) * 2
    B = logits.shape[0]
    u = counter_uniform(torch.arange(B) + 5, torch.full((B,), 2))
    got = ref.sample(logits, torch.full((B,), 0.8), torch.full((B,), 40, dtype=torch.int32),
                     torch.zeros(B, dtype=torch.int32), u, 300, torch.full((B,), 1e-6), torch.zeros(B))
    assert got.tolist() == logits.argmax(1).tolist()


def test_nucleus_distribution():
    """Ids inside the nucleus appear at their renormalised probability (within
    0.05, the bound of test_topk_support_and_distribution); none outside."""
    torch.manual_seed(0)
    logits = torch.randn(1, 500) * 3
    T, k, top_p, n = 0.6, 40, 0.8, 3000
    vals, idx = torch.topk(logits[0].double() / T, k)
    p = torch.softmax(vals, 0)
    n_p = int(torch.nonzero(torch.cumsum(p, 0) >= top_p)[0]) + 1
    assert 2 <= n_p < k
    inside = idx[:n_p].tolist()
    want = (p[:n_p] / p[:n_p].sum()).tolist()
    counts = collections.Counter(_draws(logits, T, k, top_p, None, n))
    assert set(counts) <= set(inside)
    for t, w in zip(inside, want):
        assert abs(counts[t] / n - w) < 0.05


def test_explicit_defaults_equal_the_plain_call():
    torch.manual_seed(1)
    B, V = 16, 400
    logits = torch.randn(B, V) * 2
    temp = torch.linspace(0.5, 1.5, B)
    topk = torch.tensor([1, 2, 5, 40, 64, 100, 200, 40] * 2, dtype=torch.int32)
    greedy = torch.tensor([0] * 14 + [1, 1], dtype=torch.int32)
    for step in range(4):
        u = counter_uniform(torch.arange(B) * 31 + 7, torch.full((B,), step))
        plain = ref.sample(logits, temp, topk, greedy, u, V)
        assert ref.sample(logits, temp, topk, greedy, u, V, torch.ones(B), torch.zeros(B)).tolist() == plain.tolist()
        assert ref.sample(logits, temp, topk, greedy, u, V, None, None).tolist() == plain.tolist()


def test_validation():
    for kw in (dict(top_p=0.0), dict(top_p=1.5), dict(min_p=-0.1), dict(min_p=1.5)):
        with pytest.raises(ValueError):
            SamplingParams(**kw).validate()
        SamplingParams(greedy=True, **kw).validate()  # greedy requests ignore both
    SamplingParams(top_p=1.0, min_p=0.0).validate()
    SamplingParams(top_p=0.3, min_p=1.0).validate()
    assert SamplingParams().top_p == 1.0 and SamplingParams().min_p == 0.0


def test_plan_wire_round_trip():
    plan = StepPlan(step=7, groups=[
        GroupPlan(0, ret=2, n=2, b=2, ctxb=256,
                  chunks=[Chunk(1, 3, 0, [5, 6, 7], True, 0.7, 40, False, 11, 0.8, 0.05),
                          Chunk(2, 4, 0, [8], True, 0.6, 40, False, 12)],
                  rows=[Row(3, 5, 9, 0.9, 20, False, 13, 4, 0, 0.123456789012345, 0.3),
                        Row(4, 6, 2, 0.6, 40, True, 14, 1, 1)]),
        GroupPlan(1, ret=1, n=1, b=1, ctxb=256, rows=[Row(5, 7, 3, 0.6, 40, False, 15, 2, 0)])])
    enc, dec = PlanEncoder(), PlanDecoder()
    rec, payload = enc.encode(plan)
    assert rec[0] == MAGIC_PICKLE
    out = dec.decode(rec, lambda n: payload)
    assert out == plan
    g0, g1 = out.groups
    assert (g0.chunks[0].top_p, g0.chunks[0].min_p) == (0.8, 0.05)
    assert (g0.chunks[1].top_p, g0.chunks[1].min_p) == (1.0, 0.0)  # built without them
    assert (g0.rows[0].top_p, g0.rows[0].min_p) == (0.123456789012345, 0.3)
    assert (g0.rows[1].top_p, g0.rows[1].min_p) == (1.0, 0.0)
    assert (g1.rows[0].top_p, g1.rows[0].min_p) == (1.0, 0.0)
    assert pickle.loads(pickle.dumps(plan)) == plan


def _eng(P=1, **kw):
    return Engine(EngineConfig(model_id="gpt2-test", num_stages=P, max_batch=4, device="cpu", **kw))


def test_engine_top_p_across_stage_counts_and_batches():
    sp = SamplingParams(temperature=1.0, top_k=40, top_p=0.8, seed=99, max_new_tokens=6)
    alone = [_eng(P).generate_ids([[1, 2, 3]], [sp])[0] for P in (1, 2, 4)]
    assert alone[0] == alone[1] == alone[2]
    others = [SamplingParams(temperature=0.7, top_k=5, seed=3, max_new_tokens=4),
              SamplingParams(greedy=True, max_new_tokens=8),
              SamplingParams(temperature=1.2, top_k=100, top_p=0.5, min_p=0.1, seed=4, max_new_tokens=3)]
    outs = _eng().generate_ids([[4], [1, 2, 3], [9, 8, 7, 6], [5, 5]], [others[0], sp, others[1], others[2]])
    assert outs[1] == alone[0]
    # the cut is live: the same seed without it draws other ids somewhere
    plain = SamplingParams(temperature=1.0, top_k=40, seed=99, max_new_tokens=6)
    assert _eng().generate_ids([[1, 2, 3]], [plain])[0] != alone[0]


def test_engine_tiny_top_p_is_greedy():
    prompts = [[1, 2, 3], [4], [7, 7, 7, 7]]
    e = _eng()
    want = e.generate_ids(prompts, SamplingParams(greedy=True, max_new_tokens=6))
    sps = [SamplingParams(temperature=1.3, top_k=k, top_p=1e-6, seed=s, max_new_tokens=6)
           for k, s in ((40, 1), (1000, 2), (3, 3))]  # 1000 = the whole gpt2-test vocabulary
    assert e.generate_ids(prompts, sps) == want


@pytest.fixture(scope="module")
def client():
    from fastapi.testclient import TestClient

    from llm_sharding_demo_amd.serving.server import create_app

    cfg = EngineConfig(model_id="gpt2-test", max_batch=4, device="cpu", role="coordinator")
    return TestClient(create_app(cfg, engine=Engine(cfg)))


def test_http_generate_accepts_and_validates(client):
    r = client.post("/generate", json={"prompt": "Hi, ", "max_new_tokens": 3, "top_p": 0.9, "min_p": 0.05})
    assert r.status_code == 200 and r.json()["generated"].startswith("Hi, ")
    assert client.post("/generate", json={"prompt": "Hi, ", "max_new_tokens": 3, "top_p": 0}).status_code == 422
    assert client.post("/generate", json={"prompt": "Hi, ", "max_new_tokens": 3, "min_p": -0.1}).status_code == 422
    spec = client.get("/openapi.json").json()
    props = spec["components"]["schemas"]["GenerateReq"]["properties"]
    assert "top_p" in props and "min_p" in props


def test_client_and_llm_forward_the_fields(monkeypatch):
    import requests

    from llm_sharding_demo_amd import LLM
    from llm_sharding_demo_amd.serving import client as cl

    sent = {}

    class R:
        status_code = 200

        def json(self):
            return {"generated": "x"}

    def post(url, json=None, timeout=None):
        sent.update(json)
        return R()

    monkeypatch.setattr(requests, "post", post)
    cl.generate_text("Hi, ", top_p=0.9, min_p=0.05)
    assert sent["top_p"] == 0.9 and sent["min_p"] == 0.05
    sent.clear()
    cl.generate_text("Hi, ")
    assert "top_p" not in sent and "min_p" not in sent
    llm = LLM(EngineConfig(model_id="gpt2-test", max_batch=4, device="cpu"))
    g = llm.generate_text("Hi, ", max_new_tokens=4, greedy=True)
    assert llm.generate_text("Hi, ", max_new_tokens=4, temperature=1.5, top_p=1e-6, seed=5) == g
    with pytest.raises(ValueError):
        llm.generate_text("Hi, ", max_new_tokens=4, top_p=0.0)
