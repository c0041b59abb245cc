"""Per-request token logprobs and top-N alternatives on the CPU: the host
reference (ops/reference.py logprobs), the probe rows, validation, the plan
wire, the CPU engine at several stage counts and the HTTP / client callers.

Semantics: logprobs are the log-softmax over [0, vocab) of the fp32 logits the
sampler drew from (after penalties, temperature 1, before the cuts); the
alternatives come value descending (numeric: -0.0 == +0.0), index ascending;
the drawn token's logprob is bit-equal to its entry among them.
"""
import dataclasses
import math
import pickle
import time

import numpy as np
import pytest
import torch

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.runtime.engine import Engine
from llm_sharding_demo_amd.runtime.plan import (MAGIC_PICKLE, Chunk, GroupPlan, PlanDecoder, PlanEncoder, Row,
                                                StepPlan)

from . import logprob_probes as lpp


def _ref(row, V, n, tok, W=lpp.MAXW):
    t, ti, tv = ref.logprobs(torch.from_numpy(np.asarray(row)[None]), torch.tensor([tok]), [n], V, W)
    return float(t[0]), ti[0].tolist(), tv[0].double().numpy()


def test_reference_hand_made_rows():
    # two equal entries and nothing else: ln 2 each, lower index first
    row = [0.0, -math.inf, 0.0, -math.inf]
    t, ids, lps = _ref(np.float32(row), 4, 3, 2, W=4)
    assert ids == [0, 2, 1, -1] and t == np.float32(-math.log(2.0))
    assert lps[0] == lps[1] == t and lps[2] == -math.inf and lps[3] == -math.inf
    # softmax of (1, 2, 3), padding columns never counted
    row = np.float32([1.0, 2.0, 3.0, math.inf, 3e38, 3e38, 3e38, 3e38])
    t, ids, lps = _ref(row, 3, 2, 0, W=3)
    z = math.log(math.exp(1) + math.exp(2) + math.exp(3))
    assert ids == [2, 1, -1] and abs(t - (1 - z)) < 1e-6 and abs(lps[0] - (3 - z)) < 1e-6
    # rows that did not ask: an empty record
    t, ti, tv = ref.logprobs(torch.zeros(2, 8), torch.tensor([1, 1]), [-1, 0], 8, 2)
    assert t[0] == -math.inf and ti.tolist() == [[-1, -1], [-1, -1]] and abs(float(t[1]) + math.log(8)) < 1e-6
    assert (tv == -math.inf).all()


CASES = lpp.case_list()


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_probe_rows_have_their_answer_and_path(c):
    assert lpp.predict_path(c["row"], c["V"], c["n"]) == c["path"]
    lse, tok_lp, ids, lps = lpp.expect(c["row"], c["V"], c["n"], c["tok"])
    if "lse" in c:
        assert abs(lse - c["lse"]) < 1e-12
    if "ids" in c:
        assert ids[: len(c["ids"])].tolist() == list(c["ids"])
    assert not (set(ids.tolist()) & set(range(c["V"], c["ld"])))
    # the float64 recomputation and the reference agree: ids exactly, values to
    # fp32 rounding of lse and of the difference (|lp| < 64 here: 2^-18 each)
    t, rid, rlp = _ref(c["row"], c["V"], c["n"], c["tok"])
    assert rid == ids.tolist()
    fin = np.isfinite(lps)
    assert np.array_equal(np.isfinite(rlp), fin) and np.abs(rlp[fin] - lps[fin]).max(initial=0) < 2.0 ** -16
    assert (t == tok_lp) if not math.isfinite(tok_lp) else abs(t - tok_lp) < 2.0 ** -16
    if c["tok"] in rid:  # bit-equal to its entry among the alternatives
        assert np.float32(t).tobytes() == np.float32(rlp[rid.index(c["tok"])]).tobytes()


def test_probe_set_covers_every_path_and_the_exact_values():
    assert {c["path"] for c in CASES} == {"one>rank", "one>overflow", "one>tau-inf>rank", "one>tau-inf>overflow",
                                          "one>nosel", "stream>rank", "stream>overflow", "stream>tau-inf>overflow"}
    single = next(c for c in CASES if c["name"] == "single-finite")
    assert _ref(single["row"], single["V"], 5, single["tok"])[0] == 0.0  # exactly
    cover = [c for c in CASES if c["name"].startswith("cover-")]
    assert len(cover) == 6 + 7  # V - 1 starts the last float4 (V % 4 == 1) and, at 53249, follows the chunk seam
    for c in cover:  # ln 2 to fp32 rounding; ln 3 or 0 would be a doubled / skipped position
        assert _ref(c["row"], c["V"], 2, c["tok"])[0] == -np.float32(math.log(2.0))


def test_reference_float64_sum_is_near_exact():
    """The reference's float64 lse against a compensated (fsum) evaluation on a
    random row of the largest shape: within 1e-7; its fp32 results add the
    rounding of lse (16 <= lse < 32: 2^-20) and of the difference (2^-21)."""
    g = torch.Generator().manual_seed(9)
    row = (torch.randn(1, 128256, generator=g) * 3).float()
    x = row[0].double().numpy()
    m = x.max()
    exact = m + math.log(math.fsum(np.exp(x - m).tolist()))
    assert 16 <= exact < 32 and abs(float(ref.lse64(row[0])) - exact) < 1e-7
    t, _, _ = ref.logprobs(row, torch.tensor([5]), [0], 128256, 1)
    assert abs((float(row[0, 5]) - exact) - float(t[0])) < 1e-7 + 2.0 ** -20 + 2.0 ** -21


def test_validate_bounds():
    assert SamplingParams().logprobs is None
    SamplingParams().validate()
    for ok in (0, 1, 5):
        SamplingParams(logprobs=ok).validate(5)
        SamplingParams(greedy=True, logprobs=ok).validate(5)
    SamplingParams(logprobs=20).validate()  # the hard ceiling
    for bad in (-1, 6, 1.0, "3", True):
        with pytest.raises(ValueError):
            SamplingParams(logprobs=bad).validate(5)
    with pytest.raises(ValueError):
        SamplingParams(logprobs=21).validate()
    with pytest.raises(ValueError):
        EngineConfig(max_logprobs=21)
    assert EngineConfig().max_logprobs == 5


def _plan(lp_chunk=None, lp_row=None):
    ck = {} if lp_chunk is None else {"logprobs": lp_chunk}
    rk = {} if lp_row is None else {"logprobs": lp_row}
    return StepPlan(step=7, groups=[
        GroupPlan(0, ret=2, n=2, b=2, ctxb=256,
                  chunks=[Chunk(1, 3, 0, [5, 6, 7], True, 0.7, 40, False, 11, **ck),
                          Chunk(2, 4, 0, [8], True, 0.6, 40, False, 12)],
                  rows=[Row(3, 5, 9, 0.9, 20, False, 13, 4, 0, **rk),
                        Row(4, 6, 2, 0.6, 40, True, 14, 1, 1)])])


def test_plan_wire_with_and_without_the_column():
    plan = _plan(3, 0)
    rec, payload = PlanEncoder().encode(plan)
    assert rec[0] == MAGIC_PICKLE
    out = PlanDecoder().decode(rec, lambda n: payload)
    assert out == plan and pickle.loads(pickle.dumps(plan)) == plan
    g0 = out.groups[0]
    assert (g0.chunks[0].logprobs, g0.chunks[1].logprobs) == (3, -1)
    assert (g0.rows[0].logprobs, g0.rows[1].logprobs) == (0, -1)
    # a plan without a logprob entry packs the columns it packed before the
    # field existed: 7 per chunk, 8 per row, and decodes to the defaults
    from llm_sharding_demo_amd.runtime.plan import _pack_group

    packed = _pack_group(_plan().groups[0], True)
    assert packed[7][0].shape == (2, 7) and packed[8][0].shape == (2, 8)
    packed = _pack_group(plan.groups[0], True)
    assert packed[7][0].shape == (2, 8) and packed[8][0].shape == (2, 9)
    _, p_without = PlanEncoder().encode(_plan())
    assert len(p_without) < len(payload)
    r0, p0 = PlanEncoder().encode(_plan())
    assert PlanDecoder().decode(r0, lambda n: p0) == _plan()
    only_row = _plan(None, 5)  # each of the two tables decides for itself
    r2, p2 = PlanEncoder().encode(only_row)
    assert PlanDecoder().decode(r2, lambda n: p2) == only_row


# ---------------------------------------------------------------------------
# engine (gpt2-test on the CPU)

def _eng(P=1, max_batch=4, **kw):
    return Engine(EngineConfig(model_id="gpt2-test", num_stages=P, max_batch=max_batch, device="cpu", **kw))


PROMPT = [1, 2, 3]
N = 12
GREEDY = SamplingParams(greedy=True, max_new_tokens=N, logprobs=3)
SEEDED = SamplingParams(temperature=1.0, top_k=40, seed=7, max_new_tokens=N, logprobs=5)
PENAL = SamplingParams(greedy=True, max_new_tokens=N, presence_penalty=2.0, frequency_penalty=2.0, logprobs=2)
ASK = [GREEDY, SEEDED, PENAL]


def _off(sp):
    return dataclasses.replace(sp, logprobs=None)


@pytest.fixture(scope="module")
def runs():
    e = _eng()
    return e, [e.generate_requests([PROMPT], [sp])[0] for sp in ASK]


def _check_record(req, n):
    lp = req.logprobs
    assert lp.tokens == req.output
    assert len(lp.tokens) == len(lp.token_logprobs) == len(lp.top_logprobs) == len(req.output)
    for tok, tl, alts in zip(lp.tokens, lp.token_logprobs, lp.top_logprobs):
        assert len(alts) == n and tl <= 0.0
        vals = [v for _, v in alts]
        assert vals == sorted(vals, reverse=True)
        for i, v in alts:
            if i == tok:
                assert v == tl  # the same float


def test_engine_tokens_do_not_change(runs):
    e, reqs = runs
    for sp, r in zip(ASK, reqs):
        assert e.generate_ids([PROMPT], [_off(sp)])[0] == r.output and len(r.output) == N
        assert r.logprobs is not None
        _check_record(r, sp.logprobs)
    plain = e.generate_requests([PROMPT], [_off(GREEDY)])[0]
    assert plain.logprobs is None
    assert e.generate_ids([PROMPT], [GREEDY]) == [reqs[0].output]  # generate_ids returns what it returned


def test_engine_greedy_draw_is_the_first_alternative(runs):
    _, reqs = runs
    for r in (reqs[0], reqs[2]):  # the penalised one too: the record is of the penalised logits
        lp = r.logprobs
        for tok, tl, alts in zip(lp.tokens, lp.token_logprobs, lp.top_logprobs):
            assert alts[0] == (tok, tl)
    assert reqs[2].output != reqs[0].output  # the penalties are live


def test_engine_records_are_the_reference_on_the_logits(runs):
    """Draw 0 of the greedy request against a forward of the prompt."""
    e, reqs = runs
    from llm_sharding_demo_amd.runtime.batch import BatchMeta

    st = e.stages[0]
    meta = BatchMeta.build([e.kv_slots + 1], [0], [len(PROMPT)], st.device)
    logits = st.forward(meta, torch.tensor(PROMPT, dtype=torch.int32), all_logits=True)[-1:]
    V = e.mcfg.vocab_size
    t, ti, tv = ref.logprobs(logits, torch.tensor([reqs[0].output[0]]), [3], V, 3)
    # another GEMM shape than the engine's prefill (all rows, not the last): close, not bit-equal
    assert abs(reqs[0].logprobs.token_logprobs[0] - float(t[0])) < 1e-4
    got = reqs[0].logprobs.top_logprobs[0]
    assert [i for i, _ in got] == ti[0].tolist()
    assert max(abs(v - w) for (_, v), w in zip(got, tv[0].tolist())) < 1e-4


@pytest.mark.parametrize("P", [2, 4])
def test_engine_same_records_at_every_stage_count(runs, P):
    _, reqs = runs
    e = _eng(P)
    for sp, r in zip(ASK, reqs):
        got = e.generate_requests([PROMPT], [sp])[0]
        assert got.output == r.output and got.logprobs == r.logprobs
    assert e.workers[-1].draw.logprob_launches > 0 and all(w.draw.logprob_launches == 0 for w in e.workers[:-1])


OTHERS = [SamplingParams(temperature=0.7, top_k=5, seed=3, max_new_tokens=4),
          SamplingParams(greedy=True, max_new_tokens=9, logprobs=0),
          SamplingParams(temperature=1.2, top_k=100, seed=4, max_new_tokens=15, presence_penalty=-1.0)]


def test_engine_same_records_inside_a_changing_batch(runs):
    """Six requests join and leave a running engine at different steps; the
    three that ask get the records they get alone, bit for bit.

    Bit-equal records need bit-equal logits, and this backend's GEMMs round a
    row differently beside other rows (torch's CPU matmul: row 0 of a [1, K]
    and of a [4, K] product differ in the last bits).  So the engine here runs
    two groups of one row each: sequences join and leave the batch, KV slots
    are reused, logprob and plain compositions alternate in each group, and
    every GEMM keeps the row count it has for a request alone.  Groups of
    several rows are compared in the next test, to GEMM rounding."""
    _, reqs = runs
    e = _eng(max_batch=2, num_microbatches=2)
    e.start_loop()
    try:
        first = [e.submit([4], OTHERS[0]), e.submit(PROMPT, GREEDY)]
        st = e.scheduler.stats["steps"]
        while e.scheduler.stats["steps"] < st + 2 and not all(r.done for r in first):
            time.sleep(0.001)
        late = [e.submit([9, 8, 7, 6], OTHERS[1]), e.submit(PROMPT, SEEDED), e.submit([5, 5], OTHERS[2]),
                e.submit(PROMPT, PENAL)]
        for r in first + late:
            r.wait(60)
    finally:
        e.stop_loop()
    assert e.scheduler.stats["joins"] == 6 and e.scheduler.stats["leaves"] == 6 and e.scheduler.stats["max_rows"] == 1
    for got, want in ((first[1], reqs[0]), (late[1], reqs[1]), (late[3], reqs[2])):
        assert got.output == want.output and got.logprobs == want.logprobs
    assert first[0].logprobs is None and late[2].logprobs is None
    # logprobs = 0: the drawn token's logprob, and empty alternative lists
    z = late[0].logprobs
    assert z.tokens == late[0].output and len(z.token_logprobs) == 9 and z.top_logprobs == [[]] * 9
    # the neighbours draw what they draw without the logprob requests
    assert _eng().generate_ids([[4], [5, 5]], [OTHERS[0], OTHERS[2]]) == [first[0].output, late[2].output]


def test_engine_records_in_groups_of_several_rows(runs):
    """Rows with and without records side by side in one group, leaving at
    different steps (pad rows, the per-row count column): the same tokens as
    alone, the same alternatives, and values within 1e-4 of the records alone --
    the logits themselves move by GEMM rounding with the row count (fp32 dot
    products of 128 to 512 terms at |logit| < 16: some 1e-5), nothing else
    does.  An alternative is compared by id where its neighbours are further
    than that away."""
    e, reqs = runs
    prompts = [[4], PROMPT, [9, 8, 7, 6], PROMPT, [5, 5], PROMPT]
    sps = [OTHERS[0], GREEDY, OTHERS[1], SEEDED, OTHERS[2], PENAL]
    got = e.generate_requests(prompts, sps)  # max_batch 4: two wait for a row
    assert e.scheduler.stats["max_rows"] == 4
    assert [r.logprobs is None for r in got] == [True, False, False, False, True, False]
    tol = 1e-4
    for r, want, sp in ((got[1], reqs[0], GREEDY), (got[3], reqs[1], SEEDED), (got[5], reqs[2], PENAL)):
        assert r.output == want.output
        _check_record(r, sp.logprobs)
        a, b = r.logprobs, want.logprobs
        assert max(abs(x - y) for x, y in zip(a.token_logprobs, b.token_logprobs)) < tol
        for xa, xb in zip(a.top_logprobs, b.top_logprobs):
            assert max(abs(v - w) for (_, v), (_, w) in zip(xa, xb)) < tol
            for k, ((i, v), (j, _)) in enumerate(zip(xa, xb)):
                near = [abs(v - xa[m][1]) for m in (k - 1, k + 1) if 0 <= m < len(xa)]
                if k + 1 < len(xa) and min(near, default=1.0) > 2 * tol:
                    assert i == j
    assert got[2].logprobs.top_logprobs == [[]] * 9


def test_engine_record_length_with_stop_at_eos(runs):
    e, reqs = runs
    eos = reqs[0].output[3]  # the greedy request's 4th token, made the EOS
    e2 = _eng()
    e2.mcfg = dataclasses.replace(e2.mcfg, eos_token_id=eos)
    sp = SamplingParams(greedy=True, max_new_tokens=N, logprobs=3, stop_at_eos=True)
    r = e2.generate_requests([PROMPT], [sp])[0]
    k = reqs[0].output.index(eos) + 1
    assert r.output == reqs[0].output[:k] and k < N
    assert r.logprobs.token_logprobs == reqs[0].logprobs.token_logprobs[:k]
    assert r.logprobs.top_logprobs == reqs[0].logprobs.top_logprobs[:k]


def test_engine_default_traffic_launches_nothing():
    e = _eng()
    e.generate_ids([PROMPT, [4, 5]], [_off(GREEDY), _off(SEEDED)])
    assert all(w.draw.logprob_launches == 0 and w.draw.lp_rec is None for w in e.workers)
    with pytest.raises(ValueError):
        e.generate_ids([PROMPT], [SamplingParams(logprobs=6)])  # above max_logprobs = 5
    e20 = _eng(max_logprobs=20)
    r = e20.generate_requests([PROMPT], [SamplingParams(greedy=True, max_new_tokens=2, logprobs=20)])[0]
    assert [len(a) for a in r.logprobs.top_logprobs] == [20, 20]


def test_rank_process_engines_refuse(monkeypatch):
    e = _eng()
    monkeypatch.setattr(e, "mode", "dist")  # rank 0 of a rank-process engine: the coordinator
    for call in (lambda: e.submit(PROMPT, GREEDY), lambda: e.generate_ids([PROMPT], [GREEDY])):
        with pytest.raises(ValueError, match="logprobs need the last stage in the coordinator process"):
            call()


# ---------------------------------------------------------------------------
# HTTP and client

@pytest.fixture(scope="module")
def client():
    from fastapi.testclient import TestClient

    from llm_sharding_demo_amd.serving.server import create_app

    cfg = EngineConfig(model_id="gpt2-test", max_batch=4, device="cpu", role="coordinator")
    return TestClient(create_app(cfg, engine=Engine(cfg)))


def test_http_generate(client):
    base = {"prompt": "Hi, ", "max_new_tokens": 3, "greedy": True}
    plain = client.post("/generate", json=base)
    assert plain.status_code == 200 and set(plain.json()) == {"generated"}
    r = client.post("/generate", json=dict(base, logprobs=2))
    assert r.status_code == 200
    body = r.json()
    assert set(body) == {"generated", "logprobs"} and body["generated"] == plain.json()["generated"]
    lp = body["logprobs"]
    assert set(lp) == {"tokens", "token_logprobs", "top_logprobs"}
    assert len(lp["tokens"]) == len(lp["token_logprobs"]) == len(lp["top_logprobs"]) == 3
    for tok, tl, alts in zip(lp["tokens"], lp["token_logprobs"], lp["top_logprobs"]):
        assert len(alts) == 2 and set(alts[0]) == {"id", "logprob"}
        assert alts[0] == {"id": tok, "logprob": tl}  # greedy
    assert client.post("/generate", json=dict(base, logprobs=0)).json()["logprobs"]["top_logprobs"] == [[], [], []]
    for bad in (6, -1):
        assert client.post("/generate", json=dict(base, logprobs=bad)).status_code == 422
    props = client.get("/openapi.json").json()["components"]["schemas"]["GenerateReq"]["properties"]
    assert "logprobs" in props


def test_http_non_finite_values_go_out_as_null():
    from llm_sharding_demo_amd.runtime.scheduler import Logprobs
    from llm_sharding_demo_amd.serving.server import logprobs_json

    out = logprobs_json(Logprobs([4], [-math.inf], [[(4, -0.5), (9, -math.inf)]]))
    assert out == {"tokens": [4], "token_logprobs": [None],
                   "top_logprobs": [[{"id": 4, "logprob": -0.5}, {"id": 9, "logprob": None}]]}


def test_client_forwards_the_field(monkeypatch):
    import requests

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
    cl.generate_text("Hi, ", logprobs=3)
    assert sent["logprobs"] == 3
    sent.clear()
    cl.generate_text("Hi, ")
    assert "logprobs" not in sent


def test_relay_computes_the_records_on_the_host(monkeypatch):
    """The reference-style relay over shard A / shard B (`http_generate`): the
    records come from ops/reference.py logprobs on the logits it already holds;
    the engine's records of the same greedy request agree to GEMM rounding
    (the relay recomputes the whole sequence every step: other GEMM shapes)."""
    from fastapi.testclient import TestClient

    from llm_sharding_demo_amd.serving import server as srv

    base = EngineConfig(model_id="gpt2-test", max_batch=4, device="cpu", split_points=[2],
                        shard_a_service="shard-a", shard_b_service="shard-b", shard_port=5001)
    a = TestClient(srv.create_app(base.replace(role="a"), shard=srv.ShardRunner(base, "a")))
    b = TestClient(srv.create_app(base.replace(role="b"), shard=srv.ShardRunner(base, "b")))

    class _Resp:
        def __init__(self, r):
            self.r = r

        def raise_for_status(self):
            assert self.r.status_code == 200, self.r.text

        def json(self):
            return self.r.json()

    def post(url, json=None, timeout=None):
        host, path = url.split("://", 1)[1].split("/", 1)
        return _Resp({"shard-a:5001": a, "shard-b:5001": b}[host].post("/" + path, json=json))

    import requests

    monkeypatch.setattr(requests, "post", post)
    prompt = [5, 6, 7, 8]
    sp = SamplingParams(greedy=True, max_new_tokens=4, logprobs=2)
    assert srv.http_generate(base, prompt, _off(sp)) == srv.http_generate(base, prompt, sp)  # a list, as before
    out, lp = srv.http_generate(base, prompt, sp, records=True)
    assert srv.http_generate(base, prompt, _off(sp), records=True) == (out, None)
    want = Engine(base.replace(num_stages=2, role="coordinator")).generate_requests([prompt], [sp])[0]
    assert out == want.output and lp.tokens == out
    assert [[i for i, _ in alts] for alts in lp.top_logprobs] == [[i for i, _ in alts] for alts in
                                                                  want.logprobs.top_logprobs]
    assert max(abs(x - y) for x, y in zip(lp.token_logprobs, want.logprobs.token_logprobs)) < 1e-4
    for tok, tl, alts in zip(lp.tokens, lp.token_logprobs, lp.top_logprobs):
        assert alts[0] == (tok, tl)


def test_llm_helper_and_cli(capsys):
    from llm_sharding_demo_amd import LLM
    from llm_sharding_demo_amd.__main__ import main

    llm = LLM(EngineConfig(model_id="gpt2-test", max_batch=4, device="cpu"))
    plain = llm.generate_text("Hi, ", max_new_tokens=5, greedy=True)
    got = llm.generate_text("Hi, ", max_new_tokens=5, greedy=True, logprobs=2)
    assert set(plain) == {"generated"} and got["generated"] == plain["generated"]
    assert len(got["logprobs"]["tokens"]) == 5 and all(len(a) == 2 for a in got["logprobs"]["top_logprobs"])
    with pytest.raises(ValueError):
        llm.generate_text("Hi, ", max_new_tokens=5, logprobs=6)
    assert main(["generate", "Hi, ", "--model-id", "gpt2-test", "--device", "cpu", "--max-batch", "4",
                 "--max-new-tokens", "5", "--greedy", "--logprobs", "2"]) == 0
    assert str(got["logprobs"]["tokens"]) in capsys.readouterr().out
