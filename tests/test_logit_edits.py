"""Per-request logit edits -- logit_bias, banned_token_ids, min_new_tokens --
on the CPU: validation, the host reference (ops/reference.py logit_edits) on
hand-computed rows, the plan wire, and the engine on the reference backend
with one stage and with two thread stages.

The engine tests run llama-test: its EOS token (2) lies inside its 1000-token
vocabulary, so the min_new_tokens entry is live.
"""
import math
import pickle

import numpy as np
import pytest
import torch

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.runtime.engine import Engine
from llm_sharding_demo_amd.runtime.plan import (MAGIC_PICKLE, Chunk, GroupPlan, PlanDecoder, PlanEncoder, Row, StepPlan,
                                                _pack_group, _unpack_group, has_edits, row_features)

INF = float("inf")
I32MAX = 2 ** 31 - 1


# ---------------------------------------------------------------------------
# validation

def test_defaults_validate_and_are_off():
    sp = SamplingParams()
    sp.validate()
    assert (sp.logit_bias, sp.banned_token_ids, sp.min_new_tokens) == (None, None, 0)
    assert not sp.has_logit_edits and sp.logit_edits(2) is None
    assert EngineConfig().max_logit_edits == 300
    SamplingParams(logit_bias={}, banned_token_ids=[]).validate()
    assert SamplingParams(logit_bias={}, banned_token_ids=[]).logit_edits(2) is None
    SamplingParams(logit_bias={5: 100, "7": -100.0}, banned_token_ids=(1, 1, 2), min_new_tokens=20).validate()


@pytest.mark.parametrize("kw", [
    dict(logit_bias={1.5: 1.0}), dict(logit_bias={"x": 1.0}), dict(logit_bias={True: 1.0}),
    dict(logit_bias={None: 1.0}),
    dict(logit_bias=[1, 2]), dict(banned_token_ids=[1.0]), dict(banned_token_ids=["a"]), dict(banned_token_ids="12"),
    dict(banned_token_ids=5),
    dict(logit_bias={1: float("nan")}), dict(logit_bias={1: INF}), dict(logit_bias={1: -INF}),
    dict(logit_bias={1: 100.1}), dict(logit_bias={1: -100.1}), dict(logit_bias={1: "3"}),
    dict(logit_bias={-1: 1.0}), dict(banned_token_ids=[-1]), dict(logit_bias={1: 1.0, "1": 2.0}),
    dict(min_new_tokens=-1), dict(min_new_tokens=21), dict(min_new_tokens=1.0), dict(min_new_tokens=True),
    dict(min_new_tokens=1, max_new_tokens=0),
])
def test_validate_refuses(kw):
    with pytest.raises(ValueError):
        SamplingParams(**kw).validate()
    with pytest.raises(ValueError):
        SamplingParams(greedy=True, **kw).validate()  # greedy requests are edited too


def test_validate_counts_entries_after_merging():
    bias = {t: 1.0 for t in range(200)}
    SamplingParams(logit_bias=bias, banned_token_ids=list(range(100, 300))).validate()          # 300 distinct
    SamplingParams(logit_bias=bias, banned_token_ids=list(range(100, 300)) * 2).validate()      # duplicates collapse
    with pytest.raises(ValueError):
        SamplingParams(logit_bias=bias, banned_token_ids=list(range(100, 301))).validate()      # 301
    with pytest.raises(ValueError):  # 300 + the min_new_tokens entry, even when EOS is among them
        SamplingParams(logit_bias=bias, banned_token_ids=list(range(100, 300)), min_new_tokens=1).validate()
    SamplingParams(logit_bias=bias, banned_token_ids=list(range(100, 299)), min_new_tokens=1).validate()
    # the limit is an argument, like max_logprobs
    SamplingParams(banned_token_ids=[1, 2, 3]).validate(5, 3)
    with pytest.raises(ValueError):
        SamplingParams(banned_token_ids=[1, 2, 3, 4]).validate(5, 3)
    with pytest.raises(ValueError):
        SamplingParams(banned_token_ids=[1, 2, 3], min_new_tokens=1).validate(5, 3)
    for bad in (0, 1025):
        with pytest.raises(ValueError):
            EngineConfig(max_logit_edits=bad)
    assert EngineConfig(max_logit_edits=1024).max_logit_edits == 1024


def test_entries_are_merged_and_sorted():
    sp = SamplingParams(logit_bias={"9": 0.1, 4: -3, 2: 100}, banned_token_ids=[7, 4, 7], min_new_tokens=3)
    tok, val, until = sp.logit_edits(2)
    assert tok == (2, 2, 4, 7, 9)
    assert val == (100.0, -INF, -INF, -INF, float(np.float32(0.1)))  # biased and banned: banned; values as fp32
    assert until == (I32MAX, 3, I32MAX, I32MAX, I32MAX)              # a token's permanent entry first
    assert SamplingParams(min_new_tokens=1).logit_edits(50256) == ((50256,), (-INF,), (1,))


def _eng(P=1, max_batch=4, model="llama-test", **kw):
    return Engine(EngineConfig(model_id=model, num_stages=P, max_batch=max_batch, device="cpu", **kw))


def test_engine_checks_ids_and_a_drawable_token():
    e = _eng()
    V = e.mcfg.vocab_size
    ok = SamplingParams(greedy=True, max_new_tokens=2, logit_bias={V - 1: 1.0}, banned_token_ids=[0])
    assert len(e.generate_ids([[1, 2]], [ok])[0]) == 2
    for kw in (dict(logit_bias={V: 1.0}), dict(banned_token_ids=[V]), dict(logit_bias={str(V + 5): 1.0})):
        with pytest.raises(ValueError):
            e.generate_ids([[1, 2]], [SamplingParams(max_new_tokens=2, **kw)])
        with pytest.raises(ValueError):
            e.submit([1, 2], SamplingParams(max_new_tokens=2, **kw))
    with pytest.raises(ValueError):  # more entries than this engine's table holds
        e.generate_ids([[1, 2]], [SamplingParams(max_new_tokens=2, banned_token_ids=list(range(301)))])
    # every token banned on a tiny vocabulary
    big = _eng(max_logit_edits=1024)
    eos = big.mcfg.eos_token_id
    with pytest.raises(ValueError):
        big.generate_ids([[1, 2]], [SamplingParams(max_new_tokens=2, banned_token_ids=list(range(V)))])
    with pytest.raises(ValueError):  # all but EOS, and EOS by min_new_tokens
        big.generate_ids([[1, 2]], [SamplingParams(max_new_tokens=2, min_new_tokens=1,
                                                   banned_token_ids=[t for t in range(V) if t != eos])])
    one = SamplingParams(max_new_tokens=3, banned_token_ids=[t for t in range(V) if t != 17])
    assert big.generate_ids([[1, 2]], [one])[0] == [17, 17, 17]  # one token left: drawn, seeded or not


# ---------------------------------------------------------------------------
# the host reference on hand-computed rows

def _table(rows, E=6, slots=4):
    """rows: {slot: [(tok, val, until), ...]}; everything else is filled with
    valid entries that would change the result if read."""
    cnt = torch.zeros(slots, dtype=torch.int32)
    tok = torch.full((slots, E), 3, dtype=torch.int32)
    val = torch.full((slots, E), 50.0)
    until = torch.full((slots, E), I32MAX, dtype=torch.int32)
    for s, ent in rows.items():
        cnt[s] = len(ent)
        for e, (t, v, u) in enumerate(ent):
            tok[s, e], val[s, e], until[s, e] = t, v, u
    return cnt, tok, val, until


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _segmax(logits):
    return logits.view(logits.shape[0], -1, 8).amax(-1).contiguous()


def test_reference_bias_and_ban_on_one_token():
    lg = torch.arange(16, dtype=torch.float32).repeat(2, 1)
    tab = _table({1: [(5, 2.5, I32MAX), (5, -INF, I32MAX), (9, -1.25, I32MAX)]})
    out = ref.logit_edits(lg.clone(), tab, torch.tensor([1, 0]), torch.tensor([4, 4]), 16)
    want = lg.clone()
    want[0, 5], want[0, 9] = -INF, 9 - 1.25
    assert torch.equal(_bits(out), _bits(want))  # row 1 (slot 0: count 0) bit for bit untouched
    # fp32, one rounding per addition, in table order: (1 + 2^-24) + 2^-24 stays 1; a fused sum would not
    lg = torch.ones(1, 8)
    tab = _table({0: [(2, 2.0 ** -24, I32MAX), (2, 2.0 ** -24, I32MAX), (3, 2.0 ** -23, I32MAX)]})
    out = ref.logit_edits(lg.clone(), tab, torch.tensor([0]), None, 8)
    assert out[0, 2] == 1.0 and out[0, 3] == 1.0 + 2.0 ** -23


def test_reference_until_boundary_and_step_none():
    m = 5
    tab = _table({2: [(4, 1.0, I32MAX), (4, -INF, m), (6, -2.0, m)]})
    lg = torch.zeros(4, 8)
    slots = torch.tensor([2, 2, 2, 2])
    out = ref.logit_edits(lg.clone(), tab, slots, torch.tensor([m - 1, m, m + 1, 0]), 8)
    assert out[:, 4].tolist() == [-INF, 1.0, 1.0, -INF]   # active while the counter is below `until`
    assert out[:, 6].tolist() == [-2.0, 0.0, 0.0, -2.0]
    out = ref.logit_edits(lg.clone(), tab, slots, None, 8)    # step None: draw 0
    assert out[:, 4].tolist() == [-INF] * 4 and out[:, 6].tolist() == [-2.0] * 4


def test_reference_untouched_rows_padding_and_segment_maxima():
    g = torch.Generator().manual_seed(3)
    V, Vp = 29, 32
    lg = torch.randn(5, Vp, generator=g)
    lg[0, 13] = 9.0  # the row's argmax, in a segment without padding columns
    am = int(lg[0, :V].argmax())
    lo = 8 + int(lg[1, 8:16].argmin())
    tab = _table({0: [(am, -INF, I32MAX)],                              # the argmax banned: its maximum falls
                  1: [(lo, 100.0, I32MAX)],                             # the smallest lifted above the maximum
                  2: [(16, -3.0, I32MAX), (19, 0.5, I32MAX), (V - 1, 1.0, I32MAX), (0, -1.0, 7),
                      (V, 9.0, I32MAX), (-1, 9.0, I32MAX)]})            # outside [0, V): ignored
    slots = torch.tensor([0, 1, 2, 3, 2])
    step = torch.tensor([0, 3, 7, 1, 6])
    sm0 = _segmax(lg)
    out, sm = ref.logit_edits(lg.clone(), tab, slots, step, V, sm0.clone())
    assert torch.equal(_bits(out[3]), _bits(lg[3])) and torch.equal(_bits(sm[3]), _bits(sm0[3]))  # count 0
    assert torch.equal(_bits(out[:, V:]), _bits(lg[:, V:]))      # padding columns
    assert torch.equal(_bits(sm), _bits(_segmax(out)))           # a full recompute, padding segment included
    assert out[0, am] == -INF and sm[0, am // 8] < sm0[0, am // 8]
    assert sm[1, 1] == out[1, lo] == lg[1, lo] + 100.0
    assert out[2, 0] == lg[2, 0] and out[4, 0] == lg[4, 0] - 1.0  # until 7: counter 7 off, 6 on
    assert out[2, V - 1] == lg[2, V - 1] + 1.0 and out[2, 16] == lg[2, 16] - 3.0
    changed = (_bits(out) != _bits(lg)).sum(1).tolist()
    assert changed == [1, 1, 3, 0, 4]
    # without segment maxima: the logits alone, the same bits
    assert torch.equal(_bits(ref.logit_edits(lg.clone(), tab, slots, step, V)), _bits(out))


# ---------------------------------------------------------------------------
# plan wire

ED3 = ((2, 2, 9), (100.0, -INF, float(np.float32(-0.1))), (I32MAX, 5, I32MAX))
ED1 = ((7,), (-INF,), (I32MAX,))


def _plan(chunks=True, rows=True, edits=True):
    ce = [dict(nedits=3, edits=ED3), dict(nedits=1), dict(), dict(nedits=1, edits=ED1)] if edits else [{}] * 4
    re_ = [dict(nedits=3), dict()] if edits else [{}] * 2
    gp = GroupPlan(0, ret=2, n=2, b=2, ctxb=256)
    if chunks:
        gp.chunks = [Chunk(1, 3, 0, [5, 6, 7], True, 0.7, 40, False, 11, **ce[0]),
                     Chunk(2, 4, 0, [8, 9], False, 0.6, 40, False, 12, **ce[1]),  # not final: the count alone
                     Chunk(5, 6, 0, [8], True, 0.6, 40, False, 12, **ce[2]),
                     Chunk(6, 7, 4, [1], True, 0.6, 40, True, 13, logprobs=2, **ce[3])]
    if rows:
        gp.rows = [Row(3, 5, 9, 0.9, 20, False, 13, 4, 0, presence=0.5, **re_[0]),
                   Row(4, 6, 2, 0.6, 40, True, 14, 1, 1, **re_[1])]
    return StepPlan(step=7, groups=[gp, GroupPlan(1, ret=1, n=1, b=1, ctxb=256)])


@pytest.mark.parametrize("ids", [True, False])
@pytest.mark.parametrize("chunks,rows", [(True, True), (True, False), (False, True)])
def test_plan_wire_round_trip(ids, chunks, rows):
    plan = _plan(chunks, rows)
    rec, payload = PlanEncoder(ids=ids).encode(plan)
    assert rec[0] == MAGIC_PICKLE
    out = PlanDecoder().decode(rec, lambda n: payload)
    g0 = out.groups[0]
    if chunks:
        assert [c.nedits for c in g0.chunks] == [3, 1, 0, 1]
        assert [c.edits for c in g0.chunks] == [ED3, None, None, ED1]
        assert [c.qlen for c in g0.chunks] == [3, 2, 1, 1] and g0.chunks[3].logprobs == 2
        if ids:
            assert g0.chunks[0].ids == [5, 6, 7]
    if rows:
        assert [r.nedits for r in g0.rows] == [3, 0] and g0.rows[0].presence == 0.5
    if ids:
        assert out == plan
    assert pickle.loads(pickle.dumps(plan)) == plan
    packed = _pack_group(plan.groups[0], ids)
    assert len(packed) == 10 and _unpack_group(*packed).rows == plan.groups[0].rows
    assert len(_pack_group(plan.groups[1], ids)) == 9  # a group of the same plan without edits


def test_plan_without_edits_packs_as_before():
    plan = _plan(edits=False)
    packed = _pack_group(plan.groups[0], True)
    assert len(packed) == 9
    assert _unpack_group(*packed) == plan.groups[0]
    rec, payload = PlanEncoder().encode(plan)
    _, with_edits = PlanEncoder().encode(_plan())
    assert len(payload) < len(with_edits)
    assert PlanDecoder().decode(rec, lambda n: payload) == plan
    # the gate is a flag of its own: row_features' triple does not know the field
    assert row_features(_plan().groups[0].rows) == row_features(plan.groups[0].rows) == (False, True, False)
    assert has_edits(_plan().groups[0].rows) and not has_edits(plan.groups[0].rows)
    assert has_edits(_plan().groups[0].chunks) and not has_edits(plan.groups[0].chunks)


# ---------------------------------------------------------------------------
# engine (llama-test on the CPU, reference backend)

PROMPT = [1, 2, 3]
N = 10
PLAIN = SamplingParams(greedy=True, max_new_tokens=N)
OTHERS = [SamplingParams(temperature=0.7, top_k=5, seed=3, max_new_tokens=4),
          SamplingParams(greedy=True, max_new_tokens=7),
          SamplingParams(temperature=1.2, top_k=100, seed=4, max_new_tokens=N + 3)]
OTHER_PROMPTS = [[4], [9, 8, 7, 6], [5, 5]]


@pytest.fixture(scope="module", params=[1, 2], ids=["one-stage", "two-thread-stages"])
def runs(request):
    e = _eng(request.param)
    return e, e.generate_ids([PROMPT], [PLAIN])[0]


def test_engine_default_traffic_launches_nothing(runs):
    e, plain = runs
    fresh = _eng(e.P)
    assert fresh.generate_ids([PROMPT] + OTHER_PROMPTS, [PLAIN] + OTHERS)[0] == plain
    assert all(w.draw.logit_edit_launches == 0 and w.draw.edit_tab is None for w in fresh.workers)
    zero = SamplingParams(greedy=True, max_new_tokens=N, logit_bias={}, banned_token_ids=[], min_new_tokens=0)
    assert fresh.generate_ids([PROMPT], [zero])[0] == plain
    assert all(w.draw.logit_edit_launches == 0 and w.draw.edit_tab is None for w in fresh.workers)


def test_engine_ban_is_live_and_neighbours_unchanged(runs):
    e, plain = runs
    ban = SamplingParams(greedy=True, max_new_tokens=N, banned_token_ids=[plain[0], plain[0]])
    alone = e.generate_ids([PROMPT], [ban])[0]
    assert len(alone) == N and plain[0] not in alone and alone[0] != plain[0]
    assert e.workers[-1].draw.logit_edit_launches > 0 and all(w.draw.logit_edit_launches == 0 for w in e.workers[:-1])
    without = e.generate_ids(OTHER_PROMPTS, OTHERS)
    outs = e.generate_ids([OTHER_PROMPTS[0], PROMPT] + OTHER_PROMPTS[1:], [OTHERS[0], ban] + OTHERS[1:])
    assert outs[1] == alone
    assert [outs[0]] + outs[2:] == without  # asking for edits never changes another request's draws
    # a seeded request: the banned token never appears either
    s = SamplingParams(temperature=1.5, top_k=50, seed=9, max_new_tokens=N)
    drawn = e.generate_ids([PROMPT], [s])[0]
    sb = SamplingParams(temperature=1.5, top_k=50, seed=9, max_new_tokens=N, banned_token_ids=[drawn[3]])
    got = e.generate_ids([PROMPT], [sb])[0]
    assert got[:3] == drawn[:3] and drawn[3] not in got


def test_engine_bias_of_100_wins_every_draw(runs):
    e, plain = runs
    t = 777
    assert t not in plain
    for sp in (SamplingParams(greedy=True, max_new_tokens=N, logit_bias={t: 100}),
               SamplingParams(greedy=True, max_new_tokens=N, logit_bias={str(t): 100.0}, presence_penalty=2.0,
                              frequency_penalty=2.0)):  # 100 - (2 + 2 c) for c <= 9 still wins
        assert e.generate_ids([PROMPT], [sp])[0] == [t] * N


def test_engine_min_new_tokens_holds_eos_back(runs):
    e, plain = runs
    eos = e.mcfg.eos_token_id
    assert 0 <= eos < e.mcfg.vocab_size
    sp = SamplingParams(greedy=True, max_new_tokens=N, logit_bias={eos: 100}, stop_at_eos=True, min_new_tokens=5)
    out = e.generate_ids([PROMPT], [sp])[0]
    assert len(out) == 6 and eos not in out[:5] and out[5] == eos  # draws 0-4 not EOS, draw 5 is
    assert out[:5] == plain[:5]                                    # nothing else was edited
    # the same rule without stop_at_eos: EOS from draw 5 on
    sp = SamplingParams(greedy=True, max_new_tokens=N, logit_bias={eos: 100}, min_new_tokens=5)
    assert e.generate_ids([PROMPT], [sp])[0] == plain[:5] + [eos] * (N - 5)
    sp = SamplingParams(greedy=True, max_new_tokens=N, logit_bias={eos: 100}, stop_at_eos=True)
    assert e.generate_ids([PROMPT], [sp])[0] == [eos]
    sp = SamplingParams(greedy=True, max_new_tokens=N, logit_bias={eos: 100}, stop_at_eos=True, min_new_tokens=N)
    assert eos not in e.generate_ids([PROMPT], [sp])[0]


def test_engine_logprobs_come_after_the_edits(runs):
    e, plain = runs
    big = _eng(e.P, max_logit_edits=1024)
    V = big.mcfg.vocab_size
    keep = sorted({plain[0], 500, 900})
    sp = SamplingParams(greedy=True, max_new_tokens=3, logprobs=5,
                        banned_token_ids=[t for t in range(V) if t not in keep])
    r = big.generate_requests([PROMPT], [sp])[0]
    assert r.output[0] == plain[0] and set(r.output) <= set(keep)
    for tl, alts in zip(r.logprobs.token_logprobs, r.logprobs.top_logprobs):
        assert sorted(i for i, _ in alts[:3]) == keep and all(math.isfinite(v) for _, v in alts[:3])
        assert [(i, v) for i, v in alts[3:]] == [(0, -INF), (1, -INF)]  # banned tokens: logprob -inf
        assert abs(sum(math.exp(v) for _, v in alts[:3]) - 1.0) < 1e-5  # the softmax of what was drawn from
        assert tl == alts[0][1]


@pytest.mark.parametrize("P", [1, 2])
def test_engine_slot_reuse_does_not_inherit_edits(P):
    """Two KV slots: a long neighbour with edits keeps the group's edit gate on;
    a short request with bans finishes; the plain request that takes over its
    slot draws what it draws on a fresh engine, although the ban named its
    first token."""
    plain = _eng(P, max_batch=2).generate_ids([PROMPT], [PLAIN])[0]
    e = _eng(P, max_batch=2, num_microbatches=1)  # one group: the neighbour shares it
    e.start_loop()
    try:
        nb = e.submit([9, 8, 7], SamplingParams(greedy=True, max_new_tokens=150, banned_token_ids=[11],
                                                min_new_tokens=3))
        a = e.submit(PROMPT, SamplingParams(greedy=True, max_new_tokens=3, banned_token_ids=plain[:2],
                                            logit_bias={5: -1.0}))
        got_a = a.wait(60)
        assert plain[0] not in got_a and plain[1] not in got_a
        c = e.submit(PROMPT, PLAIN)
        assert not nb.done  # precondition: the neighbour is still decoding
        got_c = c.wait(60)
        still = not nb.done
        nb.wait(120)
    finally:
        e.stop_loop()
    assert got_c == plain
    assert still  # the plain request ran beside the neighbour, behind the edit pass
