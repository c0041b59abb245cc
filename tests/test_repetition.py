"""Per-request repetition_penalty and no_repeat_ngram_size on the CPU:
validation, the host reference (ops/reference.py repetition, record_context)
against a brute-force implementation on Python lists (tests/repetition_cases.py),
the plan wire, the engine on the reference backend -- its tokens re-simulated
on the host from the logits the repetition pass was handed -- and DrawStage's
call order, allocation and counter.
"""
import contextlib
import itertools
import json
import os
import pickle
import socket
import subprocess
import sys
import textwrap
import types

import numpy as np
import pytest
import torch

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.parallel.draw import DrawStage
from llm_sharding_demo_amd.parallel.pipeline import GroupState
from llm_sharding_demo_amd.runtime.batch import counter_uniform
from llm_sharding_demo_amd.runtime.engine import Engine
from llm_sharding_demo_amd.runtime.plan import (MAGIC_PICKLE, Chunk, GroupPlan, PlanDecoder, PlanEncoder, Row, StepPlan,
                                                _pack_group, _unpack_group, has_context, has_edits, row_features)

from . import repetition_cases as rc

INF = float("inf")


# ---------------------------------------------------------------------------
# validation

def test_defaults_validate_and_are_off():
    sp = SamplingParams()
    sp.validate()
    assert (sp.repetition_penalty, sp.no_repeat_ngram_size) == (1.0, 0) and not sp.has_context
    assert SamplingParams(repetition_penalty=1).context_knobs() == (1.0, 0)
    for kw in (dict(repetition_penalty=10), dict(repetition_penalty=1e-3), dict(no_repeat_ngram_size=32),
               dict(repetition_penalty=1.3, no_repeat_ngram_size=1)):
        SamplingParams(**kw).validate()
        SamplingParams(greedy=True, **kw).validate()
        assert SamplingParams(**kw).has_context
    # the kernel multiplies by the fp32: a value that rounds to 1 is off
    assert not SamplingParams(repetition_penalty=1.0 + 1e-12).has_context
    assert SamplingParams(repetition_penalty=1.3).context_knobs() == (float(np.float32(1.3)), 0)


@pytest.mark.parametrize("kw", [
    dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=10.001),
    dict(repetition_penalty=INF), dict(repetition_penalty=float("nan")), dict(repetition_penalty="1.2"),
    dict(repetition_penalty=True), dict(repetition_penalty=None), dict(repetition_penalty=1e-60),
    dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=33), dict(no_repeat_ngram_size=2.0),
    dict(no_repeat_ngram_size=True), dict(no_repeat_ngram_size=False), dict(no_repeat_ngram_size=None),
])
def test_validate_refuses(kw):
    with pytest.raises(ValueError):
        SamplingParams(**kw).validate()
    with pytest.raises(ValueError):
        SamplingParams(greedy=True, **kw).validate()  # greedy requests get the rules too


def _eng(P=1, max_batch=4, model="gpt2-test", **kw):
    return Engine(EngineConfig(model_id=model, num_stages=P, max_batch=max_batch, device="cpu", **kw))


def test_engine_keeps_a_token_drawable():
    e = _eng(model="llama-test", max_seq_len=2048, max_logit_edits=1024)
    V = e.mcfg.vocab_size
    assert V == 1000
    prompt = list(range(1, 101))
    ok = SamplingParams(greedy=True, max_new_tokens=V - 101, no_repeat_ngram_size=1)  # 100 + 899 < 1000
    e._validate(prompt, ok)
    for bad in (SamplingParams(max_new_tokens=V - 100, no_repeat_ngram_size=1),
                SamplingParams(max_new_tokens=V - 100, no_repeat_ngram_size=32),
                SamplingParams(max_new_tokens=V - 103, no_repeat_ngram_size=2, banned_token_ids=[5, 6, 6, 7]),
                SamplingParams(max_new_tokens=V - 103, no_repeat_ngram_size=2, banned_token_ids=[5, 6],
                               min_new_tokens=1)):
        with pytest.raises(ValueError, match="no_repeat_ngram_size"):
            e._validate(prompt, bad)
        with pytest.raises(ValueError):
            e.submit(prompt, bad)
    # a logit_bias is no ban; and without the n-gram rule nothing is counted
    e._validate(prompt, SamplingParams(max_new_tokens=V - 103, no_repeat_ngram_size=2, banned_token_ids=[5, 6],
                                       logit_bias={9: -100}))
    e._validate(prompt, SamplingParams(max_new_tokens=V, repetition_penalty=2.0))
    with pytest.raises(ValueError):
        e.generate_ids([[1, 2]], [SamplingParams(max_new_tokens=2, repetition_penalty=0)])


# ---------------------------------------------------------------------------
# the host reference against brute force

@pytest.mark.parametrize("V,Vp,seg,with_step", [(1000, 1024, True, True), (1000, 1024, False, True),
                                                (1000, 1024, True, False), (50257, 50304, True, True),
                                                (128256, 128256, True, True)])
def test_reference_equals_brute_force(V, Vp, seg, with_step):
    c = rc.case(V, Vp)
    lg0, step = c["lg"], (c["step"] if with_step else None)
    sm0 = rc.segmax_of(lg0) if seg else None
    want, wsm = rc.brute(lg0, c["tab"], c["slots"], step, V, sm0)
    tab = tuple(t.clone() for t in c["tab"])
    got = lg0.clone()
    gsm = sm0.clone() if seg else None
    out = ref.repetition(got, tab, c["slots"], step, V, gsm)
    assert (out[0] is got and out[1] is gsm) if seg else out is got  # in place
    assert all(torch.equal(a, b) for a, b in zip(tab, c["tab"]))     # the table is read only
    assert torch.equal(rc.bits(got), rc.bits(want))
    if seg:
        assert torch.equal(rc.bits(gsm), rc.bits(wsm))
        assert torch.equal(rc.bits(gsm), rc.bits(rc.segmax_of(got)))  # every segment, padding included
    assert torch.equal(rc.bits(got[:, V:]), rc.bits(lg0[:, V:]))      # padding columns
    if not with_step:
        return
    # the case does what it says
    for r in (0, 1, 10):  # knobs off; the pad row; n = G - 2
        assert torch.equal(rc.bits(got[r]), rc.bits(lg0[r]))
    assert all(not torch.equal(rc.bits(got[r]), rc.bits(lg0[r])) for r in (2, 3, 4, 5, 6, 7, 8, 9))
    changed = (rc.bits(got) != rc.bits(lg0)).sum(1).tolist()
    assert changed[2] == 1 and 60 < changed[3] <= 120 and changed[5] == 2
    assert changed[4] == len(set(c["tab"][3][12].tolist()))  # n = L: every distinct token of the slot's row
    t5 = c["tok5"]
    assert got[5, t5] == lg0[5, t5] * np.float32(0.01) and got[5, t5] > lg0[5, c["seg5"] * 8: c["seg5"] * 8 + 8].max()
    inside = {t for t in c["ctx"][6] if 0 <= t < V}
    assert (got[6] == -INF).nonzero().flatten().tolist() == sorted(inside) and changed[6] == len(inside)
    am7 = int(c["am"][7])
    assert got[7, am7] == -INF and int(got[7, :V].argmax()) != am7
    assert got[8, 33] == -INF and 33 in c["ctx"][8] and changed[8] >= len(set(c["ctx"][8]))
    assert (got[9] == -INF).nonzero().flatten().tolist() == [V - 1] and changed[9] == 1
    # n = G - 1: no ban; the penalty alone: 0.0 / r, -0.0 / r, -inf * r keep their bits, nothing else moves
    assert changed[11] == 0
    assert rc.bits(got[11, 16:19]).tolist() == rc.bits(torch.tensor([0.0, -0.0, -INF])).tolist()
    if seg:
        assert gsm[5, c["seg5"]] == got[5, t5] > sm0[5, c["seg5"]]  # lifted to the new maximum
        assert gsm[7, am7 // 8] < sm0[7, am7 // 8]                  # the argmax's segment fell


def test_reference_formula_is_hf():
    q = float(np.float32(2.0) / np.float32(1.5))
    lg = torch.tensor([[2.0, -2.0, 3.0, -0.0, 0.0, 5.0, -INF, 1.0]])
    tab = (torch.tensor([4]), torch.tensor([1.5]), torch.tensor([2]), torch.tensor([[0, 1, 0, 3, 4, 6, 5, 7]]))
    out = ref.repetition(lg.clone(), tab, torch.tensor([0]), torch.tensor([3]), 8)  # x = [0, 1, 0, 3, 4, 6, 5]
    assert out[0].tolist()[:3] == [q, -3.0, 3.0] and rc.bits(out[0, 3:5]).tolist() == rc.bits(lg[0, 3:5]).tolist()
    assert out[0, 5] == np.float32(5.0) / np.float32(1.5) and out[0, 6] == -INF and out[0, 7] == 1.0
    tab = (torch.tensor([4]), torch.tensor([1.5]), torch.tensor([2]), torch.tensor([[0, 1, 0, 3, 4, 6, 0, 7]]))
    out = ref.repetition(lg.clone(), tab, torch.tensor([0]), torch.tensor([3]), 8)  # ends on 0: 1 and 3 followed it
    assert out[0, 1] == -INF and out[0, 3] == -INF and out[0, 0] == q and out[0, 7] == 1.0
    # step None: draw 0, the prompt alone -- x = [0, 1, 0, 3]: nothing follows a 3
    out = ref.repetition(lg.clone(), tab, torch.tensor([0]), None, 8)
    assert (out[0] == -INF).nonzero().flatten().tolist() == [6] and out[0, 4] == 0.0 and out[0, 0] == q


def test_reference_largest_context():
    c = rc.big_case(V=1000, Vp=1024)
    sm0 = rc.segmax_of(c["lg"])
    want, wsm = rc.brute(c["lg"], c["tab"], c["slots"], c["step"], c["V"], sm0)
    got, gsm = ref.repetition(c["lg"].clone(), c["tab"], c["slots"], c["step"], c["V"], sm0.clone())
    assert torch.equal(rc.bits(got), rc.bits(want)) and torch.equal(rc.bits(gsm), rc.bits(wsm))
    assert torch.equal(rc.bits(got[1]), rc.bits(c["lg"][1])) and got[0, int(c["lg"][0, :1000].argmax())] == -INF


def _record_case():
    L, S = 8, 5
    plen = torch.tensor([0, 3, 7, 8, 2], dtype=torch.int32)
    tab = (plen, torch.ones(S), torch.zeros(S, dtype=torch.int32), torch.full((S, L), -7, dtype=torch.int32))
    slots = torch.tensor([0, 1, 2, 3, 4, 1, 9, -1], dtype=torch.int32)   # 9 and -1: no such slot
    step = torch.tensor([0, 2, 1, 1, 6, 4, 1, 1], dtype=torch.int64)
    tokens = torch.arange(100, 108, dtype=torch.int32)
    active = torch.tensor([1, 1, 1, 1, 1, 0, 1, 1], dtype=torch.int32)
    return tab, slots, step, tokens, active


def _record_brute(tab, slots, step, tokens, active, back):
    plen, tok = tab[0].tolist(), [row[:] for row in tab[3].tolist()]
    for i, s in enumerate(slots.tolist()):
        if active is not None and not active[i]:
            continue
        j = (plen[s] if 0 <= s < len(plen) else 0) + (int(step[i]) - back if step is not None else 0)
        if 0 <= s < len(plen) and 0 <= j < len(tok[0]):
            tok[s][j] = int(tokens[i])
    return tok


@pytest.mark.parametrize("back", [0, 1])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("with_step", [True, False])
def test_record_context_equals_brute_force(back, masked, with_step):
    tab, slots, step, tokens, active = _record_case()
    active, step = (active if masked else None), (step if with_step else None)
    want = _record_brute(tab, slots, step, tokens, active, back)
    ref.record_context(tab, slots, step, tokens, active, back)
    assert tab[3].tolist() == want
    assert tab[0].tolist() == [0, 3, 7, 8, 2]
    if with_step and back == 1 and masked:
        # slot 0: position -1 dropped; slot 1: 3 + 2 - 1; slot 2: 7 + 1 - 1; slot 3: 8 + 1 - 1 >= L dropped;
        # slot 4: 2 + 6 - 1; the inactive row and the rows without a slot dropped
        assert [[j for j, t in enumerate(row) if t != -7] for row in want] == [[], [4], [7], [], [7]]


# ---------------------------------------------------------------------------
# plan wire

def _plan(chunks=True, rows=True, ctx=True, edits=False):
    cc = [dict(rpen=float(np.float32(1.3)), ngram=0, plen=3), dict(), dict(rpen=1.0, ngram=3, plen=9), dict()]
    rr = [dict(ctx=1), dict()]
    if not ctx:
        cc, rr = [{}] * 4, [{}] * 2
    if edits:
        cc[3] = dict(cc[3], nedits=1, edits=((7,), (-INF,), (2 ** 31 - 1,)))
        rr[1] = dict(rr[1], nedits=1)
    gp = GroupPlan(0, ret=2, n=2, b=2, ctxb=256)
    if chunks:
        gp.chunks = [Chunk(1, 3, 0, [5, 6, 7], True, 0.7, 40, False, 11, **cc[0]),
                     Chunk(2, 4, 0, [8, 9], False, 0.6, 40, False, 12, **cc[1]),
                     Chunk(5, 6, 4, [8, 1, 1, 2, 3], True, 0.6, 40, False, 12, **cc[2]),
                     Chunk(6, 7, 4, [1], True, 0.6, 40, True, 13, logprobs=2, **cc[3])]
    if rows:
        gp.rows = [Row(3, 5, 9, 0.9, 20, False, 13, 4, 0, presence=0.5, **rr[0]),
                   Row(4, 6, 2, 0.6, 40, True, 14, 1, 1, **rr[1])]
    plain = GroupPlan(1, ret=1, n=1, b=1, ctxb=256, chunks=[Chunk(9, 1, 0, [4, 4], True, 0.6, 40, False, 3)])
    return StepPlan(step=7, groups=[gp, plain])


@pytest.mark.parametrize("edits", [False, True])
@pytest.mark.parametrize("chunks,rows", [(True, True), (True, False), (False, True)])
def test_plan_wire_round_trip(chunks, rows, edits):
    plan = _plan(chunks, rows, edits=edits)
    g = plan.groups[0]
    assert has_context(g.chunks) == chunks and has_context(g.rows or []) == rows
    assert not has_context(plan.groups[1].chunks)
    for enc in (PlanEncoder(ids=True), PlanEncoder(ids=False, ctx_ids=True), PlanEncoder(ids=False)):
        rec, payload = enc.encode(plan)
        assert rec[0] == MAGIC_PICKLE
        out = PlanDecoder().decode(rec, lambda n: payload)
        g0, g1 = out.groups
        if chunks:
            assert [(c.rpen, c.ngram, c.plen) for c in g0.chunks] == [(float(np.float32(1.3)), 0, 3), (1.0, 0, 0),
                                                                      (1.0, 3, 9), (1.0, 0, 0)]
            assert [c.ctx for c in g0.chunks] == [True, False, True, False]
            assert [c.qlen for c in g0.chunks] == [3, 2, 5, 1]
            # a last-stage destination gets the ids of the flagged group -- all of its chunks, as stage 0 does
            if enc.ids or enc.ctx_ids:
                assert [list(c.ids) for c in g0.chunks] == [[5, 6, 7], [8, 9], [8, 1, 1, 2, 3], [1]]
            else:
                assert all(isinstance(c.ids, range) for c in g0.chunks)
        if rows:
            assert [r.ctx for r in g0.rows] == [1, 0] and g0.rows[0].presence == 0.5
            assert [r.nedits for r in g0.rows] == [0, int(edits)]
        # the group without the feature: no ids off stage 0
        assert (list(g1.chunks[0].ids) == [4, 4]) if enc.ids else isinstance(g1.chunks[0].ids, range)
        if enc.ids:
            assert out == plan
    assert pickle.loads(pickle.dumps(plan)) == plan
    packed = _pack_group(g, False, True)
    assert len(packed) == 11 and (packed[9] is not None) == edits
    assert (packed[7][3] is not None) == chunks if chunks else packed[7] is None
    back = _unpack_group(*packed)
    assert back.rows == g.rows and list(map(_fields, back.chunks)) == list(map(_fields, g.chunks))
    assert len(_pack_group(plan.groups[1], True)) == 9


def _fields(c):
    """A chunk's fields, its ids as a list (they unpack as a slice of the packed column)."""
    return {**vars(c), "ids": list(c.ids)}


def test_plan_without_the_feature_packs_as_before():
    for edits in (False, True):
        plan = _plan(ctx=False, edits=edits)
        for ids, ctx_ids in ((True, False), (False, True), (False, False)):
            packed = _pack_group(plan.groups[0], ids, ctx_ids)
            assert len(packed) == (10 if edits else 9)
            assert (packed[7][3] is not None) == ids  # token ids to stage 0 alone
            if ids:
                assert _unpack_group(*packed) == plan.groups[0]
        a = PlanEncoder(ids=False).encode(plan)[1]
        b = PlanEncoder(ids=False, ctx_ids=True).encode(plan)[1]
        assert a == b  # byte for byte what a last stage was sent before
        assert len(PlanEncoder(ids=False, ctx_ids=True).encode(_plan(edits=edits))[1]) > len(a)
    plan, flagged = _plan(ctx=False), _plan()
    assert row_features(flagged.groups[0].rows) == row_features(plan.groups[0].rows) == (False, True, False)
    assert not has_edits(flagged.groups[0].rows) and not has_context(plan.groups[0].rows)
    assert Row(1, 1, 1, 0.6, 40, False, 1, 0, 0).ctx == 0 and not Chunk(1, 1, 0, [1], True).ctx
    assert GroupPlan(0).ctx is None


# ---------------------------------------------------------------------------
# engine (gpt2-test on the CPU, reference backend: its plain greedy output repeats)

PROMPT = [5, 6, 7, 5, 6, 7, 5, 6, 9, 9, 5, 6]
N = 16
PLAIN = SamplingParams(greedy=True, max_new_tokens=N)
SEEDED = dict(temperature=1.1, top_k=50, seed=21)


class _Tap:
    """The last stage's reference backend, recording the logits every flagged
    row was handed to the repetition pass: (slot, draw counter) -> raw logits."""

    def __init__(self, be, draw):
        object.__setattr__(self, "_be", be)
        object.__setattr__(self, "_draw", draw)
        object.__setattr__(self, "seen", {})

    def __getattr__(self, name):
        return getattr(self._be, name)

    def __setattr__(self, name, value):
        setattr(self._be, name, value)

    def repetition(self, logits, table, slots, step, vocab):
        assert table is self._draw.ctx_tab
        for i, s in enumerate(slots.tolist()):
            if float(table[1][s]) != 1.0 or int(table[2][s]) != 0:
                self.seen[(s, int(step[i]) if step is not None else 0)] = logits[i].clone()
        self._be.repetition(logits, table, slots, step, vocab)


def _tapped(P=1, **kw):
    e = _eng(P, **kw)
    tap = e.stages[-1].backend = _Tap(e.stages[-1].backend, e.workers[-1].draw)
    return e, tap


def _resimulate(seen, prompt, sp, V):
    """The request's tokens from the recorded raw logits: the brute-force
    rules over prompt + the tokens drawn so far, then the host sampler."""
    r, G = sp.context_knobs()
    slot = {s for s, _ in seen}
    assert len(slot) == 1  # one flagged request ran
    s, out = slot.pop(), []
    seed = torch.tensor([sp.seed if sp.seed is not None else 0])
    for c in range(sp.max_new_tokens):
        row, _ = rc.brute_row([np.float32(v) for v in seen[(s, c)].tolist()], list(prompt) + out, r, G, V)
        lg = torch.tensor(np.array([row], dtype=np.float32))
        u = counter_uniform(seed, torch.tensor([c]))
        out.append(int(ref.sample(lg, torch.tensor([sp.temperature]), torch.tensor([sp.top_k], dtype=torch.int32),
                                  torch.tensor([int(sp.greedy)], dtype=torch.int32), u, V,
                                  torch.tensor([sp.top_p]), torch.tensor([sp.min_p]))[0]))
    return out


def _no_repeated_gram(prompt, out, G):
    x = list(prompt) + list(out)
    for e in range(len(prompt), len(x)):       # every G-gram that ends on a generated token
        if e + 1 >= G and any(x[i: i + G] == x[e + 1 - G: e + 1] for i in range(0, e + 1 - G)):
            return False
    return True


KNOBS = [dict(repetition_penalty=1.8), dict(repetition_penalty=0.5), dict(no_repeat_ngram_size=1),
         dict(no_repeat_ngram_size=2), dict(no_repeat_ngram_size=3),
         dict(repetition_penalty=1.4, no_repeat_ngram_size=2)]


@pytest.fixture(scope="module")
def plain():
    return _eng().generate_ids([PROMPT], [PLAIN])[0]


@pytest.mark.parametrize("mode", ["greedy", "seeded"])
@pytest.mark.parametrize("kw", KNOBS, ids=lambda kw: "-".join(f"{k[:4]}{v}" for k, v in kw.items()))
def test_engine_tokens_are_the_host_resimulation(plain, kw, mode):
    base = dict(greedy=True) if mode == "greedy" else SEEDED
    sp = SamplingParams(max_new_tokens=N, **base, **kw)
    e, tap = _tapped()
    got = e.generate_ids([PROMPT], [sp])[0]
    V = e.mcfg.vocab_size
    assert len(got) == N and sorted({c for _, c in tap.seen}) == list(range(N))
    assert got == _resimulate(tap.seen, PROMPT, sp, V)
    assert e.workers[-1].draw.repetition_launches == N  # the prefill draw and N - 1 decode items
    G = sp.no_repeat_ngram_size
    if G:
        assert _no_repeated_gram(PROMPT, got, G)
    unflagged = e.generate_ids([PROMPT], [SamplingParams(max_new_tokens=N, **base)])[0]
    if mode == "greedy" or not G or not _no_repeated_gram(PROMPT, unflagged, G):
        assert got != unflagged  # the knob is live (a seeded draw may never complete a G-gram by itself)
    if mode == "greedy":
        assert unflagged == plain and not _no_repeated_gram(PROMPT, plain, 1)  # precondition: plain greedy repeats
    # 2 in-process stages, and a prompt prefilled in chunks of 5: the same tokens
    e2, tap2 = _tapped(2)
    assert e2.generate_ids([PROMPT], [sp])[0] == got
    assert [w.draw.repetition_launches for w in e2.workers] == [0, N] and e2.workers[0].draw.ctx_tab is None
    assert all(torch.equal(rc.bits(tap2.seen[k]), rc.bits(v)) for k, v in tap.seen.items())
    assert _eng(prefill_chunk=5).generate_ids([PROMPT], [sp])[0] == got
    assert _eng(2, prefill_chunk=5).generate_ids([PROMPT], [sp])[0] == got


def test_engine_default_traffic_launches_nothing(plain):
    for P in (1, 2):
        e = _eng(P)
        others = [SamplingParams(temperature=0.7, top_k=5, seed=3, max_new_tokens=4),
                  SamplingParams(greedy=True, max_new_tokens=7, presence_penalty=1.0)]
        assert e.generate_ids([PROMPT, [4], [9, 8, 7, 6]], [PLAIN] + others)[0] == plain
        off = SamplingParams(greedy=True, max_new_tokens=N, repetition_penalty=1.0, no_repeat_ngram_size=0)
        assert e.generate_ids([PROMPT], [off])[0] == plain
        assert all(w.draw.repetition_launches == 0 and w.draw.ctx_tab is None for w in e.workers)
        assert e.scheduler._contexts == 0
        e.generate_ids([PROMPT], [SamplingParams(greedy=True, max_new_tokens=3, no_repeat_ngram_size=2)])
        assert e.scheduler._contexts == 0 and e.workers[-1].draw.ctx_tab is not None  # released with the request
        n = e.workers[-1].draw.repetition_launches
        assert e.generate_ids([PROMPT], [PLAIN])[0] == plain   # the table exists now: still nothing runs
        assert e.workers[-1].draw.repetition_launches == n == 3


@pytest.mark.parametrize("P", [1, 2])
def test_engine_neighbours_draw_what_they_draw_alone(P):
    e = _eng(P, num_microbatches=1)  # one group: the default requests share it with the flagged one
    seeded = SamplingParams(max_new_tokens=N, **SEEDED)
    others = [SamplingParams(temperature=0.7, top_k=5, seed=3, max_new_tokens=4), seeded,
              SamplingParams(greedy=True, max_new_tokens=9)]
    prompts = [[4], PROMPT, [9, 8, 7, 6]]
    alone = e.generate_ids(prompts, others)
    assert e.workers[-1].draw.repetition_launches == 0
    flagged = SamplingParams(max_new_tokens=N, repetition_penalty=1.5, no_repeat_ngram_size=2, **SEEDED)
    f_alone = e.generate_ids([PROMPT], [flagged])[0]
    got = e.generate_ids(prompts[:1] + [PROMPT] + prompts[1:], others[:1] + [flagged] + others[1:])
    assert got[1] == f_alone and got[:1] + got[2:] == alone
    assert alone[1] != f_alone  # the same prompt and seed: the knobs alone make the difference


@pytest.mark.parametrize("P", [1, 2])
def test_engine_slot_reuse_does_not_inherit_the_knobs(P, plain):
    """Two KV slots: a long flagged neighbour keeps the group's context gate
    on; a short flagged request finishes; the default request that takes over
    its slot draws what it draws on a fresh engine."""
    e = _eng(P, max_batch=2, num_microbatches=1)
    e.start_loop()
    try:
        nb = e.submit([9, 8, 7], SamplingParams(greedy=True, max_new_tokens=150, repetition_penalty=1.2))
        a = e.submit(PROMPT, SamplingParams(greedy=True, max_new_tokens=3, no_repeat_ngram_size=1,
                                            repetition_penalty=3.0))
        got_a = a.wait(60)
        assert got_a != plain[:3]
        c = e.submit(PROMPT, PLAIN)
        assert not nb.done  # precondition: the neighbour is still decoding
        got_c = c.wait(60)
        still = not nb.done
        nb.wait(120)
    finally:
        e.stop_loop()
    assert got_c == plain
    assert still  # the default request ran beside the neighbour, behind the repetition pass


@pytest.mark.parametrize("world,dp,chunk", [(3, 1, 5), (4, 2, 0)])
def test_rank_process_stages_get_the_prompts_that_ask(tmp_path, world, dp, chunk):
    """One process per stage over gloo (rank-process `dist` mode): the plan
    wire carries the knobs, and the prompt ids of the groups that ask reach the
    last stage's process -- the tokens of the in-process engine; a middle stage
    and the default requests' groups travel as before."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prompts = [PROMPT, [4, 4, 4], [9, 8, 7, 6, 9, 8], PROMPT[:7]]
    kws = [dict(greedy=True, repetition_penalty=1.5, no_repeat_ngram_size=2), dict(greedy=True),
           dict(no_repeat_ngram_size=1, **SEEDED), dict(repetition_penalty=0.6, **SEEDED)]
    want = _eng(max_batch=8).generate_ids(prompts, [SamplingParams(max_new_tokens=8, **kw) for kw in kws])
    script = tmp_path / "w.py"
    script.write_text(textwrap.dedent(f"""
        import sys, json, torch
        sys.path.insert(0, {root!r})
        from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
        from llm_sharding_demo_amd.runtime.engine import build_engine
        cfg = EngineConfig(model_id="gpt2-test", max_batch=8, device="cpu", transport="gloo",
                           num_microbatches=2, dp_replicas={dp}, prefill_chunk={chunk})
        eng = build_engine(cfg)
        assert (eng.P, eng.R) == ({world // dp}, {dp})
        if eng.rank != 0:
            eng.worker_loop()
        else:
            out = eng.generate_ids({prompts!r}, [SamplingParams(max_new_tokens=8, **kw) for kw in {kws!r}])
            eng.shutdown()
            print("RESULT", json.dumps(out))
    """))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={port}", str(script)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][0]
    assert json.loads(line[len("RESULT "):]) == want


def test_interfaces_forward_the_fields(monkeypatch):
    import requests
    from fastapi.testclient import TestClient

    from llm_sharding_demo_amd import LLM
    from llm_sharding_demo_amd.serving import client as cl
    from llm_sharding_demo_amd.serving.server import create_app

    sent = {}

    class R:
        status_code = 200

        def json(self):
            return {"generated": "x"}

    def post(url, json=None, timeout=None):
        sent.update(json)
        return R()

    monkeypatch.setattr(requests, "post", post)
    cl.generate_text("Hi, ", repetition_penalty=1.3, no_repeat_ngram_size=2)
    assert sent["repetition_penalty"] == 1.3 and sent["no_repeat_ngram_size"] == 2
    sent.clear()
    cl.generate_text("Hi, ")
    assert "repetition_penalty" not in sent and "no_repeat_ngram_size" not in sent
    monkeypatch.undo()
    cfg = EngineConfig(model_id="gpt2-test", max_batch=4, device="cpu", role="coordinator")
    llm = LLM(cfg)
    text = "abcabcabcabc"
    ids = llm.tokenizer.encode(text)
    kw = dict(repetition_penalty=1.5, no_repeat_ngram_size=2)
    want = llm.engine.generate_ids([ids], [SamplingParams(greedy=True, max_new_tokens=8, **kw)])[0]
    assert _no_repeated_gram(ids, want, 2)
    dec = {"generated": llm.tokenizer.decode(ids + want, skip_special_tokens=True)}
    assert llm.generate_text(text, max_new_tokens=8, greedy=True, **kw) == dec
    assert llm.generate_text(text, max_new_tokens=8, greedy=True) != dec
    client = TestClient(create_app(cfg, engine=llm.engine))
    body = {"prompt": text, "max_new_tokens": 8, "greedy": True, **kw}
    r = client.post("/generate", json=body)
    assert r.status_code == 200 and r.json() == dec
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=11), dict(no_repeat_ngram_size=33),
                dict(no_repeat_ngram_size=-1)):
        assert client.post("/generate", json={**body, **bad}).status_code == 422
    props = client.get("/openapi.json").json()["components"]["schemas"]["GenerateReq"]["properties"]
    assert "repetition_penalty" in props and "no_repeat_ngram_size" in props


def test_cli_has_the_flags(capsys):
    from llm_sharding_demo_amd.__main__ import main

    with pytest.raises(SystemExit):
        main(["generate", "--help"])
    text = capsys.readouterr().out
    assert "--repetition-penalty" in text and "--no-repeat-ngram-size" in text


# ---------------------------------------------------------------------------
# DrawStage: call order, allocation, counter (a recorder backend of its own)

CAP, B, V, L, SLOTS = 4, 2, 16, 8, 4
FLAGS = list(itertools.product((False, True), repeat=5))


class Recorder:
    def __init__(self):
        self.calls, self.draw, self.args = [], None, {}

    def _knobs(self):
        tab = self.draw.ctx_tab
        return None if tab is None else [t.tolist() for t in tab[:3]]

    def repetition(self, logits, table, slots, step, vocab):
        self.calls.append(("repetition", None))
        self.args["repetition"] = (table, slots.tolist(), step, self._knobs(), table[3].tolist())

    def penalize(self, logits, hist, slots, counts, presence, frequency, vocab):
        self.calls.append(("penalize", None))

    def logit_edits(self, logits, table, slots, step, vocab):
        self.calls.append(("logit_edits", None))

    def sample_into(self, logits, samp, vocab, out, meta):
        self.calls.append(("sample_into", None))
        out.zero_()

    def sample(self, logits, state, vocab):
        self.calls.append(("sample", None))
        return torch.full((logits.shape[0],), 13, dtype=torch.int32)

    def record_tokens(self, hist, slots, step, tokens, active=None, back=0):
        self.calls.append(("record_tokens", back))

    def record_context(self, table, slots, step, tokens, active=None, back=0):
        self.calls.append(("record_context", back))
        self.args["record_context"] = (table, slots.tolist(), step, tokens.tolist(), active)

    def logprobs(self, logits, tokens, nlp, slots, step, active, rec, vocab, back=0):
        self.calls.append(("logprobs", back))


def _no_staging(gs, arr, dst):
    raise AssertionError("the pinned staging ring is for GPUs")


def _draw(max_seq=L, device="cpu"):
    be = Recorder()
    stage = types.SimpleNamespace(backend=be, device=torch.device(device), max_seq=max_seq,
                                  cfg=types.SimpleNamespace(vocab_size=V))
    d = be.draw = DrawStage(stage, SLOTS, _no_staging, contextlib.nullcontext)
    return d, be


def _group():
    w = types.SimpleNamespace(device=torch.device("cpu"), H=4, scratch_slot=SLOTS - 1, first=True, last=True, P=1)
    return GroupState(w, 0, CAP)


def test_nothing_until_asked():
    d, be = _draw()
    assert _group().ctx is False
    d.prepare((True, True, True, True))         # the 4-tuples of before: no context
    d.prepare((True, True, True, True, False))
    d.chunks(_group(), [Chunk(0, 1, 0, [5, 6], True)])
    assert d.ctx_tab is None and d.repetition_launches == 0 and be.calls == []
    d.prepare((False, False, False, False, True))
    plen, rpen, ngram, tok = d.ctx_tab
    assert (plen.tolist(), rpen.tolist(), ngram.tolist()) == ([0] * SLOTS, [1.0] * SLOTS, [0] * SLOTS)
    assert tok.shape == (SLOTS, L) and tok.dtype == plen.dtype == ngram.dtype == torch.int32
    assert rpen.dtype == torch.float32
    tab = d.ctx_tab
    d.prepare((False, False, False, False, True))
    assert d.ctx_tab is tab  # allocated once: captured graphs hold its addresses


def test_context_longer_than_the_kernel_holds_is_refused():
    d, _ = _draw(max_seq=8193, device="meta")
    d.stage.device = types.SimpleNamespace(type="cuda")
    with pytest.raises(ValueError, match="8192"):
        d.prepare((False, False, False, False, True))
    assert d.ctx_tab is None


@pytest.mark.parametrize("cut,pen,lp,edit,ctx", FLAGS)
def test_rows_order(cut, pen, lp, edit, ctx):
    d, be = _draw()
    gs = _group()
    gs.cut, gs.pen, gs.lp, gs.edit, gs.ctx = cut, pen, lp, edit, ctx
    d.prepare((cut, pen, lp, edit, ctx))
    assert (d.ctx_tab is not None) == ctx
    d.rows(gs, torch.zeros(B, V), B, None)
    assert be.calls == ([("repetition", None)] * ctx + [("penalize", None)] * pen + [("logit_edits", None)] * edit
                        + [("sample_into", None)] + [("record_tokens", 1)] * pen + [("record_context", 1)] * ctx
                        + [("logprobs", 1)] * lp)
    assert d.repetition_launches == 0  # the caller counts: one count() per issued item, replays included
    if ctx:
        table, slots, step, _, _ = be.args["repetition"]
        assert table is d.ctx_tab and step.data_ptr() == gs.sstep.data_ptr() and slots == gs.slots[:B].tolist()
        table, slots, step, _, active = be.args["record_context"]
        assert table is d.ctx_tab and step.data_ptr() == gs.sstep.data_ptr()
        assert active.data_ptr() == gs.active.data_ptr()
    d.count(gs)
    d.count(gs)
    assert d.repetition_launches == 2 * ctx
    assert (d.penalty_launches, d.logprob_launches, d.logit_edit_launches) == (2 * pen, 2 * lp, 2 * edit)


def test_chunks_write_the_context_and_finals_run_the_pass():
    d, be = _draw()
    gs = _group()
    rp = float(np.float32(1.3))
    first = [Chunk(0, 1, 0, [5, 6, 7], False, rpen=rp, ngram=2, plen=5), Chunk(1, 2, 0, [9], True)]
    d.chunks(gs, first)
    plen, rpen, ngram, tok = d.ctx_tab
    assert (plen.tolist(), rpen.tolist(), ngram.tolist()) == ([0, 5, 0, 0], [1.0, rp, 1.0, 1.0], [0, 2, 0, 0])
    assert tok[1].tolist() == [5, 6, 7, 0, 0, 0, 0, 0] and not tok[2].any()  # a default chunk's ids stay out
    plen[2], rpen[2], ngram[2] = 4, 2.0, 3   # what an earlier request left on slot 2
    fc = [Chunk(0, 1, 3, [8, 5], True, rpen=rp, ngram=2, plen=5), Chunk(2, 2, 0, [4, 4], True)]
    d.chunks(gs, fc)  # a later chunk writes its ids alone; a default one that opens a prompt resets its slot
    assert (plen.tolist(), rpen.tolist(), ngram.tolist()) == ([0, 5, 0, 0], [1.0, rp, 1.0, 1.0], [0, 2, 0, 0])
    assert tok[1].tolist() == [5, 6, 7, 8, 5, 0, 0, 0] and not tok[2].any()
    assert be.calls == [] and d.repetition_launches == 0
    ids = d.finals(gs, fc, torch.zeros(2, V))
    assert ids.tolist() == [13, 13]
    assert be.calls == [("repetition", None), ("sample", None), ("record_context", 0)]
    assert d.repetition_launches == 1
    table, slots, step, knobs, toks = be.args["repetition"]
    assert table is d.ctx_tab and slots == [1, 2] and step is None
    assert knobs == [[0, 5, 0, 0], [1.0, rp, 1.0, 1.0], [0, 2, 0, 0]] and toks[1][:5] == [5, 6, 7, 8, 5]
    table, slots, step, tokens, active = be.args["record_context"]
    assert table is d.ctx_tab and slots == [1, 2] and step is None and tokens == [13, 13] and active is None
    # default finals: nothing of the pass, table or not
    be.calls.clear()
    d.finals(gs, [Chunk(3, 0, 0, [1], True)], torch.zeros(1, V))
    assert be.calls == [("sample", None)] and d.repetition_launches == 1
    # a flagged chunk without its ids (a plan that travelled without them) is an error, not a guess
    with pytest.raises(ValueError, match="token ids"):
        d.chunks(gs, [Chunk(0, 1, 0, range(3), False, rpen=rp, plen=3)])
    with pytest.raises(ValueError, match="max_seq_len"):
        d.chunks(gs, [Chunk(0, 1, 6, [1, 2, 3], False, ngram=1, plen=9)])
