"""Per-request bad_words on the CPU: validation, the host reference
(ops/reference.py bad_words) against a brute-force loop of the rule, the plan
wire, DrawStage with a recording backend, the engine on the reference backend
(gpt2-test, random weights) with one stage, two thread stages and rank
processes, and /generate.
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
                                                _pack_group, _unpack_group, has_allow, has_bad, has_context,
                                                has_edits, row_features)

from . import bad_words_cases as bc

INF = float("inf")
I32MAX = 2 ** 31 - 1


# ---------------------------------------------------------------------------
# validation

def test_defaults_validate_and_are_off():
    sp = SamplingParams()
    sp.validate()
    assert sp.bad_words is None and sp.bad_word_list() == [] and sp.bad_word_entries() is None
    assert not sp.has_context
    SamplingParams(bad_words=[[0]]).validate()
    SamplingParams(bad_words=([5, np.int64(7)], (5,)), greedy=True).validate()
    SamplingParams(bad_words=[list(range(32))]).validate()
    assert (EngineConfig().max_bad_words, EngineConfig().max_bad_word_tokens) == (64, 512)


@pytest.mark.parametrize("bad", [[[]], [[1], []], [[1.0]], [["1"]], [[True]], [[None]], "12", [b"12"], ["ab"], 5, [5],
                                 {1: 2}, [{1: 2}], [[-1]], [[3, -2]], [[2 ** 31]], [list(range(33))]])
def test_validate_refuses(bad):
    with pytest.raises(ValueError):
        SamplingParams(bad_words=bad).validate()
    with pytest.raises(ValueError):
        SamplingParams(greedy=True, bad_words=bad).validate()  # greedy requests are banned too


def test_limits_and_duplicates():
    sp = SamplingParams(bad_words=[[3, 4], [9], (3, 4), [4, 3], [9]])
    assert sp.bad_word_list() == [(3, 4), (9,), (4, 3)]  # exact duplicates collapse, the order stays
    assert sp.bad_word_entries() == ((2, 3, 5), (3, 4, 9, 4, 3))
    many = [[i] for i in range(65)]
    SamplingParams(bad_words=many[:64]).validate()
    with pytest.raises(ValueError, match="max_bad_words"):
        SamplingParams(bad_words=many).validate()
    SamplingParams(bad_words=many + many).validate(max_bad_words=65)  # counted after the collapse
    long_ = [list(range(i, i + 32)) for i in range(17)]               # 544 tokens
    SamplingParams(bad_words=long_[:16]).validate()
    with pytest.raises(ValueError, match="max_bad_word_tokens"):
        SamplingParams(bad_words=long_).validate()
    SamplingParams(bad_words=long_).validate(max_bad_word_tokens=544)
    for kw in (dict(max_bad_words=0), dict(max_bad_words=257), dict(max_bad_word_tokens=0),
               dict(max_bad_word_tokens=4097)):
        with pytest.raises(ValueError):
            EngineConfig(**kw)
    cfg = EngineConfig(max_bad_words=256, max_bad_word_tokens=4096)
    assert (cfg.max_bad_words, cfg.max_bad_word_tokens) == (256, 4096)


def test_limits_come_from_the_environment(monkeypatch):
    monkeypatch.setenv("MAX_BAD_WORDS", "7")
    monkeypatch.setenv("MAX_BAD_WORD_TOKENS", "99")
    cfg = EngineConfig.from_env()
    assert (cfg.max_bad_words, cfg.max_bad_word_tokens) == (7, 99)


def _eng(P=1, max_batch=4, model="gpt2-test", **kw):
    return Engine(EngineConfig(model_id=model, num_stages=P, max_batch=max_batch, device="cpu", **kw))


def test_engine_checks_ids_limits_and_a_drawable_token():
    e = _eng(model="llama-test", max_logit_edits=1024, max_bad_words=256, max_bad_word_tokens=1024)
    V, eos = e.mcfg.vocab_size, e.mcfg.eos_token_id

    def refused(prompt=(1, 2), **kw):
        sp = SamplingParams(max_new_tokens=2, **kw)
        with pytest.raises(ValueError):
            e.generate_ids([list(prompt)], [sp])
        with pytest.raises(ValueError):
            e.submit(list(prompt), sp)

    refused(bad_words=[[V]])
    refused(bad_words=[[3, V + 40, 5]])
    refused(bad_words=[[]])
    refused(bad_words=[[i] for i in range(257)])            # the engine's own limit
    small = _eng(max_bad_words=2, max_bad_word_tokens=5)
    with pytest.raises(ValueError, match="max_bad_words"):
        small.submit([1], SamplingParams(bad_words=[[1], [2], [3]]))
    with pytest.raises(ValueError, match="max_bad_word_tokens"):
        small.submit([1], SamplingParams(bad_words=[[1, 2, 3], [4, 5, 6]]))
    # the allowed set less the request's bans less the distinct last tokens must leave a token
    refused(allowed_token_ids=[5, 6], bad_words=[[9, 5], [6]])
    refused(allowed_token_ids=[5, 6, 7], banned_token_ids=[7], bad_words=[[9, 5], [8, 8, 6]])
    refused(allowed_token_ids=[eos, 7], min_new_tokens=1, bad_words=[[7]])
    ok = SamplingParams(max_new_tokens=3, allowed_token_ids=[5, 6, 7], bad_words=[[9, 5], [1, 5], [6]])  # 3 - 2 > 0
    assert e.generate_ids([[1, 2]], [ok])[0] == [7, 7, 7]
    # without a list: the vocabulary less the bans less the last tokens
    half = [[t] for t in range(744, 1000)]                  # 256 distinct last tokens
    refused(banned_token_ids=list(range(0, 744)), bad_words=half)           # 1000 - 744 - 256 = 0
    left = SamplingParams(max_new_tokens=2, banned_token_ids=list(range(1, 744)), bad_words=half)
    assert e.generate_ids([[1, 2]], [left])[0] == [0, 0]
    # the n-gram rule counts the last tokens beside prompt + max_new_tokens
    lst = list(range(100, 112))
    refused(prompt=[1] * 8, allowed_token_ids=lst, no_repeat_ngram_size=1, bad_words=[[100], [5, 101]])  # 8 + 2 + 2 >= 12
    sp = SamplingParams(max_new_tokens=2, allowed_token_ids=lst, no_repeat_ngram_size=1, bad_words=[[100], [5, 101]])
    out = e.generate_ids([[1] * 5], [sp])[0]                                                            # 5 + 2 + 2 < 12
    assert len(set(out)) == 2 and set(out) <= set(range(101, 112))


# ---------------------------------------------------------------------------
# the host reference against the brute-force rule

def _run_ref(c, seg, step="step"):
    lg = c["lg"].clone()
    sm = bc.segmax_of(c["lg"]) if seg else None
    st = c[step] if step is not None else None
    ref.bad_words(lg, c["tab"], c["ctx"], c["slots"], st, c["V"], sm)
    return lg, sm


@pytest.mark.parametrize("V,Vp", [(1000, 1024), (50257, 50304)])
@pytest.mark.parametrize("seg", [True, False])
def test_reference_equals_brute_force(V, Vp, seg):
    c = bc.case(V, Vp)
    lg0, before = c["lg"], [t.clone() for t in c["tab"] + c["ctx"]]
    for step in ("step", None):
        want, wsm = bc.brute(c, step)
        got, gsm = _run_ref(c, seg, step)
        assert torch.equal(bc.bits(got), bc.bits(want))
        if seg:
            assert torch.equal(bc.bits(gsm), bc.bits(wsm)) and torch.equal(bc.bits(gsm), bc.bits(bc.segmax_of(got)))
        assert torch.equal(bc.bits(got[:, V:]), bc.bits(lg0[:, V:]))  # padding columns
    assert all(torch.equal(a, b) for a, b in zip(before, c["tab"] + c["ctx"]))  # the tables are read only
    got, gsm = _run_ref(c, seg)
    # the case does what it says: contexts of length m - 2 and m - 1 (row 3), L (row 4), ...
    for r in range(c["B"]):
        changed = {int(t) for t in (bc.bits(got[r]) != bc.bits(lg0[r])).nonzero().flatten()}
        expect = {t for t in c["ban"].get(r, ()) if lg0[r, t] != -INF}
        assert changed == expect, r
        assert all(got[r, t] == -INF for t in c["ban"].get(r, ()))
    assert all(len(c["ban"][r]) > 0 for r in (2, 3, 4, 5, 6, 7, 8, 9, 13)) and len(c["ban"][8]) >= 64
    assert c["ban"][8] != c["ban"][9]  # two rows on one slot at different steps
    assert int(c["tab"][0][14]) == bc.N and c["ban"][7] >= {c["am"][7]}
    # draw 0: the prompts alone -- another result (row 13 bans its other sequence; row 3, step 0 already, stays)
    got0, _ = _run_ref(c, seg, None)
    assert got0[13, 91] == -INF and got0[13, 90] == lg0[13, 90] and got[13, 90] == -INF and got[13, 91] == lg0[13, 91]
    assert torch.equal(bc.bits(got0[3]), bc.bits(got[3]))


def test_reference_context_of_length_zero():
    """An empty context: only the one-token sequences apply."""
    V = 24
    lg = torch.arange(2 * V, dtype=torch.float32).reshape(2, V)
    tab = (torch.tensor([3, 3], dtype=torch.int32), torch.tensor([[1, 3, 4], [1, 3, 4]], dtype=torch.int32),
           torch.tensor([[9, 0, 10, 11], [9, 0, 10, 11]], dtype=torch.int32))
    ctx = (torch.tensor([0, 1], dtype=torch.int32), None, None, torch.zeros(2, 8, dtype=torch.int32))
    out, sm = ref.bad_words(lg.clone(), tab, ctx, torch.tensor([0, 1]), None, V, bc.segmax_of(lg))
    assert (out[0] == -INF).nonzero().flatten().tolist() == [9, 11]       # [9] and [11]; [0, 10] needs a context
    assert (out[1] == -INF).nonzero().flatten().tolist() == [9, 10, 11]   # its context is [0]
    assert sm.tolist() == [[7.0, 15.0, 23.0], [31.0, 39.0, 47.0]]
    out = ref.bad_words(lg.clone(), tab, ctx, torch.tensor([0, 1]), torch.tensor([1, 0]), V)
    assert (out[0] == -INF).nonzero().flatten().tolist() == [9, 10, 11]   # one generated token: the context is [0]


@pytest.mark.parametrize("B", [1, 3, 256])
def test_reference_random_rows(B):
    c = bc.random_case(1000, 1024, B)
    want, wsm = bc.brute(c)
    got, gsm = _run_ref(c, True)
    assert torch.equal(bc.bits(got), bc.bits(want)) and torch.equal(bc.bits(gsm), bc.bits(wsm))
    assert not torch.equal(bc.bits(got), bc.bits(c["lg"]))


def test_reference_largest_context():
    c = bc.big_case()
    want, wsm = bc.brute(c)
    got, gsm = _run_ref(c, True)
    assert torch.equal(bc.bits(got), bc.bits(want)) and torch.equal(bc.bits(gsm), bc.bits(wsm))
    assert got[0, c["am"]] == -INF and got[0, 3] == -INF and got[0, 4] == c["lg"][0, 4]
    assert torch.equal(bc.bits(got[1]), bc.bits(c["lg"][1]))


# ---------------------------------------------------------------------------
# plan wire

BAD_A = ((1, 3), (7, 8, 9))
BAD_B = ((2,), (4, 4))
ED1 = ((7,), (-INF,), (I32MAX,))
MASK = SamplingParams(allowed_token_ids=[1, 40, 95]).allowed_mask(3).tobytes()


def _plan(bad=True, edits=False, ngram=False, mask=False, defaults=False):
    """defaults: the new fields spelled out at their defaults.  Chunk 0 asks and
    is final, chunk 1 asks and is not (the count alone), chunk 3 asks too; row
    0 asks."""
    cb = [dict(nbad=2, bad=BAD_A, plen=3), dict(nbad=2, plen=9), dict(), dict(nbad=1, bad=BAD_B, plen=5)]
    rb = [dict(bad=1, ctx=1), dict()]
    if not bad:
        cb, rb = ([dict(nbad=0, bad=None)] * 4, [dict(bad=0)] * 2) if defaults else ([{}] * 4, [{}] * 2)
    if edits:
        cb[2] = dict(cb[2], nedits=1, edits=ED1)
        rb[1] = dict(rb[1], nedits=1)
    if ngram:
        cb[1] = dict(cb[1], rpen=1.0, ngram=2, plen=9)
        cb[2] = dict(cb[2], ngram=3, plen=1)
        rb[1] = dict(rb[1], ctx=1)
    if mask:
        cb[3] = dict(cb[3], allow=1, mask=MASK)
        rb[0] = dict(rb[0], allow=1)
    gp = GroupPlan(0, ret=2, n=2, b=2, ctxb=256)
    gp.chunks = [Chunk(1, 3, 0, [5, 6, 7], True, 0.7, 40, False, 11, **cb[0]),
                 Chunk(2, 4, 0, [8, 9], False, 0.6, 40, False, 12, **cb[1]),
                 Chunk(5, 6, 0, [8], True, 0.6, 40, False, 12, **cb[2]),
                 Chunk(6, 7, 4, [1], True, 0.6, 40, True, 13, logprobs=2, **cb[3])]
    gp.rows = [Row(3, 5, 9, 0.9, 20, False, 13, 4, 0, presence=0.5, **rb[0]),
               Row(4, 6, 2, 0.6, 40, True, 14, 1, 1, **rb[1])]
    return StepPlan(step=7, groups=[gp, GroupPlan(1, ret=1, n=1, b=1, ctxb=256)])


COMBOS = list(itertools.product((False, True), repeat=3))


@pytest.mark.parametrize("edits,ngram,mask", COMBOS)
def test_plan_wire_round_trip(edits, ngram, mask):
    plan = _plan(edits=edits, ngram=ngram, mask=mask)
    g = plan.groups[0]
    assert has_bad(g.chunks) and has_bad(g.rows) and not has_bad(plan.groups[1].chunks)
    assert has_context(g.chunks) and has_context(g.rows)  # an asking request is a context request
    assert [c.ctx for c in g.chunks] == [True, True, ngram, True]
    for enc in (PlanEncoder(ids=True), PlanEncoder(ids=False, ctx_ids=True), PlanEncoder(ids=False)):
        rec, payload = enc.encode(plan)
        assert rec[0] == MAGIC_PICKLE
        out = PlanDecoder().decode(rec, lambda n: payload)
        g0 = out.groups[0]
        assert [c.nbad for c in g0.chunks] == [2, 2, 0, 1]
        assert [c.bad for c in g0.chunks] == [BAD_A, None, None, BAD_B]
        assert [c.plen for c in g0.chunks] == [3, 9, int(ngram), 5]
        assert [r.bad for r in g0.rows] == [1, 0] and [r.ctx for r in g0.rows] == [1, int(ngram)]
        assert g0.rows[0].presence == 0.5
        assert [c.nedits for c in g0.chunks] == [0, 0, int(edits), 0] and g0.chunks[2].edits == (ED1 if edits else None)
        assert [c.mask for c in g0.chunks] == [None, None, None, MASK if mask else None]
        assert [r.allow for r in g0.rows] == [int(mask), 0]
        # the prompt ids of a group that asks reach a last stage, as with no_repeat_ngram_size
        if enc.ids or enc.ctx_ids:
            assert [list(c.ids) for c in g0.chunks] == [[5, 6, 7], [8, 9], [8], [1]]
        else:
            assert all(isinstance(c.ids, range) for c in g0.chunks)
        if enc.ids:
            assert out == plan
    assert pickle.loads(pickle.dumps(plan)) == plan
    packed = _pack_group(g, True)
    # one more trailing element behind the mask's place; earlier places without a tenant are held by None
    assert len(packed) == 13 and (packed[9] is not None) == edits and packed[10] is not None
    assert (packed[11] is not None) == mask
    assert _unpack_group(*packed) == g
    assert len(_pack_group(plan.groups[1], True)) == 9  # a group of the same plan without the feature


def test_plan_rows_alone_and_chunks_alone():
    plan = _plan()
    g = plan.groups[0]
    rows_only = GroupPlan(0, ret=2, n=2, b=2, ctxb=256, rows=g.rows)
    chunks_only = GroupPlan(0, ret=2, n=0, b=0, ctxb=256, chunks=g.chunks)
    for gp in (rows_only, chunks_only):
        packed = _pack_group(gp, True)
        assert len(packed) == 13 and _unpack_group(*packed) == gp


def test_plan_without_the_feature_packs_as_before():
    for edits, ngram, mask in COMBOS:
        n = 12 if mask else 11 if ngram else 10 if edits else 9
        plan = _plan(bad=False, edits=edits, ngram=ngram, mask=mask)
        spelled = _plan(bad=False, edits=edits, ngram=ngram, mask=mask, defaults=True)
        for ids, ctx_ids in ((True, False), (False, True), (False, False)):
            packed = _pack_group(plan.groups[0], ids, ctx_ids)
            assert len(packed) == n  # the 9 / 10 / 11 / 12-tuples of before
            if ids:
                assert _unpack_group(*packed) == plan.groups[0]
            a = PlanEncoder(ids=ids, ctx_ids=ctx_ids).encode(plan)
            b = PlanEncoder(ids=ids, ctx_ids=ctx_ids).encode(spelled)
            assert a[1] == b[1] and np.array_equal(a[0], b[0])  # byte for byte
            asking = PlanEncoder(ids=ids, ctx_ids=ctx_ids).encode(_plan(edits=edits, ngram=ngram, mask=mask))[1]
            assert len(asking) > len(a[1])
    plan, asking = _plan(bad=False), _plan()
    # the gate is a flag of its own: row_features' triple and the other gates do not know the field
    assert row_features(asking.groups[0].rows) == row_features(plan.groups[0].rows) == (False, True, False)
    assert not has_edits(asking.groups[0].rows) and not has_allow(asking.groups[0].rows)
    assert not has_bad(plan.groups[0].rows) and not has_bad(plan.groups[0].chunks)
    assert not has_context(plan.groups[0].rows) and not has_context(plan.groups[0].chunks)
    assert Row(1, 1, 1, 0.6, 40, False, 1, 0, 0).bad == 0
    c = Chunk(1, 1, 0, [1], True)
    assert c.nbad == 0 and c.bad is None and not c.ctx and GroupPlan(0).bad is None


# ---------------------------------------------------------------------------
# DrawStage: call order, allocation, counters (a recorder backend of its own)

CAP, B, V, L, SLOTS = 4, 2, 16, 8, 4
FLAGS = list(itertools.product((False, True), repeat=7))


class Recorder:
    def __init__(self):
        self.calls, self.draw, self.args = [], None, {}

    def repetition(self, logits, table, slots, step, vocab):
        self.calls.append(("repetition", None))

    def bad_words(self, logits, table, ctx_table, slots, step, vocab):
        self.calls.append(("bad_words", None))
        self.args["bad_words"] = (table, ctx_table, slots.tolist(), step, [t.tolist() for t in table],
                                  ctx_table[0].tolist(), ctx_table[3].tolist())

    def penalize(self, logits, hist, slots, counts, presence, frequency, vocab):
        self.calls.append(("penalize", None))

    def logit_edits(self, logits, table, slots, step, vocab):
        self.calls.append(("logit_edits", None))

    def allow_mask(self, logits, table, slots, vocab):
        self.calls.append(("allow_mask", None))

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

    def logprobs(self, logits, tokens, nlp, slots, step, active, rec, vocab, back=0):
        self.calls.append(("logprobs", back))


def _no_staging(gs, arr, dst):
    raise AssertionError("the pinned staging ring is for GPUs")


def _draw(max_seq=L, device="cpu"):
    be = Recorder()
    stage = types.SimpleNamespace(backend=be, device=torch.device(device), max_seq=max_seq,
                                  cfg=types.SimpleNamespace(vocab_size=V, vocab_padded=V))
    d = be.draw = DrawStage(stage, SLOTS, _no_staging, contextlib.nullcontext)
    d.max_bad_words, d.max_bad_word_tokens = 3, 6
    return d, be


def _group():
    w = types.SimpleNamespace(device=torch.device("cpu"), H=4, scratch_slot=SLOTS - 1, first=True, last=True, P=1)
    return GroupState(w, 0, CAP)


def test_nothing_until_asked():
    d, be = _draw()
    assert _group().bad is False
    fresh = DrawStage(d.stage, SLOTS, _no_staging, contextlib.nullcontext)
    assert (fresh.max_bad_words, fresh.max_bad_word_tokens, fresh.bad_words_launches) == (64, 512, 0)
    for feats in ((True,) * 4, (True,) * 4 + (False,), (True,) * 4 + (False, False), (True,) * 4 + (True, True, False)):
        d.prepare(feats)  # the 4-, 5- and 6-tuples of before: no bad-words table
    d.chunks(_group(), [Chunk(0, 1, 0, [5, 6], True)])
    d.finals(_group(), [Chunk(0, 1, 0, [5, 6], True, nedits=1, edits=ED1, allow=1, mask=bytes(4))], torch.zeros(1, V))
    assert d.bad_tab is None and d.bad_words_launches == 0 and "bad_words" not in dict(be.calls)
    d2, be2 = _draw()
    d2.prepare((False,) * 6 + (True,))
    cnt, end, tok = d2.bad_tab
    assert cnt.tolist() == [0] * SLOTS and end.shape == (SLOTS, 3) and tok.shape == (SLOTS, 6)
    assert cnt.dtype == end.dtype == tok.dtype == torch.int32
    assert d2.ctx_tab is not None and d2.allow_tab is None and d2.edit_tab is None  # the pass reads the context
    tab = d2.bad_tab
    d2.prepare((False,) * 6 + (True,))
    assert d2.bad_tab is tab  # allocated once: captured graphs hold its addresses
    assert be2.calls == []


@pytest.mark.parametrize("cut,pen,lp,edit,ctx,allow,bad", FLAGS)
def test_rows_order(cut, pen, lp, edit, ctx, allow, bad):
    ctx = ctx or bad  # an asking row is a context row
    d, be = _draw()
    gs = _group()
    gs.cut, gs.pen, gs.lp, gs.edit, gs.ctx, gs.allow, gs.bad = cut, pen, lp, edit, ctx, allow, bad
    d.prepare((cut, pen, lp, edit, ctx, allow, bad))
    assert (d.bad_tab is not None) == bad and (d.ctx_tab is not None) == ctx
    d.rows(gs, torch.zeros(B, V), B, None)
    assert be.calls == ([("repetition", None)] * ctx + [("bad_words", None)] * bad + [("penalize", None)] * pen
                        + [("logit_edits", None)] * edit + [("allow_mask", None)] * allow + [("sample_into", None)]
                        + [("record_tokens", 1)] * pen + [("record_context", 1)] * ctx + [("logprobs", 1)] * lp)
    assert d.bad_words_launches == 0  # the caller counts: one count() per issued item, replays included
    if bad:
        table, ctab, slots, step = be.args["bad_words"][:4]
        assert table is d.bad_tab and ctab is d.ctx_tab and step.data_ptr() == gs.sstep.data_ptr()
        assert slots == gs.slots[:B].tolist()
    d.count(gs)
    d.count(gs)
    assert d.bad_words_launches == 2 * bad and d.repetition_launches == 2 * ctx and d.allow_launches == 2 * allow


def test_finals_write_counts_and_slot_reuse_inherits_nothing():
    d, be = _draw()
    gs = _group()
    # default finals before anybody asked: no table
    d.finals(gs, [Chunk(3, 0, 0, [1], True)], torch.zeros(1, V))
    assert d.bad_tab is None and be.calls == [("sample", None)]
    be.calls.clear()
    fc = [Chunk(0, 1, 0, [5, 6, 7], True, nbad=2, bad=BAD_A, plen=3), Chunk(2, 2, 0, [4, 4], True)]
    d.chunks(gs, fc)
    assert be.calls == [] and d.bad_tab is None
    plen, _, _, ctok = d.ctx_tab
    assert plen.tolist() == [0, 3, 0, 0] and ctok[1].tolist()[:3] == [5, 6, 7] and not ctok[2].any()
    ids = d.finals(gs, fc, torch.zeros(2, V))
    assert ids.tolist() == [13, 13]
    # right after the repetition pass, which reads the same context; ahead of the draw; the token goes in behind
    assert be.calls == [("repetition", None), ("bad_words", None), ("sample", None), ("record_context", 0)]
    assert d.bad_words_launches == 1
    table, ctab, slots, step, tabv, plenv, ctokv = be.args["bad_words"]
    assert table is d.bad_tab and ctab is d.ctx_tab and slots == [1, 2] and step is None
    assert tabv[0] == [0, 2, 0, 0] and tabv[1][1] == [1, 3, 0] and tabv[2][1] == [7, 8, 9, 0, 0, 0]
    assert plenv == [0, 3, 0, 0] and ctokv[1][:3] == [5, 6, 7]  # the entries and the prompt are there ahead of the pass
    # the table exists: a default final chunk on the asker's slot writes its count, zero
    be.calls.clear()
    d.finals(gs, [Chunk(4, 1, 0, [1], True), Chunk(5, 3, 0, [2], True, nbad=1, bad=BAD_B, plen=1)], torch.zeros(2, V))
    cnt, end, tok = d.bad_tab
    assert cnt.tolist() == [0, 0, 0, 1] and end[3].tolist()[:1] == [2] and tok[3].tolist()[:2] == [4, 4]
    assert be.calls[:3] == [("repetition", None), ("bad_words", None), ("sample", None)]
    # all-default finals with the table: the counts are written, zero included, and no pass runs
    be.calls.clear()
    d.finals(gs, [Chunk(6, 3, 0, [1], True)], torch.zeros(1, V))
    assert cnt.tolist() == [0, 0, 0, 0] and be.calls == [("sample", None)] and d.bad_words_launches == 2
    # entries that are missing, or more than the table holds, are an error, not a guess
    for c in (Chunk(0, 1, 0, [5], True, nbad=2, plen=1), Chunk(0, 1, 0, [5], True, nbad=1, bad=BAD_A, plen=1),
              Chunk(0, 1, 0, [5], True, nbad=4, bad=((1, 2, 3, 4), (1, 2, 3, 4)), plen=1),
              Chunk(0, 1, 0, [5], True, nbad=1, bad=((7,), tuple(range(7))), plen=1)):
        with pytest.raises(ValueError, match="max_bad_words"):
            d.finals(gs, [c], torch.zeros(1, V))


# ---------------------------------------------------------------------------
# engine (gpt2-test on the CPU, reference backend)

PROMPT = [5, 6, 7, 5, 6, 7, 5, 6, 9, 9, 5, 6]
N = 16
PLAIN = SamplingParams(greedy=True, max_new_tokens=N)
SEEDED = dict(temperature=1.1, top_k=50, seed=21)


class _Tap:
    """The last stage's reference backend, recording the logits every asking
    row was handed to the bad-words pass: (slot, draw counter) -> raw logits."""

    def __init__(self, be, draw):
        object.__setattr__(self, "_be", be)
        object.__setattr__(self, "_draw", draw)
        object.__setattr__(self, "seen", {})

    def __getattr__(self, name):
        return getattr(self._be, name)

    def __setattr__(self, name, value):
        setattr(self._be, name, value)

    def bad_words(self, logits, table, ctx_table, slots, step, vocab):
        assert table is self._draw.bad_tab and ctx_table is self._draw.ctx_tab
        for i, s in enumerate(slots.tolist()):
            if int(table[0][s]) != 0:
                self.seen[(s, int(step[i]) if step is not None else 0)] = logits[i].clone()
        self._be.bad_words(logits, table, ctx_table, slots, step, vocab)


def _tapped(P=1, **kw):
    e = _eng(P, **kw)
    tap = e.stages[-1].backend = _Tap(e.stages[-1].backend, e.workers[-1].draw)
    return e, tap


def _resimulate(seen, prompt, sp, V):
    """The request's tokens from the recorded raw logits: the brute-force rule
    over prompt + the tokens drawn so far, then the host sampler."""
    slot = {s for s, _ in seen}
    assert len(slot) == 1  # one asking request ran
    s, out = slot.pop(), []
    seed = torch.tensor([sp.seed if sp.seed is not None else 0])
    for c in range(sp.max_new_tokens):
        row, _ = bc.brute_row([np.float32(v) for v in seen[(s, c)].tolist()], list(prompt) + out, sp.bad_words, V)
        lg = torch.tensor(np.array([row], dtype=np.float32))
        u = counter_uniform(seed, torch.tensor([c]))
        out.append(int(ref.sample(lg, torch.tensor([sp.temperature]), torch.tensor([sp.top_k], dtype=torch.int32),
                                  torch.tensor([int(sp.greedy)], dtype=torch.int32), u, V,
                                  torch.tensor([sp.top_p]), torch.tensor([sp.min_p]))[0]))
    return out


def _never_completed(prompt, out, words):
    x = list(prompt) + list(out)
    return not any(x[e + 1 - len(w): e + 1] == list(w) for w in words for e in range(len(prompt), len(x))
                   if e + 1 >= len(w))


@pytest.fixture(scope="module")
def plain():
    e = _eng()
    return e.generate_ids([PROMPT], [PLAIN])[0], e.generate_ids([PROMPT], [SamplingParams(max_new_tokens=N, **SEEDED)])[0]


def _words(plain_out):
    """Sequences the plain run completes: its first token behind the prompt's
    last two, a later bigram, a later token; and one it never meets."""
    return [PROMPT[-2:] + [plain_out[0]], list(plain_out[2:4]), [plain_out[6]], [999, 998, 997]]


@pytest.mark.parametrize("mode", ["greedy", "seeded"])
def test_engine_tokens_are_the_host_resimulation(plain, mode):
    base = dict(greedy=True) if mode == "greedy" else SEEDED
    unasked = plain[0] if mode == "greedy" else plain[1]
    words = _words(unasked)
    assert not _never_completed(PROMPT, unasked, words)  # precondition: the plain run completes them
    sp = SamplingParams(max_new_tokens=N, bad_words=words, **base)
    e, tap = _tapped()
    got = e.generate_ids([PROMPT], [sp])[0]
    Vm = e.mcfg.vocab_size
    assert len(got) == N and sorted({c for _, c in tap.seen}) == list(range(N))
    assert got == _resimulate(tap.seen, PROMPT, sp, Vm)
    assert e.workers[-1].draw.bad_words_launches == N  # the prefill draw and N - 1 decode items
    assert _never_completed(PROMPT, got, words) and got != unasked
    assert e.scheduler._badwords == 0  # released with the request
    # 2 in-process stages, and a prompt prefilled in chunks of 5: the same tokens
    e2, tap2 = _tapped(2)
    assert e2.generate_ids([PROMPT], [sp])[0] == got
    assert [w.draw.bad_words_launches for w in e2.workers] == [0, N] and e2.workers[0].draw.bad_tab is None
    assert all(torch.equal(bc.bits(tap2.seen[k]), bc.bits(v)) for k, v in tap.seen.items())
    assert _eng(prefill_chunk=5).generate_ids([PROMPT], [sp])[0] == got
    assert _eng(2, prefill_chunk=5).generate_ids([PROMPT], [sp])[0] == got


def test_engine_default_traffic_launches_nothing(plain):
    for P in (1, 2):
        e = _eng(P)
        others = [SamplingParams(temperature=0.7, top_k=5, seed=3, max_new_tokens=4),
                  SamplingParams(greedy=True, max_new_tokens=7, presence_penalty=1.0)]
        assert e.generate_ids([PROMPT, [4], [9, 8, 7, 6]], [PLAIN] + others)[0] == plain[0]
        assert all(w.draw.bad_words_launches == 0 and w.draw.bad_tab is None and w.draw.ctx_tab is None
                   for w in e.workers)
        assert e.scheduler._badwords == 0
        e.generate_ids([PROMPT], [SamplingParams(greedy=True, max_new_tokens=3, bad_words=[[plain[0][0]]])])
        assert e.scheduler._badwords == 0 and e.workers[-1].draw.bad_tab is not None
        n = e.workers[-1].draw.bad_words_launches
        assert e.generate_ids([PROMPT], [PLAIN])[0] == plain[0]   # the table exists now: still nothing runs
        assert e.workers[-1].draw.bad_words_launches == n == 3


@pytest.mark.parametrize("P", [1, 2])
def test_engine_neighbours_and_other_knobs(P, plain):
    e = _eng(P, num_microbatches=1)  # one group: the default requests share it with the asking one
    seeded = SamplingParams(max_new_tokens=N, **SEEDED)
    others = [SamplingParams(temperature=0.7, top_k=5, seed=3, max_new_tokens=4), seeded,
              SamplingParams(greedy=True, max_new_tokens=9)]
    prompts = [[4], PROMPT, [9, 8, 7, 6]]
    alone = e.generate_ids(prompts, others)
    assert alone[1] == plain[1] and e.workers[-1].draw.bad_words_launches == 0
    words = _words(plain[1])
    asking = SamplingParams(max_new_tokens=N, bad_words=words, **SEEDED)
    a_alone = e.generate_ids([PROMPT], [asking])[0]
    got = e.generate_ids(prompts[:1] + [PROMPT] + prompts[1:], others[:1] + [asking] + others[1:])
    assert got[1] == a_alone and got[:1] + got[2:] == alone  # asking never changes another request's draws
    assert a_alone != alone[1] and _never_completed(PROMPT, a_alone, words)
    # beside the n-gram ban, a penalty, edits, a mask and logprobs: both rules hold, logprobs come after the ban
    first = plain[0][0]
    sp = SamplingParams(greedy=True, max_new_tokens=8, bad_words=[[PROMPT[-1], first]], no_repeat_ngram_size=2,
                        repetition_penalty=1.3, presence_penalty=0.5, banned_token_ids=[3],
                        allowed_token_ids=list(range(0, 1000, 2)) + [first], logprobs=3)
    r = e.generate_requests([PROMPT], [sp])[0]
    assert r.output[0] != first and _never_completed(PROMPT, r.output, sp.bad_words)
    assert all(t % 2 == 0 or t == first for t in r.output) and 3 not in r.output
    x = PROMPT + r.output
    assert all(x[i: i + 2] != x[j: j + 2] for j in range(len(PROMPT) - 1, len(x) - 1) for i in range(j))
    assert all(i != first for i, _ in r.logprobs.top_logprobs[0]) or dict(r.logprobs.top_logprobs[0])[first] == -INF


@pytest.mark.parametrize("P", [1, 2])
def test_engine_slot_reuse_does_not_inherit_the_words(P, plain):
    """Two KV slots: a long asking neighbour keeps the group's gate on; a short
    asking request finishes; the default request that takes over its slot
    draws what it draws on a fresh engine."""
    e = _eng(P, max_batch=2, num_microbatches=1)
    e.start_loop()
    try:
        nb = e.submit([9, 8, 7], SamplingParams(greedy=True, max_new_tokens=150, bad_words=[[1, 2]]))
        a = e.submit(PROMPT, SamplingParams(greedy=True, max_new_tokens=3, bad_words=[[t] for t in set(plain[0])]))
        got_a = a.wait(60)
        assert not set(got_a) & set(plain[0])
        c = e.submit(PROMPT, PLAIN)
        assert not nb.done  # precondition: the neighbour is still decoding
        got_c = c.wait(60)
        still = not nb.done
        nb.wait(120)
    finally:
        e.stop_loop()
    assert got_c == plain[0]
    assert still  # the default request ran beside the neighbour, behind the bad-words pass


@pytest.mark.parametrize("world,dp,chunk", [(3, 1, 5), (4, 2, 0)])
def test_rank_process_stages_get_the_entries_and_the_prompts_that_ask(tmp_path, world, dp, chunk, plain):
    """One process per stage over gloo (rank-process `dist` mode): the plan
    wire carries the entries, and the prompt ids of the groups that ask reach
    the last stage's process -- the tokens of the in-process engine."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prompts = [PROMPT, [4, 4, 4], [9, 8, 7, 6, 9, 8], PROMPT[:7]]
    kws = [dict(greedy=True, bad_words=_words(plain[0])), dict(greedy=True),
           dict(bad_words=[[6, 9], [3]], no_repeat_ngram_size=1, **SEEDED), dict(bad_words=[[t] for t in range(40)], **SEEDED)]
    want = _eng(max_batch=8).generate_ids(prompts, [SamplingParams(max_new_tokens=8, **kw) for kw in kws])
    assert want[0] != plain[0][:8]
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


# ---------------------------------------------------------------------------
# interfaces

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
    cl.generate_text("Hi, ", bad_words=["ab"], bad_words_ids=[[5, 6]])
    assert sent["bad_words"] == ["ab"] and sent["bad_words_ids"] == [[5, 6]]
    sent.clear()
    cl.generate_text("Hi, ")
    assert "bad_words" not in sent and "bad_words_ids" not in sent
    monkeypatch.undo()
    cfg = EngineConfig(model_id="gpt2-test", max_batch=4, device="cpu", role="coordinator")
    llm = LLM(cfg)
    tok = llm.tokenizer
    text = "abcabcabcabc"
    ids = tok.encode(text)
    plain_out = llm.engine.generate_ids([ids], [SamplingParams(greedy=True, max_new_tokens=8)])[0]
    words = [[ids[-1], plain_out[0]], list(plain_out[1:3])]
    want = llm.engine.generate_ids([ids], [SamplingParams(greedy=True, max_new_tokens=8, bad_words=words)])[0]
    assert want != plain_out and _never_completed(ids, want, words)
    dec = {"generated": tok.decode(ids + want, skip_special_tokens=True)}
    assert llm.generate_text(text, max_new_tokens=8, greedy=True, bad_words=words) == dec
    client = TestClient(create_app(cfg, engine=llm.engine))
    body = {"prompt": text, "max_new_tokens": 8, "greedy": True}
    assert client.post("/generate", json=body).json() == {
        "generated": tok.decode(ids + plain_out, skip_special_tokens=True)}
    r = client.post("/generate", json={**body, "bad_words_ids": words})
    assert r.status_code == 200 and r.json() == dec
    # strings: each tokenised as given and, when that differs, with a leading space
    word = "c"
    forms = [tok.encode(word)] + ([tok.encode(" " + word)] if tok.encode(" " + word) != tok.encode(word) else [])
    want_s = llm.engine.generate_ids([ids], [SamplingParams(greedy=True, max_new_tokens=8, bad_words=forms + words)])[0]
    r = client.post("/generate", json={**body, "bad_words": [word], "bad_words_ids": words})
    assert r.status_code == 200
    assert r.json() == {"generated": tok.decode(ids + want_s, skip_special_tokens=True)}
    Vm = llm.engine.mcfg.vocab_size
    for bad in (dict(bad_words_ids=[[]]), dict(bad_words_ids=[[Vm]]), dict(bad_words_ids=[[-1]]),
                dict(bad_words_ids=[[1.5]]), dict(bad_words_ids=[["x"]]), dict(bad_words_ids="12"),
                dict(bad_words_ids=[list(range(33))]), dict(bad_words_ids=[[i] for i in range(65)]),
                dict(bad_words=[""]), dict(bad_words="ab"), dict(bad_words=[5])):
        assert client.post("/generate", json={**body, **bad}).status_code == 422, bad
    props = client.get("/openapi.json").json()["components"]["schemas"]["GenerateReq"]["properties"]
    assert "bad_words" in props and "bad_words_ids" in props


def test_http_relay_bans_on_the_host(monkeypatch):
    """The compat relay applies ref.bad_words over prompt + output ahead of ref.logit_edits."""
    import requests

    from llm_sharding_demo_amd.serving.server import http_generate

    cfg = EngineConfig(model_id="gpt2-test", device="cpu")
    Vm = cfg.model.vocab_size
    logits = torch.linspace(0, 1, Vm).tolist()  # the argmax is V - 1, then V - 2, ...

    class R:
        def __init__(self, body):
            self.body = body

        def raise_for_status(self):
            pass

        def json(self):
            return self.body

    def post(url, json=None, timeout=None):
        return R({"hidden_states": [[[0.0]]]} if "hidden_states" not in json else {"logits": [[logits]]})

    monkeypatch.setattr(requests, "post", post)
    assert http_generate(cfg, [1], SamplingParams(greedy=True, max_new_tokens=3)) == [Vm - 1] * 3
    # V - 1 may not follow the prompt's 1, nor itself; V - 2 may not follow V - 1, V - 2
    sp = SamplingParams(greedy=True, max_new_tokens=5, bad_words=[[1, Vm - 1], [Vm - 1, Vm - 1], [Vm - 1, Vm - 2, Vm - 2]])
    assert http_generate(cfg, [1], sp) == [Vm - 2, Vm - 1, Vm - 2, Vm - 1, Vm - 2]
    sp = SamplingParams(greedy=True, max_new_tokens=3, bad_words=[[Vm - 1]], banned_token_ids=[Vm - 2])
    assert http_generate(cfg, [1], sp) == [Vm - 3] * 3
