"""Per-request guided decoding on an MI355X: guide_mask_kernel and
guide_advance_kernel (csrc/kernels/guide.hip) against the host references
(ops/reference.py guide_mask / guide_advance), the sampler behind the mask, the
wrappers' refusals, and the engine path around the on-device sampler.

The mask is a pure select -- a logit keeps its bits or becomes -inf -- and the
step copies one table cell, so logits, segment maxima and states are compared
bit for bit: no tolerance, no skipped rows.
"""
import dataclasses
import re

import numpy as np
import pytest
import torch

from llm_sharding_demo_amd import compile_regex
from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.runtime.batch import counter_uniform
from llm_sharding_demo_amd.runtime.engine import Engine
from llm_sharding_demo_amd.utils.tokenizer import ByteTokenizer

from .guide_cases import B, SLOTS, UNTOUCHED, counting_guide, mask_case, table_of
from .test_repetition_gpu import _RefTailCtx

pytestmark = pytest.mark.gpu

DEV = "cuda"
INF = float("inf")
SHAPES = [(50257, 50304), (128256, 128256), (1000, 1024), (4099, 4104)]


@pytest.fixture(scope="module")
def C():
    from llm_sharding_demo_amd.ops.hip import _load

    return _load()


def _segmax(logits):
    """What linear_f32 writes beside these logits (padding columns included)."""
    n, Vp = logits.shape
    return logits.view(n, Vp // 8, 8).amax(-1).contiguous()


def _i32(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    return all(torch.equal(x.cpu(), y) for x, y in zip(a, b))


def _run(C, c, seg):
    """(reference logits, reference segmax, kernel logits, kernel segmax, segmax before)."""
    want = c["lg"].clone()
    sm0 = _segmax(c["lg"]) if seg else None
    wsm = sm0.clone() if seg else None
    ref.guide_mask(want, c["tab"], c["slots"], c["V"], wsm)
    lg = c["lg"].to(DEV)
    tab = tuple(t.to(DEV) for t in c["tab"])
    dsm = sm0.to(DEV) if seg else None
    C.guide_mask(lg, c["V"], *tab, c["slots"].to(DEV), dsm)
    torch.cuda.synchronize()
    assert _same(tab, c["tab"])  # the tables are read only
    return want, wsm, lg.cpu(), dsm.cpu() if seg else None, sm0


@pytest.mark.parametrize("V,Vp,seg", [(50257, 50304, True), (50257, 50304, False), (128256, 128256, True),
                                      (128256, 128256, False), (1000, 1024, True), (1000, 1024, False),
                                      (4099, 4104, True), (4099, 4104, False)])
def test_guide_mask_bit_equal(C, V, Vp, seg):
    c = mask_case(V, Vp)
    want, wsm, got, gsm, sm0 = _run(C, c, seg)
    lg0 = c["lg"]
    assert torch.equal(_i32(got), _i32(want))
    # the case does what it says
    for r in UNTOUCHED:  # off, scratch and out-of-range slots; everything drawable; a state at S
        assert torch.equal(_i32(got[r]), _i32(lg0[r]))
    assert torch.equal(_i32(got[:, V:]), _i32(lg0[:, V:]))  # padding columns, whatever their classes
    for r, keep in c["keep"].items():
        assert bool((got[r, :V][~keep] == -INF).all())
        assert torch.equal(_i32(got[r, :V][keep]), _i32(lg0[r, :V][keep]))
    assert int((got[3, :V] > -INF).sum()) == 1 and got[3, c["one"]] == lg0[3, c["one"]] and c["one"] != int(c["am"][3])
    assert int((got[5, :V] > -INF).sum()) == (V + 1) // 2 and int((got[6, :V] > -INF).sum()) == 8
    assert int((got[7, :V] > -INF).sum()) == 2 and V // 4 < int((got[8, :V] > -INF).sum()) < 3 * V // 4
    assert torch.equal(got[11, :V] > -INF, got[7, :V] > -INF)  # two rows on one slot: the same state
    if not seg:
        return
    assert torch.equal(_i32(gsm), _i32(wsm))
    assert torch.equal(_i32(gsm), _i32(_segmax(got)))  # every segment, touched or not, padding included
    for r in UNTOUCHED:
        assert torch.equal(_i32(gsm[r]), _i32(sm0[r]))
    s = c["seg"]
    # row 6: its one segment keeps its maximum; every other segment that lies below V falls to -inf
    assert gsm[6, s] == sm0[6, s] and int((gsm[6] > -INF).sum()) == 1 + Vp // 8 - V // 8


def test_guide_mask_unaligned_rows(C):
    """Logits and class rows that do not start on 16 bytes (V = width = 4099,
    no segment maxima): the dword walk, the same bits."""
    c = mask_case(4099, 4104)
    V = c["V"]
    lg0 = c["lg"][:, :V].contiguous()
    tab = (c["tab"][0][:, :V].contiguous(),) + c["tab"][1:]
    want = ref.guide_mask(lg0.clone(), tab, c["slots"], V)
    lg = lg0.to(DEV)
    C.guide_mask(lg, V, *(t.to(DEV) for t in tab), c["slots"].to(DEV), None)
    torch.cuda.synchronize()
    assert torch.equal(_i32(lg), _i32(want)) and not torch.equal(_i32(want), _i32(lg0))
    # aligned logits over unaligned class rows, and the other way round
    for width, cols in ((4104, 4107), (V, 4104)):
        lg0 = c["lg"][:, :width].contiguous()
        gcls = torch.zeros(c["tab"][0].shape[0], cols, dtype=torch.int16)
        gcls[:, :4104] = c["tab"][0]
        tab = (gcls,) + c["tab"][1:]
        want = ref.guide_mask(lg0.clone(), tab, c["slots"], V)
        lg = lg0.to(DEV)
        C.guide_mask(lg, V, *(t.to(DEV) for t in tab), c["slots"].to(DEV), None)
        torch.cuda.synchronize()
        assert torch.equal(_i32(lg), _i32(want))


def test_guide_advance_bit_equal(C):
    """Inactive rows, off slots, out-of-range slots, a state at S and tokens at
    or past V change nothing; every other row's slot takes the table's cell."""
    c = mask_case(1000, 1024)
    V, keep = c["V"], c["keep"]
    g = torch.Generator().manual_seed(5)
    slots = c["slots"].clone()
    tokens = torch.randint(0, V, (B,), generator=g).to(torch.int32)
    for r in (3, 6, 7, 8):  # a drawable token of the row's state
        tokens[r] = int(keep[r].nonzero()[int(torch.randint(0, int(keep[r].sum()), (1,), generator=g))])
    tokens[4] = V                                     # at V: a padding column has a class too
    tokens[5] = int((~keep[5]).nonzero()[3])          # a token the state forbids: the guide dies
    active = torch.ones(B, dtype=torch.int32)
    active[11] = 0                                    # the second row on slot 9: each row owns its slot
    active[6] = 0
    for act in (active, None):
        if act is None:
            slots[11] = -1
        tab = tuple(t.clone() for t in c["tab"])
        ref.guide_advance(tab, slots, tokens, V, act)
        dtab = tuple(t.to(DEV) for t in c["tab"])
        C.guide_advance(*dtab, V, slots.to(DEV), tokens.to(DEV), None if act is None else act.to(DEV))
        torch.cuda.synchronize()
        assert _same(dtab, tab) and _same(dtab[:3], c["tab"][:3])
        new, old = tab[3], c["tab"][3]
        changed = sorted(int(s) for s in (new != old).any(dim=1).nonzero().flatten())
        assert set(changed) <= ({7, 12, 9, 1} | ({5} if act is None else set())) and int(new[12, 1]) == -1
        assert torch.equal(new[:, 0], old[:, 0])      # the guide rows of the slots never change
        assert torch.equal(new[0], old[0]) and torch.equal(new[4], old[4])  # token at V; state at S
        if act is not None:
            assert torch.equal(new[5], old[5])        # inactive


def test_mask_sample_advance_chain(C):
    """Six steps of mask -> sample -> advance on four guided rows and two
    default ones (a compiled regex, V = 1000): tokens and states equal the
    reference chain step for step."""
    V, Vp, n = 1000, 1024, 6
    tb = ByteTokenizer(gpt2_ids=False, eos_id=2).token_bytes(V)
    pattern = r"(ab|cd+e)*f[0-9]{2}"
    gd = compile_regex(pattern, tb, 2)
    tab = table_of([counting_guide(V)[0], gd], Vp, SLOTS, cells=gd.S * gd.C + 17)
    slots = torch.tensor([4, 9, SLOTS - 1, 0, 11, 16], dtype=torch.int32)
    for s in (4, 9, 0, 11):
        tab[3][s] = torch.tensor([1, 0], dtype=torch.int32)
    g = torch.Generator().manual_seed(11)
    greedy = torch.tensor([1, 0, 0, 0, 1, 0], dtype=torch.int32)
    temp, topk = torch.full((n,), 1.5), torch.full((n,), 40, dtype=torch.int32)
    seeds = torch.arange(7, 7 + n, dtype=torch.int64)
    dtab = tuple(t.to(DEV) for t in tab)
    outs = []
    for step in range(6):
        lg0 = torch.randn(n, Vp, generator=g) * 3
        st = torch.full((n,), step, dtype=torch.int64)
        want = ref.guide_mask(lg0.clone(), tab, slots, V)
        ids = ref.sample(want, temp, topk, greedy, counter_uniform(seeds, st), V, torch.ones(n), torch.zeros(n))
        ref.guide_advance(tab, slots, ids.to(torch.int32), V)
        lg, sm = lg0.to(DEV), _segmax(lg0).to(DEV)
        C.guide_mask(lg, V, *dtab, slots.to(DEV), sm)
        got = C.sample(lg, V, temp.to(DEV), topk.to(DEV), greedy.to(DEV), seeds.to(DEV), st.to(DEV), sm, None, None)
        C.guide_advance(*dtab, V, slots.to(DEV), got, None)
        torch.cuda.synchronize()
        assert torch.equal(_i32(lg), _i32(want)) and got.cpu().tolist() == ids.tolist()
        assert _same(dtab, tab), step
        outs.append(ids.tolist())
    for r in (0, 1, 3, 4):  # the guided rows walked the guide: never dead, a prefix of a match
        toks = [o[r] for o in outs]
        assert gd.walk(toks) == int(tab[3][int(slots[r]), 1]) >= 0
    assert len({tuple(o[r] for o in outs) for r in (0, 1, 3, 4)}) > 1


@pytest.mark.parametrize("V,Vp", SHAPES[:3])
@pytest.mark.parametrize("mode", ["top_k", "greedy", "top_p"])
def test_sampler_draws_from_the_masked_logits(C, V, Vp, mode):
    """Behind the mask the sampler draws what ref.sample draws from the
    reference-masked logits, with 1, 2 and 5 drawable tokens under top_k = 40
    (more candidates than drawable tokens), greedy and top_p = 0.9; every draw
    is a drawable token."""
    g = torch.Generator().manual_seed(V + 1)
    lg0 = torch.randn(B, Vp, generator=g) * 3
    gd, lists = counting_guide(V, (1, 2, 5), seed=V)
    tab = table_of([gd], Vp, SLOTS)
    slots = torch.randperm(SLOTS, generator=g)[:B].to(torch.int32)
    states = [0, 1, 2] * 4
    for s, st in zip(slots.tolist(), states):
        tab[3][s] = torch.tensor([0, st], dtype=torch.int32)
    greedy = torch.full((B,), int(mode == "greedy"), dtype=torch.int32)
    temp = torch.tensor([0.7, 1.0, 1.3, 0.9, 1.0, 0.6, 1.0, 0.6, 1.1, 1.0, 0.8, 1.0])
    topk = torch.full((B,), 40, dtype=torch.int32)
    topp = torch.full((B,), 0.9 if mode == "top_p" else 1.0)
    minp = torch.zeros(B)
    seeds = torch.arange(100, 100 + B, dtype=torch.int64)
    step = torch.arange(B, dtype=torch.int64)
    want = ref.guide_mask(lg0.clone(), tab, slots, V)
    ids = ref.sample(want, temp, topk, greedy, counter_uniform(seeds, step), V, topp, minp)
    assert all(int(t) in lists[st] for t, st in zip(ids, states))
    lg = lg0.to(DEV)
    sm = _segmax(lg0).to(DEV)
    C.guide_mask(lg, V, *(t.to(DEV) for t in tab), slots.to(DEV), sm)
    cut = (topp.to(DEV), minp.to(DEV)) if mode == "top_p" else (None, None)
    got = C.sample(lg, V, temp.to(DEV), topk.to(DEV), greedy.to(DEV), seeds.to(DEV), step.to(DEV), sm, *cut)
    torch.cuda.synchronize()
    assert got.cpu().tolist() == ids.tolist()


def test_wrapper_refusals(C):
    """Every invalid-argument case is an error and launches nothing: the logits
    and the states handed in keep their bits although every row is guided by
    a guide that allows nothing."""
    i32, i16 = torch.int32, torch.int16
    lg = torch.randn(2, 64, device=DEV)
    keep = lg.clone()

    def tab(Vp=64, nslots=2, rows=1):
        gsl = torch.zeros(nslots, 2, dtype=i32, device=DEV)
        return (torch.zeros(rows, Vp, dtype=i16, device=DEV), torch.full((rows, 4), -1, dtype=i16, device=DEV),
                torch.tensor([[1, 1]] * rows, dtype=i32, device=DEV).reshape(rows, 2), gsl)

    def call(V=64, seg=None, logits=lg, **kw):
        C.guide_mask(logits, V, *tab(**kw), torch.zeros(logits.shape[0], dtype=i32, device=DEV), seg)

    with pytest.raises(RuntimeError):
        call(V=65)                                           # V > ld
    with pytest.raises(RuntimeError):
        call(Vp=56)                                          # Vp < ld
    with pytest.raises(RuntimeError):
        call(nslots=0)                                       # nslots <= 0
    with pytest.raises(RuntimeError):
        call(rows=0)                                         # G <= 0
    lg60 = torch.randn(2, 60, device=DEV)
    keep60 = lg60.clone()
    with pytest.raises(RuntimeError):
        call(V=60, seg=torch.zeros(2, 8, device=DEV), logits=lg60)   # segment maxima: ld % 8 != 0
    with pytest.raises(RuntimeError):
        call(seg=torch.zeros(2, 7, device=DEV))              # ldseg * 8 < ld
    torch.cuda.synchronize()
    assert torch.equal(lg, keep) and torch.equal(lg60, keep60)
    zero = torch.zeros(2, dtype=i32, device=DEV)
    for kw, V in ((dict(nslots=0), 64), (dict(rows=0), 64), (dict(Vp=56), 64)):
        t = tab(**kw)
        t[1].fill_(0)  # would step to state 0
        t[3].fill_(0)
        t[3][:, 1] = 0
        before = t[3].clone()
        with pytest.raises(RuntimeError):
            C.guide_advance(*t, V, zero, zero, None)         # nslots <= 0; G <= 0; V > Vp
        torch.cuda.synchronize()
        assert torch.equal(t[3], before)
    sm = torch.zeros(2, 8, device=DEV)
    call(seg=sm)                                             # the valid call does run
    torch.cuda.synchronize()
    assert bool((lg == -INF).all()) and bool((sm == -INF).all())


# ---------------------------------------------------------------------------
# engine (HIP backend, native executor, 2 microbatches)

class _RefTailGuide(_RefTailCtx):
    """_RefTailCtx with the two guide passes on the host too."""

    def guide_mask(self, logits, table, slots, vocab):
        c = self._c
        logits.copy_(ref.guide_mask(c(logits), tuple(map(c, table)), c(slots), vocab))

    def guide_advance(self, table, slots, tokens, vocab, active=None):
        c = self._c
        h = tuple(map(c, table))
        ref.guide_advance(h, c(slots), c(tokens), vocab, c(active))
        table[3].copy_(h[3])


PROMPTS = [[1, 2, 3, 4], [5, 6], list(range(10, 50)), [7] * 9, [3, 3], list(range(10, 50))]
N = 24
OTHERS = [SamplingParams(temperature=0.8, top_k=20, seed=11 + i, max_new_tokens=n) for i, n in enumerate((3, 6, 1, 5))]
PLAIN_G = SamplingParams(greedy=True, max_new_tokens=N)
PLAIN_S = SamplingParams(temperature=1.0, top_k=40, seed=5, max_new_tokens=N)


def _engine(graphs=True, model="gpt2-test", ref_tail=False, **kw):
    cfg = EngineConfig(model_id=model, num_stages=1, max_batch=16, device="cuda", use_graphs=graphs,
                       max_seq_len=512, num_microbatches=2, **kw)
    e = Engine(cfg, devices=["cuda:0"])
    assert e.stages[0].backend.name == "hip"
    if ref_tail:
        e.stages[0].backend = _RefTailGuide(e.stages[0].backend)
    return e


def _launches(e):
    return sum(w.draw.guide_launches for w in e.workers)


def test_engine_guided_requests_in_a_changing_batch(monkeypatch):
    """A greedy and a seeded guided request (gpt2-test has no EOS in its
    vocabulary: a pattern whose accepting states go on) draw the same ids alone
    and among default-parameter neighbours that leave at different steps, with
    decode graphs on (first run and replayed) and off; every output is a prefix
    of a match; the neighbours draw what they draw without them; the tokens are
    the reference tail's."""
    monkeypatch.setenv("LSD_NATIVE_EXEC", "1")
    e = _engine()
    plain = e.generate_ids([PROMPTS[2]], [PLAIN_G])[0]
    plain_s = e.generate_ids([PROMPTS[5]], [PLAIN_S])[0]
    without = e.generate_ids(PROMPTS[:2] + PROMPTS[3:5], OTHERS)
    default = [OTHERS[0], OTHERS[1], PLAIN_G, OTHERS[2], OTHERS[3], PLAIN_S]
    assert e.generate_ids(PROMPTS, default)[5] == plain_s  # precondition: comparable across compositions
    assert _launches(e) == 0 and all(w.draw.guide_tab is None for w in e.workers)  # an all-default session
    V = e.mcfg.vocab_size
    tb = ByteTokenizer(gpt2_ids=True).token_bytes(V)
    pattern = r"(ab|c[0-9]+;)+"
    prefix = re.compile(rb"(ab|c[0-9]+;)*(a|c[0-9]*)?")
    gd = compile_regex(pattern, tb, None)
    text = lambda out: b"".join(tb[t] for t in out)  # noqa: E731
    ask_g = dataclasses.replace(PLAIN_G, guide=gd)
    ask_s = dataclasses.replace(PLAIN_S, temperature=1.5, guide=compile_regex(pattern, tb, None))  # an equal guide: one row
    alone_g = e.generate_ids([PROMPTS[2]], [ask_g])[0]
    alone_s = e.generate_ids([PROMPTS[5]], [ask_s])[0]
    assert _launches(e) > 0 and sum(d is not None for d in e.guides.digest) == 1
    assert len(alone_g) == N and len(alone_s) == N and alone_g != plain
    assert prefix.fullmatch(text(alone_g)) and prefix.fullmatch(text(alone_s)) and alone_g != alone_s
    sps = [OTHERS[0], OTHERS[1], ask_g, OTHERS[2], OTHERS[3], ask_s]
    got = e.generate_ids(PROMPTS, sps)
    assert got[2] == alone_g and got[5] == alone_s
    assert got[:2] + got[3:5] == without  # asking never changes another request's draws
    assert e.generate_ids(PROMPTS, sps) == got  # graphs cached: native steps
    assert sum(w.native_steps for w in e.workers) > 0
    assert sum(w.native_changes for w in e.workers) > 0
    assert _engine(graphs=False).generate_ids(PROMPTS, sps) == got
    tail = _engine(graphs=False, ref_tail=True).generate_ids(PROMPTS, sps)
    assert tail[2] == alone_g and tail[5] == alone_s
    # a request that takes over a guided slot inherits nothing
    assert e.generate_ids([PROMPTS[2]], [PLAIN_G])[0] == plain
    assert e.generate_ids(PROMPTS, default)[5] == plain_s
    assert e.guides.pins == [0] * 8 and e.scheduler._guided == 0


def test_engine_guide_with_penalties_and_logprobs_match_the_reference():
    """llama-test (its EOS, 2, is in the vocabulary): guided requests that
    combine the guide with penalties, repetition_penalty, a logit_bias and
    logprobs beside default neighbours -- the tokens of the reference tail on
    the same logits, and its records (ids and -inf entries exactly; finite
    logprobs to the logprob kernel's documented 5.2e-6).  Every guided output
    matches its pattern as a whole; a forbidden token's logprob is -inf."""
    eos = 2
    tb = ByteTokenizer(gpt2_ids=False, eos_id=eos).token_bytes(1000)
    pat_a, pat_b = r"(yes|no|maybe)-[0-9]{2,3}", r'\{"k": "[a-z]{1,6}"\}'
    ga, gb = compile_regex(pat_a, tb, eos), compile_regex(pat_b, tb, eos)
    sps = [SamplingParams(greedy=True, max_new_tokens=N, stop_at_eos=True, guide=ga, logprobs=3),
           OTHERS[0],
           SamplingParams(greedy=True, max_new_tokens=N, stop_at_eos=True, presence_penalty=2.0, frequency_penalty=2.0,
                          repetition_penalty=1.3, guide=gb, logprobs=5),
           SamplingParams(temperature=1.0, top_k=40, top_p=0.9, seed=5, max_new_tokens=N, stop_at_eos=True,
                          presence_penalty=1.5, frequency_penalty=0.7, logit_bias={ord("m"): 3.0}, guide=ga, logprobs=5),
           OTHERS[1],
           SamplingParams(temperature=0.9, top_k=30, seed=8, max_new_tokens=N, repetition_penalty=0.8, guide=gb)]
    e = _engine(model="llama-test")
    r = _engine(model="llama-test", graphs=False, ref_tail=True)
    assert isinstance(r.stages[0].backend, _RefTailGuide)
    want = r.generate_requests(PROMPTS, sps)
    for _ in range(3):  # eager first use, capture, replay
        got = e.generate_requests(PROMPTS, sps)
        assert [g.output for g in got] == [w.output for w in want]
        for g, w in zip(got, want):
            if w.logprobs is None:
                assert g.logprobs is None
                continue
            assert g.logprobs.tokens == w.logprobs.tokens
            for ga_, wa in zip(g.logprobs.top_logprobs, w.logprobs.top_logprobs):
                assert [i for i, _ in ga_] == [i for i, _ in wa]
            flat = lambda lp: lp.token_logprobs + [v for alts in lp.top_logprobs for _, v in alts]  # noqa: E731
            for a, b in zip(flat(g.logprobs), flat(w.logprobs)):
                assert a == b if b == -INF else abs(a - b) <= 5.2e-6
    for i, pat in ((0, pat_a), (2, pat_b), (3, pat_a)):
        out = want[i].output
        assert out[-1] == eos and re.fullmatch(pat.encode(), bytes(out[:-1])) and want[i].finish_reason == "eos"
    out = want[5].output  # no stop_at_eos: only EOS follows the match
    k = out.index(eos)
    assert set(out[k:]) == {eos} and re.fullmatch(pat_b.encode(), bytes(out[:k]))
    # the first draw of the first request has three drawable tokens: the rest of the alternatives are -inf,
    # and the log-sum-exp runs over what is left
    alts = want[3].logprobs.top_logprobs[0]
    assert sorted(i for i, _ in alts[:3]) == sorted(b"ynm") and [v for _, v in alts[3:]] == [-INF, -INF]
    assert abs(sum(np.exp(v) for _, v in alts[:3]) - 1.0) < 1e-5
    assert _launches(e) > 0 and sum(w.draw.penalty_launches for w in e.workers) > 0
    assert sum(w.draw.repetition_launches for w in e.workers) > 0 and sum(w.native_steps for w in e.workers) > 0
    assert e.guides.pins == [0] * 8 and sum(d is not None for d in e.guides.digest) == 2
