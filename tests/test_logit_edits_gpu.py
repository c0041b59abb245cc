"""Per-request logit edits on an MI355X: logit_edit_kernel
(csrc/kernels/logit_edit.hip) against the host reference (ops/reference.py
logit_edits), the sampler behind it, and the engine path around the on-device
sampler.

The kernel adds in fp32 with one rounding per addition, a run of entries on
one token in one thread, so logits and segment maxima are compared bit for
bit: no tolerance, no skipped rows.
"""
import dataclasses

import numpy as np
import pytest
import torch

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.runtime.batch import counter_uniform
from llm_sharding_demo_amd.runtime.engine import Engine

pytestmark = pytest.mark.gpu

DEV = "cuda"
SLOTS, SCRATCH = 16, 15
I32MAX = 2 ** 31 - 1
INF = float("inf")
M = 5  # the `until` of the rows that sit on its boundary


@pytest.fixture(scope="module")
def C():
    from llm_sharding_demo_amd.ops.hip import _load

    return _load()


def _segmax(logits):
    """What linear_f32 writes beside these logits (padding columns included)."""
    B, Vp = logits.shape
    return logits.view(B, Vp // 8, 8).amax(-1).contiguous()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _entries(g, V, n, dup):
    """n random entries sorted by token (dup: drawn with replacement, so runs
    of equal tokens occur): values in [-100, 100], a tenth of them bans, a
    third with an `until` among the counters the rows use."""
    tok = (torch.randint(0, V, (n,), generator=g) if dup else torch.randperm(V, generator=g)[:n]).sort().values
    val = torch.rand(n, generator=g) * 200 - 100
    val[torch.rand(n, generator=g) < 0.1] = -INF
    until = torch.full((n,), I32MAX, dtype=torch.int32)
    some = torch.rand(n, generator=g) < 0.33
    until[some] = torch.randint(0, 11, (int(some.sum()),), generator=g, dtype=torch.int32)
    return tok.to(torch.int32), val, until


def _case(V, Vp, E=1024):
    """CPU tensors of a 12-row case on 16 slots.  The table is full of valid
    entries everywhere (other slots, entries past each count), so reading
    anything but the row's own [0, count) changes the result."""
    g = torch.Generator().manual_seed(V + E)
    B = 12
    lg = torch.randn(B, Vp, generator=g) * 3
    cnt = torch.zeros(SLOTS, dtype=torch.int32)
    tok = torch.randint(0, V, (SLOTS, E), generator=g, dtype=torch.int32)
    val = torch.full((SLOTS, E), 50.0)
    until = torch.full((SLOTS, E), I32MAX, dtype=torch.int32)

    def put(slot, ent):
        cnt[slot] = len(ent[0])
        for dst, src in zip((tok, val, until), ent):
            dst[slot, : len(ent[0])] = torch.as_tensor(src, dtype=dst.dtype)

    slots = torch.tensor([3, 7, 0, 12, 5, 9, 1, 1, 14, SCRATCH, 11, 6], dtype=torch.int32)
    step = torch.tensor([4, 0, 3, 7, 2, 9, M - 1, M, M + 1, 0, 6, 1], dtype=torch.int64)
    am = lg[:, :V].argmax(dim=1)
    put(7, ([int(am[1])], [-INF], [I32MAX]))                       # row 1: the argmax banned, 1 entry
    put(0, _entries(g, V, 300, dup=False))                          # row 2: 300 distinct tokens
    put(12, _entries(g, V, E, dup=True))                            # row 3: a full table row, with runs
    put(5, ([0, 808, 811, V - 1], [1.5, -2.25, 0.75, -INF], [I32MAX] * 4))  # row 4: both ends; one segment twice
    seg5 = 77  # row 5: a bias lifts the segment's smallest logit above its maximum
    lg[5, seg5 * 8: seg5 * 8 + 8] = lg[5, seg5 * 8: seg5 * 8 + 8].clamp(-5, 5)
    tok5 = seg5 * 8 + int(lg[5, seg5 * 8: seg5 * 8 + 8].argmin())
    put(9, ([tok5], [100.0], [I32MAX]))
    t6 = int(am[6])  # rows 6, 7 (slot 1): a run of two on one token, counters either side of M
    put(1, ([t6, t6, 321], [2.0, -INF, -1.0], [I32MAX, M, M]))
    put(14, ([int(am[8]), 17], [-INF, 3.0], [M, M]))                # row 8: counter M + 1: nothing active
    put(11, ([-1, 5, V, V + 7], [9.0, 0.5, 9.0, 9.0], [I32MAX] * 4))  # row 10: tokens outside [0, V) ignored
    top3 = lg[11, :V].topk(3).indices.sort().values.tolist()
    put(6, (top3, [-INF] * 3, [I32MAX, I32MAX, 2]))                 # row 11: its three best banned
    assert int(cnt[3]) == 0 and int(cnt[SCRATCH]) == 0              # rows 0 and 9: no entry
    return dict(lg=lg, tab=(cnt, tok, val, until), slots=slots, step=step, V=V, am=am, seg5=seg5, tok5=tok5, t6=t6)


def _run(C, c, seg, with_step=True):
    """(reference logits, reference segmax, kernel logits, kernel segmax, segmax before)."""
    want = c["lg"].clone()
    sm0 = _segmax(c["lg"]) if seg else None
    wsm = sm0.clone() if seg else None
    step = c["step"] if with_step else None
    ref.logit_edits(want, c["tab"], c["slots"], step, c["V"], wsm)
    lg = c["lg"].to(DEV)
    tab = tuple(t.to(DEV) for t in c["tab"])
    dsm = sm0.to(DEV) if seg else None
    C.logit_edits(lg, c["V"], *tab, c["slots"].to(DEV), step.to(DEV) if with_step else None, dsm)
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(tab, c["tab"]))  # the table is read only
    return want, wsm, lg.cpu(), dsm.cpu() if seg else None, sm0


@pytest.mark.parametrize("V,Vp,seg,E", [(50257, 50304, True, 1024), (50257, 50304, False, 1024),
                                        (1000, 1024, True, 1024), (128256, 128256, True, 1024),
                                        (50257, 50304, True, 300)])
def test_logit_edits_bit_equal(C, V, Vp, seg, E):
    c = _case(V, Vp, E)
    want, wsm, got, gsm, sm0 = _run(C, c, seg)
    lg0 = c["lg"]
    assert torch.equal(_bits(got), _bits(want))
    # the case does what it says: untouched rows, changed rows, padding columns
    for r in (0, 8, 9):  # count 0; nothing active at its counter; pad row on the scratch slot
        assert torch.equal(_bits(got[r]), _bits(lg0[r]))
    assert all(not torch.equal(_bits(got[r]), _bits(lg0[r])) for r in (1, 2, 3, 4, 5, 6, 7, 10, 11))
    assert torch.equal(_bits(got[:, V:]), _bits(lg0[:, V:]))
    assert got[1, c["am"][1]] == -INF
    assert got[4, 0] == lg0[4, 0] + np.float32(1.5) and got[4, V - 1] == -INF
    assert got[4, 808] == lg0[4, 808] - np.float32(2.25) and got[4, 811] == lg0[4, 811] + np.float32(0.75)
    assert got[6, c["t6"]] == -INF                                  # counter M - 1: bias and ban
    assert got[7, c["t6"]] == lg0[7, c["t6"]] + np.float32(2.0)     # counter M: the bias alone
    assert got[6, 321] == lg0[6, 321] - 1.0 and got[7, 321] == lg0[7, 321]
    assert int((_bits(got[10]) != _bits(lg0[10])).sum()) == 1 and got[10, 5] == lg0[10, 5] + np.float32(0.5)
    assert int((got[11] == -INF).sum()) == 3 and int((got[2] != lg0[2]).sum()) > 150
    if not seg:
        return
    assert torch.equal(_bits(gsm), _bits(wsm))
    assert torch.equal(_bits(gsm), _bits(_segmax(got)))  # every segment, touched or not, padding included
    a1 = int(c["am"][1])
    assert gsm[1, a1 // 8] < sm0[1, a1 // 8]                               # the argmax's segment fell
    assert gsm[5, c["seg5"]] == got[5, c["tok5"]] > sm0[5, c["seg5"]]      # lifted to the new maximum
    for r in (0, 8, 9):
        assert torch.equal(_bits(gsm[r]), _bits(sm0[r]))


def test_logit_edits_without_step_is_draw_0(C):
    c = _case(50257, 50304)
    want, wsm, got, gsm, _ = _run(C, c, True, with_step=False)
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(gsm), _bits(wsm))
    assert torch.equal(_bits(gsm), _bits(_segmax(got)))
    assert got[6, c["t6"]] == got[7, c["t6"]] == -INF and got[8, c["am"][8]] == -INF  # counter 0 < M everywhere
    c0 = dict(c, step=torch.zeros(12, dtype=torch.int64))
    assert torch.equal(_bits(_run(C, c0, True)[2]), _bits(got))


@pytest.mark.parametrize("V,Vp", [(50257, 50304), (128256, 128256), (1000, 1024)])
def test_sampler_draws_from_the_edited_logits(C, V, Vp):
    """The sampler's fast path trusts the segment maxima: behind the edit pass
    it draws what ref.sample draws from the reference-edited logits -- the row
    whose argmax was banned and the row whose new maximum a bias made among
    them (greedy, so a stale maximum changes the token)."""
    c = _case(V, Vp)
    B = 12
    want = c["lg"].clone()
    ref.logit_edits(want, c["tab"], c["slots"], c["step"], V)
    greedy = torch.tensor([0, 1, 0, 0, 0, 1, 1, 0, 0, 1, 0, 1], dtype=torch.int32)
    temp = torch.tensor([0.7, 1.0, 1.3, 0.9, 1.0, 1.0, 1.0, 0.6, 1.1, 1.0, 0.8, 1.0])
    topk = torch.tensor([40, 1, 64, 40, 5, 1, 1, 100, 40, 1, 17, 1], dtype=torch.int32)
    seeds = torch.arange(100, 100 + B, dtype=torch.int64)
    ids = ref.sample(want, temp, topk, greedy, counter_uniform(seeds, c["step"]), V)
    assert int(ids[5]) == c["tok5"] and int(ids[1]) != int(c["am"][1])
    assert int(ids[11]) not in c["lg"][11, :V].topk(3).indices.tolist()
    lg = c["lg"].to(DEV)
    sm = _segmax(c["lg"]).to(DEV)
    C.logit_edits(lg, V, *(t.to(DEV) for t in c["tab"]), c["slots"].to(DEV), c["step"].to(DEV), sm)
    got = C.sample(lg, V, temp.to(DEV), topk.to(DEV), greedy.to(DEV), seeds.to(DEV), c["step"].to(DEV), sm, None, None)
    torch.cuda.synchronize()
    assert got.cpu().tolist() == ids.tolist()


def test_wrapper_refusals(C):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    i32 = torch.int32

    def call(E, ld=64, seg=None, slots=2):
        C.logit_edits(z(1, ld), ld, z(slots, dt=i32), z(slots, E, dt=i32), z(slots, E), z(slots, E, dt=i32),
                      z(1, dt=i32), None, seg)

    call(1024)
    call(1, 60)
    with pytest.raises(RuntimeError, match="1024"):
        call(1025)
    with pytest.raises(RuntimeError, match="segmax"):  # segment maxima need rows of whole segments
        call(4, 60, z(1, 8))
    with pytest.raises(RuntimeError):
        C.logit_edits(z(1, 64), 64, z(3, dt=i32), z(2, 4, dt=i32), z(2, 4), z(2, 4, dt=i32), z(1, dt=i32), None, None)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# engine (HIP backend, native executor, 2 microbatches)

class _RefTail:
    """An engine's HIP backend with everything between the lm_head and the
    token ids -- penalties, edits, draw, history, logprob records -- done by
    ops/reference.py on host copies: what the reference backend computes from
    the same logits."""

    def __init__(self, hip):
        object.__setattr__(self, "_hip", hip)

    def __getattr__(self, name):
        return getattr(self._hip, name)

    def __setattr__(self, name, value):
        setattr(self._hip, name, value)

    @staticmethod
    def _c(t):
        return None if t is None else t.cpu()

    def _draw(self, logits, samp, vocab):
        c = self._c
        u = counter_uniform(samp.seeds.cpu(), samp.step.cpu())
        return ref.sample(logits.cpu(), c(samp.temperature), c(samp.top_k), c(samp.greedy), u, vocab,
                          c(samp.top_p), c(samp.min_p)).to(logits.device)

    def sample(self, logits, samp, vocab):
        return self._draw(logits, samp, vocab)

    def sample_into(self, logits, samp, vocab, out, meta=None):
        out.copy_(self._draw(logits, samp, vocab))
        samp.advance()
        if meta is not None:
            meta.advance()

    def penalize(self, logits, hist, slots, counts, presence, frequency, vocab):
        c = self._c
        logits.copy_(ref.penalize(c(logits), c(hist), c(slots), c(counts), c(presence), c(frequency), vocab))

    def logit_edits(self, logits, table, slots, step, vocab):
        c = self._c
        logits.copy_(ref.logit_edits(c(logits), tuple(map(c, table)), c(slots), c(step), vocab))

    def record_tokens(self, hist, slots, step, tokens, active=None, back=0):
        c = self._c
        h = c(hist)
        ref.record_tokens(h, c(slots), c(step), c(tokens), c(active), back)
        hist.copy_(h)

    def logprobs(self, logits, tokens, nlp, slots, step, active, rec, vocab, back=0):
        c = self._c
        h = [c(t) for t in rec]
        out = ref.logprobs(c(logits), c(tokens), c(nlp), vocab, rec[1].shape[2])
        ref.record_logprobs(h, c(slots), c(step), c(nlp), *out, c(active), back)
        for d, s in zip(rec, h):
            d.copy_(s)


# The requests compared alone and inside a batch take the 40-token prompt: a
# draw is only comparable between batch compositions while the prefill logits
# are (tests/test_penalties_gpu.py), which the test asserts for the plain
# seeded request first.
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
        e.stages[0].backend = _RefTail(e.stages[0].backend)
    return e


def test_engine_edited_requests_in_a_changing_batch(monkeypatch):
    """A greedy request with its first plain token banned and a seeded one
    with a ban, a bias and min_new_tokens draw the same ids alone and among
    default-parameter neighbours that leave at different steps, with decode
    graphs on (first run and replayed) and off; the neighbours draw what they
    draw without them; the greedy tokens are the reference backend's."""
    monkeypatch.setenv("LSD_NATIVE_EXEC", "1")
    e = _engine()
    plain = e.generate_ids([PROMPTS[2]], [PLAIN_G])[0]
    plain_s = e.generate_ids([PROMPTS[5]], [PLAIN_S])[0]
    without = e.generate_ids(PROMPTS[:2] + PROMPTS[3:5], OTHERS)
    default = [OTHERS[0], OTHERS[1], PLAIN_G, OTHERS[2], OTHERS[3], PLAIN_S]
    assert e.generate_ids(PROMPTS, default)[5] == plain_s  # precondition: comparable across compositions
    assert sum(w.draw.logit_edit_launches for w in e.workers) == 0 and e.workers[0].draw.edit_tab is None  # default traffic
    ed_g = dataclasses.replace(PLAIN_G, banned_token_ids=[plain[0]])
    ed_s = dataclasses.replace(PLAIN_S, banned_token_ids=[plain_s[1], plain_s[2]],
                               logit_bias={plain_s[0]: -5.0, 7: 1.0}, min_new_tokens=3)
    alone_g = e.generate_ids([PROMPTS[2]], [ed_g])[0]
    alone_s = e.generate_ids([PROMPTS[5]], [ed_s])[0]
    assert sum(w.draw.logit_edit_launches for w in e.workers) > 0
    assert len(alone_g) == N and len(alone_s) == N
    assert plain[0] not in alone_g and alone_g[0] != plain[0]  # the ban is live
    assert plain_s[1] not in alone_s and plain_s[2] not in alone_s and alone_s != plain_s
    sps = [OTHERS[0], OTHERS[1], ed_g, OTHERS[2], OTHERS[3], ed_s]
    got = e.generate_ids(PROMPTS, sps)
    assert got[2] == alone_g and got[5] == alone_s
    assert got[:2] + got[3:5] == without
    assert e.generate_ids(PROMPTS, sps) == got  # graphs cached: native steps
    assert sum(w.native_steps for w in e.workers) > 0
    assert sum(w.native_changes for w in e.workers) > 0
    assert _engine(graphs=False).generate_ids(PROMPTS, sps) == got
    assert _engine(graphs=False, ref_tail=True).generate_ids(PROMPTS, sps)[2] == alone_g
    # a bias of 100 wins every greedy draw
    assert e.generate_ids([PROMPTS[2]], [dataclasses.replace(PLAIN_G, logit_bias={"777": 100})])[0] == [777] * N


def test_engine_edits_with_penalties_and_logprobs_match_the_reference():
    """llama-test (its EOS, 2, is in the vocabulary): requests that combine
    edits with penalties and logprobs, min_new_tokens holding back an EOS that
    a bias of 100 would draw at once, beside default neighbours -- the tokens
    of the reference backend's sampler tail on the same logits, and its
    records (ids and -inf entries exactly; finite logprobs to the logprob
    kernel's documented 5.2e-6)."""
    eos = 2
    sps = [SamplingParams(greedy=True, max_new_tokens=12, logit_bias={eos: 100}, stop_at_eos=True, min_new_tokens=5,
                          logprobs=3),
           OTHERS[0],
           SamplingParams(greedy=True, max_new_tokens=N, presence_penalty=2.0, frequency_penalty=2.0,
                          banned_token_ids=list(range(100, 350)), logit_bias={t: -3.5 for t in range(400, 440)},
                          min_new_tokens=4, logprobs=5),
           SamplingParams(temperature=1.0, top_k=40, top_p=0.9, seed=5, max_new_tokens=N, presence_penalty=1.5,
                          frequency_penalty=0.7, banned_token_ids=list(range(1, 1000, 4)), logprobs=2),
           OTHERS[1],
           SamplingParams(temperature=0.9, top_k=30, seed=8, max_new_tokens=9, logit_bias={5: 4.0, 6: -4.0})]
    e = _engine(model="llama-test")
    r = _engine(model="llama-test", graphs=False, ref_tail=True)
    assert isinstance(r.stages[0].backend, _RefTail)
    want = r.generate_requests(PROMPTS, sps)
    for _ in range(3):  # eager first use, capture, replay
        got = e.generate_requests(PROMPTS, sps)
        assert [g.output for g in got] == [w.output for w in want]
        for g, w in zip(got, want):
            if w.logprobs is None:
                assert g.logprobs is None
                continue
            assert g.logprobs.tokens == w.logprobs.tokens
            for ga, wa in zip(g.logprobs.top_logprobs, w.logprobs.top_logprobs):
                assert [i for i, _ in ga] == [i for i, _ in wa]
            flat = lambda lp: lp.token_logprobs + [v for alts in lp.top_logprobs for _, v in alts]  # noqa: E731
            for a, b in zip(flat(g.logprobs), flat(w.logprobs)):
                assert a == b if b == -INF else abs(a - b) <= 5.2e-6
    out = want[0].output
    assert len(out) == 6 and eos not in out[:5] and out[5] == eos
    assert not set(want[2].output) & set(range(100, 350)) and all(t % 4 != 1 for t in want[3].output)
    assert sum(w.draw.logit_edit_launches for w in e.workers) > 0 and sum(w.draw.penalty_launches for w in e.workers) > 0
    assert sum(w.native_steps for w in e.workers) > 0
