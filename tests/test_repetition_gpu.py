"""Per-request repetition_penalty and no_repeat_ngram_size on an MI355X:
repeat_kernel and record_context_kernel (csrc/kernels/repeat.hip) against the
host reference (ops/reference.py repetition, record_context), the sampler
behind the pass, and the engine path with hipGraph decode.

The kernel rewrites every distinct context token once, in fp32 with one
rounding (an IEEE division or a product), and bans with -inf: logits and
segment maxima are compared bit for bit -- no tolerance, no skipped rows.
"""
import dataclasses

import pytest
import torch

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.runtime.batch import counter_uniform
from llm_sharding_demo_amd.runtime.engine import Engine

from . import repetition_cases as rc
from .test_logit_edits_gpu import _RefTail

pytestmark = pytest.mark.gpu

DEV = "cuda"
INF = float("inf")


@pytest.fixture(scope="module")
def C():
    from llm_sharding_demo_amd.ops.hip import _load

    return _load()


_CASES = {}


def _case(V, Vp):
    """The case and its reference results (computed once, never modified)."""
    if (V, Vp) not in _CASES:
        c = rc.case(V, Vp)
        for key, step in (("want", c["step"]), ("want0", None)):
            lg, sm = c["lg"].clone(), rc.segmax_of(c["lg"])
            ref.repetition(lg, c["tab"], c["slots"], step, V, sm)
            c[key] = (lg, sm)
        _CASES[(V, Vp)] = c
    return _CASES[(V, Vp)]


def _run(C, c, seg, with_step=True):
    """(kernel logits, kernel segmax or None) on host."""
    lg = c["lg"].to(DEV)
    tab = tuple(t.to(DEV) for t in c["tab"])
    dsm = rc.segmax_of(c["lg"]).to(DEV) if seg else None
    C.repetition(lg, c["V"], *tab, c["slots"].to(DEV), c["step"].to(DEV) if with_step else None, dsm)
    torch.cuda.synchronize()
    assert all(torch.equal(rc.bits(a), rc.bits(b)) for a, b in zip(tab, c["tab"]))  # the table is read only
    return lg.cpu(), dsm.cpu() if seg else None


@pytest.mark.parametrize("V,Vp,seg", [(50257, 50304, True), (50257, 50304, False), (1000, 1024, True),
                                      (128256, 128256, True)])
def test_repetition_bit_equal(C, V, Vp, seg):
    c = _case(V, Vp)
    want, wsm = c["want"]
    got, gsm = _run(C, c, seg)
    lg0 = c["lg"]
    assert torch.equal(rc.bits(got), rc.bits(want))
    # the case does what it says (tests/test_repetition.py checks the reference row by row)
    for r in (0, 1, 10, 11):  # knobs off; pad row on the scratch slot; n = G - 2; n = G - 1 over 0.0, -0.0, -inf
        assert torch.equal(rc.bits(got[r]), rc.bits(lg0[r]))
    assert all(not torch.equal(rc.bits(got[r]), rc.bits(lg0[r])) for r in (2, 3, 4, 5, 6, 7, 8, 9))
    assert torch.equal(rc.bits(got[:, V:]), rc.bits(lg0[:, V:]))
    am7 = int(c["am"][7])
    assert got[7, am7] == -INF and got[8, 33] == -INF and got[9, V - 1] == -INF
    assert int((got[6] == -INF).sum()) == len({t for t in c["ctx"][6] if 0 <= t < V})
    if not seg:
        return
    assert torch.equal(rc.bits(gsm), rc.bits(wsm))
    assert torch.equal(rc.bits(gsm), rc.bits(rc.segmax_of(got)))  # every segment, touched or not, padding included
    sm0 = rc.segmax_of(lg0)
    assert gsm[7, am7 // 8] < sm0[7, am7 // 8]                               # the argmax's segment fell
    assert gsm[5, c["seg5"]] == got[5, c["tok5"]] > sm0[5, c["seg5"]]        # lifted to the new maximum
    for r in (0, 1, 10, 11):
        assert torch.equal(rc.bits(gsm[r]), rc.bits(sm0[r]))


def test_repetition_without_step_is_draw_0(C):
    c = _case(50257, 50304)
    want, wsm = c["want0"]
    got, gsm = _run(C, c, True, with_step=False)
    assert torch.equal(rc.bits(got), rc.bits(want)) and torch.equal(rc.bits(gsm), rc.bits(wsm))
    assert torch.equal(rc.bits(gsm), rc.bits(rc.segmax_of(got)))
    assert not torch.equal(rc.bits(want), rc.bits(c["want"][0]))  # the prompts alone: another result
    c0 = dict(c, step=torch.zeros(12, dtype=torch.int64))
    assert torch.equal(rc.bits(_run(C, c0, True)[0]), rc.bits(got))


def test_repetition_largest_context(C):
    """L = n = 8192: the 64 KB key set plus the tail, over the default dynamic-LDS limit."""
    c = rc.big_case()
    want, wsm = c["lg"].clone(), rc.segmax_of(c["lg"])
    ref.repetition(want, c["tab"], c["slots"], c["step"], c["V"], wsm)
    got, gsm = _run(C, c, True)
    assert torch.equal(rc.bits(got), rc.bits(want)) and torch.equal(rc.bits(gsm), rc.bits(wsm))
    assert torch.equal(rc.bits(gsm), rc.bits(rc.segmax_of(got)))
    assert torch.equal(rc.bits(got[1]), rc.bits(c["lg"][1]))
    assert got[0, int(c["lg"][0, :c["V"]].argmax())] == -INF
    assert int((rc.bits(got[0]) != rc.bits(c["lg"][0])).sum()) > 7000


@pytest.mark.parametrize("back", [0, 1])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("with_step", [True, False])
def test_record_context_equals_reference(C, back, masked, with_step):
    from .test_repetition import _record_case

    tab, slots, step, tokens, active = _record_case()
    active, step = (active if masked else None), (step if with_step else None)
    d = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    tok, plen = tab[3].to(DEV), tab[0].to(DEV)
    C.record_context(tok, plen, d(slots), d(step), d(tokens), d(active), back)
    torch.cuda.synchronize()
    before = tab[3].clone()
    ref.record_context(tab, slots, step, tokens, active, back)
    assert tok.cpu().tolist() == tab[3].tolist() and plen.cpu().tolist() == tab[0].tolist()
    assert not torch.equal(before, tab[3])  # something was recorded


@pytest.mark.parametrize("V,Vp", [(50257, 50304), (128256, 128256), (1000, 1024)])
def test_sampler_draws_from_the_rewritten_logits(C, V, Vp):
    """The sampler's fast path trusts the segment maxima: behind the pass it
    draws what ref.sample draws from the reference's logits -- the row whose
    argmax was banned and the row whose new maximum the penalty made among
    them (greedy, so a stale maximum changes the token)."""
    c = _case(V, Vp)
    B = 12
    want = c["want"][0]
    greedy = torch.tensor([0, 1, 0, 0, 0, 1, 1, 1, 0, 1, 0, 1], dtype=torch.int32)
    temp = torch.tensor([0.7, 1.0, 1.3, 0.9, 1.0, 1.0, 1.0, 0.6, 1.1, 1.0, 0.8, 1.0])
    topk = torch.tensor([40, 1, 64, 40, 5, 1, 1, 1, 40, 1, 17, 1], dtype=torch.int32)
    seeds = torch.arange(100, 100 + B, dtype=torch.int64)
    ids = ref.sample(want, temp, topk, greedy, counter_uniform(seeds, c["step"]), V)
    assert int(ids[7]) != int(c["am"][7]) and int(ids[7]) == int(want[7, :V].argmax())
    lg = c["lg"].to(DEV)
    sm = rc.segmax_of(c["lg"]).to(DEV)
    C.repetition(lg, V, *(t.to(DEV) for t in c["tab"]), c["slots"].to(DEV), c["step"].to(DEV), sm)
    got = C.sample(lg, V, temp.to(DEV), topk.to(DEV), greedy.to(DEV), seeds.to(DEV), c["step"].to(DEV), sm, None, None)
    torch.cuda.synchronize()
    assert got.cpu().tolist() == ids.tolist()
    # the lifted logit wins a greedy draw over its own segment (the rest of the row cut away)
    s5 = c["seg5"]
    lg5 = torch.full((1, Vp), -INF)
    lg5[0, s5 * 8: s5 * 8 + 8] = c["lg"][5, s5 * 8: s5 * 8 + 8]
    d5, sm5 = lg5.to(DEV), rc.segmax_of(lg5).to(DEV)
    one = lambda v, dt: torch.tensor([v], dtype=dt, device=DEV)  # noqa: E731
    slot5 = c["slots"][5:6].to(DEV)
    C.repetition(d5, V, *(t.to(DEV) for t in c["tab"]), slot5, c["step"][5:6].to(DEV), sm5)
    tok = C.sample(d5, V, one(1.0, torch.float32), one(1, torch.int32), one(1, torch.int32), one(0, torch.int64),
                   one(0, torch.int64), sm5, None, None)
    torch.cuda.synchronize()
    assert tok.cpu().tolist() == [c["tok5"]]


def test_wrapper_refusals(C):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    i32 = torch.int32

    def call(L, ld=64, seg=None, slots=2):
        C.repetition(z(1, ld), ld, z(slots, dt=i32), torch.ones(slots, device=DEV), z(slots, dt=i32),
                     z(slots, L, dt=i32), z(1, dt=i32), None, seg)

    call(8192)
    call(1, 60)
    with pytest.raises(RuntimeError):  # a context longer than the LDS key set holds
        call(8193)
    with pytest.raises(RuntimeError, match="segmax"):  # segment maxima need rows of whole segments
        call(4, 60, z(1, 8))
    with pytest.raises(RuntimeError):
        C.repetition(z(1, 64), 64, z(3, dt=i32), z(2), z(2, dt=i32), z(2, 4, dt=i32), z(1, dt=i32), None, None)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# engine (HIP backend, native executor, 2 microbatches)

class _RefTailCtx(_RefTail):
    """_RefTail with the repetition pass and the context on the host too."""

    def repetition(self, logits, table, slots, step, vocab):
        c = self._c
        logits.copy_(ref.repetition(c(logits), tuple(map(c, table)), c(slots), c(step), vocab))

    def record_context(self, table, slots, step, tokens, active=None, back=0):
        c = self._c
        h = tuple(map(c, table))
        ref.record_context(h, c(slots), c(step), c(tokens), c(active), back)
        table[3].copy_(h[3])


PROMPTS = [[1, 2, 3, 4], [5, 6], [5, 6, 7, 5, 6, 7, 5, 6, 9, 9, 5, 6] * 3, [7] * 9, [3, 3], list(range(10, 50))]
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
        e.stages[0].backend = _RefTailCtx(e.stages[0].backend)
    return e


def _no_repeated_gram(prompt, out, G):
    x = list(prompt) + list(out)
    return not any(x[i: i + G] == x[e + 1 - G: e + 1]
                   for e in range(len(prompt), len(x)) if e + 1 >= G for i in range(0, e + 1 - G))


def test_engine_flagged_requests_match_the_reference_tail(monkeypatch):
    """Requests with the penalty, the n-gram ban, both, and both beside
    presence / frequency penalties and a ban, among default neighbours that
    leave at different steps: the tokens of the reference sampler tail on the
    same logits (graphs off), with decode graphs on -- first run, captured,
    replayed through the native executor.  The neighbours draw what they draw
    without them, and a group of default requests never launches the pass."""
    monkeypatch.setenv("LSD_NATIVE_EXEC", "1")
    e = _engine()
    default = [OTHERS[0], OTHERS[1], PLAIN_G, OTHERS[2], OTHERS[3], PLAIN_S]
    plain = e.generate_ids(PROMPTS, default)
    assert e.generate_ids(PROMPTS, default) == plain
    d = e.workers[0].draw
    assert d.repetition_launches == 0 and d.ctx_tab is None  # default traffic
    sets = [
        [OTHERS[0], OTHERS[1], dataclasses.replace(PLAIN_G, repetition_penalty=1.5), OTHERS[2], OTHERS[3],
         dataclasses.replace(PLAIN_S, no_repeat_ngram_size=2)],
        [OTHERS[0], dataclasses.replace(OTHERS[1], repetition_penalty=0.7, no_repeat_ngram_size=1),
         dataclasses.replace(PLAIN_G, no_repeat_ngram_size=3, repetition_penalty=1.2, presence_penalty=0.5,
                             frequency_penalty=0.25, banned_token_ids=[plain[2][0]]),
         OTHERS[2], OTHERS[3], dataclasses.replace(PLAIN_S, repetition_penalty=1.3, top_p=0.9, logprobs=2)],
    ]
    r = _engine(graphs=False, ref_tail=True)
    assert isinstance(r.stages[0].backend, _RefTailCtx)
    for sps in sets:
        want = r.generate_ids(PROMPTS, sps)
        for _ in range(3):  # eager first use, capture, replay
            assert e.generate_ids(PROMPTS, sps) == want
        flagged = [i for i, sp in enumerate(sps) if sp.has_context]
        assert all(want[i] != plain[i] for i in flagged if sps[i].greedy)  # plain greedy repeats: the knobs are live
        assert [want[i] for i in range(6) if i not in flagged] == [plain[i] for i in range(6) if i not in flagged]
        for i in flagged:
            G = sps[i].no_repeat_ngram_size
            assert not G or _no_repeated_gram(PROMPTS[i], want[i], G)
    assert d.repetition_launches > 0 and d.ctx_tab is not None
    assert sum(w.native_steps for w in e.workers) > 0
    n = d.repetition_launches
    assert e.generate_ids(PROMPTS, default) == plain  # the table exists now: default groups still run nothing
    assert d.repetition_launches == n
