"""Per-request bad_words on an MI355X: bad_words_kernel
(csrc/kernels/bad_words.hip) against the host reference (ops/reference.py
bad_words), the sampler behind it, the wrapper's refusals, and the engine path
with hipGraph decode.

The pass only stores -inf -- there is no arithmetic on logits -- so logits and
segment maxima are compared bit for bit: no tolerance, no skipped rows.
"""
import dataclasses

import pytest
import torch

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.runtime.batch import counter_uniform
from llm_sharding_demo_amd.runtime.engine import Engine

from . import bad_words_cases as bc
from .test_repetition_gpu import _RefTailCtx

pytestmark = pytest.mark.gpu

DEV = "cuda"
INF = float("inf")
SHAPES = [(50257, 50304), (1000, 1024), (128256, 128256)]


@pytest.fixture(scope="module")
def C():
    from llm_sharding_demo_amd.ops.hip import _load

    return _load()


_WANT = {}


def _want(c, key, with_step=True):
    """The reference's (logits, segmax) of a case, computed once."""
    if (key, with_step) not in _WANT:
        lg, sm = c["lg"].clone(), bc.segmax_of(c["lg"])
        ref.bad_words(lg, c["tab"], c["ctx"], c["slots"], c["step"] if with_step else None, c["V"], sm)
        _WANT[key, with_step] = (lg, sm)
    return _WANT[key, with_step]


def _run(C, c, seg, with_step=True):
    """(kernel logits, kernel segmax or None) on the host."""
    lg = c["lg"].to(DEV)
    tab = tuple(t.to(DEV) for t in c["tab"])
    plen, ctok = c["ctx"][0].to(DEV), c["ctx"][3].to(DEV)
    dsm = bc.segmax_of(c["lg"]).to(DEV) if seg else None
    C.bad_words(lg, c["V"], *tab, plen, ctok, c["slots"].to(DEV), c["step"].to(DEV) if with_step else None, dsm)
    torch.cuda.synchronize()
    # the tables are read only
    assert all(torch.equal(bc.bits(a), bc.bits(b)) for a, b in zip(tab + (plen, ctok), c["tab"] + (c["ctx"][0], c["ctx"][3])))
    return lg.cpu(), dsm.cpu() if seg else None


@pytest.mark.parametrize("V,Vp", SHAPES)
@pytest.mark.parametrize("seg", [True, False])
def test_bad_words_bit_equal(C, V, Vp, seg):
    """The 14-row case of tests/bad_words_cases.py: sequences of 1, 2 and 32
    tokens, a context shorter than a prefix and one of exactly m - 1 tokens, a
    match at n = L, two sequences banning one token, two banned tokens in one
    segment, token V - 1, a logit that is -inf already, rows with cnt == 0, the
    scratch slot, slots outside the table and a slot with cnt == N."""
    c = bc.case(V, Vp)
    want, wsm = _want(c, (V, Vp))
    got, gsm = _run(C, c, seg)
    lg0 = c["lg"]
    assert torch.equal(bc.bits(got), bc.bits(want))
    # the case does what it says (tests/test_bad_words.py checks the reference against the brute-force rule)
    for r in (0, 1, 10, 11, 12):  # cnt == 0; the scratch slot; slots outside the table; asking, nothing to ban
        assert torch.equal(bc.bits(got[r]), bc.bits(lg0[r]))
    assert torch.equal(bc.bits(got[:, V:]), bc.bits(lg0[:, V:]))  # padding columns
    for r, toks in c["ban"].items():
        changed = {int(t) for t in (bc.bits(got[r]) != bc.bits(lg0[r])).nonzero().flatten()}
        assert changed == {t for t in toks if lg0[r, t] != -INF} and all(got[r, t] == -INF for t in toks)
    assert got[6, V - 1] == -INF and got[7, c["am"][7]] == -INF and int(c["tab"][0][14]) == bc.N == 256
    if not seg:
        return
    assert torch.equal(bc.bits(gsm), bc.bits(wsm))
    assert torch.equal(bc.bits(gsm), bc.bits(bc.segmax_of(got)))  # every segment, touched or not, padding included
    sm0 = bc.segmax_of(lg0)
    for r in (0, 1, 10, 11, 12):
        assert torch.equal(bc.bits(gsm[r]), bc.bits(sm0[r]))
    assert gsm[7, c["am"][7] // 8] < sm0[7, c["am"][7] // 8]  # the argmax's segment fell


def test_bad_words_without_step_is_draw_0(C):
    c = bc.case(50257, 50304)
    want, wsm = _want(c, (50257, 50304), with_step=False)
    got, gsm = _run(C, c, True, with_step=False)
    assert torch.equal(bc.bits(got), bc.bits(want)) and torch.equal(bc.bits(gsm), bc.bits(wsm))
    assert not torch.equal(bc.bits(want), bc.bits(_want(c, (50257, 50304))[0]))  # the prompts alone: another result
    assert got[13, 91] == -INF and got[13, 90] == c["lg"][13, 90]
    c0 = dict(c, step=torch.zeros(c["B"], dtype=torch.int64))
    assert torch.equal(bc.bits(_run(C, c0, True)[0]), bc.bits(got))


@pytest.mark.parametrize("V,Vp", SHAPES)
@pytest.mark.parametrize("B", [1, 3, 256])
def test_bad_words_rows(C, V, Vp, B):
    c = bc.random_case(V, Vp, B)
    want, wsm = _want(c, (V, Vp, B))
    for seg in (True, False):
        got, gsm = _run(C, c, seg)
        assert torch.equal(bc.bits(got), bc.bits(want))
        assert not seg or (torch.equal(bc.bits(gsm), bc.bits(wsm)) and torch.equal(bc.bits(gsm), bc.bits(bc.segmax_of(got))))
    assert not torch.equal(bc.bits(want), bc.bits(c["lg"]))


def test_bad_words_largest_context(C):
    """One row at L = n = 8192 with a 32-token sequence over its last 31 tokens."""
    c = bc.big_case()
    want, wsm = _want(c, "big")
    got, gsm = _run(C, c, True)
    assert torch.equal(bc.bits(got), bc.bits(want)) and torch.equal(bc.bits(gsm), bc.bits(wsm))
    assert got[0, c["am"]] == -INF and got[0, 3] == -INF and torch.equal(bc.bits(got[1]), bc.bits(c["lg"][1]))


@pytest.mark.parametrize("V,Vp", SHAPES)
def test_sampler_draws_from_the_banned_logits(C, V, Vp):
    """The sampler's fast path trusts the segment maxima: with every row's
    argmax banned -- by a one-token sequence or by one over the context's last
    tokens -- greedy and seeded draws are what ref.sample draws from the
    reference-banned logits.  A stale maximum would change the greedy token."""
    B, SL, Lc = 12, 16, 64
    g = torch.Generator().manual_seed(V + 3)
    lg0 = torch.randn(B, Vp, generator=g) * 3
    am = lg0[:, :V].argmax(dim=1).tolist()
    tab, ctx = bc._tables(g, V, SL, Lc, 4, 16)
    slots = torch.randperm(SL, generator=g)[:B].to(torch.int32)
    step = torch.arange(B, dtype=torch.int64)
    for r, s in enumerate(slots.tolist()):
        ctx[0][s] = 5 + r
        x = ctx[3][s, : 5 + 2 * r].tolist()
        second = int(lg0[r, :V].topk(2).indices[1])
        bc._put(tab, s, [x[len(x) - r % 3:] + [am[r]], [(x[-1] + 1) % V, second]])  # the second never matches
    greedy = torch.tensor([1, 0] * 6, dtype=torch.int32)
    temp = torch.tensor([1.0, 0.7, 1.0, 1.3, 1.0, 0.9, 1.0, 0.6, 1.0, 1.1, 1.0, 0.8])
    topk = torch.tensor([1, 40, 1, 64, 1, 5, 1, 40, 1, 17, 1, 40], dtype=torch.int32)
    seeds = torch.arange(100, 100 + B, dtype=torch.int64)
    want = ref.bad_words(lg0.clone(), tab, ctx, slots, step, V)
    assert all(want[r, am[r]] == -INF for r in range(B))
    ids = ref.sample(want, temp, topk, greedy, counter_uniform(seeds, step), V)
    assert all(int(ids[r]) != am[r] for r in range(B))
    assert all(int(ids[r]) == int(want[r, :V].argmax()) for r in range(0, B, 2))
    lg, sm = lg0.to(DEV), bc.segmax_of(lg0).to(DEV)
    C.bad_words(lg, V, *(t.to(DEV) for t in tab), ctx[0].to(DEV), ctx[3].to(DEV), slots.to(DEV), step.to(DEV), sm)
    got = C.sample(lg, V, temp.to(DEV), topk.to(DEV), greedy.to(DEV), seeds.to(DEV), step.to(DEV), sm, None, None)
    torch.cuda.synchronize()
    assert got.cpu().tolist() == ids.tolist()


def test_wrapper_refusals(C):
    """Every invalid-argument case is an error and launches nothing: the logits
    handed in keep their bits although every slot bans token 0."""
    from llm_sharding_demo_amd.ops.hip import HipBackend

    i32 = torch.int32
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    lg = torch.randn(2, 64, device=DEV)
    keep = lg.clone()

    def call(V=64, N=2, T=4, L=8, nslots=2, seg=None, logits=lg, cslots=None):
        cnt, end = torch.ones(nslots, dtype=i32, device=DEV), torch.ones(nslots, N, dtype=i32, device=DEV)
        C.bad_words(logits, V, cnt, end, z(nslots, T, dt=i32), z(nslots if cslots is None else cslots, dt=i32),
                    z(nslots if cslots is None else cslots, L, dt=i32), z(logits.shape[0], dt=i32), None, seg)

    with pytest.raises(RuntimeError):
        call(V=65)                                           # V > ld
    with pytest.raises(RuntimeError):
        call(N=257)                                          # more sequences than the workgroup has threads
    with pytest.raises(RuntimeError):
        call(L=8193)                                         # past the context table's own limit
    with pytest.raises(RuntimeError):
        call(cslots=3)                                       # the two tables cover the same slots
    lg60 = torch.randn(2, 60, device=DEV)
    keep60 = lg60.clone()
    with pytest.raises(RuntimeError, match="segmax"):
        call(V=60, seg=z(2, 8), logits=lg60)                 # segment maxima: ld % 8 != 0
    with pytest.raises(RuntimeError, match="segmax"):
        call(seg=z(2, 7))                                    # not a maximum per segment
    # the backend's wrapper refuses the two sizes the kernel cannot hold before it calls
    be = HipBackend.__new__(HipBackend)
    be.C = C
    tab = lambda N: (z(2, dt=i32), z(2, N, dt=i32), z(2, 4, dt=i32))  # noqa: E731
    cx = lambda L: (z(2, dt=i32), None, None, z(2, L, dt=i32))  # noqa: E731
    with pytest.raises(ValueError, match="256"):
        be.bad_words(lg, tab(257), cx(8), z(2, dt=i32), None, 64)
    with pytest.raises(ValueError, match="8192"):
        be.bad_words(lg, tab(2), cx(8193), z(2, dt=i32), None, 64)
    torch.cuda.synchronize()
    assert torch.equal(lg, keep) and torch.equal(lg60, keep60)
    sm = bc.segmax_of(keep)
    call(N=256, L=8192, seg=sm)                              # the valid call at both limits does run
    torch.cuda.synchronize()
    assert bool((lg[:, 0] == -INF).all()) and torch.equal(lg[:, 1:], keep[:, 1:])
    assert torch.equal(sm, bc.segmax_of(lg))


# ---------------------------------------------------------------------------
# engine (HIP backend, native executor, 2 microbatches)

class _RefTailBad(_RefTailCtx):
    """_RefTailCtx with the bad-words pass on the host too."""

    def bad_words(self, logits, table, ctx_table, slots, step, vocab):
        c = self._c
        logits.copy_(ref.bad_words(c(logits), tuple(map(c, table)), tuple(map(c, ctx_table)), c(slots), c(step), vocab))


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
        e.stages[0].backend = _RefTailBad(e.stages[0].backend)
    return e


def _never_completed(prompt, out, words):
    x = list(prompt) + list(out)
    return not any(x[e + 1 - len(w): e + 1] == list(w) for w in words for e in range(len(prompt), len(x))
                   if e + 1 >= len(w))


def _words_for(prompt, plain):
    """Sequences a plain run of the request completes: its first token behind
    the prompt's last one, its next two tokens, its fifth token alone."""
    return [[prompt[-1], plain[0]], plain[1:3], [plain[4]]]


def test_engine_asking_requests_match_the_reference_tail(monkeypatch):
    """Requests with bad_words -- alone, beside an n-gram ban, penalties, a ban,
    an allowed list and logprobs -- among default neighbours that leave at
    different steps: the tokens of the reference sampler tail on the same
    logits (graphs off), with decode graphs on -- first run, captured, replayed
    through the native executor.  The neighbours draw what they draw without
    them, and a group of default requests never launches the pass."""
    monkeypatch.setenv("LSD_NATIVE_EXEC", "1")
    e = _engine()
    default = [OTHERS[0], OTHERS[1], PLAIN_G, OTHERS[2], OTHERS[3], PLAIN_S]
    plain = e.generate_ids(PROMPTS, default)
    assert e.generate_ids(PROMPTS, default) == plain
    d = e.workers[0].draw
    assert d.bad_words_launches == 0 and d.bad_tab is None and d.ctx_tab is None  # default traffic
    wg, ws = _words_for(PROMPTS[2], plain[2]), _words_for(PROMPTS[5], plain[5])
    w1 = [[PROMPTS[1][-1], plain[1][0]]]
    sets = [
        [OTHERS[0], OTHERS[1], dataclasses.replace(PLAIN_G, bad_words=wg), OTHERS[2], OTHERS[3],
         dataclasses.replace(PLAIN_S, bad_words=ws)],
        [OTHERS[0], dataclasses.replace(OTHERS[1], bad_words=w1, no_repeat_ngram_size=2),
         dataclasses.replace(PLAIN_G, bad_words=wg, repetition_penalty=1.2, presence_penalty=0.5,
                             frequency_penalty=0.25, banned_token_ids=[plain[2][0]]),
         OTHERS[2], OTHERS[3],
         dataclasses.replace(PLAIN_S, bad_words=ws, top_p=0.9, logprobs=2, allowed_token_ids=list(range(0, 1000, 3)))],
    ]
    r = _engine(graphs=False, ref_tail=True)
    assert isinstance(r.stages[0].backend, _RefTailBad)
    for sps in sets:
        want = r.generate_ids(PROMPTS, sps)
        for _ in range(3):  # eager first use, capture, replay
            assert e.generate_ids(PROMPTS, sps) == want
        asking = [i for i, sp in enumerate(sps) if sp.bad_words]
        assert all(want[i] != plain[i] for i in asking)  # every list bans the request's plain first or second token
        assert [want[i] for i in range(6) if i not in asking] == [plain[i] for i in range(6) if i not in asking]
        for i in asking:
            assert len(want[i]) == sps[i].max_new_tokens and _never_completed(PROMPTS[i], want[i], sps[i].bad_words)
    assert d.bad_words_launches > 0 and d.bad_tab is not None and d.ctx_tab is not None
    assert sum(w.native_steps for w in e.workers) > 0
    n = d.bad_words_launches
    assert e.generate_ids(PROMPTS, default) == plain  # the tables exist now: default groups still run nothing
    assert d.bad_words_launches == n


def test_engine_group_rekeys_when_an_asking_row_joins_and_leaves(monkeypatch):
    """One group: a short asking request joins long default ones and leaves
    again.  The group's decode graph is keyed by the bad-words flag, so it is
    captured for both compositions; the default rows draw what they draw
    alone, before, beside and after the asking row."""
    monkeypatch.setenv("LSD_NATIVE_EXEC", "1")
    cfg = EngineConfig(model_id="gpt2-test", num_stages=1, max_batch=4, device="cuda", use_graphs=True,
                       max_seq_len=512, num_microbatches=1)
    e = Engine(cfg, devices=["cuda:0"])
    long_g = SamplingParams(greedy=True, max_new_tokens=40)
    long_s = SamplingParams(temperature=1.0, top_k=40, seed=5, max_new_tokens=40)
    prompts = [PROMPTS[5], PROMPTS[5], PROMPTS[5]]
    alone = e.generate_ids(prompts, [long_g, long_s, SamplingParams(greedy=True, max_new_tokens=6)])
    d = e.workers[0].draw
    assert d.bad_words_launches == 0 and d.bad_tab is None
    ask = SamplingParams(greedy=True, max_new_tokens=6, bad_words=[[alone[2][0]], alone[2][1:3]])
    for _ in range(2):  # capture, replay
        n, caps = d.bad_words_launches, sum(w.captures for w in e.workers)
        got = e.generate_ids(prompts, [long_g, long_s, ask])
        assert got[:2] == alone[:2]                      # default rows keep their draws
        assert got[2] != alone[2] and _never_completed(prompts[2], got[2], ask.bad_words)
        # the pass ran while the asking row was there -- its prefill draw and 5 decode items -- and not after
        assert d.bad_words_launches - n == 6
    keys = set(e.workers[0].groups[0].graphs)
    assert {k[-1] for k in keys} == {False, True}  # the flag is the key's last part: graphs for both compositions
    assert all(k[-3] == k[-1] for k in keys) and not any(k[-2] for k in keys)  # an asking row has a context; no mask
    assert e.generate_ids(prompts[:2], [long_g, long_s]) == alone[:2]
