"""Per-request allowed_token_ids on an MI355X: allow_mask_kernel
(csrc/kernels/allow_mask.hip) against the host reference (ops/reference.py
allow_mask), the sampler behind it, the wrapper's refusals, and the engine
path around the on-device sampler.

The pass is a pure select -- a logit keeps its bits or becomes -inf -- so
logits and segment maxima are compared bit for bit: no tolerance, no skipped
rows.
"""
import dataclasses

import numpy as np
import pytest
import torch

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.runtime.batch import counter_uniform
from llm_sharding_demo_amd.runtime.engine import Engine

from .test_logit_edits_gpu import _RefTail

pytestmark = pytest.mark.gpu

DEV = "cuda"
SLOTS, SCRATCH = 16, 15
INF = float("inf")
B = 12
# rows: off slot (3), scratch slot, out of range (16), one token (7), all (0), every other (12), one segment (5),
# both ends (9), a random half (1), two rows on one slot (14, 14), out of range (-1)
ROW_SLOTS = torch.tensor([3, SCRATCH, 16, 7, 0, 12, 5, 9, 1, 14, 14, -1], dtype=torch.int32)
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


def _words(ids, W):
    return torch.from_numpy(SamplingParams(allowed_token_ids=ids).allowed_mask(W).copy())


_CASES = {}


def _case(V, Vp):
    """CPU tensors of a 12-row case on 16 slots, built once per shape and left
    unchanged.  The table is full of random bits everywhere -- the on == 0
    slots and the bits at or past V included -- so reading the wrong slot, or
    writing a padding column, changes the result."""
    if (V, Vp) in _CASES:
        return _CASES[V, Vp]
    g = torch.Generator().manual_seed(V)
    W = (Vp + 31) // 32
    lg = torch.randn(B, Vp, generator=g) * 3
    on = torch.zeros(SLOTS, dtype=torch.int32)
    bits = torch.randint(-2 ** 31, 2 ** 31, (SLOTS, W), generator=g, dtype=torch.int64).to(torch.int32)
    allowed = {}

    def put(slot, ids, keep_tail=True):
        """The slot's bits below V from `ids`; the random bits at or past V stay."""
        w = _words(ids, W)
        if keep_tail:
            tail = torch.arange(W * 32) >= V
            keep = torch.from_numpy(np.packbits(tail.numpy().astype(np.uint8), bitorder="little").view(np.int32).copy())
            w = w | (bits[slot] & keep)
        bits[slot] = w
        on[slot] = 1
        allowed[slot] = sorted(set(ids))

    am = lg[:, :V].argmax(dim=1)
    one = (int(am[3]) + 1237) % V                                   # row 3: one allowed token, not the argmax
    put(7, [one])
    put(0, list(range(V)))                                          # row 4: every token allowed
    put(12, list(range(0, V, 2)))                                   # row 5: every other token: every byte mixed
    seg = (V // 8) // 3
    put(5, list(range(8 * seg, 8 * seg + 8)))                       # row 6: exactly one whole segment
    put(9, [0, V - 1])                                              # row 7: the two ends
    put(1, torch.randperm(V, generator=g)[: V // 2].tolist())       # row 8: a random half
    put(14, torch.randperm(V, generator=g)[:5].tolist())            # rows 9, 10: two rows on one slot
    assert int(on[3]) == 0 and int(on[SCRATCH]) == 0 and int(bits[3].ne(0).sum()) > W // 2
    c = dict(lg=lg, tab=(on, bits), slots=ROW_SLOTS, V=V, W=W, am=am, one=one, seg=seg, allowed=allowed)
    _CASES[V, Vp] = c
    return c


def _allowed_of(c, r):
    return c["allowed"].get(int(c["slots"][r]))


def _run(C, c, seg):
    """(reference logits, reference segmax, kernel logits, kernel segmax, segmax before)."""
    want = c["lg"].clone()
    sm0 = _segmax(c["lg"]) if seg else None
    wsm = sm0.clone() if seg else None
    ref.allow_mask(want, c["tab"], c["slots"], c["V"], wsm)
    lg = c["lg"].to(DEV)
    tab = tuple(t.to(DEV) for t in c["tab"])
    dsm = sm0.to(DEV) if seg else None
    C.allow_mask(lg, c["V"], *tab, c["slots"].to(DEV), dsm)
    torch.cuda.synchronize()
    assert all(torch.equal(_i32(a), _i32(b)) for a, b in zip(tab, c["tab"]))  # the table is read only
    return want, wsm, lg.cpu(), dsm.cpu() if seg else None, sm0


@pytest.mark.parametrize("V,Vp,seg", [(50257, 50304, True), (50257, 50304, False), (128256, 128256, True),
                                      (1000, 1024, True), (4099, 4104, True), (4099, 4104, False)])
def test_allow_mask_bit_equal(C, V, Vp, seg):
    c = _case(V, Vp)
    want, wsm, got, gsm, sm0 = _run(C, c, seg)
    lg0 = c["lg"]
    assert torch.equal(_i32(got), _i32(want))
    # the case does what it says
    for r in (0, 1, 2, 4, 11):  # off slot; scratch slot; out-of-range slots; every token allowed
        assert torch.equal(_i32(got[r]), _i32(lg0[r]))
    assert torch.equal(_i32(got[:, V:]), _i32(lg0[:, V:]))  # padding columns, whatever their bits
    for r in (3, 5, 6, 7, 8, 9, 10):
        keep = torch.zeros(V, dtype=torch.bool)
        keep[_allowed_of(c, r)] = True
        assert bool((got[r, :V][~keep] == -INF).all())
        assert torch.equal(_i32(got[r, :V][keep]), _i32(lg0[r, :V][keep]))
    assert int((got[3, :V] > -INF).sum()) == 1 and got[3, c["one"]] == lg0[3, c["one"]] and c["one"] != int(c["am"][3])
    assert int((got[7, :V] > -INF).sum()) == 2 and int((got[8, :V] > -INF).sum()) == V // 2
    if not seg:
        return
    assert torch.equal(_i32(gsm), _i32(wsm))
    assert torch.equal(_i32(gsm), _i32(_segmax(got)))  # every segment, touched or not, padding included
    for r in (0, 1, 2, 4, 11):
        assert torch.equal(_i32(gsm[r]), _i32(sm0[r]))
    s = c["seg"]
    # row 6: its one segment keeps its maximum; every other segment that lies below V falls to -inf
    assert gsm[6, s] == sm0[6, s] and int((gsm[6] > -INF).sum()) == 1 + Vp // 8 - V // 8


def test_allow_mask_unaligned_rows(C):
    """Logits whose rows do not start on 16 bytes (V = width = 4099, no
    segment maxima): the dword walk, the same bits."""
    c = _case(4099, 4104)
    V = c["V"]
    lg0 = c["lg"][:, :V].contiguous()
    want = ref.allow_mask(lg0.clone(), c["tab"], c["slots"], V)
    lg = lg0.to(DEV)
    C.allow_mask(lg, V, *(t.to(DEV) for t in c["tab"]), c["slots"].to(DEV), None)
    torch.cuda.synchronize()
    assert torch.equal(_i32(lg), _i32(want)) and not torch.equal(_i32(want), _i32(lg0))


@pytest.mark.parametrize("V,Vp", SHAPES[:3])
@pytest.mark.parametrize("mode", ["top_k", "greedy", "top_p"])
def test_sampler_draws_from_the_masked_logits(C, V, Vp, mode):
    """Behind the mask pass the sampler draws what ref.sample draws from the
    reference-masked logits, with 1, 2 and 5 allowed tokens under top_k = 40
    (more candidates than allowed tokens), greedy and top_p = 0.9; every draw
    lies in the allowed set."""
    g = torch.Generator().manual_seed(V + 1)
    W = (Vp + 31) // 32
    lg0 = torch.randn(B, Vp, generator=g) * 3
    counts = [1, 2, 5] * 4
    lists = [torch.randperm(V, generator=g)[:n].tolist() for n in counts]
    on = torch.ones(SLOTS, dtype=torch.int32)
    bits = torch.zeros(SLOTS, W, dtype=torch.int32)
    slots = torch.randperm(SLOTS, generator=g)[:B].to(torch.int32)
    for s, ids in zip(slots.tolist(), lists):
        bits[s] = _words(ids, W)
    greedy = torch.full((B,), int(mode == "greedy"), dtype=torch.int32)
    temp = torch.tensor([0.7, 1.0, 1.3, 0.9, 1.0, 0.6, 1.0, 0.6, 1.1, 1.0, 0.8, 1.0])
    topk = torch.full((B,), 40, dtype=torch.int32)
    topp = torch.full((B,), 0.9 if mode == "top_p" else 1.0)
    minp = torch.zeros(B)
    seeds = torch.arange(100, 100 + B, dtype=torch.int64)
    step = torch.arange(B, dtype=torch.int64)
    want = ref.allow_mask(lg0.clone(), (on, bits), slots, V)
    ids = ref.sample(want, temp, topk, greedy, counter_uniform(seeds, step), V, topp, minp)
    assert all(int(t) in a for t, a in zip(ids, lists))
    lg = lg0.to(DEV)
    sm = _segmax(lg0).to(DEV)
    C.allow_mask(lg, V, on.to(DEV), bits.to(DEV), slots.to(DEV), sm)
    cut = (topp.to(DEV), minp.to(DEV)) if mode == "top_p" else (None, None)
    got = C.sample(lg, V, temp.to(DEV), topk.to(DEV), greedy.to(DEV), seeds.to(DEV), step.to(DEV), sm, *cut)
    torch.cuda.synchronize()
    assert got.cpu().tolist() == ids.tolist()


def test_wrapper_refusals(C):
    """Every invalid-argument case is an error and launches nothing: the logits
    handed in keep their bits although every flag is on and every bit clear."""
    i32 = torch.int32
    lg = torch.randn(2, 64, device=DEV)
    keep = lg.clone()

    def call(V=64, W=2, nslots=2, seg=None, logits=lg):
        C.allow_mask(logits, V, torch.ones(nslots, dtype=i32, device=DEV), torch.zeros(nslots, W, dtype=i32, device=DEV),
                     torch.zeros(logits.shape[0], dtype=i32, device=DEV), seg)

    with pytest.raises(RuntimeError):
        call(V=65)                                           # V > ld
    with pytest.raises(RuntimeError):
        call(W=1)                                            # W * 32 < ld
    with pytest.raises(RuntimeError):
        call(nslots=0)                                       # nslots <= 0
    lg60 = torch.randn(2, 60, device=DEV)
    keep60 = lg60.clone()
    with pytest.raises(RuntimeError):
        call(V=60, seg=torch.zeros(2, 8, device=DEV), logits=lg60)   # segment maxima: ld % 8 != 0
    with pytest.raises(RuntimeError):
        call(seg=torch.zeros(2, 7, device=DEV))              # ldseg * 8 < ld
    torch.cuda.synchronize()
    assert torch.equal(lg, keep) and torch.equal(lg60, keep60)
    sm = torch.zeros(2, 8, device=DEV)
    call(seg=sm)                                             # the valid call does run
    torch.cuda.synchronize()
    assert bool((lg == -INF).all()) and bool((sm == -INF).all())


# ---------------------------------------------------------------------------
# engine (HIP backend, native executor, 2 microbatches)

class _RefTailAllow(_RefTail):
    """_RefTail with the allowed-token mask on the host too."""

    def allow_mask(self, logits, table, slots, vocab):
        c = self._c
        logits.copy_(ref.allow_mask(c(logits), tuple(map(c, table)), c(slots), vocab))


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
        e.stages[0].backend = _RefTailAllow(e.stages[0].backend)
    return e


def _launches(e):
    return sum(w.draw.allow_launches for w in e.workers)


def test_engine_asking_requests_in_a_changing_batch(monkeypatch):
    """A greedy request whose list leaves its first plain token out and a
    seeded one with a 5-token list draw the same ids alone and among
    default-parameter neighbours that leave at different steps, with decode
    graphs on (first run and replayed) and off; every token, draw 0 included,
    lies in the list; the neighbours draw what they draw without them; the
    greedy tokens are the reference backend's."""
    monkeypatch.setenv("LSD_NATIVE_EXEC", "1")
    e = _engine()
    plain = e.generate_ids([PROMPTS[2]], [PLAIN_G])[0]
    plain_s = e.generate_ids([PROMPTS[5]], [PLAIN_S])[0]
    without = e.generate_ids(PROMPTS[:2] + PROMPTS[3:5], OTHERS)
    default = [OTHERS[0], OTHERS[1], PLAIN_G, OTHERS[2], OTHERS[3], PLAIN_S]
    assert e.generate_ids(PROMPTS, default)[5] == plain_s  # precondition: comparable across compositions
    assert _launches(e) == 0 and all(w.draw.allow_tab is None for w in e.workers)  # an all-default session
    V = e.mcfg.vocab_size
    list_g = [t for t in (3, 500, V - 1, 64, 65) if t != plain[0]]
    list_s = sorted({plain_s[1], 17, 900, 901, 31})
    ask_g = dataclasses.replace(PLAIN_G, allowed_token_ids=list_g)
    ask_s = dataclasses.replace(PLAIN_S, allowed_token_ids=list_s + list_s)  # duplicates collapse
    alone_g = e.generate_ids([PROMPTS[2]], [ask_g])[0]
    alone_s = e.generate_ids([PROMPTS[5]], [ask_s])[0]
    assert _launches(e) > 0
    assert len(alone_g) == N and len(alone_s) == N
    assert set(alone_g) <= set(list_g) and set(alone_s) <= set(list_s) and len(set(alone_s)) > 1
    sps = [OTHERS[0], OTHERS[1], ask_g, OTHERS[2], OTHERS[3], ask_s]
    got = e.generate_ids(PROMPTS, sps)
    assert got[2] == alone_g and got[5] == alone_s
    assert got[:2] + got[3:5] == without  # asking never changes another request's draws
    assert e.generate_ids(PROMPTS, sps) == got  # graphs cached: native steps
    assert sum(w.native_steps for w in e.workers) > 0
    assert sum(w.native_changes for w in e.workers) > 0
    assert _engine(graphs=False).generate_ids(PROMPTS, sps) == got
    assert _engine(graphs=False, ref_tail=True).generate_ids(PROMPTS, sps)[2] == alone_g
    # a request that takes over an asker's slot inherits nothing
    assert e.generate_ids([PROMPTS[2]], [PLAIN_G])[0] == plain
    assert e.generate_ids(PROMPTS, default)[5] == plain_s
    # one allowed token: drawn at every step, seeded or not
    one = dataclasses.replace(PLAIN_S, allowed_token_ids=[777])
    assert e.generate_ids([PROMPTS[2]], [one])[0] == [777] * N


def test_engine_mask_with_edits_penalties_and_logprobs_match_the_reference():
    """llama-test (its EOS, 2, is in the vocabulary): requests that combine the
    mask with bans, min_new_tokens, penalties and logprobs beside default
    neighbours -- the tokens of the reference backend's sampler tail on the
    same logits, and its records (ids and -inf entries exactly; finite
    logprobs to the logprob kernel's documented 5.2e-6).  A disallowed token's
    logprob is -inf."""
    eos = 2
    small = [eos, 40, 41, 500, 999]
    sps = [SamplingParams(greedy=True, max_new_tokens=12, logit_bias={eos: 100}, stop_at_eos=True, min_new_tokens=5,
                          allowed_token_ids=small, logprobs=3),
           OTHERS[0],
           SamplingParams(greedy=True, max_new_tokens=N, presence_penalty=2.0, frequency_penalty=2.0,
                          banned_token_ids=list(range(100, 350)), allowed_token_ids=list(range(90, 400)),
                          min_new_tokens=4, logprobs=5),
           SamplingParams(temperature=1.0, top_k=40, top_p=0.9, seed=5, max_new_tokens=N, presence_penalty=1.5,
                          frequency_penalty=0.7, banned_token_ids=[8, 12], allowed_token_ids=[4, 8, 12, 16, 20, 24],
                          logprobs=5),
           OTHERS[1],
           SamplingParams(temperature=0.9, top_k=30, seed=8, max_new_tokens=9, allowed_token_ids=list(range(0, 1000, 2)))]
    e = _engine(model="llama-test")
    r = _engine(model="llama-test", graphs=False, ref_tail=True)
    assert isinstance(r.stages[0].backend, _RefTailAllow)
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
    assert len(out) == 6 and eos not in out[:5] and out[5] == eos and set(out) <= set(small)
    assert set(want[2].output) <= set(range(90, 100)) | set(range(350, 400))
    assert set(want[3].output) <= {4, 16, 20, 24} and set(want[5].output) <= set(range(0, 1000, 2))
    # the fifth alternative of a request with four drawable tokens is a disallowed (or banned) one: -inf
    for alts in want[3].logprobs.top_logprobs:
        assert sorted(i for i, _ in alts[:4]) == [4, 16, 20, 24] and alts[4][1] == -INF
        assert abs(sum(np.exp(v) for _, v in alts[:4]) - 1.0) < 1e-5  # the log-sum-exp runs over what is left
    assert _launches(e) > 0 and sum(w.draw.penalty_launches for w in e.workers) > 0
    assert sum(w.draw.logit_edit_launches for w in e.workers) > 0 and sum(w.native_steps for w in e.workers) > 0
