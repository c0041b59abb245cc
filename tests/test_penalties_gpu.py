"""Presence / frequency penalties on an MI355X: penalize_kernel and
record_tokens_kernel (csrc/kernels/penalty.hip) and apply_rows' 16-word record
against the host reference (ops/reference.py penalize / record_tokens), and
the engine path around the on-device sampler.

The kernel counts with integer LDS atomics and rounds the product, the sum
and the difference separately, so logits and segment maxima are compared bit
for bit: no tolerance, no skipped rows.
"""
import numpy as np
import pytest
import torch

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.runtime.engine import Engine

pytestmark = pytest.mark.gpu

DEV = "cuda"
SLOTS, SCRATCH = 16, 15


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


def _case(V, Vp, L=1024):
    """CPU tensors of a 12-row case.  The history buffer is full of valid
    tokens everywhere (other slots, entries past the count), so reading
    anything but hist[slot, :count] changes the result."""
    g = torch.Generator().manual_seed(V + L)
    B = 12
    lg = torch.randn(B, Vp, generator=g) * 3
    hist = torch.randint(0, V, (SLOTS, L), generator=g, dtype=torch.int32)
    slots = torch.tensor([3, 7, 0, 12, 5, 9, 1, 14, 2, SCRATCH, 11, 6], dtype=torch.int32)
    n = [0, 1, 7, 64, 300, 1023, 64, 7, 300, 0, 1023, 300]
    pres = [1.0, 1.5, 0.0, 0.7, 2.0, 0.3, 1.0, -2.0, 0.0, 0.0, -0.1, -0.7]
    freq = [0.5, 0.0, 0.3, 0.1, 2.0, 0.013, 0.5, -2.0, 0.0, 0.0, 2.0, 0.01]
    am = lg[:, :V].argmax(dim=1)
    hist[7, 0] = am[1]                      # the row's argmax: its segment maximum must fall
    hist[0, :7] = 123                       # one token repeated throughout
    hist[12, 5], hist[12, 40] = 808, 811    # two distinct tokens in one 8-logit segment
    hist[5, 0], hist[5, 299], hist[5, 150] = 0, V - 1, V - 1  # both ends of the vocabulary
    hist[9, 1000] = am[5]
    seg6 = 40  # row 6: only the smallest logit of one segment: its maximum stays
    hist[1, :64] = seg6 * 8 + int(lg[6, seg6 * 8: seg6 * 8 + 8].argmin())
    seg7 = 77  # row 7: a negative penalty lifts the segment's smallest logit above its maximum
    tok7 = seg7 * 8 + int(lg[7, seg7 * 8: seg7 * 8 + 8].argmin())
    lg[7, seg7 * 8: seg7 * 8 + 8] = lg[7, seg7 * 8: seg7 * 8 + 8].clamp(-5, 5)
    hist[14, :7] = tok7                     # 2 + 2 * 7 = 16 > 10
    hist[11, :1023] = 999                   # count 1023
    # row 11: 40 tokens, ~7 times each, with a frequency whose products round:
    # a fused multiply-add (one rounding for product and sum) would differ
    hist[6, :300] = torch.randint(200, 240, (300,), generator=g, dtype=torch.int32)
    return dict(lg=lg, hist=hist, slots=slots, counts=torch.tensor(n, dtype=torch.int64),
                pres=torch.tensor(pres), freq=torch.tensor(freq), V=V, seg6=seg6, seg7=seg7, tok7=tok7)


def _run(C, c, seg):
    """(reference logits, reference segmax, kernel logits, kernel segmax, segmax before)."""
    want = c["lg"].clone()
    sm0 = _segmax(c["lg"]) if seg else None
    wsm = sm0.clone() if seg else None
    ref.penalize(want, c["hist"], c["slots"], c["counts"], c["pres"], c["freq"], c["V"], wsm)
    d = {k: c[k].to(DEV) for k in ("lg", "hist", "slots", "counts", "pres", "freq")}
    dsm = sm0.to(DEV) if seg else None
    C.penalize(d["lg"], c["V"], d["hist"], d["slots"], d["counts"], d["pres"], d["freq"], dsm)
    torch.cuda.synchronize()
    assert torch.equal(d["hist"].cpu(), c["hist"])
    return want, wsm, d["lg"].cpu(), dsm.cpu() if seg else None, sm0


@pytest.mark.parametrize("V,Vp,seg", [(50257, 50304, True), (50257, 50304, False), (1000, 1024, True),
                                      (128256, 128256, True)])
def test_penalize_bit_equal(C, V, Vp, seg):
    c = _case(V, Vp)
    want, wsm, got, gsm, sm0 = _run(C, c, seg)
    assert torch.equal(_bits(got), _bits(want))
    # the case does what it says: untouched rows, changed rows, padding columns
    for r in (0, 8, 9):  # empty history; 0.0 / 0.0; pad row on the scratch slot
        assert torch.equal(_bits(got[r]), _bits(c["lg"][r]))
    assert all(not torch.equal(got[r], c["lg"][r]) for r in (1, 2, 3, 4, 5, 6, 7, 10, 11))
    assert torch.equal(_bits(got[:, V:]), _bits(c["lg"][:, V:]))
    h4 = c["hist"][5, :300].tolist()  # row 4: presence 2.0, frequency 2.0 on both ends of the vocabulary
    for t in (0, V - 1):
        assert h4.count(t) >= 1 and got[4, t] == c["lg"][4, t] - np.float32(2.0 + 2.0 * h4.count(t))
    if not seg:
        return
    assert torch.equal(_bits(gsm), _bits(wsm))
    assert torch.equal(_bits(gsm), _bits(_segmax(got)))  # every segment, touched or not
    a1 = int(c["lg"][1, :V].argmax())
    assert gsm[1, a1 // 8] < sm0[1, a1 // 8]                      # the argmax's segment fell
    assert gsm[6, c["seg6"]] == sm0[6, c["seg6"]]                 # a non-maximal token: unchanged
    assert gsm[7, c["seg7"]] == got[7, c["tok7"]] > sm0[7, c["seg7"]]  # lifted to the new maximum
    for r in (0, 8, 9):
        assert torch.equal(_bits(gsm[r]), _bits(sm0[r]))


@pytest.mark.parametrize("L", [4096, 8192])
def test_penalize_long_history(C, L):
    """4095 entries fill the 64 KB table of a 4096-token history; 8191 the
    128 KB one of Llama-3's 8192 positions (the longest the kernel takes)."""
    V, Vp = 50257, 50304
    g = torch.Generator().manual_seed(L)
    lg = torch.randn(3, Vp, generator=g) * 3
    hist = torch.randint(0, V, (4, L), generator=g, dtype=torch.int32)
    hist[2, : L // 2] = torch.randint(0, 50, (L // 2,), generator=g, dtype=torch.int32)  # heavy repeats
    c = dict(lg=lg, hist=hist, slots=torch.tensor([1, 2, 0], dtype=torch.int32),
             counts=torch.tensor([L - 1, L - 1, 5], dtype=torch.int64), pres=torch.tensor([0.5, -1.0, 0.0]),
             freq=torch.tensor([0.25, 0.01, 0.0]), V=V)
    want, wsm, got, gsm, _ = _run(C, c, True)
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(gsm), _bits(wsm))
    assert torch.equal(_bits(got[2]), _bits(lg[2])) and not torch.equal(got[0], lg[0])


def test_penalize_refuses_longer_histories(C):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    with pytest.raises(RuntimeError, match="8192"):
        C.penalize(z(1, 64), 64, z(2, 8193, dt=torch.int32), z(1, dt=torch.int32), z(1, dt=torch.int64), z(1), z(1))


@pytest.mark.parametrize("with_step", [True, False])
def test_record_tokens(C, with_step):
    g = torch.Generator().manual_seed(5)
    B, L, S = 300, 64, 512
    hist = torch.full((S, L), -1, dtype=torch.int32)
    slots = torch.randperm(S, generator=g)[:B].to(torch.int32)
    step = torch.randint(1, L + 1, (B,), generator=g, dtype=torch.int64)
    step[7], step[8] = L + 1, 0  # entries L and -1: outside the history, dropped
    tokens = torch.randint(0, 50257, (B,), generator=g, dtype=torch.int32)
    active = torch.randint(0, 2, (B,), generator=g, dtype=torch.int32)
    want = hist.clone()
    ref.record_tokens(want, slots, step if with_step else None, tokens, active, 1 if with_step else 0)
    got = hist.to(DEV)
    C.record_tokens(got, slots.to(DEV), step.to(DEV) if with_step else None, tokens.to(DEV), active.to(DEV),
                    1 if with_step else 0)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want)
    assert int((want != -1).sum()) == int(active.sum()) - (int(active[7]) + int(active[8]) if with_step else 0)
    if not with_step:  # without `active` every row is written, at entry 0
        C.record_tokens(got, slots.to(DEV), None, tokens.to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(got.cpu()[slots.long(), 0], tokens) and int((got.cpu() != -1).sum()) == B


@pytest.mark.parametrize("cap,b,n", [(256, 256, 256), (256, 128, 77), (2048, 2048, 1500), (8, 8, 3)])
def test_apply_rows_16_word_record(C, cap, b, n):
    """The 16-word record scatters the presence / frequency columns f[8 cap,
    9 cap) and f[9 cap, 10 cap): pad rows 0.0, rows past b untouched; the 12-
    and 14-word records leave the two vectors alone."""
    g = torch.Generator().manual_seed(cap + b + n)
    scratch = 4321
    ri = lambda lo, hi, k: torch.randint(lo, hi, (k,), generator=g)  # noqa: E731
    cols = [ri(0, 10000, n), ri(0, 4096, n), torch.rand(n, generator=g) + 0.1, ri(1, 64, n), ri(0, 2, n),
            ri(0, cap, n), torch.rand(n, generator=g), torch.rand(n, generator=g),
            torch.rand(n, generator=g) * 4 - 2, torch.rand(n, generator=g) * 4 - 2]
    a = np.zeros(14 * cap + 1, np.int32)
    a[4 * cap] = n
    f0 = 4 * cap + 1
    for k, v in enumerate(cols):
        v = v.numpy()
        a[f0 + k * cap: f0 + k * cap + n] = v.view(np.int32) if v.dtype == np.float32 else v
    buf = torch.from_numpy(a).to(DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    f32 = dict(dtype=torch.float32, device=DEV)
    i64 = dict(dtype=torch.int64, device=DEV)
    pad = b - n

    def run(nargs):
        t = [torch.full((cap,), -1, **i32) for _ in range(3)]                                    # slots pos act
        t += [torch.full((cap,), 7.0, **f32), torch.full((cap,), -1, **i32), torch.full((cap,), -1, **i32)]
        t += [torch.full((cap,), -1, **i64), torch.full((cap,), -1, **i64)]                      # seeds sstep
        vec = [torch.full((cap,), 7.0, **f32) for _ in range(4)]                                 # topp minp pres freq
        rec = [cap, scratch, buf.data_ptr()] + [x.data_ptr() for x in t] + [0] + [x.data_ptr() for x in vec]
        C.apply_rows(torch.tensor(rec[:nargs], dtype=torch.int64), b)
        torch.cuda.synchronize()
        return t, [x.cpu() for x in vec]

    t, (topp, minp, pres, freq) = run(16)
    cat = lambda v, fill: torch.cat([v.float(), torch.full((pad,), fill)])  # noqa: E731
    assert torch.equal(pres[:b], cat(cols[8], 0.0)) and torch.equal(freq[:b], cat(cols[9], 0.0))
    assert (pres[b:] == 7.0).all() and (freq[b:] == 7.0).all()
    assert torch.equal(topp[:b], cat(cols[6], 1.0)) and torch.equal(minp[:b], cat(cols[7], 0.0))
    assert torch.equal(t[0][:b].cpu().long(), torch.cat([cols[0], torch.full((pad,), scratch)]))
    assert torch.equal(t[3][:b].cpu(), cat(cols[2], 1.0))
    _, (topp, minp, pres, freq) = run(14)
    assert torch.equal(topp[:b], cat(cols[6], 1.0)) and (pres == 7.0).all() and (freq == 7.0).all()
    _, (topp, minp, pres, freq) = run(12)
    assert all((v == 7.0).all() for v in (topp, minp, pres, freq))


# ---------------------------------------------------------------------------
# engine (gpt2-test, HIP backend, native executor, 2 microbatches)

# The two penalised requests take the 40-token prompt: a seeded draw is only
# comparable between batch compositions while the prefill logits are (the
# 3-token prompts' are not bit-equal alone and merged with others, penalty or
# not), which the test asserts for the plain seeded request first.
PROMPTS = [[1, 2, 3, 4], [5, 6], list(range(10, 50)), [7] * 9, [3, 3], list(range(10, 50))]
N = 24
PEN_G = SamplingParams(greedy=True, max_new_tokens=N, presence_penalty=2.0, frequency_penalty=2.0)
PEN_S = SamplingParams(temperature=1.0, top_k=40, seed=5, max_new_tokens=N, presence_penalty=1.5,
                       frequency_penalty=0.7)
OTHERS = [SamplingParams(temperature=0.8, top_k=20, seed=11 + i, max_new_tokens=n) for i, n in enumerate((3, 6, 1, 5))]


def _engine(graphs=True, **kw):
    cfg = EngineConfig(model_id="gpt2-test", num_stages=1, max_batch=16, device="cuda", use_graphs=graphs,
                       max_seq_len=512, num_microbatches=2, **kw)
    e = Engine(cfg, devices=["cuda:0"])
    assert e.stages[0].backend.name == "hip"
    return e


def test_engine_penalised_requests_in_a_changing_batch(monkeypatch):
    """A penalised greedy and a penalised seeded request draw the same ids
    alone and among default-parameter neighbours that leave at different
    steps, with decode graphs on (first run and replayed) and off; the
    neighbours draw what they draw without them; positive penalties first
    diverge from the plain request where it repeated a token."""
    monkeypatch.setenv("LSD_NATIVE_EXEC", "1")
    e = _engine()
    plain = e.generate_ids([PROMPTS[2]], [SamplingParams(greedy=True, max_new_tokens=N)])[0]
    plain_s = e.generate_ids([PROMPTS[5]], [SamplingParams(temperature=1.0, top_k=40, seed=5, max_new_tokens=N)])[0]
    without = e.generate_ids(PROMPTS[:2] + PROMPTS[3:5], OTHERS)
    default = [OTHERS[0], OTHERS[1], SamplingParams(greedy=True, max_new_tokens=N), OTHERS[2], OTHERS[3],
               SamplingParams(temperature=1.0, top_k=40, seed=5, max_new_tokens=N)]
    assert e.generate_ids(PROMPTS, default)[5] == plain_s  # precondition: comparable across compositions
    assert sum(w.draw.penalty_launches for w in e.workers) == 0  # all-default traffic so far
    alone_g = e.generate_ids([PROMPTS[2]], [PEN_G])[0]
    alone_s = e.generate_ids([PROMPTS[5]], [PEN_S])[0]
    assert sum(w.draw.penalty_launches for w in e.workers) > 0
    assert len(alone_g) == N and len(alone_s) == N
    assert len(set(plain)) < N           # precondition: plain greedy repeats a token
    assert alone_g != plain and alone_s != plain_s  # the penalties are live
    i = next(k for k in range(N) if plain[k] != alone_g[k])
    assert plain[i] in plain[:i]
    sps = [OTHERS[0], OTHERS[1], PEN_G, OTHERS[2], OTHERS[3], PEN_S]
    got = e.generate_ids(PROMPTS, sps)
    assert got[2] == alone_g and got[5] == alone_s
    assert got[:2] + got[3:5] == without
    assert e.generate_ids(PROMPTS, sps) == got  # graphs cached: native steps
    assert sum(w.native_steps for w in e.workers) > 0
    assert sum(w.native_changes for w in e.workers) > 0
    assert _engine(graphs=False).generate_ids(PROMPTS, sps) == got
