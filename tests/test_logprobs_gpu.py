"""Token logprobs and top-N alternatives on an MI355X: logprob_kernel
(csrc/kernels/logprob.hip) against the host reference (ops/reference.py
logprobs) and a float64 recomputation, apply_rows' 17-word record, and the
engine path behind the on-device sampler.

Ids are compared exactly, the drawn token's logprob bit for bit with its entry
among the alternatives, two launches bit for bit.  Values are compared with the
float64 recomputation on the finite entries with x - max >= -40:

    GATE = 4 x the largest |device - float64| measured on the MI355X over the
    probe rows and the random rows of this file (MEASURED below; the margin is
    for other seeds and the few-ulp freedom of the fast exp / log), and by
    condition never above 1e-4: an fp32 sum of 128 K positive terms in tree
    order, one log and the final subtraction put the derived bound near 5e-6.

Measured (profiles/logprob_ab.log): probe rows 1.0e-07 (V = 8), 4.5e-07 (1000),
6.8e-07 (50257), 9.8e-08 (53249); random rows 4.4e-07 to 7.1e-07 (V = 1000),
4.3e-07 to 9.0e-07 (50257), 1.4e-07 to 4.7e-07 (53249), 4.6e-07 to 1.3e-06
(128256).  Largest 1.296e-06, so GATE = 5.184e-06.

Every test prints the largest error it saw before it asserts.
"""
import numpy as np
import pytest
import torch

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.runtime.engine import Engine

from . import logprob_probes as lpp

pytestmark = pytest.mark.gpu

DEV = "cuda"
MEASURED = 1.296e-06  # V = 128256, B = 3 random rows; probes 6.8e-07 at most
GATE = 4 * MEASURED
assert GATE <= 1e-4
W = lpp.MAXW
SENT_F, SENT_I = 777.0, -777


@pytest.fixture(scope="module")
def C():
    from llm_sharding_demo_amd.ops.hip import _load

    return _load()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _launch(C, rows, V, toks, nlp, slots=None, step=None, back=0, active=None, L=3, nslots=None, width=W):
    """One launch over `rows` [B, ld] -> the three record buffers (CPU),
    sentinel-filled beforehand."""
    B = rows.shape[0]
    nslots = nslots or B + 2
    slots = np.arange(B) if slots is None else slots
    i32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int32).to(DEV)  # noqa: E731
    lt = torch.full((nslots, L), SENT_F, device=DEV)
    li = torch.full((nslots, L, width), SENT_I, dtype=torch.int32, device=DEV)
    lv = torch.full((nslots, L, width), SENT_F, device=DEV)
    C.logprobs(torch.as_tensor(rows).to(DEV), V, i32(toks), i32(nlp), i32(slots),
               None if step is None else torch.as_tensor(np.asarray(step), dtype=torch.int64).to(DEV),
               None if active is None else i32(active), lt, li, lv, back)
    torch.cuda.synchronize()
    return lt.cpu(), li.cpu(), lv.cpu()


def _check_rows(rows, V, toks, nlp, got, where, width=W):
    """Every live row against the reference (ids exactly) and the float64
    recomputation (values); -> largest value error over the gated entries."""
    lt, li, lv = got
    rt, ri, rv = ref.logprobs(torch.as_tensor(rows), torch.as_tensor(toks), list(nlp), V, width)
    worst = 0.0
    for r, (s, j) in enumerate(where):
        n = int(nlp[r])
        if n < 0:
            continue
        ids = li[s, j].tolist()
        assert ids == ri[r].tolist(), (r, ids, ri[r].tolist())
        assert not any(i >= V for i in ids)
        x = rows[r, :V].astype(np.float64)
        lse, tok_lp, eids, elps = lpp.expect(rows[r], V, n, int(toks[r]), width)
        assert ids == eids.tolist()
        dev = lv[s, j].double().numpy()
        fin = np.isfinite(elps)
        assert np.array_equal(np.isfinite(dev), fin) and (dev[~fin] == -np.inf).all()
        gated = fin & (np.where(eids >= 0, x[np.maximum(eids, 0)], -np.inf) - x.max() >= -40)
        if gated.any():
            worst = max(worst, float(np.abs(dev[gated] - elps[gated]).max()))
        t = float(lt[s, j])
        if np.isfinite(tok_lp):
            if x[int(toks[r])] - x.max() >= -40:
                worst = max(worst, abs(t - tok_lp))
        else:
            assert t == -np.inf
        if int(toks[r]) in ids:  # the same fl(x - lse)
            assert _bits(lt[s, j]).item() == _bits(lv[s, j, ids.index(int(toks[r]))]).item()
    return worst


PROBES = lpp.case_list()


@pytest.mark.parametrize("V", sorted({c["V"] for c in PROBES}))
def test_probe_rows(C, V):
    cs = [c for c in PROBES if c["V"] == V]
    rows = np.stack([c["row"] for c in cs])
    toks, nlp = [c["tok"] for c in cs], [c["n"] for c in cs]
    got = _launch(C, rows, V, toks, nlp)
    where = [(r, 0) for r in range(len(cs))]
    worst = _check_rows(rows, V, toks, nlp, got, where)
    print(f"logprob probes V={V}: {len(cs)} rows, max |device - float64| = {worst:.3e} (gate {GATE:.3e})")
    again = _launch(C, rows, V, toks, nlp)
    for a, b in zip(got, again):
        assert torch.equal(_bits(a), _bits(b))
    lt, li, lv = got
    for r, c in enumerate(cs):
        if "ids" in c:
            assert li[r, 0, : len(c["ids"])].tolist() == list(c["ids"]), c["name"]
        if c["name"] == "single-finite":
            assert float(lt[r, 0]) == 0.0 and float(lv[r, 0, 0]) == 0.0  # exactly
        if c["name"].startswith("cover-"):  # a skipped position gives 0, a doubled one -ln 3
            assert abs(float(lt[r, 0]) + np.log(2.0)) < 1e-6, c["name"]
        if c["name"].startswith("all-equal"):
            assert abs(float(lt[r, 0]) + np.log(V)) <= max(GATE, 1e-6)
        # records [1, L) of the slot, and the two spare slots, keep their sentinel
        assert (lt[r, 1:] == SENT_F).all() and (li[r, 1:] == SENT_I).all()
    assert (lt[len(cs):] == SENT_F).all() and (lv[len(cs):] == SENT_F).all()
    assert worst <= GATE


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("V,ld", [(1000, 1024), (50257, 50304), (53249, 53312), (128256, 128256)])
def test_random_rows(C, V, ld, B):
    """Random rows (padding columns +inf / 3e38), mixed counts, records written
    at step - 1 of shuffled slots, an inactive row among them."""
    rng = np.random.default_rng(V + B)
    rows = (rng.standard_normal((B, ld)) * 3).astype(np.float32)
    rows[:, V:] = lpp.PAD_REST
    if ld > V:
        rows[:, V] = lpp.PAD_FIRST
    counts = [20, -1, 5, 0, 1]
    nlp = np.array([counts[(r + B) % 5] for r in range(B)], dtype=np.int32)
    if B == 1:
        nlp[0] = 20
    toks = rng.integers(0, V, B)
    toks[0] = int(rows[0, :V].argmax())  # among the alternatives
    L, nslots = 4, B + 3
    slots = rng.permutation(nslots)[:B]
    step = rng.integers(1, L + 1, B)
    active = np.ones(B, dtype=np.int32)
    if B == 5:
        active[2] = 0
    got = _launch(C, rows, V, toks, nlp, slots, step, 1, active, L, nslots)
    live = nlp.copy()
    live[active == 0] = -1
    where = [(int(s), int(j) - 1) for s, j in zip(slots, step)]
    worst = _check_rows(rows, V, toks, live, got, where)
    print(f"logprob random V={V} B={B}: max |device - float64| = {worst:.3e} (gate {GATE:.3e})")
    again = _launch(C, rows, V, toks, nlp, slots, step, 1, active, L, nslots)
    for a, b in zip(got, again):
        assert torch.equal(_bits(a), _bits(b))
    # everything but the live rows' records keeps its sentinel
    lt, li, lv = (t.clone() for t in got)
    for r, (s, j) in enumerate(where):
        if live[r] >= 0:
            lt[s, j], li[s, j], lv[s, j] = SENT_F, SENT_I, SENT_F
    assert (lt == SENT_F).all() and (li == SENT_I).all() and (lv == SENT_F).all()
    assert worst <= GATE


def test_off_rows_and_guards(C):
    """Rows that did not ask and inactive rows between live ones, a slot
    outside the buffer and a record outside [0, L): their records keep the
    sentinel written beforehand."""
    V, ld = 1000, 1024
    nlp, active = lpp.off_rows()
    B = len(nlp)
    rng = np.random.default_rng(1)
    rows = (rng.standard_normal((B, ld)) * 3).astype(np.float32)
    toks = rng.integers(0, V, B)
    lt, li, lv = _launch(C, rows, V, toks, nlp, active=active, L=2)
    for r in range(B):
        on = nlp[r] >= 0 and active[r]
        assert (float(lt[r, 0]) != SENT_F) == bool(on), r
        assert bool((li[r, 0] != SENT_I).all()) == bool(on) and bool((lv[r, 0] != SENT_F).all()) == bool(on)
        if on:  # entries [n, W) are padded
            assert (li[r, 0, nlp[r]:] == -1).all() and (lv[r, 0, nlp[r]:] == -np.inf).all()
        assert float(lt[r, 1]) == SENT_F
    n5 = np.full(4, 5, dtype=np.int32)
    got = _launch(C, rows[:4], V, toks[:4], n5, slots=[-1, 6, 2, 3], step=[1, 1, 0, 3], back=1, L=2, nslots=6)
    assert all((t == (SENT_I if t.dtype == torch.int32 else SENT_F)).all() for t in got)


def test_wrapper_refusals(C):
    rows = np.zeros((1, 64), dtype=np.float32)
    with pytest.raises(RuntimeError):
        _launch(C, rows, 64, [0], [1], width=21)
    with pytest.raises(RuntimeError):
        _launch(C, rows, 65, [0], [1])
    lt, li, lv = _launch(C, rows, 64, [0], [20])  # W = 20, V = ld: taken
    assert li[0, 0].tolist() == list(range(20))


def test_apply_rows_17_word_record(C):
    """The 17-word record scatters the logprob counts f[10 cap, 11 cap): pad
    rows -1, rows past b untouched; the 16-word record leaves the vector alone."""
    cap, b, n = 64, 32, 21
    g = torch.Generator().manual_seed(3)
    a = np.zeros(15 * cap + 1, np.int32)
    a[4 * cap] = n
    f0 = 4 * cap + 1
    counts = torch.randint(-1, 21, (n,), generator=g).numpy().astype(np.int32)
    a[f0 + 10 * cap: f0 + 10 * cap + n] = counts
    a[f0 + 8 * cap: f0 + 8 * cap + n] = np.full(n, 0.5, np.float32).view(np.int32)
    buf = torch.from_numpy(a).to(DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    f32 = dict(dtype=torch.float32, device=DEV)

    def run(nargs):
        t = [torch.full((cap,), -5, **i32) for _ in range(3)]
        t += [torch.full((cap,), 7.0, **f32), torch.full((cap,), -5, **i32), torch.full((cap,), -5, **i32)]
        t += [torch.full((cap,), -5, dtype=torch.int64, device=DEV) for _ in range(2)]
        vec = [torch.full((cap,), 7.0, **f32) for _ in range(4)] + [torch.full((cap,), -5, **i32)]
        rec = [cap, 99, buf.data_ptr()] + [x.data_ptr() for x in t] + [0] + [x.data_ptr() for x in vec]
        C.apply_rows(torch.tensor(rec[:nargs], dtype=torch.int64), b)
        torch.cuda.synchronize()
        return [x.cpu() for x in vec]

    *_, pres, freq, nlp = run(17)
    assert nlp[:n].tolist() == counts.tolist() and (nlp[n:b] == -1).all() and (nlp[b:] == -5).all()
    assert (pres[:n] == 0.5).all() and (pres[n:b] == 0.0).all() and (freq[:b] == 0.0).all()
    *_, nlp = run(16)
    assert (nlp == -5).all()


# ---------------------------------------------------------------------------
# engine (gpt2-test, HIP backend, native executor)

N = 16
RND = np.random.default_rng(21)
PROMPTS = [RND.integers(1, 1000, int(RND.integers(2, 40))).tolist() for _ in range(16)]


def _params(ask: bool):
    out = []
    for i in range(16):
        kind = i % 4
        lp = (3, 0, 5, 1)[(i // 4) % 4] if ask and kind != 3 else None
        n = (N, 5, 9, 12)[i % 4]
        if kind == 0:
            out.append(SamplingParams(greedy=True, max_new_tokens=n, logprobs=lp))
        elif kind == 1:
            out.append(SamplingParams(temperature=0.9, top_k=30, seed=40 + i, max_new_tokens=n, logprobs=lp))
        elif kind == 2:
            out.append(SamplingParams(greedy=i % 8 == 2, temperature=1.0, top_k=50, top_p=0.9, seed=60 + i,
                                      max_new_tokens=n, presence_penalty=1.5, frequency_penalty=0.5, logprobs=lp))
        else:
            out.append(SamplingParams(temperature=0.8, top_k=20, seed=80 + i, max_new_tokens=n))
    return out


def _engine(P=1, graphs=True, **kw):
    cfg = EngineConfig(model_id="gpt2-test", num_stages=P, max_batch=16, device="cuda", use_graphs=graphs,
                       max_seq_len=256, num_microbatches=4, merge_prefill=False, prefill_budget=48, **kw)
    e = Engine(cfg) if P > 1 else Engine(cfg, devices=["cuda:0"])
    assert e.stages[0].backend.name == "hip"
    return e


def _records(reqs):
    return [(r.output, r.logprobs) for r in reqs]


def test_engine_changing_batch(monkeypatch):
    """Sixteen requests in four groups -- logprob, penalised and default ones,
    joining over several steps (a prefill budget of 48 tokens per group and
    step: which step a request joins at does not depend on when readouts land,
    so every run sees the same compositions and the same logits) and leaving
    at different steps -- with decode graphs (first use, capture, replay),
    without, and on two loopback stages: the tokens of the same requests
    without logprobs, and the same records everywhere."""
    monkeypatch.setenv("LSD_NATIVE_EXEC", "1")
    e = _engine()
    plain = e.generate_ids(PROMPTS, _params(False))
    assert e.generate_ids(PROMPTS, _params(False)) == plain
    assert sum(w.draw.logprob_launches for w in e.workers) == 0 and e.workers[0].draw.lp_rec is None  # all-default traffic
    native0 = sum(w.native_steps for w in e.workers)
    assert native0 > 0
    sps = _params(True)
    first = _records(e.generate_requests(PROMPTS, sps))
    assert [t for t, _ in first] == plain
    assert sum(w.draw.logprob_launches for w in e.workers) > 0
    for (toks, lp), sp in zip(first, sps):
        if sp.logprobs is None:
            assert lp is None
            continue
        assert lp.tokens == toks and len(lp.token_logprobs) == len(lp.top_logprobs) == len(toks)
        for tok, tl, alts in zip(toks, lp.token_logprobs, lp.top_logprobs):
            assert len(alts) == sp.logprobs and all(0 <= i < 1000 for i, _ in alts)
            assert [v for _, v in alts] == sorted((v for _, v in alts), reverse=True)
            assert all(v == tl for i, v in alts if i == tok)
            if sp.greedy and alts:
                assert alts[0] == (tok, tl)
    for _ in range(2):  # captured, then replayed
        assert _records(e.generate_requests(PROMPTS, sps)) == first
    assert sum(w.native_steps for w in e.workers) > native0  # the steady items still go out natively
    assert sum(w.native_changes for w in e.workers) > 0
    eager = _engine(graphs=False)
    assert _records(eager.generate_requests(PROMPTS, sps)) == first
    two = _engine(P=2, transport="devloop")
    try:
        for _ in range(3):
            assert _records(two.generate_requests(PROMPTS, sps)) == first
        assert two.workers[1].draw.logprob_launches > 0 and two.workers[0].draw.logprob_launches == 0
        assert all(w.native_steps > 0 for w in two.workers)
    finally:
        two.shutdown()
