"""Sequence scoring on an MI355X: lm_head_score (csrc/kernels/score.hip)
against float64, an exact integer case, and Engine.score against the engine's
own all-position logits.  Values are gated at 4 x the error of the EXISTING
route on the same inputs (C.linear_f32 logits, float64 log-softmax, against
float64; tools/score_ab.py): the accumulation-order noise of an fp32 GEMM, which
the fused kernel shares.  The +-300 case has its own gate, as that noise scales
with the logits.  Every test prints the largest error it saw before it asserts.
"""
import pytest
import torch

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.runtime.batch import BatchMeta
from llm_sharding_demo_amd.runtime.engine import Engine

pytestmark = pytest.mark.gpu

DEV = "cuda"
# Existing route, largest |log-softmax - float64| per case of CASES, in order (profiles/score_ab.log):
#   7.4e-07, 2.6e-06, 8.4e-06, 1.5e-06, 2.7e-06, 8.9e-06 (pad), 7.1e-05 (big), 8.0e-06, 1.3e-06, 1.4e-06
# The fused kernel on the same cases: 2.1e-07 to 4.9e-06, big 5.5e-05.
# Gates: 4 x 8.921e-06 = 3.569e-05, and for the +-300 case 4 x 7.105e-05 = 2.842e-04.
MEASURED, MEASURED_BIG = 8.921e-06, 7.105e-05
GATE, GATE_BIG = 4 * MEASURED, 4 * MEASURED_BIG

# (T, V, Vp, K, slices, kind): Vp = 1088 ends in half a tile, (257, 320) is a slice shorter than 4
# tiles; kind "big" = logits to +-300, "pad" = weight rows [V, Vp) that would win every argmax
CASES = [
    (1, 1000, 1024, 64, 1, "std"),
    (127, 1000, 1024, 192, 0, "std"),
    (129, 1030, 1088, 1600, 3, "std"),
    (300, 257, 320, 64, 0, "std"),
    (300, 1030, 1088, 192, 1, "std"),
    (129, 257, 320, 1600, 3, "pad"),
    (127, 1030, 1088, 192, 3, "big"),
    (300, 1000, 1024, 1600, 0, "std"),
    (1, 257, 320, 192, 3, "std"),
    (129, 1000, 1024, 64, 1, "std"),
]


@pytest.fixture(scope="module")
def C():
    from llm_sharding_demo_amd.ops.hip import _load
    return _load()


def make_case(T, V, Vp, K, kind, dev=DEV):
    """-> xn [T, K], w [Vp, K] bf16, targets [T] int32, float64 log-softmax [T, V]"""
    g = torch.Generator().manual_seed(1000 * T + Vp + K)
    xn = torch.randn(T, K, generator=g)
    std = 70.0 if kind == "big" else 3.0  # 4.4 sigma of 130 K logits: +-300
    w = torch.randn(Vp, K, generator=g) * (std / K ** 0.5)
    w[V:] = 0
    if kind == "pad":
        xn += 0.5
        d = xn.mean(0)
        w[V:] = 5.0 * d / d.norm()  # logit ~ 2.5 sqrt(K), far above the real columns'
    xn, w = xn.to(torch.bfloat16).to(dev), w.to(torch.bfloat16).to(dev)
    lp = torch.log_softmax(xn.double() @ w[:V].double().T, dim=1)
    t = torch.randint(0, V, (T,), generator=g).to(dev)
    fixed = torch.stack([torch.zeros(T), torch.full((T,), V - 1.0), torch.full((T,), (Vp - 1) // 128 * 128.0),
                         lp.argmax(1).cpu().double()]).long().to(dev)
    r = torch.arange(T, device=dev)
    t = torch.where(r < 8, fixed[r % 4, r], t)
    return xn, w, t.to(torch.int32), lp


def check_ids(top_id, lp, tol, what):
    """argmax against float64 on every row whose top-2 gap exceeds 8 tol; at most 2 % of rows excluded"""
    top2 = lp.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 8 * tol
    print(f"{what}: rows {lp.shape[0]}, excluded from the id check {int((~sure).sum())}")
    assert int((~sure).sum()) <= 0.02 * lp.shape[0]
    assert torch.equal(top_id.long()[sure], lp.argmax(1)[sure])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_kernel_vs_float64(C, case):
    T, V, Vp, K, slices, kind = case
    xn, w, t, lp = make_case(T, V, Vp, K, kind)
    tol = GATE_BIG if kind == "big" else GATE
    tok_lp, top_id, top_lp = C.lm_head_score(xn, w, t, V, slices)
    again = C.lm_head_score(xn, w, t, V, slices)
    e_tok = float((tok_lp.double() - lp.gather(1, t.long().view(-1, 1))[:, 0]).abs().max())
    e_top = float((top_lp.double() - lp.max(1).values).abs().max())
    print(f"score {case}: tok_lp err {e_tok:.3e}, top_lp err {e_top:.3e}, gate {tol:.3e}")
    assert e_tok <= tol and e_top <= tol
    check_ids(top_id, lp, tol, f"score {case}")
    hit = t == top_id
    assert torch.equal(tok_lp.view(torch.int32)[hit], top_lp.view(torch.int32)[hit])
    for a, b in zip((tok_lp, top_id, top_lp), again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("case", [CASES[2], CASES[3]], ids=lambda c: "-".join(map(str, c)))
def test_kernel_exact(C, case):
    """Integer logits, one planted winner per row: 8 leading dimensions carry a
    code (xn +-8, w +-4 on 256 planted columns), so the row's own column scores
    256, any other at most 192, the other dimensions add at most 4.  The gap
    makes lse the winner's logit in fp32: top_lp = 0, tok_lp the exact difference."""
    T, V, Vp, K, slices, _ = case
    g = torch.Generator().manual_seed(K)
    bits = lambda j: ((j.view(-1, 1) >> torch.arange(8)) & 1) * 2 - 1  # noqa: E731
    code = (torch.arange(T) * 37) % 256
    planted = code * V // 256
    xn = torch.randint(-1, 2, (T, K), generator=g)
    xn[:, :8] = 8 * bits(code)
    w = torch.zeros(Vp, K, dtype=torch.long)
    for _ in range(4):
        w[torch.arange(Vp), torch.randint(8, K, (Vp,), generator=g)] = torch.randint(0, 2, (Vp,), generator=g) * 2 - 1
    w[torch.arange(256) * V // 256, :8] = 4 * bits(torch.arange(256))
    w[V:] = 0
    logits = xn @ w[:V].T
    assert torch.equal(logits.argmax(1), planted) and int(logits.abs().max()) <= 260
    t = torch.randint(0, V, (T,), generator=g)
    tok_lp, top_id, top_lp = C.lm_head_score(xn.to(torch.bfloat16).to(DEV), w.to(torch.bfloat16).to(DEV),
                                             t.to(torch.int32).to(DEV), V, slices)
    assert torch.equal(top_id.cpu().long(), planted)
    want = (logits.gather(1, t.view(-1, 1))[:, 0] - logits.max(1).values).float()
    assert torch.equal(tok_lp.cpu() - top_lp.cpu(), want)


def test_refusals(C):
    from llm_sharding_demo_amd.ops.hip import HipBackend
    xn, w, t, _ = make_case(5, 1000, 1024, 64, "std")
    for bad in (-1, 1000):
        tb = t.clone()
        tb[2] = bad
        with pytest.raises(ValueError):
            HipBackend().score_rows(xn, w, tb, 1000)


@pytest.mark.parametrize("model", ["gpt2-test", "llama-test"])
def test_engine_score(model):
    eng = Engine(EngineConfig(model_id=model, num_stages=1, max_batch=4, device="cuda:0", max_seq_len=256))
    V = eng.mcfg.vocab_size
    g = torch.Generator().manual_seed(7)
    seqs = [torch.randint(0, V, (n,), generator=g).tolist() for n in (2, 65, 200)]
    got = eng.score(seqs)
    st = eng.stages[0]
    assert st.backend.name == "hip"
    for seq, sc in zip(seqs, got):
        n = len(seq) - 1
        assert len(sc.token_logprobs) == len(sc.greedy_ids) == len(sc.greedy_logprobs) == n
        meta = BatchMeta.build([eng.kv_slots + 1], [0], [len(seq)], st.device)
        logits = st.forward(meta, torch.tensor(seq, dtype=torch.int32, device=st.device), all_logits=True)[:n].cpu()
        tok, _, top = ref.logprobs(logits, torch.tensor(seq[1:]), [1] * n, V, 1)
        e_tok = float((torch.tensor(sc.token_logprobs) - tok).abs().max())
        e_top = float((torch.tensor(sc.greedy_logprobs) - top[:, 0]).abs().max())
        print(f"{model} len {len(seq)}: tok err {e_tok:.3e}, top err {e_top:.3e}, gate {GATE:.3e}")
        assert e_tok <= GATE and e_top <= GATE
        check_ids(torch.tensor(sc.greedy_ids), torch.log_softmax(logits[:, :V].double(), dim=1), GATE,
                  f"{model} len {len(seq)}")
    eng.generate_ids([seqs[1][:9], seqs[2][:5]], SamplingParams(greedy=True, max_new_tokens=4))
    assert eng.score(seqs) == got  # floats from the same bits compare equal; no NaN in a score
