"""GPU sampler with per-row top-p / min-p (csrc/kernels/sample.hip) against the
host reference (ops/reference.py sample): exact equality of the sampled ids.

The kernel's fp32 wave scans and fast exp do not round like the reference's
sequential cumsum, so a row whose cut or draw sits on a boundary may
legitimately differ.  `margins` computes, in float64 on the CPU, how far every
decision of a row is from its boundary; rows closer than 1e-3 are skipped
(worst-case fp32 summation error over 1024 terms ~ 1024 * 2^-24 = 6e-5, fast-exp
error at these arguments < 1e-5: more than a decade of room), and at most 1 row
in 8 of a case may be skipped.  The logits come from a CPU generator, so the
skip count of every case is a property of the seeds, checked without a GPU by
test_margin_skips_within_cap.
"""
import numpy as np
import pytest
import torch

from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.runtime.batch import counter_uniform

DEV = "cuda"
MARGIN = 1e-3
TOPK12 = [1, 2, 5, 40, 63, 64, 65, 200, 1024, 40, 40, 40]
# per row: every listed top_p / min_p value appears, alone and combined
TOPP12 = [0.5, 1.0, 0.8, 0.95, 1.0, 0.8, 0.5, 0.95, 0.8, 1e-6, 1.0, 0.95]
MINP12 = [0.0, 0.3, 0.0, 0.02, 1.0, 0.3, 0.02, 0.0, 0.02, 0.0, 0.0, 0.3]
GREEDY12 = [0] * 10 + [1, 1]


@pytest.fixture(scope="module")
def C():
    from llm_sharding_demo_amd.ops.hip import _load

    return _load()


def _segmax(logits):
    """What linear_f32 writes beside these logits (padding columns included)."""
    B, Vp = logits.shape
    return logits.view(B, Vp // 8, 8).amax(-1).contiguous()


# Logit scale per row.  The margin condition needs neighbouring CDF entries at
# least 2e-3 of the total apart where a cut or the draw lands: the top-k 200 row
# is nearly flat (every entry ~1/200 of the mass; its top-p 0.95 cut lands past
# the second 64-entry chunk), the top-k 1024 row peaked (entries of 1/1024 could
# never pass; its total and min-p count still run over all 16 chunks).
SCALE12 = [2, 2, 2, 2, 2, 2, 2, 0.4, 8, 2, 2, 2]
SEEDS = {"gpt2": 19, "flat": 1, "llama": 23, "small1000": 1, "small2997": 1}


def _case(name, seed=None):
    """CPU tensors of a case: logits [B, Vp] (padding columns 100.0), V and
    the per-row parameters."""
    seed = SEEDS[name] if seed is None else seed
    if name in ("gpt2", "flat"):
        B, V, Vp = 12, 50257, 50304
    elif name == "llama":
        B, V, Vp = 12, 128256, 128256
    elif name == "small1000":
        B, V, Vp = 4, 1000, 1024
    else:
        B, V, Vp = 4, 2997, 3008
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, Vp, generator=g) * (torch.tensor(SCALE12)[:, None] if B == 12 else 2)
    if name == "flat":
        # rows 0-5 flat but for 20 columns: with k >= 40 the threshold is the
        # flat value, every logit a candidate (more than fit) -> the radix
        # path, the k - 20 ties taken by index
        logits[:6] = 0.25
        for r in range(6):
            cols = torch.randperm(V, generator=g)[:20]
            logits[r, cols] += torch.rand(20, generator=g) * 3
    logits[:, V:] = 100.0
    if B == 12:
        p = dict(temp=torch.linspace(0.5, 1.5, B), topk=TOPK12, top_p=TOPP12, min_p=MINP12, greedy=GREEDY12)
    else:
        p = dict(temp=torch.tensor([0.6, 1.0, 0.6, 1.0]), topk=[20, 40, 64, 200], top_p=[0.8, 0.95, 1e-6, 0.5],
                 min_p=[0.0, 0.02, 0.0, 0.3], greedy=[0] * 4)
    p = dict(temp=p["temp"].float(), topk=torch.tensor(p["topk"], dtype=torch.int32),
             top_p=torch.tensor(p["top_p"], dtype=torch.float32), min_p=torch.tensor(p["min_p"], dtype=torch.float32),
             greedy=torch.tensor(p["greedy"], dtype=torch.int32),
             seeds=torch.arange(B, dtype=torch.int64) * 104729 + 11, step=torch.arange(B, dtype=torch.int64) + 2)
    return logits, V, p


def margins(logits, V, p):
    """Per row: True when every decision of the row (top-p cut, min-p cut,
    draw) is at least MARGIN away from its boundary, in float64."""
    B = logits.shape[0]
    u = counter_uniform(p["seeds"], p["step"]).double()
    ok = []
    for r in range(B):
        if int(p["greedy"][r]):
            ok.append(True)
            continue
        k = min(int(p["topk"][r]), V)
        v = torch.sort(logits[r, :V].double(), descending=True, stable=True).values[:k] / float(p["temp"][r])
        e = torch.exp(v - v[0])
        c = torch.cumsum(e, 0)
        total = float(c[-1])
        tp, mp = float(p["top_p"][r]), float(p["min_p"][r])
        m = []
        n_p = k
        if tp < 1.0:
            hit = torch.nonzero(c >= tp * total)
            n_p = int(hit[0]) + 1 if hit.numel() else k
            m.append(abs(float(c[n_p - 1]) - tp * total) / total)
            if n_p >= 2:
                m.append(abs(float(c[n_p - 2]) - tp * total) / total)
        n_m = k
        if mp > 0.0:
            n_m = int((e >= mp).sum())
            # e_0 = exp(0) is exactly 1 on the host and on the device: no
            # rounding boundary even at min_p = 1, so it is left out (stricter)
            if k > 1:
                m.append(float((e[1:] - mp).abs().min()) / max(mp, 1e-30))
        n = max(1, min(n_p, n_m))
        target = float(u[r]) * float(c[n - 1])
        m.append(float((c[:n] - target).abs().min()) / total)
        ok.append(min(m) >= MARGIN)
    return ok


CASES = ["gpt2", "llama", "small1000", "small2997", "flat"]


@pytest.mark.parametrize("case", CASES)
def test_margin_skips_within_cap(case):
    """The seeds of every case keep the reference's own decisions away from
    their boundaries in all but at most 1 row in 8 (no GPU needed)."""
    logits, V, p = _case(case)
    ok = margins(logits, V, p)
    assert ok.count(False) * 8 <= len(ok), ok


@pytest.mark.gpu
@pytest.mark.parametrize("seg", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_sampler_top_p_min_p(C, case, seg):
    logits, V, p = _case(case)
    B = logits.shape[0]
    ok = margins(logits, V, p)
    assert ok.count(False) * 8 <= B, ok
    exp = ref.sample(logits, p["temp"], p["topk"], p["greedy"], counter_uniform(p["seeds"], p["step"]), V,
                     p["top_p"], p["min_p"]).tolist()
    # a nucleus of 1e-6 is the argmax (lowest index), whatever else the row asks for
    amax = logits[:, :V].argmax(1).tolist()
    tiny = [r for r in range(B) if float(p["top_p"][r]) < 1e-5]
    assert tiny and all(exp[r] == amax[r] for r in tiny)
    d = {k: v.to(DEV) for k, v in p.items()}
    lg = logits.to(DEV)
    sm = _segmax(lg) if seg else None
    rows = [r for r in range(B) if ok[r]]
    out = C.sample(lg, V, d["temp"], d["topk"], d["greedy"], d["seeds"], d["step"], sm, d["top_p"], d["min_p"])
    got = out.cpu().tolist()
    print("sampled", got, "expected", exp, "compared rows", rows)
    assert [got[r] for r in rows] == [exp[r] for r in rows]
    assert all(0 <= t < V for t in got)
    assert all(got[r] == amax[r] for r in tiny)
    # only one of the two vectors given: the other cut is off
    only_p = ref.sample(logits, p["temp"], p["topk"], p["greedy"], counter_uniform(p["seeds"], p["step"]), V,
                        p["top_p"], None).tolist()
    ok_p = margins(logits, V, dict(p, min_p=torch.zeros(B)))
    got_p = C.sample(lg, V, d["temp"], d["topk"], d["greedy"], d["seeds"], d["step"], sm, d["top_p"]).cpu().tolist()
    assert [got_p[r] for r in range(B) if ok_p[r]] == [only_p[r] for r in range(B) if ok_p[r]]
    # decode-step form: same draws into a slice, counters and positions advanced by `active`
    buf = torch.full((B + 3,), -1, dtype=torch.int32, device=DEV)
    st2 = d["step"].clone()
    C.sample_into(lg, V, d["temp"], d["topk"], d["greedy"], d["seeds"], st2, buf[:B], None, None, sm,
                  d["top_p"], d["min_p"])
    assert buf[:B].cpu().tolist() == got and buf[B:].cpu().tolist() == [-1] * 3
    assert torch.equal(st2, d["step"] + 1)
    act = (torch.arange(B, device=DEV) % 3 != 0).int()
    pos = torch.arange(B, dtype=torch.int32, device=DEV) + 100
    st3 = d["step"].clone()
    C.sample_into(lg, V, d["temp"], d["topk"], d["greedy"], d["seeds"], st3, buf[:B], act, pos, sm,
                  d["top_p"], d["min_p"])
    assert buf[:B].cpu().tolist() == got and torch.equal(st3, d["step"] + act)
    assert torch.equal(pos, torch.arange(B, device=DEV).int() + 100 + act)


@pytest.mark.gpu
def test_default_vectors_equal_null(C):
    """top_p = 1 / min_p = 0 given as vectors take the uncut path: the ids of
    the call without them, on every tail."""
    logits, V, p = _case("gpt2")
    d = {k: v.to(DEV) for k, v in p.items()}
    lg = logits.to(DEV)
    B = lg.shape[0]
    one, zero = torch.ones(B, device=DEV), torch.zeros(B, device=DEV)
    for sm in (None, _segmax(lg)):
        a = C.sample(lg, V, d["temp"], d["topk"], d["greedy"], d["seeds"], d["step"], sm)
        b = C.sample(lg, V, d["temp"], d["topk"], d["greedy"], d["seeds"], d["step"], sm, one, zero)
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("words", [12, 14])
@pytest.mark.parametrize("cap,b,n,first,last", [(256, 256, 256, True, True), (256, 128, 77, True, True),
                                                (300, 64, 0, True, False), (2048, 2048, 1500, False, True),
                                                (8, 8, 3, False, False), (8, 8, 3, False, True)])
def test_apply_rows_top_p_min_p(C, cap, b, n, first, last, words):
    """apply_rows with the 14-word record: the top-p / min-p columns scattered
    into their row vectors (pad rows 1.0 / 0.0, rows past b untouched) beside
    everything the 12-word record does; the 12-word record, with the smaller
    buffer, still accepted and leaving them alone."""
    g = torch.Generator().manual_seed(cap + b + n)
    scratch = 12345
    ri = lambda lo, hi, k: torch.randint(lo, hi, (k,), generator=g)  # noqa: E731
    slot, pos, topk, greedy, src = ri(0, 10000, n), ri(0, 4096, n), ri(1, 64, n), ri(0, 2, n), ri(0, cap, n)
    temp = torch.rand(n, generator=g) + 0.1
    topp, minp = torch.rand(n, generator=g) * 0.9 + 0.1, torch.rand(n, generator=g)
    seed, step = ri(0, 1 << 62, n), ri(0, 1 << 40, n)
    a = np.zeros((12 if words == 14 else 10) * cap + 1, np.int32)
    a[: 4 * cap].view(np.int64)[:n] = seed.numpy()
    a[: 4 * cap].view(np.int64)[cap: cap + n] = step.numpy()
    a[4 * cap] = n
    f0 = 4 * cap + 1
    cols = [slot, pos, temp.float(), topk, greedy, src] + ([topp.float(), minp.float()] if words == 14 else [])
    for k, v in enumerate(cols):
        v = v.numpy()
        a[f0 + k * cap: f0 + k * cap + n] = v.view(np.int32) if v.dtype == np.float32 else v
    i32 = dict(dtype=torch.int32, device=DEV)
    buf = torch.from_numpy(a).to(DEV)
    t = dict(slots=torch.full((cap,), -1, **i32), pos=torch.full((cap,), -1, **i32), act=torch.full((cap,), -1, **i32))
    if last:
        t.update(temp=torch.zeros(cap, device=DEV), topk=torch.zeros(cap, **i32), greedy=torch.zeros(cap, **i32),
                 seeds=torch.full((cap,), -1, dtype=torch.int64, device=DEV),
                 sstep=torch.full((cap,), -1, dtype=torch.int64, device=DEV),
                 topp=torch.full((cap,), -1.0, device=DEV), minp=torch.full((cap,), -1.0, device=DEV))
    tin0 = ri(0, 50000, cap).to(torch.int32)
    tin = tin0.to(DEV)
    ptr = lambda k: t[k].data_ptr() if k in t else 0  # noqa: E731
    rec = [cap, scratch, buf.data_ptr(), ptr("slots"), ptr("pos"), ptr("act"), ptr("temp"), ptr("topk"),
           ptr("greedy"), ptr("seeds"), ptr("sstep"), tin.data_ptr() if first else 0]
    if words == 14:
        rec += [ptr("topp"), ptr("minp")]
    C.apply_rows(torch.tensor(rec, dtype=torch.int64), b)
    torch.cuda.synchronize()
    pad = b - n
    cat = lambda v, fill: torch.cat([v.to(torch.int64), torch.full((pad,), fill, dtype=torch.int64)])  # noqa: E731
    assert torch.equal(t["slots"][:b].cpu().long(), cat(slot, scratch))
    assert torch.equal(t["pos"][:b].cpu().long(), cat(pos, 0))
    assert torch.equal(t["act"][:b].cpu().long(), cat(torch.ones(n, dtype=torch.int64), 0))
    assert (t["slots"][b:] == -1).all()
    if last:
        assert torch.equal(t["temp"][:b].cpu(), torch.cat([temp.float(), torch.ones(pad)]))
        assert torch.equal(t["topk"][:b].cpu().long(), cat(topk, 1))
        assert torch.equal(t["greedy"][:b].cpu().long(), cat(greedy, 1))
        assert torch.equal(t["seeds"][:b].cpu(), cat(seed, 0))
        assert torch.equal(t["sstep"][:b].cpu(), cat(step, 0))
        if words == 14:
            assert torch.equal(t["topp"][:b].cpu(), torch.cat([topp.float(), torch.ones(pad)]))
            assert torch.equal(t["minp"][:b].cpu(), torch.cat([minp.float(), torch.zeros(pad)]))
            assert (t["topp"][b:] == -1).all() and (t["minp"][b:] == -1).all()
        else:
            assert (t["topp"] == -1).all() and (t["minp"] == -1).all()
    want = tin0.clone()
    if first:
        want[:b] = tin0[cat(src, 0)]
    assert torch.equal(tin.cpu(), want)
