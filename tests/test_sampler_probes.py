"""The sampler probes of tests/sampler_probes.py, checked on the host: every
case of tests/test_sampler_exact_gpu.py builds (no row skipped), takes the path
it names, and is accepted by the clean fp32 emulation; every fault knob of the
emulation is rejected by the probe meant for it; the random 12-row cases of
the older tests let 7 of the 16 through (pinned); and ops/reference.py
`sample` follows the contract order on boundary ties and signed zeros."""
import numpy as np
import pytest
import torch

from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.runtime.batch import counter_uniform
from . import sampler_probes as sp

CASES = sp.case_list()
BUILD = dict(CASES)


def test_extreme_uniforms():
    u = counter_uniform(torch.tensor([sp.U_SEED] * 2), torch.tensor([sp.U0_STEP, sp.U1_STEP]))
    assert float(u[0]) == 0.0 and float(u[1]) == 1.0 - 2.0 ** -24 == sp.U_MAX
    # fl(u m) lies in (m - 1, m) for every count of equal entries the probes use
    for m in (2, 40, 64, 65, 127, 128, 1000, 1024):
        t = np.float32(np.float32(sp.U_MAX) * np.float32(m))
        assert m - 1 < t < m


@pytest.mark.parametrize("stream", [0, 1, 3, 5])
def test_pick_step_covers_1024_intervals(stream):
    """2^18 counters reach the central half of each of 1024 equal intervals,
    with negative seeds, seeds above 2^32 and counter bases at 2^40."""
    seed, base = sp.STREAMS[stream]
    for j in range(1024):
        lo, hi = j / 1024, (j + 1) / 1024
        step, u = sp.pick_step(seed, lo, hi, base)
        assert base <= step < base + (1 << 18) and u == sp.uniform(seed, step)
        assert lo + 0.25 / 1024 <= u < hi - 0.25 / 1024


def test_ranked_is_the_contract_order():
    row = np.array([1.0, -0.0, 2.0, 0.0, 2.0, -0.0, -np.inf, 0.0], dtype=np.float32)
    assert sp.ranked(row, 8).tolist() == [2, 4, 0, 1, 3, 5, 7, 6]
    assert sp.ranked(row, 5).tolist() == [2, 4, 0, 1, 3]
    # torch.topk does not give it: the reason no expected id comes from there
    assert torch.topk(torch.tensor([1.0, 1, 1, 1, 2]), 3).indices.tolist() != [4, 0, 1]


@pytest.mark.parametrize("cid", [c for c, _ in CASES])
def test_case_builds_names_its_path_and_emulates_clean(cid):
    c = BUILD[cid]()
    assert c.rows and all(len(b) == c.Vp for b in c.bases)
    assert c.paths() == [r["path"] for r in c.rows]
    assert c.emulated() == c.expect()
    assert all(0 <= e < c.V for e in c.expect())
    for r in c.rows:  # every expected id is the contract order's, and the padding would outrank it
        if r["greedy"]:
            assert r["expect"] == int(sp.ranked(c.bases[r["base"]], c.V)[0])
    if c.Vp > c.V:
        assert all(np.all(b[c.V:] > b[:c.V].max()) and np.isinf(b[c.V]) for b in c.bases)


def test_every_path_has_a_case():
    seen = set()
    for _, build in CASES:
        seen |= set(build().paths())
    assert seen == sp.ALL_PATHS


# the probe meant for each knob: every listed case must reject it
MEANT = {
    "drop_kth": ["sweep-k65-plain", "sweep-k129-plain", "sweep-k1024-plain", "zeros-plain"],
    "admit_k1": ["sweep-k65-plain", "sweep-k64-plain", "sweep-k200-plain"],
    "tie_highest": ["ties-plain", "ties-seg"],
    "zero_by_key": ["zeros-plain", "zeros-seg"],
    "pad_admitted": ["sweep-k3-plain", "sweep-k64-seg", "sweep-k63-plain"],
    "drop_partial_float4": ["sweep-k64-plain", "shape-53249-53256-plain-k40-spread-tight"],
    "drop_partial_segment": ["sweep-k64-seg", "sweep-k3-seg"],
    "seg_gt": ["groups-seg", "sweep-k63-seg"],
    "low8_ignored": ["sweep-k200-plain", "sweep-k127-plain", "sweep-k1024-plain"],
    "pair_swap": ["sweep-k2-plain", "sweep-k63-plain", "sweep-k128-plain"],
    "chunk_carry_lost": ["sweep-k129-plain", "sweep-k200-plain", "sweep-k1024-plain"],
    "np_plus": ["cut-k64-plain", "cut-k64-seg", "cut-k128-plain", "cut-k200-plain", "cut-k1024-plain"],
    "np_minus": ["cut-k64-plain", "cut-k64-seg", "cut-k128-plain", "cut-k200-plain", "cut-k1024-plain"],
    "minp_gt": ["cut-k64-plain", "cut-k128-plain", "cut-k200-plain", "cut-k1024-plain"],
    "u_next": ["sweep-k3-plain", "sweep-k65-plain", "cut-k200-plain"],
    "greedy_tie_highest": ["greedy-plain", "greedy-seg"],
}


@pytest.mark.parametrize("fault", sp.FAULTS)
def test_fault_is_rejected_by_its_probe(fault):
    assert set(MEANT) == set(sp.FAULTS)
    for cid in MEANT[fault]:
        c = BUILD[cid]()
        got = c.emulated(faults=(fault,))
        wrong = [i for i, (g, e) in enumerate(zip(got, c.expect())) if g != e]
        assert wrong, f"{cid} accepts {fault}"


def test_rank_sweeps_pin_the_boundary_rows():
    """The row that gives a selector fault away is the one at rank k - 1."""
    for cid, fault in (("sweep-k65-plain", "drop_kth"), ("sweep-k65-plain", "admit_k1"),
                       ("sweep-k200-plain", "low8_ignored")):
        c = BUILD[cid]()
        got = c.emulated(faults=(fault,))
        assert got[-1] != c.expect()[-1]


def _random_cases():
    """The older tests' 12-row random cases, rebuilt on the host: gpt2 of
    test_sampler_topp_gpu.py (as is) and the `random` and `quantized` rows
    of test_kernels_gpu.py test_sampler_fast_path_and_ties (same shape, scale,
    parameters and counters; the logits from a host generator)."""
    from .test_sampler_topp_gpu import _case

    lg, V, p = _case("gpt2")
    out = [("gpt2", lg.numpy(), V, p)]
    for name in ("random", "quantized"):
        g = torch.Generator().manual_seed(5)
        lg = torch.randn(12, 50304, generator=g) * 2
        if name == "quantized":
            lg = (lg * 16).round() / 16
        lg[:, 50257:] = 100.0
        B = 12
        p = dict(temp=torch.linspace(0.5, 1.5, B), greedy=torch.tensor([0] * 11 + [1]),
                 topk=torch.tensor([1, 2, 5, 16, 40, 63, 64, 65, 40, 40, 200, 40]),
                 seeds=torch.arange(B, dtype=torch.int64) * 104729 + 11, step=torch.arange(B, dtype=torch.int64),
                 top_p=torch.ones(B), min_p=torch.zeros(B))
        out.append((name, lg.numpy(), 50257, p))
    return out


def _ids(lg, V, p, seg, faults):
    return [sp.emulate(lg[r], V, int(p["topk"][r]), float(p["temp"][r]), int(p["seeds"][r]), int(p["step"][r]),
                       float(p["top_p"][r]), float(p["min_p"][r]), seg, bool(p["greedy"][r]), faults)
            for r in range(lg.shape[0])]


# measured: the knobs that change no id of any of the three random cases, with or without segment maxima
LET_THROUGH = {"tie_highest", "zero_by_key", "drop_partial_float4", "drop_partial_segment", "low8_ignored",
               "minp_gt", "greedy_tie_highest"}


def test_random_rows_let_seven_faults_through():
    """How many of the 16 knobs the random 12-row cases cannot see: 7 (the
    boundary ties, signed zeros, partial float4 / segment, low key bits, the
    min-p comparison and the greedy tie)."""
    cases = _random_cases()
    through = set()
    for fault in sp.FAULTS:
        if all(_ids(lg, V, p, seg, (fault,)) == _ids(lg, V, p, seg, ()) for _, lg, V, p in cases
               for seg in (False, True)):
            through.add(fault)
    print("let through:", sorted(through))
    assert through == LET_THROUGH
    assert len(through) == 7


def _ref_ids(c):
    t = c.tensors()
    u = counter_uniform(t["seeds"], t["step"])
    return ref.sample(t["logits"], t["temp"], t["topk"], t["greedy"], u, c.V, t["top_p"], t["min_p"]).tolist()


@pytest.mark.parametrize("cid", ["ties-plain", "zeros-plain", "ties-seg", "zeros-seg", "greedy-plain",
                                 "sweep-k63-plain", "sweep-k65-plain", "cut-k64-plain", "cut-k200-plain"])
def test_reference_sample_follows_the_contract_order(cid):
    """ops/reference.py sample on boundary ties, signed zeros at the k
    boundary, ulp ladders and plateau cuts: the ranked-based ids.  (With
    torch.topk in it the ties and zeros cases failed.)"""
    c = BUILD[cid]()
    assert _ref_ids(c) == c.expect()


def _sample_topk(logits, temperature, top_k, uniforms, vocab):
    """The uncut draw of ref.sample as it was, through torch.topk."""
    out = []
    for r in range(logits.shape[0]):
        k = int(top_k[r])
        vals, idx = torch.topk(logits[r, :vocab].float() / float(temperature[r]), k)
        order = sorted(range(k), key=lambda j: (-float(vals[j]), int(idx[j])))
        vals, idx = vals[order], idx[order]
        c = torch.cumsum(torch.softmax(vals, dim=-1), 0)
        u = float(uniforms[r]) * float(c[-1])
        out.append(int(idx[int(torch.searchsorted(c, torch.tensor([u], dtype=c.dtype)).clamp(max=k - 1))]))
    return out


def test_reference_sample_unchanged_without_boundary_ties():
    """Continuous random rows have no ties: the stable-sort selection returns
    what the torch.topk one did, and the sorted values are bit-identical."""
    g = torch.Generator().manual_seed(3)
    lg = torch.randn(24, 50304, generator=g) * 3
    topk = torch.tensor([1, 2, 5, 40, 63, 64, 65, 200, 1024, 40, 40, 40] * 2)
    temp = torch.linspace(0.5, 1.5, 24)
    u = torch.rand(24, generator=g)
    for r in range(24):
        k = int(topk[r])
        a = torch.topk(lg[r, :50257] / float(temp[r]), k)
        b = torch.sort(lg[r, :50257], descending=True, stable=True)
        assert torch.equal(a.indices, b.indices[:k])
        assert torch.equal(a.values.view(torch.int32), (b.values[:k] / float(temp[r])).view(torch.int32))
    got = ref.sample(lg, temp, topk, torch.zeros(24, dtype=torch.int32), u, 50257).tolist()
    assert got == _sample_topk(lg, temp, topk, u, 50257)


def test_pen_hash_helpers():
    toks = sp.same_bucket_tokens(4099, 6, 63, 20)
    assert len(set(toks.tolist())) == 20 and all(sp.pen_hash(t, 6) == 63 for t in toks)
    toks = sp.same_bucket_tokens(131072, 14, 16383, 6)
    assert all(sp.pen_hash(t, 14) == 16383 for t in toks)
