"""The on-device sampler (csrc/kernels/sample.hip) on rows with exactly one
right id: tests/sampler_probes.py builds them (rank, cut and extreme-uniform
probes; ulp ladders, boundary ties, signed zeros, -inf tails; every shape at
which the kernel takes another branch) and names the path each row takes;
tests/test_sampler_probes.py checks the builders, the paths and the fault
coverage on the host.  Every comparison here is equality of ids with
`ranked`-based expectations: no tolerance, no skipped row.

Measured on an MI355X: the 54 tests take 3.2 s together, building the cases
included (3423 rows in the 47 cases of test_exact_ids); the slowest are
test_sample_into_matches_sample[sweep-k65-plain] 0.27 s, the first launch
(sweep-k1-plain) 0.18 s, the interleaved launch 0.09 s, the 53248-wide shape
0.09 s, penalize + sample 0.08 s and the 1024-row sweeps 0.05 s each; every
other test is under 0.03 s.
"""
import functools
import time

import numpy as np
import pytest
import torch

from . import sampler_probes as sp

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = sp.case_list()
BUILD = dict(CASES)


@pytest.fixture(scope="module")
def C():
    from llm_sharding_demo_amd.ops.hip import _load

    return _load()


def _launch(C, c, t=None, cut=None, logits=None):
    """Ids of one launch of case c (cut: pass the top_p / min_p vectors)."""
    t = c.tensors() if t is None else t
    d = {k: (v.to(DEV) if v is not None else None) for k, v in t.items()}
    lg = d["logits"] if logits is None else logits
    cut = c.cut if cut is None else cut
    out = C.sample(lg, c.V, d["temp"], d["topk"], d["greedy"], d["seeds"], d["step"], d["segmax"],
                   d["top_p"] if cut else None, d["min_p"] if cut else None)
    assert torch.equal(d["step"].cpu(), t["step"])  # `sample` leaves the counters alone
    return out.cpu().tolist()


def _diff(got, c):
    exp = c.expect()
    bad = [(i, c.rows[i]["path"], c.rows[i]["k"], got[i], exp[i]) for i in range(len(exp)) if got[i] != exp[i]]
    return bad[:8], len(bad)


@pytest.mark.parametrize("cid", [cid for cid, _ in CASES])
def test_exact_ids(C, cid):
    """Every row returns the ranked-based id it was built for; with top_p = 1 /
    min_p = 0 vectors the ids are those of null vectors."""
    c = BUILD[cid]()
    t = c.tensors()
    t0 = time.perf_counter()
    got = _launch(C, c, t)
    print(f"{cid}: {len(c.rows)} rows, paths {sorted(set(c.paths()))}, {time.perf_counter() - t0:.3f} s")
    assert _diff(got, c) == ([], 0)
    if not c.cut:
        assert _launch(C, c, t, cut=True) == got
    else:  # one cut given as a null vector: rows whose other cut is off keep their id
        only_p = [i for i, r in enumerate(c.rows) if r["min_p"] == 0.0]
        only_m = [i for i, r in enumerate(c.rows) if r["top_p"] == 1.0]
        assert only_p and only_m
        d = {k: (v.to(DEV) if v is not None else None) for k, v in t.items()}
        a = C.sample(d["logits"], c.V, d["temp"], d["topk"], d["greedy"], d["seeds"], d["step"], d["segmax"],
                     d["top_p"], None).cpu().tolist()
        b = C.sample(d["logits"], c.V, d["temp"], d["topk"], d["greedy"], d["seeds"], d["step"], d["segmax"],
                     None, d["min_p"]).cpu().tolist()
        assert [a[i] for i in only_p] == [got[i] for i in only_p]
        assert [b[i] for i in only_m] == [got[i] for i in only_m]


def test_every_path_is_run():
    """The cases above cover every path predict_path can name (a property of
    the builders; asserted here beside the launches that rely on it)."""
    seen = set()
    for _, build in CASES:
        seen |= set(build().paths())
    assert seen == sp.ALL_PATHS


@functools.lru_cache(maxsize=None)
def _mixed(seg):
    """Rows of every path of one shape, interleaved in shuffled order."""
    s = "seg" if seg else "plain"
    V, Vp = sp.SEG_SHAPE if seg else sp.PLAIN_SHAPE
    parts = [f"sweep-k63-{s}", f"sweep-k64-{s}", "sweep-k65-plain", "sweep-k129-plain", "sweep-k1024-plain",
             f"ties-{s}", f"zeros-{s}", f"extreme-{s}", f"groups-{s}", f"greedy-{s}", f"cut-k64-{s}",
             "cut-k200-plain"]
    m = sp.Case(f"mixed_{s}", V, Vp, seg)
    for cid in parts:
        c = BUILD[cid]()
        if (c.V, c.Vp) != (V, Vp):
            continue
        base0 = len(m.bases)
        m.bases += c.bases
        rows = c.rows if len(c.rows) <= 40 else c.rows[::max(1, len(c.rows) // 12)]
        for r in rows:
            m.rows.append(dict(r, base=r["base"] + base0))
    order = np.random.default_rng(7).permutation(len(m.rows))
    m.rows = [m.rows[i] for i in order]
    return m


@pytest.mark.parametrize("seg", [False, True])
def test_interleaved_paths_and_strided_view(C, seg):
    """One launch with rows of every path in shuffled order returns the ids of
    the separate launches; so does a launch on a row-strided view of a wider
    poisoned buffer."""
    m = _mixed(seg)
    assert m.paths() == [r["path"] for r in m.rows]
    s = ("seg" if seg else "one")
    want = {"greedy", f"{s}>rank", f"{s}>bitonic", f"{s}>overflow>radix>rank", "radix>rank", "radix>bitonic"}
    assert want <= set(m.paths())
    t = m.tensors()
    got = _launch(C, m, t)
    assert _diff(got, m) == ([], 0)
    B = len(m.rows)
    wide = torch.full((B, m.Vp + 64), float("inf"), device=DEV)
    wide[:, m.Vp:] = float("nan")
    view = wide[:, :m.Vp]
    view.copy_(t["logits"])
    assert view.stride(0) == m.Vp + 64 and not view.is_contiguous()
    assert _launch(C, m, t, logits=view) == got
    assert torch.equal(view.cpu().view(torch.int32), t["logits"].view(torch.int32))


@pytest.mark.parametrize("cid", ["sweep-k65-plain", "sweep-k64-seg", "cut-k200-plain"])
def test_sample_into_matches_sample(C, cid):
    c = BUILD[cid]()
    t = c.tensors()
    got = _launch(C, c, t)
    assert got == c.expect()
    d = {k: (v.to(DEV) if v is not None else None) for k, v in t.items()}
    B = len(c.rows)
    tp, mp = (d["top_p"], d["min_p"]) if c.cut else (None, None)
    buf = torch.full((B + 5,), -7, dtype=torch.int32, device=DEV)
    act = (torch.arange(B, device=DEV) % 3 != 0).int()
    pos = torch.arange(B, dtype=torch.int32, device=DEV) + 100
    st = d["step"].clone()
    C.sample_into(d["logits"], c.V, d["temp"], d["topk"], d["greedy"], d["seeds"], st, buf[2:B + 2], act, pos,
                  d["segmax"], tp, mp)
    assert buf[2:B + 2].cpu().tolist() == got
    assert buf[:2].cpu().tolist() == [-7, -7] and buf[B + 2:].cpu().tolist() == [-7] * 3
    assert torch.equal(st, d["step"] + act) and torch.equal(pos, torch.arange(B, device=DEV).int() + 100 + act)
    st2 = d["step"].clone()
    C.sample_into(d["logits"], c.V, d["temp"], d["topk"], d["greedy"], d["seeds"], st2, buf[2:B + 2], None, None,
                  d["segmax"], tp, mp)
    assert buf[2:B + 2].cpu().tolist() == got and torch.equal(st2, d["step"] + 1)


# ---- penalties before the draw

PV = 131072   # 16384 segments: the longest row of the segment path
PL = 8192
PRES, FREQ = 0.5, 0.25  # dyadic, like the logits: every product, sum and difference is exact
TOPS = np.array([2.875, 2.75, 2.625, 2.5, 2.375, 2.25], dtype=np.float32)
# (table bits, home bucket, history length): all tokens of a row share one home bucket; bucket 2^bits - 1
# makes the probe chain wrap past the table's end
PEN_ROWS = [(6, 63, 31), (6, 10, 32), (14, 16383, 8191), (14, 100, 8191), (14, 5000, 8191)]


@functools.lru_cache(maxsize=None)
def _pen_case():
    rng = np.random.default_rng(11)
    B = len(PEN_ROWS)
    lg = np.empty((B, PV), dtype=np.float32)
    hist = rng.integers(0, PV, size=(B + 1, PL)).astype(np.int32)  # valid tokens everywhere: none may be read
    counts, want, toks_of = [], np.empty_like(lg), []
    for r, (bits, bucket, n) in enumerate(PEN_ROWS):
        ntok = 20 if bits == 6 else 7
        toks = sp.same_bucket_tokens(PV, bits, bucket, ntok)
        row = sp.blank_row(PV, PV)
        sp.add_floors(row, PV, 64, True, rng, toks)
        row[toks[:6]] = TOPS  # the argmax is toks[0]
        if r == 4:  # one token 8191 times
            h = np.full(n, toks[0])
        else:       # toks[0] three times, every other token once or twice, the last one the rest
            h = np.concatenate([[toks[0]] * 3] + [[t] * (1 + i % 2) for i, t in enumerate(toks[1:-1])])
            h = np.concatenate([h, np.full(n - len(h), toks[-1])])
        assert len(h) == n and (1 << bits) == max(64, 1 << int(np.ceil(np.log2(2 * n))))
        hist[r + 1, :n] = rng.permutation(h)
        new = row.astype(np.float64)
        for tok, cnt in zip(*np.unique(h, return_counts=True)):
            new[tok] -= PRES + FREQ * float(cnt)
        assert np.array_equal(new.astype(np.float32).astype(np.float64), new)  # closed form, exact in fp32
        lg[r], want[r] = row, new.astype(np.float32)
        counts.append(n)
        toks_of.append(toks)
    return lg, hist, counts, want, toks_of


def test_penalize_then_sample_exact(C):
    """penalize on histories whose tokens share one home bucket of the LDS
    table (with and without a chain wrapping past its end), at table sizes 64
    and 16384, one token counted 8191 times: logits and segment maxima bit-equal
    to the closed form; then a rank probe on the penalised rows through the
    segment-maxima path, where the former argmax's segment no longer leads."""
    lg, hist, counts, want, toks_of = _pen_case()
    B = lg.shape[0]
    for r, (bits, bucket, n) in enumerate(PEN_ROWS):
        assert all(sp.pen_hash(t, bits) == bucket for t in toks_of[r])
    d_lg = torch.from_numpy(lg).to(DEV)
    sm0 = d_lg.view(B, PV // 8, 8).amax(-1).contiguous()
    d_sm = sm0.clone()
    C.penalize(d_lg, PV, torch.from_numpy(hist).to(DEV), torch.arange(1, B + 1, dtype=torch.int32, device=DEV),
               torch.tensor(counts, dtype=torch.int64, device=DEV), torch.full((B,), PRES, device=DEV),
               torch.full((B,), FREQ, device=DEV), d_sm)
    torch.cuda.synchronize()
    got, got_sm = d_lg.cpu().numpy(), d_sm.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    want_sm = want.reshape(B, PV // 8, 8).max(-1)
    assert np.array_equal(got_sm.view(np.int32), want_sm.view(np.int32))
    assert want[4, toks_of[4][0]] == np.float32(2.875 - (PRES + FREQ * 8191))
    c = sp.Case("penalised", PV, PV, True)
    for r in range(B):
        a = int(toks_of[r][0])
        assert int(lg[r].argmax()) == a and sm0[r].argmax().item() == a // 8
        assert want_sm[r, a // 8] < want_sm[r].max()  # the former argmax's segment no longer leads
        b = c.base(want[r])
        for j in range(5):
            c.add_rank(b, 5, j, "seg>rank", T=4.0)
    assert c.paths() == [r["path"] for r in c.rows]
    t = c.tensors()
    rows = torch.tensor([r["base"] for r in c.rows], device=DEV)
    d = {k: v.to(DEV) for k, v in t.items() if k not in ("logits", "segmax")}
    out = C.sample(d_lg[rows].contiguous(), PV, d["temp"], d["topk"], d["greedy"], d["seeds"], d["step"],
                   d_sm[rows].contiguous())
    assert _diff(out.cpu().tolist(), c) == ([], 0)
