"""Host-side probe rows for the logprob kernel (csrc/kernels/logprob.hip).

Every case is one fp32 row with one right answer, computed here in float64,
and names the kernel path it forces:

    one | stream        the row fits CH float4 per thread and runs from
                        registers / is re-read through L2
    tau-inf             fewer than n of the 64 thread groups hold a finite
                        logit: the threshold is -inf and every entry a candidate
    rank | overflow     at most / more than LP_CAND candidates: exact rank in
                        LDS / n rounds of block arg-max with exclusion
    nosel               n = 0: no selection at all

`predict_path` derives the path from the row by the kernel's own rules (which
thread visits which index, the n-th largest group maximum, the candidate
count); tests/test_logprobs.py checks every case's declared path against it.
The padding columns [V, ld) hold +inf, then 3e38: counted or selected, they
show at once.
"""
import math

import numpy as np

from .sampler_probes import CH, NT, PAD_FIRST, PAD_REST, ranked

ONE_PASS_MAX = CH * NT * 4
LP_CAND = 1024   # logprob.hip: candidate list in LDS
MAXW = 20        # alternatives per record
NEG = np.float32(-np.inf)
BG = np.float32(-30.0)
SHAPES = {8: 64, 1000: 1024, 50257: 50304, 53249: 53312, 128256: 128256}  # V -> row stride


def blank_row(V, fill=NEG):
    row = np.full(SHAPES[V], fill, dtype=np.float32)
    row[V:] = PAD_REST
    if SHAPES[V] > V:
        row[V] = PAD_FIRST
    return row


def group_of(idx):
    """The 16-thread group (0..63) whose threads visit row index idx."""
    return ((np.asarray(idx) // 4) % NT) // 16


def predict_path(row, V, n):
    x = np.asarray(row, dtype=np.float32)[:V]
    head = "one" if V <= ONE_PASS_MAX else "stream"
    if n == 0:
        return head + ">nosel"
    gmax = np.full(64, -np.inf)
    np.maximum.at(gmax, group_of(np.arange(V)), x.astype(np.float64))
    tau = np.sort(gmax)[::-1][n - 1]
    ncand = int((x >= tau).sum())
    return head + (">tau-inf" if tau == -np.inf else "") + (">overflow" if ncand > LP_CAND else ">rank")


def expect(row, V, n, tok, W=MAXW):
    """(lse, logprob of tok, ids [W], logprobs [W]) in float64; ids in contract
    order, -1 / -inf past min(n, V)."""
    x = np.asarray(row, dtype=np.float32)[:V].astype(np.float64)
    m = x.max()
    lse = -np.inf if m == -np.inf else m + math.log(np.exp(x - m).sum())
    with np.errstate(invalid="ignore"):
        lp = np.where(x == -np.inf, -np.inf, x - lse)
    ids = np.full(W, -1, dtype=np.int64)
    lps = np.full(W, -np.inf)
    k = min(n, V, W)
    if k > 0:
        order = ranked(row, V)[:k]
        ids[:k] = order
        lps[:k] = lp[order]
    return lse, (lp[tok] if 0 <= tok < V else -np.inf), ids, lps


def _case(name, row, V, n, tok, path, **kw):
    return dict(name=name, row=row, V=V, ld=SHAPES[V], n=n, tok=tok, path=path, **kw)


def coverage_cases():
    """-inf everywhere but an anchor at 0.0 and a probe position at 0.0: lse
    must be ln 2 (a skipped probe gives 0, a doubled one ln 3)."""
    out = []
    for V in (50257, 53249):
        head = "one" if V <= ONE_PASS_MAX else "stream"
        pos = [0, 3, 4, V - 1, V - 1 - (V - 1) % 4, NT * 4 - 1, NT * 4]
        if V > ONE_PASS_MAX:
            pos += [ONE_PASS_MAX - 1, ONE_PASS_MAX]  # the streamed path's chunk seam
        for p in sorted(set(pos)):
            anchor = 30 * 64 + 5  # group 30; no probe position shares it
            row = blank_row(V)
            row[anchor] = row[p] = 0.0
            assert group_of(anchor) != group_of(p) and V % 4 == 1
            out.append(_case(f"cover-{V}-{p}", row, V, 2, p, head + ">rank", lse=math.log(2.0),
                             ids=sorted((anchor, p))))
    return out


def single_case():
    """One finite entry: its logprob is exactly 0.0; the four -inf entries that
    fill n = 5 come in index order (tau is -inf: every entry a candidate)."""
    V = 50257
    row = blank_row(V)
    row[31337] = 7.25
    return _case("single-finite", row, V, 5, 31337, "one>tau-inf>overflow", lse=7.25, ids=[31337, 0, 1, 2, 3])


def _spread(V, k, rng, lo=0):
    """k indices in [lo, V), one per thread group, k <= 64."""
    out = []
    for g in rng.permutation(64)[:k]:
        t = int(g) * 16 + int(rng.integers(16))
        c = int(rng.integers((V - 1 - 4 * t) // (4 * NT) + 1))
        base = 4 * (t + c * NT)
        out.append(base + int(rng.integers(min(4, V - base))))
    assert all(lo <= i < V for i in out) and len(set(group_of(out).tolist())) == k
    return sorted(out)


def selection_cases():
    out = []
    rng = np.random.default_rng(11)
    for V in (50257, 53249):
        head = "one" if V <= ONE_PASS_MAX else "stream"
        # eight equal maxima in eight groups, n = 5: the five lowest indices
        row = blank_row(V, BG)
        tie = _spread(V, 8, rng)
        row[tie] = 5.0
        out.append(_case(f"tie-boundary-{V}", row, V, 5, tie[4], head + ">rank", ids=tie[:5]))
        # zeros of both signs above a negative floor: equal, so index order
        row = blank_row(V, BG)
        z = _spread(V, 6, rng)
        row[z] = [0.0, -0.0, -0.0, 0.0, -0.0, 0.0]
        out.append(_case(f"zero-tie-{V}", row, V, 4, z[1], head + ">rank", ids=z[:4]))
        # winners in the last, partial float4 (V % 4 == 1) and at its neighbours
        row = blank_row(V, BG)
        w = [V - 1, V - 2, V - 5]
        row[w] = [3.0, 2.0, 1.0]
        out.append(_case(f"last-float4-{V}", row, V, 3, V - 1, head + ">overflow", ids=w))
        # three finite entries, n = 5: then -inf entries by index
        row = blank_row(V)
        f = _spread(V, 3, rng, lo=8)
        row[f] = [1.0, 3.0, 2.0]
        out.append(_case(f"few-finite-{V}", row, V, 5, f[1], head + ">tau-inf>overflow",
                         ids=[f[1], f[2], f[0], 0, 1]))
    # fewer tokens than alternatives
    row = blank_row(8)
    row[:8] = [0.5, -1.0, 2.0, 2.0, -np.inf, 0.0, -0.0, 1.5]
    out.append(_case("tiny-vocab", row, 8, 20, 3, "one>tau-inf>rank", ids=[2, 3, 7, 0, 5, 6, 1, 4]))
    # a flat row: every entry above the threshold
    V = 50257
    row = blank_row(V, np.float32(1.25))
    out.append(_case("all-equal", row, V, 20, 12345, "one>overflow", lse=1.25 + math.log(V), ids=list(range(20))))
    row = blank_row(V, np.float32(1.25))
    out.append(_case("all-equal-n0", row, V, 0, 7, "one>nosel", lse=1.25 + math.log(V), ids=[]))
    # 16 thread groups hold the whole vocabulary: the 20th group maximum is -inf
    V = 1000
    row = blank_row(V)
    row[:V] = (np.random.default_rng(5).standard_normal(V) * 3).astype(np.float32)
    out.append(_case("v1000-n20", row, V, 20, 999, "one>tau-inf>rank"))
    out.append(_case("v1000-n5", row.copy(), V, 5, 0, "one>rank"))
    return out


def case_list():
    return coverage_cases() + [single_case()] + selection_cases()


def off_rows(B=7):
    """(nlp [B], active [B]) interleaving rows that did not ask (nlp = -1) and
    inactive rows with live ones; live = nlp >= 0 and active."""
    nlp = np.array([3, -1, 0, 5, -1, 20, 2][:B], dtype=np.int32)
    active = np.array([1, 1, 1, 0, 0, 1, 1][:B], dtype=np.int32)
    return nlp, active
