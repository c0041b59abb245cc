"""Exact probes for the on-device sampler of csrc/kernels/sample.hip (numpy /
torch on the host; importable without a GPU).

A random row with one uniform reveals only the entry that uniform lands on,
and the k-th entry of a peaked top-k list has almost no mass: a selector that
drops the k-th winner, admits the (k+1)-th or breaks a boundary tie by the
wrong index passes such a test with near certainty (tests/test_sampler_probes.py
pins how many of the fault knobs below the random 12-row cases let through).
The cases built here have one right id per row, and every row says which of
the kernel's data-dependent paths it takes.

contract  `ranked(row, V)`: value descending by numeric comparison (-0.0 ==
          +0.0), index ascending -- a stable sort of row[:V].  Every expected
          id comes from it, never from torch.topk (whose choice among equal
          values at the k boundary is unspecified).
rank      rows whose k winners carry comparable mass (values a few ulps apart:
          e_i = exp(v_i / T - v_0 / T) is 1 to within 1e-6) and a sampler
          counter chosen so that u * total falls inside entry j's interval of
          the running sum, at least 4 (k 2^-24 + 1e-5) total from both ends
          (k 2^-24: worst-case fp32 summation error; 1e-5: the fast-exp
          allowance of test_sampler_topp_gpu.py; 4: headroom).  The id is
          ranked[j] exactly; the builder raises when the guard cannot be met,
          so no row is ever skipped.
cut       two plateaus: `a` entries at the top value (e = exp(0) = 1 exactly)
          and the rest of the k at a level with e = 1/4 (T = 2 / ln 4 for a
          step of 2.0).  min_p = 0.5 lies a factor 2 from both levels, so
          n_m = a; top_p puts its threshold in the middle of entry n_p - 1's
          interval.  The draw lands in entry n - 1 of the top plateau, where
          partial sums are exact integers; only the k - a lower entries round,
          so the guard on the threshold is 4 ((k - a + 3) 2^-24 + 1e-5) total
          (the 3: top_p's own rounding, the product and the last sum).  The id
          ranked[n - 1] reveals n = max(1, min(n_p, n_m)) exactly.
extreme   seed 12345: step 4257727 gives u == 0.0, step 21624501 gives
          u == 1 - 2^-24.  u = 0 returns ranked[0] on every path; u = 1 - 2^-24
          on m < k equal finite logits over a -inf rest (every e_i exactly 1,
          every partial sum an exact integer, fl(u m) in (m - 1, m)) returns
          ranked[m - 1], never a -inf entry.
path      `predict_path` mirrors the kernel's own choice (the 64 group maxima
          in the thread-to-element layout of for_row / the segment path, tau,
          the candidate count, the overflow fallback, rank or bitonic order,
          pair or chunk draw); every case names the path it is meant for.
emulate   an fp32 host emulation of select, order, cut and draw with fault
          knobs (FAULTS); the CPU test shows each knob rejected by the probe
          meant for it.
"""
import functools

import numpy as np
import torch

from llm_sharding_demo_amd.runtime.batch import counter_uniform

SMAX, NT, CH, SCH = 1024, 1024, 13, 16  # sample.hip: max top-k, threads per row, float4 / segments per thread
ONE_PASS_MAX = CH * NT * 4              # the longest row the plain path keeps in registers
U0_STEP, U1_STEP, U_SEED = 4257727, 21624501, 12345
U_MAX = 1.0 - 2.0 ** -24
# (seed, base) pairs of the counter search: negative seeds, seeds above 2^32, bases at 2^40
STREAMS = [(12345, 0), (-7, 1 << 40), ((1 << 33) + 5, 17), (-(1 << 35) - 3, (1 << 40) + (1 << 18)),
           (104729 * 11, 1 << 20), ((1 << 62) + 9, (1 << 40) + 3)]
FAULTS = ("drop_kth", "admit_k1", "tie_highest", "zero_by_key", "pad_admitted", "drop_partial_float4",
          "drop_partial_segment", "seg_gt", "low8_ignored", "pair_swap", "chunk_carry_lost", "np_plus",
          "np_minus", "minp_gt", "u_next", "greedy_tie_highest")
PAD_FIRST, PAD_REST = np.float32(np.inf), np.float32(3.0e38)  # what the padding columns hold
BG, FLOOR = np.float32(-30.0), np.float32(-20.0)
T_CUT = float(np.float32(2.0 / np.log(4.0)))  # a step of 2.0 is a factor 1/4


def ranked(row, V):
    """Indices of row[:V] in contract order: value descending (numeric
    comparison, -0.0 == +0.0), index ascending."""
    x = np.asarray(row, dtype=np.float32)[:V].astype(np.float64)
    return np.argsort(-x, kind="stable")


def uniform(seed, step):
    return float(counter_uniform(torch.tensor([seed], dtype=torch.int64), torch.tensor([step], dtype=torch.int64))[0])


@functools.lru_cache(maxsize=None)
def _utable(seed, base):
    steps = torch.arange(base, base + (1 << 18), dtype=torch.int64)
    u = counter_uniform(torch.full_like(steps, seed), steps).numpy().astype(np.float64)
    order = np.argsort(u, kind="stable")
    return u[order], order


def pick_step(seed, lo, hi, base=0):
    """(step, u): the step in [base, base + 2^18) whose u lies nearest the middle of [lo, hi)."""
    us, order = _utable(seed, base)
    mid = 0.5 * (lo + hi)
    i = int(np.searchsorted(us, mid))
    best = min((j for j in (i - 1, i) if 0 <= j < len(us)), key=lambda j: abs(us[j] - mid))
    return base + int(order[best]), float(us[best])


def cdf64(row, V, k, T):
    """(ranked ids, e, running sum) of the top k in float64."""
    r = ranked(row, V)[:k]
    with np.errstate(invalid="ignore"):
        v = np.asarray(row, dtype=np.float32)[r].astype(np.float64) / float(np.float32(T))
        e = np.exp(v - v[0])
    return r, e, np.cumsum(e)


def guard(k, total):
    return 4.0 * (k * 2.0 ** -24 + 1e-5) * total


def _place(seed, base, lo, hi, g, what):
    """A step whose u lies in [lo, hi) at least g from both ends (all three
    relative to the mass the draw runs over)."""
    step, u = pick_step(seed, lo, hi, base)
    if not (u - lo >= g and hi - u >= g):
        raise ValueError(f"{what}: u={u} cannot keep {g} from [{lo}, {hi})")
    return step, u


def rank_probe(row, V, k, T, j, stream=0):
    """(seed, step, expected id): the draw lands in entry j of the top k."""
    seed, base = STREAMS[stream % len(STREAMS)]
    k = min(max(k, 1), min(SMAX, V))
    r, e, c = cdf64(row, V, k, T)
    total = c[-1]
    lo, hi = (c[j - 1] if j else 0.0), c[j]
    step, _ = _place(seed, base, lo / total, hi / total, guard(k, total) / total, f"rank {j} of {k}")
    return seed, step, int(r[j])


def cut_probe(row, V, k, a, n_p, n_m_binds, stream=0, top_p=None, min_p=0.5):
    """Two-plateau row (a top entries): (seed, step, top_p, min_p, n, expected id).
    top_p (unless given) sits in the middle of entry n_p - 1's interval."""
    seed, base = STREAMS[stream % len(STREAMS)]
    r, e, c = cdf64(row, V, k, T_CUT)
    total = c[-1]
    assert np.all(e[:a] == 1.0) and (a == k or (0.2 < e[a] < 0.3)), "not a two-plateau row"
    g = 4.0 * ((k - a + 3) * 2.0 ** -24 + 1e-5) * total
    if top_p is None:
        lo, hi = (c[n_p - 2] if n_p > 1 else 0.0), c[n_p - 1]
        top_p = float(np.float32(0.5 * (lo + hi) / total))
        if not (top_p * total - lo >= g and hi - top_p * total >= g):
            raise ValueError(f"top_p for n_p={n_p} of k={k}, a={a}: guard {g} does not fit [{lo}, {hi})")
    elif top_p < 1.0:
        hit = np.flatnonzero(c >= top_p * total)
        n_p = int(hit[0]) + 1
        assert abs(c[n_p - 1] - top_p * total) >= g and (n_p < 2 or abs(c[n_p - 2] - top_p * total) >= g)
    else:
        n_p = k
    n_m = int((e >= min_p).sum()) if min_p > 0 else k
    if min_p > 0 and min_p != 1.0:
        assert np.all((e >= 2 * min_p) | (e <= min_p / 2)), "min_p needs a factor 2 on both sides"
    n = max(1, min(n_p, n_m))
    assert n <= a and (n == n_m) == bool(n_m_binds or n_p == n_m), (n, n_p, n_m)
    cn = c[n - 1]  # an exact integer: the draw runs over top-plateau entries only
    lo, hi = (c[n - 2] if n > 1 else 0.0), cn
    step, _ = _place(seed, base, lo / cn, hi / cn, guard(k, cn) / cn, f"cut n={n} of k={k}")
    return seed, step, top_p, min_p, n, int(r[n - 1])


# ---- the kernel's thread-to-element layout and its choice of path

def group_of(idx, seg):
    """The 16-thread group (0..63) whose maximum element `idx` feeds."""
    idx = np.asarray(idx)
    return (((idx // 8) if seg else (idx // 4)) % NT) // 16


def segmax_of(row):
    """What linear_f32 writes beside a row: the maximum of every 8 columns, padding included."""
    return np.asarray(row, dtype=np.float32).reshape(-1, 8).max(axis=1)


def predict_path(row, V, k, seg, greedy=False):
    """The path sample_kernel takes for this row: dict(name, select, overflow,
    order, draw, k, nsel, tau).  `row` is the whole padded row; `seg` says
    whether segment maxima are passed."""
    row = np.asarray(row, dtype=np.float32)
    x = row[:V]
    if greedy:
        return dict(name="greedy", select="greedy", k=1)
    k = min(max(int(k), 1), min(SMAX, V))
    S = (V + 7) // 8
    p = dict(k=k, overflow=False, tau=None, used_seg=False)
    if k <= 64:
        gmax = np.full(64, -np.inf, dtype=np.float32)
        if seg and S <= SCH * NT:
            sm = segmax_of(row)[:S].copy()
            if V % 8:
                sm[S - 1] = x[8 * (S - 1):].max()  # the partial segment: real logits only
            np.maximum.at(gmax, (np.arange(S) % NT) // 16, sm)
            sel, p["used_seg"] = "seg", True
        else:
            np.maximum.at(gmax, group_of(np.arange(V), False), x)
            sel = "one" if V <= ONE_PASS_MAX else "reread"
        tau = np.sort(gmax)[::-1][k - 1]
        ncand = int((x >= tau).sum())
        p.update(select=sel, tau=tau, ncand=ncand, overflow=ncand > SMAX)
        nsel = k if ncand > SMAX else ncand
        name = sel + (">overflow>radix" if ncand > SMAX else "")
    else:
        p.update(select="radix")
        nsel, name = k, "radix"
    rank = k <= 128 and nsel <= 256
    p.update(nsel=nsel, order="rank" if rank else "bitonic", draw="pair" if rank else "chunk")
    p["name"] = name + (">rank" if rank else ">bitonic")
    return p


def fkey(x, canonical=True):
    """The radix path's order-preserving key; canonical: -0.0 keyed as +0.0."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    if canonical:
        u[u == 0x80000000] = 0
    return np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.int64)


def emulate(row, V, k, T, seed, step, top_p=None, min_p=None, seg=False, greedy=False, faults=()):
    """The id the kernel returns, from an fp32 emulation of its select, order,
    cut and draw; `faults` (names from FAULTS) break one step each."""
    F = frozenset(faults)
    assert F <= set(FAULTS), F - set(FAULTS)
    row = np.asarray(row, dtype=np.float32)
    x = row[:V]
    if greedy:
        idx = np.flatnonzero(x == x.max())
        return int(idx[-1] if "greedy_tie_highest" in F else idx[0])
    p = predict_path(row, V, k, seg)
    k, sel = p["k"], p["select"]
    cand = None
    if sel != "radix":
        S = (V + 7) // 8
        lim = V
        if "drop_partial_float4" in F and sel != "seg" and V % 4:
            lim = V // 4 * 4
        if "drop_partial_segment" in F and sel == "seg" and V % 8:
            lim = V // 8 * 8
        vis = np.zeros(len(row), dtype=bool)
        vis[:lim] = True
        if "pad_admitted" in F:
            vis[V:min(len(row), 8 * S if sel == "seg" else (V + 3) // 4 * 4)] = True
        if "seg_gt" in F and sel == "seg":
            sm = segmax_of(row)
            if V % 8:
                sm[S - 1] = x[8 * (S - 1):].max()
            vis &= np.repeat(sm > p["tau"], 8)
        cand = np.flatnonzero(vis & (row >= p["tau"]))
        if len(cand) > SMAX:
            cand = None
    if cand is None:  # radix select: the k-th largest key, equal keys by index
        key = fkey(x, canonical="zero_by_key" not in F)
        if "low8_ignored" in F:
            key >>= 8
        ksel = k + 1 if ("admit_k1" in F and V > k) else k
        kth = np.sort(key)[::-1][ksel - 1]
        gt, eq = np.flatnonzero(key > kth), np.flatnonzero(key == kth)
        need = ksel - len(gt)
        take = eq[len(eq) - need:] if "tie_highest" in F else eq[:need]
        if "drop_kth" in F:
            take = take[:-1]
        cand = np.concatenate([gt, take])
    o = np.lexsort((cand, -row[cand].astype(np.float64)))
    kk = k + 1 if ("admit_k1" in F and len(cand) > k) else k
    ids, vals = cand[o][:kk], row[cand[o][:kk]]
    if len(ids) < kk:  # a lost winner leaves a slot that holds nothing
        ids = np.concatenate([ids, np.full(kk - len(ids), -1)])
        vals = np.concatenate([vals, np.full(kk - len(vals), -np.inf, dtype=np.float32)])
    T32 = np.float32(T)
    with np.errstate(invalid="ignore", over="ignore"):
        q = (vals / T32).astype(np.float32)
        e = np.exp((q - q[0]).astype(np.float32)).astype(np.float32)
    u = np.float32(uniform(seed, step + (1 if "u_next" in F else 0)))
    c = np.cumsum(e, dtype=np.float32)
    tot = c[-1]
    n, target = kk, np.float32(u * tot)
    tp = 1.0 if top_p is None else float(np.float32(top_p))
    mp = 0.0 if min_p is None else float(np.float32(min_p))
    if tp < 1.0 or mp > 0.0:
        n_m = int((e > np.float32(mp)).sum() if "minp_gt" in F else (e >= np.float32(mp)).sum())
        n_p = kk
        if tp < 1.0:
            hit = np.flatnonzero(c >= np.float32(np.float32(tp) * tot))
            n_p = int(hit[0]) + 1 if len(hit) else kk
            n_p = min(kk, max(1, n_p + ("np_plus" in F) - ("np_minus" in F)))
        n = max(1, min(n_p, n_m))
        target = np.float32(u * c[n - 1])
    cd = c
    if "chunk_carry_lost" in F and p["draw"] == "chunk":
        cd = np.concatenate([np.cumsum(e[b:b + 64], dtype=np.float32) for b in range(0, kk, 64)])
    hit = np.flatnonzero(cd[:n] >= target)
    pick = int(hit[0]) if len(hit) else n - 1
    if "pair_swap" in F and p["draw"] == "pair" and (pick ^ 1) < kk:
        pick ^= 1
    return int(ids[pick])


# ---- rows

def _from_ord(o):
    o = np.asarray(o, dtype=np.int64)
    bits = np.where(o >= 0, o, (1 << 31) | (-o)).astype(np.uint32)
    return bits.view(np.float32)


# ulp ladders: consecutive floats across a low-8-bit boundary of the key, a
# bit-20 boundary, an exponent boundary, and zero (negative denormals, +0.0,
# positive denormals)
LADDERS = {"low8": 0x3F800100, "bit20": 0x3FA00000, "expo": 0x3F800000, "zero": 0}


def ladder(kind, n, below=None):
    """n consecutive floats, descending, `below` of them under the boundary."""
    below = n // 2 if below is None else below
    return _from_ord(LADDERS[kind] - below + np.arange(n))[::-1].copy()


def blank_row(V, Vp):
    row = np.full(Vp, BG, dtype=np.float32)
    if Vp > V:
        row[V:] = PAD_REST
        row[V] = PAD_FIRST
    return row


def positions(V, n, mode, seg, rng, group=5):
    """n distinct indices below V.  spread: shuffled, always with 0, V - 1 and
    the start of the last (partial) float4; one_group: inside one 16-thread
    group; per_group: entry i in group i % 64 (one winner per group)."""
    if mode == "spread":
        must = list(dict.fromkeys([V - 1, 0, (V - 1) // 4 * 4]))[:n]
        rest = np.setdiff1d(np.arange(V), must)
        pos = np.concatenate([must, rng.choice(rest, n - len(must), replace=False)]).astype(np.int64)
        return rng.permutation(pos)
    g = group_of(np.arange(V), seg)
    if mode == "one_group":
        return rng.choice(np.flatnonzero(g == group), n, replace=False)
    assert mode == "per_group"
    used, out = set(), []
    for i in range(n):
        c = [j for j in rng.permutation(np.flatnonzero(g == i % 64))[:8] if j not in used]
        used.add(int(c[0]))
        out.append(int(c[0]))
    return np.array(out)


def add_floors(row, V, n, seg, rng, taken):
    """n entries at FLOOR among the free indices: one in every group first
    (tau is then FLOOR or a winner, never the background), the rest shuffled."""
    free = np.setdiff1d(np.arange(V), taken)
    g = group_of(free, seg)
    first = [free[np.flatnonzero(g == i)[0]] for i in range(64) if np.any(g == i)][:n]
    rest = rng.permutation(np.setdiff1d(free, first))[:max(0, n - len(first))]
    row[np.concatenate([first, rest]).astype(np.int64)] = FLOOR


FLOORS = {"tight": 64, "wide": 400, "over": 1100, "none": 0}


def make_row(V, Vp, vals, mode="spread", seg=False, floors="tight", seed=0, group=5):
    """A padded row: `vals` at positions chosen by `mode`, FLOORS[floors]
    entries at -20, -30 elsewhere.  Returns (row, positions of vals)."""
    rng = np.random.default_rng(seed)
    row = blank_row(V, Vp)
    pos = positions(V, len(vals), mode, seg, rng, group)
    add_floors(row, V, min(FLOORS[floors], V - len(vals)), seg, rng, pos)
    row[pos] = vals
    return row, pos


class Case:
    """One launch: `bases` are the distinct padded rows, `rows` the launch's
    rows (dicts: base, k, T, seed, step, top_p, min_p, greedy, expect, path)."""

    def __init__(self, name, V, Vp, seg):
        self.name, self.V, self.Vp, self.seg = name, V, Vp, seg
        self.bases, self.rows = [], []

    def base(self, row):
        assert len(row) == self.Vp
        self.bases.append(np.asarray(row, dtype=np.float32))
        return len(self.bases) - 1

    def add(self, b, k, T, seed, step, expect, path, top_p=1.0, min_p=0.0, greedy=0):
        self.rows.append(dict(base=b, k=k, T=T, seed=seed, step=step, expect=expect, path=path, top_p=top_p,
                              min_p=min_p, greedy=greedy))

    def add_rank(self, b, k, j, path, T=1.0):
        seed, step, exp = rank_probe(self.bases[b], self.V, k, T, j, stream=len(self.rows))
        self.add(b, k, T, seed, step, exp, path)

    def add_u(self, b, k, step, expect, path, T=1.0, top_p=1.0, min_p=0.0):
        self.add(b, k, T, U_SEED, step, expect, path, top_p=top_p, min_p=min_p)

    @property
    def cut(self):
        return any(r["top_p"] != 1.0 or r["min_p"] != 0.0 for r in self.rows)

    def tensors(self, rows=None):
        """CPU tensors of the launch (of the listed rows)."""
        rs = self.rows if rows is None else [self.rows[i] for i in rows]
        lg = torch.from_numpy(np.stack([self.bases[r["base"]] for r in rs]))
        t = dict(logits=lg, temp=torch.tensor([r["T"] for r in rs], dtype=torch.float32),
                 topk=torch.tensor([r["k"] for r in rs], dtype=torch.int32),
                 greedy=torch.tensor([r["greedy"] for r in rs], dtype=torch.int32),
                 seeds=torch.tensor([r["seed"] for r in rs], dtype=torch.int64),
                 step=torch.tensor([r["step"] for r in rs], dtype=torch.int64),
                 top_p=torch.tensor([r["top_p"] for r in rs], dtype=torch.float32),
                 min_p=torch.tensor([r["min_p"] for r in rs], dtype=torch.float32))
        t["segmax"] = lg.view(lg.shape[0], self.Vp // 8, 8).amax(-1).contiguous() if self.seg else None
        return t

    def expect(self):
        return [r["expect"] for r in self.rows]

    def emulated(self, faults=(), rows=None):
        rs = self.rows if rows is None else [self.rows[i] for i in rows]
        return [emulate(self.bases[r["base"]], self.V, r["k"], r["T"], r["seed"], r["step"],
                        None if r["top_p"] == 1.0 else r["top_p"], None if r["min_p"] == 0.0 else r["min_p"],
                        self.seg, bool(r["greedy"]), faults) for r in rs]

    def paths(self):
        return [predict_path(self.bases[r["base"]], self.V, r["k"], self.seg, bool(r["greedy"]))["name"]
                for r in self.rows]


# 4099 / 4104: 1025 float4, so all 64 groups of the plain layout hold logits, with a partial last
# float4 and a partial last segment.  Its 513 segments fill only 33 groups of the segment path (tau is
# -inf from k = 34 on: the overflow); 8195 / 8200 is the same shape for that layout (1025 segments).
PLAIN_SHAPE, SEG_SHAPE = (4099, 4104), (8195, 8200)
KLIST = [1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 1023, 1024]
SEAMS = [0, 1, 2, 3, 62, 63, 64, 65, 126, 127, 128, 129]  # lane pairs and 64-entry chunks


def seam_ranks(k):
    return sorted({j for j in SEAMS + [k - 2, k - 1] if 0 <= j < k})


# the sweep of every rank at 4099 / 4104: (ladder, placement, floors, path without segment maxima)
SWEEP = {1: ("expo", "spread", "tight", "one>rank"), 2: ("zero", "spread", "tight", "one>rank"),
         3: ("low8", "spread", "tight", "one>rank"), 63: ("bit20", "per_group", "tight", "one>rank"),
         64: ("low8", "spread", "wide", "one>bitonic"), 65: ("zero", "spread", "tight", "radix>rank"),
         127: ("low8", "spread", "tight", "radix>rank"), 128: ("expo", "spread", "tight", "radix>rank"),
         129: ("bit20", "spread", "tight", "radix>bitonic"), 200: ("low8", "spread", "tight", "radix>bitonic"),
         1023: ("zero", "spread", "tight", "radix>bitonic"), 1024: ("low8", "spread", "tight", "radix>bitonic")}


@functools.lru_cache(maxsize=None)
def sweep_case(k, seg):
    """Every rank of a top-k list, one row per rank, over one ulp ladder of
    k + 3 values (the three below rank k must stay out)."""
    V, Vp = SEG_SHAPE if seg and k > 3 else PLAIN_SHAPE
    kind, mode, floors, path = SWEEP[k]
    c = Case(f"sweep_k{k}_{'seg' if seg else 'plain'}", V, Vp, seg)
    row, _ = make_row(V, Vp, ladder(kind, k + 3, below=(k + 3) // 2), mode, seg, floors, seed=k)
    b = c.base(row)
    if seg and k <= 64:
        path = path.replace("one", "seg")
    for j in range(k):
        c.add_rank(b, k, j, path, T=(1.0, 0.75, 1.5)[j % 3])
    return c


def _tie_row(V, Vp, k, kind, seg, floors, zeros=False, seed=1):
    """k - 3 distinct ladder values, then six equal values straddling rank k
    (three in, three out) at index 0 (or 1), two mid-row indices in distinct
    groups, and the partial float4 with V - 1.  zeros: the six are signed
    zeros, -0.0 at the three lower indices, under a positive-denormal ladder."""
    rng = np.random.default_rng(seed)
    top = _from_ord(1 + np.arange(k - 3))[::-1] if zeros else ladder(kind, k - 2, below=(k - 2) // 2)[:-1]
    tie = np.float32(0.0) if zeros else ladder(kind, k - 2, below=(k - 2) // 2)[-1]
    row = blank_row(V, Vp)
    tpos = np.array([0, 701, 2002, (V - 1) // 4 * 4, V - 2, V - 1])
    assert len(set(group_of(tpos[:3], seg))) == 3
    pos = rng.choice(np.setdiff1d(np.arange(V), tpos), len(top), replace=False)
    add_floors(row, V, FLOORS[floors], seg, rng, np.concatenate([pos, tpos]))
    row[pos] = top
    row[tpos] = tie
    if zeros:
        row[tpos[:3]] = np.float32(-0.0)
    return row


@functools.lru_cache(maxsize=None)
def tie_case(seg, zeros):
    """Boundary ties (or signed zeros) on every path: the ranks around k and rank 0."""
    V, Vp = SEG_SHAPE if seg else PLAIN_SHAPE
    s = "seg" if seg else "one"
    c = Case(f"{'zeros' if zeros else 'ties'}_{'seg' if seg else 'plain'}", V, Vp, seg)
    plan = [(5, "tight", f"{s}>rank"), (40, "tight", f"{s}>rank"), (64, "wide", f"{s}>bitonic"),
            (40, "over", f"{s}>overflow>radix>rank"), (65, "tight", "radix>rank"), (129, "tight", "radix>bitonic"),
            (200, "tight", "radix>bitonic")]
    for i, (k, floors, path) in enumerate(plan):
        b = c.base(_tie_row(V, Vp, k, ("low8", "bit20", "expo")[i % 3], seg, floors, zeros, seed=10 + i))
        for j in sorted({0, k - 4, k - 3, k - 2, k - 1}):
            c.add_rank(b, k, j, path)
    return c


def plateau_row(V, Vp, k, a, seg, floors="tight", seed=3):
    """a entries at 2.0 and k - a at 0.0 (e = 1/4 at T_CUT), shuffled."""
    vals = np.concatenate([np.full(a, 2.0), np.full(k - a, 0.0)]).astype(np.float32)
    return make_row(V, Vp, vals, "spread", seg, floors, seed=seed)[0]


NCUT = [1, 2, 3, 63, 64, 65, 127, 128, 129, 1023, 1024]


@functools.lru_cache(maxsize=None)
def cut_case(k, seg):
    """n = 1 .. 1024 where k allows, n_p and n_m the smaller in turn; then
    top_p = 1e-6, min_p = 1.0 and each cut alone."""
    V, Vp = SEG_SHAPE if seg else PLAIN_SHAPE
    path = {64: "seg>rank" if seg else "one>rank", 128: "radix>rank", 200: "radix>bitonic",
            1024: "radix>bitonic"}[k]
    c = Case(f"cut_k{k}_{'seg' if seg else 'plain'}", V, Vp, seg)
    for n in [n for n in NCUT if n <= k]:
        for m_binds in (False, True):
            if m_binds and n == k:
                continue  # n_m = k cuts nothing
            a = n if m_binds else min(k, n + 1)
            n_p = min(k, a + 1) if m_binds else n
            b = c.base(plateau_row(V, Vp, k, a, seg, seed=100 * k + n))
            seed, step, tp, mp, n_got, exp = cut_probe(c.bases[b], V, k, a, n_p, m_binds, stream=len(c.rows))
            assert n_got == n
            c.add(b, k, T_CUT, seed, step, exp, path, top_p=tp, min_p=mp)
    a = min(5, k)
    b = c.base(plateau_row(V, Vp, k, a, seg, seed=7))
    for tp, mp, binds in ((1e-6, 0.0, False), (1.0, 1.0, True), (1.0, 0.5, True), (1e-6, 1.0, False)):
        seed, step, tp, mp, n, exp = cut_probe(c.bases[b], V, k, a, None, binds, stream=len(c.rows), top_p=tp,
                                               min_p=mp)
        c.add(b, k, T_CUT, seed, step, exp, path, top_p=tp, min_p=mp)
    if k > a + 2:  # top_p alone (min_p = 0)
        seed, step, tp, mp, n, exp = cut_probe(c.bases[b], V, k, a, a - 1, False, stream=3, min_p=0.0)
        c.add(b, k, T_CUT, seed, step, exp, path, top_p=tp, min_p=0.0)
    return c


def _equal_row(V, Vp, m, seg, seed=5):
    """m equal finite logits at shuffled positions, -inf elsewhere."""
    rng = np.random.default_rng(seed)
    row = blank_row(V, Vp)
    row[:V] = -np.inf
    row[positions(V, m, "spread", seg, rng)] = np.float32(1.5)
    return row


@functools.lru_cache(maxsize=None)
def extreme_case(seg):
    """u == 0 and u == 1 - 2^-24 on every path, and a -inf tail with fewer
    than k finite logits."""
    V, Vp = SEG_SHAPE if seg else PLAIN_SHAPE
    s = "seg" if seg else "one"
    c = Case(f"extreme_{'seg' if seg else 'plain'}", V, Vp, seg)
    for k, floors, mode, path in ((40, "tight", "spread", f"{s}>rank"), (64, "wide", "spread", f"{s}>bitonic"),
                                  (40, "over", "one_group", f"{s}>overflow>radix>rank"),
                                  (100, "tight", "spread", "radix>rank"), (300, "tight", "spread", "radix>bitonic")):
        row, _ = make_row(V, Vp, ladder("low8", k + 3), mode, seg, floors, seed=20 + k)
        b = c.base(row)
        r = ranked(row, V)
        c.add_u(b, k, U0_STEP, int(r[0]), path)
        # u = 1 - 2^-24 over k entries of e within 1e-6 of 1: the last one
        c.add_u(b, k, U1_STEP, int(r[k - 1]), path)
    for k, m, path in ((64, 40, f"{s}>overflow>radix>rank"), (128, 127, "radix>rank"), (1024, 1000, "radix>bitonic"),
                       (200, 65, "radix>bitonic")):
        row = _equal_row(V, Vp, m, seg, seed=k)
        b = c.base(row)
        r = ranked(row, V)
        assert np.isfinite(row[r[m - 1]]) and row[r[m]] == -np.inf
        c.add_u(b, k, U1_STEP, int(r[m - 1]), path)
        c.add_u(b, k, U0_STEP, int(r[0]), path)
        for j in sorted({0, 1, m // 2, m - 2, m - 1}):
            c.add_rank(b, k, j, path)
    return c


@functools.lru_cache(maxsize=None)
def group_case(seg):
    """All winners inside one 16-thread group (tau low: more than 256
    candidates, or more than fit), and one winner per group."""
    V, Vp = SEG_SHAPE if seg else PLAIN_SHAPE
    s = "seg" if seg else "one"
    c = Case(f"groups_{'seg' if seg else 'plain'}", V, Vp, seg)
    for k, mode, floors, path in ((40, "one_group", "wide", f"{s}>bitonic"),
                                  (40, "one_group", "over", f"{s}>overflow>radix>rank"),
                                  (64, "per_group", "tight", f"{s}>rank"), (17, "per_group", "none", f"{s}>rank")):
        row, _ = make_row(V, Vp, ladder("bit20", k + 3), mode, seg, floors, seed=30 + k)
        b = c.base(row)
        for j in seam_ranks(k):
            c.add_rank(b, k, j, path)
    return c


@functools.lru_cache(maxsize=None)
def greedy_case(seg):
    V, Vp = SEG_SHAPE if seg else PLAIN_SHAPE
    c = Case(f"greedy_{'seg' if seg else 'plain'}", V, Vp, seg)
    row = blank_row(V, Vp)
    row[[7, 1500, V - 1]] = 3.0  # equal maxima: the lowest index
    c.add(c.base(row), 40, 1.0, 1, 1, 7, "greedy", greedy=1)
    row = blank_row(V, Vp)
    row[V - 1] = 3.0  # the last logit, next to +inf padding
    c.add(c.base(row), 40, 1.0, 1, 1, V - 1, "greedy", greedy=1)
    row = blank_row(V, Vp)
    row[[900, 2000]] = (-0.0, 0.0)  # signed zeros are equal: the lower index
    c.add(c.base(row), 1, 1.0, 1, 1, 900, "greedy", greedy=1)
    row = blank_row(V, Vp)
    row[:V] = -np.inf  # nothing finite: index 0
    c.add(c.base(row), 1, 1.0, 1, 1, 0, "greedy", greedy=1)
    return c


# shapes past 4099: (V, Vp, seg, k, placement, floors, path)
SHAPES = [
    (1000, 1000, False, 40, "spread", "tight", "one>bitonic"),     # tau -inf: every logit a candidate
    (1000, 1000, True, 40, "spread", "tight", "seg>bitonic"),
    (1000, 1000, False, 8, "per_group", "tight", "one>rank"),
    (1024, 1024, False, 40, "spread", "tight", "one>bitonic"),     # exactly SMAX candidates
    (1024, 1024, True, 40, "spread", "tight", "seg>bitonic"),
    (1025, 1032, False, 40, "spread", "tight", "one>overflow>radix>rank"),  # one more: the overflow
    (1025, 1032, True, 40, "spread", "tight", "seg>overflow>radix>rank"),
    (53248, 53248, False, 40, "spread", "tight", "one>rank"),      # the last one-pass row
    (53248, 53248, True, 64, "spread", "wide", "seg>bitonic"),
    (53249, 53256, False, 40, "spread", "tight", "reread>rank"),   # the first re-read row
    (53249, 53256, False, 64, "spread", "wide", "reread>bitonic"),
    (53249, 53256, False, 40, "one_group", "over", "reread>overflow>radix>rank"),
    (53249, 53256, False, 200, "spread", "tight", "radix>bitonic"),
    (131072, 131072, True, 40, "spread", "tight", "seg>rank"),     # 16 segment chunks per thread
    (131073, 131080, True, 40, "spread", "tight", "reread>rank"),  # too long for the segment path
]
BIG_RANKS = {131072: (0, 38, 39), 131073: (0, 1, 39)}  # two or three rows at the two largest shapes


@functools.lru_cache(maxsize=None)
def shape_case(i):
    V, Vp, seg, k, mode, floors, path = SHAPES[i]
    c = Case(f"shape_{V}_{Vp}_{'seg' if seg else 'plain'}_k{k}_{mode}_{floors}", V, Vp, seg)
    row, _ = make_row(V, Vp, ladder(("low8", "bit20", "expo", "zero")[i % 4], k + 3), mode, seg, floors, seed=40 + i)
    b = c.base(row)
    for j in BIG_RANKS.get(V, seam_ranks(k)):
        c.add_rank(b, k, j, path)
    return c


def case_list():
    """Every case of the GPU file, in order: [(id, builder)]."""
    out = []
    for k in KLIST:
        out.append((f"sweep-k{k}-plain", functools.partial(sweep_case, k, False)))
        if k <= 64:
            out.append((f"sweep-k{k}-seg", functools.partial(sweep_case, k, True)))
    for seg in (False, True):
        s = "seg" if seg else "plain"
        out += [(f"ties-{s}", functools.partial(tie_case, seg, False)),
                (f"zeros-{s}", functools.partial(tie_case, seg, True)),
                (f"extreme-{s}", functools.partial(extreme_case, seg)),
                (f"groups-{s}", functools.partial(group_case, seg)),
                (f"greedy-{s}", functools.partial(greedy_case, seg))]
    for k in (64, 128, 200, 1024):
        out.append((f"cut-k{k}-plain", functools.partial(cut_case, k, False)))
    out.append(("cut-k64-seg", functools.partial(cut_case, 64, True)))
    for i, sh in enumerate(SHAPES):
        out.append((f"shape-{sh[0]}-{sh[1]}-{'seg' if sh[2] else 'plain'}-k{sh[3]}-{sh[4]}-{sh[5]}",
                    functools.partial(shape_case, i)))
    return out


ALL_PATHS = {"greedy"} | {f"{s}{o}{d}" for s in ("seg", "one", "reread") for o in ("", ">overflow>radix")
                          for d in (">rank", ">bitonic") if not (o and d == ">bitonic")} | \
    {"radix>rank", "radix>bitonic"}


# ---- penalties before the draw

def pen_hash(t, bits):
    return ((int(t) * 2654435761) & 0xFFFFFFFF) >> (32 - bits)


def same_bucket_tokens(V, bits, bucket, n):
    """The first n tokens below V whose home bucket in a 2^bits table is `bucket`."""
    t = np.arange(V, dtype=np.uint64)
    h = ((t * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - bits)
    out = np.flatnonzero(h == bucket)[:n]
    assert len(out) == n, (V, bits, bucket, n, len(out))
    return out.astype(np.int64)
