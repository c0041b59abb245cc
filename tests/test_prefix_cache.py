"""The prefix cache (EngineConfig.prefix_cache): a finished request's KV slot
stays behind as an entry keyed by its prompt, and a later prompt that shares a
long enough prefix starts its prefill behind a copy of it.  CPU only: the two
scheduler cores plan identically and keep the cache's invariants (by
simulation), the boundaries of a hit, the host sanitizer driver of the core,
the plan wire, and on the CPU golden models a hit's tokens equal those of an
engine without the cache that chunks the prompt at the same place -- plus the
HTTP contract and a 2-rank gloo run."""
import hashlib
import json
import os
import pickle
import random
import shutil
import socket
import subprocess
import sys
import textwrap

import pytest

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
from llm_sharding_demo_amd.runtime.kv_cache import SlotAllocator as PySlots
from llm_sharding_demo_amd.runtime.plan import Chunk, GroupPlan, PlanDecoder, PlanEncoder, Row, StepPlan
from llm_sharding_demo_amd.runtime.scheduler import EV_FIRST, EV_RELEASE, PySchedCore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = 7


def _rt():
    from llm_sharding_demo_amd.runtime.native import build, load

    build()
    rt = load()
    # the native core is what this file is about: a build or import break fails, it does not skip
    assert rt is not None and hasattr(rt, "SchedCore") and hasattr(rt.SchedCore, "set_prefix_cache")
    return rt


def _make(kind, R, M, cap, budget, chunk, slots, entries, min_tokens):
    if kind == "native":
        rt = _rt()
        pools = [rt.SlotAllocator(slots) for _ in range(R)]
        core = rt.SchedCore(R, M, cap, budget, chunk, 512, pools)
    else:
        pools = [PySlots(slots) for _ in range(R)]
        core = PySchedCore(R, M, cap, budget, chunk, 512, pools)
    core.set_prefix_cache(entries, min_tokens)
    return core, pools


def _avail(p):
    a = p.available
    return a() if callable(a) else a


def _plans(p):
    return [[tuple(go[:6]) + ([tuple(c) for c in go[6]], [tuple(r) for r in go[7]]) for go in rep] for rep in p]


def _entries(core, rep):
    return [(s, p, tuple(k)) for s, p, k in core.prefix_entries(rep)]


def _lcp(a, b):
    n = 0
    for x, y in zip(a, b):
        if x != y:
            break
        n += 1
    return n


def _brute(entries, prompt, min_tokens):
    best = max((min(_lcp(k, prompt), len(prompt) - 1) for _, _, k in entries), default=0)
    return best if best >= min_tokens else 0


class Workload:
    """Requests whose prompts share prefixes: a pool of 3 stems of 20-40
    tokens, tails of 0-12, some duplicates, some families, some one-token
    prompts; a sixth opt out, a sixth insert without looking up."""

    def __init__(self, rnd, cap, slots):
        self.rnd, self.top = rnd, max(1, min(cap, slots, 4))
        self.stems = [[rnd.randint(20, 23) for _ in range(rnd.randint(20, 40))] for _ in range(3)]
        self.recent, self.sid = [], 0
        self.seqs = {}  # sid -> dict(prompt, looks, parent)

    def request(self, cores):
        rnd = self.rnd
        if self.recent and rnd.random() < 0.25:
            prompt = rnd.choice(self.recent)
        elif rnd.random() < 0.08:
            prompt = [25]
        else:
            prompt = list(rnd.choice(self.stems))
            if rnd.random() < 0.2:
                prompt = prompt[: rnd.randint(1, len(prompt))]
            prompt += [rnd.randint(30, 32) for _ in range(rnd.randint(0, 12))]
        self.recent.append(prompt)
        n = rnd.randint(2, self.top) if self.top >= 2 and rnd.random() < 0.25 else 1
        stop, mode = rnd.random() < 0.5, rnd.randrange(6)  # mode 0: opted out, 1: inserts only, else both
        wants = [rnd.choice([1, 1, 3, 20])] + [rnd.choice([1, 2, 9]) for _ in range(n - 1)]
        par = self.sid
        self.sid += n
        for c in cores:
            c.add(par, len(prompt), wants[0], stop)
            for i in range(1, n):
                if i % 2:  # ahead of set_prompt, and behind it
                    c.add_fork(par + i, par, wants[i], stop)
            if mode:
                c.set_prompt(par, prompt, mode != 1)
            for i in range(1, n):
                if not i % 2:
                    c.add_fork(par + i, par, wants[i], stop)
        self.seqs[par] = dict(prompt=prompt, looks=mode > 1, parent=-1)
        for i in range(1, n):
            self.seqs[par + i] = dict(prompt=prompt, looks=False, parent=par if len(prompt) > 1 else -1)


# ---------------------------------------------------------------------------
# twin equality, over the grids of test_fork.py test_cores_plan_families_identically
@pytest.mark.parametrize("policy", [(1, 0), (3, 2), (8, 4)])  # join policy (join_min, max_wait)
@pytest.mark.parametrize("chunk,budget", [(0, 0), (3, 0), (3, 5), (0, 16)])
@pytest.mark.parametrize("seed", range(6))
def test_cores_plan_prefix_hits_identically(seed, chunk, budget, policy):
    rt = _rt()
    rnd = random.Random(1000 * seed + 10 * chunk + budget)
    R, M = rnd.choice([1, 2]), rnd.choice([1, 2, 3])
    cap = rnd.choice([2, 4, 8])
    slots = rnd.choice([cap * M, cap, 4])
    entries, min_tokens = rnd.choice([1, 2, slots]), rnd.choice([1, 4, 16])
    npool = [rt.SlotAllocator(slots) for _ in range(R)]
    ppool = [PySlots(slots) for _ in range(R)]
    nat = rt.SchedCore(R, M, cap, budget, chunk, 512, npool)
    py = PySchedCore(R, M, cap, budget, chunk, 512, ppool)
    for c in (nat, py):
        c.set_join_policy(*policy)
        c.set_prefix_cache(entries, min_tokens)
    wl = Workload(rnd, cap, slots)
    pending, hits = [], 0

    def same_state():
        assert [_avail(p) for p in npool] == [_avail(p) for p in ppool]
        assert tuple(nat.prefix_cache_stats()) == py.prefix_cache_stats()
        for rep in range(R):
            assert _entries(nat, rep) == _entries(py, rep)

    for step in range(5000):
        if step < 160 and rnd.random() < 0.3:
            for _ in range(rnd.randint(1, 3)):
                wl.request((nat, py))
        assert nat.has_work() == py.has_work()
        if not py.has_work() and step >= 160:
            break
        if not py.has_work():
            continue
        pn, an = nat.plan(step)
        pp, ap = py.plan(step)
        assert list(an) == ap
        assert _plans(pn) == _plans(pp), step
        assert [tuple(f) for f in nat.forks()] == py.forks()
        assert [tuple(h) for h in nat.hits()] == py.hits()
        hits += len(py.hits())
        same_state()
        for rep, gos in enumerate(pp):
            for go in gos:
                if go[1]:
                    pending.append((step, rep, go[0], go[1]))
        lag = rnd.randint(0, 3)
        while pending and pending[0][0] <= step - lag:
            st, rep, g, n = pending.pop(0)
            toks = [rnd.choice([EOS, 11, 12, 13]) for _ in range(n)]
            assert [tuple(e) for e in nat.assign(rep, st, g, toks, EOS)] == py.assign(rep, st, g, toks, EOS)
            same_state()
        assert (nat.joins, nat.leaves, nat.max_rows, nat.deferred) == (py.joins, py.leaves, py.max_rows, py.deferred)
    else:
        raise AssertionError("the workload did not drain")
    while pending:
        st, rep, g, n = pending.pop(0)
        assert [tuple(e) for e in nat.assign(rep, st, g, [11] * n, EOS)] == py.assign(rep, st, g, [11] * n, EOS)
    same_state()
    assert nat.n_expect == py.n_expect == 0
    for c in (nat, py):
        c.clear_prefix_cache()
    assert [_avail(p) for p in ppool] == [_avail(p) for p in npool] == [slots] * R
    assert hits > 0 or min_tokens == 16 or entries < 2


# ---------------------------------------------------------------------------
# invariants, by simulation, on both cores
def _simulate(core, pools, R, slots, entries, min_tokens, rnd, wl, feed_until=160, clear_at=None):
    """Drive `core` with wl's requests.  Checks at every step:
      * free + cached + held slots = capacity; no slot is an entry and a
        sequence's; at most `entries` entries per replica;
      * a hit's source is an entry, pinned from the plan with the hit's first
        chunk until the read-back with the sequence's first token;
      * m = the chunk's start, min_tokens <= m <= L - 1, m is what the source's
        key gives and, in a plan that evicted nothing, the brute-force best
        over the replica's entries (a miss: that best is 0);
      * only sequences that look up hit;
      * insert: no entry's key starts with the new entry's; an entry whose key
        the new one starts with is pinned.
    -> hits seen."""
    owner, slot_of, src_of, pending = {}, {}, {}, []
    held, seen = 0, 0

    def check_slots():
        cached = 0
        for rep in range(R):
            es = _entries(core, rep)
            assert len(es) <= entries
            cached += len(es)
            assert not any((rep, s) in owner for s, _, _ in es), "a slot is an entry and a sequence's"
        assert sum(_avail(p) for p in pools) + cached + held == R * slots
        assert core.prefix_cache_stats()[0] == cached

    def readout(st, rep, g, n, toks):
        nonlocal held
        before = [{s for s, _, _ in _entries(core, r)} for r in range(R)]
        for sid, tok, flags in core.assign(rep, st, g, toks, EOS):
            if flags & EV_FIRST:
                src_of.pop(sid, None)  # the pin is back
            if flags & EV_RELEASE:
                held -= 1
                assert owner.pop(slot_of[sid]) == sid
        for r in range(R):
            es = _entries(core, r)
            for s, _, key in es:
                if s in before[r]:
                    continue
                assert len(key) >= min_tokens
                for o, pins, ok in es:
                    if o != s:
                        assert ok[: len(key)] != key, "an entry's key starts with the new entry's"
                        assert key[: len(ok)] != ok or pins > 0, "the new key starts with an unpinned entry's"
        check_slots()

    for step in range(5000):
        if step < feed_until and rnd.random() < 0.3:
            for _ in range(rnd.randint(1, 3)):
                wl.request((core,))
        if not core.has_work():
            if step >= feed_until:
                break
            continue
        if step == clear_at:
            core.clear_prefix_cache()
            assert all(p > 0 for rep in range(R) for _, p, _ in _entries(core, rep))
            check_slots()
        snap = [_entries(core, rep) for rep in range(R)]
        ev0 = core.prefix_cache_stats()[4]
        plans, admitted = core.plan(step)
        evicted = core.prefix_cache_stats()[4] != ev0
        held += len(admitted)
        now = set(admitted)
        hit_m, fork_src = dict(map(tuple, core.hits())), dict(map(tuple, core.forks()))
        assert set(hit_m) <= set(fork_src)
        found = 0
        for rep, gos in enumerate(plans):
            for go in gos:
                for sid, slot, start, ln, final in map(tuple, go[6]):
                    if sid in slot_of:
                        assert slot_of[sid] == (rep, slot)
                        continue
                    assert owner.get((rep, slot)) is None, f"slot {slot} has two owners"
                    owner[(rep, slot)] = sid
                    slot_of[sid] = (rep, slot)
                    q = wl.seqs[sid]
                    L = len(q["prompt"])
                    if q["parent"] >= 0:
                        assert sid not in hit_m
                        continue
                    m = hit_m.get(sid, 0)
                    assert start == m
                    if m:
                        found += 1
                        assert q["looks"] and min_tokens <= m <= L - 1
                        src = src_of[sid] = (rep, fork_src[sid])
                        assert src not in owner
                        pins, key = {s: (p, k) for s, p, k in _entries(core, rep)}[src[1]]
                        assert pins > 0 and min(_lcp(key, q["prompt"]), L - 1) == m
                    if sid in now and not evicted:
                        assert m == (_brute(snap[rep], tuple(q["prompt"]), min_tokens) if q["looks"] else 0)
                if go[1]:
                    pending.append((step, rep, go[0], go[1]))
        assert found == len(hit_m)
        seen += found
        for sid, (rep, src) in src_of.items():  # no first token yet: the entry is still pinned
            assert {s: p for s, p, _ in _entries(core, rep)}[src] > 0
        check_slots()
        lag = rnd.randint(0, 3)
        while pending and pending[0][0] <= step - lag:
            st, rep, g, n = pending.pop(0)
            readout(st, rep, g, n, [rnd.choice([EOS, 11, 12]) for _ in range(n)])
    else:
        raise AssertionError("the workload did not drain")
    while pending:
        st, rep, g, n = pending.pop(0)
        readout(st, rep, g, n, [11] * n)
    assert not owner and not src_of and core.n_expect == 0 and held == 0
    assert all(p == 0 for rep in range(R) for _, p, _ in _entries(core, rep))
    return seen


@pytest.mark.parametrize("kind", ["python", "native"])
@pytest.mark.parametrize("chunk,budget", [(0, 0), (3, 0), (4, 6)])
@pytest.mark.parametrize("seed", range(6))
def test_prefix_cache_invariants(kind, chunk, budget, seed):
    rnd = random.Random(91 * seed + chunk)
    R, M, cap = rnd.choice([1, 2]), rnd.choice([1, 2]), rnd.choice([3, 4, 8])
    slots = rnd.choice([cap, cap * M, cap + 1])
    entries, min_tokens = rnd.choice([1, 2, slots]), rnd.choice([1, 4, 16])
    core, pools = _make(kind, R, M, cap, budget, chunk, slots, entries, min_tokens)
    wl = Workload(rnd, cap, slots)
    _simulate(core, pools, R, slots, entries, min_tokens, rnd, wl, clear_at=70 if seed % 3 == 0 else None)
    # clear_prefix_cache() and reset() give every slot back
    if seed % 2:
        core.clear_prefix_cache()
    else:
        core.reset()
    assert [_avail(p) for p in pools] == [slots] * R and core.prefix_cache_stats()[0] == 0


@pytest.mark.parametrize("kind", ["python", "native"])
def test_hits_are_seen_and_reset_frees_pinned_entries(kind):
    """The workload of the invariants test with room to hit; then a reset()
    with hits in flight: every slot comes back, the pinned entries' too."""
    rnd = random.Random(5)
    core, pools = _make(kind, 1, 2, 4, 0, 0, 8, 8, 4)
    wl = Workload(rnd, 4, 8)
    assert _simulate(core, pools, 1, 8, 8, 4, rnd, wl) > 10
    a = list(range(40, 60))
    core.add(10_000, 20, 1, False)
    core.set_prompt(10_000, a)
    step = 6000
    while core.has_work() or core.n_expect:
        plans, _ = core.plan(step)
        for go in plans[0]:
            if go[1]:
                core.assign(0, step, go[0], [11] * go[1], EOS)
        step += 1
    core.add(10_001, 24, 5, False)
    core.set_prompt(10_001, a + [1, 2, 3, 4])
    core.plan(step)
    assert [tuple(h) for h in core.hits()] == [(10_001, 20)]
    assert any(p > 0 for _, p, _ in _entries(core, 0))
    core.clear_prefix_cache()  # the pinned entry stays
    assert [p for _, p, _ in _entries(core, 0)] == [1]
    core.reset()
    assert _avail(pools[0]) == 8 and core.prefix_cache_stats()[0] == 0 and not core.has_work()


def _run(core, step, until=lambda: False):
    """Plan and read back at once until the core is idle -> the next step."""
    while (core.has_work() or core.n_expect) and not until():
        plans, _ = core.plan(step)
        for rep, gos in enumerate(plans):
            for go in gos:
                if go[1]:
                    core.assign(rep, step, go[0], [11] * go[1], EOS)
        step += 1
    return step


@pytest.mark.parametrize("kind", ["python", "native"])
@pytest.mark.parametrize("k", [0, 1, 3])
def test_a_pool_of_cached_slots_admits_a_family(kind, k):
    """1 + k slots, every one an entry: a family of 1 + k whose prompt matches
    one of them is admitted all the same -- the match is dropped."""
    core, pools = _make(kind, 1, 1, 1 + k, 0, 0, 1 + k, 1 + k, 4)
    for i in range(1 + k):
        core.add(i, 8, 1, False)
        core.set_prompt(i, [40 + i] * 8)
    step = _run(core, 0)
    assert _avail(pools[0]) == 0 and core.prefix_cache_stats()[0] == 1 + k
    core.add(100, 9, 1, False)
    for i in range(1, 1 + k):
        core.add_fork(100 + i, 100, 1, False)
    core.set_prompt(100, [40] * 8 + [9])
    _, admitted = core.plan(step)
    assert list(admitted) == [100 + i for i in range(1 + k)] and not core.hits()
    ent, hits, misses, reused, evictions = core.prefix_cache_stats()
    assert (ent, hits, misses, evictions) == (0, 0, 2 + k, 1 + k)
    _run(core, step + 1)
    core.clear_prefix_cache()
    assert _avail(pools[0]) == 1 + k


# ---------------------------------------------------------------------------
# boundaries, min_tokens = 16
STEM = list(range(100, 140))


def _donor(kind, prompt=STEM, **kw):
    core, pools = _make(kind, 1, 1, 8, 0, 0, 8, 8, 16)
    core.add(0, len(prompt), 2, False)
    core.set_prompt(0, prompt, **kw)
    return core, pools, _run(core, 0)


def _probe(core, step, sid, prompt, prompt_kw=None):
    """Admit one request -> (its m or 0, its first chunk)."""
    core.add(sid, len(prompt), 1, False)
    if prompt_kw is not None:
        core.set_prompt(sid, prompt, **prompt_kw)
    plans, _ = core.plan(step)
    chunk = tuple(plans[0][0][6][0])
    return dict(map(tuple, core.hits())).get(sid, 0), chunk


@pytest.mark.parametrize("kind", ["python", "native"])
def test_boundaries(kind):
    core, pools, step = _donor(kind)
    assert _entries(core, 0) == [(_entries(core, 0)[0][0], 0, tuple(STEM))]
    slot = _entries(core, 0)[0][0]
    # common prefix 15: a miss; 16: a hit
    m, chunk = _probe(core, step, 1, STEM[:15] + [9] * 10, {})
    assert m == 0 and chunk[2:] == (0, 25, True) and not core.forks()
    step = _run(core, step + 1)
    m, chunk = _probe(core, step, 2, STEM[:16] + [9] * 10, {})
    assert m == 16 and chunk[2:] == (16, 10, True) and [tuple(f) for f in core.forks()] == [(2, slot)]
    assert chunk[1] != slot
    step = _run(core, step + 1)
    # a prompt identical to an entry: m = L - 1, one token is forwarded
    m, chunk = _probe(core, step, 3, STEM, {})
    assert m == 39 and chunk[2:] == (39, 1, True)
    step = _run(core, step + 1)
    # a prompt the entry's key starts with: m = L - 1 as well
    m, chunk = _probe(core, step, 4, STEM[:20], {})
    assert m == 19 and chunk[2:] == (19, 1, True)
    step = _run(core, step + 1)
    # a one-token prompt: a miss
    m, chunk = _probe(core, step, 5, [100], {})
    assert m == 0 and chunk[2:] == (0, 1, True)
    step = _run(core, step + 1)
    # the longest match wins: STEM[:16] + 9s is an entry by now, STEM matches further
    m, chunk = _probe(core, step, 6, STEM[:30] + [8], {})
    assert m == 30
    step = _run(core, step + 1)
    ent, hits, misses, reused, evictions = core.prefix_cache_stats()
    assert (hits, misses, reused, evictions) == (4, 3, 16 + 39 + 19 + 30, 0)  # the donor missed too
    core.clear_prefix_cache()
    assert _avail(pools[0]) == 8


@pytest.mark.parametrize("kind", ["python", "native"])
def test_opted_out_requests_neither_hit_nor_insert(kind):
    core, pools, step = _donor(kind)
    m, chunk = _probe(core, step, 1, STEM + [5], None)  # no set_prompt: SamplingParams.prefix_cache = False
    assert m == 0 and chunk[2] == 0
    step = _run(core, step + 1)
    assert [k for _, _, k in _entries(core, 0)] == [tuple(STEM)]  # and STEM + [5] did not replace it
    assert tuple(core.prefix_cache_stats()[1:3]) == (0, 1)  # the donor's miss alone


@pytest.mark.parametrize("kind", ["python", "native"])
def test_context_requests_insert_but_do_not_hit(kind):
    core, pools, step = _donor(kind, lookup=False)  # the donor itself is one: it inserts
    assert [k for _, _, k in _entries(core, 0)] == [tuple(STEM)]
    m, chunk = _probe(core, step, 1, STEM + [5], dict(lookup=False))
    assert m == 0 and chunk[2] == 0 and not core.forks()
    step = _run(core, step + 1)
    assert [k for _, _, k in _entries(core, 0)] == [tuple(STEM + [5])]  # the longer key replaced the one it covers
    assert tuple(core.prefix_cache_stats()[1:3]) == (0, 0)  # no lookup: neither a hit nor a miss


@pytest.mark.parametrize("kind", ["python", "native"])
def test_dedup_lru_and_ties(kind):
    core, pools = _make(kind, 1, 1, 8, 0, 0, 8, 2, 4)
    # a family leaves one entry, not n
    core.add(0, 10, 1, False)
    for i in (1, 2, 3):
        core.add_fork(i, 0, 1 + i, False)
    core.set_prompt(0, [50] * 10)
    step = _run(core, 0)
    assert [k for _, _, k in _entries(core, 0)] == [(50,) * 10] and _avail(pools[0]) == 7
    # a shorter key that an entry covers is freed
    for sid, p in ((10, [50] * 6), (11, [60] * 8)):
        core.add(sid, len(p), 1, False)
        core.set_prompt(sid, p)
        step = _run(core, step)
    assert sorted(k for _, _, k in _entries(core, 0)) == [(50,) * 10, (60,) * 8]
    assert core.prefix_cache_stats()[4] == 0 and _avail(pools[0]) == 6
    # at most 2 entries: the least recently used goes -- [60] * 8, since this one hits [50] * 10 first
    core.add(12, 10, 1, False)
    core.set_prompt(12, [50] * 9 + [1])
    step = _run(core, step)
    assert sorted(k for _, _, k in _entries(core, 0)) == [(50,) * 9 + (1,), (50,) * 10]
    assert core.prefix_cache_stats()[4] == 1 and _avail(pools[0]) == 6
    # ties go to the most recently used entry
    core2, pools2 = _make(kind, 1, 1, 8, 0, 0, 8, 4, 4)
    step = 0
    for sid, p in ((0, [1] * 8 + [2]), (1, [1] * 8 + [3])):
        core2.add(sid, 9, 1, False)
        core2.set_prompt(sid, p)
        step = _run(core2, step)
    slots = {k: s for s, _, k in _entries(core2, 0)}
    m, _ = _probe(core2, step, 2, [1] * 8 + [4], {})
    assert m == 8 and [tuple(f) for f in core2.forks()] == [(2, slots[(1,) * 8 + (3,)])]
    step = _run(core2, step + 1)
    m, _ = _probe(core2, step, 3, [1] * 8 + [2, 2], {})  # a longer match beats the more recent one
    assert m == 9 and [tuple(f) for f in core2.forks()] == [(3, slots[(1,) * 8 + (2,)])]
    with pytest.raises(Exception):
        core2.set_prompt(3, [1] * 8 + [2, 2])  # admitted already
    with pytest.raises(Exception):
        core2.set_prefix_cache(4, 8)  # an entry is pinned
    with pytest.raises(Exception):
        core2.set_prefix_cache(-1, 8)


def test_prefix_stress_under_asan_ubsan(tmp_path):
    """csrc/runtime/tests/sched_prefix_stress.cpp: random hit / evict / reset
    workloads through the native core, as a program of its own under
    AddressSanitizer + UBSan, with the invariants asserted in C++."""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path / "sps"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                        os.path.join(ROOT, "csrc", "runtime", "tests", "sched_prefix_stress.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and "cannot find" in r.stderr:
        pytest.skip(f"sanitizer runtime not available: {r.stderr[-200:]}")
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([str(exe), "48"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert r.stdout.startswith("ok 48")


# ---------------------------------------------------------------------------
# wire
def _wire_plan(hit=False):
    ch = [Chunk(3, 1, 0, [5, 6, 7], True, 0.8, 40, False, 11, 0.9, 0.0), Chunk(4, 2, 4, [9], False, 1.0, 1, True, 12)]
    ch[0].guide = 2
    rows = [Row(1, 0, 7, 0.7, 30, False, 99, 3, 0, logprobs=2), Row(2, 3, 9, 1.0, 1, True, 5, 4, 1)]
    if hit:  # a hit's first chunk: the tail of its prompt behind 48 copied positions, not final here
        ch = [Chunk(6, 4, 48, list(range(60, 92)), False, 0.8, 40, False, 12, fork=5)] + ch
    return StepPlan(step=7, replica=0, groups=[GroupPlan(0, ret=2, rows=rows, n=2, b=2, ctxb=256, chunks=ch),
                                               GroupPlan(1, chunks=[Chunk(8, 5, 0, [1, 2], True)])])


def test_plan_wire_round_trips_a_hit_and_is_unchanged_without():
    from llm_sharding_demo_amd.runtime.plan import _pack_group

    # without a hit: the bytes of the commit before the prefix cache (sha256 of
    # record + payload of this very plan, the one test_fork.py pins too)
    plain = _wire_plan()
    assert [len(_pack_group(g, True)) for g in plain.groups] == [14, 9]
    rec, payload = PlanEncoder(ids=True).encode(plain)
    assert (hashlib.sha256(rec.tobytes() + payload).hexdigest()
            == "d745935ae056e9e0a1b140d11760f1232096683bd43e907e766c1b7b102b246b")
    assert PlanDecoder().decode(rec, lambda n: payload) == plain
    hit = _wire_plan(hit=True)
    assert [len(_pack_group(g, True)) for g in hit.groups] == [15, 9]
    for ids in (True, False):
        rec, payload = PlanEncoder(ids=ids).encode(hit)
        got = PlanDecoder().decode(rec, lambda n: payload)
        assert [[(c.seq, c.slot, c.start, c.qlen, c.final, c.fork, c.seed) for c in g.chunks] for g in got.groups] == \
               [[(c.seq, c.slot, c.start, c.qlen, c.final, c.fork, c.seed) for c in g.chunks] for g in hit.groups]
        if ids:
            assert got == hit
    assert [c.opens for c in hit.groups[0].chunks] == [True, True, False]
    assert pickle.loads(pickle.dumps(hit)) == hit


# ---------------------------------------------------------------------------
# engine on the CPU golden models
from llm_sharding_demo_amd.runtime.engine import Engine  # noqa: E402

_R = random.Random(11)
A = [_R.randrange(3, 200) for _ in range(64)]
B = A[:48] + [_R.randrange(3, 200) for _ in range(32)]
SEEDED = dict(temperature=1.1, top_k=60, seed=100)
NEW = 8


def _eng(model="gpt2-test", P=1, max_batch=8, **kw):
    return Engine(EngineConfig(model_id=model, num_stages=P, max_batch=max_batch, device="cpu", **kw))


def _free(e):
    """Every slot is free or an entry, nothing is pinned, no fork is owed."""
    st = e.prefix_cache_stats()
    pins = [p for rep in range(e.R) for _, p, _ in e.scheduler.core.prefix_entries(rep)] if e.cfg.prefix_cache else []
    return (sum(p.available for p in e.slot_pools) + st["entries"] == e.kv_slots * e.R and not any(pins)
            and e.scheduler._forking == 0)


@pytest.fixture(scope="module", params=[("gpt2-test", 1), ("gpt2-test", 2), ("llama-test", 1), ("llama-test", 2)],
                ids=["gpt2-P1", "gpt2-P2", "llama-P1", "llama-P2"])
def pair(request):
    """(cache on, cache off), both with prefill_chunk = 48: B's tail runs the
    same chunk shape against the same KV on both."""
    model, P = request.param
    return _eng(model, P, prefill_chunk=48, prefix_cache=4), _eng(model, P, prefill_chunk=48)


def _a_then_b(on, off, **kw):
    """A, then B, on both engines -> (B with the cache, B without)."""
    on.prefix_cache_clear()
    assert on.prefix_cache_stats()["entries"] == 0
    before = on.prefix_cache_stats()
    sp = SamplingParams(max_new_tokens=NEW, **kw)
    ra = on.generate_requests([A], [sp])[0]
    assert ra.cached_tokens == 0 and on.prefix_cache_stats()["entries"] == 1
    launches = [w.kv_fork_launches for w in on.workers]
    rb = on.generate_requests([B], [sp])[0]
    want = off.generate_requests([B], [sp])[0]
    n = kw.get("n", 1)
    # one copy per stage for the hit, and one for the family's forks
    assert [w.kv_fork_launches - x for w, x in zip(on.workers, launches)] == [1 + (n > 1)] * on.P
    st = on.prefix_cache_stats()
    assert rb.cached_tokens == 48 and want.cached_tokens == 0
    assert (st["hits"] - before["hits"], st["tokens_reused"] - before["tokens_reused"]) == (1, 48)
    assert st["misses"] - before["misses"] == 1 and st["entries"] == 2
    assert [s.finish_reason for s in rb.samples] == [s.finish_reason for s in want.samples]
    assert _free(on) and _free(off) and off.prefix_cache_stats() == dict.fromkeys(st, 0)
    return rb, want


def test_a_hit_equals_the_engine_without_the_cache(pair):
    rb, want = _a_then_b(*pair, **SEEDED)
    assert rb.output == want.output and len(rb.output) == NEW


def test_greedy_hit(pair):
    rb, want = _a_then_b(*pair, greedy=True)
    assert rb.output == want.output


def test_hit_with_logprobs(pair):
    rb, want = _a_then_b(*pair, logprobs=2, **SEEDED)
    assert rb.output == want.output and rb.logprobs.tokens == want.logprobs.tokens == rb.output
    # same chunk shape against the same KV bits: the records are equal, not close
    assert rb.logprobs.token_logprobs == want.logprobs.token_logprobs
    assert rb.logprobs.top_logprobs == want.logprobs.top_logprobs


def test_hit_with_n(pair):
    rb, want = _a_then_b(*pair, n=3, **SEEDED)
    assert [s.output for s in rb.samples] == [s.output for s in want.samples]
    assert len({tuple(s.output) for s in rb.samples}) > 1


@pytest.mark.parametrize("P", [1, 2])
def test_hit_with_a_guide(P):
    from llm_sharding_demo_amd import compile_choice
    from llm_sharding_demo_amd.utils.tokenizer import ByteTokenizer

    vocab = ByteTokenizer(gpt2_ids=False, eos_id=2).token_bytes(1000)
    guide = compile_choice(["yes-1", "no-22", "maybe-333", "never"], vocab, 2)
    on, off = _eng("llama-test", P, prefill_chunk=48, prefix_cache=4), _eng("llama-test", P, prefill_chunk=48)
    rb, want = _a_then_b(on, off, guide=guide, stop_at_eos=True, temperature=1.3, top_k=200, seed=40)
    assert rb.output == want.output
    assert on.guides.pins == [0] * len(on.guides.pins)


@pytest.mark.parametrize("chunk", [0, 48, 7])
def test_an_opted_out_request_equals_the_engine_without_the_cache(chunk):
    on, off = _eng(prefill_chunk=chunk, prefix_cache=4), _eng(prefill_chunk=chunk)
    sp = SamplingParams(max_new_tokens=NEW, prefix_cache=False, **SEEDED)
    on.generate_requests([A], [SamplingParams(max_new_tokens=NEW, **SEEDED)])
    launches = [w.kv_fork_launches for w in on.workers]
    rb = on.generate_requests([B], [sp])[0]
    assert rb.output == off.generate_requests([B], [sp])[0].output and rb.cached_tokens == 0
    assert [w.kv_fork_launches for w in on.workers] == launches
    st = on.prefix_cache_stats()
    assert (st["entries"], st["hits"], st["misses"]) == (1, 0, 1)  # A's lookup and entry; B did neither


def test_context_requests_do_not_look_up_on_the_engine():
    on, off = _eng(prefill_chunk=48, prefix_cache=4), _eng(prefill_chunk=48)
    kws = [dict(repetition_penalty=1.4), dict(no_repeat_ngram_size=2), dict(bad_words=[[B[50], B[51]], [4]])]
    on.generate_requests([A], [SamplingParams(max_new_tokens=NEW, **SEEDED)])
    for kw in kws:
        sp = SamplingParams(max_new_tokens=NEW, **SEEDED, **kw)
        rb = on.generate_requests([B], [sp])[0]
        assert rb.cached_tokens == 0 and rb.output == off.generate_requests([B], [sp])[0].output
    st = on.prefix_cache_stats()
    assert (st["hits"], st["misses"], st["entries"]) == (0, 1, 2)  # they inserted: B's entry beside A's
    # and a plain request hits the entry that a context request left
    rb = on.generate_requests([B + [9, 9]], [SamplingParams(max_new_tokens=2, greedy=True)])[0]
    assert rb.cached_tokens == len(B)
    assert _free(on)


def test_eviction_under_pressure():
    """max_batch = 4, prefix_cache = 4, 12 distinct prompts: all finish, the
    outputs are those of the engine without the cache, the stats add up."""
    on, off = _eng(max_batch=4, prefix_cache=4), _eng(max_batch=4)
    rnd = random.Random(3)
    prompts = [[rnd.randrange(3, 200) for _ in range(rnd.randint(17, 40))] for _ in range(12)]
    sps = [SamplingParams(max_new_tokens=2 + i % 4, temperature=1.0, top_k=50, seed=i) for i in range(12)]
    got = on.generate_requests(prompts, sps)
    assert [r.output for r in got] == off.generate_ids(prompts, sps)
    st = on.prefix_cache_stats()
    assert st["hits"] == 0 and st["misses"] == 12 and st["tokens_reused"] == 0
    assert st["entries"] + st["evictions"] == 12 and 1 <= st["entries"] <= 4  # every prompt left an entry
    assert _free(on)
    again = on.generate_requests(prompts[-1:], [SamplingParams(max_new_tokens=2, greedy=True)])[0]
    assert again.cached_tokens == len(prompts[-1]) - 1
    on.prefix_cache_clear()
    assert sum(p.available for p in on.slot_pools) == on.kv_slots and on.prefix_cache_stats()["entries"] == 0
    on.scheduler.fail_all(RuntimeError("boom"))
    assert sum(p.available for p in on.slot_pools) == on.kv_slots


def test_off_means_off_and_validation():
    e = _eng()
    assert e.cfg.prefix_cache == 0 and e.scheduler._caching is False
    r = e.generate_requests([A, B], [SamplingParams(max_new_tokens=3, greedy=True)] * 2)
    assert [x.cached_tokens for x in r] == [0, 0] and [w.kv_fork_launches for w in e.workers] == [0]
    assert sum(p.available for p in e.slot_pools) == e.kv_slots
    assert tuple(e.scheduler.core.prefix_cache_stats()) == (0, 0, 0, 0, 0) and not e.scheduler.core.prefix_entries(0)
    e.prefix_cache_clear()
    with pytest.raises(ValueError, match="prefix_cache"):
        EngineConfig(model_id="gpt2-test", max_batch=4, prefix_cache=5)
    with pytest.raises(ValueError, match="prefix_cache"):
        EngineConfig(model_id="gpt2-test", prefix_cache=-1)
    with pytest.raises(ValueError, match="prefix_cache_min_tokens"):
        EngineConfig(model_id="gpt2-test", prefix_cache_min_tokens=0)
    for bad in (1, 0, None, "no"):
        with pytest.raises(ValueError, match="prefix_cache must be a bool"):
            e.generate_ids([A], SamplingParams(max_new_tokens=1, prefix_cache=bad))
    cfg = EngineConfig.from_env()
    assert (cfg.prefix_cache, cfg.prefix_cache_min_tokens) == (0, 8)
    os.environ.update(PREFIX_CACHE="8", PREFIX_CACHE_MIN_TOKENS="32")
    try:
        cfg = EngineConfig.from_env()
        assert (cfg.prefix_cache, cfg.prefix_cache_min_tokens) == (8, 32)
    finally:
        del os.environ["PREFIX_CACHE"], os.environ["PREFIX_CACHE_MIN_TOKENS"]


def test_regrouping_gives_the_entries_back():
    e = _eng(prefix_cache=4)
    e.generate_requests([A], [SamplingParams(max_new_tokens=2, greedy=True)])
    assert e.prefix_cache_stats()["entries"] == 1
    e.set_groups(2)
    assert sum(p.available for p in e.slot_pools) == e.kv_slots and e.prefix_cache_stats()["entries"] == 0
    assert e.generate_requests([A], [SamplingParams(max_new_tokens=2, greedy=True)])[0].cached_tokens == 0


# ---------------------------------------------------------------------------
# HTTP
def test_http_contract():
    from fastapi.testclient import TestClient

    from llm_sharding_demo_amd import LLM
    from llm_sharding_demo_amd.serving.server import create_app

    text = "The quick brown fox jumps over the lazy dog, twice over. "
    body = {"prompt": text + "And then?", "max_new_tokens": 4, "greedy": True}
    outs = {}
    for entries in (0, 4):
        cfg = EngineConfig(model_id="gpt2-test", max_batch=4, device="cpu", role="coordinator", prefix_cache=entries)
        llm = LLM(cfg)
        client = TestClient(create_app(cfg, engine=llm.engine))
        first = client.post("/generate", json={"prompt": text, "max_new_tokens": 4, "greedy": True})
        r = client.post("/generate", json=body)
        assert first.status_code == r.status_code == 200
        outs[entries] = r.json()["generated"]
        health, prom = client.get("/health").json(), client.get("/metrics").text
        if entries == 0:
            # the cache off: exactly the keys of before
            assert set(first.json()) == set(r.json()) == {"generated"}
            assert "prefix_cache" not in health and "prefix_cache" not in prom
            assert client.post("/generate", json={**body, "prefix_cache": False}).json() == r.json()
        else:
            n = len(llm.tokenizer.encode(text))
            assert n >= 16 and first.json()["cached_tokens"] == 0 and r.json()["cached_tokens"] == n
            assert set(r.json()) == {"generated", "cached_tokens"}
            out = client.post("/generate", json={**body, "prefix_cache": False}).json()
            assert out == {"generated": outs[4], "cached_tokens": 0}
            health, prom = client.get("/health").json(), client.get("/metrics").text
            assert health["prefix_cache"] == {"entries": 1, "hits": 1, "misses": 1, "tokens_reused": n, "evictions": 0}
            for line in ("prefix_cache_entries 1", "prefix_cache_hits_total 1", "prefix_cache_misses_total 1",
                         f"prefix_cache_tokens_reused_total {n}", "prefix_cache_evictions_total 0"):
                assert any(ln.endswith(line) for ln in prom.splitlines()), (line, prom)
        for bad in (1, "false", None, [True]):
            assert client.post("/generate", json={**body, "prefix_cache": bad}).status_code == 422
        assert "prefix_cache" in client.get("/openapi.json").json()["components"]["schemas"]["GenerateReq"]["properties"]
        llm.engine.shutdown()
    # gpt2-test greedy: the shorter chunk's GEMMs may round differently, the text is still a continuation
    assert outs[4].startswith(body["prompt"]) and outs[0].startswith(body["prompt"])


def test_http_relay_ignores_the_field(monkeypatch):
    from fastapi.testclient import TestClient

    from llm_sharding_demo_amd.serving import server

    calls = []

    def fake(cfg, ids, sp, records=False, reasons=False):
        calls.append(sp.prefix_cache)
        return [5], None, ("length", None)

    monkeypatch.setattr(server, "http_generate", fake)
    cfg = EngineConfig(model_id="gpt2-test", device="cpu", role="coordinator", prefix_cache=4)
    client = TestClient(server.create_app(cfg))
    js = client.post("/generate", json={"prompt": "ab", "max_new_tokens": 1, "prefix_cache": False}).json()
    assert set(js) == {"generated"} and calls == [False]


# ---------------------------------------------------------------------------
# rank processes
def test_two_rank_gloo_matches_local(tmp_path):
    """One process per stage over gloo: the plan wire carries the hit's
    Chunk.fork, the rank process copies its own layers' KV -- the tokens and
    the cached_tokens of the local engine."""
    sp = dict(max_new_tokens=NEW, **SEEDED)
    loc = _eng(P=2, prefill_chunk=48, prefix_cache=4)
    want = []
    for p in (A, B, B):
        r = loc.generate_requests([p], [SamplingParams(**sp)])[0]
        want.append([r.output, r.cached_tokens])
    assert [c for _, c in want] == [0, 48, len(B) - 1]
    script = tmp_path / "w.py"
    script.write_text(textwrap.dedent(f"""
        import sys, json, torch
        sys.path.insert(0, {ROOT!r})
        from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
        from llm_sharding_demo_amd.runtime.engine import build_engine
        cfg = EngineConfig(model_id="gpt2-test", max_batch=8, device="cpu", transport="gloo", num_microbatches=2,
                           prefill_chunk=48, prefix_cache=4)
        eng = build_engine(cfg)
        assert eng.P == 2
        if eng.rank != 0:
            eng.worker_loop()
        else:
            out = []
            for p in {[A, B, B]!r}:
                r = eng.generate_requests([p], [SamplingParams(**{sp!r})])[0]
                out.append([r.output, r.cached_tokens])
            eng.shutdown()
            print("RESULT", json.dumps(out))
    """))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={port}", str(script)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][0]
    assert json.loads(line[len("RESULT "):]) == want
