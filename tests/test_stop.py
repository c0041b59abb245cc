"""Per-request stop conditions (stop_token_ids, stop_sequences,
include_stop_in_output): validation, the native scheduler core
(csrc/runtime/sched_core.h set_stops) against its Python twin on random
workloads and on hand-written cases, a sanitizer stress driver of the native
core, the engine on both cores with one and two stages, and /generate.  CPU
only."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
from llm_sharding_demo_amd.runtime.engine import Engine
from llm_sharding_demo_amd.runtime.kv_cache import SlotAllocator as PySlots
from llm_sharding_demo_amd.runtime.scheduler import EV_FINISH, EV_FIRST, EV_RELEASE, EV_STOP, PySchedCore


def _rt():
    from llm_sharding_demo_amd.runtime.native import build, load

    build()
    rt = load()
    if rt is None or not hasattr(rt, "SchedCore"):
        pytest.skip("native runtime not importable")
    return rt


# ---------------------------------------------------------------------------
# validation

def test_defaults_validate_and_are_off():
    sp = SamplingParams()
    sp.validate()
    assert sp.stop_token_ids is None and sp.stop_sequences is None and sp.include_stop_in_output is False
    assert not sp.has_stops and sp.stop_list() == [] and sp.stop_match([1, 2, 3]) is None
    assert EngineConfig().max_stop_sequences == 16
    SamplingParams(stop_token_ids=[5, 5, np.int64(3)], stop_sequences=[[1, 2], (4,)], include_stop_in_output=True).validate()
    SamplingParams(stop_sequences=[list(range(32))]).validate()


def test_order_and_the_rule():
    sp = SamplingParams(stop_token_ids=[9, 3, 9], stop_sequences=[[1, 2], [3], [1, 2]])
    # stop_token_ids first, ascending, duplicates collapsed; then stop_sequences as given
    assert sp.stop_list() == [(3,), (9,), (1, 2), (3,), (1, 2)]
    assert sp.stop_match([7, 3]) == 0 and sp.stop_match([1, 2]) == 2 and sp.stop_match([2, 1]) is None
    assert sp.stop_match([2]) is None and sp.stop_match([]) is None
    held = SamplingParams(stop_token_ids=[3], min_new_tokens=2, max_new_tokens=5)
    assert held.stop_match([3]) is None and held.stop_match([3, 3]) is None and held.stop_match([3, 3, 3]) == 0


@pytest.mark.parametrize("kw", [
    dict(stop_sequences=[[]]), dict(stop_sequences=[[1], []]), dict(stop_sequences=[list(range(33))]),
    dict(stop_sequences=[[1.0]]), dict(stop_sequences=[["1"]]), dict(stop_sequences="12"), dict(stop_sequences=[5]),
    dict(stop_sequences=[[-1]]), dict(stop_sequences=[[2 ** 31]]), dict(stop_sequences={1: 2}),
    dict(stop_token_ids=[-1]), dict(stop_token_ids=[True]), dict(stop_token_ids="3"), dict(stop_token_ids=5),
    dict(stop_token_ids=[1.5]), dict(stop_token_ids=list(range(17))),
    dict(stop_token_ids=list(range(9)), stop_sequences=[[1, i] for i in range(8)]),   # 17 in total
    dict(include_stop_in_output=1),
], ids=str)
def test_validate_refuses(kw):
    with pytest.raises(ValueError):
        SamplingParams(**kw).validate()


def test_limits():
    SamplingParams(stop_token_ids=list(range(16))).validate()
    SamplingParams(stop_token_ids=list(range(8)), stop_sequences=[[1, i] for i in range(8)]).validate()
    SamplingParams(stop_token_ids=list(range(17))).validate(max_stop_sequences=17)
    for bad in (0, 65):
        with pytest.raises(ValueError):
            EngineConfig(max_stop_sequences=bad)
    assert EngineConfig(max_stop_sequences=64).max_stop_sequences == 64


def test_limit_comes_from_the_environment(monkeypatch):
    monkeypatch.setenv("MAX_STOP_SEQUENCES", "3")
    assert EngineConfig.from_env().max_stop_sequences == 3


def _eng(P=1, max_batch=4, **kw):
    return Engine(EngineConfig(model_id="gpt2-test", num_stages=P, max_batch=max_batch, device="cpu", **kw))


def test_engine_refuses_ids_outside_the_vocabulary_and_too_many():
    e = _eng(max_stop_sequences=2)
    V = e.mcfg.vocab_size
    for kw in (dict(stop_token_ids=[V]), dict(stop_sequences=[[1, V + 5]]), dict(stop_sequences=[[]]),
               dict(stop_token_ids=[1, 2, 3]), dict(stop_sequences=[list(range(33))])):
        sp = SamplingParams(max_new_tokens=2, **kw)
        with pytest.raises(ValueError):
            e.generate_ids([[1, 2]], [sp])
        with pytest.raises(ValueError):
            e.submit([1, 2], sp)
    e.generate_ids([[1, 2]], [SamplingParams(max_new_tokens=2, stop_token_ids=[V - 1], stop_sequences=[[0, V - 1]])])


# ---------------------------------------------------------------------------
# native core against the Python twin

def _stops(rnd):
    """A random stop list over the token source's alphabet: (flat, lengths, min_tokens)."""
    lens = [rnd.choice([1, 1, 2, 2, 3, 5, 32]) for _ in range(rnd.randint(1, 6))]
    flat = [rnd.choice([7, 11, 12, 13]) for _ in range(sum(lens))]
    return flat, lens, rnd.choice([0, 0, 1, 3, 10])


@pytest.mark.parametrize("policy", [(1, 0), (3, 2), (8, 4)])  # join policy (join_min, max_wait)
@pytest.mark.parametrize("collect", [False, True])
@pytest.mark.parametrize("seed", range(8))
def test_native_core_matches_python_twin(seed, collect, policy):
    rt = _rt()
    rnd = random.Random(1000 + seed)
    R, M = rnd.choice([1, 2]), rnd.choice([1, 2, 3])
    cap = rnd.choice([1, 2, 4, 8])
    slots = rnd.choice([cap * M * R, max(1, cap * M * R // 2), 3])
    budget = rnd.choice([0, 0, 5, 16, 64])
    chunk = rnd.choice([0, 0, 3, 8])
    max_seq, eos = 512, 7
    npool = [rt.SlotAllocator(slots) for _ in range(R)]
    ppool = [PySlots(slots) for _ in range(R)]
    nat = rt.SchedCore(R, M, cap, budget, chunk, max_seq, npool)
    py = PySchedCore(R, M, cap, budget, chunk, max_seq, ppool)
    nat.set_join_policy(*policy)
    py.set_join_policy(*policy)
    sid = 0
    pending = []  # (step, rep, g, n_tokens)
    stops, wants, got, nstop = {}, {}, {}, 0
    for step in range(5000):
        if step < 150 and rnd.random() < 0.3:
            for _ in range(rnd.randint(1, 4)):
                L, stop = rnd.randint(1, 40), rnd.random() < 0.3
                want = rnd.choice([rnd.randint(1, 20), rnd.randint(1, 20), rnd.randint(33, 45)])  # some outgrow the tail
                nat.add(sid, L, want, stop)
                py.add(sid, L, want, stop)
                wants[sid] = want
                if rnd.random() < 0.7:
                    stops[sid] = _stops(rnd)
                    nat.set_stops(sid, *stops[sid])
                    py.set_stops(sid, *stops[sid])
                sid += 1
        assert nat.has_work() == py.has_work()
        if not py.has_work() and step >= 150:
            break
        pn, an = nat.plan(step)
        pp, ap = py.plan(step)
        assert an == ap
        assert [[tuple(go[:6]) + ([tuple(c) for c in go[6]], [tuple(r) for r in go[7]]) for go in rep]
                for rep in pn] == [[go[:6] + (go[6], go[7]) for go in rep] for rep in pp], step
        for rep, gos in enumerate(pp):
            for go in gos:
                if go[1]:
                    pending.append((step, rep, go[0], go[1]))
        lag = rnd.randint(0, 3)
        while pending and (pending[0][0] <= step - lag):
            st, rep, g, n = pending.pop(0)
            toks = [rnd.choice([eos, 11, 12, 13]) for _ in range(n)]  # stop material at every token
            if collect:
                en, dn = nat.assign_collect(rep, st, g, np.array(toks, dtype=np.int32), eos)
                ep, dp = py.assign_collect(rep, st, g, toks, eos)
                assert [tuple(e) for e in en] == ep and [(a, list(b)) for a, b in dn] == dp
                assert all(e[2] for e in ep)  # plain tokens never come back
                for sid_, tl in dp:
                    got.setdefault(sid_, tl)
            else:
                en = [tuple(e) for e in nat.assign(rep, st, g, toks, eos)]
                ep = py.assign(rep, st, g, toks, eos)
                assert en == ep
                for e in ep:
                    if e[1] >= 0:
                        got.setdefault(e[0], []).append(e[1])
            nstop += sum(1 for e in ep if e[2] & EV_STOP)
            assert all(e[2] & EV_FINISH and not e[2] & EV_RELEASE for e in ep if e[2] & EV_STOP)
        assert [p.available for p in npool] == [p.available for p in ppool]
        assert (nat.joins, nat.leaves, nat.max_rows, nat.deferred) == (py.joins, py.leaves, py.max_rows, py.deferred)
    while pending:  # the readouts still out when the work ran dry
        st, rep, g, n = pending.pop(0)
        if collect:
            en, dn = nat.assign_collect(rep, st, g, np.full(n, 11, dtype=np.int32), eos)
            ep, dp = py.assign_collect(rep, st, g, [11] * n, eos)
            assert [tuple(e) for e in en] == ep and [(a, list(b)) for a, b in dn] == dp
            for sid_, tl in dp:
                got.setdefault(sid_, tl)
        else:
            ep = py.assign(rep, st, g, [11] * n, eos)
            assert [tuple(e) for e in nat.assign(rep, st, g, [11] * n, eos)] == ep
            for e in ep:
                if e[1] >= 0:
                    got.setdefault(e[0], []).append(e[1])
    assert nat.n_expect == py.n_expect == 0 and not py.has_work() and not nat.has_work()
    assert [p.available for p in npool] == [slots] * R  # every slot released
    assert nstop > 0
    # the finished tokens against the rule on the whole output
    for s, tl in got.items():
        assert 1 <= len(tl) <= wants[s]
        if s in stops and len(tl) < wants[s] and tl[-1] != eos:
            flat, lens, mn = stops[s]
            words, at = [], 0
            for n in lens:
                words.append(flat[at: at + n])
                at += n
            assert len(tl) > mn and any(tl[len(tl) - len(w):] == w for w in words if len(w) <= len(tl))


# ---------------------------------------------------------------------------
# behaviour of the core, both implementations

def _core(kind, cap=2):
    if kind == "native":
        rt = _rt()
        pools = [rt.SlotAllocator(cap)]
        return rt.SchedCore(1, 1, cap, 0, 0, 256, pools), pools
    pools = [PySlots(cap)]
    return PySchedCore(1, 1, cap, 0, 0, 256, pools), pools


def _feed(core, tokens, eos=99, collect=False, per_readout=1):
    """Run one sequence (sid 0, added by the caller) over the token stream:
    -> (events of sid 0 without releases, tokens it kept)."""
    ev, kept, step, it = [], None, 0, iter(tokens)
    while core.has_work():
        plans, _ = core.plan(step)
        for go in plans[0]:
            if go[1]:
                toks = [next(it, 55) for _ in range(go[1])]
                if collect:
                    e, done = core.assign_collect(0, step, go[0], np.array(toks, dtype=np.int32), eos)
                    kept = dict((a, list(b)) for a, b in done).get(0, kept)
                else:
                    e = core.assign(0, step, go[0], toks, eos)
                ev += [tuple(x) for x in e if not x[2] & EV_RELEASE]
        step += 1
        assert step < 200
    return ev, kept


KINDS = ["native", "py"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("collect", [False, True])
def test_match_across_two_readouts(kind, collect):
    core, pools = _core(kind)
    core.add(0, 3, 10, False)
    core.set_stops(0, [5, 6, 7], [3], 0)
    ev, kept = _feed(core, [1, 5, 6, 7, 8, 9], collect=collect)  # one token per readout: the match spans three
    if collect:
        assert kept == [1, 5, 6, 7] and ev == [(0, 1, EV_FIRST), (0, 7, EV_FINISH | EV_STOP)]
    else:
        assert ev == [(0, 1, EV_FIRST), (0, 5, 0), (0, 6, 0), (0, 7, EV_FINISH | EV_STOP)]
    assert pools[0].available == 2  # released; the over-issued token was dropped


@pytest.mark.parametrize("kind", KINDS)
def test_match_of_token_one_the_prefill_draw(kind):
    core, pools = _core(kind)
    core.add(0, 4, 10, False)
    core.set_stops(0, [5], [1], 0)
    ev, _ = _feed(core, [5, 5, 5])
    assert ev == [(0, 5, EV_FIRST | EV_FINISH | EV_STOP)] and pools[0].available == 2


@pytest.mark.parametrize("kind", KINDS)
def test_min_tokens_suppresses_a_match_until_its_next_occurrence(kind):
    core, _ = _core(kind)
    core.add(0, 2, 10, False)
    core.set_stops(0, [5, 6], [2], 3)   # counts from token 4 on
    ev, kept = _feed(core, [5, 6, 5, 1, 5, 6, 2], collect=True)
    assert kept == [5, 6, 5, 1, 5, 6]   # (5, 6) at token 2 is suppressed; taken at token 6
    core, _ = _core(kind)
    core.add(0, 2, 10, False)
    core.set_stops(0, [5, 6], [2], 3)
    ev, kept = _feed(core, [1, 5, 5, 6, 2], collect=True)
    assert kept == [1, 5, 5, 6]         # token 4 is the first that counts
    core, _ = _core(kind)
    core.add(0, 2, 10, False)
    core.set_stops(0, [5, 6], [2], 4)
    ev, kept = _feed(core, [1, 5, 5, 6, 2, 5, 6], collect=True)
    assert kept == [1, 5, 5, 6, 2, 5, 6]


@pytest.mark.parametrize("kind", KINDS)
def test_list_order_eos_first_and_the_length_limit(kind):
    # two sequences match at once: either ends the request; the scheduler reports the first in list order
    core, _ = _core(kind)
    core.add(0, 2, 10, False)
    core.set_stops(0, [6, 5, 6], [1, 2], 0)
    ev, _ = _feed(core, [5, 6, 1])
    assert ev[-1] == (0, 6, EV_FINISH | EV_STOP)
    sp = SamplingParams(stop_sequences=[[5, 6], [6]], stop_token_ids=[])
    assert sp.stop_match([5, 6]) == 0 and SamplingParams(stop_sequences=[[6], [5, 6]]).stop_match([5, 6]) == 0
    assert SamplingParams(stop_sequences=[[5, 6]], stop_token_ids=[6]).stop_match([5, 6]) == 0  # the token id first
    # stop_at_eos is checked first: an EOS that is also a stop token is an EOS stop
    core, _ = _core(kind)
    core.add(0, 2, 10, True)
    core.set_stops(0, [99], [1], 0)
    ev, _ = _feed(core, [1, 99, 1], eos=99)
    assert ev[-1] == (0, 99, EV_FINISH)
    # without stop_at_eos the same token is a stop
    core, _ = _core(kind)
    core.add(0, 2, 10, False)
    core.set_stops(0, [99], [1], 0)
    assert _feed(core, [1, 99, 1], eos=99)[0][-1] == (0, 99, EV_FINISH | EV_STOP)
    # a match at the want-th token is a stop too; without one the request ends by length
    core, _ = _core(kind)
    core.add(0, 2, 2, False)
    core.set_stops(0, [8], [1], 0)
    assert _feed(core, [1, 8])[0][-1] == (0, 8, EV_FINISH | EV_STOP)
    core, _ = _core(kind)
    core.add(0, 2, 2, False)
    core.set_stops(0, [8], [1], 0)
    assert _feed(core, [1, 2])[0][-1] == (0, 2, EV_FINISH)


@pytest.mark.parametrize("kind", KINDS)
def test_the_prompt_does_not_count_and_the_tail_holds_32(kind):
    # a prompt of any length: only generated tokens are matched, so (x, 5) needs a generated x
    core, _ = _core(kind)
    core.add(0, 7, 6, False)
    core.set_stops(0, [4, 5], [2], 0)
    _, kept = _feed(core, [5, 1, 4, 5, 9], collect=True)   # 5 as token 1 does not complete (4, 5)
    assert kept == [5, 1, 4, 5]
    # a 32-token sequence matched after 40 tokens: the tail keeps exactly the last 32
    w = [3 + (i * 7) % 5 for i in range(32)]
    stream = [1] * 8 + w + [2, 2]
    core, _ = _core(kind)
    core.add(0, 2, 60, False)
    core.set_stops(0, w, [32], 0)
    _, kept = _feed(core, stream, collect=True)
    assert kept == stream[:40]
    # 31 of the 32 tokens are no match, and a sequence longer than the output never matches
    core, _ = _core(kind)
    core.add(0, 2, 35, False)
    core.set_stops(0, w, [32], 0)
    _, kept = _feed(core, w[1:] + [1] * 10, collect=True)
    assert len(kept) == 35


@pytest.mark.parametrize("kind", KINDS)
def test_set_stops_refusals_and_sequences_without_stops(kind):
    core, _ = _core(kind)
    core.add(0, 2, 5, False)
    for flat, lens in (([1, 2], [1]), ([], [0]), ([1] * 33, [33]), ([1], [1, 1])):
        with pytest.raises(ValueError):
            core.set_stops(0, flat, lens, 0)
    with pytest.raises(ValueError):
        core.set_stops(7, [1], [1], 0)         # unknown sequence
    core.set_stops(0, [1], [1], 0)
    core.set_stops(0, [], [], 0)                # an empty list turns them off again
    ev, _ = _feed(core, [1, 1, 1, 1, 1])
    assert len(ev) == 5 and not any(e[2] & EV_STOP for e in ev)
    if kind == "py":
        core.add(1, 2, 5, False)
        assert core.seqs[1].stops is None and core.seqs[1].tail is None  # nothing extra is kept


def test_stop_stress_under_asan_ubsan(tmp_path):
    """csrc/runtime/tests/sched_stop_stress.cpp: 16 random workloads with
    random stop lists through the native core, as a program of its own under
    AddressSanitizer + UBSan, against a naive model of the rule."""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "sss"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                        "-fno-omit-frame-pointer",
                        os.path.join(root, "csrc", "runtime", "tests", "sched_stop_stress.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and "cannot find" in r.stderr:
        pytest.skip(f"sanitizer runtime not available: {r.stderr[-200:]}")
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([str(exe), "16"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert r.stdout.startswith("ok 16")


# ---------------------------------------------------------------------------
# engine (gpt2-test on the CPU), one and two stages, both cores

PROMPT = [1, 2, 3]
N = 24
SEEDED = dict(temperature=1.3, top_k=200, seed=17)


def _first_end(T, k_from, n):
    """The first k >= k_from at which T[k:k+n] ends for the first time: no
    earlier occurrence of that n-gram in T."""
    for k in range(k_from, len(T) - n + 1):
        w = T[k: k + n]
        if all(T[i: i + n] != w for i in range(k)):
            return k
    raise AssertionError("the plain run has no fresh n-gram")


@pytest.fixture(scope="module", params=[(1, "0"), (2, "0"), (1, "1"), (2, "1")],
                ids=["P1-native", "P2-native", "P1-twin", "P2-twin"])
def eng(request):
    P, py = request.param
    mp = pytest.MonkeyPatch()
    mp.setenv("LSD_PY_RUNTIME", py)
    try:
        e = _eng(P)
    finally:
        mp.undo()
    assert type(e.scheduler.core).__name__ == ("PySchedCore" if py == "1" else "SchedCore")
    T = e.generate_ids([PROMPT], [SamplingParams(max_new_tokens=N, **SEEDED)])[0]
    assert len(T) == N and len(set(T)) > 8
    return e, T


def _run(e, **kw):
    return e.generate_requests([PROMPT], [SamplingParams(max_new_tokens=N, **SEEDED, **kw)])[0]


def test_engine_stop_sequences(eng):
    e, T = eng
    k = _first_end(T, 3, 2)
    r = _run(e, stop_sequences=[T[k: k + 2]])
    assert r.output == T[:k] and (r.finish_reason, r.stop_reason) == ("stop", 0)
    r = _run(e, stop_sequences=[T[k: k + 2]], include_stop_in_output=True)
    assert r.output == T[:k + 2] and (r.finish_reason, r.stop_reason) == ("stop", 0)
    # the index is the one in list order; a sequence that never comes stays out of the way
    r = _run(e, stop_token_ids=[999], stop_sequences=[[998, 997], T[k: k + 2]])
    assert r.output == T[:k] and (r.finish_reason, r.stop_reason) == ("stop", 2)
    assert e.slots.available == e.slots.capacity


def test_engine_stop_token_ids(eng):
    e, T = eng
    k = _first_end(T, 2, 1)
    r = _run(e, stop_token_ids=[T[k]])
    assert r.output == T[:k] and (r.finish_reason, r.stop_reason) == ("stop", 0)
    r = _run(e, stop_token_ids=[T[k], T[k]], include_stop_in_output=True)
    assert r.output == T[:k + 1] and (r.finish_reason, r.stop_reason) == ("stop", 0)
    # token 1, the prefill draw
    r = _run(e, stop_token_ids=[T[0]])
    assert r.output == [] and (r.finish_reason, r.stop_reason) == ("stop", 0)
    # min_new_tokens: an occurrence among the first m tokens does not count
    j = next(i for i in range(k + 1, N) if T[i] == T[k]) if T[k] in T[k + 1:] else None
    r = _run(e, stop_token_ids=[T[k]], min_new_tokens=k + 1)
    assert r.output == (T[:j] if j is not None else T)
    assert r.finish_reason == ("stop" if j is not None else "length")


def test_engine_finish_reasons_without_stops(eng):
    e, T = eng
    r = _run(e)
    assert r.output == T and (r.finish_reason, r.stop_reason) == ("length", None)
    eos = e.mcfg.eos_token_id
    assert eos >= e.mcfg.vocab_size  # gpt2-test never draws its EOS by itself: force it through the bias
    r = e.generate_requests([PROMPT], [SamplingParams(max_new_tokens=0)])[0]
    assert r.output == [] and r.finish_reason == "length"


def test_engine_eos_reason():
    e = Engine(EngineConfig(model_id="llama-test", max_batch=4, device="cpu"))  # its EOS (2) is in the vocabulary
    eos = e.mcfg.eos_token_id
    sp = SamplingParams(greedy=True, max_new_tokens=8, stop_at_eos=True, min_new_tokens=3, logit_bias={eos: 100})
    r = e.generate_requests([[5, 6]], [sp])[0]
    assert r.output[-1] == eos and len(r.output) == 4 and (r.finish_reason, r.stop_reason) == ("eos", None)
    # EOS is checked first: also a stop token, still "eos"; without stop_at_eos it is a stop, dropped from the output
    r = e.generate_requests([[5, 6]], [SamplingParams(**{**sp.__dict__, "stop_token_ids": [eos]})])[0]
    assert r.output[-1] == eos and (r.finish_reason, r.stop_reason) == ("eos", None)
    r = e.generate_requests([[5, 6]], [SamplingParams(**{**sp.__dict__, "stop_token_ids": [eos], "stop_at_eos": False})])[0]
    assert len(r.output) == 3 and eos not in r.output and (r.finish_reason, r.stop_reason) == ("stop", 0)


def test_engine_neighbours_slot_reuse_and_logprobs(eng):
    e, T = eng
    k = _first_end(T, 3, 2)
    others = [SamplingParams(temperature=0.7, top_k=5, seed=3, max_new_tokens=30),
              SamplingParams(greedy=True, max_new_tokens=9)]
    prompts = [[4], [9, 8, 7, 6]]
    alone = e.generate_ids(prompts, others)
    stop = SamplingParams(max_new_tokens=N, stop_sequences=[T[k: k + 2]], logprobs=2, **SEEDED)
    plain_lp = e.generate_requests([PROMPT], [SamplingParams(max_new_tokens=N, logprobs=2, **SEEDED)])[0].logprobs
    got = e.generate_requests([prompts[0], PROMPT, prompts[1]], [others[0], stop, others[1]])
    assert [got[0].output, got[2].output] == alone          # neighbours draw what they draw alone
    assert got[1].output == T[:k] and got[1].finish_reason == "stop"
    assert got[0].finish_reason == got[2].finish_reason == "length"
    # logprob records are trimmed to the output, and are the plain run's (compared alone: other GEMM row counts
    # round the logits of a batch differently)
    assert got[1].logprobs.tokens == T[:k] and len(got[1].logprobs.token_logprobs) == k
    lp = e.generate_requests([PROMPT], [stop])[0].logprobs
    assert lp.tokens == T[:k] and len(lp.token_logprobs) == len(lp.top_logprobs) == k
    assert lp.token_logprobs == plain_lp.token_logprobs[:k] and lp.top_logprobs == plain_lp.top_logprobs[:k]
    kept = e.generate_requests([PROMPT], [SamplingParams(**{**stop.__dict__, "include_stop_in_output": True})])[0]
    assert kept.logprobs.tokens == T[:k + 2] and len(kept.logprobs.token_logprobs) == k + 2


@pytest.mark.parametrize("py", ["0", "1"])
def test_engine_stopped_slot_is_reused_by_a_queued_request(monkeypatch, py):
    """One KV slot: a request with a far length limit stops early, and the
    queued request behind it gets the slot long before that limit."""
    monkeypatch.setenv("LSD_PY_RUNTIME", py)
    e = _eng(max_batch=1)
    T = e.generate_ids([PROMPT], [SamplingParams(max_new_tokens=N, **SEEDED)])[0]
    k = _first_end(T, 2, 1)
    e.start_loop()
    try:
        a = e.submit(PROMPT, SamplingParams(max_new_tokens=900, stop_token_ids=[T[k]], **SEEDED))
        b = e.submit([4, 4], SamplingParams(greedy=True, max_new_tokens=3))
        assert a.wait(120) == T[:k] and a.finish_reason == "stop"
        assert len(b.wait(120)) == 3 and b.finish_reason == "length"
    finally:
        e.stop_loop()
    assert e.scheduler.stats["steps"] < 100  # nowhere near the 900 tokens of the length limit
    assert e.slots.available == e.slots.capacity == 1


# ---------------------------------------------------------------------------
# interfaces

def test_server_stop_fields(monkeypatch):
    import requests
    from fastapi.testclient import TestClient

    from llm_sharding_demo_amd import LLM
    from llm_sharding_demo_amd.serving import client as cl
    from llm_sharding_demo_amd.serving.server import create_app

    sent = {}

    class R:
        status_code = 200

        def json(self):
            return {"generated": "x"}

    def post(url, json=None, timeout=None):
        sent.update(json)
        return R()

    monkeypatch.setattr(requests, "post", post)
    cl.generate_text("Hi, ", stop=["a", "b"], stop_token_ids=[5], include_stop_in_output=True)
    assert sent["stop"] == ["a", "b"] and sent["stop_token_ids"] == [5] and sent["include_stop_in_output"] is True
    sent.clear()
    cl.generate_text("Hi, ")
    assert not {"stop", "stop_token_ids", "include_stop_in_output"} & set(sent)
    monkeypatch.undo()
    cfg = EngineConfig(model_id="gpt2-test", max_batch=4, device="cpu", role="coordinator")
    llm = LLM(cfg)
    tok = llm.tokenizer
    text = "abcabc"
    ids = tok.encode(text)
    # letters only, so that the output's text tokenises back to its tokens
    kw = dict(temperature=1.3, top_k=200, seed=17, allowed_token_ids=[tok.encode(ch)[0] for ch in "abcdefghij"])
    T = llm.engine.generate_ids([ids], [SamplingParams(max_new_tokens=N, **kw)])[0]
    assert tok.encode(tok.decode(T)) == T
    dec = lambda toks: tok.decode(ids + toks, skip_special_tokens=True)  # noqa: E731
    client = TestClient(create_app(cfg, engine=llm.engine))
    body = {"prompt": text, "max_new_tokens": N, **kw}
    # every existing response stays what it was: no new key unless a stop parameter is given
    assert client.post("/generate", json=body).json() == {"generated": dec(T)}
    assert client.post("/generate", json={**body, "include_stop_in_output": True}).json() == {"generated": dec(T)}
    k = _first_end(T, 2, 1)
    r = client.post("/generate", json={**body, "stop_token_ids": [T[k]]})
    assert r.status_code == 200 and r.json() == {"generated": dec(T[:k]), "finish_reason": "stop", "stop_reason": 0}
    r = client.post("/generate", json={**body, "stop_token_ids": [T[k]], "include_stop_in_output": True})
    assert r.json() == {"generated": dec(T[:k + 1]), "finish_reason": "stop", "stop_reason": 0}
    r = client.post("/generate", json={**body, "stop_token_ids": [999]})
    assert r.json() == {"generated": dec(T), "finish_reason": "length"}  # no "stop_reason" without a stop
    # stop as a string and as a list: tokenised with the server's tokenizer, as given
    k2 = _first_end(T, 2, 2)
    word = tok.decode(T[k2: k2 + 2])
    want = {"generated": dec(T[:k2]), "finish_reason": "stop", "stop_reason": 0}
    assert client.post("/generate", json={**body, "stop": word}).json() == want
    r = client.post("/generate", json={**body, "stop": ["ééé", word]})
    assert r.json() == {**want, "stop_reason": 1}
    r = client.post("/generate", json={**body, "stop": [word], "stop_token_ids": [999], "include_stop_in_output": True})
    assert r.json() == {"generated": dec(T[:k2 + 2]), "finish_reason": "stop", "stop_reason": 1}  # the ids come first
    for bad in (dict(stop_token_ids=[llm.engine.mcfg.vocab_size]), dict(stop_token_ids=[-1]), dict(stop=""),
                dict(stop=[""]), dict(stop=5), dict(stop_token_ids=list(range(17))), dict(stop=["a"] * 17),
                dict(stop_token_ids="3"), dict(include_stop_in_output="maybe")):
        assert client.post("/generate", json={**body, **bad}).status_code == 422, bad
    props = client.get("/openapi.json").json()["components"]["schemas"]["GenerateReq"]["properties"]
    assert {"stop", "stop_token_ids", "include_stop_in_output"} <= set(props)


def test_http_relay_stops_on_the_host(monkeypatch):
    import requests
    import torch

    from llm_sharding_demo_amd.serving.server import http_generate

    cfg = EngineConfig(model_id="gpt2-test", device="cpu")
    V = cfg.model.vocab_size
    logits = torch.linspace(0, 1, V).tolist()  # the argmax is V - 1

    class R:
        def __init__(self, body):
            self.body = body

        def raise_for_status(self):
            pass

        def json(self):
            return self.body

    def post(url, json=None, timeout=None):
        return R({"hidden_states": [[[0.0]]]} if "hidden_states" not in json else {"logits": [[logits]]})

    monkeypatch.setattr(requests, "post", post)
    sp = SamplingParams(greedy=True, max_new_tokens=6, stop_sequences=[[V - 1, V - 1, V - 1]])
    assert http_generate(cfg, [1], sp) == []
    assert http_generate(cfg, [1], sp, reasons=True) == ([], None, ("stop", 0))
    sp = SamplingParams(greedy=True, max_new_tokens=6, stop_token_ids=[V - 1], min_new_tokens=2, include_stop_in_output=True,
                        logprobs=1)
    out, lp, reason = http_generate(cfg, [1], sp, reasons=True)
    assert out == [V - 1] * 3 and reason == ("stop", 0) and len(lp.token_logprobs) == 3 and lp.tokens == out
    assert http_generate(cfg, [1], SamplingParams(greedy=True, max_new_tokens=2), reasons=True)[2] == ("length", None)


def test_cli_has_the_flags_and_stops(capsys):
    from llm_sharding_demo_amd.__main__ import main

    with pytest.raises(SystemExit):
        main(["generate", "--help"])
    text = capsys.readouterr().out
    assert all(f in text for f in ("--stop", "--stop-token-id", "--include-stop-in-output", "--bad-word"))
    from llm_sharding_demo_amd import LLM

    llm = LLM(EngineConfig(model_id="gpt2-test", device="cpu"))
    ids = llm.tokenizer.encode("abcabc")
    T = llm.engine.generate_ids([ids], [SamplingParams(greedy=True, max_new_tokens=6)])[0]
    dec = lambda toks: str({"generated": llm.tokenizer.decode(ids + toks, skip_special_tokens=True)}) + "\n"  # noqa: E731
    base = ["generate", "abcabc", "--model-id", "gpt2-test", "--device", "cpu", "--greedy", "--max-new-tokens", "6"]
    assert main(base) == 0
    assert capsys.readouterr().out == dec(T)
    assert main(base + ["--stop-token-id", str(T[0])]) == 0            # the prefill draw stops the request
    assert capsys.readouterr().out == dec([])
    assert main(base + ["--stop-token-id", "5", "--stop-token-id", str(T[0]), "--include-stop-in-output"]) == 0
    assert capsys.readouterr().out == dec(T[:1])
    assert main(base + ["--stop", "zz", "--bad-word", "zz"]) == 0      # texts the output never meets
    assert capsys.readouterr().out == dec(T)
