"""Iteration-level request scheduler (continuous batching) + round watchdog.

Reference behaviour (`server.py:154-210`): every /generate
runs its own decode loop in FastAPI's threadpool; concurrent requests share
nothing and each pays the full per-token HTTP round trips (measured: 4
concurrent requests -> 0.83 tok/s aggregate vs 0.69 for one).

Here one scheduler (on the thread that drives pipeline stage 0) owns every
sequence and decides, at every decode step, a `StepPlan` (runtime/plan.py)
that all stages execute:

  * requests wait in an admission queue (the native `BatchQueue`,
    csrc/runtime/batch_queue.h) and JOIN a microbatch group at the next step
    boundary when the group has a free row and the replica a free KV slot;
    their prompts are prefilled by that step's item (chunked when
    PREFILL_CHUNK is set), and the final chunk's sample is their first token;
  * a sequence LEAVES its group at the step after its last token was
    scheduled (max_new_tokens) or after its EOS (stop_at_eos) or the end of
    one of its stop sequences was read back, so a short request never waits
    behind a long one;
  * decode rows are kept compacted and padded to a power-of-two bucket, so
    the per-(group, bucket) hipGraphs stay valid across steps and requests;
  * sampled token ids come back to the host asynchronously (D2H copy + event
    per item); the scheduler runs at most a few steps ahead of the GPU.

`Watchdog` puts a deadline on pipeline progress: if the
engine makes no progress for `round_timeout_s` (a hung RCCL peer, a dead
stage) it is marked unhealthy with a clear error and waiting requests fail
instead of hanging forever.
"""
from __future__ import annotations

import collections
import itertools
import logging
import threading
import time
from dataclasses import dataclass, field
from typing import Callable, Deque, Dict, List, Optional

import torch

from ..config import SamplingParams
from ..utils import racecheck
from .plan import Chunk, GroupPlan, Row, StepPlan, sampler_values

log = logging.getLogger("llm_sharding_demo_amd.scheduler")


class RequestTimeout(RuntimeError):
    pass


_FINISH = threading.Lock()  # orders Request.finish against a waiter creating its event


@dataclass
class Logprobs:
    """Records of a request that asked for logprobs (SamplingParams.logprobs = n),
    one entry per generated token: the token, its logprob, and the n most likely
    tokens at that draw as (id, logprob), most likely first."""
    tokens: List[int]
    token_logprobs: List[float]
    top_logprobs: List[List[tuple]]


@dataclass(eq=False)
class Request:
    """One generation request.  Light on purpose: a 4096-sequence session
    creates 4096 of these on the submitting thread, so the completion event
    is made only when someone actually blocks in wait() before the request
    finishes (a threading.Event per request was ~6 us of the ~14 us
    submit cost, profiles/r6_session_host.log)."""
    prompt_ids: List[int]
    params: SamplingParams
    t_submit: float = field(default_factory=time.monotonic)
    t_start: float = 0.0        # joined the pipeline (prefill issued)
    t_first: float = 0.0        # first token read back (TTFT = t_first - t_submit)
    t_done: float = 0.0
    output: Optional[List[int]] = None
    error: Optional[BaseException] = None
    logprobs: Optional[Logprobs] = None  # set before finish() when params.logprobs is not None
    finish_reason: Optional[str] = None  # "length" | "eos" | "stop", once finished without an error
    stop_reason: Optional[int] = None    # the matched stop sequence's index in params.stop_list(), with "stop"
    guide_row: int = -1  # the row of the last stage's guide table the engine pinned for params.guide (-1: none)
    cached_tokens: int = 0  # leading prompt tokens whose KV came from a prefix-cache entry (0: a miss, or no cache)
    _flag: bool = False
    _ev: Optional[threading.Event] = None
    # params.n > 1: the n samples in sample order, this request (sample 0) first;
    # each has its own output, logprobs and finish reason
    _samples: Optional[List["Request"]] = None

    @property
    def samples(self) -> List["Request"]:
        """The request's params.n samples in sample order; sample 0 is the
        request itself (`output` is sample 0's)."""
        return self._samples if self._samples is not None else [self]

    def fork_samples(self) -> None:
        """Make the n - 1 further samples of a request with params.n > 1."""
        n = self.params.n
        if n > 1 and self._samples is None:
            self._samples = [self] + [Request(self.prompt_ids, self.params, self.t_submit) for _ in range(n - 1)]

    def wait(self, timeout: Optional[float] = None) -> List[int]:
        """Sample 0's tokens, once every sample has finished; `timeout`
        bounds the whole wait, not each sample's."""
        if self._samples is not None:
            end = None if timeout is None else time.monotonic() + timeout
            for s in self._samples[1:]:
                s.wait(None if end is None else max(0.0, end - time.monotonic()))
            if end is not None:
                timeout = max(0.0, end - time.monotonic())
        if not self._flag:
            with _FINISH:
                if not self._flag and self._ev is None:
                    self._ev = threading.Event()
                ev = self._ev
            if ev is not None and not ev.wait(timeout):
                raise RequestTimeout(f"request not finished after {timeout} s")
        if self.error is not None:
            raise self.error
        return self.output

    @property
    def done(self) -> bool:
        """Finished, every sample of it."""
        if self._samples is not None:
            return self._flag and all(s._flag for s in self._samples[1:])
        return self._flag

    def finish(self, output=None, error=None) -> None:
        if self._samples is not None:
            for s in self._samples[1:]:
                # an error fails every sample; a request without tokens to draw has none anywhere
                if not s._flag and (error is not None or self.params.max_new_tokens == 0):
                    s.finish(output=None if error is not None else [], error=error)
        self.output, self.error = output, error
        if error is None and self.finish_reason is None:
            self.finish_reason = "length"
        self.t_done = time.monotonic()
        with _FINISH:
            self._flag = True
            ev = self._ev
        if ev is not None:
            ev.set()


class PyBatchQueue(racecheck.Shared):
    """Pure-Python twin of the native `BatchQueue` (csrc/runtime/batch_queue.h):
    same interface and grouping rule; the reference the tests compare the
    native queue against, and the fallback when _runtime.so is absent."""

    def __init__(self, max_batch: int, length_ratio: float = 4.0):
        if max_batch < 1 or length_ratio < 1.0:
            raise ValueError("max_batch >= 1 and length_ratio >= 1 required")
        self.max_batch, self.ratio = max_batch, length_ratio
        self._cv = racecheck.Condition(name="batch_queue")
        self._q: "collections.deque" = collections.deque()
        self._closed = False
        self.max_seen = 0
        self.pushed = self.popped = 0

    def push(self, id: int, max_new_tokens: int) -> bool:
        with self._cv:
            if self._closed:
                return False
            self._q.append((id, max(1, max_new_tokens)))
            self.pushed += 1
            self._cv.notify()
            return True

    def push_many(self, ids: List[int], max_new_tokens: List[int]) -> bool:
        if len(ids) != len(max_new_tokens):
            raise ValueError("push_many: length mismatch")
        with self._cv:
            if self._closed:
                return False
            self._q.extend((i, max(1, n)) for i, n in zip(ids, max_new_tokens))
            self.pushed += len(ids)
            self._cv.notify_all()
            return True

    def next_groups(self, window_s: float) -> List[List[int]]:
        with self._cv:
            self._cv.wait_for(lambda: self._closed or self._q)
            if self._closed:
                return []
            deadline = time.monotonic() + max(window_s, 0.0)
            batch = []
            while True:
                while self._q and len(batch) < self.max_batch:
                    batch.append(self._q.popleft())
                if len(batch) >= self.max_batch or self._closed:
                    break
                left = deadline - time.monotonic()
                if left <= 0 or not self._cv.wait_for(lambda: self._closed or self._q, left):
                    break
            self.popped += len(batch)
            self.max_seen = max(self.max_seen, len(batch))
        batch.sort(key=lambda it: it[1])
        groups: List[List[int]] = []
        first = 0
        for id_, n in batch:
            if not groups or n > self.ratio * first:
                groups.append([])
                first = n
            groups[-1].append(id_)
        return groups

    def try_pop(self, k: int) -> List[int]:
        """Up to k queued ids in FIFO order, without waiting."""
        with self._cv:
            out = []
            while self._q and len(out) < k:
                out.append(self._q.popleft()[0])
            self.popped += len(out)
            return out

    def wait_nonempty(self, timeout_s: float) -> bool:
        with self._cv:
            return self._cv.wait_for(lambda: self._closed or self._q, timeout_s)

    def close(self) -> None:
        with self._cv:
            self._closed = True
            self._cv.notify_all()

    def drain(self) -> List[int]:
        with self._cv:
            out = [i for i, _ in self._q]
            self._q.clear()
            return out

    @property
    def depth(self) -> int:
        with self._cv:
            return len(self._q)

    @property
    def closed(self) -> bool:
        return self._closed


def make_batch_queue(max_batch: int, length_ratio: float = 4.0, native: bool = True):
    """The native queue (GIL released while the scheduler waits) when
    _runtime.so is built, else the Python twin."""
    if native:
        from .native import load

        R = load()
        if R is not None and hasattr(R, "BatchQueue") and hasattr(R.BatchQueue, "try_pop"):
            return R.BatchQueue(max_batch, length_ratio)
    return PyBatchQueue(max_batch, length_ratio)


# ---------------------------------------------------------------------------
# Scheduler core: the per-step state machine (native csrc/runtime/sched_core.h,
# or this Python twin -- same interface, same plans, compared in
# tests/test_sched_core.py)
# ---------------------------------------------------------------------------

EV_FIRST, EV_FINISH, EV_RELEASE, EV_STOP = 1, 2, 4, 8
MAX_STOP_LEN = 32  # tokens of the longest stop sequence, and of the tail a sequence with stops keeps


@dataclass
class _Seq:
    prompt_len: int
    want: int
    stop_at_eos: bool
    rep: int = 0
    g: int = -1
    slot: int = -1
    prefilled: int = 0          # prompt tokens whose chunks have been issued
    issued: int = 0             # output tokens whose production has been issued
    pos: int = 0                # next decode input position
    sstep: int = 1              # sampler counter of the next decode draw
    ntok: int = 0               # tokens read back
    stop: bool = False          # EOS read back (stop_at_eos): leave at the next step
    toks: List[int] = field(default_factory=list)  # assign_collect only
    finished: bool = False
    # set_stops: (stop sequences as tuples, min_tokens) and the last generated
    # tokens they are matched against; None / unused without stop sequences
    stops: Optional[tuple] = None
    tail: Optional[List[int]] = None
    # families (add_fork): a fork's parent (-1: none) and the slot its KV is
    # copied from; ready once the parent's final chunk has been planned.
    # forks: the fork ids of a parent whose final chunk is not planned yet,
    # cleared when it is
    parent: int = -1
    src_slot: int = -1
    ready: bool = False
    forks: List[int] = field(default_factory=list)
    # prefix cache: the prompt's ids (None: the sequence opted out), whether it
    # looks an entry up at admission, and of a hit the entry's slot (pinned
    # until this sequence's first token) and whether its first chunk is still
    # to be planned
    prompt: Optional[tuple] = None
    lookup: bool = False
    hit_new: bool = False
    hit_slot: int = -1


@dataclass
class _Entry:
    """A prefix-cache entry: the slot's key (a finished sequence's prompt), the
    hits that pin it, and the tick of its insert or last hit."""
    toks: tuple
    pins: int = 0
    used: int = 0


@dataclass
class _Cache:
    """One replica's entries by slot, and the slots by their keys' first
    min_tokens tokens."""
    entries: Dict[int, _Entry] = field(default_factory=dict)
    index: Dict[tuple, List[int]] = field(default_factory=dict)


@dataclass
class _Produced:
    """Composition of one item that produced tokens: how to read its
    token-return vector [decode rows (b) | final prefill chunks]."""
    b: int
    rows: List[int]             # seq ids of decode rows [0, n)
    finals: List[int]           # seq ids whose final prefill chunk was sampled
    release: List[int] = field(default_factory=list)  # seqs whose last item this was


@dataclass
class _Group:
    rows: List[int] = field(default_factory=list)
    prefilling: List[int] = field(default_factory=list)
    prev: Optional[_Produced] = None
    waited: int = 0  # consecutive steps this group deferred its joins


def _bucket(n: int, cap: int) -> int:
    if n <= 0:
        return 0
    b = 1
    while b < n:
        b <<= 1
    return min(b, cap)


class PySchedCore:
    """Python twin of lsd_rt::SchedCore (LSD_PY_RUNTIME=1, or no native
    runtime).  plan(step) -> ([per replica: [(g, ret, n, b, ctxb, rows_changed,
    chunks [(sid, slot, start, len, final)], rows [(sid, slot, pos, sstep,
    src)])]], admitted sids); assign(...) -> [(sid, token, flags)]."""

    def __init__(self, replicas: int, groups: int, cap: int, prefill_budget: int, chunk: int,
                 max_seq: int, pools):
        self.R, self.M, self.cap = replicas, groups, cap
        self.budget, self.chunk, self.max_seq = prefill_budget, chunk, max_seq
        self.pools = list(pools)
        self.seqs: Dict[int, _Seq] = {}
        self.waiting: Deque[int] = collections.deque()
        self.groups = [[_Group() for _ in range(groups)] for _ in range(replicas)]
        self.expect: Dict[tuple, _Produced] = {}
        self.joins = self.leaves = self.max_rows = self.steps = 0
        self.join_min, self.max_wait, self.deferred = 1, 0, 0
        self._forks: List[tuple] = []
        self._hits: List[tuple] = []
        self.caches = [_Cache() for _ in range(replicas)]
        self.pc_max, self.pc_min, self.pc_tick = 0, 8, 0
        self.pc_hits = self.pc_misses = self.pc_tokens = self.pc_evictions = 0

    # -- the prefix cache (lsd_rt::SchedCore::set_prefix_cache has the rules) --
    def set_prefix_cache(self, max_entries: int, min_tokens: int) -> None:
        if max_entries < 0 or min_tokens < 1:
            raise ValueError("set_prefix_cache: max_entries >= 0, min_tokens >= 1")
        self.clear_prefix_cache()
        if any(c.entries for c in self.caches):
            raise RuntimeError("set_prefix_cache: entries are pinned by sequences in flight")
        self.pc_max, self.pc_min = max_entries, min_tokens

    def set_prompt(self, sid: int, tokens, lookup: bool = True) -> None:
        """lsd_rt::SchedCore::set_prompt: the prompt of a sequence that is not
        admitted yet (its forks share it); it leaves an entry behind, and with
        `lookup` it may start from one."""
        s = self.seqs.get(sid)
        if s is None:
            raise ValueError("set_prompt: unknown sequence")
        if s.slot >= 0 or s.g >= 0:
            raise ValueError("set_prompt: the sequence is admitted already")
        if len(tokens) != s.prompt_len:
            raise ValueError("set_prompt: not prompt_len tokens")
        s.prompt, s.lookup = tuple(tokens), bool(lookup)
        for fid in s.forks:
            self.seqs[fid].prompt = s.prompt

    def hits(self) -> List[tuple]:
        """(sid, m) of the prefix-cache hits among forks(), in plan order."""
        return list(self._hits)

    def prefix_cache_stats(self) -> tuple:
        """(entries, hits, misses, tokens reused, evictions)."""
        return (sum(len(c.entries) for c in self.caches), self.pc_hits, self.pc_misses, self.pc_tokens,
                self.pc_evictions)

    def prefix_entries(self, rep: int) -> List[tuple]:
        """(slot, pins, key) of replica rep's entries, by slot."""
        return [(slot, e.pins, list(e.toks)) for slot, e in sorted(self.caches[rep].entries.items())]

    def clear_prefix_cache(self) -> None:
        for rep, c in enumerate(self.caches):
            for slot in [slot for slot, e in c.entries.items() if e.pins == 0]:
                self._drop_entry(rep, slot)

    def _lookup(self, rep: int, toks: tuple) -> tuple:
        """The best entry of replica rep for `toks`: (m, slot), (0, -1) without."""
        L = len(toks)
        if L - 1 < self.pc_min:
            return 0, -1
        c = self.caches[rep]
        best, best_used, src = 0, -1, -1
        for slot in c.index.get(toks[: self.pc_min], ()):
            e = c.entries[slot]
            cp = 0
            for a, b in zip(e.toks, toks):
                if a != b:
                    break
                cp += 1
            m = min(cp, L - 1)
            if m >= self.pc_min and (m > best or (m == best and e.used > best_used)):
                best, best_used, src = m, e.used, slot
        return best, src

    def _drop_entry(self, rep: int, slot: int) -> None:
        c = self.caches[rep]
        e = c.entries.pop(slot)
        b = c.index[e.toks[: self.pc_min]]
        b.remove(slot)
        if not b:
            del c.index[e.toks[: self.pc_min]]
        self.pools[rep].free([slot])

    def _evict_lru(self, rep: int, keep: int) -> None:
        slot = min((e.used, slot) for slot, e in self.caches[rep].entries.items() if e.pins == 0 and slot != keep)[1]
        self._drop_entry(rep, slot)
        self.pc_evictions += 1

    def _insert_entry(self, rep: int, slot: int, toks: tuple) -> None:
        c, L = self.caches[rep], len(toks)
        if L < self.pc_min:
            self.pools[rep].free([slot])
            return
        covered = []
        for other in c.index.get(toks[: self.pc_min], ()):
            e = c.entries[other]
            n = len(e.toks)
            if n >= L and e.toks[:L] == toks:
                self.pc_tick += 1
                e.used = self.pc_tick  # the entry covers the new key
                self.pools[rep].free([slot])
                return
            if n < L and e.pins == 0 and toks[:n] == e.toks:
                covered.append(other)
        for other in covered:
            self._drop_entry(rep, other)
        if len(c.entries) >= self.pc_max:
            if all(e.pins for e in c.entries.values()):
                self.pools[rep].free([slot])
                return
            self._evict_lru(rep, -1)
        self.pc_tick += 1
        c.entries[slot] = _Entry(toks, 0, self.pc_tick)
        c.index.setdefault(toks[: self.pc_min], []).append(slot)

    def _unpin(self, s: "_Seq") -> None:
        if s.hit_slot < 0:
            return
        e = self.caches[s.rep].entries.get(s.hit_slot)
        if e is not None and e.pins > 0:
            e.pins -= 1
        s.hit_slot = -1

    def _release_slot(self, s: "_Seq") -> None:
        """A leaving sequence's slot: an entry when it has a prompt and the
        cache is on, else back to the pool."""
        self._unpin(s)
        if s.slot >= 0:
            if self.pc_max > 0 and s.prompt is not None:
                self._insert_entry(s.rep, s.slot, s.prompt)
            else:
                self.pools[s.rep].free([s.slot])

    def add_fork(self, sid: int, parent: int, want: int, stop_at_eos: bool) -> None:
        """lsd_rt::SchedCore::add_fork: a further sample of `parent`'s prompt.
        The parent must be known and still waiting; the fork takes its prompt
        length, is admitted with it (the family as a unit) and gets its one
        chunk (sid, slot, L - 1, 1, final) in the parent's group in the step
        after the parent's final chunk, ahead of the group's other chunks.  A
        prompt of one token has nothing to copy: a plain add()."""
        p = self.seqs.get(parent)
        if p is None:
            raise ValueError("add_fork: unknown parent")
        if p.slot >= 0 or p.g >= 0 or p.parent >= 0:
            raise ValueError("add_fork: the parent is admitted already, or is a fork itself")
        if sid in self.seqs:
            raise ValueError("add_fork: the sequence exists already")
        if p.prompt_len == 1:
            self.add(sid, 1, want, stop_at_eos)
            self.seqs[sid].prompt = p.prompt
            return
        self.seqs[sid] = _Seq(p.prompt_len, want, stop_at_eos, parent=parent, prompt=p.prompt)
        p.forks.append(sid)

    def forks(self) -> List[tuple]:
        """(sid, source slot) of the chunks of the last plan() that start behind a
        copy of another slot's KV, in plan order: the families' fork chunks and
        the first chunk of every prefix-cache hit."""
        return list(self._forks)

    def set_join_policy(self, join_min: int, max_wait: int) -> None:
        """lsd_rt::SchedCore::set_join_policy: admit only with room for every
        waiting request or for join_min of them, when the group is idle, or
        after max_wait deferred steps in a row."""
        if join_min < 1 or max_wait < 0:
            raise ValueError("join_min >= 1, max_wait >= 0")
        self.join_min, self.max_wait = join_min, max_wait

    def _join_ok(self, gh: "_Group", room: int, idle: bool) -> bool:
        if not self.waiting or room <= 0:
            gh.waited = 0
            return False
        if idle or room >= min(self.join_min, len(self.waiting)) or gh.waited >= self.max_wait:
            gh.waited = 0
            return True
        gh.waited += 1
        self.deferred += 1
        return False

    def add(self, sid: int, prompt_len: int, want: int, stop_at_eos: bool) -> None:
        if prompt_len <= 0:
            raise ValueError("empty prompt")
        self.seqs[sid] = _Seq(prompt_len, want, stop_at_eos)
        self.waiting.append(sid)

    def add_many(self, sids, prompt_lens, wants, stops) -> None:
        if not len(sids) == len(prompt_lens) == len(wants) == len(stops):
            raise ValueError("add_many: length mismatch")
        if any(n <= 0 for n in prompt_lens):
            raise ValueError("empty prompt")
        for a in zip(sids, prompt_lens, wants, stops):
            self.add(*a)

    def set_stops(self, sid: int, flat_tokens, lengths, min_tokens: int) -> None:
        """lsd_rt::SchedCore::set_stops: the stop sequences of a sequence that
        has no token yet, lengths[e] tokens of flat_tokens each, tried in this
        order against its last generated tokens; a match counts from token
        min_tokens + 1 on."""
        s = self.seqs.get(sid)
        if s is None:
            raise ValueError("set_stops: unknown sequence")
        if s.ntok > 0:
            raise ValueError("set_stops: the sequence has tokens already")
        if any(not 1 <= n <= MAX_STOP_LEN for n in lengths):
            raise ValueError("set_stops: a stop sequence holds 1 to 32 tokens")
        if sum(lengths) != len(flat_tokens):
            raise ValueError("set_stops: lengths do not add up to the tokens")
        if not lengths:
            s.stops = s.tail = None
            return
        ends = list(itertools.accumulate(lengths))
        s.stops = ([tuple(flat_tokens[e - n: e]) for n, e in zip(lengths, ends)], int(min_tokens))
        s.tail = []

    @staticmethod
    def _stop_match(s: "_Seq", tok: int) -> bool:
        """The token, the ntok-th of the sequence (already counted), goes into
        the tail; True when it completes a stop sequence and ntok > min_tokens."""
        tail = s.tail
        if len(tail) == MAX_STOP_LEN:
            del tail[0]
        tail.append(tok)
        words, min_tokens = s.stops
        if s.ntok <= min_tokens:
            return False
        return any(len(w) <= len(tail) and tuple(tail[len(tail) - len(w):]) == w for w in words)

    def has_work(self) -> bool:
        if self.waiting:
            return True
        return any(g.rows or g.prefilling or g.prev is not None for rep in self.groups for g in rep)

    @property
    def n_waiting(self) -> int:
        return len(self.waiting)

    @property
    def n_seqs(self) -> int:
        return len(self.seqs)

    @property
    def n_expect(self) -> int:
        return len(self.expect)

    def plan(self, step: int):
        admitted: List[int] = []
        out = []
        self._forks = []
        self._hits = []
        for rep in range(self.R):
            gs = []
            for g in range(self.M):
                go = self._group_plan(rep, g, step, admitted)
                if go is not None:
                    gs.append(go)
            out.append(gs)
        self.steps += 1
        return out, admitted

    def _admit(self, rep: int, g: int, room: int, admitted: List[int]) -> List[int]:
        pool = self.pools[rep]
        out = []
        cache = self.caches[rep]
        while self.waiting and room > 0 and pool.available + len(cache.entries) > 0:
            sid = self.waiting[0]
            s = self.seqs[sid]
            k = len(s.forks)
            if room < 1 + k:
                break  # a family is admitted as a unit
            if self.pc_max > 0:
                looks = s.lookup and s.prompt is not None
                m, src = self._lookup(rep, s.prompt) if looks else (0, -1)
                if pool.available < 1 + k:
                    # the slots that evictions could add: every unpinned entry but the match
                    spare = sum(1 for slot, e in cache.entries.items() if e.pins == 0 and slot != src)
                    if src >= 0 and pool.available + spare < 1 + k and cache.entries[src].pins == 0:
                        m, src = 0, -1  # the family does not fit beside the entry it matched: a miss
                        spare += 1
                    if pool.available + spare < 1 + k:
                        break
                    while pool.available < 1 + k:
                        self._evict_lru(rep, src)
                if looks and src >= 0:
                    e = cache.entries[src]
                    e.pins += 1
                    self.pc_tick += 1
                    e.used = self.pc_tick
                    s.hit_slot, s.hit_new, s.prefilled = src, True, m
                    self.pc_hits += 1
                    self.pc_tokens += m
                elif looks:
                    self.pc_misses += 1
            elif pool.available < 1 + k:
                break
            self.waiting.popleft()
            s.rep, s.g = rep, g
            s.slot = pool.alloc(1)[0]
            out.append(sid)
            admitted.append(sid)
            for fid in s.forks:
                f = self.seqs[fid]
                f.rep, f.g = rep, g
                f.slot = pool.alloc(1)[0]
                f.src_slot, f.prefilled = s.slot, f.prompt_len - 1
                out.append(fid)
                admitted.append(fid)
            room -= 1 + k
            self.joins += 1 + k
        return out

    def _group_plan(self, rep: int, g: int, step: int, admitted: List[int]):
        gh = self.groups[rep][g]
        prev, gh.prev = gh.prev, None
        ret = prev.b + len(prev.finals) if prev is not None else 0
        # leaves: every token scheduled, or EOS read back
        keep = []
        for sid in gh.rows:
            s = self.seqs[sid]
            if s.issued >= s.want or s.stop:
                self.leaves += 1
                if prev is not None:
                    prev.release.append(sid)
            else:
                keep.append(sid)
        new_rows = keep + (list(prev.finals) if prev is not None else [])
        changed = new_rows != gh.rows
        # joins (capacity counts rows + sequences still prefilling)
        room = self.cap - len(new_rows) - len(gh.prefilling)
        if self._join_ok(gh, room, not new_rows and not gh.prefilling):
            gh.prefilling += self._admit(rep, g, room, admitted)
        # prefill chunks (FIFO, one chunk per sequence per step, token budget)
        budget = self.budget or (1 << 62)
        chunks, finals = [], []
        pf = list(gh.prefilling)
        # forks whose parent's final chunk was planned in the previous step: one
        # token each, ahead of every other chunk, whatever the budget has left
        for sid in pf:
            s = self.seqs[sid]
            if s.parent < 0 or not s.ready:
                continue
            L = s.prompt_len
            budget -= 1
            chunks.append((sid, s.slot, L - 1, 1, True))
            self._forks.append((sid, s.src_slot))
            s.prefilled = L
            gh.prefilling.remove(sid)
            finals.append(sid)
            s.issued, s.pos, s.sstep = 1, L, 1
        for sid in pf:
            s = self.seqs[sid]
            if s.parent >= 0:
                continue  # a fork: planned above, or waiting for its parent's final chunk
            L = s.prompt_len
            n = L - s.prefilled if self.chunk <= 0 else min(self.chunk, L - s.prefilled)
            if chunks and n > budget:
                break
            budget -= n
            a = s.prefilled
            final = a + n == L
            chunks.append((sid, s.slot, a, n, final))
            if s.hit_new:  # the first chunk of a prefix-cache hit: behind a copy of [0, a)
                self._forks.append((sid, s.hit_slot))
                self._hits.append((sid, a))
                s.hit_new = False
            s.prefilled += n
            if final:
                gh.prefilling.remove(sid)
                finals.append(sid)
                s.issued, s.pos, s.sstep = 1, L, 1
                for fid in s.forks:  # their chunks: the next step
                    self.seqs[fid].ready = True
                s.forks = []
        # decode rows
        n = len(new_rows)
        b = _bucket(n, self.cap)
        rows = []
        if changed:
            old_index = {sid: i for i, sid in enumerate(gh.rows)}
            for sid in new_rows:
                s = self.seqs[sid]
                src = old_index[sid] if sid in old_index else prev.b + prev.finals.index(sid)
                rows.append((sid, s.slot, s.pos, s.sstep, src))
        ctxb = 0
        if n:
            top = max(self.seqs[sid].pos for sid in new_rows) + 1
            ctxb = min(-(-top // 256) * 256, self.max_seq)
            for sid in new_rows:  # this step issues one token per decode row
                s = self.seqs[sid]
                s.issued += 1
                s.pos += 1
                s.sstep += 1
        gh.rows = new_rows
        self.max_rows = max(self.max_rows, n)
        if b or finals:
            gh.prev = _Produced(b, list(new_rows), finals)
        if prev is not None:  # its readout comes back in this step's token-return vector
            self.expect[(rep, step, g)] = prev
        if not (ret or b or chunks):
            return None
        return (g, ret, n, b, ctxb, changed, chunks, rows)

    def assign(self, rep: int, step: int, g: int, tokens: List[int], eos: int):
        prod = self.expect.pop((rep, step, g))
        ev = []
        for i, sid in enumerate(prod.rows):
            self._give(sid, tokens[i], eos, ev)
        for j, sid in enumerate(prod.finals):
            self._give(sid, tokens[prod.b + j], eos, ev)
        for sid in prod.release:
            s = self.seqs.pop(sid, None)
            if s is None:
                continue
            self._release_slot(s)
            ev.append((sid, -1, EV_RELEASE | (0 if s.finished else EV_FINISH)))
        return ev

    def assign_collect(self, rep: int, step: int, g: int, tokens, eos: int):
        """Twin of SchedCore::assign_collect: only FIRST / FINISH / RELEASE
        events, plus (sid, tokens) of every sequence that finished."""
        prod = self.expect.pop((rep, step, g))
        tokens = [int(t) for t in tokens]
        ev, done = [], []
        for i, sid in enumerate(prod.rows):
            self._give_collect(sid, tokens[i], eos, ev, done)
        for j, sid in enumerate(prod.finals):
            self._give_collect(sid, tokens[prod.b + j], eos, ev, done)
        for sid in prod.release:
            s = self.seqs.pop(sid, None)
            if s is None:
                continue
            if not s.finished:
                done.append((sid, list(s.toks)))
            self._release_slot(s)
            ev.append((sid, -1, EV_RELEASE | (0 if s.finished else EV_FINISH)))
        return ev, done

    def _give_collect(self, sid: int, tok: int, eos: int, ev: list, done: list) -> None:
        s = self.seqs.get(sid)
        if s is None or s.finished or s.ntok >= s.want:
            return
        flags = EV_FIRST if s.ntok == 0 else 0
        if flags:
            self._unpin(s)
        s.ntok += 1
        s.toks.append(tok)
        hit = s.stops is not None and self._stop_match(s, tok)
        if s.stop_at_eos and tok == eos:
            s.stop = True
        elif hit:
            s.stop = True
            flags |= EV_STOP
        if s.ntok >= s.want or s.stop:
            s.finished = True
            flags |= EV_FINISH
            done.append((sid, list(s.toks)))
        if flags:
            ev.append((sid, tok, flags))

    def _give(self, sid: int, tok: int, eos: int, ev: list) -> None:
        s = self.seqs.get(sid)
        if s is None or s.finished or s.ntok >= s.want:
            return
        flags = EV_FIRST if s.ntok == 0 else 0
        if flags:
            self._unpin(s)
        s.ntok += 1
        hit = s.stops is not None and self._stop_match(s, tok)
        if s.stop_at_eos and tok == eos:
            s.stop = True
        elif hit:
            s.stop = True
            flags |= EV_STOP
        if s.ntok >= s.want or s.stop:
            s.finished = True
            flags |= EV_FINISH
        ev.append((sid, tok, flags))

    def reset(self) -> None:
        for s in self.seqs.values():
            if s.slot >= 0:
                self.pools[s.rep].free([s.slot])
        for rep, c in enumerate(self.caches):  # every entry, the pinned ones too: their sequences are gone
            self.pools[rep].free(list(c.entries))
        self.caches = [_Cache() for _ in range(self.R)]
        self.seqs.clear()
        self.waiting.clear()
        self.expect.clear()
        self._forks = []
        self._hits = []
        self.groups = [[_Group() for _ in range(self.M)] for _ in range(self.R)]


def make_sched_core(replicas: int, groups: int, cap: int, prefill_budget: int, chunk: int,
                    max_seq: int, pools):
    """The native core when the runtime is built and the slot pools are its
    allocators; the Python twin otherwise (LSD_PY_RUNTIME=1)."""
    from .native import load

    rt = load()
    if rt is not None and hasattr(rt, "SchedCore") and all(isinstance(p, rt.SlotAllocator) for p in pools):
        return rt.SchedCore(replicas, groups, cap, prefill_budget, chunk, max_seq, list(pools))
    return PySchedCore(replicas, groups, cap, prefill_budget, chunk, max_seq, pools)


# ---------------------------------------------------------------------------
# Scheduler
# ---------------------------------------------------------------------------

@dataclass
class _Meta:
    req: Request
    seed: int
    values: tuple = ((), ())  # plan.sampler_values: the chunk / row sampler fields
    logprobs: int = -1  # alternatives asked with every token's logprob (-1: no records)
    edits: Optional[tuple] = None  # SamplingParams.logit_edits: (tokens, values, untils) sorted by token
    context: Optional[tuple] = None  # SamplingParams.context_knobs: (repetition_penalty as fp32, no_repeat_ngram_size)
    mask: Optional[bytes] = None  # the bytes of SamplingParams.allowed_mask: the allowed list as packed int32 words
    stops: Optional[list] = None  # SamplingParams.stop_list: the stop sequences in the order they are tried
    bad: Optional[tuple] = None  # SamplingParams.bad_word_entries: (exclusive end offsets, tokens back to back)
    guide: int = -1  # Request.guide_row: the pinned row of the guide table, given back when the KV slot is released
    rep: int = 0        # replica and KV slot, from the request's first prefill chunk
    slot: int = -1
    done: bool = False  # finished by this scheduler (plain flag: the readout loop's hot path)


class Scheduler(racecheck.Shared):
    """Continuous-batching scheduler for one engine (every pipeline replica).

    Runs on the thread that drives stage 0 of replica 0 (`Engine._drive`);
    `submit()` is thread-safe.  The per-step state machine lives in the
    scheduler core (`make_sched_core`); this class owns the request futures,
    the sampling parameters, the plan objects and the GPU readouts."""

    def __init__(self, engine, groups: int, cap: int):
        self.eng = engine
        self.R = engine.R
        self.M, self.cap = groups, cap
        self.queue = make_batch_queue(max(1, cap * groups * self.R))
        self._pending: Dict[int, Request] = {}
        self._ids = itertools.count()
        self._plock = racecheck.Lock("sched.pending")
        self.meta: Dict[int, _Meta] = {}
        self.core = make_sched_core(self.R, groups, cap, engine.cfg.prefill_budget,
                                    engine.cfg.prefill_chunk, engine.max_seq, engine.slot_pools)
        self.core.set_join_policy(max(1, engine.cfg.join_min), max(0, engine.cfg.join_max_wait))
        self.step = 0
        self.readouts: Deque[tuple] = collections.deque()  # (step, ready(), sync(), tokens, key)
        self.lock = racecheck.RLock("sched.driver")         # one driver at a time
        self.timing = False
        self.step_log: List[tuple] = []                     # (step, had_prefill) of timed steps
        self.stats = {"steps": 0, "joins": 0, "leaves": 0, "max_rows": 0, "captures": 0, "deferred": 0}
        self._rng = engine._rng
        self._edited = 0  # live requests with logit edits: _group looks at chunks and rows only then
        self._contexts = 0  # live requests with repetition_penalty / no_repeat_ngram_size, likewise
        self._allowing = 0  # live requests with allowed_token_ids, likewise
        self._badwords = 0  # live requests with bad_words, likewise
        self._guided = 0  # live requests that follow a guide, likewise
        self._forking = 0  # forks whose chunk is not planned yet: build_step asks the core for forks() only then
        # the prefix cache (EngineConfig.prefix_cache entries per replica): on, every
        # step asks the core for forks() and hits(), and opted-in requests hand
        # it their prompts.  A request that reads its prompt on the last stage
        # (repetition_penalty, no_repeat_ngram_size, bad_words) never starts
        # from an entry -- DrawStage clones a source slot's prompt ids only for
        # family forks, an entry's row is not kept valid -- but leaves one
        self._caching = engine.cfg.prefix_cache > 0
        if self._caching:
            self.core.set_prefix_cache(engine.cfg.prefix_cache, engine.cfg.prefix_cache_min_tokens)

    # -- admission ---------------------------------------------------------
    def submit(self, prompt_ids: List[int], params: SamplingParams, guide_row: int = -1) -> Request:
        """guide_row: the guide-table row the engine pinned for params.guide;
        the pin goes back (Engine.unpin_guide) when the request's KV slot is
        released, or here when the request never gets one."""
        req = Request(list(map(int, prompt_ids)), params)
        req.guide_row = guide_row
        req.fork_samples()
        if params.max_new_tokens == 0:
            for _ in range(params.n):  # one pin per sample
                self.eng.unpin_guide(guide_row)
            req.finish([])
            return req
        rid = next(self._ids)
        with self._plock:
            racecheck.note(self, "_pending")
            self._pending[rid] = req
        if not self.queue.push(rid, params.max_new_tokens):
            with self._plock:
                racecheck.note(self, "_pending")
                self._pending.pop(rid, None)
            raise RuntimeError("scheduler is closed")
        return req

    def submit_many(self, prompts: List[List[int]], params: List[SamplingParams],
                    guide_rows: Optional[List[int]] = None) -> List[Request]:
        """submit() for a whole batch: one pass under the pending-map lock
        (a 4096-sequence bench session submits everything at once)."""
        now = time.monotonic()
        # a list whose first token is a Python int is taken as a list of ints
        # and only copied (list(map(int, .)) per 64-token prompt was ~4 us,
        # 17 ms of a 4096-prompt session); anything else is converted
        reqs = [Request(list(p) if type(p) is list and p and type(p[0]) is int else list(map(int, p)), sp, now)
                for p, sp in zip(prompts, params)]
        if guide_rows is not None:  # submit's guide_row, per request
            for req, row in zip(reqs, guide_rows):
                req.guide_row = row
        live = []
        for req in reqs:
            if req.params.n > 1:
                req.fork_samples()
            if req.params.max_new_tokens == 0:
                if req.guide_row >= 0:
                    for _ in range(req.params.n):  # one pin per sample
                        self.eng.unpin_guide(req.guide_row)
                req.finish([])
            else:
                live.append((next(self._ids), req))
        with self._plock:
            racecheck.note(self, "_pending")
            self._pending.update(live)
        if not self.queue.push_many([rid for rid, _ in live], [r.params.max_new_tokens for _, r in live]):
            with self._plock:
                racecheck.note(self, "_pending")
                for rid, _ in live:
                    self._pending.pop(rid, None)
            raise RuntimeError("scheduler is closed")
        return reqs

    @property
    def queue_depth(self) -> int:
        return self.queue.depth + self.core.n_waiting

    def _take_new(self) -> None:
        ids = self.queue.try_pop(1 << 20)
        if not ids:
            return
        with self._plock:
            racecheck.note(self, "_pending")
            reqs = [self._pending.pop(i) for i in ids]
        meta, rng = self.meta, self._rng
        lens, wants, stops, asking, forks = [], [], [], [], []
        samples = []  # (sid, its Request, seed) of every sample: n per request, sample 0 under the request's id
        for i, req in zip(ids, reqs):
            p = req.params
            seed = p.seed if p.seed is not None else rng.getrandbits(62)
            samples.append((i, req, seed))
            lens.append(len(req.prompt_ids))
            wants.append(p.max_new_tokens)
            stops.append(bool(p.stop_at_eos))
            if p.n > 1:
                # samples 1 .. n - 1: sequences of their own that fork from sample
                # 0's KV (core.add_fork), sample k drawing with seed + k
                for k, sub in enumerate(req.samples[1:], 1):
                    fid = next(self._ids)
                    sub.guide_row = req.guide_row
                    samples.append((fid, sub, seed + k))
                    forks.append((fid, i, p.max_new_tokens, bool(p.stop_at_eos)))
        for i, req, seed in samples:
            p = req.params
            meta[i] = _Meta(req, seed, sampler_values(p, seed), -1 if p.logprobs is None else int(p.logprobs))
            if p.has_logit_edits:
                meta[i].edits = p.logit_edits(self.eng.mcfg.eos_token_id)
                self._edited += 1
            if p.has_context:
                meta[i].context = p.context_knobs()
                self._contexts += 1
            if p.allowed_token_ids is not None:
                meta[i].mask = p.allowed_mask(self.eng.mask_words).tobytes()
                self._allowing += 1
            if p.bad_words is not None and p.bad_word_entries() is not None:  # an empty list asks for nothing
                meta[i].bad = p.bad_word_entries()
                self._badwords += 1
            if req.guide_row >= 0:
                meta[i].guide = req.guide_row
                self._guided += 1
            if p.stop_token_ids or p.stop_sequences:
                asking.append((i, p))
        self.core.add_many(ids, lens, wants, stops)
        for f in forks:  # behind their parents, ahead of any plan: the parents are still waiting
            self.core.add_fork(*f)
        # those with a KV copy ahead: a one-token prompt's samples are plain sequences
        self._forking += sum(1 for f in forks if len(meta[f[0]].req.prompt_ids) > 1)
        if self._caching:  # the prompts of the requests that did not opt out (their forks share them)
            for i, req in zip(ids, reqs):
                p = req.params
                if p.prefix_cache:
                    self.core.set_prompt(i, req.prompt_ids, meta[i].context is None and meta[i].bad is None)
        for i, p in asking:  # the requests with stop sequences alone: the core matches their last tokens
            st = meta[i].stops = p.stop_list()
            self.core.set_stops(i, [t for w in st for t in w], [len(w) for w in st], p.min_new_tokens)

    def has_work(self) -> bool:
        """Anything left to plan OR to read back: token readouts still queued
        here, or expected by the core (replica > 0 readouts arrive later over
        the control plane), keep a serving session alive until they land."""
        return (bool(self.queue.depth) or self.core.has_work() or bool(self.readouts)
                or self.core.n_expect > 0)

    # -- plan building ---------------------------------------------------------
    def build_step(self) -> Optional[List[StepPlan]]:
        """Plans of the next step for every replica, or None when idle."""
        self._take_new()
        if not self.core.has_work():
            return None
        s = self.step
        self.step += 1
        per_rep, admitted = self.core.plan(s)
        if admitted:
            now = time.monotonic()
            for sid in admitted:
                self.meta[sid].req.t_start = now
        # (fork sid -> source slot) of this step's fork chunks
        fk = dict(self.core.forks()) if self._forking or self._caching else None
        if self._caching and fk:
            # the prefix-cache hits among them: no family fork, and the request learns its m
            for sid, m in self.core.hits():
                self.meta[sid].req.cached_tokens = m
                self._forking += 1  # _group counts every chunk it finds in fk down
        plans = [StepPlan(step=s, groups=[self._group(go, rep, fk) for go in gos], replica=rep,
                          timing=self.timing) for rep, gos in enumerate(per_rep)]
        c = self.core
        self.stats.update(steps=self.stats["steps"] + 1, joins=c.joins, leaves=c.leaves,
                          max_rows=c.max_rows, deferred=c.deferred)
        if self.timing:
            self.step_log.append((s, any(gp.chunks for p in plans for gp in p.groups)))
        return plans

    def _group(self, go, rep: int = 0, fk: Optional[dict] = None) -> GroupPlan:
        g, ret, n, b, ctxb, changed, chunks, rows = go
        gp = GroupPlan(g, ret=ret, n=n, b=b, ctxb=ctxb)
        meta = self.meta
        for sid, slot, start, _, _ in chunks:
            # where _finish fetches the logprob records: noted at the chunk that opens the prompt
            if (start == 0 or (fk and sid in fk)) and meta[sid].logprobs >= 0:
                meta[sid].rep, meta[sid].slot = rep, slot
        gp.chunks = [Chunk(sid, slot, start, m.req.prompt_ids[start:start + ln], final, *h, *t)
                     for sid, slot, start, ln, final in chunks for m in (meta[sid],) for h, t in (m.values,)]
        if fk:
            for c in gp.chunks:
                src = fk.get(c.seq)
                if src is not None:
                    c.fork = src
                    self._forking -= 1
        if changed:
            gp.rows = [Row(sid, slot, pos, *h, sstep, src, *t)
                       for sid, slot, pos, sstep, src in rows for h, t in (meta[sid].values,)]
        if self._edited:
            # requests with logit edits: every chunk and row says how many
            # entries, the final chunk brings them (the last stage writes them
            # to the slot's table ahead of the prefill draw)
            for c in gp.chunks:
                ed = meta[c.seq].edits
                if ed is not None:
                    c.nedits = len(ed[0])
                    if c.final:
                        c.edits = ed
            if changed:
                for r in gp.rows:
                    ed = meta[r.seq].edits
                    if ed is not None:
                        r.nedits = len(ed[0])
        if self._contexts:
            # requests with a repetition penalty or an n-gram ban: every chunk
            # brings the knobs and the prompt's length (the last stage copies
            # its ids into the slot's context), every row the gate
            for c in gp.chunks:
                m = meta[c.seq]
                if m.context is not None:
                    (c.rpen, c.ngram), c.plen = m.context, len(m.req.prompt_ids)
            if changed:
                for r in gp.rows:
                    if meta[r.seq].context is not None:
                        r.ctx = 1
        if self._allowing:
            # requests with allowed_token_ids: every chunk and row carries the
            # gate, the final chunk the packed mask (the last stage writes it to
            # the slot's table ahead of the prefill draw)
            for c in gp.chunks:
                mk = meta[c.seq].mask
                if mk is not None:
                    c.allow = 1
                    if c.final:
                        c.mask = mk
            if changed:
                for r in gp.rows:
                    if meta[r.seq].mask is not None:
                        r.allow = 1
        if self._badwords:
            # requests with bad_words: every chunk says how many sequences and
            # is a context chunk (the pass reads the slot's prompt + draws, so
            # the prompt's length and ids travel as with an n-gram ban), the
            # final chunk brings the entries, every row both gates
            for c in gp.chunks:
                m = meta[c.seq]
                if m.bad is not None:
                    c.nbad, c.plen = len(m.bad[0]), len(m.req.prompt_ids)
                    if c.final:
                        c.bad = m.bad
            if changed:
                for r in gp.rows:
                    if meta[r.seq].bad is not None:
                        r.bad = r.ctx = 1
        if self._guided:
            # requests that follow a guide: every chunk names the guide's row
            # of the last stage's table (the final chunk's stage starts the
            # slot's state there), every row carries the gate
            for c in gp.chunks:
                c.guide = meta[c.seq].guide
            if changed:
                for r in gp.rows:
                    if meta[r.seq].guide >= 0:
                        r.guide = 1
        if changed:
            gp.edit = bool(self._edited) and any(r.nedits for r in gp.rows)
            gp.ctx = bool(self._contexts or self._badwords) and any(r.ctx for r in gp.rows)
            gp.allow = bool(self._allowing) and any(r.allow for r in gp.rows)
            gp.bad = bool(self._badwords) and any(r.bad for r in gp.rows)
            gp.guide = bool(self._guided) and any(r.guide for r in gp.rows)
        return gp

    # -- token readout -----------------------------------------------------------
    def on_readout(self, plan: StepPlan, gp: GroupPlan, ret: torch.Tensor) -> None:
        """Stage-0 worker callback: the token-return vector of group gp.g's
        previous item is in `ret` (in stream order): copy it to the host."""
        key = (plan.replica, plan.step, gp.g)
        n = gp.ret
        if ret.is_cuda:
            from ..parallel.pipeline import GPU_GATE, wait_event

            host = torch.empty(n, dtype=torch.int32, pin_memory=True)
            host.copy_(ret[:n], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()

            # the coordinator thread polls these beside the stage threads: never
            # in the middle of a sibling's hipGraph capture (HIP refuses event
            # queries then -- hipErrorCapturedEvent -- and invalidates the
            # capture), so each query / wait holds the capture gate shared
            def ready(ev=ev):
                with GPU_GATE.shared():
                    return ev.query()

            def sync(ev=ev):
                wait_event(ev)
            self.readouts.append((plan.step, ready, sync, host, key, None))
        else:
            host = ret[:n].clone()
            self.readouts.append((plan.step, lambda: True, lambda: None, host, key, None))

    def on_readout_native(self, plan: StepPlan, gp: GroupPlan, host: torch.Tensor, ev, release) -> None:
        """Stage-0 native executor callback: the D2H copy of group gp.g's
        previous token-return vector into `host` and its completion event
        `ev` are already enqueued (csrc/stage_exec.cpp); `release(ev)` hands
        the event back to the worker's pool once the readout is applied."""
        from ..parallel.pipeline import GPU_GATE, wait_event

        def ready(ev=ev):
            with GPU_GATE.shared():
                return ev.query()

        def sync(ev=ev):
            wait_event(ev)
        self.readouts.append((plan.step, ready, sync, host, (plan.replica, plan.step, gp.g),
                              lambda ev=ev: release(ev)))

    def push_remote_readout(self, step: int, tokens: List[int], prod_key) -> None:
        """Replica > 0 readouts arrive over the control plane (dist + DP)."""
        host = torch.tensor(tokens, dtype=torch.int32)
        self.readouts.append((step, lambda: True, lambda: None, host, tuple(prod_key), None))

    def poll(self, block_until_step: Optional[int] = None) -> None:
        """Process completed readouts (in order).  With block_until_step,
        wait for every readout of steps <= that one."""
        while self.readouts:
            step, ready, sync, host, key, release = self.readouts[0]
            if not ready():
                if block_until_step is None or step > block_until_step:
                    return
                sync()
            self.readouts.popleft()
            self._assign(host, key)
            if release is not None:
                release()

    def _assign(self, host: torch.Tensor, key) -> None:
        """Apply one group readout.  The core keeps every sequence's tokens
        (assign_collect): a plain token of a running sequence costs nothing
        here, only first tokens (TTFT), finishes and slot releases come back --
        a per-row Python loop at 16 groups x 256 rows per step used to be
        stage 0's largest host cost (profiles/r3_rehearsal_all_configs.log)."""
        rep, step, g = key
        events, done = self.core.assign_collect(rep, step, g, host.numpy(), self.eng.mcfg.eos_token_id)
        if not events:
            return
        now = time.monotonic()
        done = dict(done)
        get = self.meta.get
        for sid, tok, flags in events:
            if flags & EV_RELEASE:
                m = self.meta.pop(sid, None)
                if m is not None and m.edits is not None:
                    self._edited -= 1
                if m is not None and m.context is not None:
                    self._contexts -= 1
                if m is not None and m.mask is not None:
                    self._allowing -= 1
                if m is not None and m.bad is not None:
                    self._badwords -= 1
                if m is not None and m.guide >= 0:
                    # the last item that held one of its rows has been read back:
                    # nothing enqueued or in flight reads the guide's row for it
                    self._guided -= 1
                    self.eng.unpin_guide(m.guide)
                if m is not None and flags & EV_FINISH and not m.done:
                    m.done = True
                    self._finish(m, done.get(sid, []))
                continue
            m = get(sid)
            if m is None or m.done:
                continue
            if flags & EV_FIRST:
                m.req.t_first = now
            if flags & EV_FINISH:
                m.done = True
                self._finish(m, done[sid])

    def _finish(self, m: _Meta, toks: List[int]) -> None:
        """Finish a request with its tokens; one that asked for logprobs gets
        records [0, len(toks)) of its KV slot from the last stage first.  The
        slot is still the request's: it goes back to the pool after this
        readout at the earliest, and draws issued past the last token write
        records at or past len(toks) only."""
        p = m.req.params
        if p.stop_at_eos and toks and toks[-1] == self.eng.mcfg.eos_token_id:
            m.req.finish_reason = "eos"
        elif m.stops is not None:
            # the rule the core stopped by: its first counting match ends the collected tokens
            hit = p.stop_match(toks, m.stops)
            if hit is not None:
                m.req.finish_reason, m.req.stop_reason = "stop", hit
                if not p.include_stop_in_output:
                    toks = toks[: len(toks) - len(m.stops[hit])]
        n = m.logprobs
        if n >= 0:
            try:
                lt, li, lv = self.eng.fetch_logprobs(m.rep, m.slot, len(toks))
            except BaseException as e:  # noqa: BLE001 - the request fails, the engine goes on
                m.req.finish(error=e)
                return
            ids, vals = li[:, :n].tolist(), lv[:, :n].tolist()
            m.req.logprobs = Logprobs(list(toks), lt.tolist(),
                                      [[(i, v) for i, v in zip(a, b) if i >= 0] for a, b in zip(ids, vals)])
        m.req.finish(toks)

    # -- failure -----------------------------------------------------------------
    def fail_all(self, err: BaseException) -> None:
        for m in self.meta.values():
            if not m.req.done:
                m.done = True
                m.req.finish(error=err)
        self.meta.clear()
        self._edited = self._contexts = self._allowing = self._badwords = self._guided = self._forking = 0
        self.eng.unpin_guide(None)
        self.core.reset()
        self.readouts.clear()
        with self._plock:
            pend = list(self._pending.values())
            self._pending.clear()
        for rid in self.queue.drain():
            pass
        for req in pend:
            req.finish(error=err)


class Watchdog:
    """Marks the engine unhealthy when the pipeline stops making progress or
    the data plane reports an asynchronous error, and then aborts the data
    plane: with the native RCCL transport a kernel waiting on a dead or
    stalled peer would otherwise spin forever (and every host thread waiting
    on its stream with it); ncclCommAbort makes it return, the waits drain
    and the requests fail instead of hanging (the reference
    fails a request after its 30 s HTTP timeout, server.py:173-174)."""

    def __init__(self, engine, round_timeout_s: float, poll_s: float = 0.25):
        self.engine = engine
        self.timeout = round_timeout_s
        self.poll = poll_s
        self.fired = False
        self._stop = threading.Event()
        self._thread = threading.Thread(target=self._loop, name="lsd-watchdog", daemon=True)
        self._thread.start()

    def _loop(self) -> None:
        while not self._stop.wait(self.poll):
            if self.fired:
                continue
            tr = getattr(self.engine, "data_plane", None) or getattr(self.engine, "transport", None)
            try:
                err = tr.check_async() if tr is not None else None
            except Exception as e:  # noqa: BLE001 - a broken communicator is an error too
                err = f"{type(e).__name__}: {e}"
            if err:
                self._fire("DataPlaneError", err)
                continue
            started = getattr(self.engine, "round_started", None)
            if started is None:
                continue
            elapsed = time.monotonic() - started
            if elapsed > self.timeout:
                self._fire("WatchdogTimeout",
                           f"no pipeline progress for {elapsed:.3g} s (deadline {self.timeout:.3g} s)")

    def _fire(self, kind: str, msg: str) -> None:
        self.fired = True
        log.error("watchdog: %s: %s; marking engine unhealthy and aborting the data plane", kind, msg)
        self.engine.healthy = False
        self.engine.last_error = f"{kind}: {msg}"
        tr = getattr(self.engine, "data_plane", None) or getattr(self.engine, "transport", None)
        if tr is not None:
            try:
                tr.abort()
            except Exception as e:  # noqa: BLE001
                log.error("watchdog: data-plane abort failed: %s", e)

    def close(self) -> None:
        self._stop.set()
        self._thread.join(timeout=5)
