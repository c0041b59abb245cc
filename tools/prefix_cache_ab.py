#!/usr/bin/env python3
"""What the prefix cache costs and saves (EngineConfig.prefix_cache).

    python tools/prefix_cache_ab.py [--model gpt2-xl] [--cases serve,lone,burst] [--label NAME]

serve: closed-loop serving (tools/serve_load.py: 512 in flight, 2048 requests,
16-128 new tokens) on one engine whose cache is switched off and on between the
runs (max_batch = 512 + --spare-slots: entries need slots that no running
request holds),
alternating, 3 pairs per shared prefix of 0 / 64 / 128 / 512 tokens on prompts
of prefix + 16-128 tokens.  Per run: tok/s, TTFT p50 / p90, the hit rate, the
cache's counters and the device time of the kv_fork launches.  The 0-prefix
rows are the cost of the cache on traffic that cannot hit: lookups, and slots
held by entries until an admission takes them.

lone: one request at a time on an idle engine, max_new_tokens = 1: the TTFT of
a prompt of m + 16 tokens that hits m cached tokens against the same prompt
opted out (a miss), m = 1 .. 256, alternating, median of 15 -- the smallest m
at which the hit is no slower is what prefix_cache_min_tokens should be.

burst: 256 requests of 128 + 16 tokens that hit one 128-token entry in one
item (256 reads of one source in one kv_fork launch): the launch's device
time beside the prefill step's.

One JSON line per run."""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from serve_load import CopyTimer, cache_delta, closed_loop, latency  # noqa: E402

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams  # noqa: E402
from llm_sharding_demo_amd.runtime.engine import Engine, freeze_gc  # noqa: E402


def emit(a, **kw) -> None:
    print(json.dumps({"build": a.label, "model": a.model, **kw}), flush=True)


def serve(a) -> None:
    C = a.concurrency
    top = max(a.prefixes) + 128 + 128
    # ONE engine, its cache switched between the runs: the KV of 576 slots x 768 positions of GPT-2 XL
    # (136 GB) fits a card once, not twice, and everything but the cache is the same object in both arms
    eng = Engine(EngineConfig(model_id=a.model, num_stages=1, max_batch=C + a.spare_slots, max_seq_len=top,
                              num_microbatches=2, device=a.device, seed=0, metrics_every=0,
                              prefix_cache=C, prefix_cache_min_tokens=a.min_tokens))
    assert eng.kv_slots == C + a.spare_slots, f"only {eng.kv_slots} KV slots fit"

    def switch(entries):
        with eng._lock:  # idle: no session runs
            eng.scheduler.core.set_prefix_cache(entries, a.min_tokens)
            eng.scheduler._caching = entries > 0
            eng.cfg.prefix_cache = entries

    arms = {"off": 0, "on": C}
    V = eng.mcfg.vocab_size
    timer = CopyTimer(eng)
    for pre in a.prefixes:
        rnd = random.Random(pre)
        stem = [rnd.randrange(V) for _ in range(pre)]

        def make():
            return (stem + [rnd.randrange(V) for _ in range(rnd.randint(16, 128))],
                    SamplingParams(temperature=0.6, top_k=40, max_new_tokens=rnd.randint(16, 128),
                                   seed=rnd.randrange(1 << 30)))

        for name, entries in arms.items():  # warm-up: the graphs of this prompt mix, hits' tails included
            switch(entries)
            warm = [make() for _ in range(C)]
            eng.generate_ids([w[0] for w in warm], [w[1] for w in warm])
            warm = [make() for _ in range(C)]
            eng.generate_ids([w[0] for w in warm], [w[1] for w in warm])
        freeze_gc()
        for pair in range(a.pairs):
            for name, entries in arms.items():
                switch(entries)
                before = eng.prefix_cache_stats()
                timer.take()
                eng.start_loop()
                t0 = time.monotonic()
                done = closed_loop(eng, make, C, a.requests)
                el = time.monotonic() - t0
                eng.stop_loop()
                line = dict(case="serve", cache=name, shared_prefix=pre, pair=pair, concurrency=C, spare_slots=a.spare_slots,
                            requests=len(done), **latency(done, el))
                if name == "on":
                    n, ms = timer.take()
                    line.update(cache_delta(eng, before, done), kv_fork_launches=n, kv_fork_ms=ms)
                emit(a, **line)
    eng.shutdown()


def lone(a) -> None:
    eng = Engine(EngineConfig(model_id=a.model, num_stages=1, max_batch=8, max_seq_len=512, num_microbatches=2,
                              device=a.device, seed=0, metrics_every=0, prefix_cache=4, prefix_cache_min_tokens=1))
    V = eng.mcfg.vocab_size
    rnd = random.Random(1)

    def ttft(prompt, hit):
        r = eng.generate_requests([prompt], [SamplingParams(greedy=True, max_new_tokens=1, prefix_cache=hit)])[0]
        return (r.t_first - r.t_submit) * 1e3, r.cached_tokens

    for m in a.lone:
        stem = [rnd.randrange(V) for _ in range(m)]
        eng.prefix_cache_clear()
        eng.generate_requests([stem + [1]], [SamplingParams(greedy=True, max_new_tokens=1)])  # the entry
        res = {True: [], False: []}
        for k in range(3 + a.lone_runs):
            tail = [rnd.randrange(V) for _ in range(16)]
            for hit in (False, True):
                ms, cached = ttft(stem + tail, hit)
                assert cached in ((m, m + 1) if hit else (0,)), (cached, m, hit)  # m + 1: the tail began like the donor's
                if k >= 3:  # the first ones meet new shapes
                    res[hit].append(ms)
            eng.prefix_cache_clear()  # the tails' entries; then the stem's again
            eng.generate_requests([stem + [1]], [SamplingParams(greedy=True, max_new_tokens=1)])
        emit(a, case="lone", m=m, prompt_tokens=m + 16, runs=a.lone_runs,
             ttft_miss_ms=round(statistics.median(res[False]), 3), ttft_hit_ms=round(statistics.median(res[True]), 3),
             miss_min_max=[round(min(res[False]), 3), round(max(res[False]), 3)],
             hit_min_max=[round(min(res[True]), 3), round(max(res[True]), 3)])
    eng.shutdown()


def burst(a) -> None:
    N, PRE = 256, 128
    eng = Engine(EngineConfig(model_id=a.model, num_stages=1, max_batch=2 * N, max_seq_len=PRE + 16 + 16,
                              num_microbatches=2, device=a.device, seed=0, metrics_every=0, prefix_cache=2 * N,
                              prefix_cache_min_tokens=16))
    V = eng.mcfg.vocab_size
    rnd = random.Random(2)
    timer = CopyTimer(eng)
    sp = SamplingParams(temperature=0.6, top_k=40, max_new_tokens=8, seed=3)
    for rep in range(1 + a.pairs):  # the first one warms the shapes up
        for hit in (False, True):
            stem = [rnd.randrange(V) for _ in range(PRE)]
            prompts = [stem + [rnd.randrange(V) for _ in range(16)] for _ in range(N)]
            eng.prefix_cache_clear()
            if hit:
                eng.generate_requests([stem], [sp])
            timer.take()
            before = eng.prefix_cache_stats()
            t0 = time.perf_counter()
            rs = eng.generate_requests(prompts, [sp] * N, record_timing=True)
            wall = 1e3 * (time.perf_counter() - t0)
            n, ms = timer.take()
            ls = eng.last_session
            if rep:
                emit(a, case="burst", requests=N, entry_tokens=PRE, tail_tokens=16, hits=sum(r.cached_tokens > 0 for r in rs),
                     session_ms=round(wall, 2), prefill_ms=round(ls.prefill_ms, 3) if ls is not None else None,
                     kv_fork_launches=n, kv_fork_ms=ms, **{k: v for k, v in cache_delta(eng, before, rs).items()
                                                           if k in ("tokens_reused", "hit_rate")})
    eng.shutdown()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="gpt2-xl")
    ap.add_argument("--label", default="this")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--cases", default="serve,lone,burst")
    ap.add_argument("--concurrency", type=int, default=512)
    ap.add_argument("--requests", type=int, default=2048)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--prefixes", type=lambda s: [int(x) for x in s.split(",")], default=[0, 64, 128, 512])
    ap.add_argument("--min-tokens", type=int, default=8)
    ap.add_argument("--spare-slots", type=int, default=64,
                    help="serve: max_batch = concurrency + this many on both engines -- a hit needs its entry's "
                         "slot beside its own, so a pool that running requests fill cannot hit")
    ap.add_argument("--lone", type=lambda s: [int(x) for x in s.split(",")], default=[1, 2, 4, 8, 16, 32, 64, 128, 256])
    ap.add_argument("--lone-runs", type=int, default=15)
    a = ap.parse_args()
    for case in a.cases.split(","):
        {"serve": serve, "lone": lone, "burst": burst}[case](a)


if __name__ == "__main__":
    main()
