"""Closed-loop serving load on one engine: C requests in flight, each finished
request replaced by a new one, varied prompt and output lengths -- sequences
join and leave at every step (continuous batching), unlike bench.py's session
where the whole batch joins at step 0 and leaves together.  Prints one JSON
line: output tok/s, per-token latency and TTFT percentiles, steps and how many
items the native executor issued (steady / composition changes).

  python tools/serve_load.py --model gpt2-xl --concurrency 512 --requests 2048

--shared-prefix N: every prompt starts with the same N tokens (a system
prompt), followed by its own --prompt tokens; --prefix-cache E switches the
engine's prefix cache on (EngineConfig.prefix_cache), and the line gains the
cache's counters over the measured phase and the device time of its kv_fork
launches.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams  # noqa: E402
from llm_sharding_demo_amd.runtime.engine import Engine, freeze_gc  # noqa: E402


def closed_loop(eng, make, C, n):
    """n requests from make() -> (prompt, params), C in flight -> the finished requests."""
    live = [eng.submit(*make()) for _ in range(min(C, n))]
    sent, done = len(live), []
    while live:
        keep = []
        for r in live:
            if r.done:
                done.append(r)
                if sent < n:
                    keep.append(eng.submit(*make()))
                    sent += 1
            else:
                keep.append(r)
        live = keep
        time.sleep(0.0005)
    return done


def latency(done, el) -> dict:
    """tok/s, per-token latency and TTFT percentiles of `done`, finished in el seconds."""
    toks = sum(len(r.output) for r in done)
    tpot = [(r.t_done - r.t_first) / (len(r.output) - 1) * 1e3 for r in done if len(r.output) > 1]
    ttft = sorted((r.t_first - r.t_submit) * 1e3 for r in done)
    q = lambda v, f: v[min(len(v) - 1, int(f * len(v)))]  # noqa: E731
    return {"tok_s": round(toks / el, 1), "elapsed_s": round(el, 3),
            "per_token_ms_p50": round(statistics.median(tpot), 3), "ttft_ms_p50": round(q(ttft, 0.5), 2),
            "ttft_ms_p90": round(q(ttft, 0.9), 2)}


class CopyTimer:
    """Device time of an engine's kv_fork launches: events around every call of
    the stages' backend.kv_fork (never inside a capture), read after a sync."""

    def __init__(self, eng):
        import torch

        self.torch, self.pairs = torch, []
        for st in eng.stages:
            inner = st.backend.kv_fork

            def timed(*a, _inner=inner, **kw):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                _inner(*a, **kw)
                e.record()
                self.pairs.append((s, e))
            if eng.devices[0].type == "cuda":
                st.backend.kv_fork = timed

    def take(self) -> tuple:
        """(launches, their device ms in all) since the last take()."""
        if self.pairs:
            self.torch.cuda.synchronize()
        n, ms = len(self.pairs), sum(s.elapsed_time(e) for s, e in self.pairs)
        self.pairs.clear()
        return n, round(ms, 3)


def cache_delta(eng, before: dict, done) -> dict:
    """The prefix cache's counters since `before`, and the hit rate over `done`."""
    st = eng.prefix_cache_stats()
    return {"hits": st["hits"] - before["hits"], "misses": st["misses"] - before["misses"],
            "tokens_reused": st["tokens_reused"] - before["tokens_reused"],
            "evictions": st["evictions"] - before["evictions"], "entries": st["entries"],
            "hit_rate": round(sum(1 for r in done if r.cached_tokens) / max(1, len(done)), 4)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="gpt2-xl")
    p.add_argument("--concurrency", type=int, default=512)
    p.add_argument("--requests", type=int, default=2048)
    p.add_argument("--prompt", default="16,128", help="min,max prompt tokens")
    p.add_argument("--gen", default="16,128", help="min,max new tokens")
    p.add_argument("--microbatches", type=int, default=2)
    p.add_argument("--device", default="cuda")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--join-min", type=int, default=32, help="EngineConfig.join_min (join policy)")
    p.add_argument("--join-wait", type=int, default=4, help="EngineConfig.join_max_wait")
    p.add_argument("--warm-requests", type=int, default=0,
                   help="an unmeasured closed-loop phase of this many requests first (serving-shaped "
                        "graphs captured before the clock starts)")
    p.add_argument("--shared-prefix", type=int, default=0,
                   help="every prompt starts with the same N tokens, ahead of its --prompt tokens")
    p.add_argument("--prefix-cache", type=int, default=0, help="EngineConfig.prefix_cache (entries; 0 = off)")
    p.add_argument("--prefix-min-tokens", type=int, default=8, help="EngineConfig.prefix_cache_min_tokens")
    p.add_argument("--spare-slots", type=int, default=0,
                   help="max_batch = concurrency + this many: KV slots that entries can live in while "
                        "--concurrency requests hold theirs (a hit needs its entry's slot beside its own)")
    a = p.parse_args()
    pl, ph = map(int, a.prompt.split(","))
    gl, gh = map(int, a.gen.split(","))
    C = a.concurrency
    cfg = EngineConfig(model_id=a.model, num_stages=1, max_batch=C + a.spare_slots, max_seq_len=a.shared_prefix + ph + gh,
                       num_microbatches=a.microbatches, device=a.device, seed=a.seed,
                       metrics_every=1, join_min=a.join_min, join_max_wait=a.join_wait,  # per-stage busy fraction of the serving session
                       prefix_cache=a.prefix_cache, prefix_cache_min_tokens=a.prefix_min_tokens)
    eng = Engine(cfg)
    rnd = random.Random(a.seed)
    V = eng.mcfg.vocab_size
    stem = [rnd.randrange(V) for _ in range(a.shared_prefix)]

    def make():
        n = rnd.randint(pl, ph)
        return (stem + [rnd.randrange(V) for _ in range(n)],
                SamplingParams(temperature=0.6, top_k=40, max_new_tokens=rnd.randint(gl, gh),
                               seed=rnd.randrange(1 << 30)))

    # warm-up: every bucket / context graph the run can meet is captured once
    warm = [make() for _ in range(C)]
    eng.generate_ids([w[0] for w in warm], [w[1] for w in warm])
    freeze_gc()
    if getattr(eng, "_hostprof", None) is not None:
        eng._hostprof[:] = [0.0] * len(eng._hostprof)
    copies = CopyTimer(eng) if a.prefix_cache else None
    eng.start_loop()

    if a.warm_requests:
        closed_loop(eng, make, C, a.warm_requests)
    st0 = eng.scheduler.stats["steps"]
    n0 = sum(w.native_steps for w in eng.workers), sum(w.native_changes for w in eng.workers)
    pc0 = eng.prefix_cache_stats()
    if copies is not None:
        copies.take()
    t0 = time.monotonic()
    done = closed_loop(eng, make, C, a.requests)
    el = time.monotonic() - t0
    eng.stop_loop()
    line = {
        "model": a.model, "concurrency": C, "requests": len(done), "prompt": a.prompt, "gen": a.gen,
        **latency(done, el), "steps": eng.scheduler.stats["steps"] - st0,
        "native_steps": sum(w.native_steps for w in eng.workers) - n0[0],
        "native_changes": sum(w.native_changes for w in eng.workers) - n0[1],
        "native_changes_env": os.environ.get("LSD_NATIVE_CHANGES", "1"),
        "join_min": a.join_min, "join_wait": a.join_wait, "deferred_joins": eng.scheduler.stats.get("deferred"),
        "stage0_busy": (eng.last_session.stages[0]["busy_fraction"] if eng.last_session is not None
                        and eng.last_session.stages else None)}
    if a.shared_prefix or a.prefix_cache:
        line.update(shared_prefix=a.shared_prefix, prefix_cache=a.prefix_cache, spare_slots=a.spare_slots)
    if copies is not None:
        n, ms = copies.take()
        line.update(cache_delta(eng, pc0, done), kv_fork_launches=n, kv_fork_ms=ms)
    print(json.dumps(line), flush=True)
    hp = getattr(eng, "_hostprof", None)
    if hp is not None and hp[3]:
        print(f"host per decode-only step: plan {hp[0] / hp[3] * 1e6:.1f} us, issue {hp[1] / hp[3] * 1e6:.1f} us, "
              f"readout wait {hp[2] / hp[3] * 1e6:.1f} us over {hp[3]} steps", flush=True)
    if hp is not None and hp[10]:
        print(f"host per step with prefill chunks: issue {hp[8] / hp[10] * 1e6:.1f} us, readout wait "
              f"{hp[9] / hp[10] * 1e6:.1f} us over {hp[10]} steps", flush=True)
    eng.shutdown()


if __name__ == "__main__":
    main()
