#!/usr/bin/env python3
"""What per-request n costs and saves (csrc/kernels/kv_fork.hip).

    python tools/fork_ab.py [--label NAME] [--skip-kernel] [--skip-e2e]

Kernel: kv_fork over a one-stage KV allocation of GPT-2 XL (48 layers, 25 kv
heads, head_dim 64) and Llama-3 8B (32 layers, 8 kv heads, head_dim 128), bf16,
max_seq 1024, for prompts of L = 128 and 1024 tokens (L - 1 positions are
copied) with 1, 3 and 7 forks of one parent, per launch, against the torch
slice assignment of the same bytes (ops/reference.py kv_fork on the device).
Every launch works on another family of slots, round-robin over all the slots
of the allocation, so a launch does not find the previous one's lines in
cache; the index vectors are on the device beforehand.  Times are device
events around a loop of launches, median of 5 rounds.  `bytes`: read + written,
F x runs x (L - 1) x head_dim x 2 x 2; `TB/s` = bytes / time.

End to end: GPT-2 XL on one stage, 128 random prompts of 128 tokens x n = 4, 128
new tokens, against the same 512 sequences submitted as 512 requests (each
prompt four times with seeds base .. base + 3): session wall time and the time
of the steps that carried prefill chunks (SessionStats.prefill_ms; the forks'
one-token chunks count), alternating, 3 pairs after a warm-up of each.

One JSON line per case."""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fns, rounds=5) -> tuple:
    """(median, min, max) device us per call of the callables run in order."""
    for fn in fns[: min(len(fns), 4)]:
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for fn in fns:
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) * 1e3 / len(fns))
    return statistics.median(out), min(out), max(out)


def kernel_cases(label: str) -> None:
    from llm_sharding_demo_amd.ops import reference as ref
    from llm_sharding_demo_amd.ops.hip import HipBackend

    be = HipBackend()
    S, max_seq = 32, 1024
    for model, layers, heads, hd in (("gpt2-xl", 48, 25, 64), ("llama-3-8b", 32, 8, 128)):
        buf = torch.empty(layers, 2, S, heads, max_seq, hd, dtype=torch.bfloat16, device="cuda")
        buf.view(torch.int16).random_()
        for L in (128, 1024):
            for F in (1, 3, 7):
                n = L - 1
                fams = [list(range(a, a + 1 + F)) for a in range(0, S - F, 1 + F)]
                iters = max(len(fams), (96 if L == 128 else 16) // len(fams) * len(fams))
                idx = [torch.tensor([f[0]] * F + f[1:] + [n] * F, dtype=torch.int32, device="cuda") for f in fams]

                def hip(k):
                    f = fams[k % len(fams)]
                    return lambda: be.kv_fork(buf, [f[0]] * F, f[1:], [n] * F, idx[k % len(fams)])

                def twin(k):
                    f = fams[k % len(fams)]
                    return lambda: ref.kv_fork(buf, [f[0]] * F, f[1:], [n] * F)

                moved = 2 * F * layers * 2 * heads * n * hd * 2
                for name, mk in (("kv_fork", hip), ("torch", twin)):
                    us, lo, hi = timed([mk(k) for k in range(iters)])
                    print(json.dumps({"build": label, "case": "kernel", "model": model, "L": L, "forks": F,
                                      "copy": name, "us": round(us, 2), "min": round(lo, 2), "max": round(hi, 2),
                                      "bytes": moved, "TB/s": round(moved / us / 1e6, 3)}), flush=True)
        del buf
        torch.cuda.empty_cache()


def end_to_end(label: str) -> None:
    from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
    from llm_sharding_demo_amd.runtime.engine import Engine

    P_, N, PL, GEN = 128, 4, 128, 128
    cfg = EngineConfig(model_id="gpt2-xl", num_stages=1, max_batch=P_ * N, max_seq_len=PL + GEN, device="cuda",
                       num_microbatches=2, seed=0)
    eng = Engine(cfg)
    rnd = random.Random(0)
    V = cfg.model.vocab_size
    prompts = [[rnd.randrange(V) for _ in range(PL)] for _ in range(P_)]
    kw = dict(temperature=0.6, top_k=40, max_new_tokens=GEN)

    def forked():
        return eng.generate_samples(prompts, [SamplingParams(seed=1000 * i, n=N, **kw) for i in range(P_)],
                                    record_timing=True)

    def separate():
        out = eng.generate_ids([p for p in prompts for _ in range(N)],
                               [SamplingParams(seed=1000 * i + k, **kw) for i in range(P_) for k in range(N)],
                               record_timing=True)
        return [out[N * i: N * i + N] for i in range(P_)]

    runs = {"n=4": forked, "512 requests": separate}
    for fn in runs.values():
        fn()
    res = {k: [] for k in runs}
    for _ in range(3):
        for name, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            res[name].append((1e3 * (time.perf_counter() - t0), eng.last_session.prefill_ms,
                              sum(eng.last_session.step_times_ms)))
            assert len(out) == P_ and all(len(o) == N and all(len(t) == GEN for t in o) for o in out)
    for name, r in res.items():
        print(json.dumps({"build": label, "case": "end-to-end", "model": "gpt2-xl", "prompts": P_, "n": N,
                          "prompt_tokens": PL, "new_tokens": GEN, "submitted_as": name,
                          "session_ms": [round(x[0], 1) for x in r], "prefill_ms": [round(x[1], 2) for x in r],
                          "decode_steps_ms": [round(x[2], 1) for x in r],
                          "kv_fork_launches": eng.workers[0].kv_fork_launches}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if not a.skip_kernel:
        kernel_cases(a.label)
    if not a.skip_e2e:
        end_to_end(a.label)


if __name__ == "__main__":
    main()
