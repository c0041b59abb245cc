#!/usr/bin/env python3
"""Decode attention over a bf16 against an FP8 (E4M3) KV cache.

    python tools/kv_fp8_ab.py [--label NAME] [--pairs 3]

The decode attention kernel alone at the headline shapes: 256 rows of GPT-2 XL
heads (25 x 64, the VALU kernels) and of Llama-3 8B heads (32 / 8 x 128, the
MFMA kernels), contexts of 128-256 keys, one layer's cache per call and 48
layers' caches in rotation so no call finds its keys in a cache.  bf16 and FP8
alternate, `--pairs` times; per run the median device time of a call (events
around 20 calls, 15 repeats) and the KV bytes / us it streamed.  One JSON line
per run.  The bf16 arm is the kernel default traffic runs."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from llm_sharding_demo_amd.ops.hip import HipBackend, _load  # noqa: E402

SHAPES = {"gpt2-xl": (25, 25, 64), "llama-3-8b": (32, 8, 128)}
B, S, LAYERS, CALLS, REPEATS = 256, 256, 48, 20, 15


def run(C, name, fp8: bool):
    nh, n_kv, hd = SHAPES[name]
    g = torch.Generator(device="cuda").manual_seed(1)
    mk = lambda: torch.randn(LAYERS, B, n_kv, S, hd, generator=g, device="cuda").to(torch.bfloat16)  # noqa: E731
    kc, vc = mk(), mk()
    if fp8:
        kc, vc = kc.float().to(torch.float8_e4m3fn), vc.float().to(torch.float8_e4m3fn)
    q = torch.randn(B, nh * hd, generator=g, device="cuda").to(torch.bfloat16)
    slots = torch.randperm(B, generator=g, device="cuda").int()
    pos = torch.randint(127, S, (B,), generator=g, device="cuda").int()
    splits = HipBackend.decode_attn_splits(B, nh, n_kv, hd, S)
    kv_bytes = 2 * int((pos.long() + 1).sum()) * n_kv * hd * kc.element_size()
    times = []
    for rep in range(REPEATS + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(CALLS):
            C.attn_decode(q, kc[(rep * CALLS + i) % LAYERS], vc[(rep * CALLS + i) % LAYERS], slots, pos, nh, splits)
        b.record()
        torch.cuda.synchronize()
        if rep >= 2:  # two warm-up rounds
            times.append(a.elapsed_time(b) * 1e3 / CALLS)
    us = statistics.median(times)
    return {"shape": name, "kv": "fp8_e4m3" if fp8 else "bf16", "splits": splits, "us": round(us, 2),
            "us_min": round(min(times), 2), "us_max": round(max(times), 2), "kv_bytes": kv_bytes,
            "bytes_per_us": round(kv_bytes / us)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this")
    ap.add_argument("--pairs", type=int, default=3)
    a = ap.parse_args()
    C = _load()
    for name in SHAPES:
        for pair in range(a.pairs):
            for fp8 in (False, True):
                print(json.dumps({"build": a.label, "pair": pair, **run(C, name, fp8)}), flush=True)


if __name__ == "__main__":
    main()
