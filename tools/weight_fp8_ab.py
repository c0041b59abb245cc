#!/usr/bin/env python3
"""bf16-weight vs FP8-weight GEMV (csrc/kernels/gemv.hip) over the per-layer
shapes of GPT-2 XL and Llama-3 8B at M = 1, 2, 4, 8 rows.

    python tools/weight_fp8_ab.py [--label NAME] [--hot]

Each launch reads another copy of the weight (enough copies to pass 1 GiB, so
no copy is still cached when its turn comes again; --hot: one copy, the
cache-resident figure).  The QKV shapes run the plain bf16 epilogue (no cache
to append to); the others run the epilogue the model uses.  One JSON line per
case: median of 5 rounds of graph-replayed launches, weight bytes per us, and
the FP8 speed-up against the byte ratio of 2.

    python tools/weight_fp8_ab.py --gemm [--label NAME]

The decode GEMMs of the same shapes at M = 16 .. 512 rows through the backend
(ops/hip.py), three routes alternating within each of 5 rounds: (a) the bf16
weight on the kernel ops/routing.py picks for it, (b) the FP8 weight on the
dequant route (dequant_rows_fp8 into the scratch + that kernel; w8_max_m = 0),
(c) the FP8 weight on the FP8-weight kernels (csrc/kernels/gemm_w8.hip: split-K
up to Routing.w8_sk_max_m rows, the all-rows kernel above; "w8_kernel" names
the instance that ran).  --rows M,M,... picks the row counts.  One
JSON line per case: medians in us, (b)'s spread (max - min of its rounds), the
weight TB/s of (a) and (c), and whether (c) beats (b) by more than that spread
-- what sets Routing.w8_max_m.

    python tools/weight_fp8_ab.py --dtype mxfp4 [--label NAME]

The same eight shapes at M = 1, 2, 4, 8 on MXFP4 weights (wquant.hip
quantize_rows_mxfp4), five routes alternating within each of 5 rounds, a fresh
weight copy per launch: the bf16 GEMV, the FP8 GEMV, the MXFP4 GEMV at its own
rows per wave ("mx4") and at the bf16 kernel's ("mx4_narrow",
gemv_set_mx4_wide(0)), and the MXFP4 weight on the dequant route through the
backend (gemv_max_m = 0: dequant_rows_mxfp4 into the scratch + the bf16 GEMM).
One JSON line per case: medians in us, weight TB/s of the three GEMVs (scale
bytes included), MXFP4 against FP8 (byte ratio 32 / 17 with the scale bytes),
the dequant route's spread, and whether the GEMV loses to it by more than that
spread."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sampler_topp_ab import timeit  # noqa: E402

# (model, projection, N, K, epilogue: 0 bf16, 1 gelu, 2 silu_mul, 4 residual)
SHAPES = [("gpt2-xl", "c_attn", 4800, 1600, 0), ("gpt2-xl", "attn.c_proj", 1600, 1600, 4),
          ("gpt2-xl", "c_fc", 6400, 1600, 1), ("gpt2-xl", "mlp.c_proj", 1600, 6400, 4),
          ("llama-3-8b", "qkv", 6144, 4096, 0), ("llama-3-8b", "o_proj", 4096, 4096, 4),
          ("llama-3-8b", "gate_up", 28672, 4096, 2), ("llama-3-8b", "down_proj", 4096, 14336, 4)]


def gemm_rows(a):
    from llm_sharding_demo_amd.ops import Residual
    from llm_sharding_demo_amd.ops.hip import HipBackend
    from llm_sharding_demo_amd.ops.routing import Routing

    dev = "cuda"
    bes = {}
    for route, m in (("dequant", 0), ("w8", 1 << 30)):
        be = bes[route] = HipBackend()
        be.R = Routing.from_env("").replace(w8_max_m=m)
        be._counters = torch.zeros(8, 1 << 16, dtype=torch.int32, device=dev)
    C = bes["w8"].C
    for model, name, N, K, epi in SHAPES:
        g = torch.Generator(device=dev).manual_seed(1)
        copies = max(2, -(-(1 << 30) // (N * K)))
        w16 = [(torch.randn(N, K, device=dev, generator=g) * 0.03).bfloat16() for _ in range(copies)]
        w8 = []
        for w in w16:
            q, sc = C.quantize_rows_fp8(w)
            q._lsd_scale = sc
            w8.append(q)
        for be in bes.values():
            be._wscratch = torch.empty(1, N * K, dtype=torch.bfloat16, device=dev)
        bias = None if epi == 2 else torch.zeros(N, dtype=torch.bfloat16, device=dev)
        for M in a.rows:
            x = torch.randn(M, K, device=dev, generator=g).bfloat16()
            r = Residual(torch.zeros(M, N, device=dev))
            turn = [0]

            def run(be, ws):
                turn[0] += 1
                w = ws[turn[0] % len(ws)]
                if epi == 4:
                    be.linear_residual(x, w, bias, r)
                    r.pending.clear()  # the fold into the next norm is the same on every route
                else:
                    be.linear(x, w, bias, {0: "none", 1: "gelu", 2: "silu_mul"}[epi])

            routes = {"bf16": (bes["dequant"], w16), "dequant": (bes["dequant"], w8), "w8": (bes["w8"], w8)}
            t = {k: [] for k in routes}
            for _ in range(5):
                for k, (be, ws) in routes.items():
                    t[k].append(timeit(lambda: run(be, ws), iters=max(copies, 32)))
            med = {k: statistics.median(v) for k, v in t.items()}
            run(*routes["w8"])
            tag = C.gemm_last_launch()
            spread = max(t["dequant"]) - min(t["dequant"])
            print(json.dumps({"label": a.label, "model": model, "proj": name, "N": N, "K": K, "M": M,
                              "bf16_us": round(med["bf16"], 2), "dequant_us": round(med["dequant"], 2),
                              "w8_us": round(med["w8"], 2), "w8_kernel": tag, "dequant_spread_us": round(spread, 2),
                              "bf16_TBps": round(2 * N * K / med["bf16"] / 1e6, 3),
                              "w8_TBps": round(N * K / med["w8"] / 1e6, 3),
                              "w8_vs_dequant": round(med["dequant"] / med["w8"], 3),
                              "w8_vs_bf16": round(med["bf16"] / med["w8"], 3),
                              "w8_wins": bool(med["dequant"] - med["w8"] > spread)}), flush=True)
        del w16, w8
        torch.cuda.empty_cache()


def gemv_mx4(a):
    from llm_sharding_demo_amd.ops import Residual
    from llm_sharding_demo_amd.ops.hip import HipBackend
    from llm_sharding_demo_amd.ops.routing import Routing

    dev = "cuda"
    be = HipBackend()
    be.R = Routing.from_env("").replace(gemv_max_m=0)
    be._counters = torch.zeros(8, 1 << 16, dtype=torch.int32, device=dev)
    C = be.C
    for model, name, N, K, epi in SHAPES:
        g = torch.Generator(device=dev).manual_seed(1)
        copies = max(2, -(-(1 << 30) // (N * K)))
        w16 = [(torch.randn(N, K, device=dev, generator=g) * 0.03).bfloat16() for _ in range(copies)]
        w8 = [C.quantize_rows_fp8(w) for w in w16]
        w4 = [C.quantize_rows_mxfp4(w) for w in w16]
        for q, e in w4:
            q._lsd_scale = e
        be._wscratch = torch.empty(1, N * K, dtype=torch.bfloat16, device=dev)
        bias = None if epi == 2 else torch.zeros(N, dtype=torch.bfloat16, device=dev)
        for M in (1, 2, 4, 8):
            if not all(C.gemv_ok(M, K, epi, 0, k) for k in (0, 1, 2)):
                continue
            x = torch.randn(M, K, device=dev, generator=g).bfloat16()
            res = torch.zeros(M, N, device=dev) if epi == 4 else None
            r = Residual(torch.zeros(M, N, device=dev))
            turn = [0]

            def gemv(ws):
                turn[0] += 1
                w = ws[turn[0] % copies]
                w, kw = (w[0], {"wscale": w[1]}) if isinstance(w, tuple) else (w, {})
                C.gemv(x, w, bias, epi, 0, None, None, 0.0, res, None, None, None, None, 0, 0, 0, None, **kw)

            def dequant():
                turn[0] += 1
                w = w4[turn[0] % copies][0]
                if epi == 4:
                    be.linear_residual(x, w, bias, r)
                    r.pending.clear()
                else:
                    be.linear(x, w, bias, {0: "none", 1: "gelu", 2: "silu_mul"}[epi])

            routes = {"bf16": (1, lambda: gemv(w16)), "fp8": (1, lambda: gemv(w8)), "mx4": (1, lambda: gemv(w4)),
                      "mx4_narrow": (0, lambda: gemv(w4)), "mx4_dequant": (1, dequant)}
            t = {k: [] for k in routes}
            for _ in range(5):
                for k, (wide, fn) in routes.items():
                    C.gemv_set_mx4_wide(wide)
                    t[k].append(timeit(fn, iters=max(copies, 64)))
            C.gemv_set_mx4_wide(1)
            med = {k: statistics.median(v) for k, v in t.items()}
            spread = max(t["mx4_dequant"]) - min(t["mx4_dequant"])
            print(json.dumps({"label": a.label, "model": model, "proj": name, "N": N, "K": K, "M": M,
                              **{k + "_us": round(v, 2) for k, v in med.items()},
                              "bf16_TBps": round(2 * N * K / med["bf16"] / 1e6, 3),
                              "fp8_TBps": round((N * K + 4 * N) / med["fp8"] / 1e6, 3),
                              "mx4_TBps": round(N * K * 17 / 32 / med["mx4"] / 1e6, 3),
                              "mx4_vs_fp8": round(med["fp8"] / med["mx4"], 3),
                              "mx4_vs_bf16": round(med["bf16"] / med["mx4"], 3),
                              "wide_vs_narrow": round(med["mx4_narrow"] / med["mx4"], 3),
                              "dequant_spread_us": round(spread, 2),
                              "gemv_loses_to_dequant": bool(med["mx4"] - med["mx4_dequant"] > spread)}), flush=True)
        del w16, w8, w4
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this")
    ap.add_argument("--hot", action="store_true")
    ap.add_argument("--gemm", action="store_true")
    ap.add_argument("--dtype", choices=("fp8_e4m3", "mxfp4"), default="fp8_e4m3")
    ap.add_argument("--rows", type=lambda v: [int(m) for m in v.split(",")], default=[16, 32, 64, 128, 192, 256, 384, 512])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if a.gemm:
        return gemm_rows(a)
    if a.dtype == "mxfp4":
        return gemv_mx4(a)
    from llm_sharding_demo_amd.ops.hip import _load

    C = _load()
    dev = "cuda"
    for model, name, N, K, epi in SHAPES:
        g = torch.Generator(device=dev).manual_seed(1)
        copies = 1 if a.hot else max(2, -(-(1 << 30) // (N * K)))
        w16 = [(torch.randn(N, K, device=dev, generator=g) * 0.03).bfloat16() for _ in range(copies)]
        w8 = [C.quantize_rows_fp8(w) for w in w16]
        bias = None if epi == 2 else torch.zeros(N, dtype=torch.bfloat16, device=dev)
        for M in (1, 2, 4, 8):
            if not (C.gemv_ok(M, K, epi, 0) and C.gemv_ok(M, K, epi, 0, True)):
                continue
            x = torch.randn(M, K, device=dev, generator=g).bfloat16()
            res = torch.zeros(M, N, device=dev) if epi == 4 else None
            turn = [0, 0]

            def run16():
                turn[0] += 1
                C.gemv(x, w16[turn[0] % len(w16)], bias, epi, 0, None, None, 0.0, res, None, None, None, None,
                       0, 0, 0, None)

            def run8():
                turn[1] += 1
                q, s = w8[turn[1] % len(w8)]
                C.gemv(x, q, bias, epi, 0, None, None, 0.0, res, None, None, None, None, 0, 0, 0, None, wscale=s)

            iters = max(len(w16), 64)
            t16 = statistics.median(timeit(run16, iters=iters) for _ in range(5))
            t8 = statistics.median(timeit(run8, iters=iters) for _ in range(5))
            print(json.dumps({"label": a.label, "model": model, "proj": name, "N": N, "K": K, "M": M,
                              "hot": a.hot, "bf16_us": round(t16, 2), "fp8_us": round(t8, 2),
                              "bf16_bytes_per_us": round(2 * N * K / t16), "fp8_bytes_per_us": round(N * K / t8),
                              "speedup": round(t16 / t8, 3)}), flush=True)
        del w16, w8
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
