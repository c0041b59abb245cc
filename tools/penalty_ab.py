#!/usr/bin/env python3
"""Cost of the presence / frequency penalty pass (penalty.hip) beside the
sampler: 256 rows x GPT-2 vocabulary (history buffer of 1024 positions) and
256 x Llama-3 vocabulary (8192 positions), every row penalised, lm_head's
segment maxima on.  hipGraph-replayed, warm logits.

    python tools/penalty_ab.py [--label NAME]

Per vocabulary and history length (16, 128, 1024 generated tokens per row):
  sample    the unmodified sampler alone (top-k 40), for scale
  penalize  penalize_kernel alone
  record    record_tokens_kernel alone
  pen+rec   both, as a penalised decode step adds them around the sampler
One JSON line per case: median of 7 rounds of 200 graph-replayed launches."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from llm_sharding_demo_amd.ops.hip import _load

    C = _load()
    dev, B = "cuda", 256
    for vocab, V, Vp, L in (("gpt2", 50257, 50304, 1024), ("llama3", 128256, 128256, 8192)):
        g = torch.Generator(device=dev).manual_seed(1)
        lg = torch.randn(B, Vp, device=dev, generator=g) * 3
        seg = lg.view(B, Vp // 8, 8).amax(-1).contiguous()
        t = torch.full((B,), 0.6, device=dev)
        k = torch.full((B,), 40, dtype=torch.int32, device=dev)
        gr = torch.zeros(B, dtype=torch.int32, device=dev)
        sd = torch.arange(B, dtype=torch.int64, device=dev)
        st = torch.zeros(B, dtype=torch.int64, device=dev)
        hist = torch.randint(0, V, (B + 1, L), device=dev, generator=g, dtype=torch.int32)
        slots = torch.arange(B, dtype=torch.int32, device=dev)
        act = torch.ones(B, dtype=torch.int32, device=dev)
        tok = torch.zeros(B, dtype=torch.int32, device=dev)
        pres = torch.full((B,), 0.5, device=dev)
        freq = torch.full((B,), 0.25, device=dev)
        for n in (16, 128, 1024):
            cnt = torch.full((B,), n, dtype=torch.int64, device=dev)
            pen = lambda: C.penalize(lg, V, hist, slots, cnt, pres, freq, seg)  # noqa: E731
            rec = lambda: C.record_tokens(hist, slots, cnt, tok, act, 1)  # noqa: E731
            cases = [("sample", lambda: C.sample(lg, V, t, k, gr, sd, st, seg)), ("penalize", pen), ("record", rec),
                     ("pen+rec", lambda: (pen(), rec()))]
            res = {c: [] for c, _ in cases}
            for _ in range(7):
                for c, fn in cases:
                    res[c].append(timeit(fn))
            for c, _ in cases:
                print(json.dumps({"build": a.label, "vocab": vocab, "rows": B, "history": n, "case": c,
                                  "us": round(statistics.median(res[c]), 2),
                                  "min": round(min(res[c]), 2), "max": round(max(res[c]), 2)}), flush=True)


if __name__ == "__main__":
    main()
