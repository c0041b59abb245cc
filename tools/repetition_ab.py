#!/usr/bin/env python3
"""Cost of the repetition pass (repeat.hip) plus record_context beside the
sampler: 256 rows x GPT-2 vocabulary and 256 x Llama-3 vocabulary, every row
with 16, 128 or 1024 context tokens (random ids, so mostly distinct) and
repetition_penalty alone, no_repeat_ngram_size = 3 alone, or both; a context
table of 1024 tokens per slot.  hipGraph-replayed, warm logits (as
tools/penalty_ab.py: the rows were just written by lm_head in a decode step
too).  The penalty is 1.0001, so replayed launches keep rewriting finite
logits.

    python tools/repetition_ab.py [--label NAME]

Per vocabulary:
  sample        the unmodified sampler alone (top-k 40, segment maxima), for scale
  r-n / g3-n / both-n
                repeat_kernel + record_context_kernel with n context tokens on
                every row, segment maxima repaired
  off           both kernels with the knobs off on every row (the early return)
One JSON line per case: median of 7 rounds of 200 graph-replayed launches.
Run it in several processes and compare the lines."""
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
    dev, B, L, c = "cuda", 256, 1024, 8
    for vocab, V, Vp in (("gpt2", 50257, 50304), ("llama3", 128256, 128256)):
        g = torch.Generator(device=dev).manual_seed(1)
        lg = torch.randn(B, Vp, device=dev, generator=g) * 3
        seg = lg.view(B, Vp // 8, 8).amax(-1).contiguous()
        t = torch.full((B,), 0.6, device=dev)
        k = torch.full((B,), 40, dtype=torch.int32, device=dev)
        gr = torch.zeros(B, dtype=torch.int32, device=dev)
        sd = torch.arange(B, dtype=torch.int64, device=dev)
        st = torch.zeros(B, dtype=torch.int64, device=dev)
        slots = torch.arange(B, dtype=torch.int32, device=dev)
        step = torch.full((B,), c, dtype=torch.int64, device=dev)
        active = torch.ones(B, dtype=torch.int32, device=dev)
        drawn = torch.randint(0, V, (B,), device=dev, generator=g, dtype=torch.int32)
        tok = torch.randint(0, V, (B + 1, L), device=dev, generator=g, dtype=torch.int32)

        def rep(n, r, G):
            plen = torch.full((B + 1,), n - c, dtype=torch.int32, device=dev)
            rpen = torch.full((B + 1,), r, device=dev)
            ngram = torch.full((B + 1,), G, dtype=torch.int32, device=dev)

            def fn():
                C.repetition(lg, V, plen, rpen, ngram, tok, slots, step, seg)
                # the draw's own position: behind the context the pass read
                C.record_context(tok, plen, slots, step, drawn, active, 0)
            return fn

        cases = [("sample", lambda: C.sample(lg, V, t, k, gr, sd, st, seg))]
        for n in (16, 128, 1024):
            cases += [(f"r-{n}", rep(n, 1.0001, 0)), (f"g3-{n}", rep(n, 1.0, 3)), (f"both-{n}", rep(n, 1.0001, 3))]
        cases.append(("off", rep(128, 1.0, 0)))
        res = {name: [] for name, _ in cases}
        for _ in range(7):
            for name, fn in cases:
                res[name].append(timeit(fn))
        for name, _ in cases:
            us = statistics.median(res[name])
            print(json.dumps({"build": a.label, "vocab": vocab, "rows": B, "case": name, "us": round(us, 2),
                              "min": round(min(res[name]), 2), "max": round(max(res[name]), 2)}), flush=True)


if __name__ == "__main__":
    main()
