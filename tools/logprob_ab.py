#!/usr/bin/env python3
"""Cost of the logprob pass (logprob.hip) beside the sampler: 256 rows x GPT-2
vocabulary and 256 x Llama-3 vocabulary, every row asking, records of 1024
positions, W = 20.  hipGraph-replayed, warm logits (as tools/penalty_ab.py:
the rows were just written by lm_head in a decode step too).

    python tools/logprob_ab.py [--label NAME]

Per vocabulary:
  sample      the unmodified sampler alone (top-k 40, segment maxima), for scale
  logprob-n   logprob_kernel alone with n = 0, 5, 20 alternatives on every row
  off         logprob_kernel with nlp = -1 on every row (the early return)
One JSON line per case: median of 7 rounds of 200 graph-replayed launches, the
bytes the rows hold (B x V x 4: what one read of every row moves) and the GB/s
that is per launch.  Run it in several processes and compare the lines."""
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
    dev, B, L, W = "cuda", 256, 1024, 20
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
        act = torch.ones(B, dtype=torch.int32, device=dev)
        tok = torch.randint(0, V, (B,), device=dev, generator=g, dtype=torch.int32)
        step = torch.full((B,), 17, dtype=torch.int64, device=dev)
        rec = (torch.empty(B + 1, L, device=dev), torch.empty(B + 1, L, W, dtype=torch.int32, device=dev),
               torch.empty(B + 1, L, W, device=dev))

        def lp(n):
            nlp = torch.full((B,), n, dtype=torch.int32, device=dev)
            return lambda: C.logprobs(lg, V, tok, nlp, slots, step, act, rec[0], rec[1], rec[2], 1)

        cases = [("sample", lambda: C.sample(lg, V, t, k, gr, sd, st, seg)), ("logprob-0", lp(0)),
                 ("logprob-5", lp(5)), ("logprob-20", lp(20)), ("off", lp(-1))]
        res = {c: [] for c, _ in cases}
        for _ in range(7):
            for c, fn in cases:
                res[c].append(timeit(fn))
        nbytes = B * V * 4
        for c, _ in cases:
            us = statistics.median(res[c])
            print(json.dumps({"build": a.label, "vocab": vocab, "rows": B, "case": c, "us": round(us, 2),
                              "min": round(min(res[c]), 2), "max": round(max(res[c]), 2),
                              "row_mbytes": round(nbytes / 1e6, 1),
                              "gb_per_s": None if c in ("sample", "off") else round(nbytes / us / 1e3, 1)}), flush=True)


if __name__ == "__main__":
    main()
