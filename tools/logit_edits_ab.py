#!/usr/bin/env python3
"""Cost of the logit-edit pass (logit_edit.hip) beside the sampler: 256 rows x
GPT-2 vocabulary and 256 x Llama-3 vocabulary, every row with 1, 32 or 300
entries (distinct random tokens, sorted, all active, finite values -- so a
replayed launch does the same work every time), a table of 300 entries per
slot.  hipGraph-replayed, warm logits (as tools/penalty_ab.py: the rows were
just written by lm_head in a decode step too).

    python tools/logit_edits_ab.py [--label NAME]

Per vocabulary:
  sample      the unmodified sampler alone (top-k 40, segment maxima), for scale
  edit-n      logit_edit_kernel alone with n entries on every row, segment
              maxima repaired
  off         logit_edit_kernel with count 0 on every row (the early return)
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
    dev, B, E = "cuda", 256, 300
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
        step = torch.full((B,), 17, dtype=torch.int64, device=dev)
        tok = torch.stack([torch.randperm(V, device=dev, generator=g)[:E].sort().values for _ in range(B + 1)])
        tok = tok.to(torch.int32).contiguous()
        val = (torch.rand(B + 1, E, device=dev, generator=g) - 0.5) * 1e-3  # small: the rows stay what they are
        until = torch.full((B + 1, E), 2 ** 31 - 1, dtype=torch.int32, device=dev)

        def edit(n):
            cnt = torch.full((B + 1,), n, dtype=torch.int32, device=dev)
            return lambda: C.logit_edits(lg, V, cnt, tok, val, until, slots, step, seg)

        cases = [("sample", lambda: C.sample(lg, V, t, k, gr, sd, st, seg)), ("edit-1", edit(1)),
                 ("edit-32", edit(32)), ("edit-300", edit(300)), ("off", edit(0))]
        res = {c: [] for c, _ in cases}
        for _ in range(7):
            for c, fn in cases:
                res[c].append(timeit(fn))
        for c, _ in cases:
            us = statistics.median(res[c])
            print(json.dumps({"build": a.label, "vocab": vocab, "rows": B, "case": c, "us": round(us, 2),
                              "min": round(min(res[c]), 2), "max": round(max(res[c]), 2)}), flush=True)


if __name__ == "__main__":
    main()
