#!/usr/bin/env python3
"""Cost of the allowed-token mask pass (allow_mask.hip) beside the sampler: 256
rows x GPT-2 vocabulary and 256 x Llama-3 vocabulary, every row asking with 1,
1000 or V / 2 allowed tokens (distinct random tokens; a row's own slot), or
every row on a slot with on == 0.  hipGraph-replayed, warm logits (as
tools/logit_edits_ab.py: the rows were just written by lm_head in a decode
step too).  The pass is idempotent -- a masked logit stays -inf -- so a
replayed launch does the same stores every time: all-clear segments are
stored without being read, mixed ones are read, selected and stored.

    python tools/allowed_tokens_ab.py [--label NAME]

Per vocabulary:
  sample      the unmodified sampler alone (top-k 40, segment maxima), on
              unmasked logits, for scale
  allow-n     allow_mask_kernel alone with n allowed tokens on every row,
              segment maxima repaired
  off         allow_mask_kernel with on == 0 on every row (the early return)
One JSON line per case: median of 7 rounds of 200 graph-replayed launches.
Run it in several processes and compare the lines."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
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
    for vocab, V, Vp in (("gpt2", 50257, 50304), ("llama3", 128256, 128256)):
        g = torch.Generator(device=dev).manual_seed(1)
        W = (Vp + 31) // 32
        plain = torch.randn(B, Vp, device=dev, generator=g) * 3
        pseg = plain.view(B, Vp // 8, 8).amax(-1).contiguous()
        t = torch.full((B,), 0.6, device=dev)
        k = torch.full((B,), 40, dtype=torch.int32, device=dev)
        gr = torch.zeros(B, dtype=torch.int32, device=dev)
        sd = torch.arange(B, dtype=torch.int64, device=dev)
        st = torch.zeros(B, dtype=torch.int64, device=dev)
        slots = torch.arange(B, dtype=torch.int32, device=dev)
        rng = np.random.default_rng(1)

        def allow(n, on=1):
            """A table with n random allowed tokens per slot and logits of its own."""
            words = np.zeros((B, W), dtype=np.uint32)
            for s in range(B):
                ids = rng.choice(V, size=n, replace=False)
                np.bitwise_or.at(words[s], ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
            bits = torch.from_numpy(words.view(np.int32)).to(dev)
            flag = torch.full((B,), on, dtype=torch.int32, device=dev)
            lg, seg = plain.clone(), pseg.clone()
            return lambda: C.allow_mask(lg, V, flag, bits, slots, seg)

        cases = [("sample", lambda: C.sample(plain, V, t, k, gr, sd, st, pseg)), ("allow-1", allow(1)),
                 ("allow-1000", allow(1000)), (f"allow-{V // 2}", allow(V // 2)), ("off", allow(1, on=0))]
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
