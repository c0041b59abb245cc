#!/usr/bin/env python3
"""Cost of the bad-words pass (bad_words.hip) beside the sampler: 256 rows x
GPT-2 vocabulary and 256 x Llama-3 vocabulary, every row asking with 1, 32 or
N = 256 sequences of 1, 2 or 8 tokens (a row's own slot; every second
sequence ends the row's context, so it matches and bans its last token, the
others are compared and dropped), or every row on a slot with cnt == 0.
hipGraph-replayed, warm logits (as tools/allowed_tokens_ab.py: the rows were
just written by lm_head in a decode step too).  The pass is idempotent -- a
banned logit stays -inf -- so a replayed launch does the same compares and
stores every time.

    python tools/bad_words_ab.py [--label NAME]

Per vocabulary:
  sample      the unmodified sampler alone (top-k 40, segment maxima), on
              unbanned logits, for scale
  bad-n-m     bad_words_kernel alone with n sequences of m tokens on every
              row, segment maxima repaired
  off         bad_words_kernel with cnt == 0 on every row (the early return)
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
    dev, B, N, L = "cuda", 256, 256, 1024
    for vocab, V, Vp in (("gpt2", 50257, 50304), ("llama3", 128256, 128256)):
        g = torch.Generator(device=dev).manual_seed(1)
        plain = torch.randn(B, Vp, device=dev, generator=g) * 3
        pseg = plain.view(B, Vp // 8, 8).amax(-1).contiguous()
        t = torch.full((B,), 0.6, device=dev)
        k = torch.full((B,), 40, dtype=torch.int32, device=dev)
        gr = torch.zeros(B, dtype=torch.int32, device=dev)
        sd = torch.arange(B, dtype=torch.int64, device=dev)
        st = torch.zeros(B, dtype=torch.int64, device=dev)
        slots = torch.arange(B, dtype=torch.int32, device=dev)
        rng = np.random.default_rng(1)
        # contexts: 200 prompt tokens and 56 draws on every slot
        ctok_h = rng.integers(0, V, size=(B, L), dtype=np.int32)
        plen = torch.full((B,), 200, dtype=torch.int32, device=dev)
        step = torch.full((B,), 56, dtype=torch.int64, device=dev)
        ctok = torch.from_numpy(ctok_h).to(dev)
        n_ctx = 256

        def bad(n, m, on=True):
            """A table with n sequences of m tokens per slot and logits of its own."""
            T = N * 8
            end = np.zeros((B, N), dtype=np.int32)
            tok = np.zeros((B, T), dtype=np.int32)
            for s in range(B):
                for e in range(n):
                    w = rng.integers(0, V, size=m, dtype=np.int32)
                    if e % 2 == 0 and m > 1:
                        w[: m - 1] = ctok_h[s, n_ctx - (m - 1): n_ctx]  # ends the context: a match
                    tok[s, e * m: (e + 1) * m] = w
                    end[s, e] = (e + 1) * m
            cnt = torch.full((B,), n if on else 0, dtype=torch.int32, device=dev)
            end_d, tok_d = torch.from_numpy(end).to(dev), torch.from_numpy(tok).to(dev)
            lg, seg = plain.clone(), pseg.clone()
            return lambda: C.bad_words(lg, V, cnt, end_d, tok_d, plen, ctok, slots, step, seg)

        cases = [("sample", lambda: C.sample(plain, V, t, k, gr, sd, st, pseg))]
        cases += [(f"bad-{n}-{m}", bad(n, m)) for n in (1, 32, N) for m in (1, 2, 8)]
        cases += [("off", bad(32, 2, on=False))]
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
