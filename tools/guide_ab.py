#!/usr/bin/env python3
"""Cost of the guided-decoding passes (guide.hip) beside the sampler, and beside
allow_mask_kernel at the same drawable sets: 256 rows x GPT-2 vocabulary and
256 x Llama-3 vocabulary, every row guided and in a state of its own that
leaves 1, about 1000 or about V / 2 tokens drawable, or every row on a slot
that follows no guide.  hipGraph-replayed, warm logits (as
tools/allowed_tokens_ab.py: the rows were just written by lm_head in a decode
step too).  Both masks are idempotent -- a masked logit stays -inf -- and every
state of the guides here leads to itself, so a replayed launch does the same
loads and stores every time.

    python tools/guide_ab.py [--label NAME]

One guide per case, S = 256 states (row r is in state r):
  1         257 classes: 256 single tokens and the rest; state s allows class s
  1000, V/2 1024 classes, every token in a random one; state s allows as many
            random classes as hold about that many tokens
Per vocabulary:
  sample      the unmodified sampler alone (top-k 40, segment maxima), on
              unmasked logits, for scale
  guide-n     guide_mask_kernel alone, segment maxima repaired
  allow-n     allow_mask_kernel alone on the same rows' drawable sets as
              bitmasks: the yardstick.  guide_mask reads 2 bytes of classes per
              column where allow_mask reads one bit, and looks every class up
              in LDS
  advance     guide_advance_kernel alone, every row stepping on a drawable token
  guide-off   guide_mask_kernel with every slot on no guide (the early return)
  advance-off guide_advance_kernel likewise
One JSON line per case: median of 7 rounds of 200 graph-replayed launches, and
the mean number of drawable tokens per row.  Run it in several processes and
compare the lines."""
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


def make_guide(V: int, n: int, S: int, rng) -> tuple:
    """(cls int16 [V], next int16 [S, C], drawable bool [S, V]) of the case
    that leaves about n tokens drawable in each of S states."""
    if n == 1:
        C = S + 1
        cls = np.full(V, S, dtype=np.int16)
        cls[rng.choice(V, size=S, replace=False)] = np.arange(S, dtype=np.int16)
        allowed = np.zeros((S, C), dtype=bool)
        allowed[np.arange(S), np.arange(S)] = True
    else:
        C = 1024
        cls = rng.integers(0, C, size=V).astype(np.int16)
        k = max(1, round(n * C / V))
        allowed = np.zeros((S, C), dtype=bool)
        for s in range(S):
            allowed[s, rng.choice(C, size=k, replace=False)] = True
    nxt = np.where(allowed, np.arange(S, dtype=np.int16)[:, None], np.int16(-1)).astype(np.int16)
    return cls, nxt, allowed[:, cls]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from llm_sharding_demo_amd.ops.hip import _load

    C = _load()
    dev, B, G, CELLS = "cuda", 256, 8, 1 << 18
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
        drawn = {}

        def guided(n, on=True, row=3):
            """The table of the case in guide row `row` (slot r in state r, or
            on no guide), its rows' drawable sets as allow_mask's table, and a
            drawable token per row."""
            cls, nxt, ok = make_guide(V, n, B, rng)
            drawn[n] = float(ok.sum(axis=1).mean())
            gcls = torch.zeros(G, Vp, dtype=torch.int16)
            gcls[row, :V] = torch.from_numpy(cls)
            gnext = torch.zeros(G, CELLS, dtype=torch.int16)
            gnext[row, : nxt.size] = torch.from_numpy(nxt.reshape(-1))
            gdim = torch.zeros(G, 2, dtype=torch.int32)
            gdim[row] = torch.tensor(nxt.shape, dtype=torch.int32)
            gsl = torch.stack([torch.full((B,), row if on else -1), torch.arange(B)], dim=1).to(torch.int32)
            words = np.ascontiguousarray(np.packbits(np.pad(ok, ((0, 0), (0, W * 32 - V))), axis=1,
                                                     bitorder="little")).view(np.int32)
            toks = torch.from_numpy(ok.argmax(axis=1).astype(np.int32))
            return (tuple(x.to(dev) for x in (gcls, gnext, gdim, gsl)),
                    (torch.ones(B, dtype=torch.int32, device=dev), torch.from_numpy(words.copy()).to(dev)), toks.to(dev))

        def mask(tab):
            lg, seg = plain.clone(), pseg.clone()
            return lambda: C.guide_mask(lg, V, *tab, slots, seg)

        def allow(atab):
            lg, seg = plain.clone(), pseg.clone()
            return lambda: C.allow_mask(lg, V, *atab, slots, seg)

        cases = [("sample", lambda: C.sample(plain, V, t, k, gr, sd, st, pseg))]
        for n in (1, 1000, V // 2):
            tab, atab, toks = guided(n)
            cases += [(f"guide-{n}", mask(tab)), (f"allow-{n}", allow(atab))]
        cases.append(("advance", lambda tab=tab, toks=toks: C.guide_advance(*tab, V, slots, toks, None)))
        off, _, toks0 = guided(1, on=False)
        cases += [("guide-off", mask(off)), ("advance-off", lambda: C.guide_advance(*off, V, slots, toks0, None))]
        res = {c: [] for c, _ in cases}
        for _ in range(7):
            for c, fn in cases:
                res[c].append(timeit(fn))
        for c, _ in cases:
            us = statistics.median(res[c])
            n = c.split("-")[1] if c[:5] in ("guide", "allow") and c[-3:] != "off" else None
            print(json.dumps({"build": a.label, "vocab": vocab, "rows": B, "case": c, "us": round(us, 2),
                              "min": round(min(res[c]), 2), "max": round(max(res[c]), 2),
                              **({"drawable": round(drawn[int(n)], 1)} if n else {})}), flush=True)


if __name__ == "__main__":
    main()
