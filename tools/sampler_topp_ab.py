#!/usr/bin/env python3
"""Sampler kernel time with the per-row top-p / min-p vectors (sample.hip):
256 rows x GPT-2 vocabulary and 256 x Llama-3 vocabulary, top-k 40, lm_head's
segment maxima on.  hipGraph-replayed, warm logits (tools/microbench.py timeit).

    python tools/sampler_topp_ab.py [--ext PATH/_C.so] [--label NAME] [--cases null,default]

--ext times another build's extension (one without the two arguments runs the
"null" case only), so two builds can be alternated process by process:
  null     no top_p / min_p tensors (the call every build has)
  default  vectors of 1.0 / 0.0 -- what the engine's decode graphs pass
  p0.9     top_p = 0.9 on every row
  p0.9m    top_p = 0.9 and min_p = 0.05 on every row
One JSON line per case: median of 7 rounds of 200 graph-replayed launches."""
from __future__ import annotations

import argparse
import importlib.machinery
import importlib.util
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load(path):
    if path is None:
        from llm_sharding_demo_amd.ops.hip import _load

        return _load()
    loader = importlib.machinery.ExtensionFileLoader("_C", path)
    spec = importlib.util.spec_from_loader("_C", loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    return mod


def timeit(fn, iters=200, warm=3):
    """Device time per call in us: `iters` calls captured into one hipGraph."""
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        for _ in range(warm):
            fn()
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    s.record()
    g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ext")
    ap.add_argument("--label", default="this")
    ap.add_argument("--cases", help="comma-separated subset (a process that times one case "
                                    "compares like with like against a build that has only that one)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    C = load(a.ext)
    has = "top_p" in (C.sample.__doc__ or "")
    dev, B = "cuda", 256
    for vocab, V, Vp in (("gpt2", 50257, 50304), ("llama3", 128256, 128256)):
        g = torch.Generator(device=dev).manual_seed(1)
        lg = torch.randn(B, Vp, device=dev, generator=g) * 3
        seg = lg.view(B, Vp // 8, 8).amax(-1).contiguous()
        t = torch.full((B,), 0.6, device=dev)
        k = torch.full((B,), 40, dtype=torch.int32, device=dev)
        gr = torch.zeros(B, dtype=torch.int32, device=dev)
        sd = torch.arange(B, dtype=torch.int64, device=dev)
        st = torch.zeros(B, dtype=torch.int64, device=dev)
        f = lambda v: torch.full((B,), v, device=dev)  # noqa: E731
        cases = [("null", lambda: C.sample(lg, V, t, k, gr, sd, st, seg))]
        if has:
            one, zero, p9, m05 = f(1.0), f(0.0), f(0.9), f(0.05)
            cases += [("default", lambda: C.sample(lg, V, t, k, gr, sd, st, seg, one, zero)),
                      ("p0.9", lambda: C.sample(lg, V, t, k, gr, sd, st, seg, p9, zero)),
                      ("p0.9m", lambda: C.sample(lg, V, t, k, gr, sd, st, seg, p9, m05))]
            assert torch.equal(cases[0][1](), cases[1][1]())  # default vectors: the uncut draws
        if a.cases:
            cases = [c for c in cases if c[0] in a.cases.split(",")]
        res = {n: [] for n, _ in cases}
        for _ in range(7):
            for n, fn in cases:
                res[n].append(timeit(fn))
        for n, _ in cases:
            print(json.dumps({"build": a.label, "vocab": vocab, "rows": B, "case": n,
                              "us": round(statistics.median(res[n]), 2),
                              "min": round(min(res[n]), 2), "max": round(max(res[n]), 2)}), flush=True)


if __name__ == "__main__":
    main()
