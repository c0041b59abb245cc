#!/usr/bin/env python3
"""Host cost of the per-row sampler fields' paths at a 4096-sequence join
burst (CPU only): what runs once per composition change between the
scheduler's decision and the packed buffer of apply_rows.

    python tools/row_fields_ab.py [--label NAME] [--root CHECKOUT] [--rounds N]

--root: time the package of another checkout (the parent commit's) with the
same script.  A checkout from before runtime/plan.py ROW_FIELDS has no pure
packer and no single feature pass: there the script times the code that
checkout runs in their place (its StageWorker._rows_pack fill and its three
_rows_* predicates, copied below as `_legacy_*`).

For 4096 rows and 4096 single-chunk joins, default traffic ("default") and
every 4th request with a cut, a penalty and logprobs ("mixed"):
  group     Scheduler._group: the Chunk and Row lists of one GroupPlan
  wire      PlanEncoder.encode + PlanDecoder.decode of that plan
  pack      the native packer into a preallocated int32 array (last stage of one)
  features  the (cut, pen, lp) pass over the rows
One JSON line per (traffic, path): median / min / max ms over the rounds.  Run
both checkouts alternately, several times each, and compare the lines."""
from __future__ import annotations

import argparse
import gc
import json
import os
import statistics
import sys
import time
import types

import numpy as np

N, CAP = 4096, 4096


def _legacy_features(rows):
    return (any(r.top_p < 1.0 or r.min_p > 0.0 for r in rows),
            any(r.presence != 0.0 or r.frequency != 0.0 for r in rows),
            any(r.logprobs >= 0 for r in rows))


def _legacy_pack(rows, cap, first, last, feats, a):
    _, pen, lp = _legacy_features(rows)  # the old packer asked again
    n = len(rows)
    a[4 * cap] = n
    f0 = 4 * cap + 1
    a[f0: f0 + n] = [r.slot for r in rows]
    a[f0 + cap: f0 + cap + n] = [r.pos for r in rows]
    if last:
        a[f0 + 2 * cap: f0 + 2 * cap + n] = np.asarray([r.temperature for r in rows], np.float32).view(np.int32)
        a[f0 + 3 * cap: f0 + 3 * cap + n] = [r.top_k for r in rows]
        a[f0 + 4 * cap: f0 + 4 * cap + n] = [1 if r.greedy else 0 for r in rows]
        a[f0 + 6 * cap: f0 + 6 * cap + n] = np.asarray([r.top_p for r in rows], np.float32).view(np.int32)
        a[f0 + 7 * cap: f0 + 7 * cap + n] = np.asarray([r.min_p for r in rows], np.float32).view(np.int32)
        if pen or lp:
            a[f0 + 8 * cap: f0 + 8 * cap + n] = np.asarray([r.presence for r in rows], np.float32).view(np.int32)
            a[f0 + 9 * cap: f0 + 9 * cap + n] = np.asarray([r.frequency for r in rows], np.float32).view(np.int32)
        if lp:
            a[f0 + 10 * cap: f0 + 10 * cap + n] = [r.logprobs for r in rows]
        a64 = a[: 4 * cap].view(np.int64)
        a64[:n] = [r.seed for r in rows]
        a64[cap: cap + n] = [r.step for r in rows]
    if first:
        a[f0 + 5 * cap: f0 + 5 * cap + n] = [r.src for r in rows]


def _ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--rounds", type=int, default=15)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from llm_sharding_demo_amd.config import SamplingParams
    from llm_sharding_demo_amd.runtime import plan as P
    from llm_sharding_demo_amd.runtime.scheduler import Scheduler, _Meta

    table = hasattr(P, "ROW_FIELDS")
    pack = P.pack_rows if table else _legacy_pack
    features = P.row_features if table else _legacy_features
    for traffic in ("default", "mixed"):
        meta = {}
        for i in range(N):
            p = SamplingParams(temperature=0.7, top_k=40, seed=(1 << 61) + i, max_new_tokens=8)
            if traffic == "mixed" and i % 4 == 0:
                p = SamplingParams(temperature=0.7, top_k=40, seed=(1 << 61) + i, max_new_tokens=8, top_p=0.9,
                                   presence_penalty=0.5, logprobs=2)
            req = types.SimpleNamespace(prompt_ids=list(range(1, 65)), params=p)
            if table:
                meta[i] = _Meta(req, p.seed, P.sampler_values(p, p.seed), -1 if p.logprobs is None else p.logprobs)
            else:
                meta[i] = _Meta(req, p.seed, (p.temperature, p.top_k, p.greedy, p.seed),
                                (p.top_p, p.min_p, float(p.presence_penalty), float(p.frequency_penalty),
                                 -1 if p.logprobs is None else int(p.logprobs)))
        sched = types.SimpleNamespace(meta=meta)
        go = (0, N, N, N, 256, True, [(i, i, 0, 64, True) for i in range(N)],
              [(i, i, 64, 1, i) for i in range(N)])
        gp = Scheduler._group(sched, go)
        plan = P.StepPlan(step=3, groups=[gp])
        enc, dec = P.PlanEncoder(), P.PlanDecoder()
        buf = np.zeros(15 * CAP + 1, np.int32)
        feats = features(gp.rows)

        def wire():
            rec, payload = enc.encode(plan)
            return dec.decode(rec, lambda n: payload[:n])

        assert wire() == plan
        paths = (("group", lambda: Scheduler._group(sched, go)), ("wire", wire),
                 ("pack", lambda: pack(gp.rows, CAP, True, True, feats, buf)),
                 ("features", lambda: features(gp.rows)))
        gc.collect()
        gc.freeze()  # as the engine does after start-up (freeze_gc): the fixtures are not walked again
        for name, fn in paths:
            fn()
            gc.collect()
            t = _ms(fn, a.rounds)
            print(json.dumps({"build": a.label, "traffic": traffic, "path": name, "ms": round(statistics.median(t), 3),
                              "min": round(min(t), 3), "max": round(max(t), 3)}), flush=True)


if __name__ == "__main__":
    main()
