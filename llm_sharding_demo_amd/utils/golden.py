"""Full-dimension numerics check of the HIP path against an fp32 golden.

The reference delegates all math to HF transformers on CPU in fp32
(`/root/reference/server.py:41,85,100-102`).  Here the golden is the same
model (same bf16-initialised weights, widened to fp32) run through the plain
PyTorch ops of ops/reference.py -- on the same GPU, so full GPT-2 XL and
Llama-3 8B dimensions are affordable -- and the HIP model (bf16 weights and
activations, fp32 accumulation, bf16 or FP8 KV cache) is compared logit by logit
over a prefill plus teacher-forced decode steps (both models are fed the
golden's greedy tokens, so one near-tie cannot derail the rest of the run).

Tolerance (bf16 inputs, fp32 accumulation): per row, max |logit error| <=
`tol` x the golden row's logit standard deviation, and greedy top-1
agreement on >= `min_agree` of the rows.
"""
from __future__ import annotations

from typing import Dict, List

import torch

from ..config import get_model_config
from ..models.stage import StageModel
from ..models.weights import init_stage_weights
from ..ops import ReferenceBackend
from ..runtime.batch import BatchMeta
from ..runtime.kv_cache import kv_dtype_of


def compare_with_golden(model_id, prompts: List[List[int]], steps: int = 8,
                        device: str = "cuda", seed: int = 0, inject=1.0, kv_dtype=None,
                        weight_dtype: str = "bf16"):
    """`inject` scales the HIP logits' deviation from the golden before it is
    measured (1.0: as computed); a tuple of factors returns one result per
    factor from the same forward passes.  The gate tests use 3.0 to show that
    a kernel regression of that size fails the bounds.

    `kv_dtype` (a torch dtype, e.g. torch.float8_e4m3fn; None: as ever) gives
    the HIP model that KV cache and adds a third model to the same loop: the
    fp32 golden's ops over a cache of that dtype -- the cost of the cache
    format alone.  All three are fed the fp32 golden's tokens, and the result
    is {"golden_kv": metrics of golden/kv_dtype vs golden/fp32,
        "hip_kv":    metrics of HIP/kv_dtype vs golden/fp32}.

    `weight_dtype="fp8_e4m3"` (or `"mxfp4"`) gives the HIP model FP8 (MXFP4)
    weights (EngineConfig's field).  Its reference is then the fp32 golden over the *dequantised*
    weights -- the same numbers the kernels multiply by -- and the result is
    {"hip_w":    metrics of HIP/FP8 weights vs golden over dequantised weights,
     "golden_w": metrics of that golden vs the golden over the bf16 weights:
                 the quantisation's own cost}."""
    if weight_dtype != "bf16":
        if kv_dtype is not None:
            raise ValueError("compare_with_golden: one of kv_dtype / weight_dtype at a time")
        return _compare_weight_dtype(model_id, prompts, steps, device, seed, inject, weight_dtype)
    if isinstance(kv_dtype, str):  # an EngineConfig.kv_dtype name; "bf16" is the default cache
        kv_dtype = kv_dtype_of(kv_dtype)[0]
    mc = get_model_config(model_id) if isinstance(model_id, str) else model_id
    dev = torch.device(device)
    L = mc.n_layers
    max_seq = max(len(p) for p in prompts) + steps + 1
    B = len(prompts)
    w = init_stage_weights(mc, range(L), True, True, seed, dev, torch.bfloat16)
    wf = {k: v.float() for k, v in w.items()}
    gold = StageModel(mc, 0, L, True, True, device=dev, dtype=torch.float32, weights=wf,
                      max_slots=B, max_seq=max_seq, backend=ReferenceBackend())
    hip = StageModel(mc, 0, L, True, True, device=dev, dtype=torch.bfloat16, weights=w,
                     max_slots=B, max_seq=max_seq, kv_dtype=kv_dtype)
    # the models measured against the golden, in the order of the results
    cands = [hip]
    if kv_dtype is not None:
        cands.insert(0, StageModel(mc, 0, L, True, True, device=dev, dtype=torch.float32, weights=wf,
                                   max_slots=B, max_seq=max_seq, backend=ReferenceBackend(), kv_dtype=kv_dtype))
    del w, wf
    V = mc.vocab_size
    slots = list(range(B))
    factors = tuple(inject) if isinstance(inject, (tuple, list)) else (inject,)
    flat = torch.tensor([t for p in prompts for t in p], dtype=torch.int32, device=dev)
    meta = lambda: BatchMeta.build(slots, [0] * B, [len(p) for p in prompts], dev)  # noqa: E731
    errs = [[[] for _ in factors] for _ in cands]
    agree = [[0] * len(factors) for _ in cands]
    rows = 0
    with torch.no_grad():
        lg = gold.forward(meta(), flat)[:, :V].float()
        lhs = [m.forward(meta(), flat)[:, :V].float() for m in cands]
        for step in range(steps + 1):
            std = lg.std(dim=1, keepdim=True)
            for c, lh in enumerate(lhs):
                for i, f in enumerate(factors):
                    lf = lh if f == 1.0 else lg + f * (lh - lg)
                    errs[c][i].append(((lf - lg).abs().amax(dim=1, keepdim=True) / std).squeeze(1))
                    agree[c][i] += int((lf.argmax(1) == lg.argmax(1)).sum())
            rows += B
            if step == steps:
                break
            tok = lg.argmax(1).to(torch.int32)  # teacher forcing: the golden's tokens
            pos = [len(p) + step for p in prompts]
            dm = lambda: BatchMeta.decode(slots, pos, dev, max(pos) + 1)  # noqa: E731
            lg = gold.forward(dm(), tok)[:, :V].float()
            lhs = [m.forward(dm(), tok)[:, :V].float() for m in cands]
    res = []
    for c in range(len(cands)):
        out = []
        for i in range(len(factors)):
            e = torch.cat(errs[c][i])
            out.append({"rows": rows, "top1_agreement": agree[c][i] / rows, "max_rel_err": float(e.max()),
                        "mean_rel_err": float(e.mean()),
                        "per_step": [round(float(x.max()), 4) for x in errs[c][i]]})
        res.append(out if isinstance(inject, (tuple, list)) else out[0])
    return res[0] if kv_dtype is None else {"golden_kv": res[0], "hip_kv": res[1]}


def _compare_weight_dtype(model_id, prompts, steps, device, seed, inject, weight_dtype):
    """compare_with_golden(weight_dtype=): see there.  The golden over the
    dequantised weights is the reference backend's own FP8 path (it dequantises
    in ref.linear), whose quantiser the HIP one matches bit for bit."""
    mc = get_model_config(model_id) if isinstance(model_id, str) else model_id
    dev = torch.device(device)
    L = mc.n_layers
    max_seq = max(len(p) for p in prompts) + steps + 1
    B = len(prompts)
    w = init_stage_weights(mc, range(L), True, True, seed, dev, torch.bfloat16)
    mk = lambda dt, ww, be, wd: StageModel(mc, 0, L, True, True, device=dev, dtype=dt, weights=ww,  # noqa: E731
                                           max_slots=B, max_seq=max_seq, backend=be, weight_dtype=wd)
    gold = mk(torch.float32, {k: v.float() for k, v in w.items()}, ReferenceBackend(), weight_dtype)
    gold16 = mk(torch.float32, {k: v.float() for k, v in w.items()}, ReferenceBackend(), "bf16")
    hip = mk(torch.bfloat16, w, None, weight_dtype)
    del w
    V = mc.vocab_size
    slots = list(range(B))
    factors = tuple(inject) if isinstance(inject, (tuple, list)) else (inject,)
    flat = torch.tensor([t for p in prompts for t in p], dtype=torch.int32, device=dev)
    # (candidate, its reference): HIP vs the golden it shares weights with, that golden vs the bf16 one
    pairs = [(hip, gold), (gold, gold16)]
    errs = [[[] for _ in factors] for _ in pairs]
    agree = [[0] * len(factors) for _ in pairs]
    rows = 0
    with torch.no_grad():
        meta = lambda: BatchMeta.build(slots, [0] * B, [len(p) for p in prompts], dev)  # noqa: E731
        for step in range(steps + 1):
            out = {id(m): m.forward(meta(), inp)[:, :V].float() for m, inp in
                   ((m, flat if step == 0 else tok) for m in (gold, gold16, hip))}
            for c, (cand, refm) in enumerate(pairs):
                lg, lh = out[id(refm)], out[id(cand)]
                std = lg.std(dim=1, keepdim=True)
                for i, f in enumerate(factors):
                    lf = lh if f == 1.0 else lg + f * (lh - lg)
                    errs[c][i].append(((lf - lg).abs().amax(dim=1, keepdim=True) / std).squeeze(1))
                    agree[c][i] += int((lf.argmax(1) == lg.argmax(1)).sum())
            rows += B
            tok = out[id(gold)].argmax(1).to(torch.int32)  # teacher forcing: the golden's tokens
            pos = [len(p) + step for p in prompts]
            meta = lambda: BatchMeta.decode(slots, pos, dev, max(pos) + 1)  # noqa: E731
    res = []
    for c in range(len(pairs)):
        o = []
        for i in range(len(factors)):
            e = torch.cat(errs[c][i])
            o.append({"rows": rows, "top1_agreement": agree[c][i] / rows, "max_rel_err": float(e.max()),
                      "mean_rel_err": float(e.mean()),
                      "per_step": [round(float(x.max()), 4) for x in errs[c][i]]})
        res.append(o if isinstance(inject, (tuple, list)) else o[0])
    return {"hip_w": res[0], "golden_w": res[1]}


class Bf16EmulationBackend(ReferenceBackend):
    """The fp32 reference ops with the HIP path's bf16 rounding points:
    norm outputs, q, attention outputs and MLP intermediates are rounded to
    bf16 (the KV cache is bf16 by dtype), accumulation stays fp32.  HIP
    matching THIS much closer than the fp32 golden shows the remaining
    golden gap is bf16 storage, not a kernel error."""

    name = "bf16-emulation"

    @staticmethod
    def _r(x):
        return x.to(torch.bfloat16).float()

    def layernorm(self, r, w, b, eps):
        return self._r(super().layernorm(r, w, b, eps))

    def rmsnorm(self, r, w, eps):
        return self._r(super().rmsnorm(r, w, eps))

    def norm_rows(self, x, w, b, eps, rms, rows=None):
        return self._r(super().norm_rows(x, w, b, eps, rms, rows))

    def qkv_kv_append(self, xn, w, b, cache_k, cache_v, meta, mcfg):
        return self._r(super().qkv_kv_append(xn, w, b, cache_k, cache_v, meta, mcfg))

    def attention(self, q, cache_k, cache_v, meta):
        return self._r(super().attention(q, cache_k, cache_v, meta))

    def linear(self, a, w, b=None, act="none"):
        return self._r(super().linear(a, w, b, act))


def compare_three_way(model_id, prompts: List[List[int]], steps: int = 3, device: str = "cuda",
                      seed: int = 0) -> Dict[str, float]:
    """max |error| / golden std of HIP vs fp32 golden and of HIP vs the bf16
    emulation of the same model (prefill + teacher-forced decode)."""
    mc = get_model_config(model_id) if isinstance(model_id, str) else model_id
    dev = torch.device(device)
    L = mc.n_layers
    max_seq = max(len(p) for p in prompts) + steps + 1
    B = len(prompts)
    w = init_stage_weights(mc, range(L), True, True, seed, dev, torch.bfloat16)
    mk = lambda dt, be, ww: StageModel(mc, 0, L, True, True, device=dev, dtype=dt,  # noqa: E731
                                       weights=ww, max_slots=B, max_seq=max_seq, backend=be)
    gold = mk(torch.float32, ReferenceBackend(), {k: v.float() for k, v in w.items()})
    emu = mk(torch.bfloat16, Bf16EmulationBackend(), w)
    hip = mk(torch.bfloat16, None, w)
    V = mc.vocab_size
    slots = list(range(B))
    flat = torch.tensor([t for p in prompts for t in p], dtype=torch.int32, device=dev)
    out = {"golden": [], "emulation": []}
    with torch.no_grad():
        metas = lambda: BatchMeta.build(slots, [0] * B, [len(p) for p in prompts], dev)  # noqa: E731
        lg, le, lh = (m.forward(metas(), flat)[:, :V].float() for m in (gold, emu, hip))
        for step in range(steps + 1):
            std = lg.std(dim=1)
            out["golden"].append(float(((lh - lg).abs().amax(1) / std).max()))
            out["emulation"].append(float(((lh - le).abs().amax(1) / std).max()))
            if step == steps:
                break
            tok = lg.argmax(1).to(torch.int32)
            pos = [len(p) + step for p in prompts]
            lg, le, lh = (m.forward(BatchMeta.decode(slots, pos, dev, max(pos) + 1), tok)[:, :V].float()
                          for m in (gold, emu, hip))
    return out
