"""Sequence scoring on one MI355X: numbers for profiles/score_ab.log.

  gates   per case of tests/test_score_gpu.py: the error of the existing route
          (C.linear_f32 logits, float64 log-softmax) and of the fused kernel,
          both against float64 -- the test's gates are 4 x the former
  kernel  fused pair (lm_head_score) vs the existing route (linear_f32, torch
          log_softmax, gather, argmax) at GPT-2 XL T = 1024 and Llama-3 8B
          T = 8192: warm-up, the two routes alternating, medians, and the peak
          memory each route adds
  engine  Engine.score wall time of one sequence, split into forward and head

    python tools/score_ab.py [gates] [kernel] [engine=gpt2-xl:1024,...] [out=profiles/score_ab.log]
"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda"
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def gates(C):
    from tests.test_score_gpu import CASES, make_case

    say("== gates: largest |value - float64| per case (T, V, Vp, K, slices, kind)")
    worst = {"std": 0.0, "big": 0.0}
    for case in CASES:
        T, V, Vp, K, slices, kind = case
        xn, w, t, lp = make_case(T, V, Vp, K, kind)
        old = torch.log_softmax(C.linear_f32(xn, w, True, 1, None)[:, :V].double(), dim=1)
        e_old = float((old - lp).abs().max())
        tok_lp, top_id, top_lp = C.lm_head_score(xn, w, t, V, slices)
        e_tok = float((tok_lp.double() - lp.gather(1, t.long().view(-1, 1))[:, 0]).abs().max())
        e_top = float((top_lp.double() - lp.max(1).values).abs().max())
        ids = float((top_id.long() == lp.argmax(1)).float().mean())
        key = "big" if kind == "big" else "std"
        worst[key] = max(worst[key], e_old)
        say(f"{str(case):42s} existing {e_old:.3e} | fused tok_lp {e_tok:.3e} top_lp {e_top:.3e} ids equal {ids:.4f}")
    say(f"MEASURED = {worst['std']:.3e} (gate {4 * worst['std']:.3e}), "
        f"MEASURED_BIG = {worst['big']:.3e} (gate {4 * worst['big']:.3e})")


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def kernel(C, reps=7):
    say("== kernel: fused pair vs linear_f32 + log_softmax + gather + argmax (ms, medians of alternating runs)")
    for name, T, V, Vp, K in (("gpt2-xl", 1024, 50257, 50304, 1600), ("llama-3-8b", 8192, 128256, 128256, 4096)):
        g = torch.Generator(device=DEV).manual_seed(1)
        xn = torch.randn(T, K, device=DEV, generator=g).to(torch.bfloat16)
        w = (torch.randn(Vp, K, device=DEV, generator=g) * (3 / K ** 0.5)).to(torch.bfloat16)
        t = torch.randint(0, V, (T,), device=DEV, generator=g).to(torch.int32)

        def fused():
            return C.lm_head_score(xn, w, t, V, 0)

        def old():
            lp = torch.log_softmax(C.linear_f32(xn, w, True, 1, None)[:, :V], dim=1)
            top = lp.max(1)
            return lp.gather(1, t.long().view(-1, 1))[:, 0], top.indices, top.values

        for _ in range(2):
            fused(), old()
        tf, to = [], []
        for _ in range(reps):
            tf.append(_timed(fused))
            to.append(_timed(old))
        say(f"{name} T={T} V={V} K={K} slices={C.score_slices(T, Vp)}: fused {statistics.median(tf):.3f} "
            f"(min {min(tf):.3f}) | existing {statistics.median(to):.3f} (min {min(to):.3f}) | "
            f"extra memory fused {_peak(fused):.1f} MiB, existing {_peak(old):.1f} MiB")
        a, b = fused(), old()
        say(f"    agreement: tok_lp max diff {float((a[0] - b[0]).abs().max()):.3e}, "
            f"ids equal {float((a[1].long() == b[1]).float().mean()):.4f}")
        del xn, w, t, a, b


def engine(specs, reps=3):
    from llm_sharding_demo_amd.config import EngineConfig
    from llm_sharding_demo_amd.runtime.batch import BatchMeta
    from llm_sharding_demo_amd.runtime.engine import Engine

    say("== engine: Engine.score of one sequence (ms wall, median), forward / head split")
    for spec in specs:
        model, T = spec.split(":")
        T = int(T)
        eng = Engine(EngineConfig(model_id=model, num_stages=1, max_batch=4, device="cuda:0", max_seq_len=T))
        st = eng.stages[0]
        seq = torch.randint(0, eng.mcfg.vocab_size, (T,), generator=torch.Generator().manual_seed(3)).tolist()
        ids = torch.tensor(seq, dtype=torch.int32, device=st.device)
        tg = ids[1:].contiguous()
        meta = BatchMeta.build([eng.kv_slots + 1], [0], [T], st.device)
        eng.score([seq])
        whole, fwd, head = [], [], []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.score([seq])
            whole.append((time.perf_counter() - t0) * 1e3)
            x = [None]
            fwd.append(_timed(lambda: x.__setitem__(0, st.forward(meta, ids, head=False))))
            head.append(_timed(lambda: st.score_head(x[0][: T - 1], meta, tg)))
        say(f"{model} T={T}: score {statistics.median(whole):.2f} | forward {statistics.median(fwd):.2f} "
            f"| head {statistics.median(head):.2f}")
        eng.shutdown()
        del eng, st
        torch.cuda.empty_cache()


def main():
    from llm_sharding_demo_amd.ops.hip import _load

    C = _load()
    args = sys.argv[1:]
    out = next((a[4:] for a in args if a.startswith("out=")), None)
    say(f"# tools/score_ab.py {' '.join(args)}  ({torch.cuda.get_device_name(0)})")
    if "gates" in args:
        gates(C)
    if "kernel" in args:
        kernel(C)
    for a in args:
        if a.startswith("engine="):
            engine(a[7:].split(","))
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "a") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
