"""HTTP API -- wire-compatible with the reference FastAPI app.

Reference contract (`/root/reference/server.py:116-210`):
  POST /generate   {prompt, max_new_tokens=20}  -> {"generated": prompt + continuation}
  POST /forward    {input_ids: [int]}           -> {"hidden_states": [1][S][H]}   (shard A)
  POST /forward_b  {hidden_states: [B][S][H]}   -> {"logits": [B][S][V]}          (shard B)
  wrong role -> HTTP 200 {"error": "This instance is not shard A." | "...shard B." |
  "...coordinator."}  (kept for compat, quirk Q8)

Roles (env SHARD_ROLE, `server.py:21`):
  coordinator  /generate through the MI355X engine (local or torchrun pipeline);
               with TRANSPORT=http it instead drives remote a/b shards over
               HTTP exactly like the reference (compat / multi-node mode).
  a            stage 0 = embeddings + blocks[0:SPLIT_AT]          -> /forward
  b            blocks[SPLIT_AT:] + ln_f + lm_head                 -> /forward_b
  all          one process answers every endpoint (debug)
Additions: optional sampling fields on /generate (temperature, top_k, top_p,
min_p, presence_penalty, frequency_penalty, logprobs, logit_bias, banned_token_ids,
min_new_tokens, repetition_penalty, no_repeat_ngram_size, allowed_token_ids, bad_words,
bad_words_ids, stop, stop_token_ids, include_stop_in_output, guided_regex, guided_choice,
greedy, seed, stop_at_eos, prefix_cache;
defaults = reference sampler; with logprobs the response gains a "logprobs" object
beside "generated"; with stop / stop_token_ids it gains "finish_reason" and, after
a stop, "stop_reason"; a stop string is tokenised with the server's tokenizer as
given and matches that tokenisation only), 422 on empty/over-long
prompts (instead of the reference's 500, quirk Q9), GET /health, GET /metrics
(Prometheus text).  Concurrent /generate calls are batched at decode-step
granularity by the engine's continuous-batching scheduler
(runtime/scheduler.py): a request joins the running batch at the next step
and leaves as soon as it has its tokens; a progress watchdog turns a hung
pipeline into 503s instead of hanging requests.
"""
from __future__ import annotations

import logging
import os
import time
from typing import Dict, List, Optional, Union

import torch
from pydantic import BaseModel, StrictBool

from ..config import EngineConfig, SamplingParams
from ..utils import racecheck
from ..utils.metrics import Metrics
from ..utils.tokenizer import encode_bad_words, encode_stops, load_tokenizer

log = logging.getLogger("llm_sharding_demo_amd.server")


# Wire schemas -- `server.py:116-124`, plus optional sampling fields.
class InputIDs(BaseModel):
    input_ids: List[int]


class HiddenStates(BaseModel):
    hidden_states: list  # nested lists (batch, seq, hidden_dim)


class GenerateReq(BaseModel):
    prompt: str
    max_new_tokens: int = 20
    temperature: float = 0.6
    top_k: int = 40
    greedy: bool = False
    seed: Optional[int] = None
    stop_at_eos: bool = False
    top_p: float = 1.0   # nucleus cut inside the top-k candidates (1 = off)
    min_p: float = 0.0   # keep tokens >= min_p x the most likely one (0 = off)
    presence_penalty: float = 0.0   # off every generated token's logit, once (in [-2, 2])
    frequency_penalty: float = 0.0  # off it again per occurrence so far (in [-2, 2])
    # alternatives returned with every generated token's logprob (None = no "logprobs" in the response)
    logprobs: Optional[int] = None
    # logit edits ahead of every draw: {token id: value in [-100, 100]} added to the logits,
    # tokens that can never be drawn, and draws (from the first) in which EOS cannot be drawn
    logit_bias: Optional[Dict[str, float]] = None
    banned_token_ids: Optional[List[int]] = None
    min_new_tokens: int = 0
    # the two rules over prompt + output: logits of tokens already there / r (* r when negative),
    # r in (0, 10]; and no G-gram (G in [0, 32]) that is already there is completed again
    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    # the only tokens that may be drawn (None = the whole vocabulary): every other logit is -inf
    allowed_token_ids: Optional[List[int]] = None
    # token sequences that may never be completed over prompt + output: as strings -- each tokenised
    # with the server's tokenizer as given and, when that differs, with a leading space -- and as ids
    bad_words: Optional[List[str]] = None
    bad_words_ids: Optional[List[List[int]]] = None
    # the request ends when its output completes one of these: strings -- each tokenised with the
    # server's tokenizer as given; a stop string matches that tokenisation only -- and token ids.
    # The matched tokens are left out of the output unless include_stop_in_output is set
    stop: Optional[Union[str, List[str]]] = None
    stop_token_ids: Optional[List[int]] = None
    include_stop_in_output: bool = False
    # guided decoding: the output, as bytes, matches the regular expression as a whole (guide.py
    # compile_regex's syntax) or is one of the strings; at most one of the two.  Compiled with the
    # server's tokenizer; EOS is allowed exactly where the match is complete, so set stop_at_eos
    guided_regex: Optional[str] = None
    guided_choice: Optional[List[str]] = None
    # samples of the prompt (at most MAX_SAMPLES, the microbatch capacity and the KV slots):
    # sample i draws with seed + i; with n > 1 the response keeps "generated" for sample 0
    # and adds "choices", one object per sample
    n: int = 1
    # false: the request neither starts from the engine's prefix cache (PREFIX_CACHE entries)
    # nor leaves an entry behind; a JSON bool.  While the cache is on the response gains
    # "cached_tokens", the leading prompt tokens whose prefill an entry's KV replaced
    prefix_cache: StrictBool = True


class GuideCache:
    """The guides /generate compiled, least recently used out first: (kind,
    pattern) -> TokenGuide.  Thread-safe; a guide is compiled outside the lock,
    so two first requests for one pattern may both compile it (equal guides:
    the engine interns them to one table row)."""

    def __init__(self, tok, vocab: int, eos: Optional[int], size: int = 32):
        import collections

        self.tok, self.vocab, self.eos, self.size = tok, vocab, eos, size
        self._bytes = None
        self._lru = collections.OrderedDict()
        self._lock = racecheck.Lock("guide_cache")

    def get(self, kind: str, pattern):
        from ..guide import compile_choice, compile_regex

        key = (kind, pattern if kind == "regex" else tuple(pattern))
        with self._lock:
            g = self._lru.get(key)
            if g is not None:
                self._lru.move_to_end(key)
                return g
            if self._bytes is None:
                self._bytes = self.tok.token_bytes(self.vocab)
            tb = self._bytes
        g = (compile_regex if kind == "regex" else compile_choice)(pattern, tb, self.eos)
        with self._lock:
            self._lru[key] = g
            self._lru.move_to_end(key)
            while len(self._lru) > self.size:
                self._lru.popitem(last=False)
        return g


def logprobs_json(lp) -> dict:
    """The "logprobs" object of a /generate response from a request's records
    (runtime/scheduler.py Logprobs); non-finite values go out as null."""
    import math

    num = lambda v: v if math.isfinite(v) else None  # noqa: E731
    return {"tokens": list(lp.tokens), "token_logprobs": [num(v) for v in lp.token_logprobs],
            "top_logprobs": [[{"id": i, "logprob": num(v)} for i, v in alts] for alts in lp.top_logprobs]}


class ShardRunner:
    """A single shard process (role a or b): one StageModel over a layer range."""

    def __init__(self, cfg: EngineConfig, role: str, device=None):
        from ..models.stage import StageModel
        from ..runtime.engine import _dtype, resolve_device

        mc = cfg.model
        split = (cfg.split_points or [1])[0]
        if not 0 <= split <= mc.n_layers:
            raise ValueError(f"SPLIT_AT={split} outside [0, {mc.n_layers}]")
        dev = resolve_device(device or cfg.device)
        a, b = (0, split) if role == "a" else (split, mc.n_layers)
        self.stage = StageModel(mc, a, b, first=(role == "a"), last=(role == "b"), device=dev,
                                dtype=_dtype(cfg.dtype, dev), seed=cfg.seed,
                                weights_path=cfg.weights, max_slots=1,
                                max_seq=min(cfg.max_seq_len, mc.max_positions))
        self.role = role
        self.lock = racecheck.Lock("shard_runner")

    def run(self, x: torch.Tensor, seq_len: int) -> torch.Tensor:
        from ..runtime.batch import BatchMeta

        st = self.stage
        if seq_len > st.max_seq:
            raise ValueError(f"sequence length {seq_len} exceeds {st.max_seq}")
        with self.lock:
            meta = BatchMeta.build([0], [0], [seq_len], st.device)
            out = st.forward(meta, x.to(st.device), all_logits=True)
        return out


def create_app(cfg: EngineConfig, engine=None, shard: Optional[ShardRunner] = None):
    from fastapi import FastAPI, HTTPException
    from fastapi.responses import PlainTextResponse

    role = cfg.role
    mc = cfg.model
    tok = load_tokenizer(cfg.model_id, mc.arch, cfg.weights, mc.eos_token_id)
    guides = GuideCache(tok, mc.vocab_size, mc.eos_token_id)
    metrics = Metrics()
    app = FastAPI(title="llm-sharding-demo (MI355X)")
    app.state.engine, app.state.shard, app.state.metrics = engine, shard, metrics
    watchdog = None
    if engine is not None:
        from ..runtime.scheduler import Watchdog

        engine.start_loop()
        # dist engines run their own (every rank); local ones get one here
        watchdog = getattr(engine, "watchdog", None) or Watchdog(engine, cfg.round_timeout_s)
    app.state.watchdog = watchdog

    def _role_is(*roles):
        return role in roles or role == "all"

    @app.post("/forward")
    def forward_a(req: InputIDs):
        if not _role_is("a"):
            return {"error": "This instance is not shard A."}
        if not req.input_ids:
            raise HTTPException(422, "input_ids must be non-empty")
        ids = torch.tensor(req.input_ids, dtype=torch.int32)
        try:
            if shard is not None:
                h = shard.run(ids, len(req.input_ids))
            else:
                h = engine.forward_a(req.input_ids)
        except ValueError as e:
            raise HTTPException(422, str(e))
        except RuntimeError as e:  # e.g. a single-stage engine has no shard A / B split
            raise HTTPException(400, str(e))
        return {"hidden_states": h.float().cpu().unsqueeze(0).tolist()}

    @app.post("/forward_b")
    def forward_b(req: HiddenStates):
        if not _role_is("b"):
            return {"error": "This instance is not shard B."}
        hidden = torch.tensor(req.hidden_states, dtype=torch.float32)
        if hidden.dim() != 3 or hidden.shape[-1] != mc.hidden:
            raise HTTPException(422, f"hidden_states must be [B][S][{mc.hidden}]")
        B, S, H = hidden.shape
        outs = []
        try:
            for b in range(B):
                if shard is not None:
                    lg = shard.run(hidden[b], S)[:, : mc.vocab_size]
                else:
                    lg = engine.forward_b(hidden[b])
                outs.append(lg.float().cpu())
        except ValueError as e:
            raise HTTPException(422, str(e))
        except RuntimeError as e:
            raise HTTPException(400, str(e))
        return {"logits": torch.stack(outs).tolist()}

    @app.post("/generate")
    def generate(req: GenerateReq):
        if not _role_is("coordinator"):
            return {"error": "This instance is not coordinator."}
        ids = tok.encode(req.prompt)
        bad = None
        if req.bad_words is not None or req.bad_words_ids is not None:
            bad = [list(w) for w in req.bad_words_ids or ()] + encode_bad_words(tok, req.bad_words or ())
        stops = encode_stops(tok, req.stop) if req.stop is not None else None
        guide = None
        if req.guided_regex is not None and req.guided_choice is not None:
            raise HTTPException(422, "guided_regex and guided_choice: give one of the two")
        if req.guided_regex is not None or req.guided_choice is not None:
            try:
                guide = (guides.get("regex", req.guided_regex) if req.guided_regex is not None
                         else guides.get("choice", req.guided_choice))
            except ValueError as e:
                raise HTTPException(422, str(e))
        asked_stop = req.stop is not None or req.stop_token_ids is not None
        sp = SamplingParams(temperature=req.temperature, top_k=req.top_k, greedy=req.greedy,
                            seed=req.seed, max_new_tokens=req.max_new_tokens,
                            stop_at_eos=req.stop_at_eos, top_p=req.top_p, min_p=req.min_p,
                            presence_penalty=req.presence_penalty, frequency_penalty=req.frequency_penalty,
                            logprobs=req.logprobs, logit_bias=req.logit_bias,
                            banned_token_ids=req.banned_token_ids, min_new_tokens=req.min_new_tokens,
                            repetition_penalty=req.repetition_penalty,
                            no_repeat_ngram_size=req.no_repeat_ngram_size,
                            allowed_token_ids=req.allowed_token_ids, bad_words=bad,
                            stop_token_ids=req.stop_token_ids, stop_sequences=stops,
                            include_stop_in_output=req.include_stop_in_output, guide=guide, n=req.n,
                            prefix_cache=req.prefix_cache)
        if req.max_new_tokens == 0 and req.logprobs is None and req.n == 1:
            return {"generated": tok.decode(ids, skip_special_tokens=True)}
        if not ids:
            raise HTTPException(422, "prompt must encode to at least one token")
        t0 = time.perf_counter()
        from ..runtime.scheduler import RequestTimeout

        lp = None
        reason = ("length", None)
        cached = 0  # Request.cached_tokens
        each = None  # n > 1: (tokens, logprob records, reasons) of every sample
        try:
            sp.validate(cfg.max_logprobs, cfg.max_logit_edits, cfg.max_bad_words, cfg.max_bad_word_tokens,
                        cfg.max_stop_sequences, max_guide_classes=cfg.max_guide_classes,
                        max_guide_cells=cfg.max_guide_cells)
            if sp.n > cfg.max_samples:
                raise ValueError(f"n = {sp.n} exceeds max_samples = {cfg.max_samples}")
            if req.max_new_tokens == 0:
                from ..runtime.scheduler import Logprobs

                out, lp = [], Logprobs([], [], []) if req.logprobs is not None else None
                each = [(out, lp, reason)] * sp.n
            elif engine is not None:
                if len(ids) + sp.max_new_tokens > engine.max_seq:
                    raise ValueError(f"prompt ({len(ids)}) + max_new_tokens ({sp.max_new_tokens}) "
                                     f"exceeds the context limit {engine.max_seq}")
                req_ = engine.submit(ids, sp)
                out = req_.wait(timeout=cfg.request_timeout_s)
                lp, reason, cached = req_.logprobs, (req_.finish_reason, req_.stop_reason), req_.cached_tokens
                each =[(s.wait(0), s.logprobs, (s.finish_reason, s.stop_reason)) for s in req_.samples]
                metrics.observe_request(sum(len(e[0]) for e in each), time.perf_counter() - t0,
                                        ttft_s=(req_.t_first - req_.t_submit) if req_.t_first else None)
            else:
                # the relay has no engine: the samples one after another, sample i with seed + i
                import dataclasses

                base = sp.seed
                if base is None and sp.n > 1:
                    base = int.from_bytes(os.urandom(7), "little")
                each = [http_generate(cfg, ids, dataclasses.replace(sp, n=1, seed=None if base is None else base + i),
                                      records=True, reasons=True) for i in range(sp.n)]
                out, lp, reason = each[0]
                metrics.observe_request(sum(len(e[0]) for e in each), time.perf_counter() - t0)
        except ValueError as e:
            raise HTTPException(422, str(e))
        except RequestTimeout as e:
            raise HTTPException(504, str(e))
        except RuntimeError as e:
            if engine is not None and not engine.healthy:
                raise HTTPException(503, f"engine unhealthy: {engine.last_error}")
            raise
        def sample_json(out, lp, reason):
            b = {"generated": tok.decode(ids + out, skip_special_tokens=True)}
            if lp is not None:
                b["logprobs"] = logprobs_json(lp)
            if asked_stop:
                b["finish_reason"] = reason[0]
                if reason[1] is not None:
                    b["stop_reason"] = reason[1]
            return b

        body = sample_json(out, lp, reason)
        if sp.n > 1:
            body["choices"] = [sample_json(*e) for e in each]
        if engine is not None and engine.cfg.prefix_cache > 0:
            body["cached_tokens"] = cached
        return body

    @app.get("/health")
    def health():
        ok = engine.healthy if engine is not None else True
        body = {"status": "ok" if ok else "unhealthy", "role": role, "model": mc.name}
        if engine is not None:
            body.update(stages=engine.P, plan=engine.plan, unit_plan=engine.unit_plan, mode=engine.mode,
                        devices=[str(d) for d in engine.devices], **engine.kv_info())
            if engine.cfg.prefix_cache > 0:
                body["prefix_cache"] = engine.prefix_cache_stats()
            if not ok:
                body["error"] = engine.last_error
        if shard is not None:
            body.update(layers=[shard.stage.layer_start, shard.stage.layer_end],
                        device=str(shard.stage.device))
        return body

    @app.get("/metrics", response_class=PlainTextResponse)
    def prom():
        gauges, counters = {}, {}
        if engine is not None:
            sch = engine.scheduler
            kv = engine.kv_info()
            gauges = {"engine_healthy": 1 if engine.healthy else 0,
                      "engine_stages": engine.P,
                      "kv_slots_free": kv["kv_slots_free"],
                      "kv_slots_total": kv["kv_slots"] * engine.R,
                      "kv_cache_bytes_stage0": kv["kv_bytes_stage0"],
                      "queue_depth": sch.queue_depth,
                      "max_batch_rows_seen": sch.stats["max_rows"]}
            counters = {"pipeline_steps_total": sch.stats["steps"],
                        "sequence_joins_total": sch.stats["joins"],
                        "sequence_leaves_total": sch.stats["leaves"],
                        "hipgraph_captures_total": sum(w.captures for w in engine.workers)}
            if engine.cfg.prefix_cache > 0:
                pc = engine.prefix_cache_stats()
                gauges["prefix_cache_entries"] = pc["entries"]
                counters.update(prefix_cache_hits_total=pc["hits"], prefix_cache_misses_total=pc["misses"],
                                prefix_cache_tokens_reused_total=pc["tokens_reused"],
                                prefix_cache_evictions_total=pc["evictions"])
            ls = engine.last_session
            if ls is not None:
                if ls.step_times_ms:
                    metrics.observe_steps(ls.step_times_ms, key=id(ls))
                for st in ls.stages:
                    tag = f"stage{st['stage']}" + (f"_replica{st['replica']}" if st.get("replica") else "")
                    gauges[f"{tag}_busy_fraction"] = st["busy_fraction"]
                    gauges[f"{tag}_bubble_fraction"] = 1.0 - st["busy_fraction"]
        return metrics.render(gauges, counters)

    return app


def http_generate(cfg: EngineConfig, ids: List[int], sp: SamplingParams, records: bool = False,
                  reasons: bool = False):
    """Reference-style coordinator loop over remote shards (`server.py:169-206`):
    full-sequence recompute on every step, hidden states relayed through here.
    Kept for deployments where the shards are separate hosts without xGMI.
    This relay keeps the reference's sampler: presence_penalty and
    frequency_penalty, repetition_penalty and no_repeat_ngram_size are ignored
    here; logit_bias, banned_token_ids and
    min_new_tokens are applied on the host (ops/reference.py logit_edits; ids
    outside the vocabulary are ignored), allowed_token_ids behind them
    (ops/reference.py allow_mask), bad_words ahead of both over prompt +
    output (ops/reference.py bad_words), a guide last of all, its state in a
    one-slot table here (ops/reference.py guide_mask / guide_advance);
    stop_token_ids and stop_sequences end
    the loop by SamplingParams.stop_match (reasons=True: -> (tokens, records,
    (finish_reason, stop_reason))).  records=True: -> (tokens, the logprob
    records of a request that asked for them or None), computed on the host
    from the logits this loop already holds (ops/reference.py logprobs)."""
    import requests

    from ..ops import reference as ref
    from ..runtime.batch import counter_uniform

    seed = sp.seed if sp.seed is not None else int.from_bytes(__import__("os").urandom(7), "little")
    vocab = cfg.model.vocab_size
    out: List[int] = []
    lp = None
    if sp.logprobs is not None:
        from ..runtime.scheduler import Logprobs

        lp = Logprobs(out, [], [])
    table = None
    if sp.has_logit_edits:
        table = tuple(torch.tensor([col], dtype=dt) for col, dt in zip(
            sp.logit_edits(cfg.model.eos_token_id), (torch.int32, torch.float32, torch.int32)))
        table = (torch.tensor([table[0].shape[1]], dtype=torch.int32),) + table
    allow = None
    if sp.allowed_token_ids is not None:
        allow = (torch.ones(1, dtype=torch.int32),
                 torch.from_numpy(sp.allowed_mask((cfg.model.vocab_padded + 31) // 32))[None])
    bad = None
    if sp.bad_words is not None and sp.bad_word_entries() is not None:
        ends, toks = sp.bad_word_entries()
        bad = (torch.tensor([len(ends)], dtype=torch.int32), torch.tensor([ends], dtype=torch.int32),
               torch.tensor([toks], dtype=torch.int32))
    gtab = None
    if sp.guide is not None:
        import numpy as np

        g, width = sp.guide, max(cfg.model.vocab_padded, sp.guide.vocab)
        cls = np.zeros((1, width), dtype=np.int16)
        cls[0, : g.vocab] = g.cls
        # one guide row, one slot in the start state
        gtab = (torch.from_numpy(cls), torch.from_numpy(np.ascontiguousarray(g.next).reshape(1, -1).copy()),
                torch.tensor([[g.S, g.C]], dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32))
    stops, reason = sp.stop_list(), ("length", None)
    seq = list(ids)
    url_a = f"http://{cfg.shard_a_service}:{cfg.shard_port}/forward"
    url_b = f"http://{cfg.shard_b_service}:{cfg.shard_port}/forward_b"
    for step in range(sp.max_new_tokens):
        r = requests.post(url_a, json={"input_ids": seq}, timeout=30)
        r.raise_for_status()
        hidden = r.json()["hidden_states"]
        r2 = requests.post(url_b, json={"hidden_states": hidden}, timeout=30)
        r2.raise_for_status()
        logits = torch.tensor(r2.json()["logits"], dtype=torch.float32)[0, -1:]
        if bad is not None:
            # a one-slot context table: the whole sequence so far as the prompt, draw 0
            ctx = (torch.tensor([len(seq)], dtype=torch.int32), None, None, torch.tensor([seq], dtype=torch.int32))
            ref.bad_words(logits, bad, ctx, torch.tensor([0]), None, min(vocab, logits.shape[1]))
        if table is not None:
            ref.logit_edits(logits, table, torch.tensor([0]), torch.tensor([step]), vocab)
        if allow is not None:
            ref.allow_mask(logits, allow, torch.tensor([0]), min(vocab, logits.shape[1]))
        if gtab is not None:
            ref.guide_mask(logits, gtab, torch.tensor([0]), min(vocab, logits.shape[1]))
        u = counter_uniform(torch.tensor([seed]), torch.tensor([step]))
        nxt = int(ref.sample(logits, torch.tensor([sp.temperature]), torch.tensor([sp.top_k]),
                             torch.tensor([1 if sp.greedy else 0]), u, vocab,
                             torch.tensor([sp.top_p]), torch.tensor([sp.min_p]))[0])
        if gtab is not None:
            ref.guide_advance(gtab, torch.tensor([0]), torch.tensor([nxt]), min(vocab, logits.shape[1]))
        seq.append(nxt)
        out.append(nxt)
        if lp is not None:
            t, ti, tv = ref.logprobs(logits, torch.tensor([nxt]), [sp.logprobs], vocab, sp.logprobs)
            lp.token_logprobs.append(float(t[0]))
            lp.top_logprobs.append([(i, v) for i, v in zip(ti[0].tolist(), tv[0].tolist()) if i >= 0])
        hit = sp.stop_match(out, stops) if stops else None
        if hit is not None:
            reason = ("stop", hit)
            if not sp.include_stop_in_output:
                keep = len(out) - len(stops[hit])
                del out[keep:]  # the records' token list too
                if lp is not None:
                    del lp.token_logprobs[keep:], lp.top_logprobs[keep:]
            break
    if reasons:
        return out, lp, reason
    return (out, lp) if records else out
