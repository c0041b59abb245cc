"""Op backends.

The model code (models/stage.py: the GPT-2 and Llama blocks of one pipeline
stage) is written once against the `Backend` interface below.  Two implementations exist:

* `ReferenceBackend` -- plain PyTorch in fp32 (ops/reference.py).  Used on CPU
  (tests, golden numerics, the tiny-gpt2 reference config).
* `HipBackend` (ops/hip.py) -- the hand-written CDNA4 kernels in
  csrc/kernels/*.hip, routed by one table (ops/routing.py).  Used for every
  tensor on a GPU; hipBLASLt only runs when an A/B run asks for it
  (LSD_ROUTING=blaslt=1).  There is no silent fallback: if the extension is
  missing on a GPU box, `get_backend` raises.

Residual stream convention: the residual `x` is fp32 [T, H].  GEMMs whose
epilogue is "add into the residual" may split K across workgroups; their
fp32 partial slabs are parked in `Residual.pending` and folded into `x` by the
next norm (or `flush`).  This keeps the reduction deterministic and costs no
extra kernel launch.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import torch

from . import reference as ref


@dataclass
class Residual:
    x: torch.Tensor  # fp32 [T, H]
    pending: List[Tuple[torch.Tensor, Optional[torch.Tensor]]] = field(default_factory=list)


class Backend:
    name = "abstract"

    def prepare_stage(self, stage) -> None:  # optional weight re-layout
        pass


class ReferenceBackend(Backend):
    """fp32 PyTorch implementation of the engine ops (CPU golden path)."""

    name = "reference"

    def embed(self, ids, pos, wte, wpe):
        return ref.embed(ids, pos, wte, wpe)

    def _combine(self, r: Residual) -> None:
        for slabs, bias in r.pending:
            r.x += slabs.sum(0)
            if bias is not None:
                r.x += bias.float()
        r.pending.clear()

    def flush(self, r: Residual) -> torch.Tensor:
        self._combine(r)
        return r.x

    def layernorm(self, r: Residual, w, b, eps):
        self._combine(r)
        return ref.layernorm(r.x, w, b, eps)

    def rmsnorm(self, r: Residual, w, eps):
        self._combine(r)
        return ref.rmsnorm(r.x, w, eps)

    def norm_rows(self, x, w, b, eps, rms: bool, rows=None):
        if rows is not None:
            x = x.index_select(0, rows.long())
        return ref.rmsnorm(x, w, eps) if rms else ref.layernorm(x, w, b, eps)

    def qkv_kv_append(self, xn, w, b, cache_k, cache_v, meta, mcfg):
        """QKV projection; K,V appended to the cache at (slot, pos); returns q [T, nh, hd]."""
        y = ref.linear(xn, w, b)
        T = y.shape[0]
        hd = mcfg.head_dim
        q = y[:, : mcfg.q_size].reshape(T, mcfg.n_heads, hd)
        k = y[:, mcfg.q_size: mcfg.q_size + mcfg.kv_size].reshape(T, mcfg.n_kv_heads, hd)
        v = y[:, mcfg.q_size + mcfg.kv_size:].reshape(T, mcfg.n_kv_heads, hd)
        if mcfg.arch == "llama":
            q = ref.apply_rope(q, meta.token_pos.cpu(), mcfg.rope_theta)
            k = ref.apply_rope(k, meta.token_pos.cpu(), mcfg.rope_theta)
        ref.kv_append(cache_k, cache_v, k, v, meta.token_slots, meta.token_pos)
        return q

    def attention(self, q, cache_k, cache_v, meta):
        o = ref.attention(q, cache_k, cache_v, meta.seq_slots, meta.q_start, meta.cu_q)
        return o.reshape(o.shape[0], -1)

    def linear(self, a, w, b=None, act: str = "none"):
        y = ref.linear(a, w, b)
        if act == "gelu":
            y = ref.gelu_new(y)
        elif act == "silu_mul":
            f = y.shape[1] // 2
            y = ref.silu_mul(y[:, :f], y[:, f:])
        return y

    def linear_residual(self, a, w, b, r: Residual) -> None:
        self._combine(r)
        r.x += ref.linear(a, w, b)

    def logits(self, xn, w):
        return ref.linear(xn, w)

    def sample(self, logits, samp, vocab: int):
        return ref.sample(logits, samp.temperature, samp.top_k, samp.greedy,
                          samp.uniforms(), vocab, samp.top_p, samp.min_p)

    def sample_into(self, logits, samp, vocab: int, out, meta=None) -> None:
        """Decode step: sampled ids into `out`, then the sampler counters (and,
        given the decode `meta`, its positions) advance."""
        out.copy_(self.sample(logits, samp, vocab))
        samp.advance()
        if meta is not None:
            meta.advance()

    def penalize(self, logits, hist, slots, counts, presence, frequency, vocab: int) -> None:
        """Presence / frequency penalties of the rows' generated-token
        histories, in place on the fp32 logits, ahead of the sampler."""
        ref.penalize(logits, hist, slots, counts, presence, frequency, vocab)

    def logit_edits(self, logits, table, slots, step, vocab: int) -> None:
        """The rows' logit_bias / ban / min_new_tokens entries (table = the
        last stage's per-slot cnt, tok, val, until), in place on the fp32
        logits, after the penalties and ahead of the sampler; step None = draw 0."""
        ref.logit_edits(logits, table, slots, step, vocab)

    def repetition(self, logits, table, slots, step, vocab: int) -> None:
        """HF-style repetition_penalty and no_repeat_ngram_size over the rows'
        prompt + generated tokens (table = the last stage's per-slot plen,
        rpen, ngram, tok), in place on the fp32 logits, ahead of the penalties,
        the logit edits and the sampler; step None = draw 0."""
        ref.repetition(logits, table, slots, step, vocab)

    def record_context(self, table, slots, step, tokens, active=None, back: int = 0) -> None:
        ref.record_context(table, slots, step, tokens, active, back)

    def bad_words(self, logits, table, ctx_table, slots, step, vocab: int) -> None:
        """The rows' bad_words (table = the last stage's per-slot cnt, end,
        tok; ctx_table = its context table): -inf at the last token of every
        sequence whose other tokens the row's prompt + generated tokens end
        with, in place on the fp32 logits, right after the repetition pass;
        step None = draw 0."""
        ref.bad_words(logits, table, ctx_table, slots, step, vocab)

    def allow_mask(self, logits, table, slots, vocab: int) -> None:
        """The rows' allowed_token_ids (table = the last stage's per-slot on,
        bits): -inf at every token of [0, vocab) whose bit is clear, in place
        on the fp32 logits, after the edits and ahead of the sampler."""
        ref.allow_mask(logits, table, slots, vocab)

    def guide_mask(self, logits, table, slots, vocab: int) -> None:
        """The rows' guides (table = the last stage's gcls, gnext, gdim, gsl):
        -inf at every token of [0, vocab) that the state of the row's slot
        does not allow, in place on the fp32 logits, the last edit ahead of
        the sampler."""
        ref.guide_mask(logits, table, slots, vocab)

    def guide_advance(self, table, slots, tokens, vocab: int, active=None) -> None:
        """Behind the draw: the state of every active guided row's slot
        becomes the one its drawn token leads to."""
        ref.guide_advance(table, slots, tokens, vocab, active)

    def record_tokens(self, hist, slots, step, tokens, active=None, back: int = 0) -> None:
        ref.record_tokens(hist, slots, step, tokens, active, back)

    def logprobs(self, logits, tokens, nlp, slots, step, active, rec, vocab: int, back: int = 0) -> None:
        """Logprob records of the rows with nlp >= 0 (ops/reference.py logprobs),
        after the sampler wrote `tokens`: into rec = (lp_tok, lp_top_id,
        lp_top) at [slots[i], step[i] - back]."""
        W = rec[1].shape[2]
        ref.record_logprobs(rec, slots, step, nlp, *ref.logprobs(logits, tokens, nlp, vocab, W), active, back)

    def kv_fork(self, buf, src, dst, lens, idx=None) -> None:
        """Fork prompts' KV (SamplingParams.n): positions [0, lens[f]) of slot
        src[f] of a stage's whole KV allocation go to slot dst[f], for every
        layer, K and V, and head.  src, dst, lens: host integers; idx: the
        same on the device (the HIP backend's kernel reads them there)."""
        ref.kv_fork(buf, src, dst, lens)

    def gather_rows(self, x, idx):
        return x.index_select(0, idx.long())


_REFERENCE = ReferenceBackend()


def hip_available() -> bool:
    try:
        from . import hip  # noqa: F401
        return hip.extension_loaded()
    except Exception:  # pragma: no cover - depends on build
        return False


def get_backend(device) -> Backend:
    dev = torch.device(device)
    if dev.type == "cpu":
        return _REFERENCE
    from .hip import HipBackend  # raises loudly if the extension is missing

    return HipBackend()  # one per stage: owns that stage's split-K counters / tables
