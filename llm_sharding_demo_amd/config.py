"""Configuration: model presets, engine settings, env-var compatibility.

The reference configures itself only through six environment variables
(`/root/reference/server.py:20-25`): MODEL_ID, SHARD_ROLE, SPLIT_AT,
SHARD_A_SERVICE, SHARD_B_SERVICE, SHARD_PORT.  Those names are kept here with
the same defaults; everything else the MI355X engine needs (stage count,
microbatching, KV budget, sampling defaults) is a dataclass field that can be
set from CLI > env > defaults.

Sampling defaults match the reference's hard-coded sampler
(`server.py:187-188`: temperature 0.6, top-k 40, multinomial).
"""
from __future__ import annotations

import dataclasses
import math
import operator
import os
from dataclasses import dataclass, field
from typing import Mapping, Optional, Sequence


# ---------------------------------------------------------------------------
# Model presets
# ---------------------------------------------------------------------------

@dataclass(frozen=True)
class ModelConfig:
    """Architecture description shared by the GPT-2 and Llama families."""

    name: str
    arch: str  # "gpt2" | "llama"
    vocab_size: int
    hidden: int
    n_layers: int
    n_heads: int
    n_kv_heads: int
    ffn: int
    max_positions: int
    norm_eps: float
    tie_embeddings: bool
    rope_theta: float = 0.0
    bos_token_id: int = 50256
    eos_token_id: int = 50256

    @property
    def head_dim(self) -> int:
        return self.hidden // self.n_heads

    @property
    def q_size(self) -> int:
        return self.n_heads * self.head_dim

    @property
    def kv_size(self) -> int:
        return self.n_kv_heads * self.head_dim

    @property
    def qkv_size(self) -> int:
        return self.q_size + 2 * self.kv_size

    @property
    def vocab_padded(self) -> int:
        """Vocab rounded up to a multiple of 64 so lm_head tiles evenly."""
        return (self.vocab_size + 63) // 64 * 64

    def block_params(self) -> int:
        h, f = self.hidden, self.ffn
        if self.arch == "gpt2":
            return 12 * h * h + 13 * h  # qkv+proj+fc+proj weights/biases + 2 LN
        return h * self.qkv_size + self.q_size * h + 3 * h * f + 2 * h

    def embed_params(self) -> int:
        n = self.vocab_size * self.hidden
        if self.arch == "gpt2":
            n += self.max_positions * self.hidden
        return n

    def lm_head_params(self) -> int:
        return self.vocab_size * self.hidden

    def kv_bytes_per_token_per_layer(self, dtype_bytes: int = 2) -> int:
        return 2 * self.kv_size * dtype_bytes


def _gpt2(name: str, h: int, l: int, nh: int, vocab: int = 50257) -> ModelConfig:
    return ModelConfig(
        name=name, arch="gpt2", vocab_size=vocab, hidden=h, n_layers=l,
        n_heads=nh, n_kv_heads=nh, ffn=4 * h, max_positions=1024,
        norm_eps=1e-5, tie_embeddings=True)


# Dims from [tf5.15] models/gpt2/configuration_gpt2.py and SURVEY.md §2.5.
MODEL_PRESETS = {
    # sshleifer/tiny-gpt2: the reference default MODEL_ID (server.py:20)
    "tiny-gpt2": _gpt2("tiny-gpt2", 2, 2, 2),
    "gpt2": _gpt2("gpt2", 768, 12, 12),
    "gpt2-medium": _gpt2("gpt2-medium", 1024, 24, 16),
    "gpt2-large": _gpt2("gpt2-large", 1280, 36, 20),
    "gpt2-xl": _gpt2("gpt2-xl", 1600, 48, 25),
    # Small GPT-2 shapes used by kernel / pipeline tests (hd = 64 like real GPT-2).
    "gpt2-test": _gpt2("gpt2-test", 128, 4, 2, vocab=1000),
    "llama-3-8b": ModelConfig(
        name="llama-3-8b", arch="llama", vocab_size=128256, hidden=4096,
        n_layers=32, n_heads=32, n_kv_heads=8, ffn=14336, max_positions=8192,
        norm_eps=1e-5, tie_embeddings=False, rope_theta=500000.0,
        bos_token_id=128000, eos_token_id=128001),
    "llama-test": ModelConfig(
        name="llama-test", arch="llama", vocab_size=1000, hidden=256,
        n_layers=4, n_heads=4, n_kv_heads=2, ffn=512, max_positions=2048,
        norm_eps=1e-5, tie_embeddings=False, rope_theta=10000.0,
        bos_token_id=1, eos_token_id=2),
}

_ALIASES = {
    "sshleifer/tiny-gpt2": "tiny-gpt2",
    "openai-community/gpt2": "gpt2",
    "gpt2-small": "gpt2",
    "openai-community/gpt2-medium": "gpt2-medium",
    "openai-community/gpt2-large": "gpt2-large",
    "openai-community/gpt2-xl": "gpt2-xl",
    "meta-llama/Meta-Llama-3-8B": "llama-3-8b",
    "meta-llama/Llama-3.1-8B": "llama-3-8b",
    "llama3-8b": "llama-3-8b",
}


def get_model_config(model_id: str) -> ModelConfig:
    """Resolve a preset name or HF-style id to a ModelConfig."""
    key = _ALIASES.get(model_id, model_id)
    if key in MODEL_PRESETS:
        return MODEL_PRESETS[key]
    # A local HF directory with a config.json: read the dims from it.
    cfg_path = os.path.join(model_id, "config.json")
    if os.path.isfile(cfg_path):
        return model_config_from_hf_json(cfg_path)
    raise KeyError(f"unknown model {model_id!r}; presets: {sorted(MODEL_PRESETS)}")


def model_config_from_hf_json(path: str) -> ModelConfig:
    import json

    with open(path) as f:
        c = json.load(f)
    mt = c.get("model_type", "gpt2")
    if mt == "gpt2":
        h = c["n_embd"]
        return ModelConfig(
            name=os.path.basename(os.path.dirname(path)) or "gpt2", arch="gpt2",
            vocab_size=c["vocab_size"], hidden=h, n_layers=c["n_layer"],
            n_heads=c["n_head"], n_kv_heads=c["n_head"],
            ffn=c.get("n_inner") or 4 * h, max_positions=c["n_positions"],
            norm_eps=c.get("layer_norm_epsilon", 1e-5), tie_embeddings=True,
            bos_token_id=c.get("bos_token_id", 50256),
            eos_token_id=c.get("eos_token_id", 50256))
    if mt == "llama":
        eos = c.get("eos_token_id", 2)
        if isinstance(eos, list):
            eos = eos[0]
        return ModelConfig(
            name=os.path.basename(os.path.dirname(path)) or "llama", arch="llama",
            vocab_size=c["vocab_size"], hidden=c["hidden_size"],
            n_layers=c["num_hidden_layers"], n_heads=c["num_attention_heads"],
            n_kv_heads=c.get("num_key_value_heads", c["num_attention_heads"]),
            ffn=c["intermediate_size"], max_positions=c.get("max_position_embeddings", 8192),
            norm_eps=c.get("rms_norm_eps", 1e-5),
            tie_embeddings=c.get("tie_word_embeddings", False),
            rope_theta=c.get("rope_theta", 10000.0),
            bos_token_id=c.get("bos_token_id", 1), eos_token_id=eos)
    raise ValueError(f"unsupported model_type {mt!r} in {path}")


# ---------------------------------------------------------------------------
# Sampling
# ---------------------------------------------------------------------------

MAX_SAMPLES_CEILING = 64  # samples of one request (SamplingParams.n): one family, admitted as a unit
MAX_LOGPROBS_CEILING = 20  # alternatives per token the logprob kernel's record can hold
MAX_LOGIT_EDITS_CEILING = 1024  # entries per request the logit-edit kernel's 256 threads visit in 4 trips
MAX_BAD_WORDS_CEILING = 256  # sequences per request: one thread of the bad_words kernel's workgroup each
MAX_BAD_WORD_TOKENS_CEILING = 4096  # tokens of a request's bad_words in all
MAX_STOP_SEQUENCES_CEILING = 64  # stop sequences per request (stop_token_ids and stop_sequences together)
MAX_STOP_LEN = 32  # tokens of one stop sequence: the scheduler core keeps a request's last 32 tokens to match
MAX_GUIDES_CEILING = 64  # rows of the last stage's guide table: guides in flight at once
MAX_GUIDE_CLASSES_CEILING = 4096  # token classes of one guide: the mask kernel's LDS flags, one byte each
MAX_GUIDE_CELLS_CEILING = 1 << 20  # states x classes of one guide
MAX_BAD_WORD_LEN = 32  # tokens of one sequence: its prefix fits the kernel's 31-token context tail
INT32_MAX = 2 ** 31 - 1


def _fp32(v) -> float:
    import struct

    return struct.unpack("f", struct.pack("f", float(v)))[0]


def _token_id(t) -> int:
    """A token id given as an int or, as JSON object keys arrive, a decimal string."""
    try:
        if isinstance(t, str) and t.strip().lstrip("+-").isdecimal():
            return int(t)
        if not isinstance(t, (bool, str)):
            return operator.index(t)
    except (TypeError, ValueError):
        pass
    raise ValueError(f"token ids must be integers (or decimal strings), got {t!r}")


def _strict_id(t) -> int:
    """A token id given as an integer (no bool, no string, no float)."""
    try:
        if not isinstance(t, (bool, str, bytes, float)):
            return operator.index(t)
    except TypeError:
        pass
    raise ValueError(f"token ids must be integers, got {t!r}")


@dataclass
class SamplingParams:
    """Per-request sampling.  Defaults reproduce `server.py:187-205`.

    top_p / min_p cut the sorted top-k candidates before the draw: min_p keeps
    the tokens at least min_p times as likely as the most likely one, top_p the
    shortest prefix holding top_p of the top-k-renormalised mass (at least one
    token stays).  They work inside the top-k candidates and top_k is capped at
    1024, so pure nucleus sampling is top_k=1024 with top_p.  The defaults
    (1.0 / 0.0) disable both; greedy requests ignore them.

    presence_penalty / frequency_penalty act on the tokens the request has
    generated so far (the prompt does not count; OpenAI / vLLM rule): before
    each draw every token t generated c(t) > 0 times gets
    logit[t] -= presence_penalty + frequency_penalty * c(t), on the raw logits,
    ahead of temperature, top-k, top-p, min-p and the greedy argmax -- greedy
    requests are penalised too.  Both default to 0.0 (off) and must be finite
    and in [-2, 2]; negative values raise the logits of repeated tokens.

    logprobs: None (off; nothing changes for the request) or n in
    [0, EngineConfig.max_logprobs]: every generated token, the prefill draw
    included, comes back with its logprob and with the n most likely tokens and
    theirs (Request.logprobs).  Logprobs are the log-softmax over the whole
    vocabulary of the fp32 logits the sampler drew from: after the presence /
    frequency penalties, at temperature 1, before the top-k / top-p / min-p
    cuts -- for an unpenalised request the model's own distribution.  The
    alternatives come most likely first, equal logits (-0.0 == +0.0) by
    ascending token id; when the drawn token is among them its logprob is
    bit-equal to that entry's; a -inf logit has logprob -inf; a vocabulary of
    fewer than n tokens pads with id -1 and -inf (trimmed from
    Request.logprobs).  Asking never changes a draw: the same seed gives the
    same tokens with and without.

    logit_bias / banned_token_ids / min_new_tokens edit the row's fp32 logits
    before every draw: each entry is logit[t] <- logit[t] + v, one rounding per
    addition, applied after the presence / frequency penalties and ahead of
    temperature, top-k, top-p, min-p and the greedy argmax -- greedy requests
    are edited too.  logit_bias maps token ids (ints, or decimal strings as
    JSON gives them) to finite values in [-100, 100]; banned_token_ids can
    never be drawn (v = -inf; duplicates collapse; a token both biased and
    banned is banned); min_new_tokens = m keeps the model's EOS token from
    being drawn in the first m draws (the prefill draw is draw 0; 0 <= m <=
    max_new_tokens), whether or not stop_at_eos is set: the entry (eos, -inf)
    holds while the draw's sampler counter is below m, every other entry for
    good.  A request's entries -- the distinct tokens of logit_bias and
    banned_token_ids, plus one with min_new_tokens > 0 -- number at most
    EngineConfig.max_logit_edits; the ids must lie in the vocabulary and some
    token must stay drawable.  All three default to off (None / None / 0), and
    such a request runs nothing extra.  Logprobs are taken after the edits (a
    banned token has logprob -inf), and asking for edits never changes
    another request's draws.

    repetition_penalty / no_repeat_ngram_size are the two HF generate() rules
    that read the prompt: before each draw the request's context is its prompt
    followed by the tokens it has generated so far.  repetition_penalty = r
    rewrites the logit of every distinct context token once, logit * r when it
    is negative and logit / r otherwise (one fp32 rounding; r is used as
    rounded to fp32; r > 1 discourages repeats, r < 1 encourages them);
    no_repeat_ngram_size = G then sets to -inf every token that would complete
    a G-gram already in the context (G = 1: every context token).  Both run on
    the raw logits ahead of the presence / frequency penalties, the logit
    edits, temperature, top-k, top-p, min-p and the greedy argmax -- greedy
    requests get them too -- and logprobs are taken after them.
    repetition_penalty is finite and in (0, 10], no_repeat_ngram_size an
    integer in [0, 32]; with an n-gram ban the engine wants prompt +
    max_new_tokens + banned tokens below the vocabulary size, so that some
    token always stays drawable.  The defaults (1.0 / 0) are off: such a
    request runs nothing extra and its prompt never reaches the last stage.
    Asking never changes another request's draws.

    allowed_token_ids: None (off; nothing runs, travels or is allocated for
    the request) or a non-empty list of token ids of the vocabulary: before
    every draw, the prefill draw (draw 0) included, every token of the
    vocabulary that is not in the list has its fp32 logit set to -inf.  The
    mask is the last edit of the logits: after the repetition pass, the
    presence / frequency penalties and the logit edits, ahead of temperature,
    top-k, top-p, min-p and the greedy argmax -- greedy requests are masked
    too.  Duplicates collapse.  top_k may exceed the number of allowed tokens:
    a -inf candidate has probability 0 and is never drawn.  Logprobs are taken
    after the mask: a disallowed token has logprob -inf, the log-sum-exp runs
    over what is left, and alternatives past the allowed set come back as
    -inf.  Some allowed token must stay drawable after the request's own bans
    (banned_token_ids, and the EOS of min_new_tokens > 0); with an n-gram ban
    the engine wants prompt + max_new_tokens below the number of allowed
    tokens that are not banned.  The list travels as a bitmask over the
    vocabulary, so its length costs nothing.  Asking never changes another
    request's draws.

    bad_words: None (off; nothing runs, travels or is allocated for the
    request) or a list of non-empty token-id sequences that may never be
    completed (HF bad_words_ids, vLLM bad_words).  Before every draw, the
    prefill draw (draw 0) included, the request's context is its prompt
    followed by the tokens it has generated so far -- the context
    no_repeat_ngram_size reads -- and every sequence whose tokens but the last
    the context ends with has its last token's fp32 logit set to -inf; a
    sequence of one token is a plain ban.  The pass runs right after the
    repetition pass, ahead of the presence / frequency penalties, the logit
    edits, the allowed-token mask, temperature, top-k, top-p, min-p and the
    greedy argmax -- greedy requests are banned too -- and logprobs are taken
    after it.  Bans are pure stores of -inf, so they commute with every other
    edit.  Exact duplicates collapse.  A request carries at most
    EngineConfig.max_bad_words sequences of 1 to 32 tokens each and
    EngineConfig.max_bad_word_tokens tokens in all; the ids must lie in the
    vocabulary, and some token must stay drawable: the vocabulary (or the
    allowed set) minus the request's own bans minus the distinct last tokens
    must be positive, with an n-gram ban also minus prompt + max_new_tokens.
    Such a request's prompt reaches the last stage, as with
    no_repeat_ngram_size.  Asking never changes another request's draws.

    stop_token_ids / stop_sequences / include_stop_in_output end a request
    when its output completes a token sequence; the sampler is not involved
    and the draws do not change.  stop_token_ids are token ids (duplicates
    collapse), each a stop sequence of one token; stop_sequences are non-empty
    token-id sequences.  After the request's j-th generated token is read back
    (the prefill draw is token 1) the sequences are tried in order --
    stop_token_ids ascending, then stop_sequences as given -- and one matches
    when it equals the last len generated tokens: the prompt never takes part.
    A match counts only when j > min_new_tokens, the draw from which EOS itself
    may appear; the first counting match ends the request as a read-back EOS
    does (stop_at_eos is checked first): it leaves at the next step and its
    KV slot is released.  Request.output drops the matched tokens unless
    include_stop_in_output is set, Request.logprobs is trimmed to the same
    length, Request.finish_reason is "stop" and Request.stop_reason the index
    of the matched sequence in the order above (else "length" or "eos", and
    None).  A request carries at most EngineConfig.max_stop_sequences
    sequences of 1 to 32 tokens; the ids must lie in the vocabulary.  The
    defaults (None / None / False) are off: such a request takes the path it
    always took.

    guide: None (off; nothing runs, travels or is allocated for the request)
    or a guide.TokenGuide, a deterministic automaton over tokens
    (guide.compile_regex / compile_choice build one from a regular expression
    or a list of strings): the request starts in state 0, and before every
    draw, the prefill draw (draw 0) included, every token t of the vocabulary
    with next[state, cls[t]] < 0 has its fp32 logit set to -inf; behind the
    draw the state becomes next[state, cls[drawn token]].  The state lives on
    the last stage and advances inside the captured decode graphs: the host
    never reads it.  The mask is the last edit of the logits: after the
    repetition pass, the bad-words pass, the presence / frequency penalties,
    the logit edits and the allowed-token mask, ahead of temperature, top-k,
    top-p, min-p and the greedy argmax -- greedy requests are guided too.
    Logprobs are taken after it: a token the guide forbids has logprob -inf.
    EOS is an ordinary token of the guide; a compiled guide allows it exactly
    where the match is complete, so with stop_at_eos the output matches the
    pattern as a whole, and without an EOS (or when max_new_tokens ends the
    request first) it is a prefix of a match.  A guide has at most
    EngineConfig.max_guide_classes token classes and max_guide_cells = states
    x classes cells, its vocab must be the model's and its eos the model's or
    None, and every state reachable from the start must keep a token to draw.
    No static check shows that a token stays drawable beside another field
    that can itself produce -inf, so a guide is refused together with
    banned_token_ids, allowed_token_ids, bad_words, no_repeat_ngram_size and
    min_new_tokens > 0; it combines with temperature, top-k, top-p, min-p, the
    presence / frequency penalties, repetition_penalty, finite logit_bias,
    logprobs and the stop sequences.  Equal guides (TokenGuide.digest) share
    one of the EngineConfig.max_guides rows of the last stage's table (G rows
    of the classes of the padded vocabulary's Vp columns and of
    max_guide_cells cells, and a (row, state) pair per KV slot: G x (2 Vp +
    2 max_guide_cells + 8) + 8 x slots bytes, allocated when the first guided
    request arrives); a row is pinned from submit until the request's KV slot
    is released, a new guide takes a free row or the least recently used
    unpinned one, and a request whose guide finds none is refused.  A row's
    contents are never rewritten while an enqueued or in-flight kernel can
    read them: the pin goes back once the tokens of the last item that held
    one of the request's rows have been read back, and the state's step is
    enqueued ahead of that token return.  Asking never changes another
    request's draws."""

    temperature: float = 0.6
    top_k: int = 40
    greedy: bool = False
    seed: Optional[int] = None
    max_new_tokens: int = 20
    stop_at_eos: bool = False  # reference never stops early (quirk Q10)
    top_p: float = 1.0
    min_p: float = 0.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    logprobs: Optional[int] = None
    logit_bias: Optional[Mapping[int, float]] = None
    banned_token_ids: Optional[Sequence[int]] = None
    min_new_tokens: int = 0
    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    allowed_token_ids: Optional[Sequence[int]] = None
    bad_words: Optional[Sequence[Sequence[int]]] = None
    stop_token_ids: Optional[Sequence[int]] = None
    stop_sequences: Optional[Sequence[Sequence[int]]] = None
    include_stop_in_output: bool = False
    guide: Optional["TokenGuide"] = None
    # n samples of the prompt, each a sequence of its own: sample i draws with
    # seed + i (of the one random seed the scheduler draws when seed is None)
    # and every other field applies to each sample independently.  The prompt
    # is prefilled once; samples 1 .. n - 1 start from a copy of its KV
    # (csrc/kernels/kv_fork.hip).  At most EngineConfig.max_samples, the
    # microbatch capacity and the KV slot count.  greedy gives n equal samples
    n: int = 1
    # The per-request opt-out of the engine's prefix cache
    # (EngineConfig.prefix_cache): False and the request neither starts from a
    # cached prompt's KV nor leaves its own behind, so its tokens are exactly
    # those of an engine without the cache.  Nothing while the cache is off.
    # A request that reads its prompt on the last stage (repetition_penalty,
    # no_repeat_ngram_size, bad_words) never starts from an entry -- the
    # entry's prompt ids are not kept there -- but still leaves one
    prefix_cache: bool = True

    @property
    def has_stops(self) -> bool:
        return bool(self.stop_token_ids) or bool(self.stop_sequences)

    def stop_list(self) -> list:
        """The request's stop sequences as tuples of ints in the order they
        are tried: stop_token_ids ascending (duplicates collapsed), then
        stop_sequences as given (empty without any)."""
        out = []
        for name in ("stop_token_ids", "stop_sequences"):
            v = getattr(self, name)
            if v is not None and (isinstance(v, (str, bytes, Mapping)) or not hasattr(v, "__iter__")):
                raise ValueError(f"{name} must be a sequence")
        if self.stop_token_ids is not None:
            out += [(t,) for t in sorted({_strict_id(t) for t in self.stop_token_ids})]
        for w in self.stop_sequences or ():
            if isinstance(w, (str, bytes, Mapping)) or not hasattr(w, "__iter__"):
                raise ValueError("stop_sequences must be a sequence of token-id sequences")
            out.append(tuple(_strict_id(t) for t in w))
        return out

    def stop_match(self, generated: Sequence[int], stops: Optional[list] = None) -> Optional[int]:
        """The index in stop_list() of the first stop sequence that the
        generated tokens end with, when the match counts (more tokens than
        min_new_tokens); None otherwise."""
        n = len(generated)
        if n <= self.min_new_tokens:
            return None
        for i, w in enumerate(self.stop_list() if stops is None else stops):
            if len(w) <= n and tuple(generated[n - len(w):]) == tuple(w):
                return i
        return None

    def bad_word_list(self) -> list:
        """The distinct bad_words sequences as tuples of ints, in the order
        given (empty without any)."""
        if self.bad_words is None:
            return []
        bw = self.bad_words
        if isinstance(bw, (str, bytes, Mapping)) or not hasattr(bw, "__iter__"):
            raise ValueError("bad_words must be a sequence of token-id sequences")
        out = {}
        for w in bw:
            if isinstance(w, (str, bytes, Mapping)) or not hasattr(w, "__iter__"):
                raise ValueError("bad_words must be a sequence of token-id sequences")
            out[tuple(_strict_id(t) for t in w)] = None
        return list(out)

    def bad_word_entries(self) -> Optional[tuple]:
        """The request's bad_words as the last stage's table row holds them:
        (exclusive end offsets, the sequences' tokens back to back), or None
        without any."""
        ws = self.bad_word_list()
        if not ws:
            return None
        import itertools

        return tuple(itertools.accumulate(map(len, ws))), tuple(t for w in ws for t in w)

    def allowed_set(self) -> Optional[frozenset]:
        """The distinct allowed token ids, or None without a list."""
        if self.allowed_token_ids is None:
            return None
        return frozenset(_strict_id(t) for t in self.allowed_token_ids)

    def allowed_mask(self, words: int):
        """The allowed list as the packed words of the last stage's mask
        table: int32 numpy [words], bit t & 31 of word t >> 5 set for every
        allowed t (ids at or past 32 * words are an error), or None."""
        if self.allowed_token_ids is None:
            return None
        import numpy as np

        t = np.array(sorted(self.allowed_set()), dtype=np.int64)
        if t.size and (t[0] < 0 or t[-1] >= 32 * words):
            raise ValueError(f"allowed_token_ids must lie in [0, {32 * words})")
        w = np.zeros(words, dtype=np.uint32)
        np.bitwise_or.at(w, t >> 5, np.uint32(1) << (t & 31).astype(np.uint32))
        return w.view(np.int32)

    @property
    def has_context(self) -> bool:
        """repetition_penalty (as the fp32 the kernel multiplies by) or
        no_repeat_ngram_size is on: the last stage keeps the request's prompt."""
        return self.context_knobs() != (1.0, 0)

    def context_knobs(self) -> tuple:
        """(repetition_penalty rounded to fp32, no_repeat_ngram_size)."""
        return _fp32(self.repetition_penalty), int(self.no_repeat_ngram_size)

    @property
    def has_logit_edits(self) -> bool:
        return bool(self.logit_bias) or bool(self.banned_token_ids) or self.min_new_tokens != 0

    def logit_edits(self, eos: int) -> Optional[tuple]:
        """The request's edit entries as (tokens, values, untils), sorted by
        token (a token's permanent entry ahead of the min_new_tokens one), or
        None without any: what the last stage's table holds for its KV slot.
        Values are rounded to fp32 here; a ban is -inf, `until` INT32_MAX for
        a permanent entry and min_new_tokens for the EOS one."""
        if not self.has_logit_edits:
            return None
        ent = {}
        for t, v in (self.logit_bias or {}).items():
            t = _token_id(t)
            if t in ent:
                raise ValueError(f"logit_bias names token {t} twice")
            ent[t] = _fp32(v)
        for t in self.banned_token_ids or ():
            ent[_token_id(t)] = -math.inf
        rows = [(t, v, INT32_MAX) for t, v in ent.items()]
        if self.min_new_tokens > 0:
            rows.append((int(eos), -math.inf, int(self.min_new_tokens)))
        rows.sort(key=lambda r: (r[0], -r[2]))
        return tuple(zip(*rows)) if rows else None

    def validate(self, max_logprobs: int = MAX_LOGPROBS_CEILING, max_logit_edits: int = 300,
                 max_bad_words: int = 64, max_bad_word_tokens: int = 512, max_stop_sequences: int = 16,
                 max_guide_classes: int = 1024, max_guide_cells: int = 1 << 18) -> None:
        if self.max_new_tokens < 0:
            raise ValueError("max_new_tokens must be >= 0")
        if isinstance(self.n, bool) or not isinstance(self.n, int) or self.n < 1:
            raise ValueError("n must be an integer >= 1")
        m = self.min_new_tokens
        if isinstance(m, bool) or not isinstance(m, int) or not (0 <= m <= self.max_new_tokens):
            raise ValueError("min_new_tokens must be an integer in [0, max_new_tokens]")
        r, G = self.repetition_penalty, self.no_repeat_ngram_size
        if isinstance(r, bool) or not isinstance(r, (int, float)) or not math.isfinite(r) or not 0.0 < r <= 10.0:
            raise ValueError("repetition_penalty must be finite and in (0, 10]")
        if _fp32(r) == 0.0:
            raise ValueError("repetition_penalty must be finite and in (0, 10] as a float32")
        if isinstance(G, bool) or not isinstance(G, int) or not 0 <= G <= 32:
            raise ValueError("no_repeat_ngram_size must be an integer in [0, 32]")
        if self.allowed_token_ids is not None:
            a = self.allowed_token_ids
            if isinstance(a, (str, bytes, Mapping)) or not hasattr(a, "__iter__"):
                raise ValueError("allowed_token_ids must be a sequence of token ids")
            ids = self.allowed_set()
            if not ids:
                raise ValueError("allowed_token_ids must not be empty (None turns the mask off)")
            if any(t < 0 or t > INT32_MAX for t in ids):
                raise ValueError("allowed_token_ids must be >= 0")
        if self.guide is not None:
            from .guide import TokenGuide

            if not isinstance(self.guide, TokenGuide):
                raise ValueError("guide must be None or a TokenGuide")
            self.guide.validate(max_classes=max_guide_classes, max_cells=max_guide_cells)
            clash = [name for name, on in (("banned_token_ids", bool(self.banned_token_ids)),
                                           ("allowed_token_ids", self.allowed_token_ids is not None),
                                           ("bad_words", bool(self.bad_words)),
                                           ("no_repeat_ngram_size", G != 0),
                                           ("min_new_tokens", m > 0)) if on]
            if clash:
                raise ValueError(f"guide cannot be combined with {', '.join(clash)}: each can set logits to -inf "
                                 "itself, and no static check shows that a token stays drawable in every state")
        if not isinstance(self.include_stop_in_output, bool):
            raise ValueError("include_stop_in_output must be a bool")
        if not isinstance(self.prefix_cache, bool):
            raise ValueError("prefix_cache must be a bool")
        if self.stop_token_ids is not None or self.stop_sequences is not None:
            st = self.stop_list()
            if any(not 1 <= len(w) <= MAX_STOP_LEN for w in st):
                raise ValueError(f"stop_sequences: every sequence must hold 1 to {MAX_STOP_LEN} tokens")
            if any(t < 0 or t > INT32_MAX for w in st for t in w):
                raise ValueError("stop_token_ids / stop_sequences: token ids must be >= 0")
            if len(st) > max_stop_sequences:
                raise ValueError(f"stop_token_ids and stop_sequences make {len(st)} sequences; at most "
                                 f"{max_stop_sequences} (max_stop_sequences)")
        if self.bad_words is not None:
            ws = self.bad_word_list()
            if any(not 1 <= len(w) <= MAX_BAD_WORD_LEN for w in ws):
                raise ValueError(f"bad_words: every sequence must hold 1 to {MAX_BAD_WORD_LEN} tokens")
            if any(t < 0 or t > INT32_MAX for w in ws for t in w):
                raise ValueError("bad_words: token ids must be >= 0")
            if len(ws) > max_bad_words:
                raise ValueError(f"bad_words: {len(ws)} sequences; at most {max_bad_words} (max_bad_words)")
            if sum(map(len, ws)) > max_bad_word_tokens:
                raise ValueError(f"bad_words: {sum(map(len, ws))} tokens in all; at most {max_bad_word_tokens} "
                                 "(max_bad_word_tokens)")
        if self.logit_bias is not None or self.banned_token_ids is not None:
            if self.logit_bias is not None and not isinstance(self.logit_bias, Mapping):
                raise ValueError("logit_bias must map token ids to values")
            if isinstance(self.banned_token_ids, (str, bytes, Mapping)):
                raise ValueError("banned_token_ids must be a sequence of token ids")
            for v in (self.logit_bias or {}).values():
                if (isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v)
                        or not -100.0 <= v <= 100.0):
                    raise ValueError("logit_bias values must be finite and in [-100, 100]")
            try:
                toks = set(map(_token_id, self.logit_bias or ())) | set(map(_token_id, self.banned_token_ids or ()))
            except TypeError:
                raise ValueError("banned_token_ids must be a sequence of token ids") from None
            if len(toks) < len(self.logit_bias or ()):
                raise ValueError("logit_bias names a token twice")
            if any(t < 0 or t > INT32_MAX for t in toks):
                raise ValueError("token ids must be >= 0")
            if len(toks) + (m > 0) > max_logit_edits:
                raise ValueError(f"logit_bias, banned_token_ids and min_new_tokens make {len(toks) + (m > 0)} "
                                 f"entries; at most {max_logit_edits} (max_logit_edits)")
        if self.logprobs is not None:
            n = self.logprobs
            if isinstance(n, bool) or not isinstance(n, int) or not (0 <= n <= max_logprobs):
                raise ValueError(f"logprobs must be None or an integer in [0, {max_logprobs}] (max_logprobs)")
        for name in ("presence_penalty", "frequency_penalty"):  # greedy requests too
            v = getattr(self, name)
            if not (isinstance(v, (int, float)) and math.isfinite(v) and -2.0 <= v <= 2.0):
                raise ValueError(f"{name} must be finite and in [-2, 2]")
        if not self.greedy:
            if self.temperature <= 0:
                raise ValueError("temperature must be > 0 (use greedy=True for argmax)")
            if not (1 <= self.top_k <= 1024):
                raise ValueError("top_k must be in [1, 1024]")
            if not (0 < self.top_p <= 1):
                raise ValueError("top_p must be in (0, 1]")
            if not (0 <= self.min_p <= 1):
                raise ValueError("min_p must be in [0, 1]")


# ---------------------------------------------------------------------------
# Engine config
# ---------------------------------------------------------------------------

def _env(name: str, default: str) -> str:
    return os.environ.get(name, default)


@dataclass
class EngineConfig:
    model_id: str = "sshleifer/tiny-gpt2"
    # Pipeline: number of stages (= GPUs, one rank per GPU) and the layer split.
    num_stages: int = 1
    # Data parallelism over whole pipelines: world = num_stages x dp_replicas
    # ranks; replica r owns ranks [r*P, (r+1)*P).  Requests are spread over
    # the replicas (SURVEY.md §2.2 "DP -- request-level replicas").
    dp_replicas: int = 1
    # Explicit split points (len num_stages-1), e.g. SPLIT_AT=2 -> [2].  None = cost model.
    split_points: Optional[Sequence[int]] = None
    # Explicit split points in half-layer units: a stage starts at unit u, where
    # u = 2i is layer i's attention half and u = 2i + 1 its MLP half, e.g.
    # [13] cuts layer 6 between attention and MLP.
    split_units: Optional[Sequence[int]] = None
    # Auto partition may cut between a layer's attention and MLP halves
    # (finer balance of the last stage's lm_head + sampler).
    half_layer_split: bool = True
    dtype: str = "bf16"  # compute / storage dtype on GPU; CPU golden runs in fp32
    device: str = "auto"  # "auto" -> cuda if available else cpu
    max_batch: int = 64  # max concurrent sequences (KV slots)
    max_seq_len: int = 1024
    num_microbatches: int = 0  # 0 -> num_stages (1 when single stage)
    use_graphs: bool = True  # hipGraph-capture decode steps
    seed: int = 0
    weights: Optional[str] = None  # safetensors / HF dir; None -> random init
    sampling: SamplingParams = field(default_factory=SamplingParams)
    # Compat roles (reference server.py:21): "coordinator" | "a" | "b" | "engine".
    role: str = "coordinator"
    shard_a_service: str = "llm-shard-a"
    shard_b_service: str = "llm-shard-b"
    shard_port: int = 5000
    # auto | nccl | rccl | gloo | local | http | loopback (P stage threads on
    # one GPU, device-async event hand-off) | devloop (P stage threads on one
    # GPU joined by device loopback channels with graph-captured transfers:
    # the single-GPU rehearsal of the rccl data plane) | strict (host queues
    # per (edge, lane) with receive-size checks: CPU protocol tests)
    transport: str = "auto"
    # Boundary hidden states on the wire: "fp32" (the residual stream as is:
    # bit-identical to one stage) or "bf16" (half the bytes per hop; the
    # stream is rounded to bf16 at each stage boundary).  The reference ships
    # them as JSON floats (server.py:140,148).
    wire_dtype: str = "fp32"
    # Serving (runtime/scheduler.py): concurrent /generate requests arriving
    # within batch_window_ms share one pipeline round; a round running longer
    # than round_timeout_s marks the engine unhealthy; an HTTP request waits at
    # most request_timeout_s.
    batch_window_ms: float = 2.0
    # Chunked prefill: prompts are prefilled in steps of at most this many
    # tokens per sequence (0 = whole prompt in one step).  Bounds prefill
    # activation memory for long contexts and lets chunks of different
    # microbatches pipeline across stages.
    prefill_chunk: int = 0
    round_timeout_s: float = 600.0
    request_timeout_s: float = 900.0
    # Prefill tokens per microbatch group per step when requests join a
    # running batch (0 = unlimited: every waiting prompt joins at once).
    prefill_budget: int = 0
    # Join policy (runtime/sched_core.h set_join_policy): a running group
    # admits waiting requests only when it has room for all of them or for
    # join_min of them, when idle, or after deferring join_max_wait steps --
    # larger, rarer prefill items (1: admit whatever fits at every step).  Closed-loop serving, 512
    # in flight (profiles/r6_join_policy.log), 1 -> 32 / 4: GPT-2 XL 37.4-38.2k
    # -> 41.4k tok/s, GPT-2 small 156-164k -> 209k, Llama-3 8B 20.1k -> 21.6k,
    # TTFT p50 lower, p90 unchanged.
    join_min: int = 32
    join_max_wait: int = 4
    # One stage: a step's prefill items of groups that all only join
    # sequences run as one forward (parallel/pipeline.py _merged_prefill).
    # Off for references that must match a multi-stage pipeline bit for bit
    # (other GEMM row counts round differently).
    merge_prefill: bool = True
    # Fraction of the HBM left after the weights that the KV cache may use.
    kv_fraction: float = 0.85
    # Serving: record per-stage busy / bubble timing on one pipeline session
    # in this many (0 = never) -- it costs a control-plane gather per session.
    metrics_every: int = 16
    # Most alternatives a request may ask for per token (SamplingParams.logprobs);
    # sizes the last stage's logprob records, slots x max_seq x (4 + 8 W) bytes,
    # allocated when the first such request arrives.  At most 20.
    max_logprobs: int = 5
    # Most logit-edit entries a request may carry (SamplingParams.logit_bias,
    # banned_token_ids, min_new_tokens); sizes the last stage's edit table,
    # slots x (4 + 12 E) bytes, allocated when the first such request arrives.
    # At most 1024.
    max_logit_edits: int = 300
    # Most bad_words sequences a request may carry and most tokens they hold in
    # all (SamplingParams.bad_words); size the last stage's bad-words table,
    # slots x (4 + 4 N + 4 T) bytes, allocated when the first such request
    # arrives.  At most 256 and 4096.
    max_bad_words: int = 64
    max_bad_word_tokens: int = 512
    # Most stop sequences a request may carry (SamplingParams.stop_token_ids and
    # stop_sequences together); the scheduler core tries them at every token of
    # such a request.  At most 64.
    max_stop_sequences: int = 16
    # Guided decoding (SamplingParams.guide): the distinct guides in flight at
    # once, and the most token classes and states x classes cells one may have;
    # size the last stage's guide table, G x (2 Vp + 2 max_guide_cells + 8) +
    # 8 x slots bytes, allocated when the first such request arrives.  At most
    # 64, 4096 and 1 << 20.
    max_guides: int = 8
    max_guide_classes: int = 1024
    max_guide_cells: int = 1 << 18
    # Most samples one request may ask for (SamplingParams.n); a request's
    # samples are admitted together, so n is also bounded by the microbatch
    # capacity and the KV slot count.  At most 64.
    max_samples: int = 8
    # Prefix cache (runtime/sched_core.h set_prefix_cache): a finished
    # request's KV slot stays behind as an entry keyed by its prompt, at most
    # this many per replica (0 = off), and a later prompt that shares at least
    # prefix_cache_min_tokens leading tokens with one starts its prefill
    # behind a copy of them (csrc/kernels/kv_fork.hip).  Entries are slots of
    # the replica's pool: they go back to it, least recently used first, when
    # an admission needs them.  8: a lone hit's first token on GPT-2 XL was no
    # later than the miss's from 8 reused tokens on (tools/prefix_cache_ab.py
    # --cases lone, profiles/prefix_cache_ab.log), by less than the runs' spread.
    prefix_cache: int = 0
    prefix_cache_min_tokens: int = 8

    def __post_init__(self):
        if not (0 <= self.prefix_cache <= self.max_batch):
            raise ValueError("prefix_cache must be in [0, max_batch]: an entry is one of the replica's KV slots")
        if self.prefix_cache_min_tokens < 1:
            raise ValueError("prefix_cache_min_tokens must be at least 1")
        if not (1 <= self.max_samples <= MAX_SAMPLES_CEILING):
            raise ValueError(f"max_samples must be in [1, {MAX_SAMPLES_CEILING}]")
        if not (1 <= self.max_guides <= MAX_GUIDES_CEILING):
            raise ValueError(f"max_guides must be in [1, {MAX_GUIDES_CEILING}]")
        if not (1 <= self.max_guide_classes <= MAX_GUIDE_CLASSES_CEILING):
            raise ValueError(f"max_guide_classes must be in [1, {MAX_GUIDE_CLASSES_CEILING}]")
        if not (1 <= self.max_guide_cells <= MAX_GUIDE_CELLS_CEILING):
            raise ValueError(f"max_guide_cells must be in [1, {MAX_GUIDE_CELLS_CEILING}]")
        if not (1 <= self.max_stop_sequences <= MAX_STOP_SEQUENCES_CEILING):
            raise ValueError(f"max_stop_sequences must be in [1, {MAX_STOP_SEQUENCES_CEILING}]")
        if not (1 <= self.max_bad_words <= MAX_BAD_WORDS_CEILING):
            raise ValueError(f"max_bad_words must be in [1, {MAX_BAD_WORDS_CEILING}]")
        if not (1 <= self.max_bad_word_tokens <= MAX_BAD_WORD_TOKENS_CEILING):
            raise ValueError(f"max_bad_word_tokens must be in [1, {MAX_BAD_WORD_TOKENS_CEILING}]")
        if not (0 <= self.max_logprobs <= MAX_LOGPROBS_CEILING):
            raise ValueError(f"max_logprobs must be in [0, {MAX_LOGPROBS_CEILING}]")
        if not (1 <= self.max_logit_edits <= MAX_LOGIT_EDITS_CEILING):
            raise ValueError(f"max_logit_edits must be in [1, {MAX_LOGIT_EDITS_CEILING}]")

    @property
    def model(self) -> ModelConfig:
        return get_model_config(self.model_id)

    @classmethod
    def from_env(cls, **overrides) -> "EngineConfig":
        """Build from the reference's env vars (server.py:20-25) plus extras."""
        split = _env("SPLIT_AT", "")
        cfg = cls(
            model_id=_env("MODEL_ID", "sshleifer/tiny-gpt2"),
            role=_env("SHARD_ROLE", "coordinator").lower(),
            split_points=[int(s) for s in split.split(",") if s.strip()] or None,
            shard_a_service=_env("SHARD_A_SERVICE", "llm-shard-a"),
            shard_b_service=_env("SHARD_B_SERVICE", "llm-shard-b"),
            shard_port=int(_env("SHARD_PORT", "5000")),
            num_stages=int(_env("NUM_STAGES", "0") or 0) or 1,
            max_batch=int(_env("MAX_BATCH", "64")),
            max_seq_len=int(_env("MAX_SEQ_LEN", "1024")),
            dtype=_env("DTYPE", "bf16"),
            weights=os.environ.get("WEIGHTS") or None,
            transport=_env("TRANSPORT", "auto"),
            wire_dtype=_env("WIRE_DTYPE", "fp32"),
            dp_replicas=int(_env("DP_REPLICAS", "1") or 1),
            batch_window_ms=float(_env("BATCH_WINDOW_MS", "2.0")),
            prefill_chunk=int(_env("PREFILL_CHUNK", "0")),
            round_timeout_s=float(_env("ROUND_TIMEOUT_S", "600")),
            request_timeout_s=float(_env("REQUEST_TIMEOUT_S", "900")),
            prefill_budget=int(_env("PREFILL_BUDGET", "0")),
            join_min=int(_env("JOIN_MIN", "32")),
            join_max_wait=int(_env("JOIN_MAX_WAIT", "4")),
            kv_fraction=float(_env("KV_FRACTION", "0.85")),
            metrics_every=int(_env("METRICS_EVERY", "16")),
            max_logprobs=int(_env("MAX_LOGPROBS", "5")),
            max_logit_edits=int(_env("MAX_LOGIT_EDITS", "300")),
            max_bad_words=int(_env("MAX_BAD_WORDS", "64")),
            max_bad_word_tokens=int(_env("MAX_BAD_WORD_TOKENS", "512")),
            max_stop_sequences=int(_env("MAX_STOP_SEQUENCES", "16")),
            max_guides=int(_env("MAX_GUIDES", "8")),
            max_guide_classes=int(_env("MAX_GUIDE_CLASSES", "1024")),
            max_guide_cells=int(_env("MAX_GUIDE_CELLS", str(1 << 18))),
            max_samples=int(_env("MAX_SAMPLES", "8")),
            prefix_cache=int(_env("PREFIX_CACHE", "0")),
            prefix_cache_min_tokens=int(_env("PREFIX_CACHE_MIN_TOKENS", "8")),
        )
        if cfg.split_points and cfg.num_stages == 1:
            cfg.num_stages = len(cfg.split_points) + 1
        for k, v in overrides.items():
            if not hasattr(cfg, k):
                raise AttributeError(f"EngineConfig has no field {k!r}")
            setattr(cfg, k, v)
        return cfg

    def replace(self, **kw) -> "EngineConfig":
        return dataclasses.replace(self, **kw)

    @property
    def microbatches(self) -> int:
        return self.num_microbatches or self.num_stages
