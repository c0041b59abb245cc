"""Per-step execution plans: iteration-level (continuous) batching.

The reference serves every /generate independently in FastAPI's threadpool
(`/root/reference/server.py:154-155`): a short request never waits behind a
long one, but nothing is batched either.  Here the engine keeps M microbatch
*groups* permanently in flight through the pipeline and re-decides their
composition at every decode step:

  * a sequence LEAVES its group as soon as it has its tokens (max_new_tokens,
    or EOS seen), freeing its row and KV slot for the next request;
  * a new request JOINS at the next step boundary: its prompt is prefilled
    (in chunks if PREFILL_CHUNK is set) by the group's item of that step,
    the final chunk's last position is sampled, and from the step after it
    the sequence is a decode row like any other.

A group's decode rows are compacted into rows [0, n) and run as a padded
bucket of b >= n rows (b a power of two, at most the group capacity): the
pad rows point at a scratch KV slot and are masked out of the position /
sampler advance, so one captured hipGraph per (group, b, context bucket) is
replayed for as long as the shapes stay put -- across steps and requests.

Stage 0's scheduler decides a `StepPlan` per step and every other stage
executes the same plan (in-process queue, or the gloo control plane in dist
mode), so all stages agree on shapes without any device->host sync.
"""
from __future__ import annotations

import io
import itertools
import operator
import pickle
from dataclasses import dataclass, field, fields
from typing import List, NamedTuple, Optional


@dataclass
class Chunk:
    """One prefill chunk of a joining sequence."""
    seq: int            # scheduler sequence id
    slot: int           # KV slot
    start: int          # first prompt position of the chunk
    ids: List[int]      # the chunk's token ids (consumed by stage 0 only)
    final: bool         # holds the prompt's last token: the last stage samples it
    temperature: float = 0.6
    top_k: int = 40
    greedy: bool = False
    seed: int = 0
    top_p: float = 1.0
    min_p: float = 0.0
    presence: float = 0.0   # presence / frequency penalties over the generated tokens
    frequency: float = 0.0
    logprobs: int = -1      # alternatives recorded with every draw's logprob (-1: no record)
    nedits: int = 0         # logit-edit entries of the request (logit_bias, bans, min_new_tokens)
    # the entries, SamplingParams.logit_edits' (tokens, values, untils) sorted by
    # token: on the final chunk only, whose stage writes them to the slot's table
    edits: Optional[tuple] = None
    # repetition_penalty / no_repeat_ngram_size and the prompt's length: the two
    # knobs that read the prompt.  On every chunk of such a request, whose ids
    # the last stage copies into the slot's context (has_context)
    rpen: float = 1.0
    ngram: int = 0
    plen: int = 0
    # allowed_token_ids: 1 on every chunk of an asking request (has_allow); the
    # packed mask (the bytes of SamplingParams.allowed_mask's int32 words, one bit
    # per logits column) on the final chunk only, whose stage writes it to the
    # slot's table
    allow: int = 0
    mask: Optional[bytes] = None
    # bad_words: the request's sequences on every chunk of an asking request
    # (has_bad), which is a context request too -- the pass reads the slot's
    # context, so plen is set and the ids travel as with no_repeat_ngram_size;
    # the entries, SamplingParams.bad_word_entries' (exclusive end offsets,
    # tokens back to back), on the final chunk only, whose stage writes them to
    # the slot's table
    nbad: int = 0
    bad: Optional[tuple] = None
    # guide: the row of the last stage's guide table that holds the request's
    # TokenGuide (the engine put it there before the request was planned), on
    # every chunk of an asking request; -1 without one (has_guide).  The final
    # chunk's stage writes (row, state 0) to the slot's entry
    guide: int = -1
    # fork (SamplingParams.n): the KV slot whose positions [0, start) every
    # stage copies into `slot` ahead of this chunk (csrc/kernels/kv_fork.hip),
    # -1 for an ordinary chunk.  A fork's chunk is its prompt's last token
    # (start = L - 1, final): it *opens* the prompt on its slot as a start == 0
    # chunk does, without prefilling it
    fork: int = -1

    @property
    def opens(self) -> bool:
        """The first chunk its slot sees of a prompt."""
        return self.start == 0 or self.fork >= 0

    @property
    def qlen(self) -> int:
        return len(self.ids)

    @property
    def ctx(self) -> bool:
        return self.rpen != 1.0 or self.ngram != 0 or self.nbad > 0


@dataclass
class Row:
    """State of one decode row (written to the device when a group's
    composition changes)."""
    seq: int
    slot: int
    pos: int            # position of the row's NEXT input token
    temperature: float
    top_k: int
    greedy: bool
    seed: int
    step: int           # sampler counter of the next draw (prefill draw = 0)
    src: int            # stage 0: index of the row's input token in the previous
                        # item's token-return vector (kept rows: their old row;
                        # newly activated rows: prev_b + final-chunk index)
    top_p: float = 1.0
    min_p: float = 0.0
    presence: float = 0.0
    frequency: float = 0.0
    logprobs: int = -1
    nedits: int = 0     # logit-edit entries in the slot's table: the group's edit gate (has_edits)
    ctx: int = 0        # repetition_penalty / no_repeat_ngram_size asked: the group's context gate (has_context)
    allow: int = 0      # allowed_token_ids asked: the group's mask gate (has_allow)
    bad: int = 0        # bad_words asked (then ctx = 1 too): the group's bad-words gate (has_bad)
    guide: int = 0      # a guide asked: the group's guide gate (has_guide)


def has_edits(xs) -> bool:
    """Some Row / Chunk carries logit edits: the edit pass runs ahead of the
    draw.  A flag of its own beside row_features' triple, which keys what the
    packed row state and apply_rows' record hold -- the edit pass adds no row
    vector."""
    return any(map(operator.attrgetter("nedits"), xs))


def has_context(xs) -> bool:
    """Some Row / Chunk asks for repetition_penalty or no_repeat_ngram_size:
    the repetition pass runs ahead of the penalties and the slot's context is
    kept (a chunk's prompt ids, a row's draws).  A flag of its own like
    has_edits: the pass reads a per-slot table and adds no row vector."""
    return any(map(operator.attrgetter("ctx"), xs))


def has_allow(xs) -> bool:
    """Some Row / Chunk asks for allowed_token_ids: the mask pass runs right
    ahead of the draw.  A flag of its own like has_edits: the pass reads a
    per-slot table and adds no row vector."""
    return any(map(operator.attrgetter("allow"), xs))


def has_bad(xs) -> bool:
    """Some Row (its flag) / Chunk (its sequence count) asks for bad_words: the
    bad-words pass runs right after the repetition pass.  A flag of its own
    like has_edits: the pass reads two per-slot tables and adds no row vector."""
    return any(map(operator.attrgetter("nbad" if xs and type(xs[0]) is Chunk else "bad"), xs))


def has_guide(xs) -> bool:
    """Some Row (its flag) / Chunk (its table row, -1 without) follows a guide:
    the guide's mask runs last ahead of the draw and its step behind it.  A
    flag of its own like has_edits: the passes read the guide table and the
    slots' states and add no row vector."""
    if xs and type(xs[0]) is Chunk:
        return any(c.guide >= 0 for c in xs)
    return any(map(operator.attrgetter("guide"), xs))


@dataclass
class GroupPlan:
    g: int                                  # group (microbatch) index
    ret: int = 0                            # stage 0: token-return elements to receive first
    rows: Optional[List[Row]] = None        # new composition (None = unchanged)
    n: int = 0                              # active decode rows
    b: int = 0                              # decode bucket rows (0: no decode this step)
    ctxb: int = 0                           # context bucket of the decode graph
    chunks: List[Chunk] = field(default_factory=list)
    # compat forward (reference /forward_b through stages 1..P-1): hidden rows
    kind: str = "step"                      # "step" | "fwd_b"
    fwd_rows: int = 0
    # row_features(rows), once a last stage has computed it (not part of the plan: never sent)
    feats: Optional[tuple] = field(default=None, compare=False, repr=False)
    # has_edits(rows), from the scheduler or once a last stage has computed it (never sent)
    edit: Optional[bool] = field(default=None, compare=False, repr=False)
    # has_context(rows), likewise (never sent)
    ctx: Optional[bool] = field(default=None, compare=False, repr=False)
    # has_allow(rows), likewise (never sent)
    allow: Optional[bool] = field(default=None, compare=False, repr=False)
    # has_bad(rows), likewise (never sent)
    bad: Optional[bool] = field(default=None, compare=False, repr=False)
    # has_guide(rows), likewise (never sent)
    guide: Optional[bool] = field(default=None, compare=False, repr=False)

    @property
    def n_final(self) -> int:
        return sum(1 for c in self.chunks if c.final)

    @property
    def prefill_tokens(self) -> int:
        return sum(c.qlen for c in self.chunks)

    @property
    def has_work(self) -> bool:
        """Anything for stages other than 0's token receive."""
        return self.b > 0 or bool(self.chunks) or self.kind != "step"


@dataclass
class StepPlan:
    step: int
    groups: List[GroupPlan] = field(default_factory=list)
    replica: int = 0
    timing: bool = False                    # record per-item compute events
    end: bool = False                       # session end: followers return
    stop: bool = False                      # shut the follower down


# ---------------------------------------------------------------------------
# Per-row sampler fields: THE list.  The plan wire, the scheduler's request
# state, GroupState's vectors, apply_rows' packed buffer and its argument
# record all read it: a new field is one line here, the dataclass field on Row
# / Chunk (same order) and the SamplingParams plumbing in sampler_values.
# ---------------------------------------------------------------------------
class RowField(NamedTuple):
    name: str    # attribute of Row / Chunk
    dtype: str   # on the device, torch's and numpy's name: "float32" | "int32" | "int64"
    idle: float  # pad rows' value: what apply_rows_kernel writes for i >= n
    gate: str    # travels always ("last": on the last stage) or while a row has a "cut" / "pen" / "lp"
    col: int     # packed buffer (layout: above apply_rows_kernel, csrc/kernels/elementwise.hip):
                 # f[col cap, (col + 1) cap); an int64 field: the col-th int64 vector
    word: int    # the word of apply_rows' argument record that holds the row vector's address
    vec: str     # the row vector, an attribute of parallel/pipeline.py GroupState


ROW_FIELDS = (
    RowField("temperature", "float32", 1.0, "last", 2, 6, "temp"),
    RowField("top_k", "int32", 1, "last", 3, 7, "topk"),
    RowField("greedy", "int32", 1, "last", 4, 8, "greedy"),
    RowField("seed", "int64", 0, "last", 0, 9, "seeds"),
    RowField("step", "int64", 0, "last", 1, 10, "sstep"),
    RowField("top_p", "float32", 1.0, "cut", 6, 12, "topp"),
    RowField("min_p", "float32", 0.0, "cut", 7, 13, "minp"),
    RowField("presence", "float32", 0.0, "pen", 8, 14, "presence"),
    RowField("frequency", "float32", 0.0, "pen", 9, 15, "frequency"),
    RowField("logprobs", "int32", -1, "lp", 10, 16, "nlp"),
)
_GATES = ("last", "cut", "pen", "lp")
NO_FEATURES = (False, False, False)
_STEP = [f.name for f in ROW_FIELDS].index("step")


def _through(gate: str) -> tuple:
    """The fields up to a gate.  Record and wire are positional: what travels
    with a gate travels with every later one (logprobs carry the penalties)."""
    return tuple(f for f in ROW_FIELDS if _GATES.index(f.gate) <= _GATES.index(gate))


def device_fields(last: bool, feats=NO_FEATURES) -> tuple:
    """The fields a composition with the features (cut, pen, lp) writes to the
    device: none off the last stage; on it the top-p / min-p vectors always
    (the sampler reads them only with a cut)."""
    return _through("lp" if feats[2] else "pen" if feats[1] else "cut") if last else ()


def packed_size(cap: int, fields: tuple) -> tuple:
    """(int32 words of the packed buffer to copy, words of the argument record)
    of a composition that writes `fields`; without any: KV slot, position and
    stage 0's gather index (column 5), record words [0, 12)."""
    cols = max([6] + [f.col + 1 for f in fields if f.dtype != "int64"])
    return (4 + cols) * cap + 1, max([12] + [f.word + 1 for f in fields])


_SCAN = operator.attrgetter("top_p", "min_p", "presence", "frequency", "logprobs")
_SCAN_OFF = (1.0, 0.0, 0.0, 0.0, -1)


def _scan(xs) -> tuple:
    """(cut, pen, lp, wide) of Rows / Chunks in one pass that stops once all
    are set; wide: an entry's top_p / min_p is not the default (what the wire
    must carry to be exact, whether or not it cuts)."""
    cut = pen = lp = wide = False
    for tp, mp, pp, fp, n in itertools.filterfalse(_SCAN_OFF.__eq__, map(_SCAN, xs)):
        wide = wide or tp != 1.0 or mp != 0.0
        cut = cut or tp < 1.0 or mp > 0.0
        pen = pen or pp != 0.0 or fp != 0.0
        lp = lp or n >= 0
        if cut and pen and lp:
            break
    return cut, pen, lp, wide


def row_features(xs) -> tuple:
    """(cut, pen, lp) of a list of Rows or Chunks, one pass, no side effect:
    some entry has top_p < 1 or min_p > 0; a nonzero penalty; logprobs >= 0."""
    return _scan(xs)[:3]


def sampler_values(p, seed: int) -> tuple:
    """A request's values of ROW_FIELDS in the order Chunk and Row declare
    them, as (those ahead of the per-draw step, those behind it): a Chunk takes
    both in a row, a Row its step and src between them.  p: its SamplingParams."""
    v = (p.temperature, p.top_k, p.greedy, seed, p.top_p, p.min_p, float(p.presence_penalty),
         float(p.frequency_penalty), -1 if p.logprobs is None else int(p.logprobs))
    return v[:_STEP], v[_STEP:]


def pack_rows(rows, cap: int, first: bool, last: bool, feats, a) -> tuple:
    """Fill the int32 array `a` with the rows' state in the layout documented
    above apply_rows_kernel (pad rows are the kernel's) -> packed_size."""
    import numpy as np

    fields = device_fields(last, feats)
    n, f0 = len(rows), 4 * cap + 1
    a[4 * cap] = n
    cols = [("slot", "int32", 0), ("pos", "int32", 1)] + ([("src", "int32", 5)] if first else [])
    for name, dtype, c in cols + [(f.name, f.dtype, f.col) for f in fields] if n else ():
        dst = (a[: 4 * cap] if dtype == "int64" else a[f0:]).view(dtype)
        # np.fromiter over the attribute: the cheapest way from 4096 objects to a column
        dst[c * cap: c * cap + n] = np.fromiter(map(operator.attrgetter(name), rows), dtype, n)
    return packed_size(cap, fields)


# ---------------------------------------------------------------------------
# Binary wire format of the control plane (dist mode: rank 0 -> every rank)
# ---------------------------------------------------------------------------
# A plan travels as ONE fixed-size int32 record of PLAN_WORDS words (a gloo
# message must be received into a buffer of the exact size):
#   REPEAT  [magic, step]                         same groups as the previous
#                                                 plan to this rank, step + 1
#   STEADY  [magic, step, replica, flags, G,      decode-only groups (no
#            (g, ret, n, b, ctxb) x G]            composition change, no chunk)
#   PICKLE  [magic, nbytes]                       a pickled StepPlan follows as
#                                                 a second message (joins,
#                                                 leaves, prefill chunks, compat)
# In steady-state decode every step is REPEAT or STEADY: no pickling, one
# 512-byte message per follower.  The reference's control "plane" is a JSON
# POST per token per shard (`/root/reference/server.py:172-181`).
PLAN_WORDS = 128
MAGIC_REPEAT, MAGIC_STEADY, MAGIC_PICKLE = 0x4C534452, 0x4C534453, 0x4C534450
_MAX_STEADY_GROUPS = (PLAN_WORDS - 5) // 5
_F_TIMING, _F_END, _F_STOP = 1, 2, 4


def _steady_groups(plan: StepPlan):
    """(g, ret, n, b, ctxb) per group when the plan is decode-only, else None."""
    out = []
    for gp in plan.groups:
        if gp.rows is not None or gp.chunks or gp.kind != "step":
            return None
        out.append((gp.g, gp.ret, gp.n, gp.b, gp.ctxb))
    return out if len(out) <= _MAX_STEADY_GROUPS else None


# Non-steady plans (joins, leaves, prefill chunks) are pickled with every
# GroupPlan in a columnar form: one int32 / float64 / int64 column per Chunk
# and Row field instead of one pickled dataclass per sequence.  A step that
# joins 4096 sequences pickled in ~14 ms and unpickled in ~17 ms on every
# follower as objects (631 KB: too big for a plan-ring slot, so it went over
# gloo to each follower); as columns without the token ids -- which only a
# replica's stage 0 reads -- ~6 / ~7 ms and 182 KB, inline in the ring.
# The columns come from ROW_FIELDS: float64 [n] temperatures while every entry
# has the default top_p / min_p (the common case stays as small as before),
# else [n, 3], or [n, 5] when an entry has a penalty; int64 columns of the
# entry's own fields and the integer ones of the list, the gated ones (the
# logprob counts) only when some entry asks.  A chunk has no step, and its
# seeds travel as a column of their own.
_FLOATS = tuple(f.name for f in ROW_FIELDS if f.dtype == "float32")
_INTS = tuple(f.name for f in _through("last") if f.dtype != "float32")
_ASKED_INTS = tuple(f.name for f in ROW_FIELDS if f.dtype != "float32" and f.gate != "last")
_CHUNK_INTS = ("seq", "slot", "start", "qlen", "final") + tuple(n for n in _INTS if n not in ("seed", "step"))
_ROW_INTS = ("seq", "slot", "pos") + _INTS + ("src",)
_DEFAULTS = {cls: tuple((f.name, f.default) for f in fields(cls)) for cls in (Chunk, Row)}
# sampler_values' order is the order both dataclasses declare the fields in
assert all([n for n, _ in _DEFAULTS[cls] if n in _FLOATS + _INTS + _ASKED_INTS and n != "step"]
           == [f.name for f in ROW_FIELDS if f.name != "step"] for cls in (Chunk, Row))


def _pack_cols(xs, ints: tuple) -> tuple:
    """(int64 [n, w], float64 [n] or [n, w]) columns of Chunks / Rows."""
    import numpy as np

    _, pen, lp, wide = _scan(xs)
    if lp:
        ints = ints + _ASKED_INTS
    floats = [f.name for f in _through("pen" if pen else "cut" if wide else "last") if f.dtype == "float32"]
    fl = np.array(list(map(operator.attrgetter(*floats), xs)), dtype=np.float64)
    return (np.array(list(map(operator.attrgetter(*ints), xs)), dtype=np.int64).reshape(-1, len(ints)),
            fl if len(floats) == 1 else fl.reshape(-1, len(floats)))


def _unpack_cols(cls, ints_names: tuple, ints, floats, **more) -> list:
    """Inverse of _pack_cols (`more`: further columns by field name): the
    entries, fields that did not travel at their defaults."""
    if ints.shape[1] > len(ints_names):
        ints_names = ints_names + _ASKED_INTS
    cols = dict(zip(ints_names, ints.T.tolist()), **more)
    if floats.ndim == 1:
        cols[_FLOATS[0]] = floats.tolist()
    else:
        cols.update(zip(_FLOATS, floats.T.tolist()))
    for nm in ("final", "greedy"):
        if nm in cols:
            cols[nm] = map(bool, cols[nm])
    if "qlen" in cols:
        lens, tok = cols.pop("qlen"), cols.pop("tok")
        if tok is None:
            cols["ids"] = map(range, lens)
        else:
            cols["ids"] = (tok[e - ln: e] for ln, e in zip(lens, itertools.accumulate(lens)))
    return list(itertools.starmap(cls, zip(*(cols[nm] if nm in cols else itertools.repeat(d)
                                             for nm, d in _DEFAULTS[cls]))))


def has_fork(xs) -> bool:
    """Some Chunk starts from a copy of another slot's KV (Chunk.fork)."""
    return any(c.fork >= 0 for c in xs)


def _pack_group(gp: GroupPlan, ids: bool, ctx_ids: bool = False):
    """ctx_ids: the destination runs a last stage, which copies the prompt ids
    of chunks that ask for a context into its table -- a group with such a
    chunk travels with its ids."""
    import numpy as np

    ch = None
    cx = has_context(gp.chunks)
    if gp.chunks:
        c = gp.chunks
        tok = None
        if ids or (ctx_ids and cx):
            tok = np.fromiter(itertools.chain.from_iterable(x.ids for x in c), dtype=np.int32,
                              count=sum(len(x.ids) for x in c))
        ch = _pack_cols(c, _CHUNK_INTS) + (np.array([x.seed for x in c], dtype=np.int64), tok)
    rows = _pack_cols(gp.rows, _ROW_INTS) if gp.rows is not None else None
    out = (gp.g, gp.ret, gp.n, gp.b, gp.ctxb, gp.kind, gp.fwd_rows, ch, rows)
    cx = cx or (gp.rows is not None and has_context(gp.rows))
    if has_edits(gp.chunks) or (gp.rows is not None and has_edits(gp.rows)):
        out += (_pack_edits(gp),)  # a group without edits: the 9-tuple, as before
    elif cx:
        out += (None,)
    if cx:
        out += (_pack_context(gp),)  # one more element: 11, the edits' place held by None without any
    if has_allow(gp.chunks) or (gp.rows is not None and has_allow(gp.rows)):
        # one more: 12, the edits' and the context's places held by None without any
        out += (None,) * (11 - len(out)) + (_pack_allow(gp),)
    if has_bad(gp.chunks) or (gp.rows is not None and has_bad(gp.rows)):
        # one more: 13, behind the mask's place (the context's is taken: an asking request has one)
        out += (None,) * (12 - len(out)) + (_pack_bad(gp),)
    if has_guide(gp.chunks) or (gp.rows is not None and has_guide(gp.rows)):
        # one more: 14, every earlier place held by None without its feature
        out += (None,) * (13 - len(out)) + (_pack_guide(gp),)
    if has_fork(gp.chunks):
        # one more: 15, the chunks' source slots; a plan without a fork encodes as before
        import numpy as np

        out += (None,) * (14 - len(out)) + (np.array([c.fork for c in gp.chunks], dtype=np.int32),)
    return out


def _pack_guide(gp: GroupPlan) -> tuple:
    """The guides of a group, the last element of its wire tuple: (the rows'
    guide column or None, the chunks' table rows or None).  Small integers
    only: the guides' arrays never travel, the engine has written them into
    the last stage's table."""
    import numpy as np

    rows = np.array([r.guide for r in gp.rows], dtype=np.int8) if gp.rows is not None else None
    ch = np.array([c.guide for c in gp.chunks], dtype=np.int16) if gp.chunks else None
    return rows, ch


def _pack_bad(gp: GroupPlan) -> tuple:
    """The bad_words of a group, the last element of its wire tuple: (the rows'
    bad column or None, the chunks' -- (nbad column, offsets [n + 1] into the
    concatenated entries of the chunks that carry theirs (the final asking
    ones), end offsets int32, token offsets [n + 1], tokens int32) -- or
    None)."""
    import numpy as np

    rows = np.array([r.bad for r in gp.rows], dtype=np.int8) if gp.rows is not None else None
    ch = None
    if gp.chunks:
        bd = [c.bad or ((), ()) for c in gp.chunks]
        eoff, toff = np.zeros(len(bd) + 1, dtype=np.int64), np.zeros(len(bd) + 1, dtype=np.int64)
        np.cumsum([len(b[0]) for b in bd], out=eoff[1:])
        np.cumsum([len(b[1]) for b in bd], out=toff[1:])
        ends = np.fromiter(itertools.chain.from_iterable(b[0] for b in bd), dtype=np.int32, count=int(eoff[-1]))
        toks = np.fromiter(itertools.chain.from_iterable(b[1] for b in bd), dtype=np.int32, count=int(toff[-1]))
        ch = (np.array([c.nbad for c in gp.chunks], dtype=np.int32), eoff, ends, toff, toks)
    return rows, ch


def _pack_allow(gp: GroupPlan) -> tuple:
    """The allowed-token masks of a group, the last element of its wire tuple:
    (the rows' allow column or None, the chunks' -- (allow column, which chunks
    carry their mask (the final asking ones), those k chunks' packed words
    [k W] int32 in chunk order) -- or None).  Packed words: the size does not depend
    on how many tokens a list names."""
    import numpy as np

    rows = np.array([r.allow for r in gp.rows], dtype=np.int8) if gp.rows is not None else None
    ch = None
    if gp.chunks:
        masks = [c.mask for c in gp.chunks if c.mask is not None]
        ch = (np.array([c.allow for c in gp.chunks], dtype=np.int8),
              np.array([len(c.mask) if c.mask is not None else -1 for c in gp.chunks], dtype=np.int32),
              np.frombuffer(b"".join(masks), dtype=np.int32) if masks else None)
    return rows, ch


def _pack_context(gp: GroupPlan) -> tuple:
    """The context knobs of a group, the last element of its wire tuple: (the
    rows' ctx column or None, the chunks' (rpen float64, ngram int32, plen
    int32) columns or None)."""
    import numpy as np

    rows = np.array([r.ctx for r in gp.rows], dtype=np.int32) if gp.rows is not None else None
    ch = None
    if gp.chunks:
        ch = (np.array([c.rpen for c in gp.chunks], dtype=np.float64),
              np.array([c.ngram for c in gp.chunks], dtype=np.int32),
              np.array([c.plen for c in gp.chunks], dtype=np.int32))
    return rows, ch


def _pack_edits(gp: GroupPlan) -> tuple:
    """The logit edits of a group, the tenth element of its wire tuple: (the
    rows' nedits column or None, the chunks' -- (nedits column, offsets [n + 1]
    into the concatenated entries of the chunks that carry theirs (the final
    ones), tokens int32, values float32, untils int32) -- or None)."""
    import numpy as np

    rows = np.array([r.nedits for r in gp.rows], dtype=np.int32) if gp.rows is not None else None
    ch = None
    if gp.chunks:
        ed = [c.edits or ((), (), ()) for c in gp.chunks]
        off = np.zeros(len(ed) + 1, dtype=np.int64)
        np.cumsum([len(e[0]) for e in ed], out=off[1:])
        tok, val, until = (np.fromiter(itertools.chain.from_iterable(e[k] for e in ed), dtype=dt, count=int(off[-1]))
                           for k, dt in enumerate((np.int32, np.float32, np.int32)))
        ch = (np.array([c.nedits for c in gp.chunks], dtype=np.int32), off, tok, val, until)
    return rows, ch


def _unpack_edits(ed) -> tuple:
    """Inverse of _pack_edits -> (rows' nedits list or None, chunks' nedits
    list or None, chunks' edits list or None)."""
    rows, ch = ed
    if ch is None:
        return (rows.tolist() if rows is not None else None), None, None
    n, off, tok, val, until = ch
    off, tok, val, until = off.tolist(), tok.tolist(), val.tolist(), until.tolist()
    edits = [(tuple(tok[a:b]), tuple(val[a:b]), tuple(until[a:b])) if b > a else None
             for a, b in zip(off, off[1:])]
    return (rows.tolist() if rows is not None else None), n.tolist(), edits


def _unpack_group(g, ret, n, b, ctxb, kind, fwd_rows, ch, rows, ed=None, cx=None, al=None, bw=None,
                  gd=None, fk=None) -> GroupPlan:
    """Inverse of _pack_group.  Chunks sent without their token ids carry
    range(len) in their place (their stage reads only the lengths)."""
    gp = GroupPlan(g, ret=ret, n=n, b=b, ctxb=ctxb, kind=kind, fwd_rows=fwd_rows)
    more_r, more_c = {}, {}
    if ed is not None:
        rn, cn, ce = _unpack_edits(ed)
        if rn is not None:
            more_r = dict(nedits=rn)
        if cn is not None:
            more_c = dict(nedits=cn, edits=ce)
    if cx is not None:
        rc, cc = cx
        if rc is not None:
            more_r["ctx"] = rc.tolist()
        if cc is not None:
            more_c.update(zip(("rpen", "ngram", "plen"), (col.tolist() for col in cc)))
    if al is not None:
        ra, ca = al
        if ra is not None:
            more_r["allow"] = ra.tolist()
        if ca is not None:
            flag, lens, words = ca
            buf, at, masks = (words.tobytes() if words is not None else b""), 0, []
            for n in lens.tolist():
                masks.append(buf[at: at + n] if n >= 0 else None)
                at += max(n, 0)
            more_c.update(allow=flag.tolist(), mask=masks)
    if gd is not None:
        rg, cg = gd
        if rg is not None:
            more_r["guide"] = rg.tolist()
        if cg is not None:
            more_c["guide"] = cg.tolist()
    if fk is not None:
        more_c["fork"] = fk.tolist()
    if bw is not None:
        rb, cb = bw
        if rb is not None:
            more_r["bad"] = rb.tolist()
        if cb is not None:
            nb, eoff, ends, toff, toks = cb
            eoff, ends, toff, toks = eoff.tolist(), ends.tolist(), toff.tolist(), toks.tolist()
            more_c.update(nbad=nb.tolist(),
                          bad=[(tuple(ends[a:b]), tuple(toks[c:d])) if b > a else None
                               for a, b, c, d in zip(eoff, eoff[1:], toff, toff[1:])])
    if ch is not None:
        ints, floats, seeds, tok = ch
        gp.chunks = _unpack_cols(Chunk, _CHUNK_INTS, ints, floats, seed=seeds.tolist(),
                                 tok=tok.tolist() if tok is not None else None, **more_c)
    if rows is not None:
        gp.rows = _unpack_cols(Row, _ROW_INTS, *rows, **more_r)
    return gp


class _PlanPickler(pickle.Pickler):
    """Pickles every GroupPlan through _pack_group (ids: with token ids)."""

    def __init__(self, file, ids: bool, ctx_ids: bool = False):
        super().__init__(file, protocol=pickle.HIGHEST_PROTOCOL)
        self.ids, self.ctx_ids = ids, ctx_ids

    def reducer_override(self, obj):
        if type(obj) is GroupPlan:
            return _unpack_group, _pack_group(obj, self.ids, self.ctx_ids)
        return NotImplemented


def _plan_dumps(plan: StepPlan, ids: bool, ctx_ids: bool = False) -> bytes:
    buf = io.BytesIO()
    _PlanPickler(buf, ids, ctx_ids).dump(plan)
    return buf.getvalue()


class PlanEncoder:
    """Per-destination encoder (remembers what it sent last for REPEAT).
    ids=False: the destination stages never read prefill token ids (every
    stage but a replica's first), so the chunks travel without them --
    except, with ctx_ids=True (a last stage is among the destinations), those
    of a group with a chunk that asks for repetition_penalty or
    no_repeat_ngram_size: the last stage keeps that prompt."""

    def __init__(self, ids: bool = True, ctx_ids: bool = False):
        self._prev = None  # (step, replica, flags, groups) of the last plan sent
        self.ids, self.ctx_ids = ids, ctx_ids

    def encode(self, plan: StepPlan):
        """-> (int32 numpy record, pickle payload bytes or None)."""
        import numpy as np

        rec = np.zeros(PLAN_WORDS, dtype=np.int32)
        flags = (_F_TIMING if plan.timing else 0) | (_F_END if plan.end else 0) | (_F_STOP if plan.stop else 0)
        groups = _steady_groups(plan)
        if groups is None:
            payload = _plan_dumps(plan, self.ids, self.ctx_ids)
            rec[0], rec[1] = MAGIC_PICKLE, len(payload)
            self._prev = None
            return rec, payload
        prev = self._prev
        if (prev is not None and plan.step == prev[0] + 1 and plan.replica == prev[1]
                and flags == prev[2] and groups == prev[3] and groups):
            rec[0], rec[1] = MAGIC_REPEAT, plan.step
        else:
            rec[0], rec[1], rec[2], rec[3], rec[4] = MAGIC_STEADY, plan.step, plan.replica, flags, len(groups)
            if groups:
                rec[5: 5 + 5 * len(groups)] = np.asarray(groups, dtype=np.int32).reshape(-1)
        self._prev = (plan.step, plan.replica, flags, groups)
        return rec, None


class PlanDecoder:
    """Per-source decoder (holds the previous plan's groups for REPEAT)."""

    def __init__(self):
        self._prev = None  # (replica, flags, groups)

    def decode(self, rec, fetch_payload) -> StepPlan:
        """rec: int32 sequence of PLAN_WORDS; fetch_payload(nbytes) -> bytes."""
        magic = int(rec[0])
        if magic == MAGIC_PICKLE:
            self._prev = None
            # our own plan records, produced by this job's rank 0
            return pickle.loads(fetch_payload(int(rec[1])))
        if magic == MAGIC_REPEAT:
            if self._prev is None:
                raise ValueError("plan REPEAT record without a previous plan")
            replica, flags, groups = self._prev
            step = int(rec[1])
        elif magic == MAGIC_STEADY:
            step, replica, flags, G = (int(x) for x in rec[1:5])
            vals = [int(x) for x in rec[5: 5 + 5 * G]]
            groups = [tuple(vals[5 * i: 5 * i + 5]) for i in range(G)]
            self._prev = (replica, flags, groups)
        else:
            raise ValueError(f"bad plan record magic {magic:#x}")
        # fresh GroupPlan objects every step (workers key posted receives by id)
        return StepPlan(step=step, replica=replica, timing=bool(flags & _F_TIMING),
                        end=bool(flags & _F_END), stop=bool(flags & _F_STOP),
                        groups=[GroupPlan(g, ret=r, n=n, b=b, ctxb=c) for g, r, n, b, c in groups])
