"""Refusals of csrc/bindings.cpp for the argument kinds its entry points share:
the per-row vectors (step, active, pos, top_p / min_p, slots), the segment
maxima of a logits matrix and the QKV target (token slots / positions, caches,
RoPE table).

Every call here has exactly one malformed tensor -- a wrong dtype, a wrong
length or a non-contiguous view -- beside well-formed ones of the smallest
shapes, and must raise a RuntimeError that names the argument from the
binding's host checks: no case reaches a launcher, so no kernel ever sees the
bad tensor.  (A few messages name the group -- "row vectors", "sampling params"
-- rather than the one argument; the patterns allow for that.)
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, LD, V, SLOTS, WIDTH = 2, 64, 50, 3, 4
N_KV, MAX_SEQ, HD = 1, 8, 64
Q_SIZE = KV_SIZE = N_KV * HD
f32, f64, i16, i32, i64, bf16 = (torch.float32, torch.float64, torch.int16, torch.int32, torch.int64,
                                 torch.bfloat16)


@pytest.fixture(scope="module")
def C():
    from llm_sharding_demo_amd.ops.hip import _load

    return _load()


def z(*shape, dt=f32):
    return torch.zeros(*shape, dtype=dt, device=DEV)


@pytest.fixture(scope="module")
def pool():
    """Well-formed arguments by name; no test writes to them."""
    return {
        "logits": z(B, LD), "V": V, "segmax": z(B, LD // 8),
        # per-row vectors
        "slots": z(B, dt=i32), "step": z(B, dt=i64), "active": z(B, dt=i32), "pos": z(B, dt=i32),
        "top_p": z(B), "min_p": z(B), "tokens": z(B, dt=i32), "nlp": z(B, dt=i32), "out": z(B, dt=i32),
        "temp": z(B), "topk": z(B, dt=i32), "greedy": z(B, dt=i32), "seeds": z(B, dt=i64),
        "counts": z(B, dt=i64), "presence": z(B), "frequency": z(B),
        # per-slot tables, 4 entries wide
        "cnt": z(SLOTS, dt=i32), "plen": z(SLOTS, dt=i32), "rpen": z(SLOTS), "ngram": z(SLOTS, dt=i32),
        "on": z(SLOTS, dt=i32), "tab_i": z(SLOTS, WIDTH, dt=i32), "tab_f": z(SLOTS, WIDTH),
        "gcls": z(1, LD, dt=i16), "gnext": z(1, WIDTH, dt=i16), "gdim": z(1, 2, dt=i32), "gsl": z(SLOTS, 2, dt=i32),
        "lp_tok": z(SLOTS, WIDTH), "lp_top_id": z(SLOTS, WIDTH, WIDTH, dt=i32), "lp_top": z(SLOTS, WIDTH, WIDTH),
        # QKV target and the projections in front of it
        "kc": z(SLOTS, N_KV, MAX_SEQ, HD, dt=bf16), "vc": z(SLOTS, N_KV, MAX_SEQ, HD, dt=bf16),
        "tslot": z(B, dt=i32), "tpos": z(B, dt=i32), "rope": z(MAX_SEQ, HD // 2, 2),
        "a": z(B, LD, dt=bf16), "w_qkv": z(Q_SIZE + 2 * KV_SIZE, LD, dt=bf16), "y_qkv": z(B, Q_SIZE + 2 * KV_SIZE),
        "w": z(LD, LD, dt=bf16),
        "none": None, "0": 0, "1": 1, "6": 6, "0.0": 0.0, "q_size": Q_SIZE, "kv_size": KV_SIZE, "hd": HD,
    }


# entry point -> the pool names of its positional arguments
ENTRIES = {
    "sample": "logits V temp topk greedy seeds step segmax top_p min_p",
    "sample_into": "logits V temp topk greedy seeds step out active pos segmax top_p min_p",
    "penalize": "logits V tab_i slots counts presence frequency segmax",
    "logit_edits": "logits V cnt tab_i tab_f tab_i slots step segmax",
    "allow_mask": "logits V on tab_i slots segmax",
    "guide_mask": "logits V gcls gnext gdim gsl slots segmax",
    "guide_advance": "gcls gnext gdim gsl V slots tokens active",
    "repetition": "logits V plen rpen ngram tab_i slots step segmax",
    "bad_words": "logits V cnt tab_i tab_i plen tab_i slots step segmax",
    "record_context": "tab_i plen slots step tokens active 0",
    "record_tokens": "tab_i slots step tokens active 0",
    "logprobs": "logits V tokens nlp slots step active lp_tok lp_top_id lp_top 0",
    "linear_f32": "a w 1 1 none segmax",
    "gemv_logits": "a w 0 none none 0.0 segmax",
    "linear_qkv": "a w_qkv none kc vc tslot tpos q_size kv_size hd rope 0 1 none",
    "gemv": "a w_qkv none 6 0 none none 0.0 none kc vc tslot tpos q_size kv_size hd rope",
    "qkv_post": "y_qkv none kc vc tslot tpos q_size kv_size hd rope",
}

# argument -> what a refusal of it says
NAMES = {"step": "step|sampling params", "active": "active", "pos": "pos", "top_p": "top_p", "min_p": "min_p",
         "slots": "slots|vectors", "segmax": "segmax", "tslot": "token_slots", "tpos": "token_pos", "kc": "cache",
         "rope": "rope"}

CASES = [(entry, arg, defect) for entry, args in ENTRIES.items() for arg in args.split() if arg in NAMES
         for defect in ("dtype", "length", "strided")]


def malformed(t, defect):
    """`t` with one defect: another dtype of its class, a last dimension that
    is one short (one long for a vector; half for a cache), or the same shape
    as every second element of a tensor twice as wide."""
    if defect == "dtype":
        return t.to({i32: i64, i64: i32, f32: f64, bf16: f32}[t.dtype])
    shape = list(t.shape)
    if defect == "length":
        shape[-1] = shape[-1] + 1 if t.dim() == 1 else shape[-1] // 2 if t.dim() == 4 else shape[-1] - 1
        return z(*shape, dt=t.dtype)
    shape[-1] *= 2
    v = z(*shape, dt=t.dtype)[..., ::2]
    assert v.shape == t.shape and not v.is_contiguous()
    return v


def test_cases_cover_every_kind():
    kinds = {arg for _, arg, _ in CASES}
    assert kinds == set(NAMES) and len(CASES) == 3 * sum(a in NAMES for e in ENTRIES.values() for a in e.split())


@pytest.mark.parametrize("entry,arg,defect", CASES, ids=["-".join(c) for c in CASES])
def test_refused_on_the_host(C, pool, entry, arg, defect):
    args = [malformed(pool[n], defect) if n == arg else pool[n] for n in ENTRIES[entry].split()]
    with pytest.raises(RuntimeError, match=NAMES[arg]):
        getattr(C, entry)(*args)
