"""The prefix cache on an MI355X: a hit's KV copy by the HIP kv_fork kernel
against the torch twin in its place (same schedule, exact copy: same tokens,
same KV bits), the copied positions against the entry's, a hit against the
engine without the cache, many hits of one entry in one launch, a prompt that
would have matched an evicted entry, and the cache switched off."""
import random

import pytest
import torch

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.runtime.engine import Engine

pytestmark = pytest.mark.gpu

_R = random.Random(11)
A = [_R.randrange(3, 200) for _ in range(64)]
B = A[:48] + [_R.randrange(3, 200) for _ in range(32)]
SEEDED = dict(temperature=1.1, top_k=60, seed=100, stop_at_eos=False)
NEW = 8


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _engine(model, P=1, twin=False, max_batch=16, **kw):
    cfg = EngineConfig(model_id=model, num_stages=P, max_batch=max_batch, device="cuda", use_graphs=True,
                       max_seq_len=512, num_microbatches=2, **kw)
    e = Engine(cfg, devices=["cuda:0"] * P)
    assert all(st.backend.name == "hip" for st in e.stages)
    if twin:
        for st in e.stages:  # the op swapped for the torch twin, everything else as it is
            st.backend.kv_fork = lambda buf, src, dst, lens, idx=None: ref.kv_fork(buf, src, dst, lens)
    return e


def _slot_of(e, prompt):
    """The slot of the entry whose key is `prompt` (replica 0)."""
    return {tuple(k): s for s, _, k in e.scheduler.core.prefix_entries(0)}[tuple(prompt)]


@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("model", ["gpt2-test", "llama-test"])
def test_a_then_b(model, P):
    """A (64 tokens), then B (A's first 48 + 32 others), chunks of 48."""
    a, b = (_engine(model, P, twin=t, prefill_chunk=48, prefix_cache=4) for t in (False, True))
    off = _engine(model, P, prefill_chunk=48)
    sp = SamplingParams(max_new_tokens=NEW, **SEEDED)
    for e in (a, b):
        assert e.generate_requests([A], [sp])[0].cached_tokens == 0
    torch.cuda.synchronize()
    before = [st.kv.buf.clone() for st in a.stages]
    launches = [w.kv_fork_launches for w in a.workers]
    ra, rb = (e.generate_requests([B], [sp])[0] for e in (a, b))
    # the HIP copy against the torch twin in its place: tokens and every stage's KV bits
    assert ra.cached_tokens == rb.cached_tokens == 48
    assert ra.output == rb.output and len(ra.output) == NEW
    torch.cuda.synchronize()
    for sa, sb in zip(a.stages, b.stages):
        assert torch.equal(_bits(sa.kv.buf), _bits(sb.kv.buf))
    assert [w.kv_fork_launches - x for w, x in zip(a.workers, launches)] == [1] * P
    assert [w.kv_fork_launches for w in a.workers] == [w.kv_fork_launches for w in b.workers]
    # B's slot (an entry by now; its decode wrote at 80 and past): positions
    # [0, 48) are the entry's bit for bit, on every stage; no other slot changed
    sa_, sb_ = _slot_of(a, A), _slot_of(a, B)
    assert sa_ != sb_
    for st, was in zip(a.stages, before):
        buf = st.kv.buf
        if buf.shape[0] == 0:
            continue
        assert torch.equal(_bits(buf[:, :, sb_, :, :48]), _bits(buf[:, :, sa_, :, :48]))
        assert not torch.equal(_bits(buf[:, :, sb_, :, 48:80]), _bits(was[:, :, sb_, :, 48:80]))  # the tail ran
        others = [s for s in range(a.kv_slots) if s != sb_]
        assert torch.equal(_bits(buf[:, :, others]), _bits(was[:, :, others]))
    # a sampled hit and a greedy hit against the engine without the cache, same chunking
    assert ra.output == off.generate_requests([B], [sp])[0].output
    g = SamplingParams(max_new_tokens=NEW, greedy=True, stop_at_eos=False)
    a.prefix_cache_clear()
    a.generate_requests([A], [g])
    got = a.generate_requests([B], [g])[0]
    assert got.cached_tokens == 48 and got.output == off.generate_requests([B], [g])[0].output
    st = a.prefix_cache_stats()
    assert (st["hits"], st["tokens_reused"], st["evictions"]) == (2, 96, 0)
    assert sum(p.available for p in a.slot_pools) + st["entries"] == a.kv_slots


@pytest.mark.parametrize("model,P", [("gpt2-test", 1), ("llama-test", 2)])
def test_many_hits_of_one_entry_in_one_step(model, P):
    """8 requests behind one 48-token stem, submitted together once the stem's
    donor has finished: one group's item, ONE kv_fork launch per stage with
    eight reads of one source; the outputs of the torch-twin engine."""
    stem = A[:48]
    rnd = random.Random(5)
    prompts = [stem + [rnd.randrange(3, 200) for _ in range(n)] for n in (1, 5, 32, 1, 5, 32, 5, 32)]
    sps = [SamplingParams(max_new_tokens=NEW, temperature=1.0, top_k=50, seed=20 + i, stop_at_eos=False)
           for i in range(8)]
    outs = []
    for twin in (False, True):
        e = _engine(model, P, twin=twin, prefix_cache=8)
        e.generate_requests([stem], [SamplingParams(max_new_tokens=2, greedy=True, stop_at_eos=False)])
        launches = [w.kv_fork_launches for w in e.workers]
        rs = e.generate_requests(prompts, sps)
        assert [r.cached_tokens for r in rs] == [48] * 8
        assert [w.kv_fork_launches - x for w, x in zip(e.workers, launches)] == [1] * P
        outs.append([r.output for r in rs])
        torch.cuda.synchronize()
        # the eight slots are entries now (the stem's own was covered by the first
        # longer key): each holds the stem's KV, the same bits at positions [0, 48)
        slots = [_slot_of(e, p) for p in prompts]
        assert len(set(slots)) == 8
        for stg in e.stages:
            buf = stg.kv.buf
            for s in slots[1:]:
                assert torch.equal(_bits(buf[:, :, s, :, :48]), _bits(buf[:, :, slots[0], :, :48]))
        st = e.prefix_cache_stats()
        assert st["hits"] == 8 and st["tokens_reused"] == 8 * 48
        assert sum(p.available for p in e.slot_pools) + st["entries"] == e.kv_slots
    assert outs[0] == outs[1] and all(len(o) == NEW for o in outs[0])


def test_reuse_after_eviction():
    """max_batch = 4, prefix_cache = 2: a hit, then four distinct prompts that
    evict both entries and rewrite their slots on both lanes; a prompt that
    would have matched the evicted entry misses, and draws what the engine
    without the cache draws."""
    rnd = random.Random(9)
    fresh = lambda n: [rnd.randrange(3, 200) for _ in range(n)]  # noqa: E731
    p0 = fresh(40)
    hit, late = p0[:32] + fresh(9), p0[:32] + fresh(12)
    others = [fresh(30 + 3 * i) for i in range(4)]
    sp = SamplingParams(max_new_tokens=NEW, **SEEDED)
    on, off = _engine("gpt2-test", max_batch=4, prefix_cache=2), _engine("gpt2-test", max_batch=4)
    assert on.kv_slots == 4
    on.generate_requests([p0], [sp])
    assert on.generate_requests([hit], [sp])[0].cached_tokens == 32
    assert on.prefix_cache_stats()["entries"] == 2
    # four at once: every slot is needed, both entries go, both groups (lanes) prefill and decode
    rs = on.generate_requests(others, [sp] * 4)
    assert [r.cached_tokens for r in rs] == [0] * 4 and on.prefix_cache_stats()["evictions"] >= 2
    keys = [tuple(k) for _, _, k in on.scheduler.core.prefix_entries(0)]
    assert tuple(p0) not in keys and tuple(hit) not in keys
    r = on.generate_requests([late], [sp])[0]
    assert r.cached_tokens == 0
    assert r.output == off.generate_requests([late], [sp])[0].output
    # and what is cached now still serves: the same prompt again starts behind all but its last token
    assert on.generate_requests([late], [sp])[0].cached_tokens == len(late) - 1
    st = on.prefix_cache_stats()
    assert sum(p.available for p in on.slot_pools) + st["entries"] == on.kv_slots and st["entries"] <= 2


def test_off_means_off():
    e = _engine("gpt2-test")
    assert e.cfg.prefix_cache == 0
    e.generate_ids([A, B, A], SamplingParams(max_new_tokens=6, seed=1))
    e.generate_ids([B], SamplingParams(max_new_tokens=6, seed=1))
    assert all(w.kv_fork_launches == 0 for w in e.workers)
    assert sum(p.available for p in e.slot_pools) == e.kv_slots
    core = e.scheduler.core
    assert tuple(core.prefix_cache_stats()) == (0, 0, 0, 0, 0) and not core.prefix_entries(0) and not core.hits()
    assert e.prefix_cache_stats() == {"entries": 0, "hits": 0, "misses": 0, "tokens_reused": 0, "evictions": 0}
