"""Per-request n on an MI355X: the kv_fork kernel against its torch twin, whole
buffer bit for bit, and the engine with forked samples -- the HIP copy against
the torch twin in its place (same schedule, exact copy: same tokens, same KV
bits), greedy samples against the n = 1 output, and the launch counter."""
import pytest
import torch

from llm_sharding_demo_amd.config import EngineConfig, SamplingParams
from llm_sharding_demo_amd.ops import reference as ref
from llm_sharding_demo_amd.runtime.engine import Engine

pytestmark = pytest.mark.gpu


def _backend():
    from llm_sharding_demo_amd.ops.hip import HipBackend

    return HipBackend()


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _random_buf(shape, dtype, seed, offset=0):
    """Random bit patterns (NaNs and all) on the GPU; offset: elements the
    buffer starts past a 16-byte boundary."""
    g = torch.Generator().manual_seed(seed)
    n = 1
    for d in shape:
        n *= d
    idt = torch.int16 if dtype == torch.bfloat16 else torch.int32
    lo, hi = (-2 ** 15, 2 ** 15) if idt == torch.int16 else (-2 ** 31, 2 ** 31)
    raw = torch.randint(lo, hi, (n + offset,), dtype=idt, generator=g).cuda()
    return raw[offset:].view(dtype).view(shape)


def _check(buf, src, dst, lens):
    want = buf.clone()
    ref.kv_fork(want, src, dst, lens)
    _backend().kv_fork(buf, src, dst, lens)
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), _bits(want))
    return want


# several forks in one launch, two of them from one source; every length of
# {0, 1, 7, 39} at every place
LENS = [(0, 1, 7), (1, 7, 39), (39, 0, 1), (7, 39, 0), (39, 39, 39), (0, 0, 0)]


@pytest.mark.parametrize("lens", LENS, ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("hd", [8, 64, 128])
def test_kernel_equals_twin_bit_for_bit(hd, dtype, lens):
    buf = _random_buf((3, 2, 6, 2, 40, hd), dtype, seed=hd + len(lens))
    before = buf.clone()
    got = _check(buf, [0, 0, 3], [1, 2, 4], list(lens))
    # the twin itself: sources, slot 5 and everything at or past len are untouched
    for s in (0, 3, 5):
        assert torch.equal(_bits(got[:, :, s]), _bits(before[:, :, s]))
    for d, n in zip((1, 2, 4), lens):
        assert torch.equal(_bits(got[:, :, d, :, n:]), _bits(before[:, :, d, :, n:]))


@pytest.mark.parametrize("dtype,hd,offset", [(torch.float32, 8, 1), (torch.bfloat16, 8, 1), (torch.bfloat16, 8, 2),
                                             (torch.bfloat16, 2, 0), (torch.bfloat16, 1, 0), (torch.float32, 3, 0)],
                         ids=["fp32-base+4", "bf16-base+2", "bf16-base+4", "bf16-hd2", "bf16-hd1", "fp32-hd3"])
def test_kernel_narrow_accesses(dtype, hd, offset):
    """A base or a position's bytes that are no multiple of 16: dword or byte accesses."""
    buf = _random_buf((3, 2, 6, 2, 40, hd), dtype, seed=7, offset=offset)
    assert buf.data_ptr() % 16 == (offset * buf.element_size()) % 16
    _check(buf, [0, 0, 3], [1, 2, 4], [39, 7, 1])


def test_kernel_run_split_over_pieces():
    """1025 positions x 128 bytes: nine 16 KiB pieces per run, the last one partial."""
    buf = _random_buf((1, 2, 3, 2, 1100, 64), torch.bfloat16, seed=3)
    _check(buf, [1, 1], [0, 2], [1025, 300])


def test_wrapper_refuses_overlap_and_bad_indices():
    buf = _random_buf((3, 2, 6, 2, 40, 8), torch.bfloat16, seed=1)
    before = buf.clone()
    be = _backend()
    for src, dst, lens in ([[0, 1], [2, 2], [3, 3]],      # one destination twice
                           [[0, 1], [1, 2], [3, 3]],      # a destination that is a source
                           [[0], [0], [3]],               # onto itself
                           [[0], [6], [3]], [[-1], [2], [3]],  # slots out of range
                           [[0], [1], [41]], [[0], [1], [-1]],  # lengths out of range
                           [[0, 1], [2], [3, 3]]):        # ragged
        with pytest.raises(ValueError):
            be.kv_fork(buf, src, dst, lens)
        with pytest.raises(ValueError):
            ref.kv_fork(buf, src, dst, lens)
    with pytest.raises(ValueError):
        be.kv_fork(buf[:, :, :, :, :, :4], [0], [1], [3])  # not the whole allocation
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), _bits(before))


# ---------------------------------------------------------------------------
# engine
PROMPTS = [[5, 9, 3, 7, 11, 2, 8, 4, 6, 1, 12], list(range(20, 57))]


def _engine(model, P=1, twin=False, **kw):
    cfg = EngineConfig(model_id=model, num_stages=P, max_batch=16, device="cuda", use_graphs=True,
                       max_seq_len=512, num_microbatches=2, **kw)
    e = Engine(cfg, devices=["cuda:0"] * P)
    assert all(st.backend.name == "hip" for st in e.stages)
    if twin:
        for st in e.stages:  # the op swapped for the torch twin, everything else as it is
            st.backend.kv_fork = lambda buf, src, dst, lens, idx=None: ref.kv_fork(buf, src, dst, lens)
    return e


@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("model", ["gpt2-test", "llama-test"])
def test_engine_sampled_hip_copy_equals_twin_copy(model, P):
    """Same requests, same schedule, and the copy is exact: the tokens of all
    samples and the KV buffers' bits agree between the HIP kv_fork and the
    torch twin in its place."""
    sps = [SamplingParams(n=4, max_new_tokens=8, temperature=1.0, top_k=50, seed=7, stop_at_eos=False),
           SamplingParams(n=4, max_new_tokens=8, temperature=1.3, top_k=200, seed=90, stop_at_eos=False,
                          repetition_penalty=1.3, logprobs=2)]
    a, b = _engine(model, P), _engine(model, P, twin=True)
    ra, rb = a.generate_requests(PROMPTS, sps), b.generate_requests(PROMPTS, sps)
    outs = [[s.output for s in r.samples] for r in ra]
    assert outs == [[s.output for s in r.samples] for r in rb]
    assert all(len(o) == 4 and all(len(t) == 8 for t in o) for o in outs)
    assert len({tuple(t) for t in outs[0]}) > 1  # the samples drew with their own seeds
    for x, y in zip(ra[1].samples, rb[1].samples):
        assert x.logprobs.tokens == y.logprobs.tokens == x.output
        assert x.logprobs.token_logprobs == y.logprobs.token_logprobs
    torch.cuda.synchronize()
    for sa, sb in zip(a.stages, b.stages):
        assert torch.equal(_bits(sa.kv.buf), _bits(sb.kv.buf))
    assert [w.kv_fork_launches for w in a.workers] == [w.kv_fork_launches for w in b.workers]
    assert all(w.kv_fork_launches >= 1 for w in a.workers)
    # every slot came back
    assert sum(p.available for p in a.slot_pools) == a.kv_slots


@pytest.mark.parametrize("P,chunk", [(1, 0), (2, 0), (2, 5)])
@pytest.mark.parametrize("model", ["gpt2-test", "llama-test"])
def test_engine_greedy_samples_equal_the_single_output(model, P, chunk):
    sp = dict(greedy=True, max_new_tokens=8)
    one = _engine(model).generate_ids(PROMPTS, SamplingParams(**sp))
    got = _engine(model, P, prefill_chunk=chunk).generate_samples(PROMPTS, SamplingParams(n=3, **sp))
    assert got == [[o] * 3 for o in one]


def test_default_traffic_launches_no_copy():
    e = _engine("gpt2-test")
    e.generate_ids(PROMPTS, SamplingParams(max_new_tokens=6, seed=1))
    e.generate_samples(PROMPTS, SamplingParams(max_new_tokens=6, seed=1, n=1))
    assert all(w.kv_fork_launches == 0 for w in e.workers) and e.scheduler._forking == 0
    e.generate_samples(PROMPTS, SamplingParams(max_new_tokens=6, seed=1, n=4))
    assert all(w.kv_fork_launches >= 1 for w in e.workers)
