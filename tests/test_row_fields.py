"""The per-row sampler fields (runtime/plan.py ROW_FIELDS) against values
written out by hand from the layout comment above apply_rows_kernel
(csrc/kernels/elementwise.hip): the native packer bit for bit, the argument
record's pointers, the torch path's row vectors, the feature pass and the
plan wire's arrays.  Every expected value is a literal offset here, never the
table under test."""
import types

import numpy as np
import pytest
import torch

from llm_sharding_demo_amd.parallel.pipeline import GroupState, StageWorker
from llm_sharding_demo_amd.runtime.plan import (Chunk, GroupPlan, Row, _pack_group, _unpack_group, pack_rows,
                                                row_features)

SENT = -777
# feature set -> ((cut, pen, lp), words per cap on the last stage, record words on the last stage)
SETS = {"none": ((False, False, False), 12, 14), "cut": ((True, False, False), 12, 14),
        "pen": ((False, True, False), 14, 16), "lp_pen": ((False, True, True), 15, 17),
        "lp_nopen": ((False, False, True), 15, 17)}


def _rows(n, kind, src=None):
    """n rows whose every field differs per row: seeds >= 2^61 and steps >=
    2^32 (a swapped int32 half or a misaligned int64 view shows), fp32 bits
    that are no small integer."""
    out = []
    for i in range(n):
        r = Row(seq=i, slot=100 + i, pos=7 + 3 * i, temperature=0.7 + 0.013 * i, top_k=40 + i, greedy=i % 2 == 0,
                seed=(1 << 61) + 0x1234567 + i, step=(1 << 32) + 5 + i, src=(n - 1 - i) if src is None else src[i])
        if kind == "cut":
            r.top_p, r.min_p = 0.9 - 0.01 * i, 0.05 + 0.01 * i
        if kind in ("pen", "lp_pen"):
            r.presence, r.frequency = 0.3 + 0.1 * i, -0.2 - 0.1 * i
        if kind in ("lp_pen", "lp_nopen"):
            r.logprobs = i % 4
        out.append(r)
    return out


def _bits(xs):
    return np.asarray(xs, np.float32).view(np.int32).tolist()


@pytest.mark.parametrize("cap,n", [(8, 3), (64, 64), (300, 0)])
@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("last", [True, False])
@pytest.mark.parametrize("kind", list(SETS))
def test_packer_bit_for_bit(cap, n, first, last, kind):
    feats, per_cap, nargs = SETS[kind]
    rows = _rows(n, kind)
    a = np.full(15 * cap + 1, SENT, np.int32)
    words, rec = pack_rows(rows, cap, first, last, feats, a)
    assert (words, rec) == ((per_cap * cap + 1, nargs) if last else (10 * cap + 1, 12))
    assert a[4 * cap] == n
    f0 = 4 * cap + 1

    def col(k):
        return a[f0 + k * cap: f0 + k * cap + n].tolist()

    def untouched(k):
        return (a[f0 + k * cap: f0 + (k + 1) * cap] == SENT).all()

    assert col(0) == [r.slot for r in rows] and col(1) == [r.pos for r in rows]
    assert col(5) == [r.src for r in rows] if first else untouched(5)
    s64 = a[: 4 * cap].view(np.int64)
    if not last:
        assert (a[: 4 * cap] == SENT).all() and all(untouched(k) for k in (2, 3, 4, 6, 7, 8, 9, 10))
        return
    assert s64[:n].tolist() == [r.seed for r in rows] and s64[cap: cap + n].tolist() == [r.step for r in rows]
    if n:  # little-endian halves, seeds in [0, 2 cap), steps from 2 cap
        assert a[0] == (rows[0].seed & 0xFFFFFFFF) and a[1] == rows[0].seed >> 32
        assert a[2 * cap] == 5 and a[2 * cap + 1] == 1
        assert _bits([rows[0].temperature])[0] == 0x3F333333 and col(2)[0] == 0x3F333333
    assert col(2) == _bits([r.temperature for r in rows])
    assert col(3) == [r.top_k for r in rows] and col(4) == [int(r.greedy) for r in rows]
    assert col(6) == _bits([r.top_p for r in rows]) and col(7) == _bits([r.min_p for r in rows])
    if kind in ("pen", "lp_pen", "lp_nopen"):  # the record is positional: logprobs carry the penalties
        assert col(8) == _bits([r.presence for r in rows]) and col(9) == _bits([r.frequency for r in rows])
    else:
        assert untouched(8) and untouched(9)
    assert col(10) == [r.logprobs for r in rows] if kind.startswith("lp") else untouched(10)
    if n == cap:  # full: nothing ran past a column's end
        assert a[4 * cap] == n and a.size == 15 * cap + 1


def _worker(first, last, P=2):
    return types.SimpleNamespace(device=torch.device("cpu"), H=4, scratch_slot=99, first=first, last=last, P=P)


@pytest.mark.parametrize("first,last", [(True, True), (False, True), (True, False)])
def test_record_pointers(first, last):
    w = _worker(first, last)
    gs = GroupState(w, 0, 16)
    rec = gs.rows_record(w).tolist()
    assert len(rec) == (17 if last else 12)
    assert rec[:3] == [16, 99, gs.rows_dev.data_ptr()]
    assert gs.rows_dev.numel() == ((15 if last else 10) * 16 + 1) and gs.rows_dev.dtype == torch.int32
    assert rec[3:6] == [gs.slots.data_ptr(), gs.pos.data_ptr(), gs.active.data_ptr()]
    if last:
        assert rec[6:11] == [t.data_ptr() for t in (gs.temp, gs.topk, gs.greedy, gs.seeds, gs.sstep)]
        assert rec[12:17] == [t.data_ptr() for t in (gs.topp, gs.minp, gs.presence, gs.frequency, gs.nlp)]
        assert (gs.temp.dtype, gs.topk.dtype, gs.greedy.dtype, gs.seeds.dtype, gs.sstep.dtype, gs.topp.dtype,
                gs.minp.dtype, gs.presence.dtype, gs.frequency.dtype, gs.nlp.dtype) == (
            torch.float32, torch.int32, torch.int32, torch.int64, torch.int64, torch.float32, torch.float32,
            torch.float32, torch.float32, torch.int32)
        # a fresh group idles at what apply_rows_kernel writes into pad rows
        assert [t[0].item() for t in (gs.temp, gs.topk, gs.greedy, gs.seeds, gs.sstep, gs.topp, gs.minp, gs.presence,
                                      gs.frequency, gs.nlp)] == [1, 1, 1, 0, 0, 1, 0, 0, 0, -1]
        assert len({rec[k] for k in (3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14, 15, 16)}) == 13
    else:
        assert rec[6:11] == [0] * 5
    assert rec[11] == (gs.tin.data_ptr() if first else 0)


VECS = ("slots", "pos", "active", "temp", "topk", "greedy", "seeds", "sstep", "topp", "minp", "presence",
        "frequency", "nlp")


def sentinel_group(w, cap):
    gs = GroupState(w, 0, cap)
    for name in VECS:
        if hasattr(gs, name):
            getattr(gs, name).fill_(SENT)
    if w.first:
        gs.tin.copy_(torch.arange(10, 10 + cap, dtype=torch.int32))
    return gs


@pytest.mark.parametrize("kind", list(SETS))
def test_torch_path_vectors_and_gather(kind):
    cap, n, b = 8, 3, 4
    w = _worker(True, True)
    gs = sentinel_group(w, cap)
    gs.cut, gs.pen, gs.lp = SETS[kind][0]
    rows = _rows(n, kind, src=[2, 0, 1])  # sources are rows this same change overwrites
    StageWorker._apply_rows_torch(w, gs, rows, b)

    def check(vec, live, idle):
        v = vec.tolist()
        assert v[:n] == live and v[n:b] == [idle] * (b - n) and v[b:] == [SENT] * (cap - b)

    f32 = lambda xs: np.asarray(xs, np.float32).tolist()  # noqa: E731
    check(gs.slots, [100, 101, 102], 99)
    check(gs.pos, [7, 10, 13], 0)
    check(gs.active, [1, 1, 1], 0)
    check(gs.temp, f32([r.temperature for r in rows]), 1.0)
    check(gs.topk, [40, 41, 42], 1)
    check(gs.greedy, [1, 0, 1], 1)
    check(gs.seeds, [r.seed for r in rows], 0)
    check(gs.sstep, [(1 << 32) + 5, (1 << 32) + 6, (1 << 32) + 7], 0)
    check(gs.topp, f32([r.top_p for r in rows]), 1.0)
    check(gs.minp, f32([r.min_p for r in rows]), 0.0)
    if kind in ("pen", "lp_pen", "lp_nopen"):
        check(gs.presence, f32([r.presence for r in rows]), 0.0)
        check(gs.frequency, f32([r.frequency for r in rows]), 0.0)
    else:
        assert (gs.presence == SENT).all() and (gs.frequency == SENT).all()
    if kind.startswith("lp"):
        check(gs.nlp, [0, 1, 2], -1)
    else:
        assert (gs.nlp == SENT).all()
    assert gs.tin.tolist() == [12, 10, 11, 10, 14, 15, 16, 17]  # pad row: index 0 of the old vector


def _r(**kw):
    return types.SimpleNamespace(**{"top_p": 1.0, "min_p": 0.0, "presence": 0.0, "frequency": 0.0, "logprobs": -1, **kw})


@pytest.mark.parametrize("rows,want", [
    ([], (False, False, False)),
    ([_r(), _r()], (False, False, False)),
    ([_r(), _r(top_p=0.9)], (True, False, False)),
    ([_r(min_p=0.1), _r()], (True, False, False)),
    ([_r(top_p=1.0, min_p=0.0)], (False, False, False)),
    ([_r(presence=0.5)], (False, True, False)),
    ([_r(), _r(frequency=-0.25)], (False, True, False)),
    ([_r(presence=-0.0, frequency=-0.0)], (False, False, False)),
    ([_r(logprobs=0)], (False, False, True)),
    ([_r(), _r(), _r(logprobs=3)], (False, False, True)),
    ([_r(top_p=0.5), _r(frequency=1.0), _r(logprobs=0)], (True, True, True)),
    ([_r(top_p=0.5, presence=1.0, logprobs=2), _r()], (True, True, True)),
])
def test_feature_pass(rows, want, monkeypatch):
    old = (any(r.top_p < 1.0 or r.min_p > 0.0 for r in rows),
           any(r.presence != 0.0 or r.frequency != 0.0 for r in rows), any(r.logprobs >= 0 for r in rows))
    assert old == want

    def no_alloc(*a, **k):
        raise AssertionError("the feature pass allocated a tensor")

    for fn in ("empty", "zeros", "ones", "full", "tensor"):
        monkeypatch.setattr(torch, fn, no_alloc)
    assert row_features(rows) == want


def _wire_plan(chunk_kw, row_kw):
    chunks = [Chunk(5, 6, 0, [11, 12, 13], True, 0.75, 30, False, (1 << 61) + 9, **chunk_kw[0]),
              Chunk(7, 8, 64, [14, 15], False, 0.5, 50, True, 3, **chunk_kw[1])]
    rows = [Row(1, 4, 9, 0.75, 40, False, (1 << 61) + 1, (1 << 40) + 2, 1, **row_kw[0]),
            Row(2, 5, 19, 0.25, 10, True, 7, 3, 0, **row_kw[1])]
    return GroupPlan(3, ret=2, n=2, b=2, ctxb=256, chunks=chunks, rows=rows)


C_INTS = [[5, 6, 0, 3, 1, 30, 0], [7, 8, 64, 2, 0, 50, 1]]
R_INTS = [[1, 4, 9, 40, 0, (1 << 61) + 1, (1 << 40) + 2, 1], [2, 5, 19, 10, 1, 7, 3, 0]]


@pytest.mark.parametrize("chunk_kw,row_kw,c_fl,r_fl,c_lp,r_lp", [
    (({}, {}), ({}, {}), [0.75, 0.5], [0.75, 0.25], None, None),
    (({}, {"min_p": 0.125}), ({"top_p": 0.5}, {}),
     [[0.75, 1.0, 0.0], [0.5, 1.0, 0.125]], [[0.75, 0.5, 0.0], [0.25, 1.0, 0.0]], None, None),
    (({"presence": 0.5}, {}), ({}, {"frequency": -1.5, "top_p": 0.75}),
     [[0.75, 1.0, 0.0, 0.5, 0.0], [0.5, 1.0, 0.0, 0.0, 0.0]],
     [[0.75, 1.0, 0.0, 0.0, 0.0], [0.25, 0.75, 0.0, 0.0, -1.5]], None, None),
    (({}, {"logprobs": 0}), ({}, {}), [0.75, 0.5], [0.75, 0.25], [-1, 0], None),
    (({}, {}), ({"logprobs": 4}, {}), [0.75, 0.5], [0.75, 0.25], None, [4, -1]),
])
def test_wire_arrays(chunk_kw, row_kw, c_fl, r_fl, c_lp, r_lp):
    gp = _wire_plan(chunk_kw, row_kw)
    packed = _pack_group(gp, True)
    assert packed[:7] == (3, 2, 2, 2, 256, "step", 0)
    (c_ints, c_floats, c_seeds, tok), (r_ints, r_floats) = packed[7], packed[8]

    def same(arr, want, dtype):
        want = np.array(want, dtype=dtype)
        assert arr.dtype == dtype and arr.shape == want.shape and (arr == want).all()

    same(c_ints, [r + [c] for r, c in zip(C_INTS, c_lp)] if c_lp else C_INTS, np.int64)
    same(r_ints, [r + [c] for r, c in zip(R_INTS, r_lp)] if r_lp else R_INTS, np.int64)
    same(c_floats, c_fl, np.float64)
    same(r_floats, r_fl, np.float64)
    same(c_seeds, [(1 << 61) + 9, 3], np.int64)
    same(tok, [11, 12, 13, 14, 15], np.int32)
    assert _unpack_group(*packed) == gp
    assert _pack_group(gp, False)[7][3] is None
