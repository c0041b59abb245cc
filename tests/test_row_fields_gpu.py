"""The host packer against the kernel that reads its buffer: plan.pack_rows
and GroupState.rows_record feed apply_rows (csrc/kernels/elementwise.hip) on
an MI355X, and every row vector and the gathered input tokens must equal,
exactly, what the torch path writes into CPU copies of the same vectors."""
import types

import numpy as np
import pytest
import torch

from llm_sharding_demo_amd.parallel.pipeline import StageWorker
from llm_sharding_demo_amd.runtime.plan import pack_rows

from .test_row_fields import SETS, VECS, _rows, _worker, sentinel_group

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def C():
    from llm_sharding_demo_amd.ops.hip import _load

    return _load()


@pytest.mark.parametrize("cap,b,n", [(64, 32, 21), (8, 8, 8)])
@pytest.mark.parametrize("kind", list(SETS))
@pytest.mark.parametrize("first,last", [(True, True), (False, True), (True, False)])
def test_packer_feeds_kernel(C, cap, b, n, kind, first, last):
    feats = SETS[kind][0] if last else (False, False, False)
    src = np.random.default_rng(n).integers(0, cap, n).tolist()  # any entry of the old vector, rows [0, b) included
    rows = _rows(n, kind, src=src)
    wc, wg = _worker(first, last), _worker(first, last)
    wg.device = torch.device("cuda")
    ref, gs = sentinel_group(wc, cap), sentinel_group(wg, cap)
    ref.cut, ref.pen, ref.lp = gs.cut, gs.pen, gs.lp = feats
    StageWorker._apply_rows_torch(wc, ref, rows, b)

    rec = gs.rows_record(wg)
    a = np.zeros(gs.rows_dev.numel(), np.int32)
    words, nargs = pack_rows(rows, cap, first, last, feats, a)
    assert words <= gs.rows_dev.numel() and nargs <= rec.numel() and b <= cap
    gs.rows_dev[:words].copy_(torch.from_numpy(a[:words]))
    C.apply_rows(rec[:nargs], b)
    torch.cuda.synchronize()
    # the torch path on the GPU (one staged copy through the pinned ring) writes the same
    wg._PF_PIN = StageWorker._PF_PIN
    wg._stage_h2d = types.MethodType(StageWorker._stage_h2d, wg)
    staged = sentinel_group(wg, cap)
    staged.cut, staged.pen, staged.lp = feats
    StageWorker._apply_rows_torch(wg, staged, rows, b)
    torch.cuda.synchronize()
    for name in VECS + ("tin",):
        if hasattr(ref, name):
            want = getattr(ref, name)
            bits = torch.int64 if want.dtype == torch.int64 else torch.int32
            for path, g in (("kernel", gs), ("staged", staged)):
                got = getattr(g, name).cpu()
                assert got.dtype == want.dtype and torch.equal(got.view(bits), want.view(bits)), (path, name)
