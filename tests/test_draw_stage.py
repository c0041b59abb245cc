"""DrawStage (parallel/draw.py): which backend passes run around the sampler,
in which order, for decode rows (`rows`, the body captured into the decode
graphs) and for a finished prompt's first draw (`finals`); what the launch
counters count; when the edit table is allocated and written.  A recording
backend stands in for the kernels; the expected sequences are those of the
code before DrawStage existed (StageWorker._sample_rows, _edit_finals,
_record_finals), which the same recorder was run against."""
import contextlib
import itertools
import types

import pytest
import torch

from llm_sharding_demo_amd.parallel.draw import DrawStage
from llm_sharding_demo_amd.parallel.pipeline import GroupState
from llm_sharding_demo_amd.runtime.plan import Chunk

CAP, B, V, L, SLOTS = 4, 2, 16, 8, 4
FLAGS = list(itertools.product((False, True), repeat=4))


class Recorder:
    """Backend that records (method, `back` where there is one) per call, and
    the edit table's counts as each pass that reads the table saw them."""

    def __init__(self):
        self.calls, self.draw, self.samp, self.args = [], None, None, {}

    def _counts(self):
        tab = self.draw.edit_tab
        return None if tab is None else tab[0].tolist()

    def penalize(self, logits, hist, slots, counts, presence, frequency, vocab):
        self.calls.append(("penalize", None))
        self.args["penalize"] = (hist, counts)

    def logit_edits(self, logits, table, slots, step, vocab):
        self.calls.append(("logit_edits", None))
        self.args["logit_edits"] = (table, slots.tolist(), step, self._counts())

    def sample_into(self, logits, samp, vocab, out, meta):
        self.calls.append(("sample_into", None))
        self.samp = samp
        out.zero_()

    def sample(self, logits, state, vocab):
        self.calls.append(("sample", None))
        self.args["sample"] = self._counts()
        return torch.zeros(logits.shape[0], dtype=torch.int32)

    def record_tokens(self, hist, slots, step, tokens, active=None, back=0):
        self.calls.append(("record_tokens", back))
        self.args["record_tokens"] = (hist, slots.tolist(), step, active)

    def logprobs(self, logits, tokens, nlp, slots, step, active, rec, vocab, back=0):
        self.calls.append(("logprobs", back))
        self.args["logprobs"] = (nlp.tolist(), slots.tolist(), step, active, rec)


def _no_staging(gs, arr, dst):
    raise AssertionError("the pinned staging ring is for GPUs")


def _draw():
    be = Recorder()
    stage = types.SimpleNamespace(backend=be, device=torch.device("cpu"), max_seq=L,
                                  cfg=types.SimpleNamespace(vocab_size=V))
    d = be.draw = DrawStage(stage, SLOTS, _no_staging, contextlib.nullcontext)
    return d, be


def _group():
    w = types.SimpleNamespace(device=torch.device("cpu"), H=4, scratch_slot=SLOTS - 1, first=True, last=True, P=1)
    return GroupState(w, 0, CAP)


def _counters(d):
    return d.penalty_launches, d.logprob_launches, d.logit_edit_launches


def test_nothing_until_asked():
    d, be = _draw()
    d.prepare((True, False, False, False))  # a top-p / min-p cut needs no table
    assert d.pen_hist is None and d.lp_rec is None and d.edit_tab is None
    assert _counters(d) == (0, 0, 0) and be.calls == []
    assert (d.max_logprobs, d.max_logit_edits) == (5, 300)


@pytest.mark.parametrize("cut,pen,lp,edit", FLAGS)
def test_rows_order(cut, pen, lp, edit):
    d, be = _draw()
    gs = _group()
    gs.cut, gs.pen, gs.lp, gs.edit = cut, pen, lp, edit
    d.prepare((cut, pen, lp, edit))
    assert (d.pen_hist is not None, d.lp_rec is not None, d.edit_tab is not None) == (pen, lp, edit)
    d.rows(gs, torch.zeros(B, V), B, None)
    assert be.calls == ([("penalize", None)] * pen + [("logit_edits", None)] * edit + [("sample_into", None)]
                        + [("record_tokens", 1)] * pen + [("logprobs", 1)] * lp)
    assert _counters(d) == (0, 0, 0)  # the caller counts: one count() per issued item, replays included
    # cut decides only whether the sampler gets the top-p / min-p vectors
    assert (be.samp.top_p is not None, be.samp.min_p is not None) == (cut, cut)
    assert be.samp.num_rows == B and be.samp.step.data_ptr() == gs.sstep.data_ptr()
    # every pass works on the tables DrawStage owns and on the draw's own counters
    if pen:
        assert be.args["penalize"][0] is d.pen_hist and be.args["record_tokens"][0] is d.pen_hist
        assert be.args["penalize"][1].data_ptr() == gs.sstep.data_ptr()
    if edit:
        assert be.args["logit_edits"][0] is d.edit_tab and be.args["logit_edits"][2].data_ptr() == gs.sstep.data_ptr()
    if lp:
        assert be.args["logprobs"][4] is d.lp_rec and be.args["logprobs"][2].data_ptr() == gs.sstep.data_ptr()
    d.count(gs)
    d.count(gs)
    assert _counters(d) == (2 * pen, 2 * lp, 2 * edit)


EDITS = ((3, 9), (-2.5, float("-inf")), (0, 4))  # (tokens, values, untils)


def _chunks(pen, lp, ed):
    """Two final chunks on slots 1 and 2: the first carries the features, the
    second none."""
    a = Chunk(seq=0, slot=1, start=0, ids=[5, 6], final=True, presence=0.5 if pen else 0.0,
              logprobs=2 if lp else -1, nedits=2 if ed else 0, edits=EDITS if ed else None)
    return [a, Chunk(seq=1, slot=2, start=0, ids=[7], final=True)]


@pytest.mark.parametrize("pen,lp,ed,table", FLAGS)
def test_finals_order_counters_and_table(pen, lp, ed, table):
    d, be = _draw()
    if table:  # an earlier request had edits; slots 1 and 2 still hold its counts
        d.prepare((False, False, False, True))
        d.edit_tab[0].fill_(7)
    fc = _chunks(pen, lp, ed)
    ids = d.finals(_group(), fc, torch.zeros(2, V))
    assert ids.tolist() == [0, 0]
    assert be.calls == ([("logit_edits", None)] * ed + [("sample", None)] + [("record_tokens", 0)] * pen
                        + [("logprobs", 0)] * lp)
    assert _counters(d) == (int(pen), int(lp), int(ed))
    if not (ed or table):
        assert d.edit_tab is None  # no edits and no table: nothing allocated, nothing written
    else:
        want = [7 if table else 0, 2 if ed else 0, 0, 7 if table else 0]  # both chunks wrote, zero included
        cnt, tok, val, until = d.edit_tab
        assert cnt.tolist() == want
        assert be.args["sample"] == want  # written ahead of the draw ...
        if ed:  # ... and ahead of the edit pass, which reads the chunks' slots and no counter
            table_seen, slots, step, counts = be.args["logit_edits"]
            assert table_seen is d.edit_tab and slots == [1, 2] and step is None and counts == want
            assert tok[1, :2].tolist() == [3, 9] and until[1, :2].tolist() == [0, 4]
            assert val[1, :2].tolist() == [-2.5, float("-inf")]
            assert not tok[2].any() and not val[2].any() and not until[2].any()
    if pen:
        hist, slots, step, active = be.args["record_tokens"]
        assert hist is d.pen_hist and slots == [1, 2] and step is None and active is None
    else:
        assert d.pen_hist is None
    if lp:
        nlp, slots, step, active, rec = be.args["logprobs"]
        assert nlp == [2, -1] and slots == [1, 2] and step is None and active is None and rec is d.lp_rec
    else:
        assert d.lp_rec is None


@pytest.mark.parametrize("nedits,edits,limit", [(2, None, 300), (2, ((3,), (1.0,), (0,)), 300), (2, EDITS, 1)])
def test_finals_rejects_missing_or_oversized_edits(nedits, edits, limit):
    d, be = _draw()
    d.max_logit_edits = limit
    fc = [Chunk(seq=0, slot=1, start=0, ids=[5], final=True, nedits=nedits, edits=edits)]
    with pytest.raises(ValueError, match="max_logit_edits"):
        d.finals(_group(), fc, torch.zeros(1, V))
    assert be.calls == [] and _counters(d) == (0, 0, 0) and not d.edit_tab[0].any()


def test_fetch_logprobs_shapes():
    d, _ = _draw()
    d.max_logprobs = 3
    d.prepare((False, False, True, False))
    d.lp_rec[0][2, :5] = torch.arange(5.0)
    tok, top_id, top = d.fetch_logprobs(2, 5)
    assert tok.tolist() == [0, 1, 2, 3, 4] and top_id.shape == (5, 3) and top.shape == (5, 3)
    assert top_id.dtype == torch.int32 and top.dtype == torch.float32
