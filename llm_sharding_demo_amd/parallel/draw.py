"""What happens to a row's logits between `lm_head` and the returned token.

A `StageWorker` (parallel/pipeline.py) moves a step through its stage; its
`DrawStage` decides what runs on the logits of the last stage: the repetition
pass, the bad-words pass, the penalty pass, the logit edits, the allowed-token
mask, the guide's mask, the sampler, the guide's step, the token history, the
context and the logprob records, for the decode rows of a group (`rows`,
captured into the decode graphs) and for the first draw of a finished prompt
(`finals`, eager); `chunks` copies the prompts that the repetition pass reads
into its table as they are prefilled.  It owns the six per-KV-slot tables and
the guide table these passes read and write, and counts the items that ran each pass.  Every
stage has one; off the last stage it stays empty.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
import torch

from ..runtime.batch import SamplingState
from ..runtime.plan import has_allow, has_bad, has_context, has_edits, has_guide, row_features
from ..utils import racecheck


class DrawStage(racecheck.Shared):
    def __init__(self, stage, slots: int, stage_h2d: Callable, gpu: Callable):
        """`stage`: the StageModel (backend, device, vocabulary, max_seq --
        read at each call: a test may wrap the backend after construction);
        `slots`: KV slots, scratch and compat included; `stage_h2d(gs, host
        int32 array, device tensor)`: the worker's pinned staging copy;
        `gpu()`: the worker's shared hold on the capture gate."""
        self.stage = stage
        self.slots = slots
        self._stage_h2d, self._gpu = stage_h2d, gpu
        # per-KV-slot tables, each allocated when the first request that needs
        # it arrives (_hist, _lp_rec, _edit_tab), beside the items whose
        # sampler ran with that pass around it
        self.pen_hist: Optional[torch.Tensor] = None  # generated tokens, by the draw's sampler counter
        self.penalty_launches = 0
        self.lp_rec: Optional[tuple] = None  # logprob records, indexed like the history, W = max_logprobs wide
        self.max_logprobs = 5
        self.logprob_launches = 0
        self.edit_tab: Optional[tuple] = None  # logit_bias / banned tokens / min_new_tokens, E = max_logit_edits
        self.max_logit_edits = 300
        self.logit_edit_launches = 0
        self.ctx_tab: Optional[tuple] = None  # repetition_penalty / no_repeat_ngram_size and prompt + generated tokens
        self.repetition_launches = 0
        self.allow_tab: Optional[tuple] = None  # allowed_token_ids: a flag and a bitmask over the logits' columns
        self.allow_launches = 0
        self.bad_tab: Optional[tuple] = None  # bad_words: the sequences back to back, N = max_bad_words, T = max_bad_word_tokens
        self.max_bad_words, self.max_bad_word_tokens = 64, 512
        self.bad_words_launches = 0
        self.guide_tab: Optional[tuple] = None  # guide: G guides' classes and cells, and (guide row, state) per KV slot
        self.max_guides, self.max_guide_cells = 8, 1 << 18
        self.guide_launches = 0
        self._guide_lock = racecheck.Lock("draw.guide")  # the table is first asked for by a submitting thread (load_guide)

    # ------------------------------------------------------------------
    # tables
    def _hist(self) -> torch.Tensor:
        """Generated-token history, [KV slots (scratch and compat included),
        max_seq] int32.  Entries at or past a row's sampler counter are never
        read, so it needs no initial value and a reused slot no clearing."""
        if self.pen_hist is None:
            L, dev = self.stage.max_seq, self.stage.device
            if L > 8192 and dev.type == "cuda":
                raise ValueError(f"presence / frequency penalties: max_seq_len {L} exceeds the 8192-token "
                                 "history the penalty kernel's LDS table holds")
            # no fill: one enqueued on this lane could land after another lane's first record
            self.pen_hist = torch.empty(self.slots, L, dtype=torch.int32, device=dev)
        return self.pen_hist

    def _lp_rec(self) -> tuple:
        """Logprob records: (lp_tok [KV slots, max_seq] fp32, lp_top_id [.., W]
        int32, lp_top [.., W] fp32), record j of a slot = the draw with sampler
        counter j.  Records at or past a sequence's token count are never
        fetched, so no initial value and no clearing."""
        if self.lp_rec is None:
            S, L, W, dev = self.slots, self.stage.max_seq, self.max_logprobs, self.stage.device
            # no fill: one enqueued on this lane could land after another lane's first record
            self.lp_rec = (torch.empty(S, L, dtype=torch.float32, device=dev),
                           torch.empty(S, L, W, dtype=torch.int32, device=dev),
                           torch.empty(S, L, W, dtype=torch.float32, device=dev))
        return self.lp_rec

    def _edit_tab(self) -> tuple:
        """Logit-edit table: (cnt [KV slots, scratch and compat included]
        int32, tok [.., E] int32, val [.., E] fp32, until [.., E] int32), E =
        max_logit_edits.  Unlike the history and the logprob records its stale
        contents ARE read: a group whose rows joined before the table existed
        runs the edit pass once a row with edits joins it, and reads its other
        rows' counts.  So the counts start at zero, and visibly to every lane:
        this thread waits for the fill before anything that reads the table can
        be enqueued, on this lane or another (_hist: a fill merely enqueued
        here could land after another lane's reader).  Allocated once, outside
        any capture, and never reallocated: captured graphs hold its addresses.
        From then on every final chunk writes its slot's count (finals)."""
        if self.edit_tab is None:
            S, E, dev = self.slots, self.max_logit_edits, self.stage.device
            self.edit_tab = (torch.zeros(S, dtype=torch.int32, device=dev),
                             torch.zeros(S, E, dtype=torch.int32, device=dev),
                             torch.zeros(S, E, dtype=torch.float32, device=dev),
                             torch.zeros(S, E, dtype=torch.int32, device=dev))
            if dev.type == "cuda":
                torch.cuda.current_stream(dev).synchronize()
        return self.edit_tab

    def _ctx_tab(self) -> tuple:
        """Context table: (plen [KV slots, scratch and compat included] int32,
        rpen [..] fp32, ngram [..] int32, tok [.., max_seq] int32): a slot's
        prompt length, repetition_penalty, no_repeat_ngram_size, and its
        prompt followed by its generated tokens.  Like the edit table's counts
        its stale parameters ARE read -- by the other rows of a group with a
        flagged row, and by every pad row on the scratch slot -- so they start
        at "off" (0, 1.0, 0), visibly to every lane: this thread waits for the
        fill (_edit_tab).  Allocated once, outside any capture, and never
        reallocated: captured graphs hold its addresses.  From then on every
        first chunk of a prompt writes its slot's parameters (chunks)."""
        if self.ctx_tab is None:
            S, L, dev = self.slots, self.stage.max_seq, self.stage.device
            if L > 8192 and dev.type == "cuda":
                raise ValueError(f"repetition_penalty / no_repeat_ngram_size: max_seq_len {L} exceeds the "
                                 "8192-token context the repetition kernel's LDS key set holds")
            self.ctx_tab = (torch.zeros(S, dtype=torch.int32, device=dev),
                            torch.ones(S, dtype=torch.float32, device=dev),
                            torch.zeros(S, dtype=torch.int32, device=dev),
                            torch.zeros(S, L, dtype=torch.int32, device=dev))
            if dev.type == "cuda":
                torch.cuda.current_stream(dev).synchronize()
        return self.ctx_tab

    def _allow_tab(self) -> tuple:
        """Allowed-token table: (on [KV slots, scratch and compat included]
        int32, bits [.., W] int32), W = one bit per column of the padded
        vocabulary: token t of a slot is allowed when bit t & 31 of word t >> 5
        is set, and the mask pass touches only rows whose slot has on != 0.
        Like the edit table's counts its stale flags ARE read -- by the other
        rows of a group with an asking row, and by every pad row on the
        scratch slot -- so they start at zero, visibly to every lane: this
        thread waits for the fill (_edit_tab).  Allocated once, outside any
        capture, and never reallocated: captured graphs hold its addresses.
        From then on every final chunk writes its slot's flag (finals)."""
        if self.allow_tab is None:
            S, dev = self.slots, self.stage.device
            W = (self.stage.cfg.vocab_padded + 31) // 32
            self.allow_tab = (torch.zeros(S, dtype=torch.int32, device=dev),
                              torch.zeros(S, W, dtype=torch.int32, device=dev))
            if dev.type == "cuda":
                torch.cuda.current_stream(dev).synchronize()
        return self.allow_tab

    def _bad_tab(self) -> tuple:
        """Bad-words table: (cnt [KV slots, scratch and compat included]
        int32, end [.., N] int32, tok [.., T] int32), N = max_bad_words, T =
        max_bad_word_tokens: sequence e < cnt of a slot is tok[end[e - 1] ..
        end[e]) of its row (end[-1] = 0), and the bad-words pass touches only
        rows whose slot has cnt != 0.  Like the edit table's counts its stale
        counts ARE read -- by the other rows of a group with an asking row,
        and by every pad row on the scratch slot -- so they start at zero,
        visibly to every lane: this thread waits for the fill (_edit_tab).
        Allocated once, outside any capture, and never reallocated: captured
        graphs hold its addresses.  From then on every final chunk writes its
        slot's count (finals)."""
        if self.bad_tab is None:
            S, N, T, dev = self.slots, self.max_bad_words, self.max_bad_word_tokens, self.stage.device
            self.bad_tab = (torch.zeros(S, dtype=torch.int32, device=dev),
                            torch.zeros(S, N, dtype=torch.int32, device=dev),
                            torch.zeros(S, T, dtype=torch.int32, device=dev))
            if dev.type == "cuda":
                torch.cuda.current_stream(dev).synchronize()
        return self.bad_tab

    def _guide_tab(self) -> tuple:
        """Guide table: (gcls [G, Vp] int16, gnext [G, max_guide_cells] int16,
        gdim [G, 2] int32, gsl [KV slots, scratch and compat included, 2]
        int32), G = max_guides: row g holds one TokenGuide -- the class of
        every column of the padded vocabulary (columns at or past the
        vocabulary: 0), its next[S, C] row-major, (S, C) -- and gsl[s] = (the
        guide row the request on slot s follows or -1, its current state).
        G x (2 Vp + 2 max_guide_cells + 8) + 8 x slots bytes.  Like the edit
        table's counts the stale entries of gsl ARE read -- by the other rows
        of a group with a guided row, and by every pad row on the scratch slot
        -- so they start at (-1, 0), "off", and the guide rows at zero, visibly
        to every lane: this thread waits for the fill (_edit_tab).  Allocated
        once, outside any capture, and never reallocated: captured graphs hold
        its addresses.  From then on every final chunk writes its slot's entry
        (finals), and the engine writes a guide's row before the first request
        that follows it is planned (load_guide)."""
        with self._guide_lock:
            if self.guide_tab is None:
                S, G, dev = self.slots, self.max_guides, self.stage.device
                gsl = torch.zeros(S, 2, dtype=torch.int32, device=dev)
                gsl[:, 0] = -1
                tab = (torch.zeros(G, self.stage.cfg.vocab_padded, dtype=torch.int16, device=dev),
                       torch.zeros(G, self.max_guide_cells, dtype=torch.int16, device=dev),
                       torch.zeros(G, 2, dtype=torch.int32, device=dev), gsl)
                if dev.type == "cuda":
                    torch.cuda.current_stream(dev).synchronize()
                self.guide_tab = tab
            return self.guide_tab

    def load_guide(self, row: int, guide) -> None:
        """Write `guide` (a validated TokenGuide) into row `row` of the guide
        table.  For the engine's submitting thread, before the first request
        that follows the guide is handed to the scheduler.  The row's contents
        are never rewritten while an enqueued or in-flight kernel can read
        them: the engine reuses a row only when no request pins it, and a
        request unpins its row when its KV slot is released -- after the
        tokens of the last item that held one of its rows were read back, and
        guide_advance is enqueued ahead of the token return, so by then
        nothing reads the row; a stale gsl entry that still names it belongs
        to a free slot, which no row of a plan uses until a final chunk has
        rewritten the entry.  The copy is waited for here, and the whole runs
        under a shared hold of the capture gate (a sibling stage thread may be
        capturing), as fetch_logprobs does."""
        dev = self.stage.device
        with self._gpu():
            gcls, gnext, gdim, _ = self._guide_tab()
            S, C, V = guide.S, guide.C, guide.vocab
            if not 0 <= row < gcls.shape[0] or V > gcls.shape[1] or S * C > gnext.shape[1]:
                raise ValueError(f"guide: row {row}, vocabulary {V} or {S} x {C} cells do not fit the guide table "
                                 f"({gcls.shape[0]} rows, {gcls.shape[1]} columns, {gnext.shape[1]} cells)")
            cls = np.zeros(gcls.shape[1], dtype=np.int16)
            cls[:V] = guide.cls
            gcls[row].copy_(torch.from_numpy(cls))
            gnext[row, : S * C].copy_(torch.from_numpy(np.ascontiguousarray(guide.next).reshape(-1)))
            gdim[row].copy_(torch.tensor([S, C], dtype=torch.int32))
            if dev.type == "cuda":
                torch.cuda.current_stream(dev).synchronize()

    def prepare(self, feats: tuple) -> None:
        """A composition with the features (cut, pen, lp, edit[, ctx[, allow[,
        bad[, guide]]]]) is being applied: what they need -- the token history,
        the logprob records, the edit table, the context table, the
        allowed-token table, the bad-words table, the guide table -- allocated
        here, on the host side of the change (never inside a capture)."""
        _, pen, lp, edit, *more = feats
        if more and more[0]:
            self._ctx_tab()
        if more[1:] and more[1]:
            self._allow_tab()
        if more[2:] and more[2]:
            self._ctx_tab()
            self._bad_tab()
        if more[3:] and more[3]:
            self._guide_tab()
        if pen:
            self._hist()
        if lp:
            self._lp_rec()
        if edit:
            self._edit_tab()

    def fetch_logprobs(self, slot: int, n: int) -> tuple:
        """Host copies of records [0, n) of KV slot `slot`: (lp_tok [n],
        lp_top_id [n, W], lp_top [n, W]).  For the coordinator thread, once it
        has read the n-th token back: each record is written ahead of its
        token's return in stream order.  Holds the capture gate shared (a
        sibling stage thread may be capturing)."""
        rec = self._lp_rec()
        with self._gpu():
            return tuple(t[slot, :n].cpu() for t in rec)

    # ------------------------------------------------------------------
    def count(self, gs) -> None:
        """One decode item of group `gs` was issued -- eagerly, captured or as
        a replayed graph: count the passes that ran around its sampler."""
        if gs.pen:
            self.penalty_launches += 1
        if gs.lp:
            self.logprob_launches += 1
        if gs.edit:
            self.logit_edit_launches += 1
        if gs.ctx:
            self.repetition_launches += 1
        if gs.allow:
            self.allow_launches += 1
        if gs.bad:
            self.bad_words_launches += 1
        if gs.guide:
            self.guide_launches += 1

    def chunks(self, gs, chunks) -> None:
        """Prefill chunks are about to run on the last stage (every prefill
        item, eager or replayed; never inside a capture).  Nothing while no
        context table exists and no chunk asks for one.  Once it exists every
        chunk that opens a prompt (start == 0, or a fork's chunk: Chunk.opens)
        writes its slot's (plen, rpen, ngram), the defaults included -- a
        request that reuses a slot must not inherit its predecessor's -- and
        every chunk that asks writes its token ids to
        tok[slot, start : start + qlen].  ONE host-to-device copy through the
        group's pinned staging ring: [slots H | plen H | rpen bits H | ngram H]
        of the H opening chunks, then [flat table index T | ids T]."""
        flagged = [c for c in chunks if c.ctx and c.qlen]
        if self.ctx_tab is None and not flagged:
            return
        plen, rpen, ngram, tok = self._ctx_tab()
        heads = [c for c in chunks if c.opens]
        if not heads and not flagged:
            return
        L = tok.shape[1]
        for c in flagged:
            # a fork's chunk (SamplingParams.n): the prompt's ids [0, start) are
            # the source slot's, cloned on the device -- the source's own chunks
            # wrote them on this lane, in an earlier item -- and the chunk's own
            # id lands behind them below
            if c.fork >= 0 and c.start > 0:
                if not (0 <= c.fork < self.slots and 0 <= c.slot < self.slots and c.start < L):
                    raise ValueError("a fork chunk's slots or start lie outside the context table")
                tok[c.slot, : c.start].copy_(tok[c.fork, : c.start])
        for c in flagged:
            if isinstance(c.ids, range) or c.start + c.qlen > L or not 0 <= c.slot < self.slots:
                raise ValueError("a prefill chunk with repetition_penalty / no_repeat_ngram_size reached the last "
                                 f"stage without its token ids, or past max_seq_len = {L}")
        cols = [[c.slot for c in heads], [c.plen for c in heads],
                np.array([c.rpen for c in heads], dtype=np.float32).view(np.int32), [c.ngram for c in heads]]
        if flagged:
            cols += [np.concatenate([c.slot * L + c.start + np.arange(c.qlen) for c in flagged]),
                     [t for c in flagged for t in c.ids]]
        arr = np.concatenate([np.asarray(c, dtype=np.int32) for c in cols])
        dev = self.stage.device
        if dev.type == "cuda":
            buf = torch.empty(arr.size, dtype=torch.int32, device=dev)
            self._stage_h2d(gs, arr, buf)
        else:
            buf = torch.from_numpy(arr)
        slots, pl, rp, ng, *ids = buf.split([len(c) for c in cols])
        if heads:
            at = slots.long()
            plen.index_copy_(0, at, pl)
            rpen.index_copy_(0, at, rp.view(torch.float32))
            ngram.index_copy_(0, at, ng)
        if ids:
            tok.view(-1).index_copy_(0, ids[0].long(), ids[1])

    def rows(self, gs, logits: torch.Tensor, b: int, meta) -> None:
        """Decode rows of a group: draw into the token-return vector, advance
        the sampler counters and positions.  A composition with a penalised
        row runs penalize and record_tokens around the sampler.  One with an
        edited row runs the edit pass right ahead of the sampler (after the
        penalties; the counters it compares are the ones the draw uses).  One
        with a logprob row then runs the logprob kernel over the logits the
        sampler drew from.  One with a repetition penalty or an n-gram ban runs
        the repetition pass first of all, and record_context behind the draw.
        One with a row that gave allowed_token_ids runs the mask pass last of
        the edits: the sampler and the logprob kernel see the masked logits.
        One with a row that gave bad_words -- a context row too -- runs the
        bad-words pass right after the repetition pass, which reads the same
        context.  One with a row that follows a guide runs the guide's mask
        right after the allowed-token mask -- the last edit: the sampler and
        the logprob kernel see it -- and the guide's step behind the sampler,
        beside the records and ahead of the token return.  Any other runs the
        sampler alone."""
        be, V = self.stage.backend, self.stage.cfg.vocab_size
        slots, step, out = gs.slots[:b], gs.sstep[:b], gs.tokret[:b]
        if gs.ctx:
            be.repetition(logits, self.ctx_tab, slots, step, V)
        if gs.bad:
            be.bad_words(logits, self.bad_tab, self.ctx_tab, slots, step, V)
        if gs.pen:
            be.penalize(logits, self.pen_hist, slots, step, gs.presence[:b], gs.frequency[:b], V)
        if gs.edit:
            be.logit_edits(logits, self.edit_tab, slots, step, V)
        if gs.allow:
            be.allow_mask(logits, self.allow_tab, slots, V)
        if gs.guide:
            be.guide_mask(logits, self.guide_tab, slots, V)
        be.sample_into(logits, gs.samp(b), V, out, meta)
        if gs.guide:
            be.guide_advance(self.guide_tab, slots, out, V, gs.active[:b])
        if gs.pen:
            # the sampler has advanced the counters: the draw used counter - 1
            be.record_tokens(self.pen_hist, slots, step, out, gs.active[:b], 1)
        if gs.ctx:
            be.record_context(self.ctx_tab, slots, step, out, gs.active[:b], 1)
        if gs.lp:
            be.logprobs(logits, out, gs.nlp[:b], slots, step, gs.active[:b], self.lp_rec, V, 1)

    def finals(self, gs, fc, logits: torch.Tensor) -> torch.Tensor:
        """First generated token (draw 0) of the final chunks `fc`, drawn from
        `logits`.  Eager, on the item's lane, outside any graph.  Ahead of the
        draw their logit edits go into their KV slots' table rows and the edit
        pass runs over `logits`: nothing without a table and without edits;
        once the table exists every final chunk writes its slot's count, zero
        included -- a request that reuses a slot must not inherit its
        predecessor's entries.  Behind it the token goes into the history when
        a chunk carries a penalty (its history is empty, so this draw needs no
        penalty pass), and its logprob record is taken from `logits` when one
        asked.  A chunk with a repetition penalty or an n-gram ban runs the
        repetition pass first of all -- over its prompt, which `chunks` has
        put into the context table -- and the token goes in behind the prompt.
        The allowed-token table goes like the edit table: nothing without a
        table and without an asking chunk; once it exists every final chunk
        writes its slot's flag, zero included, an asking one its mask words too,
        and the mask pass runs last ahead of the draw.  So does the bad-words
        table: every final chunk writes its slot's count, zero included, an
        asking one its end offsets and tokens too, and the bad-words pass
        runs right after the repetition pass, over the prompt.  The guide
        table likewise: once it exists every final chunk writes its slot's
        entry, (its guide's row or -1, state 0) -- a request that reuses a slot
        inherits nothing -- the guide's mask runs with the start state last
        ahead of the draw, and the guide's step behind it."""
        be, V, dev = self.stage.backend, self.stage.cfg.vocab_size, self.stage.device
        _, pen, lp = row_features(fc)
        ed, cx, al, bw, gd = has_edits(fc), has_context(fc), has_allow(fc), has_bad(fc), has_guide(fc)
        tab = self._edit_tab() if ed or self.edit_tab is not None else None
        atab = self._allow_tab() if al or self.allow_tab is not None else None
        btab = self._bad_tab() if bw or self.bad_tab is not None else None
        gtab = self._guide_tab() if gd or self.guide_tab is not None else None
        slots = nlp = None
        if tab is not None or atab is not None or btab is not None or gtab is not None or pen or lp or cx:
            slots, nlp = self._stage_finals(gs, fc, tab, atab, btab, gtab)
        if cx:
            be.repetition(logits, self._ctx_tab(), slots, None, V)
            self.repetition_launches += 1
        if bw:
            be.bad_words(logits, btab, self._ctx_tab(), slots, None, V)
            self.bad_words_launches += 1
        if ed:
            be.logit_edits(logits, tab, slots, None, V)
            self.logit_edit_launches += 1
        if al:
            be.allow_mask(logits, atab, slots, V)
            self.allow_launches += 1
        if gd:
            be.guide_mask(logits, gtab, slots, V)
            self.guide_launches += 1
        ids = be.sample(logits, SamplingState.of(fc, dev), V)
        if gd:
            be.guide_advance(gtab, slots, ids, V, None)
        if pen:
            be.record_tokens(self._hist(), slots, None, ids, None, 0)
            self.penalty_launches += 1
        if cx:
            be.record_context(self.ctx_tab, slots, None, ids, None, 0)
        if lp:
            be.logprobs(logits, ids, nlp, slots, None, None, self._lp_rec(), V, 0)
            self.logprob_launches += 1
        return ids

    def _stage_finals(self, gs, fc, tab: Optional[tuple], atab: Optional[tuple] = None,
                      btab: Optional[tuple] = None, gtab: Optional[tuple] = None) -> tuple:
        """What the passes around the first draw of `fc` read, on the device
        in ONE host-to-device copy through the group's pinned staging ring:
        [slots J | logprob widths J | edit counts J], then with n edits among
        them [flat table index n | tokens n | value bits n | untils n].  With
        a table, its rows are written from the copy.  With an allowed-token
        table `atab` then [allow flags J], and with k asking chunks among them
        [their slots k | their mask words k W]; its flags and rows are written
        from the copy too.  With a bad-words table `btab` then [sequence
        counts J], and with m sequences of t tokens among them [flat end index
        m | end offsets m | flat token index t | tokens t], written likewise.
        With a guide table `gtab` then [guide rows J | states J] (the chunk's
        guide row or -1, 0), written to the slots' entries.
        -> (slots, widths)."""
        cols = [[c.slot for c in fc], [c.logprobs for c in fc], [c.nedits for c in fc]]
        if tab is not None:
            cnt, tok, val, until = tab
            E = tok.shape[1]
            if any(c.nedits and (c.edits is None or len(c.edits[0]) != c.nedits or c.nedits > E) for c in fc):
                raise ValueError(f"a final chunk's logit edits are missing or exceed max_logit_edits = {E}")
            ent = [c.edits for c in fc if c.nedits]
            if ent:
                cols += [np.concatenate([c.slot * E + np.arange(c.nedits) for c in fc if c.nedits]),
                         [t for e in ent for t in e[0]],
                         np.array([v for e in ent for v in e[1]], dtype=np.float32).view(np.int32),
                         [u for e in ent for u in e[2]]]
        ask = []
        if atab is not None:
            on, bits = atab
            W = bits.shape[1]
            ask = [c for c in fc if c.allow]
            if any(c.mask is None or len(c.mask) != 4 * W or not 0 <= c.slot < self.slots for c in ask):
                raise ValueError(f"a final chunk's allowed-token mask is missing or not {W} words long")
            cols += [[1 if c.allow else 0 for c in fc]]
            if ask:
                cols += [[c.slot for c in ask], np.frombuffer(b"".join(c.mask for c in ask), dtype=np.int32)]
        words = []
        if btab is not None:
            bcnt, bend, btok = btab
            N, T = bend.shape[1], btok.shape[1]
            words = [c for c in fc if c.nbad]
            if any(c.bad is None or len(c.bad[0]) != c.nbad or c.nbad > N or len(c.bad[1]) > T
                   or len(c.bad[1]) != c.bad[0][-1] or not 0 <= c.slot < self.slots for c in words):
                raise ValueError("a final chunk's bad_words are missing or exceed max_bad_words = "
                                 f"{N} / max_bad_word_tokens = {T}")
            cols += [[c.nbad for c in fc]]
            if words:
                cols += [np.concatenate([c.slot * N + np.arange(c.nbad) for c in words]),
                         [e for c in words for e in c.bad[0]],
                         np.concatenate([c.slot * T + np.arange(len(c.bad[1])) for c in words]),
                         [t for c in words for t in c.bad[1]]]
        if gtab is not None:
            if any(not -1 <= c.guide < gtab[0].shape[0] or not 0 <= c.slot < self.slots for c in fc):
                raise ValueError(f"a final chunk's guide row lies outside the guide table's {gtab[0].shape[0]} rows")
            cols += [[c.guide for c in fc], [0] * len(fc)]
        arr = np.concatenate([np.asarray(c, dtype=np.int32) for c in cols])
        dev = self.stage.device
        if dev.type == "cuda":
            buf = torch.empty(arr.size, dtype=torch.int32, device=dev)
            self._stage_h2d(gs, arr, buf)
        else:
            buf = torch.from_numpy(arr)
        slots, nlp, counts, *more = buf.split([len(c) for c in cols])
        if gtab is not None:
            gsl = gtab[3]
            gsl.index_copy_(0, slots.long(), torch.stack(more[-2:], dim=1))
            more = more[:-2]
        edits, more = (more[:4], more[4:]) if tab is not None and ent else ((), more)
        if tab is not None:
            cnt.index_copy_(0, slots.long(), counts)
        if atab is not None:
            on.index_copy_(0, slots.long(), more[0])
            if ask:
                bits.index_copy_(0, more[1].long(), more[2].view(len(ask), W))
            more = more[3 if ask else 1:]
        if btab is not None:
            bcnt.index_copy_(0, slots.long(), more[0])
            if words:
                bend.view(-1).index_copy_(0, more[1].long(), more[2])
                btok.view(-1).index_copy_(0, more[3].long(), more[4])
        if edits:
            at, t, v, u = edits
            at = at.long()
            tok.view(-1).index_copy_(0, at, t)
            val.view(-1).index_copy_(0, at, v.view(torch.float32))
            until.view(-1).index_copy_(0, at, u)
        return slots, nlp
