"""Beam-search caption decoding with cached state.

The reference's caption evaluation (main_task_caption.py:434-618 with modules/beam.py) calls
`model.decoder_caption(...)` once per generated token on the COMPLETE prefixes of all n_inst x 5 beams: the 2-layer
cross encoder over cat(text, video) and the 3-layer decoder are recomputed from scratch up to max_words times, the
beams are re-assembled on the host with one `.item()` per token, and only the last position's logits are used
(`dec_output[:, -1, :]`, :452).  In eval mode everything that does not depend on the newest token is a pure function
of earlier inputs, so here:

  * the cross encoder runs ONCE per instance (not per beam, not per step) and each decoder layer's encoder-attention
    K/V projections of its output are computed once;
  * the decoder keeps a key/value cache per beam: a step embeds one token per beam, projects q/k/v for that position
    only, attends over the cache (attention kernel with Sq = 1 and a cache batch stride), and the five beams of an
    instance share the instance's encoder K/V by running encoder attention as B = n_inst, Sq = n_beams;
  * beam bookkeeping (Beam.advance, beam.py:63-87) is the LAST launch of each position's plan (univl_beam_step,
    csrc/beam.hip): top-n_bm over the flattened (beam x vocab) candidates, back-pointers = id // vocab, tokens = id % vocab
    written straight into the buffers the next position's embedding and cache gather read, plus one row of a device-side
    history.  One position is one graph replay and nothing else: no ATen kernel, no host read.  The host looks at the
    per-instance `done` bytes every `sync_every` positions only to stop early; finished instances keep their slots (static
    shapes) and are frozen, which is what removing them (collate_active_info, :404-416) amounts to, so the result does
    not depend on when the host looks.  Hypotheses are walked back on the device too (univl_beam_backtrack).
  * `beam_step="host"` keeps the earlier bookkeeping (torch.topk / where on the device, one host read per position) as the
    comparand of the tests and the A/B of the timing; it fills the same result object.

  * `beam_groups=G > 1` is Diverse Beam Search (Vijayakumar et al.): the n_bm beams of an instance are G groups of width
    k' = n_bm / G, searched in order at every position, each penalised by `diversity_penalty` times the number of beams of
    earlier groups that chose the same token at that position.  Only the last launch of a position changes
    (univl_beam_group_step instead of univl_beam_step): to every other launch and to the walk-back the session is an ordinary
    search on n_inst * G pseudo-instances of width k'.  The penalty is a device word (set_diversity).

Same results as the reference's procedure on the same logits: first step uses beam 0's distribution only (beam.py:69),
an instance is done when its top beam emits EOS (beam.py:84), the reported hypotheses are the n_best best-scored beams walked
back through the back-pointers (beam.py:108-116, collect_hypothesis_and_scores).  Candidates of exactly equal fp32 value
are ordered by lower flat index first in the device path (include/univl_hip.h); torch.topk leaves that order open.

Three layers, each naming what it owns:
  steps.InstanceSession   the cross encoder over n_inst instances on supplied features, idle slots, n_active, graph-or-eager replay
                          (score.CaptionScorer builds on this layer alone);
  CachedDecoder           the row decoder: encoder K/V, the per-row cache, the (position, form) plans, the loop over the positions;
  CaptionBeamSearch       the beam state, its history and the beam step (sample.CaptionSampler: the sampling state and the sample step).
                          _beam_step(t) is the one statement of the step's arguments: (op name, descriptor) of the plain, the group
                          or the pooled step, for the tail of a position's plan and for the pooled finish.
BeamResult and PoolBeamResult share _BeamHistory (the history rows and steps_run).
"""
import math

import torch

from . import _ab, ops
from .engine import DecoderLayer, DecoderStack, Plan, _gemm_desc
from .steps import InstanceSession, VocabHead, H


def check_beam_groups(n_bm, beam_groups=1, diversity_penalty=0.0):
    """The argument rule of group search, on the host and before any device work: beam_groups divides n_bm, the penalty is finite
    and >= 0 (a negative one would lift candidates that the per-row candidate lists of the beam step do not hold).  Returns
    (G, k' = n_bm // G, penalty as float); ValueError otherwise."""
    if isinstance(beam_groups, bool) or not isinstance(beam_groups, int) or not isinstance(n_bm, int):
        raise ValueError("beam_groups=%r, n_bm=%r: expected integers" % (beam_groups, n_bm))
    if not 1 <= beam_groups <= n_bm or n_bm % beam_groups:
        raise ValueError("beam_groups=%d does not divide n_bm=%d (1 <= beam_groups <= n_bm)" % (beam_groups, n_bm))
    try:
        pen = float(diversity_penalty)
    except (TypeError, ValueError):
        raise ValueError("diversity_penalty=%r is not a number" % (diversity_penalty,))
    if not math.isfinite(pen) or pen < 0.0:
        raise ValueError("diversity_penalty=%r, expected a finite value >= 0" % (diversity_penalty,))
    return beam_groups, n_bm // beam_groups, pen


class _BeamHistory:
    """What both results of CaptionBeamSearch.decode hold of the run: parents / step_tokens / step_scores [steps_run, n, n_bm]."""

    def __init__(self, parents, step_tokens, step_scores):
        self.parents, self.step_tokens, self.step_scores = parents, step_tokens, step_scores

    @property
    def steps_run(self):
        return self.parents.shape[0]


class BeamResult(_BeamHistory):
    """What CaptionBeamSearch.decode returns -- DEVICE tensors only:
      tokens  [n, n_best, Tmax] int32   the n_best best hypotheses of every instance, -1 padded
      scores  [n, n_best] fp32          their accumulated log-probabilities (non-increasing in k)
      lengths [n] int32                 generated tokens per instance (all n_best hypotheses of an instance share it)
      parents / step_tokens / step_scores  [steps_run, n, n_bm]   the history; steps_run is the max_len of the call, rows at or
                                        past an instance's length are frozen rows (identity parents, state repeated).
      groups  G                         1 for a plain search, whose shapes are the ones above.  For a group search (G > 1, n_best
                                        counted PER GROUP): tokens [n, G * n_best, Tmax] and scores [n, G * n_best] group-major
                                        (entry g * n_best + k is the k-th best of group g; non-increasing in k within a group),
                                        lengths [n, G], and the history's n_bm axis is G runs of k' beams with parents LOCAL to
                                        their group."""

    def __init__(self, tokens, scores, lengths, parents, step_tokens, step_scores, groups=1):
        super().__init__(parents, step_tokens, step_scores)
        self.tokens, self.scores, self.lengths = tokens, scores, lengths
        self.groups = groups

    def captions(self, eos, pad, eos_dev=None):
        """The reference's cut of every hypothesis at the first eos ("[SEP]"), then at the first pad ("[PAD]")
        (main_task_caption.py:555-560), on the device (ops.beam_captions): (cap_tokens [n, n_best, Tmax] int32, -1 past the cut;
        cap_len [n, n_best] int32), device tensors.  eos / pad: token ids, negative for none; eos_dev: a device word read instead
        of eos.  `tokens` is left as it is.  A group search's hypotheses are cut at their own group's length; the shapes follow
        `tokens` ([n, G * n_best, Tmax] and [n, G * n_best])."""
        n, gk, Tmax = self.tokens.shape
        P = n * self.groups                  # the (instance, group) view; groups = 1: the tensors as they are
        cap, cap_len = ops.beam_captions(self.tokens.reshape(P, gk // self.groups, Tmax), self.lengths.reshape(P), eos, pad, eos_dev=eos_dev)
        return cap.view(n, gk, Tmax), cap_len.view(n, gk)

    def hypotheses(self):
        """[n][n_best] token lists, as collect_hypothesis_and_scores(inst_dec_beams, n_best) gives them -- the one place that
        copies to the host."""
        n, gk, _ = self.tokens.shape
        tok, lens = self.tokens.cpu().tolist(), self.lengths.reshape(n, self.groups).cpu().tolist()
        nb = gk // self.groups
        return [[row[:lens[i][j // nb]] for j, row in enumerate(inst)] for i, inst in enumerate(tok)]


def check_length_penalty(length_penalty, early_stopping=False, beam_groups=1, beam_step="device"):
    """The argument rule of the pooled search, on the host and before any device work.  length_penalty: None (the reference search:
    returns None) or a finite number >= 0; early_stopping: a bool (or 0 / 1).  The pooled search has neither a group form nor a host
    comparand: together with beam_groups > 1 or beam_step="host" it is a ValueError.  Returns (alpha as float, early_stopping as int)."""
    if length_penalty is None:
        if early_stopping not in (False, 0):
            raise ValueError("early_stopping=%r needs a length_penalty (0.0 for none); length_penalty=None is the reference search, "
                             "which stops when the top beam emits the end token" % (early_stopping,))
        return None
    ops.length_weights(length_penalty, 0)            # ValueError unless a finite number >= 0
    if early_stopping not in (False, True, 0, 1):
        raise ValueError("early_stopping=%r, expected a bool" % (early_stopping,))
    if beam_groups != 1:
        raise ValueError("length_penalty= with beam_groups=%r: the pooled search has no group form (out of scope); use one or the "
                         "other" % (beam_groups,))
    if beam_step == "host":
        raise ValueError("length_penalty= with beam_step='host': the pooled search has no host comparand (out of scope); it needs "
                         "beam_step='device'")
    return float(length_penalty), int(bool(early_stopping))


class PoolBeamResult(_BeamHistory):
    """What CaptionBeamSearch.decode returns in a session built with a length_penalty -- DEVICE tensors only:
      tokens      [n, n_best, Tmax] int32  the n_best best entries of every instance's pool, in pool order, -1 padded; a FINISHED
                                           hypothesis ends with the end token, as a plain search's does
      scores      [n, n_best] fp32         their RAW summed log-probabilities (the end token's included): what score.score_beams,
                                           caption_metrics.consensus and rl compare, as with BeamResult; not sorted
      norm_scores [n, n_best] fp32         the keys raw * len ** -alpha the pool is ordered by (non-increasing in k)
      lengths     [n, n_best] int32        tokens PER HYPOTHESIS (the end token counts)
      finished    [n, n_best] uint8        1: ended with the end token; 0: a live beam when the positions ran out
      positions   [n] int32                positions the instance ran before it was done
      parents / step_tokens / step_scores  [steps_run, n, n_bm]   the history, as in BeamResult.
    A slot past an instance's pool (never the case when it ran a position and n_best <= n_bm) is -1 tokens, -inf, -inf, 0, 0."""
    groups = 1

    def __init__(self, tokens, scores, norm_scores, lengths, finished, positions, parents, step_tokens, step_scores):
        super().__init__(parents, step_tokens, step_scores)
        self.tokens, self.scores, self.norm_scores, self.lengths, self.finished = tokens, scores, norm_scores, lengths, finished
        self.positions = positions

    def captions(self, eos, pad, eos_dev=None):
        """BeamResult.captions on per-hypothesis lengths: (cap_tokens [n, n_best, Tmax] int32, cap_len [n, n_best] int32).  The rows
        are cut as n * n_best instances of one hypothesis each."""
        n, nb, Tmax = self.tokens.shape
        cap, cap_len = ops.beam_captions(self.tokens.reshape(n * nb, 1, Tmax), self.lengths.reshape(n * nb).contiguous(), eos, pad,
                                         eos_dev=eos_dev)
        return cap.view(n, nb, Tmax), cap_len.view(n, nb)

    def hypotheses(self):
        """[n][n_best] token lists, each of its own length -- the one place that copies to the host."""
        tok, lens = self.tokens.cpu().tolist(), self.lengths.cpu().tolist()
        return [[row[:lens[i][j]] for j, row in enumerate(inst)] for i, inst in enumerate(tok)]


class CachedDecoder(InstanceSession):
    """The cached row decoder over an InstanceSession: R = n_inst * n_rows rows (the n_rows rows of an instance share its encoder K/V),
    the per-layer encoder K/V computed once per batch (encode()), a self-attention cache per row, and one plan per (position, form),
    replayed as a hipGraph.  A subclass names its forms and says per form whether rows change places between positions
    (_reorders(form)) and what follows the vocabulary classifier (_plan_tail(pl, t, form)); it owns the state its tails read and write
    and resets it before _run_positions, the one loop over the positions."""

    NH = 12
    FORMS = ()           # the subclass's plan forms; a plan's key in self.steps is (t, form)

    def __init__(self, model, n_inst, W, F, n_rows, n_done, max_len=None, use_graphs=True, constraints=None):
        """n_done: the length of the done buffer that _run_positions polls.
        constraints: a constrain.DecodeConstraints or None.  The session binds a copy (self.constraints); the subclass's _plan_tail adds
        ONE launch, univl_decode_constrain, in front of its selection kernel.  None adds no launch, no buffer and no plan entry."""
        self.Tmax = Tmax = int(max_len or model.task_config.max_words)
        assert Tmax <= model.decoder_config.max_target_embeddings
        if constraints is not None:          # validated against this session before any device work
            constraints = constraints.bind(model.bert_config.vocab_size, Tmax, next(model.parameters()).device)
        self.constraints = constraints
        super().__init__(model, n_inst, W, F, use_graphs)
        self.n_rows = n_rows
        self.R = R = n_inst * n_rows
        self.V = model.bert_config.vocab_size
        self.L = L = model.decoder_config.num_decoder_layers
        cx, S = self.cx, self.S
        e, ct, fl, dt = cx.e, cx.ct, cx.fl, cx.dt
        # ---- once per batch, after the cross encoder: encoder K/V of every decoder layer
        self.kv2 = [e(n_inst * S, 2 * H, dtype=ct) for _ in range(L)]
        for l in range(L):
            nm = DecoderStack._names(l)
            self.plan.add("univl_gemm", _gemm_desc(dt, self.run.out16, H, fl.wop_fused(nm["c_kv_w"]), H, n_inst * S, 2 * H, H,
                                                   out16=self.kv2[l], ldc=2 * H, bias=fl.w32_fused(nm["c_kv_b"])))
        # ---- per step buffers (R rows)
        self.ids = e(R, dtype=torch.int64)
        self.ey, self.est, self.e32 = e(R, H), e(R, 2), e(R, H)
        self.e16 = e(R, H, dtype=ct) if cx.bf else self.e32
        self.cache = [[torch.zeros(R, Tmax, 2 * H, device=cx.dev, dtype=ct) for _ in range(2)] for _ in range(L)]
        self.ws = [dict(DecoderStack.layer_workspace(e, ct, R), q1=e(R, H, dtype=ct)) for _ in range(L)]
        self.head = VocabHead(cx, "decoder.classifier.cls.predictions", R)
        self.src = e(R, dtype=torch.int32)               # cache row each row continues from (forms that reorder)
        self.steps = {}
        self.eos_dev = torch.full((1,), -1, dtype=torch.int32, device=cx.dev)     # a device word: the captured plans serve any eos
        self.done_host = torch.zeros(n_done, dtype=torch.uint8).pin_memory()
        self.done_event = torch.cuda.Event()

    # ------------------------------------------------------------------------------------------ step plans
    def _step_plan(self, t, form):
        """The plan of position t in one of the subclass's forms: embedding .. vocabulary classifier, then _plan_tail."""
        pl = self.steps.get((t, form))
        if pl is not None:
            return pl
        if form not in self.FORMS:
            raise ValueError("%s: no plan form %r, expected one of %r" % (type(self).__name__, form, self.FORMS))
        cx, fl, dt, R, Tmax, S = self.cx, self.cx.fl, self.cx.dt, self.R, self.Tmax, self.S
        W32 = fl.w32
        es = 2 if cx.bf else 4
        pl = Plan()
        reorder = self._reorders(form)
        cur, prev = (t % 2, (t + 1) % 2) if reorder else (0, 0)     # rows that stay where they are need one cache buffer and no gather
        pos = W32("bert.embeddings.position_embeddings.weight")[t:]
        pl.add("univl_embed_text_fwd", ops.embed_text_desc(
            dt, R, 1, self.ids, W32("bert.embeddings.word_embeddings.weight"), pos, W32("decoder.embeddings.LayerNorm.weight"),
            W32("decoder.embeddings.LayerNorm.bias"), y=self.ey, stats=self.est, out32=self.e32,
            out16=self.e16 if cx.bf else None))
        x32, x16 = self.e32, self.e16
        for l in range(self.L):
            ws = self.ws[l]
            lay = DecoderLayer(pl, fl, l, ws, R)
            nm = lay.nm
            cache = self.cache[l][cur]
            if t > 0 and reorder:        # rows continue from re-ordered parents: gather positions [0, t) of the parent rows
                src_c, stride, nbytes = self.cache[l][prev], Tmax * 2 * H * es, t * 2 * H * es
                pl.add_callable(lambda s=src_c, d=cache, st=stride, nb=nbytes: ops.gather_rows(s, d, self.src, R, st, nb))
            wqkv, bqkv = fl.wop_fused(nm["s_qkv_w"]), fl.w32_fused(nm["s_qkv_b"])
            pl.add("univl_gemm", _gemm_desc(dt, x16, H, wqkv[:H], H, R, H, H, out16=ws["q1"], ldc=H, bias=bqkv[:H]))
            kv_slot = cache[:, t]                                      # [R, 2H] view, row stride Tmax*2H
            pl.add("univl_gemm", _gemm_desc(dt, x16, H, wqkv[H:], H, R, 2 * H, H, out16=kv_slot, ldc=Tmax * 2 * H, bias=bqkv[H:]))
            pl.add("univl_attention_fwd", ops.attention_desc(
                dt, R, self.NH, 1, t + 1, ws["q1"], H, (cache, 0), 2 * H, (cache, H), 2 * H, ws["ctx1"], H, ws["lse1"],
                bsk=Tmax * 2 * H, bsv=Tmax * 2 * H))
            lay.attn_output("s_", x32)
            lay.enc_query()
            lay.enc_attention(self.n_inst, self.n_rows, S, self.kv2[l], self.run.cmask)
            lay.attn_output("c_", ws["a32"])
            lay.ffn()
            x32, x16 = ws["o32"], ws["o16"]
        self.head.build_forward(pl, x16, with_loss=False)
        self._plan_tail(pl, t, form)
        pl.keepalive = (pos,)
        self.steps[(t, form)] = pl
        return pl

    def _reorders(self, form):
        raise NotImplementedError

    def _plan_tail(self, pl, t, form):
        raise NotImplementedError

    def _prefix_buffers(self):
        """Each row's emitted tokens, two [R, Tmax] int32 buffers used with parity t % 2 like self.cache (rows change places between
        positions).  Allocated when the first plan that needs them is built -- plans are built outside any capture -- so a session
        whose rows stay in place (CaptionSampler reads its own tokens_out) has none.  Zero-filled: the rows of idle slots are copied
        along, from defined memory."""
        if not hasattr(self, "prefix"):
            self.prefix = [torch.zeros(self.R, self.Tmax, dtype=torch.int32, device=self.cx.dev) for _ in range(2)]
        return self.prefix

    # ------------------------------------------------------------------------------------------------- run
    def set_constraints(self, ngram=None, min_len=None):
        """Rewrite the blocked n-gram order and / or the minimum length of a session built with constraints (None: keep).  They are
        device words that the captured launches read: nothing is captured again.  The suppress list is fixed for the session's life
        (its length is baked into the captures); another list is another session."""
        if self.constraints is None:
            raise ValueError("set_constraints: this session was built with constraints=None; its plans carry no constraint launch")
        self.constraints.set(ngram=ngram, min_len=min_len)

    @torch.no_grad()
    def encode(self, sequence_output, visual_output, input_mask, video_mask, n_active=None):
        self.load_features(sequence_output, visual_output, input_mask, video_mask, self._active(n_active), "encode")
        self.plan.run()

    def _run_positions(self, form, max_len, sync_every, done):
        """One replay of the form's plan per position 0 .. max_len-1; returns the number of positions run.  Every sync_every positions
        (0: never) the host reads the `done` bytes through the pinned buffer and an event wait -- the only host read of the loop -- and
        stops when all are set.  Finished rows are frozen by the tails, so the result does not depend on when the host looks."""
        for t in range(max_len):
            self._replay(self._step_plan(t, form))
            if sync_every and (t + 1) % sync_every == 0 and t + 1 < max_len:
                self.done_host.copy_(done, non_blocking=True)
                self.done_event.record()
                self.done_event.synchronize()
                if bool(self.done_host.all()):
                    return t + 1
        return max_len


class CaptionBeamSearch(CachedDecoder):
    """Compiled decoding session for a fixed (n_inst, max_words W, max_frames F, beam size, max_len): the beam state, its history and
    the beam step as the tail of CachedDecoder's plans.  The forms are True (embedding .. log-probabilities .. univl_beam_step, with t,
    the history row and first_step baked into that position's descriptor; what decode() replays) and False (the same launches without
    the beam step: what step_logprobs replays; it neither reads nor advances the beam state).  Rows change places in both.

    Partial batches (steps.InstanceSession): encode() / decode() / __call__ take n_active.  The `done` byte of an idle slot is preset
    to 1 and its `length` to 0 before position 0, so the beam scan skips it and the select kernel writes frozen rows for it, as both do
    for an instance that has finished.  The BeamResult holds the first n_active instances only."""

    def __init__(self, model, n_inst, W, F, n_bm=5, max_len=None, use_graphs=True, beam_step=None, constraints=None, beam_groups=1,
                 diversity_penalty=0.0, length_penalty=None, early_stopping=False):
        """beam_step: "device" (default; univl_beam_step as the tail of each position's plan) | "host" (the ATen comparand);
        None: the UNIVL_AB key `beam_step` (default device).
        constraints: a constrain.DecodeConstraints (no repeated n-gram, a minimum length, suppressed ids) or None.  The launch sits
        between the log-softmax and the beam step, so both beam_step modes decode under the same constraints, and step_logprobs returns
        constrained rows PROVIDED positions are visited in order from 0 with `parents` given (the launch keeps each row's prefix up to
        date from them).  The minimum length counts against the `eos` of decode().  Every live row must keep n_bm finite columns: the
        caller's condition.
        beam_groups, diversity_penalty: Diverse Beam Search with G groups of n_bm // G beams (check_beam_groups states the rule).
        1 (default) is the plain search: the same plans launch for launch, no new buffer, the penalty unused.  With G > 1 the last
        launch of a position is univl_beam_group_step, `done` / `length` hold one entry per (instance, group), constraints see
        done_stride = k', the penalty is a device word (set_diversity), and beam_step="host" is a ValueError: the host comparand
        has no group form.
        length_penalty, early_stopping: None (default) is the search above, the same plans launch for launch, no new buffer.  A
        finite alpha >= 0 is beam search with a pool of finished hypotheses (include/univl_hip.h: univl_beam_pool_step): a beam that
        emits the end token leaves the beams for the pool, hypotheses are ranked by raw * len ** -alpha, an instance is done when
        its pool is full and (early_stopping, or no live beam can still enter it), and decode() returns a PoolBeamResult.  The last
        launch of a position is univl_beam_pool_step; alpha and the mode are device words (set_length_penalty).  Out of scope, a
        ValueError: together with beam_groups > 1 or beam_step="host"."""
        self.G, self.kp, penalty = check_beam_groups(n_bm, beam_groups, diversity_penalty)
        G, kp = self.G, self.kp
        if beam_step is None:
            beam_step = "device" if _ab.get("beam_step") else "host"
        if beam_step not in ("device", "host"):
            raise ValueError("CaptionBeamSearch: beam_step must be 'device' or 'host', got %r" % (beam_step,))
        if G > 1 and beam_step != "device":
            raise ValueError("CaptionBeamSearch: beam_groups=%d needs beam_step='device'; the host path has no group form" % G)
        pooled = check_length_penalty(length_penalty, early_stopping, G, beam_step)
        self.pooled = pooled is not None
        self.beam_step, self.n_bm = beam_step, n_bm
        P = n_inst * G                                   # (instance, group) pairs, the pseudo-instances of width k'
        super().__init__(model, n_inst, W, F, n_bm, P, max_len=max_len, use_graphs=use_graphs, constraints=constraints)
        dev, R, Tmax = self.cx.dev, self.R, self.Tmax
        # ---- beam state and history (read and written by univl_beam_step; the host path fills the same buffers)
        self.scores = torch.zeros(n_inst, n_bm, device=dev)
        self.done = torch.zeros(P, dtype=torch.uint8, device=dev)
        self.length = torch.zeros(P, dtype=torch.int32, device=dev)
        self.hist_par = torch.zeros(Tmax, n_inst, n_bm, dtype=torch.int32, device=dev)
        self.hist_tok = torch.zeros(Tmax, n_inst, n_bm, dtype=torch.int32, device=dev)
        self.hist_sc = torch.zeros(Tmax, n_inst, n_bm, device=dev)
        self.base = torch.arange(n_inst, device=dev, dtype=torch.int64)[:, None] * n_bm
        self.ident = torch.arange(R, device=dev, dtype=torch.int32)
        self.ident_nb = torch.arange(kp, device=dev, dtype=torch.int32).repeat(G).expand(n_inst, n_bm)      # parents are local to a group
        self.beam_ws = ops.beam_ws(n_inst, n_bm, dev) if beam_step == "device" else None
        if G > 1:
            self.diversity_dev = torch.full((1,), penalty, dtype=torch.float32, device=dev)     # a device word: the captured plans serve any penalty
        if self.pooled:
            # device words: the captured plans serve any penalty, stopping mode and max_len
            self.length_penalty, self.early_stopping = pooled
            self.pool_w = ops.length_weights(pooled[0], Tmax).to(dev)
            self.pool_params = torch.tensor([pooled[1], Tmax], dtype=torch.int32, device=dev)
            self.pool = ops.beam_pool(n_inst, n_bm, dev)

    # ------------------------------------------------------------------------------------------ step plans
    FORMS = (False, True)

    def _reorders(self, beam):
        return True

    def _plan_tail(self, pl, t, beam):
        pl.add_callable(lambda: ops.log_softmax_rows(self.head.logits, self.V))
        if self.constraints is not None:
            c, prefix = self.constraints, self._prefix_buffers()
            pl.add("univl_decode_constrain", ops.decode_constrain_desc(
                self.head.logits, self.V, t, prefix_in=prefix[(t + 1) % 2], prefix_out=prefix[t % 2], src=self.src, last=self.ids,
                done=self.done, done_stride=self.kp, eos_dev=self.eos_dev, params_dev=c.params_dev, suppress=c.suppress_dev))
        if beam:
            pl.add(*self._beam_step(t))

    def _beam_step(self, t):
        """The session's beam step at position t as (op name, descriptor): the pooled, the group or the plain one."""
        lp = (self.head.logits, self.V, self.n_inst, self.n_bm)
        state = dict(scores=self.scores, done=self.done, length=self.length, tokens=self.ids, src=self.src, hist_parents=self.hist_par,
                     hist_tokens=self.hist_tok, hist_scores=self.hist_sc, ws=self.beam_ws, eos_dev=self.eos_dev)
        if self.pooled:
            return "univl_beam_pool_step", ops.beam_pool_step_desc(*lp, t, w=self.pool_w, params=self.pool_params, **self.pool, **state)
        if self.G > 1:
            return "univl_beam_group_step", ops.beam_group_step_desc(*lp, self.G, t, diversity_dev=self.diversity_dev, **state)
        return "univl_beam_step", ops.beam_step_desc(*lp, t, **state)

    # ------------------------------------------------------------------------------------------------- run
    def set_length_penalty(self, alpha, early_stopping=None):
        """Rewrite the length penalty and (None: keep) the stopping mode of a session built with a length_penalty.  They are a device
        table and a device word that the captured beam step reads: nothing is captured again."""
        if not self.pooled:
            raise ValueError("set_length_penalty: this session was built with length_penalty=None; its plans carry no pool step")
        if alpha is None:
            raise ValueError("set_length_penalty: alpha=None; the reference search is another session (length_penalty=None)")
        alpha, es = check_length_penalty(alpha, self.early_stopping if early_stopping is None else early_stopping)
        self.pool_w.copy_(ops.length_weights(alpha, self.Tmax))
        self.pool_params[0:1].fill_(es)
        self.length_penalty, self.early_stopping = alpha, es

    def set_diversity(self, penalty):
        """Rewrite the diversity penalty of a session built with beam_groups > 1.  It is a device word that the captured beam step
        reads: nothing is captured again."""
        if self.G == 1:
            raise ValueError("set_diversity: this session was built with beam_groups=1; its plans carry no group step")
        self.diversity_dev.fill_(check_beam_groups(self.n_bm, self.G, penalty)[2])

    @torch.no_grad()
    def step_logprobs(self, t, last_tokens, parents=None):
        """One cached decoder step: log-probabilities [R, V] of the token after position t, given each beam's token at
        position t and (t > 0) the cache row it continues from.  Exposed for the parity tests.  In a session with constraints the
        rows are the constrained ones when positions are visited in order from 0 with `parents` given (class __init__), under the
        session's state AS IT STANDS: the launch reads self.done (a finished instance's rows come back unconstrained) and self.eos_dev
        (the end token of the minimum length), which decode() sets and leaves as its last batch ended.  A caller that drives this
        method itself sets them first: `session.done.zero_(); session.eos_dev.fill_(eos)`."""
        self.ids.copy_(last_tokens.reshape(-1))
        if t > 0:
            self.src.copy_(parents.reshape(-1).to(torch.int32))
        self._replay(self._step_plan(t, False))
        return self.head.logits[:, :self.V]

    @torch.no_grad()
    def decode(self, sequence_output, visual_output, input_mask, video_mask, bos, eos, max_len=None, n_best=1, sync_every=8,
               n_active=None):
        """Beam search over at most max_len positions; returns a BeamResult (device tensors).  n_best <= n_bm hypotheses per
        instance; in a group search n_best <= k' is counted PER GROUP and the result is group-major (BeamResult).  sync_every: the host reads the done flags every that many positions to stop early (0: never, run to max_len);
        finished instances are frozen, so the result does not depend on it.  n_active: instances in this batch (class docstring);
        the result then has n_active instances."""
        n, G, kp, Tmax, n_best = self.n_inst, self.G, self.kp, self.Tmax, int(n_best)
        m = self._active(n_active)
        max_len = min(int(max_len or Tmax), Tmax)
        if not 1 <= n_best <= kp:
            raise ValueError("CaptionBeamSearch.decode: n_best=%r, expected 1 .. %s=%d" % (n_best, "n_bm" if G == 1 else "n_bm / beam_groups", kp))
        self.encode(sequence_output, visual_output, input_mask, video_mask, n_active=n_active)
        # state reset (outside the position loop)
        self.scores.zero_()
        self.done.zero_()
        self.length.zero_()
        if m < n:
            self.done[m * G:].fill_(1)       # idle slots: done from the start (every group), length 0
        self.ids.fill_(int(bos))
        self.src.copy_(self.ident)
        self.eos_dev.fill_(int(eos))
        if self.pooled:
            self.pool["pool_count"].zero_()
            self.pool_params[1:2].fill_(max_len)
        if self.beam_step == "device":
            ran = self._run_positions(True, max_len, sync_every, self.done)
        else:
            ran = self._host_steps(max_len, int(eos))
        if ran < max_len:            # every instance is done: the rows not run are the frozen rows the kernel would have written
            self.hist_par[ran:max_len] = self.ident_nb
            self.hist_tok[ran:max_len] = self.hist_tok[ran - 1]
            self.hist_sc[ran:max_len] = self.hist_sc[ran - 1]
        if self.pooled:
            tokens, raw, key, lens, fin = ops.beam_pool_finish(self._beam_step(0)[1], n_best)
            return PoolBeamResult(tokens[:m], raw[:m], key[:m], lens[:m], fin[:m], self.length[:m].clone(), self.hist_par[:max_len, :m].clone(),
                                  self.hist_tok[:max_len, :m].clone(), self.hist_sc[:max_len, :m].clone())
        # the walk-back on the (n * G, k') view: the history's parents are local to their group (G = 1: the tensors as they are)
        tokens, scores = ops.beam_backtrack(self.hist_par.view(Tmax, n * G, kp), self.hist_tok.view(Tmax, n * G, kp),
                                            self.scores.view(n * G, kp), self.length, n_best)
        tokens, scores = tokens.view(n, G * n_best, Tmax), scores.view(n, G * n_best)
        lengths = self.length[:m * G].clone()
        return BeamResult(tokens[:m], scores[:m], lengths if G == 1 else lengths.view(m, G), self.hist_par[:max_len, :m].clone(),
                          self.hist_tok[:max_len, :m].clone(), self.hist_sc[:max_len, :m].clone(), groups=G)

    def _host_steps(self, max_len, eos):
        """beam_step="host": the bookkeeping as ATen calls on the device with one host read per position -- the arithmetic of the
        path this class had before univl_beam_step, kept as the comparand; it leaves state and history in the same buffers."""
        n, nb, V, dev = self.n_inst, self.n_bm, self.V, self.cx.dev
        scores = torch.zeros(n, nb, device=dev)
        done = self.done.bool()                # zeros, but for the idle slots of a partial batch
        length = torch.zeros(n, dtype=torch.int64, device=dev)
        tokens = self.ids.view(n, nb).clone()
        ident = torch.arange(nb, device=dev).expand(n, nb)
        parents = ident.contiguous()
        ran = max_len
        for t in range(max_len):
            lp = self.step_logprobs(t, tokens, (self.base + parents) if t > 0 else None).view(n, nb, V)
            if t == 0:
                best, ids = lp[:, 0, :].topk(nb, dim=1, largest=True, sorted=True)             # beam.py:69-72
            else:
                best, ids = (lp + scores[:, :, None]).view(n, nb * V).topk(nb, dim=1, largest=True, sorted=True)
            pk, ny = ids // V, ids % V
            act = ~done
            scores = torch.where(act[:, None], best, scores)
            parents = torch.where(act[:, None], pk, ident)
            tokens = torch.where(act[:, None], ny, tokens)
            self.hist_par[t].copy_(parents)
            self.hist_tok[t].copy_(tokens)
            self.hist_sc[t].copy_(scores)
            length += act.to(torch.int64)
            done = done | (act & (ny[:, 0] == eos))                                           # beam.py:84
            if bool(done.all()):
                ran = t + 1
                break
        self.scores.copy_(scores)
        self.done.copy_(done)
        self.length.copy_(length)
        self.ids.copy_(tokens.reshape(-1))
        self.src.copy_((self.base + parents).reshape(-1))
        return ran

    @torch.no_grad()
    def __call__(self, sequence_output, visual_output, input_mask, video_mask, bos, eos, max_len=None, n_active=None):
        """Returns (hypotheses: list of n_inst (n_active) token lists, as collect_hypothesis_and_scores(n_best=1) gives them,
        scores: [n_inst] ([n_active]) fp32 tensor of the best beams' accumulated log-probabilities)."""
        res = self.decode(sequence_output, visual_output, input_mask, video_mask, bos, eos, max_len=max_len, n_best=1,
                          n_active=n_active)
        return [h[0] for h in res.hypotheses()], res.scores[:, 0].clone()
