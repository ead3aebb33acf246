"""Teacher-forced caption scoring: how likely is this caption for this video?

`UniVL.decoder_caption` answers that only through the [captions, Wd, 30522] fp32 logits (122 KB per token), with log-softmax,
gather and arg-max left to the caller, and it runs the cross encoder once per caption.  CaptionScorer is the compiled session for the
question itself:

  * the cross encoder runs ONCE per instance (video + its text); its output rows and the concatenated key mask are replicated to the
    n_cand captions of the instance with univl_gather_rows (n_cand = 1: the decoder reads the cross encoder's buffers in place);
  * the decoder stack runs over n_inst * n_cand captions of Wd positions (evaluation mode, causal self-attention);
  * the vocabulary head's transform feeds univl_vocab_score (csrc/vocab_score.h): per token the label's log-probability, the arg-max
    and its log-probability, per caption their sum, the number of tokens that count and the number the arg-max gets right.  The
    logits are never written; the session allocates no [rows, V] buffer at all.

One Plan on one stream, replayed as a hipGraph; no host read anywhere in score().  Labels follow the reference's convention
(CrossEntropyLoss(ignore_index=-1), modeling.py:253): -1 marks a position that does not count.
"""
import torch

from . import ops
from .engine import DecoderStack
from .steps import InstanceSession, VocabHead, H


class CaptionScores:
    """What CaptionScorer.score returns -- DEVICE tensors only (n instances, n_cand captions each):
      token_logprob [n, n_cand, Wd] fp32   log p(label | video, earlier input tokens); 0 where the label is -1
      top_token     [n, n_cand, Wd] int32  the arg-max of every position (equal logits: the lower id)
      top_logprob   [n, n_cand, Wd] fp32   its log-probability
      seq_logprob   [n, n_cand] fp32       the sum of token_logprob over the caption, in position order
      seq_tokens    [n, n_cand] int32      positions that count
      seq_correct   [n, n_cand] int32      positions that count and whose arg-max is the label"""

    def __init__(self, token_logprob, top_token, top_logprob, seq_logprob, seq_tokens, seq_correct):
        self.token_logprob, self.top_token, self.top_logprob = token_logprob, top_token, top_logprob
        self.seq_logprob, self.seq_tokens, self.seq_correct = seq_logprob, seq_tokens, seq_correct

    def normalized(self, alpha=1.0):
        """seq_logprob / max(seq_tokens, 1) ** alpha (length-normalised log-likelihood), on the tensors' device."""
        return self.seq_logprob / self.seq_tokens.clamp(min=1).to(torch.float32) ** float(alpha)


def beam_inputs_labels(tokens, lengths, bos, eos, pad, Wd):
    """Teacher-forcing inputs for the hypotheses of a decode.BeamResult, as tensor operations on the tensors' own device (no host
    read).  tokens [n, n_best, Tmax] (-1 padded), lengths [n] -- or [n, n_best], one per hypothesis, as a sample.SampleResult has them --
    (clamped to [0, Tmax]); Tmax <= Wd.  Per hypothesis, with
    cut = the position after the first eos inside the length, or the length when there is none:
      labels [n, n_best, Wd] int64   the hypothesis tokens at positions < cut, -1 after
      inputs [n, n_best, Wd] int64   [bos] + hyp[:-1] at positions < cut, pad after
      mask   [n, n_best, Wd] int64   1 at positions < cut
    eos: a negative id means none."""
    n, nb, T = tokens.shape
    if T > Wd:
        raise ValueError("beam_inputs_labels: hypotheses of %d positions do not fit Wd=%d" % (T, Wd))
    tok = tokens.to(torch.int64)
    if T < Wd:
        tok = torch.nn.functional.pad(tok, (0, Wd - T), value=-1)
    pos = torch.arange(Wd, device=tok.device)
    length = lengths.to(torch.int64).clamp(0, T).view(n, -1, 1)          # [n, 1, 1] or [n, n_best, 1]
    at_eos = (tok == int(eos)) & (pos < length) & (int(eos) >= 0)
    first = torch.where(at_eos, pos, torch.full_like(pos, Wd)).min(dim=-1, keepdim=True).values
    keep = pos < torch.minimum(first + 1, length)
    prev = torch.cat([torch.full_like(tok[..., :1], int(bos)), tok[..., :-1]], dim=-1)
    labels = torch.where(keep, tok, torch.full_like(tok, -1))
    inputs = torch.where(keep, prev, torch.full_like(tok, int(pad)))
    return inputs, labels, keep.to(torch.int64)


class CaptionScorer(InstanceSession):
    """Compiled scoring session for a fixed (n_inst, max_words W, max_frames F, caption length Wd, n_cand captions per instance).

    The encoder half is steps.InstanceSession (the cross encoder alone, once per instance; idle slots; n_active); this class appends the
    decoder over the captions and the scoring head to its plan.  Partial batches: score() takes n_active (None: n_inst); the tensors
    then carry n_active instances.  The labels of idle slots are set to -1 and their decoder masks and input ids to 0.  No launch
    reduces across instances or captions, so the active results do not depend on idle contents.  The result holds the first n_active
    instances only.

    The scores are the model's UNSMOOTHED log-probabilities: model.caption_label_smoothing shapes the training loss only and is not
    looked at here."""

    def __init__(self, model, n_inst, W, F, Wd, n_cand=1, use_graphs=True):
        if n_inst < 1 or n_cand < 1 or Wd < 1:
            raise ValueError("CaptionScorer: n_inst=%r, n_cand=%r, Wd=%r must be positive" % (n_inst, n_cand, Wd))
        assert Wd <= model.decoder_config.max_target_embeddings
        if n_cand > 1 and (W + F) % 2:
            raise ValueError("CaptionScorer: n_cand > 1 needs an even W + F (univl_gather_rows moves the int64 key mask in 16-byte units)")
        super().__init__(model, n_inst, W, F, use_graphs)
        self.Wd, self.n_cand = Wd, n_cand
        self.n_cross_ops = len(self.plan)
        cx, run, pl, S = self.cx, self.run, self.plan, self.S
        e, ct, bf, fl, dt, dev = cx.e, cx.ct, cx.bf, cx.fl, cx.dt, cx.dev
        B = self.B = n_inst * n_cand
        T = self.T = B * Wd
        # ---- the cross encoder's output and key mask, once per caption
        if n_cand == 1:
            enc16, enc_mask = run.out16, run.cmask
        else:
            enc16, enc_mask = e(B * S, H, dtype=ct), e(B, S, dtype=torch.int64)
            self.owner = torch.arange(n_inst, device=dev, dtype=torch.int32).repeat_interleave(n_cand).contiguous()
            nbytes = S * H * (2 if bf else 4)
            pl.add_callable(lambda: ops.gather_rows(run.out16, enc16, self.owner, B, nbytes, nbytes))
            pl.add_callable(lambda: ops.gather_rows(run.cmask, enc_mask, self.owner, B, S * 8, S * 8))
        self.enc16, self.enc_mask = enc16, enc_mask
        # ---- decoder over the B captions (the wiring of steps.DecoderRun, without its loss)
        W32 = fl.w32
        self.cap_ids, self.dmask = e(B, Wd, dtype=torch.int64), e(B, Wd, dtype=torch.int64)
        self.ey, self.est, self.e0_32 = e(T, H), e(T, 2), e(T, H)
        self.e0_16 = e(T, H, dtype=ct) if bf else self.e0_32
        pl.add("univl_embed_text_fwd", ops.embed_text_desc(
            dt, B, Wd, self.cap_ids, W32("bert.embeddings.word_embeddings.weight"), W32("bert.embeddings.position_embeddings.weight"),
            W32("decoder.embeddings.LayerNorm.weight"), W32("decoder.embeddings.LayerNorm.bias"), y=self.ey, stats=self.est,
            out32=self.e0_32, out16=self.e0_16 if bf else None))
        L = model.decoder_config.num_decoder_layers
        self.stack = DecoderStack(fl, L, B, Wd, S, self.dmask, enc_mask, 0.0, cx.seed_dev, cx.sites)
        self.stack.build_forward(pl, self.e0_32, self.e0_16, enc16, False)
        # ---- head: transform, then the scoring form of K16 (no logits buffer)
        self.head = head = VocabHead(cx, "decoder.classifier.cls.predictions", T, transform_only=True)
        head.build_transform(pl, self.stack.output()[1])
        head.labels.fill_(-1)
        nm = head.names()
        self.V = V = head.V
        self.vs_desc, self.out = ops.vocab_score_desc(head.h16, fl.wop(nm["emb"]), W32(nm["bias"]), head.labels, V, Wd)
        pl.add("univl_vocab_score", self.vs_desc)

    def _captions(self, t, m, what):
        nc, Wd = self.n_cand, self.Wd
        if t.numel() != m * nc * Wd or t.shape[-1] != Wd:
            raise ValueError("CaptionScorer.score: %s of shape %s, expected [%d, %d, %d]" % (what, tuple(t.shape), m, nc, Wd))
        return t.reshape(m * nc, Wd)

    @torch.no_grad()
    def score(self, sequence_output, visual_output, input_mask, video_mask, input_caption_ids, decoder_mask, output_caption_ids,
              n_active=None):
        """Caption tensors: [n, n_cand, Wd] ([n, Wd] when n_cand == 1), n = n_active or n_inst; output_caption_ids holds -1 at the
        positions that do not count.  Returns a CaptionScores of new device tensors."""
        n, nc, Wd = self.n_inst, self.n_cand, self.Wd
        m = self._active(n_active)
        self.load_features(sequence_output, visual_output, input_mask, video_mask, m, "score")
        ids = self._captions(input_caption_ids, m, "input_caption_ids")
        dm = self._captions(decoder_mask, m, "decoder_mask")
        lab = self._captions(output_caption_ids, m, "output_caption_ids")
        k = m * nc
        self.cap_ids[:k].copy_(ids, non_blocking=True)
        self.dmask[:k].copy_(dm, non_blocking=True)
        labels = self.head.labels.view(n * nc, Wd)
        labels[:k].copy_(lab, non_blocking=True)
        if m < n:
            self.cap_ids[k:].zero_()
            self.dmask[k:].zero_()
            labels[k:].fill_(-1)
        self._replay(self.plan)
        o = self.out
        tok = lambda name: o[name].view(n, nc, Wd)[:m].clone()
        seq = lambda name: o[name].view(n, nc)[:m].clone()
        return CaptionScores(tok("token_logprob"), tok("top_token"), tok("top_logprob"), seq("seq_logprob"), seq("seq_tokens"),
                             seq("seq_correct"))

    __call__ = score

    @torch.no_grad()
    def score_beams(self, result, sequence_output, visual_output, input_mask, video_mask, bos, eos, pad):
        """Score the n_best hypotheses of a decode.BeamResult (n_best <= n_cand) under teacher forcing: input [bos] + hyp[:-1], labels
        the hypothesis tokens up to and including the first eos inside the instance's length (beam_inputs_labels).  With
        .normalized() this re-ranks decode()'s n-best list by length-normalised likelihood.  Candidates n_best .. n_cand - 1 are idle;
        the result holds n_best captions per instance."""
        m, nb, _ = result.tokens.shape
        if nb > self.n_cand:
            raise ValueError("CaptionScorer.score_beams: n_best=%d hypotheses, session built for n_cand=%d" % (nb, self.n_cand))
        inputs, labels, mask = beam_inputs_labels(result.tokens, result.lengths, bos, eos, pad, self.Wd)
        if nb < self.n_cand:
            fill = (0, 0, 0, self.n_cand - nb)
            inputs = torch.nn.functional.pad(inputs, fill, value=int(pad))
            labels = torch.nn.functional.pad(labels, fill, value=-1)
            mask = torch.nn.functional.pad(mask, fill, value=0)
        r = self.score(sequence_output, visual_output, input_mask, video_mask, inputs, mask, labels,
                       n_active=None if m == self.n_inst else m)
        return CaptionScores(r.token_logprob[:, :nb], r.top_token[:, :nb], r.top_logprob[:, :nb], r.seq_logprob[:, :nb],
                             r.seq_tokens[:, :nb], r.seq_correct[:, :nb])
