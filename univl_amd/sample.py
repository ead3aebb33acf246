"""Caption sampling: several DIFFERENT captions per video by ancestral sampling with top-k, temperature and top-p.

Beam search answers "what is the best caption"; its n_best list is near-copies of one sentence.  CaptionSampler draws n_samp
independent captions per instance from the decoder's own distribution (cut to the k most likely tokens, sharpened or flattened by
a temperature, cut again to a nucleus of mass top_p) and reports, per token and per caption, both the model's log-probability and
the proposal's, so that a consumer can re-rank or importance-weight the samples.

The session is a decode.CachedDecoder with n_samp rows per instance: from steps.InstanceSession the cross encoder once per instance,
idle slots for partial batches and the graph-or-eager replay; from CachedDecoder the per-layer encoder K/V, the per-row self-attention
cache, the rows of an instance sharing its encoder K/V, one hipGraph per position and the loop over the positions.  CaptionSampler
itself owns the sampling state and two forms of a position's plan, "logits" and "sample":

  * rows never change places, so both forms use ONE cache buffer per layer and have no cache gather;
  * the tail of "sample" is univl_sample_step (csrc/sample.hip) on the RAW logits: no univl_log_softmax_rows, no beam step.  Top-k,
    weights, nucleus, the draw, the token into the buffer the next position's embedding reads, the log-probabilities and the per-row
    done / length all happen in its two launches.  temperature, top_p, the seed and the end token are device words, so one capture
    serves every value of them.  "logits" has no tail.

A draw is a pure function of (the row's logits, top_k, temperature, top_p, seed, position, row): the same seed gives the same
captions whatever sync_every or n_active is, and two rows of one instance differ because the row index keys the generator.
"""
import torch

from . import ops
from ._lib import SAMPLE_KMAX
from .decode import CachedDecoder


class SampleResult:
    """What CaptionSampler.sample returns -- DEVICE tensors only:
      tokens         [n, n_samp, Tmax] int32   the sampled captions, -1 past each row's length
      token_logprobs [n, n_samp, Tmax] fp32    the model's log-probability of every sampled token (temperature 1, whole vocabulary), 0 past the length
      token_q_logprobs [n, n_samp, Tmax] fp32  the proposal's log-probability of it (after top-k / temperature / top-p), 0 past the length
      seq_logprob / seq_q_logprob [n, n_samp] fp32   their left-to-right fp32 sums over the row's positions
      lengths        [n, n_samp] int32         generated tokens per ROW (an end token counts)."""

    def __init__(self, tokens, token_logprobs, token_q_logprobs, seq_logprob, seq_q_logprob, lengths):
        self.tokens, self.token_logprobs, self.token_q_logprobs = tokens, token_logprobs, token_q_logprobs
        self.seq_logprob, self.seq_q_logprob, self.lengths = seq_logprob, seq_q_logprob, lengths

    def captions(self, eos, pad, eos_dev=None):
        """The reference's cut at the first eos, then at the first pad, on the device (ops.beam_captions, called with every row as an
        instance of one hypothesis because lengths are per row): (cap_tokens [n, n_samp, Tmax] int32, -1 past the cut; cap_len
        [n, n_samp] int32).  `tokens` is left as it is."""
        n, ns, Tmax = self.tokens.shape
        cap, cap_len = ops.beam_captions(self.tokens.reshape(n * ns, 1, Tmax), self.lengths.reshape(n * ns), eos, pad, eos_dev=eos_dev)
        return cap.view(n, ns, Tmax), cap_len.view(n, ns)

    def hypotheses(self):
        """[n][n_samp] token lists -- the one place that copies to the host."""
        tok, lens = self.tokens.cpu().tolist(), self.lengths.cpu().tolist()
        return [[row[:lens[i][k]] for k, row in enumerate(inst)] for i, inst in enumerate(tok)]


class CaptionSampler(CachedDecoder):
    """Compiled sampling session for a fixed (n_inst, max_words W, max_frames F, n_samp, max_len, top_k).  temperature and top_p given
    here are the defaults of sample(); they, the seed and the end token live in device words and never force a new capture.
    Partial batches: n_active as in steps.InstanceSession; the rows of idle slots have `row_done` preset to 1."""

    def __init__(self, model, n_inst, W, F, n_samp=5, max_len=None, top_k=50, temperature=1.0, top_p=1.0, use_graphs=True, constraints=None):
        """constraints: a constrain.DecodeConstraints or None.  With one, univl_decode_constrain runs on the RAW logits between the
        vocabulary classifier and univl_sample_step (each row's prefix is its row of tokens_out), so the draw is from the masked
        distribution and tok_logprob / seq_logprob are log-probabilities UNDER THE MASKED LOGITS (renormalised over the unbanned columns),
        not the unconstrained model's.  top_k <= the number of unbanned columns of every live row is the caller's condition.  step_logits
        stays the unconstrained classifier output.  None adds no launch."""
        if not 1 <= int(n_samp) <= 8:
            raise ValueError("CaptionSampler: n_samp=%r, expected 1 .. 8" % (n_samp,))
        V = model.bert_config.vocab_size
        if not 1 <= int(top_k) <= min(SAMPLE_KMAX, V):
            raise ValueError("CaptionSampler: top_k=%r, expected 1 .. min(%d, vocabulary %d)" % (top_k, SAMPLE_KMAX, V))
        self._check_sampling(temperature, top_p)
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("CaptionSampler needs a model on a HIP device (got %s); there is no CPU fallback" % dev)
        self.n_samp, self.top_k, self.temperature, self.top_p = int(n_samp), int(top_k), float(temperature), float(top_p)
        super().__init__(model, n_inst, W, F, self.n_samp, n_inst * self.n_samp, max_len=max_len, use_graphs=use_graphs,
                         constraints=constraints)
        R, Tmax, dev = self.R, self.Tmax, self.cx.dev
        # ---- sampling state (read and written by univl_sample_step), all per ROW
        self.row_done = torch.zeros(R, dtype=torch.uint8, device=dev)
        self.row_length = torch.zeros(R, dtype=torch.int32, device=dev)
        self.tokens_out = torch.full((R, Tmax), -1, dtype=torch.int32, device=dev)
        self.tok_lp = torch.zeros(R, Tmax, device=dev)
        self.q_lp = torch.zeros(R, Tmax, device=dev)
        self.seq_lp = torch.zeros(R, device=dev)
        self.seq_q = torch.zeros(R, device=dev)
        self.sampling_dev = torch.tensor([1.0 / self.temperature, self.top_p], dtype=torch.float32, device=dev)
        self.seed_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self.sample_ws = ops.sample_ws(R, self.top_k, dev)

    @staticmethod
    def _check_sampling(temperature, top_p):
        if not (float(temperature) > 0.0 and float(temperature) != float("inf")):
            raise ValueError("CaptionSampler: temperature=%r, expected a finite value > 0" % (temperature,))
        if not float(top_p) > 0.0:
            raise ValueError("CaptionSampler: top_p=%r, expected a value > 0 (>= 1: no nucleus cut)" % (top_p,))

    # ------------------------------------------------------------------------------------------ step plans
    FORMS = ("logits", "sample")

    def _reorders(self, form):
        return False

    def _plan_tail(self, pl, t, form):
        """"logits": nothing after the vocabulary classifier (step_logits).  "sample": univl_sample_step on the raw logits."""
        if form == "logits":
            return
        if self.constraints is not None:
            c = self.constraints
            pl.add("univl_decode_constrain", ops.decode_constrain_desc(
                self.head.logits, self.V, t, prefix_in=self.tokens_out, done=self.row_done, done_stride=1, eos_dev=self.eos_dev,
                params_dev=c.params_dev, suppress=c.suppress_dev))
        pl.add("univl_sample_step", ops.sample_step_desc(
            self.head.logits, self.V, self.top_k, t, done=self.row_done, length=self.row_length, ids=self.ids,
            tokens_out=self.tokens_out, tok_logprob=self.tok_lp, q_logprob=self.q_lp, seq_logprob=self.seq_lp,
            seq_q_logprob=self.seq_q, ws=self.sample_ws, sampling_dev=self.sampling_dev, seed_dev=self.seed_dev, eos_dev=self.eos_dev))

    # ------------------------------------------------------------------------------------------------- run
    @torch.no_grad()
    def step_logits(self, t, last_tokens):
        """One cached decoder step of the sampling session: the RAW logits [R, V] of the token after position t, given each row's
        token at position t (the rows' cache holds positions [0, t) from the calls before).  The position plan without the sample
        tail; it neither reads nor advances the sampling state.  Exposed for the parity tests."""
        self.ids.copy_(last_tokens.reshape(-1))
        self._replay(self._step_plan(t, "logits"))
        return self.head.logits[:, :self.V]

    @torch.no_grad()
    def sample(self, sequence_output, visual_output, input_mask, video_mask, bos, eos, seed, max_len=None, sync_every=8, n_active=None,
               temperature=None, top_p=None):
        """n_samp sampled captions per instance over at most max_len positions; returns a SampleResult (device tensors).  seed: any
        integer (taken modulo 2^64).  temperature / top_p: None for the session's defaults.  sync_every: the host reads the done
        bytes every that many positions to stop early (0: never); finished rows are frozen, so the result does not depend on it."""
        ns = self.n_samp
        m = self._active(n_active)
        max_len = min(int(max_len or self.Tmax), self.Tmax)
        temperature = self.temperature if temperature is None else temperature
        top_p = self.top_p if top_p is None else top_p
        self._check_sampling(temperature, top_p)
        self.encode(sequence_output, visual_output, input_mask, video_mask, n_active=n_active)
        # state reset (outside the position loop)
        self.row_done.zero_()
        self.row_length.zero_()
        if m < self.n_inst:
            self.row_done[m * ns:].fill_(1)      # idle slots: done from the start, length 0
        self.tokens_out.fill_(-1)
        self.tok_lp.zero_()
        self.q_lp.zero_()
        self.seq_lp.zero_()
        self.seq_q.zero_()
        self.ids.fill_(int(bos))
        self.eos_dev.fill_(int(eos))
        s = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.seed_dev.fill_(s - (1 << 64) if s >= (1 << 63) else s)          # the word's 64 bits in int64 storage
        self.sampling_dev[0:1].fill_(1.0 / float(temperature))               # rounded to fp32 once: the contract's inv_T
        self.sampling_dev[1:2].fill_(float(top_p))
        self._run_positions("sample", max_len, sync_every, self.row_done)
        R = m * ns
        view = lambda x: x[:R].view(m, ns, *x.shape[1:]).clone()
        return SampleResult(view(self.tokens_out), view(self.tok_lp), view(self.q_lp), view(self.seq_lp), view(self.seq_q),
                            view(self.row_length))
