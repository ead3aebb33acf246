"""Reward-weighted caption training: learn from sampled captions and their scores.

The caption side can draw several captions per video with every token's log-probability on the device (sample.CaptionSampler), score a
caption against references on the device (univl_caption_overlap, csrc/metric.hip) and form teacher-forced inputs from decoded tokens
(score.beam_inputs_labels).  This module closes the loop:

  caption_rewards  sampled captions against each video's references -> rewards [n, n_samp] fp64            (one overlap launch)
  advantages       rewards -> per-caption weights [n, n_samp] fp32: leave-one-out or a given baseline     (univl_caption_advantage)
  scst_step        sample -> reward -> advantage -> UniVL.forward(..., caption_weight=A): the loss of one self-critical
                   sequence-training step; the caller does backward() / clip / optimizer.step()

The loss is sum_r w_r nll_r / n_valid over the counting positions of all sampled captions (univl_vocab_ce_weighted_fwd / _bwd: the
[tokens, 30522] logits never exist), so its gradient is the REINFORCE estimate with the advantage as the weight.  Everything between
the end of sampling and the returned loss stays on the device: no score is read on the host.
"""
import collections

import torch

from . import ops
from ._lib import OVERLAP_TMAX
from .caption_metrics import DocumentFrequency
from .score import beam_inputs_labels

_LAYOUTS = {}


def _reward_layout(n, ns, n_ref, dev):
    """Item tables of "every sample against the references of its video" over the concatenated symbol matrix (n * ns sample rows, then
    n * n_ref reference rows), built with device arithmetic once per shape."""
    key = (n, ns, n_ref, str(dev))
    if key not in _LAYOUTS:
        items = n * ns
        item = torch.arange(items, dtype=torch.int32, device=dev)
        ref = torch.arange(n_ref, dtype=torch.int32, device=dev)[None, :]
        refs = items + (item // ns)[:, None] * n_ref + ref
        _LAYOUTS[key] = (item, torch.arange(items + 1, dtype=torch.int32, device=dev) * n_ref, refs.reshape(-1).to(torch.int32).contiguous())
    return _LAYOUTS[key]


def caption_rewards(sample_result, ref_ids, ref_len, eos, pad, metric="rouge_l", eos_dev=None, return_stats=False, df=None):
    """The reward of every sampled caption: its ROUGE_L ("rouge_l"), sentence BLEU-4 ("bleu") or CIDEr-D ("cider") against the
    references of its video, [n, n_samp] fp64 on the device.  The samples are the rows of SampleResult.captions(eos, pad); ref_ids [n, n_ref, T] holds each
    video's references and ref_len [n, n_ref] their lengths (integer tensors; positions past a length are not read).

    PIECE-level, as caption_metrics.consensus is: the symbols are piece ids after the cut, not words -- "##" continuation pieces count
    as symbols of their own -- so the numbers are not those of a word-level evaluation of the detokenised text.

    metric="cider" needs df, a caption_metrics.DocumentFrequency on the samples' device (DocumentFrequency.from_ids over the training
    set's references, built once): the kernel's clipped tf-idf with the Gaussian length penalty of sigma 6, idf from df.n_docs documents.
    The values carry CIDEr's factor 10 -- `scale` of advantages / scst_step exists for that.  The other metrics ignore df.

    One ops.caption_overlap launch over the concatenated symbol matrix; nothing is read on the host (so the launch's status word is not
    looked at: piece ids above 65534 would be clamped).  return_stats: also the launch's whole output dictionary (guess / correct
    [n * n_samp, 4], hyp_len, ref_len, lcs, rouge_l, bleu, status)."""
    if metric not in ("rouge_l", "bleu", "cider"):
        raise ValueError("caption_rewards: metric=%r, expected 'rouge_l', 'bleu' or 'cider'" % (metric,))
    tokens = sample_result.tokens
    if metric == "cider":
        if not isinstance(df, DocumentFrequency):
            raise ValueError("caption_rewards: metric='cider' needs df, a caption_metrics.DocumentFrequency (got %s)" % type(df).__name__)
        if df.n_docs < 1:
            raise ValueError("caption_rewards: metric='cider' with a document-frequency table of %d documents" % df.n_docs)
        if df.device != tokens.device:
            raise ValueError("caption_rewards: metric='cider' with df on %s, the samples are on %s" % (df.device, tokens.device))
    if tokens.dim() != 3:
        raise ValueError("caption_rewards: sampled tokens of shape %s, expected [n, n_samp, Tmax]" % (tuple(tokens.shape),))
    n, ns, Tmax = tokens.shape
    if ref_ids.dim() != 3 or ref_ids.shape[0] != n or ref_ids.shape[1] < 1 or ref_ids.shape[2] < 1:
        raise ValueError("caption_rewards: ref_ids of shape %s, expected [%d, n_ref, T] with n_ref, T >= 1 (one row of references per video)"
                         % (tuple(ref_ids.shape), n))
    n_ref, T = int(ref_ids.shape[1]), int(ref_ids.shape[2])
    if tuple(ref_len.shape) != (n, n_ref):
        raise ValueError("caption_rewards: ref_len of shape %s, expected [%d, %d]" % (tuple(ref_len.shape), n, n_ref))
    if ref_ids.is_floating_point() or ref_len.is_floating_point():
        raise ValueError("caption_rewards: ref_ids / ref_len must be integer tensors")
    if max(Tmax, T) > OVERLAP_TMAX:
        raise ValueError("caption_rewards: rows of %d positions; the kernel carries at most %d" % (max(Tmax, T), OVERLAP_TMAX))
    cap, cap_len = sample_result.captions(eos, pad, eos_dev=eos_dev)
    dev, Tw = cap.device, max(Tmax, T)
    sym = torch.zeros(n * (ns + n_ref), Tw, dtype=torch.int32, device=dev)
    sym[:n * ns, :Tmax] = cap.view(n * ns, Tmax)
    sym[n * ns:, :T] = ref_ids.to(dev).reshape(n * n_ref, T)
    lens = torch.cat([cap_len.reshape(-1), ref_len.to(dev).reshape(-1).to(torch.int32)]).contiguous()
    hyp_row, ref_begin, ref_rows = _reward_layout(n, ns, n_ref, dev)
    o = ops.caption_overlap(sym, lens, hyp_row, ref_begin, ref_rows, n * ns * n_ref, bleu=(metric == "bleu"),
                            tables=df.tables if metric == "cider" else None)
    r = o[metric].view(n, ns)
    return (r, o) if return_stats else r


def advantages(rewards, baseline="loo", scale=1.0, status=None):
    """Rewards [n, n_samp] fp64 -> per-caption training weights [n, n_samp] fp32 (univl_caption_advantage, one launch, no host read).
    baseline "loo": every sample against the mean reward of its video's OTHER samples (needs n_samp >= 2); a tensor [n]: that reward
    per video, e.g. the greedy or beam caption's.  The difference is multiplied by `scale` in fp64 and rounded once.  A non-finite
    reward gives weight 0 and sets bit 0 of `status` (an int32 device word; default: a fresh one nobody reads)."""
    if rewards.dim() != 2 or rewards.dtype != torch.float64:
        raise ValueError("advantages: rewards of shape %s and dtype %s, expected [n, n_samp] float64" % (tuple(rewards.shape), rewards.dtype))
    n, ns = rewards.shape
    if n < 1 or ns < 1:
        raise ValueError("advantages: rewards of shape %s, expected at least one video and one sample" % (tuple(rewards.shape),))
    if isinstance(baseline, str):
        if baseline != "loo":
            raise ValueError("advantages: baseline=%r, expected 'loo' or a tensor of one reward per video" % (baseline,))
        if ns < 2:
            raise ValueError("advantages: the leave-one-out baseline needs at least 2 samples per video (got %d)" % ns)
        b = None
    else:
        if not isinstance(baseline, torch.Tensor) or baseline.numel() != n:
            raise ValueError("advantages: baseline of shape %s, expected one reward per video ([%d])"
                             % (tuple(getattr(baseline, "shape", ())), n))
        b = baseline
    if not float(scale) == float(scale) or float(scale) in (float("inf"), float("-inf")):
        raise ValueError("advantages: scale=%r, expected a finite number" % (scale,))
    if not rewards.is_cuda:
        raise RuntimeError("advantages needs HIP device tensors (got %s); there is no CPU fallback" % rewards.device)
    if b is not None:
        b = b.to(rewards.device, torch.float64).reshape(n).contiguous()
    weight, _ = ops.caption_advantage(rewards.contiguous(), b, scale, status)
    return weight


ScstResult = collections.namedtuple("ScstResult", "loss rewards advantages lengths samples")
ScstResult.__doc__ = """What scst_step returns: loss (UniVL.forward's loss tensor: backward() / float() as usual) and the device tensors rewards
[n, n_samp] fp64, advantages [n, n_samp] fp32, lengths [n, n_samp] int32 (sampled tokens per caption, an end token counts); samples
is the sample.SampleResult they were computed from."""


def scst_step(model, sampler, batch, ref_ids, ref_len, bos, eos, pad, seed, metric="rouge_l", baseline="loo", scale=1.0, df=None):
    """One self-critical sequence-training step up to the loss.  batch: the five encoder inputs of UniVL.forward (a dict with
    input_ids, token_type_ids, attention_mask, video, video_mask, or that tuple); sampler: a sample.CaptionSampler of this model for
    the batch's shape; ref_ids / ref_len / metric / df as in caption_rewards (metric="cider" needs df); baseline / scale as in advantages.

      1. encoder features in evaluation form (UniVL.get_sequence_visual_output: no dropout; a pending optimizer update is applied first)
      2. sampler.sample(...): n_samp captions per video
      3. rewards (caption_rewards) and advantages
      4. teacher-forced inputs, labels (-1 past the end token) and decoder masks from the sampled tokens (score.beam_inputs_labels)
      5. model.forward(..., caption_weight=advantages) in training mode

    Returns a ScstResult.  The caller does loss.backward(), clip_grad_norm_ and optimizer.step().  Between the end of sampling and the
    return nothing is read on the host; the sampler's own `done` bytes are the only host read of the whole call."""
    if not model.training:
        raise RuntimeError("scst_step: the model must be in training mode (model.train())")
    if isinstance(batch, dict):
        batch = tuple(batch[k] for k in ("input_ids", "token_type_ids", "attention_mask", "video", "video_mask"))
    input_ids, token_type_ids, attention_mask, video, video_mask = batch
    W = input_ids.shape[-1]
    B = input_ids.numel() // W
    if ref_ids.dim() != 3 or ref_ids.shape[0] != B or tuple(ref_len.shape) != tuple(ref_ids.shape[:2]):
        raise ValueError("scst_step: ref_ids of shape %s / ref_len of shape %s, expected [%d, n_ref, T] / [%d, n_ref]"
                         % (tuple(ref_ids.shape), tuple(ref_len.shape), B, B))
    if not 1 <= B <= sampler.n_inst:
        raise ValueError("scst_step: a batch of %d videos, the sampler was built for at most %d" % (B, sampler.n_inst))
    with torch.no_grad():
        seq, vis = model.get_sequence_visual_output(input_ids, token_type_ids, attention_mask, video, video_mask)
        am = attention_mask.reshape(B, W)
        vm = video_mask.reshape(B, video_mask.shape[-1])
        res = sampler.sample(seq, vis, am, vm, bos, eos, seed, n_active=None if B == sampler.n_inst else B)
        # ---- from here on: device work only
        rewards = caption_rewards(res, ref_ids, ref_len, eos, pad, metric=metric, eos_dev=sampler.eos_dev, df=df)
        adv = advantages(rewards, baseline=baseline, scale=scale)
        inputs, labels, mask = beam_inputs_labels(res.tokens, res.lengths, bos, eos, pad, res.tokens.shape[-1])
    loss = model(input_ids, token_type_ids, attention_mask, video, video_mask, input_caption_ids=inputs, decoder_mask=mask,
                 output_caption_ids=labels, caption_weight=adv)
    return ScstResult(loss, rewards, adv, res.lengths, res)
