"""Evaluation entry points for callers that can be edited: eval_retrieval, eval_retrieval_streamed, eval_caption and eval_caption_loss (below).

Retrieval: the device-resident equivalent of main_task_retrieval.py:367-450 (`_run_on_single_gpu`,
`eval_epoch`) for callers that can be edited.  The unchanged script keeps working through UniVL.get_* and
nn.parallel.replicate (tests/test_eval_gpu.py); these helpers avoid its per-block D2H copies and numpy concatenations:
all blocks of the N_t x N_v similarity matrix are written into one device tensor and the metrics need 2 N integers
from the GPU (univl_amd.metrics).

Caption: eval_caption is the body of main_task_caption.py:490-618 (`eval_epoch`) around ONE decoding session
(univl_amd.decode.CaptionBeamSearch) that every batch of the loader reuses, the short last one included (n_active); the
reference's cut of each hypothesis at "[SEP]" / "[PAD]" runs on the device (univl_beam_captions) and each batch is copied to the
host once.

Caption likelihood: eval_caption_loss is the validation loss the caption task's training never reports -- the teacher-forced
CrossEntropyLoss(ignore_index=-1) of modeling.py:246-254 over a whole loader, with perplexity and token accuracy, around ONE scoring
session (univl_amd.score.CaptionScorer).

Localisation: eval_localization scores where in its own video every text is found (retrieval.VideoIndex.localize) against annotated
segments: mIoU and R1@0.3 / 0.5 / 0.7 over frame indices, and with n_best = n the R{n}@ columns over the n windows that temporal
non-maximum suppression leaves.  eval_step_alignment does it for ORDERED lists of steps laid over their video
jointly (retrieval.VideoIndex.align_steps): step recall by the centre frame of every step's window, and mIoU.  eval_segmentation
labels every frame of a video out of a set of label texts (retrieval.VideoIndex.segment) and counts COIN's frame accuracy;
eval_label_transfer counts the same for labels carried over from an annotated exemplar video (retrieval.VideoIndex.align_videos)."""
import contextlib
import math
import os

import numpy as np

import torch

from .metrics import compute_metrics


@torch.no_grad()
def similarity_matrix(model, masks_t, masks_v, seq_outs, vis_outs):
    """masks_t[i] / seq_outs[i]: attention mask (b_i, W) and text features (b_i, W, 768) of text batch i; likewise for the
    video batches.  Returns the (sum b_i) x (sum b_j) fp32 device tensor of get_similarity_logits blocks."""
    nt = sum(int(s.shape[0]) for s in seq_outs)
    nv = sum(int(v.shape[0]) for v in vis_outs)
    out = torch.empty(nt, nv, device=seq_outs[0].device, dtype=torch.float32)
    r = 0
    for mt, so in zip(masks_t, seq_outs):
        c = 0
        for mv, vo in zip(masks_v, vis_outs):
            blk = model.get_similarity_logits(so, vo, mt, mv)
            out[r:r + so.shape[0], c:c + vo.shape[0]] = blk
            c += vo.shape[0]
        r += so.shape[0]
    return out


@torch.no_grad()
def eval_retrieval(model, batches, device="cuda"):
    """batches: iterable of (input_ids, input_mask, segment_ids, video, video_mask, ...) tuples in the reference
    loader's order (main_task_retrieval.py:396).  Returns (metrics dict, similarity matrix on the device)."""
    masks_t, masks_v, seqs, viss = [], [], [], []
    with _eval_mode(model):
        for batch in batches:
            input_ids, input_mask, segment_ids, video, video_mask = [t.to(device) for t in batch[:5]]
            so, vo = model.get_sequence_visual_output(input_ids, segment_ids, input_mask, video, video_mask)
            seqs.append(so)
            viss.append(vo)
            masks_t.append(input_mask.reshape(-1, input_mask.shape[-1]))
            masks_v.append(video_mask.reshape(-1, video_mask.shape[-1]))
        sim = similarity_matrix(model, masks_t, masks_v, seqs, viss)
    return compute_metrics(sim), sim


@contextlib.contextmanager
def _eval_mode(model):
    """model.eval() for the block; model.training is put back however the block ends."""
    was_training = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(was_training)


def _text_rows(who, text_batches, n, device):
    """The walk both target-per-text evaluators make: yields (input_ids, segment_ids, input_mask, row, b) for every text batch moved to
    `device`, row the batch's first text row and b its rows.  ValueError, in `who`'s name, when the batches hold more or fewer than n rows."""
    row = 0
    for batch in text_batches:
        input_ids, input_mask, segment_ids = [t.to(device) for t in batch[:3]]
        b = input_ids.numel() // input_ids.shape[-1]
        if row + b > n:
            raise ValueError("%s: more text rows than targets (%d)" % (who, n))
        yield input_ids, segment_ids, input_mask, row, b
        row += b
    if row != n:
        raise ValueError("%s: %d text rows for %d targets" % (who, row, n))


@torch.no_grad()
def eval_retrieval_streamed(model, text_batches, video_batches, targets, device="cuda", capacity=1024, bank_batches=None, beta=20.0,
                            hub_k=1, dynamic=True):
    """Retrieval metrics without the N_t x N_v matrix and without a paired test set.  video_batches: iterable of (video, video_mask);
    text_batches: iterable of (input_ids, input_mask, segment_ids), the loader's order (main_task_retrieval.py:396); targets: for
    every text row, in order, the gallery row (= position among all videos added) that is its ground truth -- several texts may name
    one video, and the number of texts need not be the number of videos.  The videos go into a retrieval.VideoIndex, every text batch
    is searched for its two rank counts only (univl_sim_topk with k = 0), and R@1 / R@5 / R@10 / MR come from the counts through
    metrics.compute_metrics.  Joint-head similarity only (what VideoIndex holds).  Returns (metrics dict, (gt, eq) host arrays).
    bank_batches: an iterable of text batches like text_batches (training captions, say); they fill a retrieval.QueryBank(beta, hub_k,
    dynamic) and the counts, hence the metrics, are those of the query-bank normalised score.  None: the raw score, as ever."""
    from .retrieval import QueryBank, VideoIndex, check_bank_args
    if bank_batches is not None:
        check_bank_args(beta, hub_k)
    with _eval_mode(model):
        index = VideoIndex(model, capacity=capacity)
        for video, video_mask in video_batches:
            index.add(video.to(device), video_mask.to(device))
        bank = None
        if bank_batches is not None:
            bank = QueryBank(index, beta=beta, hub_k=hub_k, dynamic=dynamic)
            for batch in bank_batches:
                input_ids, input_mask, segment_ids = [t.to(device) for t in batch[:3]]
                bank.add(input_ids, segment_ids, input_mask)
            bank.fit()
        targets = torch.as_tensor(targets).reshape(-1).to(device=device, dtype=torch.int32)
        if targets.numel() and (int(targets.min()) < 0 or int(targets.max()) >= len(index)):
            raise ValueError("eval_retrieval_streamed: targets must lie in [0, %d)" % len(index))
        gts, eqs = [], []
        for input_ids, segment_ids, input_mask, row, b in _text_rows("eval_retrieval_streamed", text_batches, targets.numel(), device):
            gt, eq = index.search(input_ids, segment_ids, input_mask, k=0, targets=targets[row:row + b], bank=bank)
            gts.append(gt)
            eqs.append(eq)
    gt, eq = torch.cat(gts).cpu().numpy(), torch.cat(eqs).cpu().numpy()
    return compute_metrics((gt, eq)), (gt, eq)


@torch.no_grad()
def eval_localization(model, index, text_batches, targets, gt_start, gt_len, window, device="cuda", n_best=1, nms=(1, 2)):
    """Step localisation: every text is localised in ITS OWN video and the window found is compared with the annotated one.
    index: a retrieval.VideoIndex(model, keep_frames=True) holding the videos; text_batches: iterable of (input_ids, input_mask,
    segment_ids), the loader's order; targets / gt_start / gt_len: for every text row, in order, its gallery row and its annotated
    segment, frames gt_start .. gt_start + gt_len - 1 (gt_len >= 1); window = (lmin, lmax): the lengths searched
    (VideoIndex.localize).  Temporal IoU over frame indices; a threshold is decided in integers (10 * inter >= 3 * union, ...), so no
    rounding enters a count.  A text whose video has no candidate window counts as IoU 0 and is reported in n_empty.
    Returns {"mIoU", "R1@0.3", "R1@0.5", "R1@0.7"} (fractions of the n texts; mIoU a float64 mean taken on the host), "n", "n_empty".
    n_best = n > 1 (at most MOMENT_NBEST_MAX): every text is localised with VideoIndex.localize(n_best=n, nms=nms) and the dictionary
    gains "R{n}@0.3", "R{n}@0.5", "R{n}@0.7": a text counts if ANY of its n windows meets the same integer threshold -- the "R@n, IoU = m"
    columns of the moment-retrieval tables.  mIoU, R1@ and n_empty are those of slot 0, the window of n_best = 1.  Still one host read."""
    from .retrieval import check_nbest
    if index.model is not model:
        raise ValueError("eval_localization: the index belongs to another model")
    if n_best is None:
        raise ValueError("eval_localization: n_best=None, need an integer (1: the best window alone)")
    check_nbest("eval_localization", n_best, nms)
    many = {"n_best": n_best, "nms": nms} if n_best > 1 else {}           # n_best = 1: the call, the launch and the dictionary of before
    as_i32 = lambda x: torch.as_tensor(x).reshape(-1).to(device=device, dtype=torch.int32)
    targets, gt_start, gt_len = as_i32(targets), as_i32(gt_start), as_i32(gt_len)
    n = targets.numel()
    if gt_start.numel() != n or gt_len.numel() != n:
        raise ValueError("eval_localization: %d targets, %d gt_start, %d gt_len" % (n, gt_start.numel(), gt_len.numel()))
    if n and (int(targets.min()) < 0 or int(targets.max()) >= len(index) or int(gt_len.min()) < 1 or int(gt_start.min()) < 0):
        raise ValueError("eval_localization: targets must lie in [0, %d), gt_start >= 0 and gt_len >= 1" % len(index))
    starts, lengths = [], []
    with _eval_mode(model):
        for input_ids, segment_ids, input_mask, row, b in _text_rows("eval_localization", text_batches, n, device):
            s, l, _ = index.localize(input_ids, segment_ids, input_mask, targets[row:row + b].reshape(b, 1), window, **many)
            starts.append(s.reshape(b, -1))
            lengths.append(l.reshape(b, -1))
    if n == 0:
        raise ValueError("eval_localization: no texts")
    s, l = torch.cat(starts), torch.cat(lengths)                          # [n, n_best]; an empty slot is (-1, 0): it meets no frame
    g0, g1 = gt_start[:, None], (gt_start + gt_len)[:, None]
    inter = (torch.minimum(s + l, g1) - torch.maximum(s, g0)).clamp_(min=0)
    inter = torch.where(l > 0, inter, torch.zeros_like(inter))
    union = l + gt_len[:, None] - inter
    host = torch.stack([inter, union, l]).cpu().numpy().astype(np.int64)  # the one host read
    inter, union, l = host
    out = {"mIoU": float(np.mean(inter[:, 0].astype(np.float64) / union[:, 0].astype(np.float64)))}
    for name, num in (("R1@0.3", 3), ("R1@0.5", 5), ("R1@0.7", 7)):
        out[name] = float(np.sum(10 * inter[:, 0] >= num * union[:, 0])) / n
    out["n"], out["n_empty"] = n, int(np.sum(l[:, 0] == 0))
    if n_best > 1:
        for num in (3, 5, 7):
            out["R%d@0.%d" % (n_best, num)] = float(np.sum(np.any(10 * inter >= num * union, axis=1))) / n
    return out


def eval_step_alignment(model, index, step_batches, targets, gt_start, gt_len, window, device="cuda"):
    """Action step localisation: every ordered list of steps is laid over ITS OWN video (VideoIndex.align_steps: all steps at once, in
    order, never overlapping) and each step's window is compared with the annotated one.  index: a retrieval.VideoIndex(model,
    keep_frames=True) holding the videos; step_batches: iterable of (input_ids [b, K, W], input_mask, segment_ids, counts [b]), the
    loader's order -- a list's steps are its first counts texts; targets [n]: every list's gallery row; gt_start, gt_len [n, K]: step
    k's annotated segment, frames gt_start .. gt_start + gt_len - 1, with gt_len == 0 for a step that is not annotated in this video:
    it is still aligned (it holds its place in the order) but stays out of every denominator, as do the slots past counts; window =
    (lmin, lmax): the length of a step's window -- with (1, 1) the recall is CrossTask's.  A list whose video cannot hold its steps
    (or whose count is outside [1, K]) is infeasible: all its annotated steps are misses with IoU 0.  Returns, from one host read,
      "recall"    annotated steps whose window's centre frame start + (length - 1) // 2 lies in the annotated segment / n_steps
      "mIoU"      mean temporal IoU over the annotated steps (a float64 mean taken on the host over integer counts)
      "n_lists", "n_steps" (annotated steps), "n_infeasible" (lists)
      "hits", "annotated"   int64 arrays [n]: per list, for a macro average per task."""
    if index.model is not model:
        raise ValueError("eval_step_alignment: the index belongs to another model")
    targets = torch.as_tensor(targets).reshape(-1).to(device=device, dtype=torch.int32)
    gt_start, gt_len = (torch.as_tensor(x).to(device=device, dtype=torch.int32) for x in (gt_start, gt_len))
    n = targets.numel()
    if gt_start.dim() != 2 or gt_start.shape != gt_len.shape or gt_start.shape[0] != n:
        raise ValueError("eval_step_alignment: %d targets, gt_start %s, gt_len %s (both [lists, steps])"
                         % (n, tuple(gt_start.shape), tuple(gt_len.shape)))
    if n == 0:
        raise ValueError("eval_step_alignment: no lists")
    if int(targets.min()) < 0 or int(targets.max()) >= len(index) or int(gt_len.min()) < 0 or int(gt_start.min()) < 0:
        raise ValueError("eval_step_alignment: targets must lie in [0, %d), gt_start >= 0 and gt_len >= 0" % len(index))
    K = gt_start.shape[1]
    starts, lengths, totals, steps = [], [], [], []
    row = 0
    with _eval_mode(model):
        for batch in step_batches:
            input_ids, input_mask, segment_ids, counts = [t.to(device) for t in batch[:4]]
            b = input_ids.shape[0]
            if input_ids.dim() != 3 or input_ids.shape[1] != K or counts.numel() != b:
                raise ValueError("eval_step_alignment: a batch of shape %s with %d counts, the annotation holds %d steps per list"
                                 % (tuple(input_ids.shape), counts.numel(), K))
            if row + b > n:
                raise ValueError("eval_step_alignment: more lists than targets (%d)" % n)
            s, l, _, tot = index.align_steps(input_ids, segment_ids, input_mask, counts, targets[row:row + b].reshape(b, 1), window)
            starts.append(s[:, 0])
            lengths.append(l[:, 0])
            totals.append(tot[:, 0])
            steps.append(counts.reshape(b).to(torch.int32))
            row += b
    if row != n:
        raise ValueError("eval_step_alignment: %d lists for %d targets" % (row, n))
    s, l, steps = torch.cat(starts), torch.cat(lengths), torch.cat(steps)          # an empty slot is (-1, 0): it meets no frame
    annotated = (gt_len > 0) & (torch.arange(K, device=s.device)[None, :] < steps[:, None])
    centre = s + torch.div(l - 1, 2, rounding_mode="floor")
    hit = annotated & (l > 0) & (centre >= gt_start) & (centre < gt_start + gt_len)
    inter = (torch.minimum(s + l, gt_start + gt_len) - torch.maximum(s, gt_start)).clamp_(min=0)
    inter = torch.where(l > 0, inter, torch.zeros_like(inter))
    union = l + gt_len - inter
    infeasible = torch.isinf(torch.cat(totals)).to(torch.int32)
    host = torch.cat([t.to(torch.int32).reshape(-1) for t in (hit, annotated, inter, union, infeasible)]).cpu().numpy().astype(np.int64)
    hit, annotated, inter, union = (host[i * n * K:(i + 1) * n * K].reshape(n, K) for i in range(4))       # the one host read
    n_steps = int(annotated.sum())
    if n_steps == 0:
        raise ValueError("eval_step_alignment: no annotated step")
    on = annotated != 0
    return {"recall": float(hit.sum()) / n_steps, "mIoU": float(np.mean(inter[on].astype(np.float64) / union[on].astype(np.float64))),
            "n_lists": n, "n_steps": n_steps, "n_infeasible": int(host[4 * n * K:].sum()), "hits": hit.sum(1), "annotated": annotated.sum(1)}


def eval_segmentation(model, index, label_batches, targets, gt_labels, switch_penalty=0.0, background=None, device="cuda"):
    """Action segmentation: every frame of a video gets one of a set of label texts or the background (VideoIndex.segment), each set in
    ITS OWN video, and the labels are compared with the annotated ones frame by frame -- COIN's frame accuracy, here in its zero-shot,
    label-text form.  index: a retrieval.VideoIndex(model, keep_frames=True) holding the videos; label_batches: iterable of (input_ids
    [b, K, W], input_mask, segment_ids, counts [b]), the loader's order -- a set's labels are its first counts texts; targets [n]: every
    set's gallery row; gt_labels [n, F] integers: k for label k of the set, -1 for the background, -2 for a frame that is not annotated
    and is never counted; a frame the video's mask excludes is not counted either.  switch_penalty, background: as VideoIndex.segment's.
    Every decision is an integer comparison.  Returns, from one host read,
      "frame_accuracy"      correct / annotated over all annotated valid frames
      "frame_accuracy_fg"   the same over the frames whose annotation is a label, not the background (NaN without one)
      "correct", "annotated"   int64 arrays [n]: per set, for a macro average per task
      "n_lists", "n_frames" (annotated valid frames), "n_segments" (predicted runs of one label), "n_empty" (sets with nothing to
      label: no valid frame, or a count outside [1, K])."""
    from .retrieval import check_segment_args
    if index.model is not model:
        raise ValueError("eval_segmentation: the index belongs to another model")
    check_segment_args("eval_segmentation", switch_penalty, background)
    targets = torch.as_tensor(targets).reshape(-1).to(device=device, dtype=torch.int32)
    gt = torch.as_tensor(gt_labels).to(device=device, dtype=torch.int32)
    n = targets.numel()
    if gt.dim() != 2 or gt.shape[0] != n:
        raise ValueError("eval_segmentation: %d targets, gt_labels %s (need [lists, frames])" % (n, tuple(gt.shape)))
    if n == 0:
        raise ValueError("eval_segmentation: no lists")
    if int(targets.min()) < 0 or int(targets.max()) >= len(index) or int(gt.min()) < -2:
        raise ValueError("eval_segmentation: targets must lie in [0, %d) and gt_labels be >= -2" % len(index))
    labels, totals, nsegs = [], [], []
    row = 0
    with _eval_mode(model):
        for batch in label_batches:
            input_ids, input_mask, segment_ids, counts = [t.to(device) for t in batch[:4]]
            b = input_ids.shape[0]
            if input_ids.dim() != 3 or counts.numel() != b:
                raise ValueError("eval_segmentation: a batch of shape %s with %d counts (need [lists, labels, words] and one count per list)"
                                 % (tuple(input_ids.shape), counts.numel()))
            if row + b > n:
                raise ValueError("eval_segmentation: more lists than targets (%d)" % n)
            lab, _, tot, ns = index.segment(input_ids, segment_ids, input_mask, counts, targets[row:row + b].reshape(b, 1), switch_penalty,
                                            background)
            if lab.shape[2] != gt.shape[1]:
                raise ValueError("eval_segmentation: gt_labels holds %d frames per list, the videos %d" % (gt.shape[1], lab.shape[2]))
            labels.append(lab[:, 0])
            totals.append(tot[:, 0])
            nsegs.append(ns[:, 0])
            row += b
    if row != n:
        raise ValueError("eval_segmentation: %d lists for %d targets" % (row, n))
    lab = torch.cat(labels)                                               # [n, F]; -2 on a masked frame
    per_list = list(frame_label_counts(lab, gt))
    host = torch.stack(per_list + [torch.cat(nsegs), torch.isinf(torch.cat(totals)).to(torch.int32)]).cpu().numpy().astype(np.int64)
    correct, annotated, correct_fg, annotated_fg, nseg, empty = host                                                 # the one host read
    n_frames, n_fg = int(annotated.sum()), int(annotated_fg.sum())
    if n_frames == 0:
        raise ValueError("eval_segmentation: no annotated valid frame")
    return {"frame_accuracy": float(correct.sum()) / n_frames, "frame_accuracy_fg": float(correct_fg.sum()) / n_fg if n_fg else float("nan"),
            "correct": correct, "annotated": annotated, "n_lists": n, "n_frames": n_frames, "n_segments": int(nseg.sum()),
            "n_empty": int(empty.sum())}


def frame_label_counts(pred, gt):
    """The counters of eval_segmentation and eval_label_transfer for labels pred [.., F] (-1 background or not on the path, -2 a masked frame) against annotations
    gt of the same shape (-2: not annotated): per-pair (correct, annotated, correct_fg, annotated_fg) as one [4, P, C] int32 device
    tensor.  A frame counts if it is annotated and not masked; every decision is an integer comparison."""
    counted = (gt != -2) & (pred != -2)
    right = counted & (pred == gt)
    fg = counted & (gt >= 0)
    return torch.stack([t.to(torch.int32).sum(-1, dtype=torch.int32) for t in (right, counted, right & fg, fg)])


def eval_label_transfer(index, ref, ref_labels, rows, gt_labels, tau=1.0):
    """One-shot label transfer: the frame labels of annotated exemplar videos are carried to other videos of the same task along a
    global alignment (VideoIndex.align_videos with local=False, then transfer_labels) and compared with those videos' annotations frame
    by frame -- eval_segmentation's counters and conventions.  index: a retrieval.VideoIndex(keep_frames=True); ref [P]: the exemplars'
    gallery rows; ref_labels [P, F] integers >= -1: their frame labels (-1 the background); rows [P, C]: the videos labelled from each;
    gt_labels [P, C, F]: their annotations, k, -1 for the background, -2 for a frame that is not annotated and is never counted; a
    frame the video's mask excludes is not counted either.  Returns, from one host read,
      "frame_accuracy"      correct / annotated over all annotated valid frames
      "frame_accuracy_fg"   the same over the frames annotated with a label, not the background (NaN without one)
      "correct", "annotated"   int64 arrays [P, C]: per pair
      "n_pairs", "n_frames" (annotated valid frames), "n_empty" (pairs with nothing to align)."""
    result = index.align_videos(ref, rows, tau, False)
    P, C, F = result.match.shape
    dev = result.match.device
    gt = torch.as_tensor(gt_labels).to(device=dev, dtype=torch.int32)
    if gt.shape != (P, C, F):
        raise ValueError("eval_label_transfer: gt_labels %s for %d exemplars, %d candidates each, %d frames" % (tuple(gt.shape), P, C, F))
    pred = index.transfer_labels(ref_labels, result)
    counts = frame_label_counts(pred, gt)
    empty = (result.path_len == 0).to(torch.int32).unsqueeze(0)
    host = torch.cat([counts, empty]).cpu().numpy().astype(np.int64)                                                 # the one host read
    correct, annotated, correct_fg, annotated_fg, empty = host
    n_frames, n_fg = int(annotated.sum()), int(annotated_fg.sum())
    if n_frames == 0:
        raise ValueError("eval_label_transfer: no annotated valid frame")
    return {"frame_accuracy": float(correct.sum()) / n_frames, "frame_accuracy_fg": float(correct_fg.sum()) / n_fg if n_fg else float("nan"),
            "correct": correct, "annotated": annotated, "n_pairs": P * C, "n_frames": n_frames, "n_empty": int(empty.sum())}


def ids_to_caption(tokenizer, ids):
    """Token ids -> caption text, exactly as main_task_caption.py:554-562 (hypotheses) and :566-574 (ground truth) do it: cut at
    the first "[SEP]", then at the first "[PAD]", join with ' ', glue "##" pieces.  (`.strip("##")` strips the CHARACTER '#' from
    both ends, as the reference does.)"""
    toks = tokenizer.convert_ids_to_tokens([int(i) for i in ids])
    if "[SEP]" in toks:
        toks = toks[:toks.index("[SEP]")]
    if "[PAD]" in toks:
        toks = toks[:toks.index("[PAD]")]
    return ' '.join(toks).replace(" ##", "").strip("##").strip()


class CaptionEvalResult:
    """What eval_caption returns.  Items are in loader order.
      hyps     list[str]             the best hypothesis of every item (what the reference writes to hyp.txt)
      refs     list[str]             pairs_output_caption_ids through the same id-to-text rule: the SINGLE-reference list.  The
                                     MSRVTT regrouping of main_task_caption.py:599-607 needs the dataset object and is the caller's.
      hyp_ids  list[list[list[int]]] [item][k] token ids of the k-th best hypothesis after the "[SEP]" / "[PAD]" cut, k < n_best
      scores   [items, n_best] fp32  accumulated log-probabilities, non-increasing in k (host tensor)
      lengths  [items] int32         generated tokens per item, before the cut (host tensor)
      metrics  nlg_eval.compute_metrics(ref_list=[refs], hyp_list=hyps), or None without nlg_eval
      session  the CaptionBeamSearch that decoded every batch (None for a stage-one model)
    float(result) is metrics["Bleu_4"] (the reference's return value), 0.0 without metrics."""

    def __init__(self, hyps, refs, hyp_ids, scores, lengths, metrics, session):
        self.hyps, self.refs, self.hyp_ids, self.scores, self.lengths = hyps, refs, hyp_ids, scores, lengths
        self.metrics, self.session = metrics, session

    def __float__(self):
        return float(self.metrics["Bleu_4"]) if self.metrics else 0.0


@torch.no_grad()
def eval_caption(model, batches, tokenizer, *, n_bm=5, n_best=1, max_len=None, session=None, output_dir=None, nlg_eval=None,
                 device="cuda", constraints=None, beam_groups=1, diversity_penalty=0.0, length_penalty=None, early_stopping=False):
    """Caption evaluation over a loader (main_task_caption.py:490-618).  batches: the reference loader's 12-tuples (:504-506);
    tokenizer: any object with vocab["[CLS]"], vocab["[SEP]"], vocab["[PAD]"] and convert_ids_to_tokens.  One CaptionBeamSearch,
    sized by the first batch (or the `session` passed in), decodes every batch; a smaller batch runs with n_active, a larger one is
    a ValueError.  max_len: positions decoded per batch (default: the model's max_words, the reference's bound).  output_dir:
    hyp.txt and ref.txt are written there as :588-597 writes them.  nlg_eval: optional metric object (NLGEval).
    constraints: a constrain.DecodeConstraints for the session this call builds; together with a `session` it is a ValueError, because
    a session owns the constraints it was built with.
    beam_groups, diversity_penalty: Diverse Beam Search for the session this call builds (decode.CaptionBeamSearch); with a `session`
    they are a ValueError for the same reason.  With G > 1 groups n_best is counted per group, hyp_ids[item] holds G * n_best
    hypotheses group-major, scores is [items, G * n_best] and lengths [items, G].  hyps / hyp.txt still get the best hypothesis of
    group 0, which no penalty reaches: at ANY penalty that is the result of a plain beam search of width n_bm / G.
    length_penalty, early_stopping: the pooled search for the session this call builds (decode.CaptionBeamSearch: a pool of finished
    hypotheses ranked by raw * len ** -alpha); with a `session` they are a ValueError for the same reason.  scores stay the RAW sums
    (not sorted then), lengths is [items, n_best], one per hypothesis, and hyps / hyp.txt get hypothesis 0, the pool's best.
    Returns a CaptionEvalResult; for a stage-one model an empty one (float() == 0.0, :495) without decoding anything."""
    from .decode import CaptionBeamSearch, check_beam_groups, check_length_penalty
    if session is not None and constraints is not None:
        raise ValueError("eval_caption: constraints= with a supplied session; the session already owns its constraints "
                         "(CaptionBeamSearch(..., constraints=))")
    if session is not None and (beam_groups != 1 or diversity_penalty != 0.0):
        raise ValueError("eval_caption: beam_groups= / diversity_penalty= with a supplied session; the session already owns them "
                         "(CaptionBeamSearch(..., beam_groups=, diversity_penalty=))")
    if session is not None and (length_penalty is not None or early_stopping not in (False, 0)):
        raise ValueError("eval_caption: length_penalty= / early_stopping= with a supplied session; the session already owns them "
                         "(CaptionBeamSearch(..., length_penalty=, early_stopping=))")
    check_beam_groups(n_bm, beam_groups, diversity_penalty)
    check_length_penalty(length_penalty, early_stopping, beam_groups)
    if model._stage_one:
        return CaptionEvalResult([], [], [], torch.zeros(0, n_best), torch.zeros(0, dtype=torch.int32), None, None)
    bos, eos, pad = tokenizer.vocab["[CLS]"], tokenizer.vocab["[SEP]"], tokenizer.vocab["[PAD]"]
    hyps, refs, hyp_ids, scores, lengths = [], [], [], [], []
    with _eval_mode(model):
        for batch in batches:
            input_ids, input_mask, segment_ids, video, video_mask = [t.to(device, non_blocking=True) for t in batch[:5]]
            so, vo = model.get_sequence_visual_output(input_ids, segment_ids, input_mask, video, video_mask)
            n = int(so.shape[0])
            if session is None:
                session = CaptionBeamSearch(model, n, so.shape[1], vo.shape[1], n_bm=n_bm, max_len=max_len, constraints=constraints,
                                            beam_groups=beam_groups, diversity_penalty=diversity_penalty,
                                            length_penalty=length_penalty, early_stopping=early_stopping)
            if n > session.n_inst:
                raise ValueError("eval_caption: a batch of %d items does not fit the decoding session's %d instances"
                                 % (n, session.n_inst))
            res = session.decode(so, vo, input_mask, video_mask, bos, eos, max_len=max_len, n_best=n_best,
                                 n_active=None if n == session.n_inst else n)
            cap, cap_len = res.captions(eos, pad)
            # the one host copy of the batch: tokens, cut lengths, scores and lengths
            cap, cap_len, sc, ln = cap.cpu().tolist(), cap_len.cpu().tolist(), res.scores.cpu(), res.lengths.cpu()
            for i in range(n):
                ids = [cap[i][k][:cap_len[i][k]] for k in range(len(cap[i]))]
                hyp_ids.append(ids)
                hyps.append(ids_to_caption(tokenizer, ids[0]))
            scores.append(sc)
            lengths.append(ln)
            truth = batch[11]
            for row in truth.reshape(-1, truth.shape[-1]).cpu().tolist():
                refs.append(ids_to_caption(tokenizer, row))
    if output_dir is not None:
        with open(os.path.join(output_dir, "hyp.txt"), "w", encoding="utf-8") as writer:
            for txt in hyps:
                writer.write(txt + "\n")
        with open(os.path.join(output_dir, "ref.txt"), "w", encoding="utf-8") as writer:
            for txt in refs:
                writer.write(txt + "\n")
    metrics = nlg_eval.compute_metrics(ref_list=[refs], hyp_list=hyps) if nlg_eval is not None else None
    scores = torch.cat(scores) if scores else torch.zeros(0, n_best)
    lengths = torch.cat(lengths) if lengths else torch.zeros(0, dtype=torch.int32)
    return CaptionEvalResult(hyps, refs, hyp_ids, scores, lengths, metrics, session)


class CaptionLossResult:
    """What eval_caption_loss returns.  Items are in loader order.
      seq_logprob [items] float32, seq_tokens [items] int32, seq_correct [items] int32   per-item host arrays (numpy)
      loss            -sum(seq_logprob) / sum(seq_tokens): CrossEntropyLoss(ignore_index=-1) over the concatenated loader (NaN when no
                      token counts, as torch's)
      perplexity      exp(loss)
      token_accuracy  sum(seq_correct) / sum(seq_tokens)
      session         the CaptionScorer that scored every batch (None for a stage-one model)
    float(result) is loss.  The sums are taken in float64 on the host."""

    def __init__(self, seq_logprob, seq_tokens, seq_correct, session):
        self.seq_logprob = np.asarray(seq_logprob, dtype=np.float32).reshape(-1)
        self.seq_tokens = np.asarray(seq_tokens, dtype=np.int32).reshape(-1)
        self.seq_correct = np.asarray(seq_correct, dtype=np.int32).reshape(-1)
        self.session = session
        n = int(self.seq_tokens.astype(np.int64).sum())
        self.loss = -float(self.seq_logprob.astype(np.float64).sum()) / n if n else float("nan")
        self.perplexity = math.exp(self.loss) if n else float("nan")
        self.token_accuracy = float(self.seq_correct.astype(np.int64).sum()) / n if n else float("nan")

    def __float__(self):
        return self.loss


@torch.no_grad()
def eval_caption_loss(model, batches, *, session=None, device="cuda"):
    """Teacher-forced caption likelihood over a loader.  batches: the reference caption loader's 12-tuples (main_task_caption.py:353-355):
    input_caption_ids, decoder_mask and output_caption_ids are elements 9, 10 and 11, labels of -1 do not count (modeling.py:253).
    One CaptionScorer, sized by the first batch (or the `session` passed in, n_cand = 1), scores every batch; a smaller batch runs
    with n_active, a larger one is a ValueError.  Each batch's three per-item results come to the host in one copy.
    Returns a CaptionLossResult; for a stage-one model an empty one (loss NaN) without a launch.
    The loss is the UNSMOOTHED likelihood whatever model.caption_label_smoothing is: the property shapes the training loss only."""
    from .score import CaptionScorer
    if model._stage_one:
        return CaptionLossResult([], [], [], None)
    packed = []
    with _eval_mode(model):
        for batch in batches:
            input_ids, input_mask, segment_ids, video, video_mask = [t.to(device, non_blocking=True) for t in batch[:5]]
            cap_in, cap_mask, cap_out = [t.to(device, non_blocking=True) for t in batch[9:12]]
            so, vo = model.get_sequence_visual_output(input_ids, segment_ids, input_mask, video, video_mask)
            n, Wd = int(so.shape[0]), int(cap_in.shape[-1])
            if session is None:
                W, F = int(so.shape[1]), int(vo.shape[1])
                session = model._eval_session(("caption_score", n, W, F, Wd), lambda: CaptionScorer(model, n, W, F, Wd))
            else:
                model._flush_pending()                   # what _eval_session does ahead of a session it owns
                model.flat.refresh_shadow()
            if n > session.n_inst:
                raise ValueError("eval_caption_loss: a batch of %d items does not fit the scoring session's %d instances"
                                 % (n, session.n_inst))
            if session.n_cand != 1:
                raise ValueError("eval_caption_loss: the session scores %d captions per item, expected 1" % session.n_cand)
            r = session.score(so, vo, input_mask, video_mask, cap_in.reshape(n, Wd), cap_mask.reshape(n, Wd), cap_out.reshape(n, Wd),
                              n_active=None if n == session.n_inst else n)
            # the one host copy of the batch: three words per item (the int32 counts travel as their bit patterns)
            packed.append(torch.stack([r.seq_logprob.reshape(-1), r.seq_tokens.reshape(-1).view(torch.float32),
                                       r.seq_correct.reshape(-1).view(torch.float32)]).cpu())
    if not packed:
        return CaptionLossResult([], [], [], session)
    host = torch.cat(packed, dim=1)
    return CaptionLossResult(host[0].numpy(), host[1].contiguous().view(torch.int32).numpy(), host[2].contiguous().view(torch.int32).numpy(),
                             session)
