"""Teacher-forced caption scoring: score.CaptionScorer against the path that gives the same answer without it --
decoder_caption(get_logits=True) + torch.log_softmax + gather + sum.  cfg4 model shape (max_words 128, max_frames 96, 2 cross + 3
decoder layers), bf16, 16 videos x 1 and x 5 candidate captions of Wd = 48 positions.

    python scripts/mb_vocab_score.py [--cands 1,5] [--rounds 7] [--out profiles/caption_scoring.txt]

Timing: both sides are warmed up (plans built, the scorer's graph captured), then timed with HIP events in alternating rounds inside
this one process (new, old, new, old, ...); the table shows the median round and the spread.  A round is as many back-to-back calls
as fill ~100 ms (at most 50).  Bytes allocated per caption: the growth of torch.cuda.memory_allocated() over building each side's
session and making its first call, divided by the number of captions (the features and captions are allocated before the baseline).
No ratio is fixed in advance: the file records what was measured."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from univl_amd import UniVL  # noqa: E402
from univl_amd.score import CaptionScorer  # noqa: E402

DEV = "cuda"
N, W, F, WD = 16, 128, 96, 48


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cands", default="1,5")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="profiles/caption_scoring.txt")
    a = ap.parse_args()
    tc = argparse.Namespace(max_words=W, max_frames=F, video_dim=1024, batch_size=N, n_gpu=1, n_pair=1, margin=0.1,
                            negative_weighting=1, hard_negative_rate=0.5, use_mil=False, do_pretrain=False, task_type="caption",
                            stage_two=True, text_num_hidden_layers=12, visual_num_hidden_layers=6, cross_num_hidden_layers=2,
                            decoder_num_hidden_layers=3, local_rank=0, dropout_prob=0.1, compute_dtype="bf16", seed=1)
    torch.manual_seed(0)
    model = UniVL.from_pretrained("bert-base-uncased", "visual-base", "cross-base", "decoder-base", task_config=tc).to(DEV).eval()
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1000, 30000, (N, W), generator=g).to(DEV)
    am = torch.ones(N, W, dtype=torch.int64, device=DEV)
    vm = torch.ones(N, F, dtype=torch.int64, device=DEV)
    video = torch.randn(N, F, 1024, generator=g, dtype=torch.float64).to(DEV)
    lines = ["caption scoring, %d videos, Wd = %d, cfg4 model shape, bf16, %s" % (N, WD, torch.cuda.get_device_name(0)),
             "new = CaptionScorer.score (one hipGraph; cross encoder once per video; univl_vocab_score, no logits)",
             "old = decoder_caption(get_logits=True) + torch.log_softmax + gather + sum (cross encoder once per caption; [captions, Wd, V] fp32 logits)",
             "median of %d alternating rounds (min .. max); bytes = growth of memory_allocated over building the side and its first call" % a.rounds,
             "%6s %9s %22s %22s %8s %16s %16s %14s" % ("cands", "captions", "new ms", "old ms", "old/new", "new B/caption", "old B/caption", "max |diff|")]
    with torch.no_grad():
        so, vo = model.get_sequence_visual_output(ids, torch.zeros_like(ids), am, video, vm)
        for nc in [int(x) for x in a.cands.split(",")]:
            B = N * nc
            cap_in = torch.randint(1000, 30000, (N, nc, WD), generator=g).to(DEV)
            lens = torch.randint(8, WD + 1, (N, nc, 1), generator=g).to(DEV)
            mask = (torch.arange(WD, device=DEV) < lens).to(torch.int64)
            labels = torch.where(mask > 0, torch.randint(1000, 30000, (N, nc, WD), generator=g).to(DEV), torch.full_like(mask, -1))
            rep = lambda t: t.repeat_interleave(nc, dim=0)
            so_r, vo_r, am_r, vm_r = rep(so), rep(vo), rep(am), rep(vm)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            scorer = CaptionScorer(model, N, W, F, WD, n_cand=nc)
            new_res = scorer.score(so, vo, am, vm, cap_in, mask, labels)
            torch.cuda.synchronize()
            new_bytes = (torch.cuda.memory_allocated() - base - sum(t.numel() * t.element_size() for t in vars(new_res).values())) / B
            new = lambda: scorer.score(so, vo, am, vm, cap_in, mask, labels)

            def old():
                lg = model.decoder_caption(so_r, vo_r, None, am_r, vm_r, cap_in.view(B, WD), mask.view(B, WD), shaped=True, get_logits=True)
                lp = torch.log_softmax(lg, dim=-1)
                tl = lp.gather(-1, labels.view(B, WD).clamp(min=0)[..., None])[..., 0] * (labels.view(B, WD) >= 0)
                return tl, tl.sum(-1)
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            old_tl, old_sum = old()
            torch.cuda.synchronize()
            old_bytes = (torch.cuda.max_memory_allocated() - base) / B     # the session's buffers + the call's peak (logits, log-softmax)
            diff = float((new_res.token_logprob.view(B, WD) - old_tl).abs().max())
            n_calls, ms = {}, {"new": [], "old": []}
            for name, fn in (("new", new), ("old", old)):
                fn()
                n_calls[name] = max(1, min(50, int(100.0 / max(timed(fn, 2), 1e-3))))
            for _ in range(a.rounds):
                for name, fn in (("new", new), ("old", old)):
                    ms[name].append(timed(fn, n_calls[name]))
            med = {k: statistics.median(v) for k, v in ms.items()}
            fmt = lambda k: "%8.3f (%.3f .. %.3f)" % (med[k], min(ms[k]), max(ms[k]))
            lines.append("%6d %9d %22s %22s %8.2f %16.0f %16.0f %14.3e" % (nc, B, fmt("new"), fmt("old"), med["old"] / med["new"], new_bytes,
                                                                            old_bytes, diff))
            del scorer, new_res, old_tl, old_sum
            model._steps.clear()
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
