"""Micro-benchmark of caption sampling (univl_amd/csrc/sample.hip: univl_sample_step; univl_amd/sample.py: CaptionSampler).

    python scripts/mb_sample_step.py [--rounds 3] [--out profiles/caption_sampling.txt]

1. The kernel alone at R = 80 rows, V = 30522 (row stride 30528), k in {1, 50, 64}: both launches of one position, HIP events around
   back-to-back calls, median of the rounds.  Beside it the tail it replaces in a position of decode(): univl_log_softmax_rows
   followed by univl_beam_step (16 x 5) on the same buffer.
2. sample() at 16 instances x 5 samples x 32 positions in bf16 (the shape of `bench.py --measure decode`) against decode() at 16 x 5
   beams x 32 positions, both sessions built on ONE model in this process and timed in alternating rounds (sample, decode, sample,
   ...), eos = -1 so that every row runs all 32 positions -- the form of profiles/beam_step_bench_decode.txt."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import univl_oracle as O  # noqa: E402
from univl_amd import UniVL, ops  # noqa: E402
from univl_amd.decode import CaptionBeamSearch  # noqa: E402
from univl_amd.sample import CaptionSampler  # noqa: E402

DEV = "cuda"
V, LD, R, TMAX = 30522, 30528, 80, 32


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n * 1e3          # microseconds per call


def kernel_alone(rounds, lines):
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(R, LD, device=DEV, generator=g) * 3.0
    lines.append("kernel alone: R = %d, V = %d, ld = %d, fp32 logits ~ N(0, 3), T = 0.9, top_p = 0.95; microseconds per position" % (R, V, LD))
    lines.append("%28s %10s" % ("launches", "us"))
    for k in (1, 50, 64):
        st = dict(done=torch.zeros(R, dtype=torch.uint8, device=DEV), length=torch.zeros(R, dtype=torch.int32, device=DEV),
                  ids=torch.zeros(R, dtype=torch.int64, device=DEV), tokens_out=torch.zeros(R, TMAX, dtype=torch.int32, device=DEV),
                  tok_logprob=torch.zeros(R, TMAX, device=DEV), q_logprob=torch.zeros(R, TMAX, device=DEV),
                  seq_logprob=torch.zeros(R, device=DEV), seq_q_logprob=torch.zeros(R, device=DEV), ws=ops.sample_ws(R, k, DEV))
        fn = lambda: ops.sample_step(x, V, k, 3, inv_T=1.0 / 0.9, top_p=0.95, seed=1, **st)
        timed(fn, 20)
        lines.append("%28s %10.1f" % ("univl_sample_step k=%d" % k, statistics.median(timed(fn, 200) for _ in range(rounds))))
    n, nb = 16, 5
    lp = x.clone()
    bst = dict(scores=torch.zeros(n, nb, device=DEV), done=torch.zeros(n, dtype=torch.uint8, device=DEV),
               length=torch.zeros(n, dtype=torch.int32, device=DEV), tokens=torch.zeros(R, dtype=torch.int64, device=DEV),
               src=torch.zeros(R, dtype=torch.int32, device=DEV), hist_parents=torch.zeros(TMAX, n, nb, dtype=torch.int32, device=DEV),
               hist_tokens=torch.zeros(TMAX, n, nb, dtype=torch.int32, device=DEV), hist_scores=torch.zeros(TMAX, n, nb, device=DEV),
               ws=ops.beam_ws(n, nb, DEV))
    for name, fn in (("univl_log_softmax_rows", lambda: ops.log_softmax_rows(lp, V)),
                     ("univl_beam_step 16 x 5", lambda: ops.beam_step(lp, V, n, nb, 3, **bst)),
                     ("both (decode()'s tail)", lambda: (ops.log_softmax_rows(lp, V), ops.beam_step(lp, V, n, nb, 3, **bst)))):
        timed(fn, 20)
        lines.append("%28s %10.1f" % (name, statistics.median(timed(fn, 200) for _ in range(rounds))))


def whole_runs(rounds, lines):
    cfg = O.OracleConfig(batch_size=4, stage_two=True, task_type="caption", max_words=128, max_frames=96)
    ns = argparse.Namespace(**cfg.to_dict(), local_rank=0, compute_dtype="bf16")
    model = UniVL.from_pretrained("bert-base-uncased", "visual-base", "cross-base", "decoder-base", task_config=ns)
    model.to(DEV).eval()
    n, nb, T, W, F = 16, 5, 32, cfg.max_words, cfg.max_frames
    g = torch.Generator(device="cpu").manual_seed(99)
    ids = torch.randint(1000, V, (n, 1, W), generator=g)
    ids[..., 0] = 101
    b = [t.to(DEV) for t in (ids, torch.zeros(n, 1, W, dtype=torch.int64), torch.ones(n, 1, W, dtype=torch.int64),
                             torch.randn(n, 1, F, 1024, generator=g, dtype=torch.float64), torch.ones(n, 1, F, dtype=torch.int64))]
    with torch.no_grad():
        so, vo = model.get_sequence_visual_output(*b)
    enc = (so, vo, b[2].view(n, -1), b[4].view(n, -1))
    smp = CaptionSampler(model, n, W, F, n_samp=nb, max_len=T, top_k=50, temperature=0.9, top_p=0.95)
    bsr = CaptionBeamSearch(model, n, W, F, n_bm=nb, max_len=T)
    runs = {"sample()": lambda: smp.sample(*enc, bos=101, eos=-1, seed=1), "decode()": lambda: bsr.decode(*enc, bos=101, eos=-1)}
    for fn in runs.values():          # plans and graph captures
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / 3)
    lines.append("")
    lines.append("whole runs: %d instances x %d rows x %d positions, bf16, top_k = 50, T = 0.9, top_p = 0.95, eos = -1; one model, alternating rounds" % (n, nb, T))
    lines.append("%10s %s %12s %14s" % ("", " ".join("%9s" % ("round %d" % (i + 1)) for i in range(rounds)), "median ms", "ms / position"))
    for name, ts in times.items():
        med = statistics.median(ts)
        lines.append("%10s %s %12.3f %14.4f" % (name, " ".join("%9.3f" % (t * 1e3) for t in ts), med * 1e3, med * 1e3 / T))
    lines.append("sample() / decode() per position: %.3f" % (statistics.median(times["sample()"]) / statistics.median(times["decode()"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/caption_sampling.txt")
    a = ap.parse_args()
    lines = ["caption sampling on %s" % torch.cuda.get_device_name(0)]
    kernel_alone(a.rounds, lines)
    whole_runs(a.rounds, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
