"""Micro-benchmark of the pooled beam search (univl_amd/csrc/beam.hip: univl_beam_pool_step; decode.CaptionBeamSearch(length_penalty=)) at
the shape of profiles/decode_constraints.txt and `bench.py --measure decode`: 16 instances x 5 beams x 32 positions, bf16, cfg4 (128
words, 96 frames, 2 cross + 3 decoder layers), run to max_len (sync_every=0).

    python scripts/mb_pool_beam.py [--rounds 5] [--reps 3] [--out profiles/pool_beam.txt]

Two sessions on one model in this one process: length_penalty=None (univl_beam_step as the tail of a position) and length_penalty=1.0
(univl_beam_pool_step in its place, the same launch count, and univl_beam_pool_finish for the walk-back).  The end token is "[SEP]"
(102) for both; the table says how many positions the instances of either ran before they were done (a done instance is frozen: its
rows are not scanned) and how many hypotheses finished -- with random weights none may, and the figure is then that of live positions.  Both are warmed up (graph capture), then decode() is timed in
alternating rounds with a host clock around `reps` calls that end in a device synchronise, the method of
profiles/beam_step_bench_decode.txt; the table shows every round, the median and the run-to-run spread.  The two beam steps' own time
is a HIP-event loop over back-to-back eager calls (both launches) at the same shape, position 16, no instance done."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from univl_amd import UniVL, ops  # noqa: E402
from univl_amd.decode import CaptionBeamSearch  # noqa: E402

DEV = "cuda"
N, NB, W, F, T = 16, 5, 128, 96, 32
ALPHA, BOS, EOS = 1.0, 101, 102


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="profiles/pool_beam.txt")
    a = ap.parse_args()
    tc = argparse.Namespace(max_words=W, max_frames=F, video_dim=1024, batch_size=N, n_gpu=1, n_pair=1, margin=0.1, negative_weighting=1,
                            hard_negative_rate=0.5, use_mil=False, do_pretrain=False, task_type="caption", stage_two=True,
                            train_sim_after_cross=False, text_num_hidden_layers=12, visual_num_hidden_layers=6, cross_num_hidden_layers=2,
                            decoder_num_hidden_layers=3, local_rank=0, dropout_prob=0.0, compute_dtype="bf16", seed=42)
    torch.manual_seed(0)
    model = UniVL.from_pretrained("bert-base-uncased", "visual-base", "cross-base", "decoder-base", task_config=tc).to(DEV).eval()
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1000, 30522, (N, 1, W), generator=g)
    ids[..., 0] = 101
    b = [t.to(DEV) for t in (ids, torch.zeros(N, 1, W, dtype=torch.int64), torch.ones(N, 1, W, dtype=torch.int64),
                             torch.randn(N, 1, F, 1024, generator=g, dtype=torch.float64), torch.ones(N, 1, F, dtype=torch.int64))]
    with torch.no_grad():
        so, vo = model.get_sequence_visual_output(*b)
    am, vm = b[2].view(N, -1), b[4].view(N, -1)
    sessions = [("length_penalty=None", CaptionBeamSearch(model, N, W, F, n_bm=NB, max_len=T)),
                ("length_penalty=%g" % ALPHA, CaptionBeamSearch(model, N, W, F, n_bm=NB, max_len=T, length_penalty=ALPHA))]

    def decode(bs):
        return bs.decode(so, vo, am, vm, bos=BOS, eos=EOS, sync_every=0)

    def run(bs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            decode(bs)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.reps / T * 1e3

    for _, bs in sessions:                       # graph capture, then one replayed call
        decode(bs)
        decode(bs)
    ms = {name: [] for name, _ in sessions}
    for _ in range(a.rounds):
        for name, bs in sessions:
            ms[name].append(run(bs))
    launches = [len(bs.steps[(T - 1, True)]) for _, bs in sessions]
    plain, pooled = decode(sessions[0][1]), decode(sessions[1][1])
    ran = [plain.lengths.float().mean().item(), pooled.positions.float().mean().item()]
    # the two beam steps alone: eager calls back to back at the decode shape (80 rows, position 16)
    R, V = N * NB, sessions[0][1].V
    ld = (V + 7) // 8 * 8
    x = torch.log_softmax(torch.randn(R, ld, device=DEV), dim=1)

    def state():
        return dict(scores=-torch.rand(N, NB, device=DEV), done=torch.zeros(N, dtype=torch.uint8, device=DEV),
                    length=torch.zeros(N, dtype=torch.int32, device=DEV), tokens=torch.zeros(R, dtype=torch.int64, device=DEV),
                    src=torch.zeros(R, dtype=torch.int32, device=DEV), hist_parents=torch.zeros(T, N, NB, dtype=torch.int32, device=DEV),
                    hist_tokens=torch.zeros(T, N, NB, dtype=torch.int32, device=DEV), hist_scores=torch.zeros(T, N, NB, device=DEV),
                    ws=ops.beam_ws(N, NB, DEV))
    s1, s2 = state(), state()
    s2.update(ops.beam_pool(N, NB, DEV), w=ops.length_weights(ALPHA, T).to(DEV),
              params=torch.tensor([0, T], dtype=torch.int32, device=DEV))

    def pool_call():                             # an empty pool every call: `done` is never set, every call does a live position's work
        ops.beam_pool_step(x, V, N, NB, 16, eos=EOS, **s2)
    calls = [lambda: ops.beam_step(x, V, N, NB, 16, **s1), pool_call]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kern = [[], []]
    for call in calls:
        for _ in range(20):
            call()
    for _ in range(a.rounds):
        for k, call in enumerate(calls):
            s2["pool_count"].zero_()
            e0.record()
            for _ in range(200):
                call()
            e1.record()
            e1.synchronize()
            kern[k].append(e0.elapsed_time(e1) / 200 * 1e3)
    frozen = int(s2["done"].sum())
    lines = ["python scripts/mb_pool_beam.py (16 instances x %d beams, 32 positions, 128 x 96, 3 decoder layers, bf16, eos = %d, sync_every=0),"
             % (NB, EOS),
             "one MI355X, one process, two sessions on one model, alternating rounds of %d decode() calls each; ms per position, host clock."
             % a.reps]
    for (name, _), n, r in zip(sessions, launches, ran):
        v = ms[name]
        lines.append("%-22s %s  median %.4f  spread %.4f  (%d launches per position; instances ran %.1f of %d positions on average)"
                     % (name, " / ".join("%.4f" % x_ for x_ in v), statistics.median(v), max(v) - min(v), n, r, T))
    d = statistics.median(ms[sessions[1][0]]) - statistics.median(ms[sessions[0][0]])
    lines.append("difference of the medians: %+.1f us per position (the pooled decode() also ends in univl_beam_pool_finish where the plain one"
                 % (d * 1e3))
    lines.append("ends in univl_beam_backtrack: one launch per call either way)")
    for name, v in zip(("univl_beam_step", "univl_beam_pool_step"), kern):
        lines.append("%-24s both launches, eager, back to back: %s us  median %.1f"
                     % (name, " / ".join("%.1f" % x_ for x_ in v), statistics.median(v)))
    lines.append("instances the eager loop of univl_beam_pool_step left done (frozen, cheaper calls): %d of %d" % (frozen, N))
    lines.append("finished hypotheses among the %d x %d returned by the pooled session at n_best = 1: %d"
                 % (N, 1, int(pooled.finished.sum())))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
