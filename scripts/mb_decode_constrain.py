"""Micro-benchmark of the decoding constraints (univl_amd/csrc/constrain.hip: univl_decode_constrain; univl_amd/constrain.py) at the
shape `bench.py --measure decode` times: 16 instances x 5 beams x 32 positions, bf16, cfg4 (128 words, 96 frames, 2 cross + 3 decoder
layers), eos = -1 so that every instance runs all 32 positions.

    python scripts/mb_decode_constrain.py [--rounds 3] [--reps 3] [--out profiles/decode_constraints.txt]

Two sessions on one model in this one process: constraints=None (the plans of the parent commit, launch for launch) and
DecodeConstraints(3, 5, <the special ids>): [PAD] [UNK] [CLS] [SEP] [MASK] and the [unusedNN] rows of the BERT table, 999 ids.  Both are
warmed up (graph capture), then decode() is timed in alternating rounds (none, constrained, none, ...) with a host clock around `reps`
calls that end in a device synchronise; the table shows every round and the median.  The kernel's own time is a HIP-event loop over
back-to-back eager launches at the same shape (80 rows, position 16), which is an upper bound on what it adds inside a replayed graph."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from univl_amd import UniVL, ops  # noqa: E402
from univl_amd.constrain import DecodeConstraints  # noqa: E402
from univl_amd.decode import CaptionBeamSearch  # noqa: E402

DEV = "cuda"
N, NB, W, F, T = 16, 5, 128, 96, 32
SPECIAL = tuple(range(0, 999))           # [PAD], [unused0..98], [UNK], [CLS], [SEP], [MASK], [unused99..993]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="profiles/decode_constraints.txt")
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
    sessions = [("constraints=None", CaptionBeamSearch(model, N, W, F, n_bm=NB, max_len=T)),
                ("DecodeConstraints(3, 5, %d ids)" % len(SPECIAL),
                 CaptionBeamSearch(model, N, W, F, n_bm=NB, max_len=T, constraints=DecodeConstraints(3, 5, SPECIAL)))]

    def run(bs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            bs.decode(so, vo, am, vm, bos=101, eos=-1, sync_every=0)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.reps / T * 1e3

    for _, bs in sessions:                       # graph capture, then one replayed call
        bs.decode(so, vo, am, vm, bos=101, eos=-1, sync_every=0)
        bs.decode(so, vo, am, vm, bos=101, eos=-1, sync_every=0)
    ms = {name: [] for name, _ in sessions}
    for _ in range(a.rounds):
        for name, bs in sessions:
            ms[name].append(run(bs))
    launches = [len(bs.steps[(T - 1, True)]) for _, bs in sessions]
    # the kernel alone: eager launches back to back at the decode shape
    R, V = N * NB, sessions[1][1].V
    x = torch.randn(R, (V + 7) // 8 * 8, device=DEV)
    pre = [torch.randint(1000, V, (R, T), dtype=torch.int32, device=DEV) for _ in range(2)]
    src = torch.arange(R, dtype=torch.int32, device=DEV)
    last = torch.randint(1000, V, (R,), dtype=torch.int64, device=DEV)
    done = torch.zeros(N, dtype=torch.uint8, device=DEV)
    c = sessions[1][1].constraints
    call = lambda: ops.decode_constrain(x, V, 16, prefix_in=pre[0], prefix_out=pre[1], src=src, last=last, done=done, done_stride=NB,
                                        params_dev=c.params_dev, suppress=c.suppress_dev)
    for _ in range(20):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kern = []
    for _ in range(a.rounds):
        e0.record()
        for _ in range(200):
            call()
        e1.record()
        e1.synchronize()
        kern.append(e0.elapsed_time(e1) / 200 * 1e3)
    med = {name: statistics.median(v) for name, v in ms.items()}
    names = [name for name, _ in sessions]
    lines = ["decoding constraints, %d x %d beams x %d positions, bf16, %s" % (N, NB, T, torch.cuda.get_device_name(0)),
             "ms per position of decode() (host clock around %d calls, device synchronise at the end), alternating rounds" % a.reps]
    for name, n in zip(names, launches):
        lines.append("%-34s plan entries %3d   rounds %s   median %.4f" % (name, n, " ".join("%.4f" % t for t in ms[name]), med[name]))
    lines.append("difference of the medians: %.1f us per position; spread of the unconstrained rounds: %.1f us"
                 % ((med[names[1]] - med[names[0]]) * 1e3, (max(ms[names[0]]) - min(ms[names[0]])) * 1e3))
    lines.append("univl_decode_constrain alone (80 rows, position 16, order 3, %d suppressed ids; 200 eager launches back to back per round, "
                 "HIP events): %s us per launch" % (len(SPECIAL), " ".join("%.2f" % t for t in kern)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
