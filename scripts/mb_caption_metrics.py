"""Micro-benchmark of the caption metrics (univl_amd/csrc/metric.hip: univl_caption_overlap, univl_consensus_pick;
univl_amd/caption_metrics.py: CaptionMetrics, consensus).

    python scripts/mb_caption_metrics.py [--rounds 3] [--out profiles/caption_metrics.txt]

1. Corpus size: 3000 items x 20 references x 48 tokens (random words of a 2000-word vocabulary, Zipf-like, lengths 8 .. 48).  Timed in
   alternating rounds (kernel, compute_ids, restatement, kernel, ...):
     kernel        the one launch with the tables already on the device, HIP events around back-to-back calls;
     compute_ids   the whole call: packing, document frequency with numpy on the host, uploads, the launch, the copies back and the
                   corpus arithmetic (wall clock);
     restatement   the dictionary restatement of tests/test_caption_metrics_cpu.py on all 3000 items, its document frequencies
                   included (plain Python; wall clock; about ten seconds a round).
2. Consensus size: 16 videos x 5 samples x 32 positions: one call of the overlap launch + univl_consensus_pick on device rows, as the
   time that elapses per call between two HIP events around 50 back-to-back calls -- output allocation and enqueue cost included, NOT a
   kernel time -- against the restatement of the same 80 items (wall clock)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from univl_amd import ops  # noqa: E402
from univl_amd import caption_metrics as M  # noqa: E402
from test_caption_metrics_cpu import item_stats, restate  # noqa: E402  (the restatement lives with the tests that define it)

DEV = "cuda"
ITEMS, REFS, TOKENS, VOCAB = 3000, 20, 48, 2000


def events(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n                 # milliseconds per call


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def corpus(rounds, lines):
    rng = np.random.RandomState(0)
    word = lambda n: np.minimum((rng.pareto(1.1, size=n) * 4).astype(np.int64), VOCAB - 1).tolist()
    hyps = [word(rng.randint(8, TOKENS + 1)) for _ in range(ITEMS)]
    refs = [[word(rng.randint(8, TOKENS + 1)) for _ in range(REFS)] for _ in range(ITEMS)]
    cm = M.CaptionMetrics(DEV)
    # the kernel alone: what compute_ids uploads, kept on the device
    rows = hyps + [r for rr in refs for r in rr]
    sym, lens = M._pack(rows)
    ref_begin = (np.arange(ITEMS + 1) * REFS).astype(np.int32)
    ref_rows = np.arange(ITEMS, ITEMS + ITEMS * REFS, dtype=np.int32)
    keys, cnts, begin = M.document_frequency(sym, lens, ref_begin, ref_rows)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    d = [up(sym), up(lens), up(np.arange(ITEMS, dtype=np.int32)), up(ref_begin), up(ref_rows)]
    tables = (up(keys.view(np.int64)), up(cnts), begin, ITEMS)
    kernel = lambda: ops.caption_overlap(*d, ITEMS * REFS, tables=tables)
    plain = lambda: ops.caption_overlap(*d, ITEMS * REFS)
    restatement = lambda: restate(hyps, refs)
    runs = {"kernel (with CIDEr)": lambda: events(kernel, 5), "kernel (no tables)": lambda: events(plain, 5),
            "compute_ids": lambda: wall(lambda: cm.compute_ids(hyps, refs)), "restatement": lambda: wall(restatement)}
    kernel(), plain(), cm.compute_ids(hyps[:64], refs[:64])
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            times[name].append(fn())
    lines.append("corpus: %d items x %d references x 8 .. %d tokens, %d table entries; milliseconds, alternating rounds"
                 % (ITEMS, REFS, TOKENS, begin[4]))
    lines.append("%24s %s %12s" % ("", " ".join("%10s" % ("round %d" % (i + 1)) for i in range(rounds)), "median ms"))
    for name, ts in times.items():
        lines.append("%24s %s %12.3f" % (name, " ".join("%10.3f" % t for t in ts), statistics.median(ts)))
    t0 = time.perf_counter()
    M.document_frequency(sym, lens, ref_begin, ref_rows)
    lines.append("of compute_ids, the host's document frequency alone (one call): %.1f ms" % ((time.perf_counter() - t0) * 1e3))


def consensus_size(rounds, lines):
    n, ns, T = 16, 5, 32
    rng = np.random.RandomState(1)
    cap = rng.randint(0, 40, size=(n, ns, T)).astype(np.int32)
    cap_len = rng.randint(4, T + 1, size=(n, ns)).astype(np.int32)
    d_cap, d_len = torch.from_numpy(cap).to(DEV), torch.from_numpy(cap_len).to(DEV)
    hyp_row, ref_begin, ref_rows = M._consensus_layout(n, ns, torch.device(DEV, 0))

    def device():
        o = ops.caption_overlap(d_cap.view(n * ns, T), d_len.view(-1), hyp_row, ref_begin, ref_rows, n * ns * (ns - 1))
        return ops.consensus_pick(o["rouge_l"].view(n, ns))

    def host():
        for i in range(n):
            cut = [cap[i, s, :cap_len[i, s]].tolist() for s in range(ns)]
            [item_stats(c, [o for j, o in enumerate(cut) if j != s])["rouge_l"] for s, c in enumerate(cut)]
    runs = {"overlap + pick, per call": lambda: events(device, 50), "restatement (host)": lambda: wall(host)}
    device()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            times[name].append(fn())
    lines.append("")
    lines.append("consensus: %d videos x %d samples x up to %d positions (%d items x %d references); milliseconds (per call between events: allocation and enqueue included), alternating rounds"
                 % (n, ns, T, n * ns, ns - 1))
    lines.append("%24s %s %12s" % ("", " ".join("%10s" % ("round %d" % (i + 1)) for i in range(rounds)), "median ms"))
    for name, ts in times.items():
        lines.append("%24s %s %12.4f" % (name, " ".join("%10.4f" % t for t in ts), statistics.median(ts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/caption_metrics.txt")
    a = ap.parse_args()
    lines = ["caption metrics on %s" % torch.cuda.get_device_name(0)]
    corpus(a.rounds, lines)
    consensus_size(a.rounds, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
