"""Micro-benchmark of the retrieval search (univl_amd/csrc/retrieve.hip: univl_sim_topk) against what the library had before it: the
dense product into an [Nq, Ng] fp32 matrix (ops.gemm) followed by torch.topk (plus univl_rank_counts where Nq == Ng, the only shape
it takes).  Cells: Nq in {1, 64, 1024} x Ng in {1e4, 1e5, 1e6}, k = 10.

    python scripts/mb_sim_topk.py [--nq 1,64,1024] [--ng 10000,100000,1000000] [--out profiles/retrieval_search.txt]

Timing: both sides are warmed up, then timed with HIP events in alternating rounds inside this one process (new, old, new, old, ...);
the table shows the median round.  A round is as many back-to-back calls as fill ~50 ms (at most 50).  Galleries below 600 MB are
allocated several times and the calls rotate through the copies, so that a call does not find its gallery in the 256 MB Infinity
Cache left there by the call before.  The roofline column is the new call's algorithmic gallery bytes (Ng * 3072) per second against
the 6.3 TB/s a streaming kernel reaches on this part (8 TB/s is the data sheet's number)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from univl_amd import ops  # noqa: E402

DEV = "cuda"
H, K = 768, 10
HBM_TBS = 6.3
MATRIX_LIMIT = 16 * 2 ** 30          # a comparand whose score matrix is larger than this is skipped, and the table says so


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", default="1,64,1024")
    ap.add_argument("--ng", default="10000,100000,1000000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/retrieval_search.txt")
    a = ap.parse_args()
    lines = ["retrieval search, k = %d, fp32, %s" % (K, torch.cuda.get_device_name(0)),
             "new = univl_sim_topk (scan + merge); old = ops.gemm into [Nq, Ng] fp32 + torch.topk; median of alternating rounds",
             "%6s %9s %7s %12s %12s %9s %10s %9s" % ("Nq", "Ng", "copies", "new ms", "old ms", "old/new", "new GB/s", "roofline")]
    gen = torch.Generator(device=DEV).manual_seed(0)
    for Ng in [int(x) for x in a.ng.split(",")]:
        copies = max(1, min(20, -(-600 * 2 ** 20 // (Ng * H * 4))))
        gs = [torch.nn.functional.normalize(torch.randn(Ng, H, device=DEV, generator=gen), dim=-1) for _ in range(copies)]
        for Nq in [int(x) for x in a.nq.split(",")]:
            # rows padded to a multiple of 4, as get_similarity_logits allocates the operands of the same ops.gemm call
            qp = torch.zeros((Nq + 3) // 4 * 4, H, device=DEV)
            qp[:Nq] = torch.nn.functional.normalize(torch.randn(Nq, H, device=DEV, generator=gen), dim=-1)
            q = qp[:Nq]
            new = lambda i: ops.sim_topk(q, gs[i % copies], K)
            old = None
            if Nq * Ng * 4 <= MATRIX_LIMIT:
                sim = torch.empty(Nq, Ng, device=DEV)

                def old(i):
                    ops.gemm(q, gs[i % copies], Nq, Ng, H, out32=sim)
                    out = torch.topk(sim, K, dim=1)
                    if Nq == Ng:
                        ops.rank_counts(sim)
                    return out
            sides = [("new", new)] + ([("old", old)] if old else [])
            n_calls, ms = {}, {}
            for name, fn in sides:                      # warm-up: twice, the second one timed to size the rounds
                timed(fn, 1)
                t = timed(fn, 1)
                n_calls[name] = max(1, min(50, int(50.0 / max(t, 1e-3))))
                ms[name] = []
            rounds = a.rounds if max(n_calls.values()) > 1 else min(a.rounds, 2)      # multi-second cells: two rounds
            for r in range(rounds):
                for name, fn in sides:
                    ms[name].append(timed(fn, n_calls[name]))
            t_new = statistics.median(ms["new"])
            gbs = Ng * H * 4 / (t_new * 1e-3) / 1e9
            if old:
                t_old = statistics.median(ms["old"])
                lines.append("%6d %9d %7d %12.4f %12.4f %9.2f %10.0f %8.1f%%" % (Nq, Ng, copies, t_new, t_old, t_old / t_new, gbs,
                                                                               100 * gbs / (HBM_TBS * 1e3)))
            else:
                lines.append("%6d %9d %7d %12.4f %12s %9s %10.0f %8.1f%%   (old skipped: a %.1f GB matrix)"
                             % (Nq, Ng, copies, t_new, "-", "-", gbs, 100 * gbs / (HBM_TBS * 1e3), Nq * Ng * 4 / 2 ** 30))
            lines.append("        rounds new: %s%s" % (" ".join("%.4f" % t for t in ms["new"]),
                                                      ("   old: " + " ".join("%.4f" % t for t in ms["old"])) if old else ""))
            print("\n".join(lines[-2:]), flush=True)
            del q, qp
            if old:
                del sim
        del gs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:3]))


if __name__ == "__main__":
    main()
