"""Micro-benchmark of query-bank normalised search (univl_amd/csrc/retrieve.hip: univl_sim_colstat, univl_sim_topk_norm).

    python scripts/mb_qbnorm.py [--out profiles/qbnorm.txt]

Cells:
  column term        univl_sim_colstat at (Nb, Ng) = (1 000, 1 000) and (10 000, 10 000) against the dense way: ops.gemm into the
                     [Nb, Ng] fp32 matrix, then torch.logsumexp over the bank (scaled by beta before, divided after);
  normalised search  static (one normalised scan) and dynamic (plain top-1, gate, normalised scan) against the plain ops.sim_topk,
                     Nq in {16, 64} x Ng in {10 000, 100 000}, k = 10, a 1 000-row bank fitted beforehand (not timed);
  accuracy           max |c - c64| over the grid of tests/test_qbnorm_gpu.py (random unit vectors, beta in {1, 20, 100}).

Timing as scripts/mb_sim_topk.py: both sides warmed up, HIP events, alternating rounds in this one process, the median round; a round
is as many back-to-back calls as fill ~50 ms (at most 50); galleries rotate through copies so that a call does not find its gallery
in the Infinity Cache.  A losing cell is reported as it is."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from univl_amd import ops  # noqa: E402

DEV = "cuda"
H, K, BETA = 768, 10, 20.0


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def race(sides, rounds):
    """sides: [(name, fn)].  {name: (median ms, [round ms])}, the sides timed in alternating rounds."""
    n_calls, ms = {}, {}
    for name, fn in sides:
        timed(fn, 1)
        n_calls[name] = max(1, min(50, int(50.0 / max(timed(fn, 1), 1e-3))))
        ms[name] = []
    for r in range(rounds):
        for name, fn in sides:
            ms[name].append(timed(fn, n_calls[name]))
    return {name: (statistics.median(v), v) for name, v in ms.items()}


def unit(n, gen):
    return torch.nn.functional.normalize(torch.randn(n, H, device=DEV, generator=gen), dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/qbnorm.txt")
    a = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    lines = ["query-bank normalised search, fp32, beta = %g, %s; median of %d alternating rounds" % (BETA, torch.cuda.get_device_name(0), a.rounds),
             "", "column term: new = univl_sim_colstat (scan + merge); old = ops.gemm into [Nb, Ng] fp32 + torch.logsumexp",
             "%7s %7s %7s %10s %10s %9s" % ("Nb", "Ng", "copies", "new ms", "old ms", "old/new")]
    for Nb, Ng in ((1000, 1000), (10000, 10000)):
        copies = max(1, min(20, -(-600 * 2 ** 20 // (Ng * H * 4))))
        gs = [unit(Ng, gen) for _ in range(copies)]
        bank, sim, c = unit(Nb, gen), torch.empty(Nb, Ng, device=DEV), torch.empty(Ng, device=DEV)

        def old(i):
            ops.gemm(bank, gs[i % copies], Nb, Ng, H, out32=sim)
            return torch.logsumexp(sim.mul_(BETA), dim=0).div_(BETA)
        res = race([("new", lambda i: ops.sim_colstat(bank, gs[i % copies], BETA, out=c)), ("old", old)], a.rounds)
        lines.append("%7d %7d %7d %10.4f %10.4f %9.2f" % (Nb, Ng, copies, res["new"][0], res["old"][0], res["old"][0] / res["new"][0]))
        lines.append("        rounds new: %s   old: %s" % (" ".join("%.4f" % t for t in res["new"][1]), " ".join("%.4f" % t for t in res["old"][1])))
        err = float((ops.sim_colstat(bank, gs[0], BETA) - old(0)).abs().max())
        lines.append("        max |new - old| = %.3e" % err)
        print("\n".join(lines[-3:]), flush=True)
        del gs, bank, sim
        torch.cuda.empty_cache()

    lines += ["", "normalised search, k = %d: plain = ops.sim_topk; static = ops.sim_topk_norm; dynamic = ops.sim_topk (k = 1) + ops.hub_gate + "
              "ops.sim_topk_norm" % K, "%5s %8s %7s %10s %10s %10s %13s %14s" % ("Nq", "Ng", "copies", "plain ms", "static ms", "dynamic ms",
                                                                               "static/plain", "dynamic/plain")]
    for Ng in (10000, 100000):
        copies = max(1, min(20, -(-600 * 2 ** 20 // (Ng * H * 4))))
        gs = [unit(Ng, gen) for _ in range(copies)]
        bank = unit(1000, gen)
        cs = [ops.sim_colstat(bank, g, BETA) for g in gs]
        hubs = [ops.hub_flags(ops.sim_topk(bank, g, 1)[1], Ng) for g in gs]
        for Nq in (16, 64):
            q = unit(Nq, gen)

            def dynamic(i):
                g = gs[i % copies]
                gate = ops.hub_gate(ops.sim_topk(q, g, 1)[1], hubs[i % copies])
                return ops.sim_topk_norm(q, g, K, cs[i % copies], row_gate=gate)
            res = race([("plain", lambda i: ops.sim_topk(q, gs[i % copies], K)),
                        ("static", lambda i: ops.sim_topk_norm(q, gs[i % copies], K, cs[i % copies])), ("dynamic", dynamic)], a.rounds)
            p, s, d = res["plain"][0], res["static"][0], res["dynamic"][0]
            lines.append("%5d %8d %7d %10.4f %10.4f %10.4f %13.2f %14.2f" % (Nq, Ng, copies, p, s, d, s / p, d / p))
            lines.append("        rounds " + "   ".join("%s: %s" % (n, " ".join("%.4f" % t for t in res[n][1])) for n in ("plain", "static", "dynamic")))
            print("\n".join(lines[-2:]), flush=True)
        del gs, cs, hubs
        torch.cuda.empty_cache()

    # accuracy of the column term: the grid of tests/test_qbnorm_gpu.py::test_column_term_against_fp64
    cpu = torch.Generator().manual_seed(31)
    u64 = lambda n: torch.nn.functional.normalize(torch.randn(n, H, generator=cpu, dtype=torch.float64), dim=-1).float()
    bank, g = u64(1000), u64(300)
    s64 = (bank.double() @ g.double().t()).numpy()
    bank, g, worst = bank.to(DEV), g.to(DEV), 0.0
    for beta in (1.0, 20.0, 100.0):
        for Nb in (1, 5, 127, 128, 129, 1000):
            for Ng in (1, 17, 33, 300):
                s = s64[:Nb, :Ng]
                m = s.max(0)
                c64 = m + np.log(np.exp(beta * (s - m)).sum(0)) / beta
                worst = max(worst, float(np.abs(ops.sim_colstat(bank[:Nb], g[:Ng], beta).cpu().numpy().astype(np.float64) - c64).max()))
    lines += ["", "accuracy: max |c - c64| = %.3e over beta in {1, 20, 100} x Nb in {1, 5, 127, 128, 129, 1000} x Ng in {1, 17, 33, 300} "
              "(random unit vectors; the tests' gate is 2e-4)" % worst]
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
