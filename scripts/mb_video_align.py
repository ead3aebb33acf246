"""Micro-benchmark of video-to-video alignment (univl_amd/csrc/valign.hip: univl_video_align).

    python scripts/mb_video_align.py [--out profiles/video_align.txt]

Cells: 256 (exemplar, candidate) pairs -- 256 exemplars, one candidate each, out of 256 gallery rows -- for F in {48, 128}, prefix
masks of F / 2 .. F valid frames, local in {0, 1}; tau = 1 global, 0.05 local (frames are independent normal vectors, cosines near 0).
Beside every cell:
  torch    a torch formulation on the device of the same programme: one batched [F, 768] x [768, F] product per pair over frames
           gathered beforehand (the gather is not timed), the division by the norms, then a Python loop over the 2 F - 1
           anti-diagonals with maximum / where over all pairs at once; it yields the table H and the score, no path.  The scores of the
           two sides are held against each other on every pair before anything is timed;
  accuracy the largest errors against float64 over the grid of tests/test_video_align_gpu.py::test_kernel_against_fp64.

Timing as scripts/mb_moment.py: warmed up, HIP events, alternating rounds in this one process, the median round; a round is as many
back-to-back calls as fill ~50 ms (at most 50)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from univl_amd import ops  # noqa: E402
from mb_moment import race  # noqa: E402
import video_align_ref as VR  # noqa: E402

DEV = "cuda"
H, N, PAIRS = 768, 256, 256
NEG_INF = float("-inf")


def torch_programme(xa, xb, ta, tb, tau, local):
    """score [P] of the programme.  xa, xb: [P, F, H] gathered frames; ta, tb: [P] valid prefix lengths (>= 1)."""
    P, F = xa.shape[:2]
    na = xa.norm(dim=2).clamp_min(1e-12)
    nb = xb.norm(dim=2).clamp_min(1e-12)
    e = torch.bmm(xa, xb.transpose(1, 2)) / (na[:, :, None] * nb[:, None, :]) - tau
    Hp = torch.full((P, F + 1, F + 1), NEG_INF, device=xa.device)         # a border of -inf: the predecessors that do not exist
    for d in range(2 * F - 1):
        i = torch.arange(max(0, d - F + 1), min(d, F - 1) + 1, device=xa.device)
        j = d - i
        pm = torch.maximum(torch.maximum(Hp[:, i, j], Hp[:, i, j + 1]), Hp[:, i + 1, j])
        ed = e[:, i, j]
        Hp[:, i + 1, j + 1] = torch.where(pm > 0, ed + pm, ed) if local else torch.where(torch.isinf(pm), ed, ed + pm)
    Hh = Hp[:, 1:, 1:]
    if local:
        ar = torch.arange(F, device=xa.device)
        ok = (ar[None, :, None] < ta[:, None, None]) & (ar[None, None, :] < tb[:, None, None])
        return torch.where(ok, Hh, torch.full_like(Hh, NEG_INF)).flatten(1).max(1)[0]
    return Hh[torch.arange(P, device=xa.device), ta - 1, tb - 1]


def accuracy():
    """[match_score error, objective gap per cell, score error per cell], the largest over the parity grid."""
    worst = np.zeros(3)
    for F in VR.PARITY_F:
        frames, mask, ref, rows = VR.parity_case(F)
        d = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (frames, mask, ref, rows)]
        has = mask.any(1)
        for local in (0, 1):
            for tau in VR.PARITY_TAUS:
                out = [t.cpu().numpy() for t in ops.video_align(*d, tau, bool(local))]
                for p, c in zip(*np.nonzero(has[ref][:, None] & has[rows])):
                    E0, fa, gb = VR.parity_scores(F, int(ref[p]), int(rows[p, c]))
                    worst = np.maximum(worst, VR.check_pair(out, p, c, E0 - tau, fa, gb, F, local, 2e-4))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/video_align.txt")
    a = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    lines = ["video-to-video alignment, fp32, %s; median of %d alternating rounds" % (torch.cuda.get_device_name(0), a.rounds), "",
             "align = ops.video_align (univl_video_align and its six output allocations), %d exemplars x 1 candidate out of %d rows, prefix "
             "masks of F / 2 .. F frames; torch = bmm + a Python loop over the 2 F - 1 anti-diagonals with maximum / where, table and "
             "score only, no path" % (PAIRS, N),
             "%5s %6s %5s %10s %10s %12s" % ("F", "local", "tau", "align ms", "torch ms", "align/torch")]
    lost = []
    for F in (48, 128):
        frames = torch.randn(N, F, H, device=DEV, generator=gen)
        lv = torch.randint(F // 2, F + 1, (N,), device=DEV, generator=gen)
        mask = (torch.arange(F, device=DEV)[None, :] < lv[:, None]).long()
        ref = torch.randint(0, N, (PAIRS,), device=DEV, generator=gen, dtype=torch.int32)
        rows = torch.randint(0, N, (PAIRS, 1), device=DEV, generator=gen, dtype=torch.int32)
        xa, xb = frames[ref.long()].contiguous(), frames[rows[:, 0].long()].contiguous()
        ta, tb = lv[ref.long()], lv[rows[:, 0].long()]
        for local, tau in ((False, 1.0), (True, 0.05)):
            sides = [("align", lambda i: ops.video_align(frames, mask, ref, rows, tau, local)),
                     ("torch", lambda i: torch_programme(xa, xb, ta, tb, tau, local))]
            got, want = ops.video_align(frames, mask, ref, rows, tau, local), torch_programme(xa, xb, ta, tb, tau, local)
            worst = float(((got[0][:, 0] - want).abs() / got[1][:, 0]).max())
            assert worst <= 2e-4, worst                                   # one thing, computed twice: per path cell
            res = race(sides, a.rounds)
            m = {k: v[0] for k, v in res.items()}
            lines.append("%5d %6d %5g %10.4f %10.4f %12.4f" % (F, local, tau, m["align"], m["torch"], m["align"] / m["torch"]))
            lines.append("      rounds " + "   ".join("%s: %s" % (n, " ".join("%.4f" % t for t in res[n][1])) for n in res))
            lines.append("      largest |score - torch score| / path_len over the pairs: %.3e; mean path_len %.1f"
                         % (worst, float(got[1].float().mean())))
            if m["align"] > m["torch"]:
                lost.append("F=%d local=%d" % (F, local))
            print("\n".join(lines[-3:]), flush=True)
        del frames, xa, xb
        torch.cuda.empty_cache()
    lines += ["", "cells where the kernel LOSES to the torch formulation: " + (", ".join(lost) if lost else "none")]
    w = accuracy()
    lines += ["", "accuracy against float64 over the grid of the parity test (F in %s, both modes, tau in %s; frames of norm ~28; the tests' "
              "gate is 2e-4 per cell):" % (list(VR.PARITY_F), list(VR.PARITY_TAUS)),
              "  max |match_score - e64| = %.3e   max |objective64(returned) - optimum64| / path_len = %.3e   max |score - objective64(returned)| "
              "/ path_len = %.3e" % (w[0], w[1], w[2])]
    print("\n".join(lines[-4:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
