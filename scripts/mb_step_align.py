"""Micro-benchmark of ordered step alignment (univl_amd/csrc/moment.hip: univl_step_align).

    python scripts/mb_step_align.py [--out profiles/step_align.txt] [--parent-lib PATH]

Cells: 256 (list, video) pairs -- 256 lists of K steps, one candidate each, out of 256 gallery rows -- for K in {1, 8, 32}, F in
{48, 128} and window in {(1, 1), (1, 8)}, a normalising model.  Beside every cell:
  loc      univl_moment_localize on the same 256 pairs with the lists' first step alone (K = 1): what one step costs on its own.
           Called on a descriptor filled once, without the wrapper's allocations: the kernel, not the host, is timed;
  parent   with --parent-lib: the same call on the same descriptor through a library built from the parent commit, loaded into this
           process, in the same alternating rounds (the two localisers share their device code now; this shows what that cost);
  torch    window (1, 1) only: a torch formulation on the device of the same programme -- one batched [K, 768] x [768, F] product
           per pair over frames gathered beforehand (the gather is not timed), the division by the frame norms, and per step one
           add and one reversed cummax over the frames.  It computes the totals only: no windows, no tie rule, no walk.
  accuracy the largest score error and total error per step against float64 over the grid of
           tests/test_step_align_gpu.py::test_kernel_against_fp64 (tests/step_align_ref.py's fixed-seed inputs).

Timing as scripts/mb_moment.py: warmed up, HIP events, alternating rounds in this one process, the median round; a round is as many
back-to-back calls as fill ~50 ms (at most 50)."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from univl_amd import _lib, ops  # noqa: E402
from mb_moment import race  # noqa: E402
import moment_ref as R  # noqa: E402
import step_align_ref as SR  # noqa: E402

DEV = "cuda"
H, N, PAIRS = 768, 256, 256


def torch_programme(q, x, inv_norm, valid):
    """Totals of the (1, 1) programme.  q: [P, K, H], x: [P, F, H] gathered frames, inv_norm: [P, F], valid: [P, F] bool."""
    P, K, F = q.shape[0], q.shape[1], x.shape[1]
    w = torch.bmm(q, x.transpose(1, 2)) * inv_norm[:, None, :]
    w = torch.where(valid[:, None, :], w, torch.full_like(w, float("-inf")))
    G = torch.zeros(P, F + 1, device=q.device)
    for k in range(K - 1, -1, -1):
        A = w[:, k] + G[:, 1:]
        G = torch.cat([A.flip(1).cummax(1)[0].flip(1), torch.full((P, 1), float("-inf"), device=q.device)], 1)
    return G[:, 0]


def raw_localize(path, q, frames, mask, wnorm, rows, lmin, lmax):
    """A closure that calls univl_moment_localize of the library at `path` on these tensors (UnivlMoment is the parent's too)."""
    L = C.CDLL(path)
    L.univl_moment_localize.argtypes, L.univl_moment_localize.restype = [C.c_void_p, C.c_void_p], C.c_int32
    d = _lib.Moment()
    assert L.univl_moment_sizeof() == C.sizeof(d)
    p = lambda t: C.c_void_p(t.data_ptr())
    d.frames, d.ld_row, d.mask, d.wnorm = p(frames), frames.stride(0), p(mask), p(wnorm)
    d.N, d.F, d.H, d.normalize = frames.shape[0], frames.shape[1], H, 1
    d.q, d.ldq, d.rows, d.Nq, d.K, d.lmin, d.lmax = p(q), q.stride(0), p(rows), rows.shape[0], rows.shape[1], lmin, lmax
    keep = [torch.empty(rows.shape, dtype=torch.int32, device=DEV), torch.empty(rows.shape, dtype=torch.int32, device=DEV),
            torch.empty(rows.shape, dtype=torch.float32, device=DEV)]
    d.start, d.length, d.score = (p(t) for t in keep)

    def call(i):
        rc = L.univl_moment_localize(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
    call.keep = keep
    return call


def accuracy():
    worst_score = worst_total = 0.0
    for F, K in SR.parity_shapes():
        frames, mask, q, counts, rows = SR.parity_case(F, K)
        d = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (frames, mask, q, counts, rows)]
        wnorm = ops.window_norms(d[0], d[1])
        for normalize in (True, False):
            for (lmin, lmax), (_, _, _, r_total) in SR.parity_reference(F, K, normalize).items():
                start, length, score, total = (t.cpu().numpy() for t in ops.step_align(d[2], d[3], d[0], d[1], d[4], lmin, lmax, wnorm=wnorm,
                                                                                        normalize=normalize))
                for i, c in zip(*np.nonzero(np.isfinite(r_total))):
                    n = int(counts[i])
                    S = SR.parity_scores(F, K, int(i), int(rows[i, c]), normalize)
                    s, l = start[i, c, :n], length[i, c, :n]
                    w64 = np.array([S[k, s[k], l[k] - 1] for k in range(n)])
                    worst_score = max(worst_score, float(np.abs(score[i, c, :n] - w64).max()))
                    worst_total = max(worst_total, abs(float(total[i, c]) - r_total[i, c]) / n, abs(SR.total_of(S, s, l) - r_total[i, c]) / n)
    return worst_score, worst_total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/step_align.txt")
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    lines = ["ordered step alignment, fp32, normalising, %s; median of %d alternating rounds" % (torch.cuda.get_device_name(0), a.rounds), "",
             "align = ops.step_align (univl_step_align and its four output allocations), %d lists of K steps x 1 candidate out of %d rows; "
             "loc = univl_moment_localize on the same pairs, first step only, descriptor filled once; parent = the parent commit's univl_moment_localize, same call; torch = bmm + K reversed cummax passes, totals only, "
             "window (1, 1)" % (PAIRS, N),
             "%5s %4s %8s %10s %10s %10s %10s %12s" % ("F", "K", "window", "align ms", "loc ms", "parent ms", "torch ms", "align/torch")]
    lost = []
    for F in (48, 128):
        frames = torch.randn(N, F, H, device=DEV, generator=gen)
        lv = torch.randint(F // 2, F + 1, (N,), device=DEV, generator=gen)
        mask = (torch.arange(F, device=DEV)[None, :] < lv[:, None]).long()
        wnorm = ops.window_norms(frames, mask)
        rows = torch.randint(0, N, (PAIRS, 1), device=DEV, generator=gen, dtype=torch.int32)
        x = frames[rows[:, 0].long()].contiguous()
        valid = mask[rows[:, 0].long()] != 0
        inv_norm = 1.0 / wnorm[rows[:, 0].long(), :, 0].clamp_min(1e-12)
        for K in (1, 8, 32):
            q = torch.nn.functional.normalize(torch.randn(PAIRS, K, H, device=DEV, generator=gen), dim=-1)
            counts = torch.full((PAIRS,), K, dtype=torch.int32, device=DEV)
            q1 = q[:, 0].contiguous()
            for window in ((1, 1), (1, 8)):
                sides = [("align", lambda i: ops.step_align(q, counts, frames, mask, rows, window[0], window[1], wnorm=wnorm)),
                         ("loc", raw_localize(_lib.LIB_PATH, q1, frames, mask, wnorm, rows, window[0], window[1]))]
                if a.parent_lib:
                    sides.append(("parent", raw_localize(a.parent_lib, q1, frames, mask, wnorm, rows, window[0], window[1])))
                if window == (1, 1):
                    sides.append(("torch", lambda i: torch_programme(q, x, inv_norm, valid)))
                    got, want = ops.step_align(q, counts, frames, mask, rows, 1, 1, wnorm=wnorm)[3][:, 0], torch_programme(q, x, inv_norm, valid)
                    ok = torch.isfinite(want)
                    assert torch.equal(torch.isfinite(got), ok) and float((got[ok] - want[ok]).abs().max()) <= K * 2e-4      # one thing, computed twice
                res = race(sides, a.rounds)
                m = {k: v[0] for k, v in res.items()}
                cell = lambda k: "%10.4f" % m[k] if k in m else "%10s" % "-"
                lines.append("%5d %4d %8s %s %s %s %s %12s" % (F, K, "(%d, %d)" % window, cell("align"), cell("loc"), cell("parent"), cell("torch"),
                                                                "%.2f" % (m["align"] / m["torch"]) if "torch" in m else "-"))
                lines.append("      rounds " + "   ".join("%s: %s" % (n, " ".join("%.4f" % t for t in res[n][1])) for n in res))
                if "torch" in m and m["align"] > m["torch"]:
                    lost.append("F=%d K=%d" % (F, K))
                print("\n".join(lines[-2:]), flush=True)
        del frames, wnorm, x
        torch.cuda.empty_cache()
    lines += ["", "cells where the kernel LOSES to the torch formulation (which returns no windows): " + (", ".join(lost) if lost else "none")]
    worst_score, worst_total = accuracy()
    lines += ["", "accuracy against float64 over the (F, K) grid and windows of the parity test, both modes (frames of norm ~28, unit step "
              "vectors; the tests' gate is 2e-4 per step):",
              "  max |score - score64| = %.3e   max |total - total64| / n = %.3e" % (worst_score, worst_total)]
    print("\n".join(lines[-4:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
