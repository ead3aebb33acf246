"""Micro-benchmark of n-best moment search with temporal NMS (univl_amd/csrc/moment.hip: univl_moment_nbest).

    python scripts/mb_moment_nbest.py [--out profiles/moment_nbest.txt] [--parent-lib PATH]

Cells: 64 queries x 10 candidates out of 1024 gallery rows (the pairs of scripts/mb_moment.py), at 48 and 128 frames, window lengths
1 .. F, a normalising model and use_mil.  Beside every cell:
  nbest    univl_moment_nbest at M = 1 / 5 / 16 with nms (1, 2), on a descriptor filled once: the kernel, not the wrapper's three
           allocations, is timed;
  loc      univl_moment_localize on the same pairs, same way: what one window per pair costs -- nbest M = 1 over loc is the price of
           storing every score;
  parent   with --parent-lib: univl_moment_localize of a library built from the parent commit, loaded into this process, same call,
           same alternating rounds (the two kernels share their reduction now; this shows what that cost);
  loc 2    loc once more, right after parent.  In a round loc follows the torch formulation, which has just streamed hundreds of MB
           through the caches, while parent follows loc and finds the pairs' frames where loc left them: loc 2 is the same code as loc
           in parent's place, so parent is read against loc 2 and the difference loc - loc 2 is the place's, not the code's;
  torch    a torch formulation on the device: the frame products of every pair as one bmm over frames gathered beforehand (the gather
           of the frames and of the norm-table rows is not timed), every window's numerator as a difference of prefix sums, the
           division, -inf off the mask and the length range -- the [pairs, F, F] score matrix -- then M rounds of a flat argmax and an
           integer IoU mask.  It reads 42 MB of scores per round at 128 frames; its numerators are prefix differences, so its scores
           are not the kernel's to the bit and only slot 0 is held against the kernel's (1e-3).

Timing as scripts/mb_moment.py: warmed up, HIP events, alternating rounds in this one process, the median round; a round is as many
back-to-back calls as fill ~50 ms (at most 50)."""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from univl_amd import _lib, ops  # noqa: E402
from mb_moment import race  # noqa: E402

DEV = "cuda"
H, N, NQ, K = 768, 1024, 64, 10
NMS = (1, 2)
NEG_INF = float("-inf")


def _fill(d, q, frames, mask, wnorm, rows, lmin, lmax, normalize, slots):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    d.frames, d.ld_row, d.mask, d.wnorm = p(frames), frames.stride(0), p(mask), p(wnorm if normalize else None)
    d.N, d.F, d.H, d.normalize = frames.shape[0], frames.shape[1], H, 1 if normalize else 0
    d.q, d.ldq, d.rows, d.Nq, d.K, d.lmin, d.lmax = p(q), q.stride(0), p(rows), rows.shape[0], rows.shape[1], lmin, lmax
    shape = tuple(rows.shape) + ((slots,) if slots else ())
    keep = [torch.empty(shape, dtype=torch.int32, device=DEV), torch.empty(shape, dtype=torch.int32, device=DEV),
            torch.empty(shape, dtype=torch.float32, device=DEV)]
    d.start, d.length, d.score = (p(t) for t in keep)
    return keep


def raw_call(path, name, d):
    """A closure that calls entry point `name` of the library at `path` on the filled descriptor d."""
    L = C.CDLL(path)
    fn = getattr(L, name)
    fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p], C.c_int32
    assert getattr(L, name + "_sizeof" if name != "univl_moment_localize" else "univl_moment_sizeof")() == C.sizeof(d)

    def call(i):
        rc = fn(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
    return call


def torch_nbest(q, x, den, dead, M, num, iou_den):
    """q: [P, H]; x: [P, F, H] gathered frames; den: [P, F, F] the windows' denominators (s, L - 1); dead: [P, F, F] bool, no candidate.
    Returns (start, length, score) [P, M]."""
    P, F = x.shape[0], x.shape[1]
    d = torch.bmm(x, q[:, :, None])[:, :, 0]
    c = torch.nn.functional.pad(torch.cumsum(d, 1), (1, F))                                   # c[t] = d_0 + .. + d_{t-1}; zeros past the end
    s = torch.arange(F, device=q.device)
    end = s[:, None] + s[None, :] + 1                                                         # s + L
    sc = (c[:, end] - c[:, s][:, :, None]) / den
    sc = sc.masked_fill(dead, NEG_INF).reshape(P, F * F)
    s0, l0 = s[None, :, None], (s + 1)[None, None, :]
    out = []
    for m in range(M):
        v, at = sc.max(1)
        ps, pl = (at // F)[:, None, None], (at % F + 1)[:, None, None]
        out.append((torch.where(v > NEG_INF, ps[:, 0, 0], -1), torch.where(v > NEG_INF, pl[:, 0, 0], 0), v))
        inter = (torch.minimum(s0 + l0, ps + pl) - torch.maximum(s0, ps)).clamp_(min=0)
        kill = (iou_den * inter > num * (l0 + pl - inter)) | ((s0 == ps) & (l0 == pl))
        sc = sc.masked_fill(kill.reshape(P, F * F), NEG_INF)
    return tuple(torch.stack(t, 1) for t in zip(*out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/moment_nbest.txt")
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    Ms = (1, 5, 16)
    lines = ["n-best moment search, fp32, %s; median of %d alternating rounds" % (torch.cuda.get_device_name(0), a.rounds), "",
             "%d queries x %d candidates out of %d rows, lengths 1 .. F, nms (1, 2); nbest = univl_moment_nbest at M slots, loc = "
             "univl_moment_localize, parent = the parent commit's univl_moment_localize, loc 2 = loc again in parent's place of the round (all on "
             "descriptors filled once); torch = bmm, "
             "prefix differences, division and mask into a [pairs, F, F] matrix, then M rounds of argmax + IoU mask" % (NQ, K, N),
             "%5s %10s %9s %9s %9s %9s %9s %9s %9s %9s %9s %10s" % ("F", "mode", "loc", "parent", "loc 2", "nbest 1", "nbest 5", "nbest 16", "torch 1",
                                                                    "torch 5", "torch 16", "nb1 / loc")]
    lost = []
    for F in (48, 128):
        frames = torch.randn(N, F, H, device=DEV, generator=gen)
        lv = torch.randint(F // 2, F + 1, (N,), device=DEV, generator=gen)
        mask = (torch.arange(F, device=DEV)[None, :] < lv[:, None]).long()
        q = torch.nn.functional.normalize(torch.randn(NQ, H, device=DEV, generator=gen), dim=-1)
        rows = torch.randint(0, N, (NQ, K), device=DEV, generator=gen, dtype=torch.int32)
        wnorm = ops.window_norms(frames, mask)
        flat = rows.reshape(-1).long()
        x, qp = frames[flat].contiguous(), q.repeat_interleave(K, 0).contiguous()
        Ls = torch.arange(1, F + 1, device=DEV, dtype=torch.float32)
        fits = (torch.arange(F, device=DEV)[:, None] + torch.arange(1, F + 1, device=DEV)[None, :]) <= lv[flat][:, None, None]
        for normalize in (True, False):
            mode = "normalize" if normalize else "use_mil"
            den = torch.maximum(wnorm[flat], 1e-12 * Ls) if normalize else Ls.expand(flat.numel(), F, F).contiguous()
            dead = ~fits
            d_loc = _lib.Moment()
            keep = [_fill(d_loc, q, frames, mask, wnorm, rows, 1, F, normalize, 0)]
            sides = [("loc", raw_call(_lib.LIB_PATH, "univl_moment_localize", d_loc))]
            if a.parent_lib:
                sides.append(("parent", raw_call(a.parent_lib, "univl_moment_localize", d_loc)))
                sides.append(("loc 2", sides[0][1]))
            for M in Ms:
                d = _lib.MomentNbest()
                keep.append(_fill(d, q, frames, mask, wnorm, rows, 1, F, normalize, M))
                d.M, d.iou_num, d.iou_den = M, NMS[0], NMS[1]
                sides.append(("nbest %d" % M, raw_call(_lib.LIB_PATH, "univl_moment_nbest", d)))
                sides.append(("torch %d" % M, lambda i, M=M: torch_nbest(qp, x, den, dead, M, NMS[0], NMS[1])))
            # one thing, computed twice: slot 0 of the kernel against the torch formulation, and against univl_moment_localize bit for bit
            got = ops.moment_nbest(q, frames, mask, rows, 1, F, 16, NMS, wnorm=wnorm if normalize else None, normalize=normalize)
            loc = ops.moment_localize(q, frames, mask, rows, 1, F, wnorm=wnorm if normalize else None, normalize=normalize)
            want = torch_nbest(qp, x, den, dead, 16, NMS[0], NMS[1])
            assert all(torch.equal(g[:, :, 0], l) for g, l in zip(got, loc))
            assert float((got[2][:, :, 0].reshape(-1) - want[2][:, 0]).abs().max()) <= 1e-3
            res = race(sides, a.rounds)
            m = {k: v[0] for k, v in res.items()}
            cell = lambda k: "%9.4f" % m[k] if k in m else "%9s" % "-"
            lines.append("%5d %10s %s %s %s %s %s %s %s %s %s %10.2f" % (F, mode, cell("loc"), cell("parent"), cell("loc 2"), cell("nbest 1"),
                                                                          cell("nbest 5"), cell("nbest 16"), cell("torch 1"), cell("torch 5"),
                                                                          cell("torch 16"), m["nbest 1"] / m["loc"]))
            lines.append("      rounds " + "   ".join("%s: %s" % (n, " ".join("%.4f" % t for t in res[n][1])) for n in res))
            lost += ["F=%d %s M=%d" % (F, mode, M) for M in Ms if m["nbest %d" % M] > m["torch %d" % M]]
            print("\n".join(lines[-2:]), flush=True)
            del den, dead, keep
        del frames, wnorm, x
        torch.cuda.empty_cache()
    lines += ["", "cells where the kernel LOSES to the torch formulation: " + (", ".join(lost) if lost else "none")]
    print("\n".join(lines[-1:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
