"""Micro-benchmark of moment search (univl_amd/csrc/moment.hip: univl_window_norms, univl_moment_localize).

    python scripts/mb_moment.py [--out profiles/moment_search.txt]

Cells:
  window norms   univl_window_norms over 1024 gallery rows at 48 and at 128 frames (once per row in the life of an index);
  localize       univl_moment_localize for 64 queries x 10 candidates out of those 1024 rows, window lengths 1 .. F, normalising
                 and use_mil, beside ops.sim_topk for the same 64 queries over the 1024 pooled rows (k = 10): what
                 VideoIndex.search_vectors runs, i.e. the search whose hits are being localised;
  accuracy       the largest score error and relative table error against float64 over the grid of
                 tests/test_moment_gpu.py::test_kernels_against_fp64 (tests/moment_ref.py's fixed-seed inputs).

Timing as scripts/mb_qbnorm.py: warmed up, HIP events, alternating rounds in this one process, the median round; a round is as many
back-to-back calls as fill ~50 ms (at most 50).  The 1024-row gallery is 151 MB at 48 frames and 403 MB at 128, so at 48 frames a
call may find part of it in the Infinity Cache, as a search that has just pooled these videos would."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from univl_amd import ops  # noqa: E402
import moment_ref as R  # noqa: E402

DEV = "cuda"
H, N, NQ, K = 768, 1024, 64, 10


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/moment_search.txt")
    a = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    lines = ["moment search, fp32, %s; median of %d alternating rounds" % (torch.cuda.get_device_name(0), a.rounds), "",
             "norms = univl_window_norms over %d rows; loc = univl_moment_localize, %d queries x %d candidates, lengths 1 .. F; "
             "topk = ops.sim_topk, %d queries x %d pooled rows, k = %d" % (N, NQ, K, NQ, N, K),
             "%5s %10s %12s %12s %10s %14s" % ("F", "norms ms", "loc norm ms", "loc mil ms", "topk ms", "loc norm/topk")]
    for F in (48, 128):
        frames = torch.randn(N, F, H, device=DEV, generator=gen)
        lv = torch.randint(F // 2, F + 1, (N,), device=DEV, generator=gen)
        mask = (torch.arange(F, device=DEV)[None, :] < lv[:, None]).long()
        q = torch.nn.functional.normalize(torch.randn(NQ, H, device=DEV, generator=gen), dim=-1)
        pooled = torch.nn.functional.normalize(frames.mean(1), dim=-1)
        rows = torch.randint(0, N, (NQ, K), device=DEV, generator=gen, dtype=torch.int32)
        wnorm = torch.empty(N, F, F, device=DEV)
        ops.window_norms(frames, mask, out=wnorm)
        res = race([("norms", lambda i: ops.window_norms(frames, mask, out=wnorm)),
                    ("loc_norm", lambda i: ops.moment_localize(q, frames, mask, rows, 1, F, wnorm=wnorm)),
                    ("loc_mil", lambda i: ops.moment_localize(q, frames, mask, rows, 1, F, normalize=False)),
                    ("topk", lambda i: ops.sim_topk(q, pooled, K))], a.rounds)
        m = {k: v[0] for k, v in res.items()}
        lines.append("%5d %10.4f %12.4f %12.4f %10.4f %14.2f" % (F, m["norms"], m["loc_norm"], m["loc_mil"], m["topk"], m["loc_norm"] / m["topk"]))
        lines.append("      rounds " + "   ".join("%s: %s" % (n, " ".join("%.4f" % t for t in res[n][1])) for n in res))
        print("\n".join(lines[-2:]), flush=True)
        del frames, wnorm
        torch.cuda.empty_cache()

    worst_score = worst_table = 0.0
    for F in R.PARITY_F:
        for P in R.PARITY_P:
            frames, mask, q, rows = R.parity_case(F, P)
            d = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (frames, mask, q, rows)]
            wnorm = ops.window_norms(d[0], d[1])
            for normalize in (True, False):
                ref, tables = R.parity_reference(F, P, normalize)
                if normalize:
                    t = wnorm.cpu().numpy().astype(np.float64)
                    worst_table = max(worst_table, float((np.abs(t - tables)[tables > 0] / tables[tables > 0]).max()))
                for (lmin, lmax), (_, _, score, _) in ref.items():
                    got = ops.moment_localize(d[2], d[0], d[1], d[3], lmin, lmax, wnorm=wnorm, normalize=normalize)[2].cpu().numpy()
                    ok = np.isfinite(score)
                    if ok.any():
                        worst_score = max(worst_score, float(np.abs(got[ok].astype(np.float64) - score[ok]).max()))
    lines += ["", "accuracy against float64 over F in {1, 2, 16, 48, 50, 128} x P in {1, 5, 37} x the length ranges of the parity test, both "
              "modes (frames of norm ~28, unit queries; the tests' gate is 2e-4):",
              "  max |score - score64| = %.3e   max relative table error = %.3e" % (worst_score, worst_table)]
    print("\n".join(lines[-2:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
