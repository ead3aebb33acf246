"""Micro-benchmark of the device-built document-frequency tables (univl_amd/csrc/ngram_df.hip: univl_ngram_df; univl_amd/caption_metrics.py:
DocumentFrequency, CaptionMetrics(df="device"); univl_amd/rl.py: caption_rewards(metric="cider")).

    python scripts/mb_ngram_df.py [--rounds 3] [--out profiles/ngram_df.txt]
    python scripts/mb_ngram_df.py --launches 3          # only a few ops.ngram_df calls at corpus size: the workload for a kernel trace

One process, alternating rounds.
(a) The workload of scripts/mb_caption_metrics.py: 3000 items x 20 references x 8 .. 48 tokens.  ops.ngram_df on rows already on the
    device (HIP events around back-to-back calls: workspace and output allocation and the enqueue of its launches included) against
    caption_metrics.document_frequency on the same rows (numpy on the host, wall clock).  The tables are compared before anything is timed.
(b) CaptionMetrics.compute_ids as a whole with df="host" and df="device" (wall clock).
(c) rl.caption_rewards + rl.advantages at 16 videos x 5 samples x 32 positions, 5 references each, with metric="cider" and the table of
    (a), against metric="rouge_l" (per call between HIP events around 50 back-to-back calls: allocation and enqueue included)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from univl_amd import ops, rl  # noqa: E402
from univl_amd import caption_metrics as M  # noqa: E402
from univl_amd.sample import SampleResult  # noqa: E402

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


def workload():
    rng = np.random.RandomState(0)
    word = lambda n: np.minimum((rng.pareto(1.1, size=n) * 4).astype(np.int64), VOCAB - 1).tolist()
    hyps = [word(rng.randint(8, TOKENS + 1)) for _ in range(ITEMS)]
    refs = [[word(rng.randint(8, TOKENS + 1)) for _ in range(REFS)] for _ in range(ITEMS)]
    rows = hyps + [r for rr in refs for r in rr]
    sym, lens = M._pack(rows)
    ref_begin = (np.arange(ITEMS + 1) * REFS).astype(np.int32)
    ref_rows = np.arange(ITEMS, ITEMS + ITEMS * REFS, dtype=np.int32)
    return hyps, refs, sym, lens, ref_begin, ref_rows


def table(lines, name, times, rounds, fmt="%10.3f"):
    if name is not None:
        lines.append(name)
    lines.append("%34s %s %12s %12s" % ("", " ".join("%10s" % ("round %d" % (i + 1)) for i in range(rounds)), "median ms", "max - min"))
    for k, ts in times.items():
        lines.append("%34s %s %12.4f %12.4f" % (k, " ".join(fmt % t for t in ts), statistics.median(ts), max(ts) - min(ts)))


def run(rounds, lines):
    hyps, refs, sym, lens, ref_begin, ref_rows = workload()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    d = [up(sym), up(lens), up(ref_begin), up(ref_rows)]
    n_refs = ITEMS * REFS
    device = lambda: ops.ngram_df(*d, n_refs)
    host = lambda: M.document_frequency(sym, lens, ref_begin, ref_rows)
    keys, cnt, begin_dev, status = device()
    begin = begin_dev.cpu().tolist()
    wk, wc, wb = host()
    same = (begin == list(wb) and int(status.cpu()[0]) == 0 and np.array_equal(keys.cpu().numpy().view(np.uint64)[:begin[4]], wk)
            and np.array_equal(cnt.cpu().numpy()[:begin[4]], wc))
    lines.append("(a) %d items x %d references x 8 .. %d tokens: %d rows, bound of %d keys, %d table entries; device tables equal the host's: %s"
                 % (ITEMS, REFS, TOKENS, n_refs, n_refs * 4 * sym.shape[1], begin[4], same))
    runs = {"ops.ngram_df (events, 5 calls)": lambda: events(device, 5), "document_frequency (host, wall)": lambda: wall(host)}
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            times[name].append(fn())
    table(lines, None, times, rounds)
    # ---- (b)
    cms = {"compute_ids df='host'": M.CaptionMetrics(DEV, df="host"), "compute_ids df='device'": M.CaptionMetrics(DEV, df="device")}
    for cm in cms.values():
        cm.compute_ids(hyps[:64], refs[:64])
    times = {k: [] for k in cms}
    results = {}
    for _ in range(rounds):
        for name, cm in cms.items():
            times[name].append(wall(lambda: results.__setitem__(name, cm.compute_ids(hyps, refs))))
    a, b = results.values()
    lines.append("")
    table(lines, "(b) CaptionMetrics.compute_ids on the same corpus, wall clock; every metric equal: %s"
          % all(a[k] == b[k] for k in a if k != "METEOR"), times, rounds)
    # ---- (c)
    n, ns, T, n_ref = 16, 5, 32, 5
    rng = np.random.RandomState(1)
    tok = torch.from_numpy(rng.randint(0, 40, size=(n, ns, T)).astype(np.int32)).to(DEV)
    z = torch.zeros(n, ns, T, device=DEV)
    res = SampleResult(tok, z, z.clone(), z[..., 0].clone(), z[..., 0].clone(),
                       torch.from_numpy(rng.randint(4, T + 1, size=(n, ns)).astype(np.int32)).to(DEV))
    ref_ids = torch.from_numpy(rng.randint(0, 40, size=(n, n_ref, T))).to(DEV)
    ref_len = torch.from_numpy(rng.randint(4, T + 1, size=(n, n_ref))).to(DEV)
    df = M.DocumentFrequency(keys[:begin[4]].clone(), cnt[:begin[4]].clone(), begin, ITEMS)
    runs = {"rewards + advantages, cider": lambda: rl.advantages(rl.caption_rewards(res, ref_ids, ref_len, -1, -1, metric="cider", df=df)),
            "rewards + advantages, rouge_l": lambda: rl.advantages(rl.caption_rewards(res, ref_ids, ref_len, -1, -1, metric="rouge_l"))}
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            times[name].append(events(fn, 50))
    lines.append("")
    table(lines, "(c) %d videos x %d samples x up to %d positions, %d references each, a table of %d entries; per call between events "
          "(allocation and enqueue included)" % (n, ns, T, n_ref, begin[4]), times, rounds, "%10.4f")
    build = lambda: M.DocumentFrequency.from_ids(ref_ids, ref_len)
    build()
    lines.append("    DocumentFrequency.from_ids of these %d x %d references, one call with its host read (wall): %.3f ms"
                 % (n, n_ref, wall(build)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/ngram_df.txt")
    ap.add_argument("--launches", type=int, default=0, help="only this many ops.ngram_df calls at corpus size, nothing written")
    a = ap.parse_args()
    if a.launches:
        _, _, sym, lens, ref_begin, ref_rows = workload()
        d = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (sym, lens, ref_begin, ref_rows)]
        for _ in range(a.launches):
            ops.ngram_df(*d, ITEMS * REFS)
        torch.cuda.synchronize()
        return
    lines = ["document-frequency tables on %s" % torch.cuda.get_device_name(0)]
    run(a.rounds, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
