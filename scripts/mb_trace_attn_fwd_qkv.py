"""Where the microseconds of ONE fused q | k | v + attention forward launch go (univl_attention_fwd_fused, csrc/gemm.hip:
attn_fwd_qkv_kernel), as the step runs it: 4 x 48 tokens, K = 768, 12 heads, with the BertAdam chunks of a quarter of a layer riding.

    python univl_amd/build.py --trace                                              # lib/libunivl_hip_trace.so: the product's ring
    python univl_amd/build.py --variant trace2 -DUNIVL_TRACE -DUNIVL_ATTN_QKV_STAGES=2     # one stage in flight: the former schedule
    UNIVL_LIB=univl_amd/lib/libunivl_hip_trace2.so python scripts/mb_trace_attn_fwd_qkv.py [--chunks 216] [--batch 4] [--seq 48]

Method and clock: scripts/mb_trace_gemm.py (thread 0 of every workgroup stamps the 100 MHz device clock; stamp kernels in front of and
behind the launch, all captured into a hipGraph and replayed; weights and optimizer state rotate over > 256 MB so that every replay reads
them from HBM).  Attention workgroups stamp entry / first stage landed / end of the K loop / end; rider workgroups entry / end (last
store ISSUED).  Printed, medians over the replays, us:

    attn   tile1   entry -> first stage landed        (median / max over the attention workgroups)
           kloop   first stage -> end of the K loop
           epi     K loop -> end (epilogue + attention)
           wg      entry -> end
    rider  wg      entry -> end                        (median / max over the rider workgroups)
           last    first entry of the launch -> last rider end
    span   first entry -> last end of any workgroup;   total: stamp -> stamp
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("UNIVL_LIB", os.path.join(ROOT, "univl_amd", "lib", "libunivl_hip_trace.so"))

import torch  # noqa: E402

from univl_amd import _lib, ops  # noqa: E402

DEV, bf = "cuda", torch.bfloat16
CHUNK = 8192


def med(x):
    x = sorted(x)
    return x[len(x) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=216, help="riding chunks of 8192 elements (a quarter of a BERT-base layer: 216)")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--seq", type=int, default=48)
    ap.add_argument("--reps", type=int, default=24)
    a = ap.parse_args()
    B, S, H, K = a.batch, a.seq, 12, 768
    T, HD = B * S, H * 64
    L = _lib.lib()
    print("device:", torch.cuda.get_device_name(0), " lib:", os.environ["UNIVL_LIB"])
    rot = 8
    Ws = [torch.randn(3 * HD, K, device=DEV).to(bf) * 0.02 for _ in range(max(rot, int(300e6 // (3 * HD * K * 2)) + 1))]
    x = torch.randn(T, K, device=DEV).to(bf)
    bias = torch.randn(3 * HD, device=DEV)
    qkv = torch.zeros(T, 3 * HD, device=DEV, dtype=bf)
    ctx = torch.zeros(T, HD, device=DEV, dtype=bf)
    lse = torch.zeros(B, H, S, device=DEV)
    seed = torch.full((1,), 4321, dtype=torch.int64, device=DEV)
    at = ops.attention_desc(ops.dtype_code(bf), B, H, S, S, (qkv, 0), 3 * HD, (qkv, HD), 3 * HD, (qkv, 2 * HD), 3 * HD, ctx, HD, lse,
                            p_drop=0.1, offset=3 << 40, seed_dev=seed)
    # the riding update: ONE tensor of rot * chunks chunks; replay i carries chunks [i * chunks, + chunks)
    n = max(a.chunks, 1) * rot * CHUNK
    p = torch.randn(n, device=DEV) * 0.05
    g = torch.randn(n, device=DEV) * 1e-3
    m = torch.randn(n, device=DEV) * 1e-3
    v = torch.rand(n, device=DEV) * 1e-6
    p16, p16lo = p.to(bf), torch.zeros(n, device=DEV, dtype=bf)
    tb = ops.adam_tables([(0, n, 3e-5, 0.01, -1.0, 1)], [(0, c * CHUNK, CHUNK) for c in range(n // CHUNK)], DEV)
    keep = dict(sumsq=torch.ones(1, device=DEV), step=torch.zeros(1, dtype=torch.int32, device=DEV), seg_scalars=torch.zeros(2, device=DEV))
    ad = ops.adam_desc(tb, p, g, m, v, p16=p16, p16_lo=p16lo, **keep)
    ops.bert_adam_range(ad, 0, 0, do_prep=True)

    def launch(i):
        gd = ops.gemm_desc(x, Ws[i % len(Ws)], T, 3 * HD, K, out16=qkv, bias=bias)
        if a.chunks > 0:
            assert ops.attention_fwd_fused(at, gd, adam=ad, chunk_begin=(i % rot) * a.chunks, chunk_count=a.chunks)
        else:
            assert ops.attention_fwd_fused(at, gd)

    n_attn = B * H
    n_pad = (n_attn + 7) // 8 * 8
    cap = 4096
    trace = torch.zeros(cap * 4, dtype=torch.int64, device=DEV)
    st = torch.zeros(2, dtype=torch.int64, device=DEV)
    L.univl_trace_set.argtypes = [C.c_void_p, C.c_int]
    assert L.univl_trace_set(C.c_void_p(trace.data_ptr()), cap) == 0
    launch(0)                                     # the large-LDS opt-in, outside the capture
    torch.cuda.synchronize()
    graphs = []
    for i in range(rot):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            x.mul_(1.0)                           # the producing kernel of the step: leaves the activation in L2
            ops.stamp(st[0:1])
            launch(i)
            ops.stamp(st[1:2])
        graphs.append(gr)
    rows = []
    u = lambda t: float(t) / 100.0
    for r in range(a.reps):
        trace.zero_()
        torch.cuda.synchronize()
        graphs[r % rot].replay()
        torch.cuda.synchronize()
        t = trace.view(cap, 4).cpu().double()
        s0, s1 = [int(z) for z in st.cpu()]
        at_ = t[:n_attn]
        rd = t[n_pad:n_pad + a.chunks]
        first = min(float(at_[:, 0].min()), float(rd[:, 0].min()) if a.chunks else 1e30)
        last = max(float(at_[:, 3].max()), float(rd[:, 3].max()) if a.chunks else 0.0)
        row = dict(inn=u(first - s0), tile1_med=u((at_[:, 1] - at_[:, 0]).median()), tile1_max=u((at_[:, 1] - at_[:, 0]).max()),
                   kloop_med=u((at_[:, 2] - at_[:, 1]).median()), kloop_max=u((at_[:, 2] - at_[:, 1]).max()),
                   epi_med=u((at_[:, 3] - at_[:, 2]).median()), epi_max=u((at_[:, 3] - at_[:, 2]).max()),
                   wg_med=u((at_[:, 3] - at_[:, 0]).median()), wg_max=u((at_[:, 3] - at_[:, 0]).max()),
                   attn_last=u(at_[:, 3].max() - first), span=u(last - first), out=u(s1 - last), total=u(s1 - s0))
        if a.chunks:
            row.update(r_med=u((rd[:, 3] - rd[:, 0]).median()), r_max=u((rd[:, 3] - rd[:, 0]).max()), r_skew=u(rd[:, 0].max() - first),
                       r_last=u(rd[:, 3].max() - first))
        rows.append(row)
    rows = rows[4:]
    mm = {k: med([r[k] for r in rows]) for k in rows[0]}
    print("B %d S %d K %d, %d riding chunks, %d replays" % (B, S, K, a.chunks, len(rows)))
    print("attn : in %4.1f | tile1 %4.1f/%4.1f kloop %4.1f/%4.1f epi %4.1f/%4.1f wg %4.1f/%4.1f | last attention end %5.1f"
          % (mm["inn"], mm["tile1_med"], mm["tile1_max"], mm["kloop_med"], mm["kloop_max"], mm["epi_med"], mm["epi_max"], mm["wg_med"],
             mm["wg_max"], mm["attn_last"]))
    if a.chunks:
        print("rider: wg %4.1f/%4.1f | last rider entry %4.1f | last rider end %5.1f" % (mm["r_med"], mm["r_max"], mm["r_skew"], mm["r_last"]))
    print("span %5.1f out %4.1f | total %5.1f" % (mm["span"], mm["out"], mm["total"]))


if __name__ == "__main__":
    main()
