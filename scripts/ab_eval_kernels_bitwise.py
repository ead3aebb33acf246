"""One fixed, seeded input set through the evaluation entry points that share csrc/ranked.h and csrc/vocab_ce.h, every output tensor
written to an .npz: run it once per build of the library, each in a fresh process, and compare the files with numpy.array_equal.

    python scripts/ab_eval_kernels_bitwise.py <libunivl_hip.so> <out.npz>

Entry points: univl_beam_step (a first and a later step, n_bm = 5), univl_beam_group_step (G = 2, lambda = 0.5, a first and a later
step), univl_beam_pool_step over a run of tests/pool_beam_ref.py (n_bm = 5) with univl_beam_pool_finish (n_best = 3), univl_beam_backtrack
-- each at (V, ld) = (37, 40) and (30522, 30528) with one of 3 instances preset done --, univl_sample_step (k = 50), univl_sim_topk (Nq = 33, Ng = 300,
k = 10, with a target), univl_sim_colstat (Nb = 129, Ng = 33), univl_hub_flags / univl_hub_gate, univl_sim_topk_norm (Nq = 17, Ng = 65,
k = 10, gated and with a target), univl_window_norms and univl_moment_localize (F = 8 and 50, a masked frame, candidates outside the
gallery), univl_vocab_score, univl_vocab_ce_fwd / _bwd.  Every input set holds engineered ties: equal values whose order only the tie
rule (lower index first) decides."""
import os
import sys

import numpy as np


def main(lib_path, out_path):
    os.environ["UNIVL_LIB"] = os.path.abspath(lib_path)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from univl_amd import _lib, ops
    assert os.path.samefile(_lib.LIB_PATH, lib_path)
    dev = "cuda"
    out = {}

    def gen(*shape, seed, scale=1.0):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale

    def keep(prefix, **ts):
        torch.cuda.synchronize()
        for k, t in ts.items():
            t = t.detach().cpu()
            out[prefix + "." + k] = (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy()

    # ---- univl_beam_step: 4 instances x 5 beams, V = 30522 (row stride 30528); ties inside a row, across slices and across beams
    n_inst, nb, V, LD, Tmax = 4, 5, 30522, 30528, 4
    R = n_inst * nb
    lp = torch.log_softmax(gen(R, LD, seed=11), 1)
    top = float(lp.max()) + 1.0
    lp[0, [7, 8, 20000, 30521]] = top                  # first step reads row 0 of an instance: four equal best, two slices
    lp[5, [100, 101]] = top
    lp[6, 3] = lp[7, 3] = top + 1.0                    # later step: with equal scores, beams 1 and 2 of instance 1 tie on a flat index
    lp[6, 30000] = lp[7, 29999] = top + 1.0
    lp = lp.to(dev)
    state = dict(scores=torch.zeros(R, device=dev), done=torch.zeros(n_inst, dtype=torch.uint8, device=dev),
                 length=torch.zeros(n_inst, dtype=torch.int32, device=dev), tokens=torch.zeros(R, dtype=torch.int64, device=dev),
                 src=torch.zeros(R, dtype=torch.int32, device=dev), hist_parents=torch.zeros(Tmax, R, dtype=torch.int32, device=dev),
                 hist_tokens=torch.zeros(Tmax, R, dtype=torch.int32, device=dev), hist_scores=torch.zeros(Tmax, R, device=dev),
                 ws=torch.zeros(R * _lib.BEAM_SLICES * nb * 2, device=dev))
    ops.beam_step(lp, V, n_inst, nb, 0, **state)
    keep("beam.first", **{k: v.clone() for k, v in state.items() if k != "ws"})
    state["scores"][5:10] = 0.25                       # instance 1: five equal accumulated scores
    state["done"][3] = 1                               # a frozen instance
    ops.beam_step(lp, V, n_inst, nb, 1, **state)
    keep("beam.later", **{k: v for k, v in state.items() if k != "ws"})

    # ---- the group step, the pooled step with its finish, and the walk-back: 3 instances (the last one preset done: frozen rows) on
    # the log-probabilities of tests/pool_beam_ref.py (multiples of 1/4: ties everywhere), scalar loads in one slice and 16-byte
    # loads in several
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import pool_beam_ref as PR
    n3, T3 = PR.N_INST, PR.TMAX

    def beam_state(nb, units):
        R3 = n3 * nb
        s = dict(scores=torch.zeros(R3, device=dev), done=torch.zeros(units, dtype=torch.uint8, device=dev),
                 length=torch.zeros(units, dtype=torch.int32, device=dev), tokens=torch.zeros(R3, dtype=torch.int64, device=dev),
                 src=torch.zeros(R3, dtype=torch.int32, device=dev), hist_parents=torch.zeros(T3, n3, nb, dtype=torch.int32, device=dev),
                 hist_tokens=torch.zeros(T3, n3, nb, dtype=torch.int32, device=dev), hist_scores=torch.zeros(T3, n3, nb, device=dev),
                 ws=ops.beam_ws(n3, nb, dev))
        s["done"][units - 1] = 1
        return s

    for Vb, ldb in ((37, 40), (30522, 30528)):
        tag = "V%d" % Vb
        lps = [torch.from_numpy(x).to(dev) for x in PR.make_lps(21, 4, Vb, ldb)]
        s = beam_state(4, n3 * 2)
        for t, name in ((0, "first"), (1, "later")):
            ops.beam_group_step(lps[t], Vb, n3, 4, 2, t, diversity=0.5, eos=PR.EOS, **s)
            keep("group.%s.%s" % (tag, name), **{k: v.clone() for k, v in s.items() if k != "ws"})
        lps = [torch.from_numpy(x).to(dev) for x in PR.make_lps(PR.case_seed(5, Vb, 0, 0.6, False), 5, Vb, ldb)]
        s = beam_state(5, n3)
        pool = dict(ops.beam_pool(n3, 5, dev), w=ops.length_weights(0.6, T3).to(dev),
                    params=torch.tensor([0, T3], dtype=torch.int32, device=dev))
        for t in range(T3):
            ops.beam_pool_step(lps[t], Vb, n3, 5, t, eos=PR.EOS, **s, **pool)
            keep("pool.%s.t%d" % (tag, t), **{k: v.clone() for k, v in list(s.items()) + list(pool.items()) if k not in ("ws", "w", "params")})
        hyp, raw, key, ln, fin = ops.beam_pool_finish(ops.beam_pool_step_desc(lps[0], Vb, n3, 5, 0, eos=PR.EOS, **s, **pool), 3)
        keep("pool.%s.finish" % tag, hyp=hyp, raw=raw, key=key, len=ln, finished=fin)
        hyp, hs = ops.beam_backtrack(s["hist_parents"], s["hist_tokens"], s["scores"].view(n3, 5), s["length"], 3)
        keep("backtrack.%s" % tag, hyp=hyp, hyp_scores=hs)

    # ---- univl_sample_step: 12 rows, k = 50, top-p 0.9; rows of few distinct values, so that the k-th entry sits inside a tie
    Rs, k, Ts = 12, 50, 3
    x = gen(Rs, LD, seed=12, scale=2.0)
    x[0] = torch.round(x[0])                           # integers: thousands of equal logits
    x[1, :] = -1.0
    x[1, [30521, 5, 4096, 2048]] = 3.0
    x[2, 1000:1100] = float(x[2].max()) + 0.5          # a hundred equal best, k of them kept: the lowest columns
    x = x.to(dev)
    for name, ld_x in (("vec", x), ("scalar", x[:, 1:])):          # 16-byte loads, and the unaligned view that takes the scalar path
        Vs = V - 1 if name == "scalar" else V
        s = dict(done=torch.zeros(Rs, dtype=torch.uint8, device=dev), length=torch.zeros(Rs, dtype=torch.int32, device=dev),
                 ids=torch.zeros(Rs, dtype=torch.int64, device=dev), tokens_out=torch.full((Rs, Ts), -1, dtype=torch.int32, device=dev),
                 tok_logprob=torch.zeros(Rs, Ts, device=dev), q_logprob=torch.zeros(Rs, Ts, device=dev),
                 seq_logprob=torch.zeros(Rs, device=dev), seq_q_logprob=torch.zeros(Rs, device=dev), ws=ops.sample_ws(Rs, k, dev),
                 topk_idx=torch.zeros(Rs, k, dtype=torch.int32, device=dev), topk_val=torch.zeros(Rs, k, device=dev))
        s["done"][11] = 1
        for t in range(2):
            ops.sample_step(ld_x, Vs, k, t, inv_T=1.25, top_p=0.9, seed=1234, **s)
        keep("sample." + name, **{kk: v for kk, v in s.items() if kk != "ws"})

    # ---- univl_sim_topk: Nq = 33 (two query blocks, the second partial), Ng = 300 (three gallery tiles), k = 10, with a target;
    # integer operands: exact scores, many equal; duplicated gallery rows tie exactly, within a tile and across tiles; two slice counts
    q = torch.randint(-2, 3, (33, 768), generator=torch.Generator().manual_seed(13)).float()
    g = torch.randint(-2, 3, (300, 768), generator=torch.Generator().manual_seed(14)).float()
    g[5] = g[4] = g[200] = g[299] = g[130]
    target = (torch.arange(33, dtype=torch.int32) * 9) % 300
    target[3] = 130
    for slices in (0, 1):
        score, idx, gt, eq = ops.sim_topk(q.to(dev), g.to(dev), 10, target=target.to(dev), slices=slices)
        keep("sim_topk.slices%d" % slices, score=score, idx=idx, gt=gt, eq=eq)
    score, idx = ops.sim_topk(q[:7].to(dev), g.to(dev), 64)         # one query block, the longest list
    keep("sim_topk.k64", score=score, idx=idx)

    # ---- query-bank normalisation: univl_sim_colstat at Nb = 129 (two bank tiles, the second one row), Ng = 33 (two gallery blocks);
    # univl_hub_flags / univl_hub_gate; univl_sim_topk_norm at Nq = 17, Ng = 65, k = 10 with a gate and a target.  Real-valued unit
    # vectors for the column term (its exp / log are the point), the integer operands above for the normalised search (ties).
    unit = lambda n, seed: torch.nn.functional.normalize(gen(n, 768, seed=seed), dim=-1)
    bank, gal = unit(129, 19).to(dev), unit(33, 20).to(dev)
    gal[7] = gal[30]
    keep("sim_colstat.Nb129", c=ops.sim_colstat(bank, gal, 20.0), c_beta1=ops.sim_colstat(bank, gal, 1.0))
    _, top = ops.sim_topk(bank, gal, 2)
    hub = ops.hub_flags(top, 33)
    _, top1 = ops.sim_topk(gal[:17], gal, 3)
    keep("hub", top=top, flags=hub, gate=ops.hub_gate(top1, hub), gate_1d=ops.hub_gate(top1[:, 0].contiguous(), hub))
    qn, gn = q[:17].to(dev), g[:65].to(dev)
    bias = (torch.arange(65) % 7).float().to(dev)                      # integers: the normalised scores stay exact, and tie
    gate = (torch.arange(17, dtype=torch.int32) % 3 != 1).to(torch.int32).to(dev)
    tgt = ((torch.arange(17, dtype=torch.int32) * 5) % 65).to(dev)
    score, idx, gt, eq = ops.sim_topk_norm(qn, gn, 10, bias, row_gate=gate, target=tgt)
    keep("sim_topk_norm.gated", score=score, idx=idx, gt=gt, eq=eq)
    score, idx = ops.sim_topk_norm(qn, gn, 10, bias)
    keep("sim_topk_norm.static", score=score, idx=idx)

    # ---- moment search: univl_window_norms and univl_moment_localize at F = 8 and F = 50, 5 gallery rows, a masked frame inside
    # row 1 and a short row 2, candidates that name every row, a row twice, -1 and a row past the gallery; both score forms
    for F in (8, 50):
        frames = gen(5, F, 768, seed=21 + F).to(dev)
        frames[3, 2] = frames[3, 1]                                    # equal frames: equal window scores, the tie rule decides
        fmask = torch.ones(5, F, dtype=torch.int64)
        fmask[1, F // 2] = 0
        fmask[2, F - 3:] = 0
        fmask = fmask.to(dev)
        wn = ops.window_norms(frames, fmask)
        qm = gen(3, 768, seed=23 + F).to(dev)
        rows = torch.tensor([[0, 1, 2, 3], [4, 4, -1, 5], [3, 2, 1, 0]], dtype=torch.int32, device=dev)
        for norm in (True, False):
            st, ln, sc = ops.moment_localize(qm, frames, fmask, rows, 1, F, wnorm=wn if norm else None, normalize=norm)
            st2, ln2, sc2 = ops.moment_localize(qm, frames, fmask, rows, 2, min(F, 5), wnorm=wn if norm else None, normalize=norm)
            keep("moment.F%d.%s" % (F, "norm" if norm else "mil"), start=st, length=ln, score=sc, start_w=st2, length_w=ln2, score_w=sc2)
        keep("window_norms.F%d" % F, wnorm=wn)

    # ---- the vocabulary head, both forms and the backward, fp32 (K = 32) and bf16 (K = 64): 130 rows x 1002 columns of integer
    # operands (exact logits), columns 3 / 130 / 1001 identical and lifted to the top on every third row; then real-valued operands at
    # 50 x 30522
    for dtype, K in ((torch.float32, 32), (torch.bfloat16, 64)):
        tag = "fp32" if dtype == torch.float32 else "bf16"
        gi = torch.Generator().manual_seed(15)
        rows, Vh = 130, 1002
        xi = torch.randint(-2, 3, (rows, K), generator=gi)
        ti = torch.randint(-2, 3, (Vh, K), generator=gi)
        bi = torch.randint(-3, 4, (Vh,), generator=gi)
        xi[:, 0], ti[:, 0] = 0, 0
        xi[::3, 0] = 1
        for c in (3, 130, 1001):
            ti[c], bi[c] = ti[3], bi[3]
            ti[c, 0] = 512
        lab = torch.randint(0, Vh, (rows,), generator=gi)
        lab[::5], lab[1], lab[2] = -1, 3, 1001
        cases = [("ties", xi.to(dev, dtype), ti.to(dev, dtype), bi.to(dev, torch.float32), lab.to(dev), Vh, 10),
                 ("big", gen(50, K, seed=16).to(dev, dtype), gen(V, K, seed=17, scale=0.2).to(dev, dtype), gen(V, seed=18, scale=0.5).to(dev),
                  torch.randint(-1, V, (50,), generator=gi).to(dev), V, 5)]
        for name, xx, tt, bb, ll, Vv, seq_len in cases:
            d, b = ops.vocab_score_desc(xx, tt, bb, ll, Vv, seq_len)
            ops.vocab_score(d)
            keep("vocab_score.%s.%s" % (tag, name), **{kk: v for kk, v in b.items() if kk != "keep"})
            dl = torch.zeros(xx.shape[0], (Vv + 7) // 8 * 8, device=dev, dtype=dtype)
            d, b = ops.vocab_ce_desc(xx, tt, bb, ll, dl, Vv)
            ops.vocab_ce_fwd(d)
            ops.vocab_ce_bwd(d)
            keep("vocab_ce.%s.%s" % (tag, name), dlogits=dl, **{kk: v for kk, v in b.items() if kk != "keep"})

    np.savez(out_path, **out)
    print("wrote %d arrays to %s (library %s)" % (len(out), out_path, lib_path))
    return 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
