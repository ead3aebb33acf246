"""Kernel-level fp64 parity WITH dropout: attention, LayerNorm and text-embedding kernels at p in {0.1, 0.5} against fp64 references
that apply the identical mask, rebuilt on the host from (seed, offset, index) by tests/dropout_ref.py.  Needs a real MI355X (`-m gpu`).

Every test has two steps.  Step 1 reads the mask out of the kernel (a launch whose output shows which elements were kept) and requires
equality with dropout_ref.keep_mask: a failure there says "the mask contract moved" (seed, offset, index formula, threshold).  Step 2
compares values and gradients with the fp64 reference under that mask: a failure there says "the arithmetic is wrong" (a lost
1 / (1 - p), a mask applied at the wrong place, a backward that regenerates another mask).

Gates are those of the p = 0 tests of the same kernels in test_kernels_gpu.py (dropout only zeroes and rescales terms): tol(dtype)
for attention, twice that for bf16 attention gradients, 1e-5 for the fp32 LayerNorm / embedding forward, 1e-4 for their gradients.
Observed worst errors: profiles/dropout_parity.txt."""
import numpy as np
import pytest
import torch

import dropout_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from univl_amd import ops

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
PS = [0.1, 0.5]
SEED_DEV_WORD = -(2 ** 63) + 0x1234567                  # int64 storage, high bit set: read as 2**63 + 0x1234567 by the kernels


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def tol(dtype):
    return 1e-3 if dtype == torch.float32 else 1e-2


def gen(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _seeds(with_dev, seed):
    """-> (seed_dev tensor or None, the effective seed the kernels use)."""
    if not with_dev:
        return None, R.effective_seed(seed)
    return torch.tensor([SEED_DEV_WORD], dtype=torch.int64, device=DEV), R.effective_seed(seed, SEED_DEV_WORD)


def _report(kernel, dtype, p, errs):
    print("[dropout parity] %s %s p=%g  " % (kernel, str(dtype).replace("torch.", ""), p)
          + "  ".join("%s=%.3e" % kv for kv in errs.items()))


# --------------------------------------------------------------------------------------------- attention
#             B   Sq   Sk  causal  layout    seed  offset
ATTN_CASES = [(2, 48, 48, False, "packed", 7, 3),
              (3, 20, 20, False, "split", 2 ** 63 + 11, 5 << 40),
              (2, 40, 56, False, "split", 42, 1 << 40),
              (2, 24, 24, True, "split", 9, 12),
              (1, 128, 128, False, "split", 42, 117 << 40),
              (1, 80, 80, True, "packed", 5, 2 << 40)]
H, D = 12, 64


def _attn_bias(mask, Sq, Sk, causal):
    """[B,1,Sq,Sk] additive bias as the kernels build it: -10000 where the key is masked or (causal) ahead of the query, else 0."""
    blocked = (mask[:, None, None, :] == 0).expand(mask.shape[0], 1, Sq, Sk)
    if causal:
        blocked = blocked | torch.triu(torch.ones(Sq, Sk, dtype=torch.bool), diagonal=1)[None, None]
    return blocked.double() * -10000.0


def _attn_buffers(layout, B, Sq, Sk, q, k, v, dtype):
    """q [B*Sq, H*D], k / v [B*Sk, H*D] (CPU fp32) -> device buffers in the layout, the positional arguments of ops.attention_* up to
    ldv, and a function that places gradient buffers the same way."""
    HDm = H * D
    if layout == "packed":
        assert Sq == Sk
        buf = torch.cat([q, k, v], dim=1).to(DEV, dtype).contiguous()
        a = ((buf, 0), 3 * HDm, (buf, HDm), 3 * HDm, (buf, 2 * HDm), 3 * HDm)

        def grads():
            g = torch.zeros_like(buf)
            kw = dict(dq=(g, 0), lddq=3 * HDm, dk=(g, HDm), lddk=3 * HDm, dv=(g, 2 * HDm), lddv=3 * HDm)
            return kw, lambda: (g[:, :HDm], g[:, HDm:2 * HDm], g[:, 2 * HDm:])
        return a, grads
    qb = q.to(DEV, dtype).contiguous()
    kvb = torch.cat([k, v], dim=1).to(DEV, dtype).contiguous()
    a = (qb, HDm, (kvb, 0), 2 * HDm, (kvb, HDm), 2 * HDm)

    def grads():
        gq, gkv = torch.zeros_like(qb), torch.zeros_like(kvb)
        kw = dict(dq=gq, lddq=HDm, dk=(gkv, 0), lddk=2 * HDm, dv=(gkv, HDm), lddv=2 * HDm)
        return kw, lambda: (gq, gkv[:, :HDm], gkv[:, HDm:])
    return a, grads


def _attn_read_probs(dtype, layout, B, Sq, Sk, q, k, mask_dev, causal, **drop):
    """The (dropped) probabilities [B,H,Sq,Sk] as the kernel computes them: V[b, key, h*64 + d] = (key - 64 * half == d), so that
    out[b, q, h*64 + d] is the probability of key 64 * half + d; one launch per 64 keys."""
    probs = torch.zeros(B, H, Sq, Sk)
    for half in range((Sk + 63) // 64):
        v = torch.zeros(B, Sk, H, D)
        for key in range(64 * half, min(Sk, 64 * half + 64)):
            v[:, key, :, key - 64 * half] = 1.0
        a, _ = _attn_buffers(layout, B, Sq, Sk, q, k, v.view(B * Sk, H * D), dtype)
        out = torch.zeros(B * Sq, H * D, device=DEV, dtype=dtype)
        lse = torch.zeros(B, H, Sq, device=DEV)
        ops.attention_fwd(ops.dtype_code(dtype), B, H, Sq, Sk, *a, out, H * D, lse, key_mask=mask_dev, causal=causal, **drop)
        n = min(Sk, 64 * half + 64) - 64 * half
        probs[..., 64 * half:64 * half + n] = out.float().cpu().view(B, Sq, H, D).permute(0, 2, 1, 3)[..., :n]
    return probs


def _attn_kernel_keep(dtype, layout, B, Sq, Sk, q, k, mask, causal, bias, **drop):
    """Step 1 for attention -> (keep bits read out of the kernel, the positions that can show theirs)."""
    mask_dev = mask.to(DEV)
    p0 = _attn_read_probs(dtype, layout, B, Sq, Sk, q, k, mask_dev, causal)
    pd = _attn_read_probs(dtype, layout, B, Sq, Sk, q, k, mask_dev, causal, **drop)
    # only a non-zero probability can show its mask bit; exp(-10000 - max) underflows to 0 exactly when the row has an unmasked key,
    # so the positions that cannot are exactly the masked keys of partly masked rows (a fully masked row is uniform, every key shows)
    blocked = (bias != 0).expand(B, 1, Sq, Sk)
    partly = (~blocked).any(-1, keepdim=True)
    hidden = (blocked & partly).expand(B, H, Sq, Sk)
    assert torch.equal(p0 == 0, hidden), "the undropped probabilities are zero somewhere else than at masked keys of partly masked rows"
    assert not bool(((pd != 0) & hidden).any())
    return (pd != 0), ~hidden


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(len(ATTN_CASES)))
def test_attention_dropout_parity(case, dtype, p):
    B, Sq, Sk, causal, layout, seed, offset = ATTN_CASES[case]
    with_dev = (case + PS.index(p)) % 2 == 1             # half of the cases: seed alone; the others: seed + a device word, high bit set
    seed_dev, eff = _seeds(with_dev, seed)
    q = gen(B * Sq, H * D, seed=1).to(dtype).float()     # the operands the kernel sees, exactly
    k = gen(B * Sk, H * D, seed=2).to(dtype).float()
    v = gen(B * Sk, H * D, seed=3).to(dtype).float()
    g = torch.Generator().manual_seed(3)
    lens = torch.randint(1, Sk + 1, (B,), generator=g)
    lens[0] = Sk
    mask = (torch.arange(Sk)[None] < lens[:, None]).long()          # ragged key masks
    if B > 1 and not causal:
        mask[1] = 0                                                 # a fully masked row
    if B == 1:
        mask[0, Sk - 5:] = 0
    bias = _attn_bias(mask, Sq, Sk, causal)
    drop = dict(p_drop=p, seed=seed, offset=offset, seed_dev=seed_dev)
    keep = R.keep_mask(eff, offset, R.attn_idx(B, H, Sq, Sk), p)

    # step 1: the kernel's mask is the host's
    got, shows = _attn_kernel_keep(dtype, layout, B, Sq, Sk, q, k, mask, causal, bias, **drop)
    want = torch.from_numpy(keep)
    assert torch.equal(got[shows], want[shows]), "attention forward: %d mask bits differ" % int((got != want)[shows].sum())
    assert 0.5 * (1 - p) < float(want.float().mean()) < 1 - 0.5 * p

    # step 2: values and gradients under that mask
    dt = ops.dtype_code(dtype)
    a, grads = _attn_buffers(layout, B, Sq, Sk, q, k, v, dtype)
    out = torch.zeros(B * Sq, H * D, device=DEV, dtype=dtype)
    lse = torch.zeros(B, H, Sq, device=DEV)
    args = (dt, B, H, Sq, Sk) + a + (out, H * D, lse)
    ops.attention_fwd(*args, key_mask=mask.to(DEV), causal=causal, **drop)
    qr = q.double().view(B, Sq, H * D).requires_grad_(True)
    kr = k.double().view(B, Sk, H * D).requires_grad_(True)
    vr = v.double().view(B, Sk, H * D).requires_grad_(True)
    ref = R.attention_ref(qr, kr, vr, bias, H, scale=R.scale_of(keep, p))
    errs = dict(out=rel_err(out.float().view(B, Sq, -1), ref))
    dout = gen(B * Sq, H * D, seed=4).to(DEV, dtype)
    ref.backward(dout.double().cpu().view(B, Sq, -1))
    gkw, views = grads()
    ops.attention_bwd(*args, key_mask=mask.to(DEV), causal=causal, dout=dout, lddo=H * D, **gkw, **drop)
    dq, dk, dv = views()
    errs["dq"] = rel_err(dq.float().view(B, Sq, -1), qr.grad)
    errs["dk"] = rel_err(dk.float().reshape(B, Sk, -1), kr.grad)
    errs["dv"] = rel_err(dv.float().reshape(B, Sk, -1), vr.grad)
    _report("attention", dtype, p, errs)
    t = tol(dtype) * (2 if dtype == torch.bfloat16 else 1)
    assert errs["out"] < tol(dtype), errs
    assert errs["dq"] < t and errs["dk"] < t and errs["dv"] < t, errs


# --------------------------------------------------------------------------------------------- LayerNorm
LN_SHAPES = [(768, 61), (768, 192), (1024, 100)]
#            mode     off_pre      off_post
LN_MODES = [("pre", 11, 0), ("post", 0, 3 << 40), ("both", 1 << 40, 2 << 40), ("both", 12, 11)]


def _no_exact_zero(t, what, floor=1e-6):
    """An fp32 kernel result is exactly 0 only where dropout put the zero: the fp64 value it rounds stays `floor` away from 0 (a
    normalised value carries the fp32 error of its row mean, some 1e-7; a copied input carries none)."""
    assert float(t.abs().min()) > floor, (what, float(t.abs().min()))


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", range(len(LN_MODES)))
@pytest.mark.parametrize("N,rows", LN_SHAPES)
def test_layernorm_dropout_parity(N, rows, mode, dtype, p):
    which, off_pre, off_post = LN_MODES[mode]
    p_pre, p_post = (p if which != "post" else 0.0), (p if which != "pre" else 0.0)
    with_dev = (mode + PS.index(p) + LN_SHAPES.index((N, rows))) % 2 == 1
    seed = 5 if mode % 2 == 0 else 2 ** 63 + 77
    seed_dev, eff = _seeds(with_dev, seed)
    dt = ops.dtype_code(dtype)
    period = 7
    x, res, pos = gen(rows, N, seed=1), gen(rows, N, seed=2), gen(period, N, seed=3)
    gamma, beta = 1 + 0.1 * gen(N, seed=4), 0.1 * gen(N, seed=5)
    dout = gen(rows, N, seed=6)
    keep_pre = R.keep_mask(eff, off_pre, R.ln_idx(rows, N), p_pre) if p_pre else np.ones((rows, N), dtype=bool)
    keep_post = R.keep_mask(eff, off_post, R.ln_idx(rows, N), p_post) if p_post else np.ones((rows, N), dtype=bool)
    s_pre = R.scale_of(keep_pre, p_pre) if p_pre else None
    s_post = R.scale_of(keep_post, p_post) if p_post else None
    drop = dict(p_pre=p_pre, p_post=p_post, seed=seed, off_pre=off_pre, off_post=off_post, seed_dev=seed_dev)
    dv = lambda t: t.to(DEV)
    empty = lambda *s, **kw: torch.empty(*s, device=DEV, **kw)
    zeros = lambda *s: torch.zeros(*s, device=DEV)

    # step 1: x alone, gamma = 1, beta = 0 -- y != 0 is the pre-mask, out32 != 0 the post-mask; nothing is excluded, because neither
    # the input nor the normalised rows of the masked input come near an exact zero
    # (inputs of magnitude >= 1 for this step: of ~1e5 normal draws some land within 1e-6 of their row mean)
    x1 = torch.sign(x) * (1 + x.abs())
    _no_exact_zero(x1.double(), "x", floor=0.0)
    _, _, _, plain = R.layernorm_ref(x1.double(), torch.ones(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64), scale_pre=s_pre)
    _no_exact_zero(plain, "LN(masked x)")
    y1, o1 = empty(rows, N), empty(rows, N)
    ops.layernorm_fwd(dtype=dt, rows=rows, N=N, x=dv(x1), gamma=torch.ones(N, device=DEV), beta=zeros(N), y=y1, out32=o1, **drop)
    assert torch.equal((y1 != 0).cpu(), torch.from_numpy(keep_pre)), "LayerNorm forward: the pre-dropout mask differs"
    assert torch.equal((o1 != 0).cpu(), torch.from_numpy(keep_post)), "LayerNorm forward: the post-dropout mask differs"

    # step 2: out = Mpost s_post LN(Mpre s_pre x + residual + pos)
    y, stats = empty(rows, N), empty(rows, 2)
    out32, out16 = empty(rows, N), empty(rows, N, dtype=dtype)
    ops.layernorm_fwd(dtype=dt, rows=rows, N=N, x=dv(x), residual=dv(res), pos=dv(pos), pos_period=period, gamma=dv(gamma), beta=dv(beta),
                      y=y, stats=stats, out32=out32, out16=out16, **drop)
    xr, rr, pr = (t.double().requires_grad_(True) for t in (x, res, pos))
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    yr, mean, rstd, ref = R.layernorm_ref(xr, gr, br, residual=rr, rowpos=pr[torch.arange(rows) % period], scale_pre=s_pre, scale_post=s_post)
    yr.retain_grad()
    errs = dict(y=rel_err(y, yr), mean=rel_err(stats[:, 0], mean), rstd=rel_err(stats[:, 1], rstd), out32=rel_err(out32, ref),
                out16=rel_err(out16.float(), ref))
    assert bool((out32.cpu()[~torch.from_numpy(keep_post)] == 0).all()), "a dropped output is not exactly 0.0"
    ref.backward(dout.double())
    dx32, dxd32, dxd16 = empty(rows, N), empty(rows, N), empty(rows, N, dtype=dtype)
    dg, db, dbias, dpos = zeros(N), zeros(N), zeros(N), zeros(period, N)
    ops.layernorm_bwd(dtype=dt, rows=rows, N=N, gamma=dv(gamma), y=y, stats=stats, dout=dv(dout), dx32=dx32, dxd32=dxd32, dxd16=dxd16,
                      dgamma=dg, dbeta=db, dbias=dbias, dpos=dpos, pos_period=period, **drop)
    errs.update(dx32=rel_err(dx32, yr.grad), dxd32=rel_err(dxd32, xr.grad), dxd16=rel_err(dxd16.float(), xr.grad),
                dgamma=rel_err(dg, gr.grad), dbeta=rel_err(db, br.grad), dbias=rel_err(dbias, xr.grad.sum(0)), dpos=rel_err(dpos, pr.grad))
    _report("layernorm[%s]" % which, dtype, p, errs)
    assert bool((dxd32.cpu()[~torch.from_numpy(keep_pre)] == 0).all()), "the gradient of a dropped input is not exactly 0.0"
    for k in ("y", "mean", "rstd", "out32"):
        assert errs[k] < 1e-5, (k, errs)
    for k in ("dx32", "dxd32", "dgamma", "dbeta", "dbias", "dpos"):
        assert errs[k] < 1e-4, (k, errs)
    assert errs["out16"] < tol(dtype) and errs["dxd16"] < tol(dtype), errs


# -------------------------------------------------------------------------------------------- embeddings
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_embed_text_dropout_parity(dtype, p):
    B, S, V, N = 3, 20, 500, 768
    with_dev = (DTYPES.index(dtype) + PS.index(p)) % 2 == 1
    seed, off = (42, 4 << 40) if p == 0.1 else (2 ** 63 + 3, 9)
    seed_dev, eff = _seeds(with_dev, seed)
    dt = ops.dtype_code(dtype)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, V, (B, S), generator=g)
    ids[0, :4] = 7                                        # repeated ids: scatter-add collisions
    tts = torch.randint(0, 2, (B, S), generator=g)
    word, pos, typ = gen(V, N, seed=2, scale=0.02), gen(64, N, seed=3, scale=0.02), gen(2, N, seed=4, scale=0.02)
    gamma, beta = 1 + 0.1 * gen(N, seed=5), 0.1 * gen(N, seed=6)
    keep = R.keep_mask(eff, off, R.ln_idx(B * S, N), p)
    s_post = R.scale_of(keep, p)
    drop = dict(p_post=p, seed=seed, off_post=off, seed_dev=seed_dev)
    dv = lambda t: t.to(DEV)
    tk = dict(type_ids=dv(tts), type_emb=dv(typ))

    # step 1: gamma = 1, beta = 0 -- out32 != 0 is the mask
    summed = (word.double()[ids] + pos.double()[torch.arange(S)][None] + typ.double()[tts]).view(B * S, N)
    _, _, _, plain = R.layernorm_ref(summed, torch.ones(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64))
    _no_exact_zero(plain, "LN(embedding sum)")
    o1 = torch.empty(B * S, N, device=DEV)
    ops.embed_text_fwd(dt, B, S, dv(ids), dv(word), dv(pos), torch.ones(N, device=DEV), torch.zeros(N, device=DEV), out32=o1, **tk, **drop)
    assert torch.equal((o1 != 0).cpu(), torch.from_numpy(keep)), "embedding forward: the dropout mask differs"

    # step 2
    y, stats = torch.empty(B * S, N, device=DEV), torch.empty(B * S, 2, device=DEV)
    out32, out16 = torch.empty(B * S, N, device=DEV), torch.empty(B * S, N, device=DEV, dtype=dtype)
    a = (dt, B, S, dv(ids), dv(word), dv(pos), dv(gamma), dv(beta))
    ops.embed_text_fwd(*a, y=y, stats=stats, out32=out32, out16=out16, **tk, **drop)
    wr, pr, tr = word.double().requires_grad_(True), pos.double().requires_grad_(True), typ.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    e = (wr[ids] + pr[torch.arange(S)][None] + tr[tts]).view(B * S, N)
    _, _, _, ref = R.layernorm_ref(e, gr, br, scale_post=s_post)
    errs = dict(out32=rel_err(out32, ref), out16=rel_err(out16.float(), ref))
    assert bool((out32.cpu()[~torch.from_numpy(keep)] == 0).all())
    dout = gen(B * S, N, seed=7)
    ref.backward(dout.double())
    dw, dp, dty = torch.zeros(V, N, device=DEV), torch.zeros(64, N, device=DEV), torch.zeros(2, N, device=DEV)
    dg, db = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    ops.embed_text_bwd(*a, y=y, stats=stats, dout=dv(dout), dword=dw, dpos=dp, dtype_emb=dty, dgamma=dg, dbeta=db, **tk, **drop)
    for name, got, want in (("dword", dw, wr.grad), ("dpos", dp, pr.grad), ("dtype_emb", dty, tr.grad), ("dgamma", dg, gr.grad),
                            ("dbeta", db, br.grad)):
        errs[name] = rel_err(got, want)
    _report("embed_text", dtype, p, errs)
    assert errs["out32"] < 1e-5 and errs["out16"] < tol(dtype), errs
    for name in ("dword", "dpos", "dtype_emb", "dgamma", "dbeta"):
        assert errs[name] < 1e-4, (name, errs)


# ------------------------------------------------------------- one training step against the oracle: the offset wiring
def _hook(offsets, host_seeds, word, p, seen):
    """The oracle's dropout hook: the mask of every site as the step's kernels draw it -- the site's stream offset and host seed (the
    model's read-only accessors), the device word of this step, the kernels' index formulas."""
    def drop(x, site):
        assert site in offsets, site
        seen.append(site)
        seed = R.effective_seed(host_seeds[site], word)
        if site.endswith(".probs"):
            B, nh, Sq, Sk = x.shape
            idx = R.attn_idx(B, nh, Sq, Sk)
        else:
            B, S, N = x.shape
            idx = R.ln_idx(B * S, N).reshape(B, S, N)
        return x * R.scale_of(R.keep_mask(seed, offsets[site], idx, p), p).to(x.dtype)
    return drop


@pytest.mark.parametrize("p,deterministic", [(0.1, True), (0.1, False), (0.0, True)])
def test_training_step_with_dropout_matches_the_oracle_under_the_same_masks(p, deterministic):
    """caption_small (text, video and cross stacks, decoder: every kind of dropout site) in fp32, two training steps: loss and every
    parameter gradient against the fp64 oracle whose dropout hook applies the host-rebuilt masks.  A forward and a backward plan that
    disagree about a site's offset, a site that shares a neighbour's stream, a device word that does not advance by exactly one per
    step -- each leaves the gradients of a different function than the oracle's.  Gates: those of the p = 0 comparison of the same
    quantities (test_model_gpu.py: test_joint_full_gradients_vs_oracle_elementwise, GATES[float32]); the p = 0 run through the same
    hook shows what the harness itself contributes."""
    import univl_amd
    import univl_oracle as O
    import test_model_gpu as M
    was = univl_amd._lib.deterministic()
    univl_amd.set_deterministic(deterministic)
    try:
        cfg, rows, dseed = M.case_config("caption_small")
        ns = M.task_ns(cfg, torch.float32)
        ns.dropout_prob = p
        model = univl_amd.UniVL.from_pretrained("bert-base-uncased", "visual-base", "cross-base", "decoder-base", cache_dir=None,
                                                state_dict=None, task_config=ns)
        P = O.procedural_params(cfg, 0)
        sd = dict(P)
        for alias, owner in O.tied_aliases(cfg).items():
            sd[alias] = P[owner]
        model.load_state_dict(sd, strict=True)
        model.to(DEV).train()
        batch = O.synthetic_batch(cfg, rows, seed=dseed)
        words = []
        for step in range(2):
            model.zero_grad(set_to_none=True)
            loss = M.call(model, batch)
            loss.backward()
            torch.cuda.synchronize()
            (offsets,), (host_seeds,) = model.dropout_offsets().values(), model.dropout_host_seeds().values()
            assert len(set(offsets.values())) == len(offsets) == 3 * 3 + 4 + 5 * cfg.decoder_num_hidden_layers
            assert all(o > 0 and o % (1 << 40) == 0 for o in offsets.values())
            assert {host_seeds[s] for s in host_seeds if s.endswith(".embeddings")} == {model._seed}
            word = int(model._seed_dev.item()) if p > 0 else 0
            words.append(word)
            seen = []
            Pr = {k: v.double().clone().requires_grad_(True) for k, v in P.items()}
            ref = O.univl_forward(Pr, cfg, batch, training=True, drop=_hook(offsets, host_seeds, word, p, seen))
            ref.backward()
            assert sorted(seen) == sorted(offsets), "the oracle and the step disagree about the dropout sites"
            worst, errs = 0.0, dict(loss=abs(float(loss) - float(ref.detach())))
            assert errs["loss"] < 1e-3, (step, float(loss), float(ref))
            for n, q in model.named_parameters():
                if Pr[n].grad is None:
                    assert q.grad is None, n
                    continue
                d = float((q.grad.double().cpu() - Pr[n].grad).norm())
                refn = float(Pr[n].grad.norm())
                assert d < 1e-3 * refn + 1e-6, (step, n, d, refn)
                if refn > 1e-3:
                    worst = max(worst, d / refn)
            errs["worst_tensor"] = worst
            _report("caption_small step %d (%s)" % (step, "deterministic" if deterministic else "atomic"), torch.float32, p, errs)
        if p > 0:
            assert words[1] == words[0] + 1, words             # one bump of the device word per forward
    finally:
        univl_amd.set_deterministic(was)
