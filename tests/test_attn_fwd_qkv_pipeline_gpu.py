"""The K loop of univl_attention_fwd_fused's 64-row form (csrc/gemm.hip: attn_fwd_qkv_kernel<NT, false>) is a ring of 64-deep LDS stages
with counted DMA waits.  Everything here is BIT FOR BIT against the two launches it replaces (univl_gemm, then univl_attention_fwd) and,
for the chunks that ride in the launch, against univl_bert_adam_range on a copy -- never against the fused kernel itself.

Shapes: the projection depth K decides how the walk meets the ring (64: shorter than the ring; 128, 192: as long as / one short of the
slots that are in flight; 320: an odd count that wraps the ring once; 768: the step's), the sequence length S which rows of the 64-row block
exist (1, 20, 48, 64), B * H (12, 36, 48) how many padding workgroups sit between the attention ids and the rider ids.

Operand pairs at K = 192: univl_gemm itself walks a paired contraction in 128-deep steps and refuses K = 192, so the two-launch reference
there is univl_gemm on the CONCATENATED operands ([x | x | x_lo] . [W | W_lo | W]^T, 3 K deep, no lo halves): the same terms in the same
order through the same ascending 32-chunks into the same fp32 accumulators.  At K = 128, where univl_gemm takes the pair, the test
holds the two references against each other first."""
import functools

import pytest
import torch

import test_optim_gpu as OG

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from univl_amd import ops, _lib

DEV = "cuda"
H, D = 12, 64
HD = H * D
BF = torch.bfloat16
bits = OG.bits


def gen(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def pair(x32):
    hi = x32.to(BF)
    return hi, (x32 - hi.float()).to(BF)


@functools.lru_cache(maxsize=None)
def weights(K):
    """(W hi, W lo, bias) of the projection [3 * H * 64, K], on the device; made once per depth and never written."""
    wh, wl = pair(gen(3 * HD, K, seed=2, scale=0.05).to(DEV))
    return wh, wl, gen(3 * HD, seed=3).to(DEV)


@functools.lru_cache(maxsize=None)
def inputs(B, S, K):
    """(x hi, x lo, key mask): ragged lengths, row 0 full, row 1 (where there is one) fully masked."""
    xh, xl = pair(gen(B * S, K, seed=1).to(DEV))
    lens = torch.randint(1, S + 1, (B,), generator=torch.Generator().manual_seed(7))
    lens[0] = S
    mask = (torch.arange(S)[None] < lens[:, None]).long()
    if B > 1:
        mask[1] = 0
    return xh, xl, mask.to(DEV)


def run(B, S, K, p_drop, fused, which="", concat=False, riders=None):
    """One forward: (qkv, ctx, ctx lo half, lse).  fused: univl_attention_fwd_fused (riders = (desc, begin, count, max_blocks) ride in
    it); else univl_gemm + univl_attention_fwd -- concat: the paired product as one plain product over the concatenated contraction."""
    dt = ops.dtype_code(BF)
    T = B * S
    xh, xl, km = inputs(B, S, K)
    wh, wl, bias = weights(K)
    a_lo = xl if "a" in which else None
    b_lo = wl if "b" in which else None
    seed = torch.full((1,), 4321, dtype=torch.int64, device=DEV)
    kw = dict(key_mask=km, p_drop=p_drop, offset=3 << 40, seed_dev=seed)
    qkv = torch.full((T + 2, 3 * HD), 5.0, device=DEV, dtype=BF)[:T]          # (two guard rows behind the buffer)
    ctx, ctx_lo = torch.zeros(T, HD, device=DEV, dtype=BF), torch.zeros(T, HD, device=DEV, dtype=BF)
    lse = torch.zeros(B, H, S, device=DEV)
    args = (dt, B, H, S, S, (qkv, 0), 3 * HD, (qkv, HD), 3 * HD, (qkv, 2 * HD), 3 * HD, ctx, HD, lse)
    out_lo = dict(out_lo=ctx_lo) if which else {}
    if fused:
        gd = ops.gemm_desc(xh, wh, T, 3 * HD, K, out16=qkv, bias=bias, a_lo=a_lo, b_lo=b_lo)
        rk = {} if riders is None else dict(adam=riders[0], chunk_begin=riders[1], chunk_count=riders[2], max_blocks=riders[3])
        assert ops.attention_fwd_fused(ops.attention_desc(*args, **out_lo, **kw), gd, **rk)
    else:
        if concat:
            xs = [xh] + ([xh] if b_lo is not None else []) + ([xl] if a_lo is not None else [])
            ws = [wh] + ([wl] if b_lo is not None else []) + ([wh] if a_lo is not None else [])
            xc, wc = torch.cat(xs, dim=1).contiguous(), torch.cat(ws, dim=1).contiguous()
            ops.gemm(xc, wc, T, 3 * HD, xc.shape[1], out16=qkv, bias=bias)
        else:
            gd = ops.gemm_desc(xh, wh, T, 3 * HD, K, out16=qkv, bias=bias, a_lo=a_lo, b_lo=b_lo)
            _lib.check(_lib.lib().univl_gemm(ops._BYREF(gd), ops._stream()), "gemm")
        ops.attention_fwd(*args, **out_lo, **kw)
    torch.cuda.synchronize()
    return qkv.clone(), ctx, ctx_lo, lse


def same(got, ref, what):
    for name, g, r in zip(("qkv", "ctx", "ctx_lo", "lse"), got, ref):
        assert torch.equal(bits(g), bits(r)), "%s: %s differs in %d places" % (what, name, int((bits(g) != bits(r)).sum()))


@pytest.mark.parametrize("S", [1, 20, 48, 64])
@pytest.mark.parametrize("K", [64, 128, 192, 320, 768])
def test_every_projection_depth_and_sequence_length_equals_the_two_launches(K, S):
    """B = 1 and B = 3 (12 and 36 attention workgroups: 4 padding workgroups behind them) and the step's B = 4; key-padding masks with a
    fully masked row; dropout off and at 0.1."""
    for B in (1, 3, 4):
        for p_drop in (0.0, 0.1):
            ref = run(B, S, K, p_drop, fused=False)
            assert bool(ref[0].float().abs().max() > 0)
            same(run(B, S, K, p_drop, fused=True), ref, "B %d p_drop %g" % (B, p_drop))


@pytest.mark.parametrize("which", ["b", "ab"])
@pytest.mark.parametrize("K", [128, 192])
def test_operand_pairs_with_a_term_boundary_inside_the_ring(K, which):
    """2 or 3 terms of 2 or 3 stages each: the pointers are re-pointed at stage 2 / 3 (K = 128: the last slot of the prologue and the
    first re-issued one; K = 192: the first slot of the second lap) and again at 4 / 6."""
    for B, S, p_drop in ((3, 20, 0.1), (4, 48, 0.0), (1, 64, 0.1)):
        ref = run(B, S, K, p_drop, fused=False, which=which, concat=True)
        if K % 128 == 0:
            same(run(B, S, K, p_drop, fused=False, which=which), ref, "univl_gemm: paired descriptor against the concatenated product")
        assert bool(ref[2].float().abs().max() > 0)
        same(run(B, S, K, p_drop, fused=True, which=which), ref, "B %d S %d" % (B, S))


def _chunk_ranges():
    """(begin, count, max_blocks): one chunk (a full 8192-element one); more chunks than rider workgroups, ending with the tensor of
    2 * 8192 + 7 elements, whose last chunk has a scalar tail."""
    lay = OG.layout()
    full = next(i for i, c in enumerate(lay.chunks) if c[2] == 8192)
    last = max(i for i, c in enumerate(lay.chunks) if c[0] == 9)
    assert lay.segs[9][1] % 4 != 0 and lay.chunks[last][2] % 4 != 0 and last + 1 > 3
    return [(full, 1, 0), (0, last + 1, 3)]


@pytest.mark.parametrize("B,K", [(4, 768), (3, 128)])
def test_riding_chunks_equal_bert_adam_range(B, K):
    S, p_drop = 48, 0.1
    ref = run(B, S, K, p_drop, fused=False)
    # no chunks, no descriptor
    same(run(B, S, K, p_drop, fused=True, riders=(None, 0, 0, 0)), ref, "adam = NULL")
    for begin, count, mb in _chunk_ranges():
        a, da, b, db = OG.prepared()
        same(run(B, S, K, p_drop, fused=True, riders=(da, begin, count, mb)), ref, "chunks [%d, +%d)" % (begin, count))
        ops.bert_adam_range(db, begin, count)
        OG.same_state(a, b)                                  # p / g / m / v and both shadows
        assert not torch.equal(bits(a.p), bits(a.orig["p"]))
        a.assert_guards(also_unchanged=("g",))


def test_grids_the_ring_does_not_take_keep_the_two_stage_form():
    """The ring's LDS holds the launch to one workgroup per compute unit; the host takes it where every attention workgroup has a unit
    and the riders pass in two rounds over the rest (256 units).  B = 22: 264 attention workgroups; B = 21: 252 (256 with padding)
    and riders with no unit left.  Same bits either way."""
    S, K = 20, 128
    ref = run(22, S, K, 0.1, fused=False)
    same(run(22, S, K, 0.1, fused=True), ref, "B 22")
    ref = run(21, S, K, 0.1, fused=False)
    begin, count, mb = _chunk_ranges()[1]
    a, da, b, db = OG.prepared()
    same(run(21, S, K, 0.1, fused=True, riders=(da, begin, count, mb)), ref, "B 21 with riders")
    ops.bert_adam_range(db, begin, count)
    OG.same_state(a, b)
    a.assert_guards(also_unchanged=("g",))


def test_twenty_launches_with_riders_repeat_the_first():
    """A missing wait on a ring slot shows as a run-to-run difference, not on every launch."""
    B, S, K = 4, 48, 768
    ref = run(B, S, K, 0.1, fused=False)
    a, da, b, db = OG.prepared()
    n = a.tb.nchunk
    first = run(B, S, K, 0.1, fused=True, riders=(da, 0, n, 5))
    same(first, ref, "launch 0")
    for it in range(1, 20):
        same(run(B, S, K, 0.1, fused=True, riders=(da, 0, n, 5)), first, "launch %d" % it)
    for _ in range(20):
        ops.bert_adam_range(db, 0, n)
    OG.same_state(a, b)
    a.assert_guards(also_unchanged=("g",))
