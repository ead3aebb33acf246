"""Tensor-level wrappers over the C ABI (one call = one enqueue on torch's current HIP stream).

PyTorch is used here only for device memory and streams.  Every function fills the C descriptor from tensor
pointers/strides and raises RuntimeError on a non-zero status.  The execution plans in `univl_amd.engine` build the
same descriptors once and replay them; these wrappers are the eager form (unit tests, small host-side ops)."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import DT_BF16, DT_F32

_BYREF = C.byref


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def dtype_code(dtype):
    if dtype == torch.float32:
        return DT_F32
    if dtype == torch.bfloat16:
        return DT_BF16
    raise RuntimeError("univl_amd: unsupported compute dtype %s (float32 or bfloat16)" % dtype)


def _require_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("univl_amd kernels need HIP device tensors (got %s); there is no CPU fallback" % t.device)


def _ld(t):
    assert t.dim() == 2 and t.stride(1) == 1, "expected a row-major 2-D view"
    return t.stride(0)


def _row_views(*ts):          # q, g, bank of the retrieval entry points; width, row stride and alignment are the library's to refuse
    assert all(t.dtype == torch.float32 and t.dim() == 2 for t in ts)


def _workspace(d, need, dev):
    """d.ws / d.ws_bytes: a fresh workspace of `need` bytes (a query's refusal, < 0, gets the least one), alive as long as d is."""
    d._ws_tensor = torch.empty(max(int(need), 16), dtype=torch.uint8, device=dev)
    d.ws, d.ws_bytes = _p(d._ws_tensor), d._ws_tensor.numel()


def _status_word(status, dev):
    """The optional status argument: the caller's int32 word, or a fresh zero."""
    status = torch.zeros(1, dtype=torch.int32, device=dev) if status is None else status
    assert status.dtype == torch.int32 and status.numel() == 1
    return status


def probe_layouts():
    out = torch.zeros(1792, device="cuda", dtype=torch.float32)
    _lib.check(_lib.lib().univl_probe_layouts(_p(out), 1792, _stream()), "probe_layouts")
    return out


def gemm_desc(A, B, M, N, K, *, trans_a=False, trans_b=False, out32=None, out16=None, bias=None, residual=None, aux=None,
              gelu=None, accumulate=False, dbias=None, dbias_atomic=False, ksplit=1, tile=0, alpha=1.0, sumsq=None,
              sumsq_rows=0, sumsq_stride=0, stages=0, waves=0, aux_f32=False, a_lo=None, b_lo=None, out16_lo=None):
    """a_lo / b_lo / out16_lo: the lo halves of operand pairs (include/univl_hip.h: UnivlGemm.A_lo), same shape and strides as A / B / out16."""
    _require_gpu(A, B, out32, out16, a_lo, b_lo, out16_lo)
    d = _lib.Gemm()
    d.dtype = dtype_code(A.dtype)
    assert B.dtype == A.dtype
    d.trans_a, d.trans_b = int(trans_a), int(trans_b)
    d.M, d.N, d.K = M, N, K
    d.A, d.lda, d.B, d.ldb = _p(A), _ld(A), _p(B), _ld(B)
    d.C32, d.C16 = _p(out32), _p(out16)
    d.ldc = _ld(out32) if out32 is not None else _ld(out16)
    if out32 is not None and out16 is not None:
        assert _ld(out32) == _ld(out16)
    d.bias = _p(bias)
    d.R, d.ldr = _p(residual), (_ld(residual) if residual is not None else 0)
    d.aux, d.ldaux = _p(aux), (_ld(aux) if aux is not None else 0)
    d.dbias = _p(dbias)
    d.alpha = alpha
    flags = 0
    if accumulate:
        flags |= _lib.GEMM_ACCUM
    if gelu == "fwd":
        flags |= _lib.GEMM_GELU_FWD
    elif gelu == "bwd":
        flags |= _lib.GEMM_GELU_BWD
    if dbias_atomic:
        flags |= _lib.GEMM_DBIAS_ATOMIC
    if aux_f32:
        flags |= _lib.GEMM_AUX_F32
    d.flags, d.ksplit, d.tile = flags, ksplit, tile
    d.sumsq, d.sumsq_rows, d.sumsq_stride = _p(sumsq), sumsq_rows, sumsq_stride
    d.stages, d.waves = int(stages), int(waves)
    for lo, hi in ((a_lo, A), (b_lo, B), (out16_lo, out16)):
        assert lo is None or (lo.dtype == hi.dtype and lo.stride() == hi.stride())
    d.A_lo, d.B_lo, d.C16_lo = _p(a_lo), _p(b_lo), _p(out16_lo)
    return d


def gemm(A, B, M, N, K, **kw):
    """C[M,N] = epi(alpha * A_op . B_op^T); A/B are 2-D row-major views ([rows,K] or, if trans_x, [K,rows])."""
    d = gemm_desc(A, B, M, N, K, **kw)
    _lib.check(_lib.lib().univl_gemm(_BYREF(d), _stream()), "gemm")


def gemm_group(descs, max_blocks=0):
    """Independent GEMMs (same dtype and operand layouts, at most GEMM_GROUP_MAX) in one launch; max_blocks > 0 caps the
    grid (the kernel walks its tiles)."""
    arr = (_lib.Gemm * len(descs))(*descs)
    _lib.check(_lib.lib().univl_gemm_group_limited(arr, len(descs), int(max_blocks), _stream()), "gemm_group")


def gemm_pair(dgrad, wgrad, dry_run=False):
    """One launch for a dgrad product and the weight-gradient product fed by the same upstream gradient
    (univl_gemm_pair).  Returns False when the C side does not take the pair (not bf16 / not on the 64 tile)."""
    rc = _lib.lib().univl_gemm_pair(_BYREF(dgrad), _BYREF(wgrad), int(bool(dry_run)), _stream())
    if rc == -3:
        return False
    _lib.check(rc, "gemm_pair")
    return True


def gemm_ln(gemm, ln, counters, dry_run=False, adam=None, chunk_begin=0, chunk_count=0, max_blocks=0):
    """A forward product and the LayerNorm that consumes its fp32 output in ONE launch (univl_gemm_ln).  Returns False when the C side
    does not carry the pair (deterministic mode, other tiles / layouts); counters: int32 [2 * ceil(M / 64)], zero.  adam (adam_desc) +
    chunk_begin / chunk_count / max_blocks: chunks of a prepared BertAdam update riding in the launch (default: none)."""
    rc = _lib.lib().univl_gemm_ln(_BYREF(gemm), _BYREF(ln), C.c_void_p(counters.data_ptr()), None if adam is None else _BYREF(adam),
                                  int(chunk_begin), int(chunk_count), int(max_blocks), int(bool(dry_run)), _stream())
    if rc == _lib.EUNSUPPORTED:
        return False
    _lib.check(rc, "gemm_ln")
    return True


def gemm_pair_ln(dgrad, wgrad, ln, counters, dry_run=False):
    """univl_gemm_pair with the LayerNorm backward fed by the dgrad's fp32 output finished inside the launch (univl_gemm_pair_ln)."""
    rc = _lib.lib().univl_gemm_pair_ln(_BYREF(dgrad), _BYREF(wgrad), _BYREF(ln), C.c_void_p(counters.data_ptr()), int(bool(dry_run)), _stream())
    if rc == _lib.EUNSUPPORTED:
        return False
    _lib.check(rc, "gemm_pair_ln")
    return True


def layernorm_desc(dtype, rows, N, *, x=None, x_f64=False, residual=None, pos=None, pos_period=0, gamma=None,
                   beta=None, eps=1e-12, y=None, stats=None, out32=None, out16=None, p_pre=0.0, p_post=0.0, seed=0,
                   off_pre=0, off_post=0, seed_dev=None, dout=None, dx32=None, dxd32=None, dxd16=None, dgamma=None,
                   dbeta=None, dbias=None, dpos=None, out16_lo=None):
    d = _lib.LayerNorm()
    d.dtype, d.rows, d.N, d.x_f64 = dtype, rows, N, int(x_f64)
    d.x, d.residual, d.pos, d.pos_period = _p(x), _p(residual), _p(pos), pos_period
    d.gamma, d.beta, d.eps = _p(gamma), _p(beta), eps
    d.y, d.stats, d.out32, d.out16 = _p(y), _p(stats), _p(out32), _p(out16)
    d.p_pre, d.p_post, d.seed, d.off_pre, d.off_post, d.seed_dev = p_pre, p_post, seed, off_pre, off_post, _p(seed_dev)
    d.dout, d.dx32, d.dxd32, d.dxd16 = _p(dout), _p(dx32), _p(dxd32), _p(dxd16)
    d.dgamma, d.dbeta, d.dbias, d.dpos = _p(dgamma), _p(dbeta), _p(dbias), _p(dpos)
    d.out16_lo = _p(out16_lo)
    return d


def layernorm_fwd(**kw):
    d = layernorm_desc(**kw)
    _lib.check(_lib.lib().univl_layernorm_fwd(_BYREF(d), _stream()), "layernorm_fwd")


def layernorm_bwd(**kw):
    d = layernorm_desc(**kw)
    _lib.check(_lib.lib().univl_layernorm_bwd(_BYREF(d), _stream()), "layernorm_bwd")


def attention_desc(dtype, B, H, Sq, Sk, q, ldq, k, ldk, v, ldv, out, ldo, lse, *, key_mask=None, causal=False,
                   p_drop=0.0, seed=0, offset=0, seed_dev=None, dout=None, lddo=0, dq=None, lddq=0, dk=None, lddk=0,
                   dv=None, lddv=0, bsk=0, bsv=0, out_lo=None):
    """q/k/v/out/... are (tensor, element_offset) pairs or tensors; ld in elements."""
    def ptr(t):
        if t is None:
            return None
        if isinstance(t, tuple):
            return C.c_void_p(t[0].data_ptr() + t[1] * t[0].element_size())
        return C.c_void_p(t.data_ptr())
    d = _lib.Attention()
    d.dtype, d.B, d.H, d.Sq, d.Sk = dtype, B, H, Sq, Sk
    d.q, d.ldq, d.k, d.ldk, d.v, d.ldv = ptr(q), ldq, ptr(k), ldk, ptr(v), ldv
    d.key_mask, d.causal = _p(key_mask), int(causal)
    d.out, d.ldo, d.lse = ptr(out), ldo, _p(lse)
    d.p_drop, d.seed, d.offset, d.seed_dev = p_drop, seed, offset, _p(seed_dev)
    d.dout, d.lddo, d.dq, d.lddq, d.dk, d.lddk, d.dv, d.lddv = ptr(dout), lddo, ptr(dq), lddq, ptr(dk), lddk, ptr(dv), lddv
    d.bsk, d.bsv = bsk, bsv
    d.out_lo = ptr(out_lo)
    return d


def attention_fwd(*a, **kw):
    d = attention_desc(*a, **kw)
    _lib.check(_lib.lib().univl_attention_fwd(_BYREF(d), _stream()), "attention_fwd")


def attention_bwd(*a, **kw):
    d = attention_desc(*a, **kw)
    _lib.check(_lib.lib().univl_attention_bwd(_BYREF(d), _stream()), "attention_bwd")


def attention_bwd_fused(attn, odgrad, owgrad=None, dry_run=False):
    """univl_attention_bwd with the attention-output dgrad that produces its upstream gradient computed inside the launch, the weight
    gradient of that projection optionally riding (univl_attention_bwd_fused).  Returns False where the C side does not carry the pair."""
    rc = _lib.lib().univl_attention_bwd_fused(_BYREF(attn), _BYREF(odgrad), _BYREF(owgrad) if owgrad is not None else None,
                                              int(bool(dry_run)), _stream())
    if rc == _lib.EUNSUPPORTED:
        return False
    _lib.check(rc, "attention_bwd_fused")
    return True


def attention_fwd_fused(attn, qkv, dry_run=False, adam=None, chunk_begin=0, chunk_count=0, max_blocks=0):
    """univl_attention_fwd with the q | k | v projection computed inside the launch (univl_attention_fwd_fused).  Returns False where
    the C side does not carry the pair.  adam (adam_desc) + chunk_begin / chunk_count / max_blocks: chunks of a prepared BertAdam update
    riding in the launch (default: none)."""
    rc = _lib.lib().univl_attention_fwd_fused(_BYREF(attn), _BYREF(qkv), None if adam is None else _BYREF(adam), int(chunk_begin),
                                              int(chunk_count), int(max_blocks), int(bool(dry_run)), _stream())
    if rc == _lib.EUNSUPPORTED:
        return False
    _lib.check(rc, "attention_fwd_fused")
    return True


def embed_text_desc(dtype, B, S, ids, word, pos, gamma, beta, *, type_ids=None, type_emb=None, eps=1e-12, y=None,
                    stats=None, out32=None, out16=None, p_post=0.0, seed=0, off_post=0, seed_dev=None, dout=None,
                    dword=None, dpos=None, dtype_emb=None, dgamma=None, dbeta=None, drows=None, out16_lo=None):
    d = _lib.EmbedText()
    d.dtype, d.B, d.S, d.N = dtype, B, S, 768
    d.ids, d.type_ids = _p(ids), _p(type_ids)
    d.word, d.pos, d.type = _p(word), _p(pos), _p(type_emb)
    d.gamma, d.beta, d.eps = _p(gamma), _p(beta), eps
    d.y, d.stats, d.out32, d.out16 = _p(y), _p(stats), _p(out32), _p(out16)
    d.p_post, d.seed, d.off_post, d.seed_dev = p_post, seed, off_post, _p(seed_dev)
    d.dout, d.dword, d.dpos, d.dtype_emb, d.dgamma, d.dbeta = _p(dout), _p(dword), _p(dpos), _p(dtype_emb), _p(dgamma), _p(dbeta)
    d.drows = _p(drows)
    d.out16_lo = _p(out16_lo)
    return d


def embed_text_fwd(*a, **kw):
    d = embed_text_desc(*a, **kw)
    _lib.check(_lib.lib().univl_embed_text_fwd(_BYREF(d), _stream()), "embed_text_fwd")


def embed_text_bwd(*a, **kw):
    d = embed_text_desc(*a, **kw)
    _lib.check(_lib.lib().univl_embed_text_bwd(_BYREF(d), _stream()), "embed_text_bwd")


def pool_desc(B, S, x, mask, *, skip_first, normalize, mean=None, out=None, dout=None, dx=None, ldx_row=768, accumulate=False,
              dsim=None, other=None, n_other=0, transpose=False, gscale=None):
    """dsim / other / n_other / transpose / gscale: the backward takes its upstream gradient from d loss / d sim instead of dout
    (include/univl_hip.h: UnivlPool.dsim)."""
    d = _lib.Pool()
    d.B, d.S, d.N = B, S, 768
    d.x, d.ldx_row, d.mask = _p(x), ldx_row, _p(mask)
    d.skip_first, d.normalize = int(skip_first), int(normalize)
    d.mean, d.out, d.dout, d.dx = _p(mean), _p(out), _p(dout), _p(dx)
    d.accumulate = int(accumulate)
    d.dsim, d.ldsim = _p(dsim), (dsim.stride(0) if dsim is not None else 0)
    d.other, d.n_other, d.transpose, d.gscale = _p(other), int(n_other), int(bool(transpose)), _p(gscale)
    return d


def pool_fwd(*a, **kw):
    d = pool_desc(*a, **kw)
    _lib.check(_lib.lib().univl_pool_fwd(_BYREF(d), _stream()), "pool_fwd")


def pool_bwd(*a, **kw):
    d = pool_desc(*a, **kw)
    _lib.check(_lib.lib().univl_pool_bwd(_BYREF(d), _stream()), "pool_bwd")


def pool_pair_fwd(da, db):
    _lib.check(_lib.lib().univl_pool_pair_fwd(_BYREF(da), _BYREF(db), _stream()), "pool_pair_fwd")


def pool_pair_bwd(da, db):
    _lib.check(_lib.lib().univl_pool_pair_bwd(_BYREF(da), _BYREF(db), _stream()), "pool_pair_bwd")


def maxmargin_loss(sim, margin, weight, loss, dsim):
    """sim/dsim: [n, ld] row-major views (ld = stride(0) >= n)."""
    n = sim.shape[0]
    assert dsim.stride(0) == sim.stride(0)
    _lib.check(_lib.lib().univl_maxmargin_loss(_p(sim), n, sim.stride(0), margin, _p(weight), _p(loss), _p(dsim), _stream()), "maxmargin")


def crossen_loss(sim, loss, dsim):
    assert dsim.stride(0) == sim.stride(0)
    _lib.check(_lib.lib().univl_crossen_loss(_p(sim), sim.shape[0], sim.stride(0), _p(loss), _p(dsim), _stream()), "crossen")


def milnce_loss(sim, batch_size, n_pair, loss, dsim):
    assert dsim.stride(0) == sim.stride(0)
    _lib.check(_lib.lib().univl_milnce_loss(_p(sim), batch_size, n_pair, sim.stride(0), _p(loss), _p(dsim), _stream()), "milnce")


def scale_by_device_scalar(x, s):
    _lib.check(_lib.lib().univl_scale_by_device_scalar(_p(x), x.numel(), _p(s), _stream()), "scale_by_device_scalar")


def zero_many(tensors):
    """One launch that clears up to 16 device buffers."""
    import ctypes as C
    L = _lib.lib()
    for i in range(0, len(tensors), 16):
        ts = tensors[i:i + 16]
        ptrs = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        sizes = (C.c_int64 * len(ts))(*[t.numel() * t.element_size() for t in ts])
        _lib.check(L.univl_zero_many(ptrs, sizes, len(ts), _stream()), "zero_many")


def copy_many(pairs):
    """One launch for several device-to-device copies: pairs = [(dst, src), ...], same device, contiguous, equal byte sizes."""
    import ctypes as C
    L = _lib.lib()
    for i in range(0, len(pairs), 16):
        ps = pairs[i:i + 16]
        srcs = (C.c_void_p * len(ps))(*[s.data_ptr() for _, s in ps])
        dsts = (C.c_void_p * len(ps))(*[d.data_ptr() for d, _ in ps])
        sizes = (C.c_int64 * len(ps))(*[d.numel() * d.element_size() for d, _ in ps])
        _lib.check(L.univl_copy_many(srcs, dsts, sizes, len(ps), _stream()), "copy_many")


def rows_zero(table, lst, meta):
    _lib.check(_lib.lib().univl_rows_zero(_p(table), table.shape[0], _p(lst), _p(meta), _stream()), "rows_zero")


def rows_append(ids, lst, meta, reset, ever=None):
    """ever: optional uint8 [rows] sticky "row has been written" flags (engine.FlatParams.word_ever)."""
    _lib.check(_lib.lib().univl_rows_append(_p(ids), ids.numel(), _p(lst), lst.numel(), _p(meta), int(bool(reset)), _p(ever),
                                            0 if ever is None else ever.numel(), _stream()), "rows_append")


def rows_sumsq(table, lst, meta, out):
    _lib.check(_lib.lib().univl_rows_sumsq(_p(table), table.shape[0], _p(lst), _p(meta), _p(out), _stream()), "rows_sumsq")


def embed_scatter(ids, rows, scale, dword):
    _require_gpu(ids, rows, dword)
    _lib.check(_lib.lib().univl_embed_scatter(_p(ids), _p(rows), ids.numel(), float(scale), _p(dword), _stream()), "embed_scatter")


def rows_gather_sum(rows, period, out):
    """out[s, :] += sum of rows[s::period, :] (fixed order); rows [n_rows, n] fp32, out [period, n] fp32 (a view of a table's first rows)."""
    _require_gpu(rows, out)
    _lib.check(_lib.lib().univl_rows_gather_sum(_p(rows), rows.shape[0], int(period), rows.shape[1], _p(out), _stream()), "rows_gather_sum")


def sumsq_finish(partials, seg, start, count, out):
    _lib.check(_lib.lib().univl_sumsq_finish(_p(partials), _p(seg), _p(start), _p(count), seg.numel(), _p(out), _stream()),
               "sumsq_finish")


def gather_rows(src, dst, idx, rows, row_stride_bytes, copy_bytes):
    _require_gpu(src, dst, idx)
    _lib.check(_lib.lib().univl_gather_rows(_p(src), _p(dst), _p(idx), rows, row_stride_bytes, copy_bytes, _stream()), "gather_rows")


def log_softmax_rows(x, n):
    """x: [rows, ld] fp32 (ld >= n), in place over the first n columns."""
    _require_gpu(x)
    _lib.check(_lib.lib().univl_log_softmax_rows(_p(x), x.shape[0], n, x.stride(0), _stream()), "log_softmax_rows")


def beam_ws(n_inst, n_bm, device):
    """Scratch of univl_beam_step for n_inst x n_bm beams (include/univl_hip.h: UnivlBeamStep.ws)."""
    return torch.empty(n_inst * n_bm * _lib.BEAM_SLICES * n_bm * 2, dtype=torch.float32, device=device)


def _beam_common(d, n_units, lp, V, n_inst, n_bm, t, scores, done, length, tokens, src, hist_parents, hist_tokens, hist_scores, ws, eos,
                 eos_dev, first_step):
    """The part of a beam step descriptor that UnivlBeamStep, UnivlBeamGroupStep and UnivlBeamPoolStep share: checks the shapes and
    dtypes of the common arguments (the builders' own, in their order) and fills d's common fields.  n_units: the entries of done /
    length (n_inst, or n_inst * n_groups).  Shapes and dtypes are looked at before the device, so a wrong argument is an
    AssertionError wherever the tensors live.  Returns d."""
    R = n_inst * n_bm
    assert lp.dtype == torch.float32 and lp.dim() == 2 and lp.stride(1) == 1 and lp.shape[0] >= R
    assert scores.dtype == torch.float32 and scores.numel() == R and scores.is_contiguous()
    assert done.dtype in (torch.uint8, torch.bool) and done.numel() == n_units and done.is_contiguous()
    assert length.dtype == torch.int32 and length.numel() == n_units and length.is_contiguous()
    assert tokens.dtype == torch.int64 and tokens.numel() == R and src.dtype == torch.int32 and src.numel() == R
    Tmax = hist_parents.shape[0]
    for h, dt_ in ((hist_parents, torch.int32), (hist_tokens, torch.int32), (hist_scores, torch.float32)):
        assert h.dtype == dt_ and h.is_contiguous() and h.shape[0] == Tmax and h.numel() == Tmax * R
    assert eos_dev is None or eos_dev.dtype == torch.int32
    _require_gpu(lp, scores, done, length, tokens, src, hist_parents, hist_tokens, hist_scores, ws, eos_dev)
    d.lp, d.ld, d.n_inst, d.n_bm, d.V = _p(lp), lp.stride(0), n_inst, n_bm, V
    d.first_step, d.eos, d.eos_dev, d.t, d.Tmax = int(t == 0 if first_step is None else first_step), int(eos), _p(eos_dev), t, Tmax
    d.scores, d.done, d.length, d.tokens, d.src = _p(scores), _p(done), _p(length), _p(tokens), _p(src)
    d.hist_parents, d.hist_tokens, d.hist_scores = _p(hist_parents), _p(hist_tokens), _p(hist_scores)
    d.ws, d.ws_bytes = _p(ws), ws.numel() * ws.element_size()
    return d


def beam_step_desc(lp, V, n_inst, n_bm, t, *, scores, done, length, tokens, src, hist_parents, hist_tokens, hist_scores, ws, eos=-1,
                   eos_dev=None, first_step=None):
    """lp: [n_inst * n_bm, ld] fp32 view (row stride ld >= V); state / outputs as in include/univl_hip.h: UnivlBeamStep.  first_step
    defaults to t == 0.  Shapes and dtypes are checked here; the argument RANGE is the library's to refuse."""
    return _beam_common(_lib.BeamStep(), n_inst, lp, V, n_inst, n_bm, t, scores, done, length, tokens, src, hist_parents, hist_tokens,
                        hist_scores, ws, eos, eos_dev, first_step)


def beam_step(*a, **kw):
    d = beam_step_desc(*a, **kw)
    _lib.check(_lib.lib().univl_beam_step(_BYREF(d), _stream()), "beam_step")


def beam_group_step_desc(lp, V, n_inst, n_bm, n_groups, t, *, scores, done, length, tokens, src, hist_parents, hist_tokens, hist_scores, ws,
                         diversity=0.0, diversity_dev=None, eos=-1, eos_dev=None, first_step=None):
    """beam_step_desc for n_groups groups of n_bm // n_groups beams (include/univl_hip.h: UnivlBeamGroupStep): done and length have
    n_inst * n_groups entries, one per (instance, group); diversity_dev: fp32 device word read instead of diversity.  ws: beam_ws(n_inst,
    n_bm).  Shapes and dtypes are checked here; the argument RANGE is the library's to refuse."""
    d = _beam_common(_lib.BeamGroupStep(), n_inst * n_groups, lp, V, n_inst, n_bm, t, scores, done, length, tokens, src, hist_parents,
                     hist_tokens, hist_scores, ws, eos, eos_dev, first_step)
    assert diversity_dev is None or (diversity_dev.dtype == torch.float32 and diversity_dev.numel() == 1)
    _require_gpu(diversity_dev)
    d.n_groups, d.diversity, d.diversity_dev = int(n_groups), float(diversity), _p(diversity_dev)
    return d


def beam_group_step(*a, **kw):
    d = beam_group_step_desc(*a, **kw)
    _lib.check(_lib.lib().univl_beam_group_step(_BYREF(d), _stream()), "beam_group_step")


def length_weights(alpha, Tmax):
    """The length-weight table of univl_beam_pool_step as a CPU fp32 tensor of Tmax + 2 entries: w[L] = float32(float64(L) ** -alpha),
    w[0] = 1.  alpha: a finite number >= 0 (ValueError otherwise; bool is refused)."""
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not math.isfinite(alpha) or alpha < 0:
        raise ValueError("length_penalty=%r, expected a finite number >= 0" % (alpha,))
    w = np.ones(Tmax + 2, dtype=np.float64)
    w[1:] = np.arange(1, Tmax + 2, dtype=np.float64) ** -float(alpha)
    return torch.from_numpy(w.astype(np.float32))


def beam_pool(n_inst, n_bm, device):
    """The pool arrays of univl_beam_pool_step for n_inst x n_bm beams, empty: a dict of the descriptor builder's pool arguments."""
    z = lambda dt: torch.zeros(n_inst, n_bm, dtype=dt, device=device)
    return dict(pool_key=z(torch.float32), pool_raw=z(torch.float32), pool_end_t=z(torch.int32), pool_beam=z(torch.int32),
                pool_finished=z(torch.uint8), pool_count=torch.zeros(n_inst, dtype=torch.int32, device=device))


def beam_pool_step_desc(lp, V, n_inst, n_bm, t, *, scores, done, length, tokens, src, hist_parents, hist_tokens, hist_scores, ws, w, params,
                        pool_key, pool_raw, pool_end_t, pool_beam, pool_finished, pool_count, eos=-1, eos_dev=None, first_step=None):
    """beam_step_desc for the pooled search (include/univl_hip.h: UnivlBeamPoolStep).  w: fp32 [Tmax + 2] device table
    (length_weights); params: int32 [2] device words {early_stopping, Lmax}; pool_*: [n_inst, n_bm] (beam_pool).  Shapes and dtypes
    are checked here; the argument RANGE is the library's to refuse."""
    d = _beam_common(_lib.BeamPoolStep(), n_inst, lp, V, n_inst, n_bm, t, scores, done, length, tokens, src, hist_parents, hist_tokens,
                     hist_scores, ws, eos, eos_dev, first_step)
    assert w.dtype == torch.float32 and w.numel() == d.Tmax + 2 and w.is_contiguous()
    assert params.dtype == torch.int32 and params.numel() == 2 and params.is_contiguous()
    for h, dt_ in ((pool_key, torch.float32), (pool_raw, torch.float32), (pool_end_t, torch.int32), (pool_beam, torch.int32),
                   (pool_finished, torch.uint8)):
        assert h.dtype == dt_ and h.numel() == n_inst * n_bm and h.is_contiguous()
    assert pool_count.dtype == torch.int32 and pool_count.numel() == n_inst and pool_count.is_contiguous()
    _require_gpu(w, params, pool_key, pool_raw, pool_end_t, pool_beam, pool_finished, pool_count)
    d.w, d.params = _p(w), _p(params)
    d.pool_key, d.pool_raw, d.pool_end_t, d.pool_beam = _p(pool_key), _p(pool_raw), _p(pool_end_t), _p(pool_beam)
    d.pool_finished, d.pool_count = _p(pool_finished), _p(pool_count)
    return d


def beam_pool_step(*a, **kw):
    d = beam_pool_step_desc(*a, **kw)
    _lib.check(_lib.lib().univl_beam_pool_step(_BYREF(d), _stream()), "beam_pool_step")


def beam_pool_finish(desc, n_best):
    """univl_beam_pool_finish on a descriptor of beam_pool_step_desc (its lp, ws and t are not looked at).  Returns (hyp [n, n_best,
    Tmax] int32, -1 padded; raw [n, n_best] fp32; key [n, n_best] fp32; len [n, n_best] int32; finished [n, n_best] uint8)."""
    n, Tmax, dev = desc.n_inst, desc.Tmax, torch.device("cuda", torch.cuda.current_device())
    n_best = int(n_best)
    hyp = torch.empty(n, max(n_best, 1), Tmax, dtype=torch.int32, device=dev)
    raw, key = (torch.empty(n, max(n_best, 1), dtype=torch.float32, device=dev) for _ in range(2))
    ln = torch.empty(n, max(n_best, 1), dtype=torch.int32, device=dev)
    fin = torch.empty(n, max(n_best, 1), dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().univl_beam_pool_finish(_BYREF(desc), n_best, _p(hyp), _p(raw), _p(key), _p(ln), _p(fin), _stream()),
               "beam_pool_finish")
    return hyp, raw, key, ln, fin


def sample_ws(R, k, device):
    """Scratch of univl_sample_step for R rows and a top-k of k (include/univl_hip.h: UnivlSampleStep.ws)."""
    return torch.empty(R * _lib.SAMPLE_SLICES * (2 * k + 4), dtype=torch.float32, device=device)


def sample_step_desc(x, V, k, t, *, done, length, ids, tokens_out, tok_logprob, q_logprob, seq_logprob, seq_q_logprob, ws, inv_T=1.0,
                     top_p=1.0, seed=0, eos=-1, sampling_dev=None, seed_dev=None, eos_dev=None, topk_idx=None, topk_val=None):
    """x: [R, ld] fp32 view of raw logits (row stride ld >= V); state / outputs as in include/univl_hip.h: UnivlSampleStep.
    sampling_dev: fp32 [2] device {inv_T, top_p}; seed_dev: one 64-bit device word (int64 storage, read as uint64); eos_dev: int32
    device word -- each read instead of the scalar.  Shapes and dtypes are checked here; the argument RANGE is the library's to refuse."""
    _require_gpu(x, done, length, ids, tokens_out, tok_logprob, q_logprob, seq_logprob, seq_q_logprob, ws, sampling_dev, seed_dev,
                 eos_dev, topk_idx, topk_val)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    R = x.shape[0]
    assert done.dtype in (torch.uint8, torch.bool) and done.numel() == R and length.dtype == torch.int32 and length.numel() == R
    assert ids.dtype == torch.int64 and ids.numel() == R
    Tmax = tokens_out.shape[1]
    for h, dt_ in ((tokens_out, torch.int32), (tok_logprob, torch.float32), (q_logprob, torch.float32)):
        assert h.dtype == dt_ and h.is_contiguous() and h.shape == (R, Tmax)
    for h in (seq_logprob, seq_q_logprob):
        assert h.dtype == torch.float32 and h.numel() == R and h.is_contiguous()
    assert sampling_dev is None or (sampling_dev.dtype == torch.float32 and sampling_dev.numel() == 2)
    assert seed_dev is None or (seed_dev.dtype == torch.int64 and seed_dev.numel() == 1)
    assert eos_dev is None or eos_dev.dtype == torch.int32
    assert topk_idx is None or (topk_idx.dtype == torch.int32 and topk_idx.is_contiguous() and topk_idx.shape == (R, k))
    assert topk_val is None or (topk_val.dtype == torch.float32 and topk_val.is_contiguous() and topk_val.shape == (R, k))
    d = _lib.SampleStep()
    d.x, d.ld, d.R, d.V, d.k, d.t, d.Tmax, d.eos = _p(x), x.stride(0), R, V, k, t, Tmax, int(eos)
    d.inv_T, d.top_p, d.seed = inv_T, top_p, int(seed) & 0xFFFFFFFFFFFFFFFF
    d.sampling_dev, d.seed_dev, d.eos_dev = _p(sampling_dev), _p(seed_dev), _p(eos_dev)
    d.done, d.length, d.ids = _p(done), _p(length), _p(ids)
    d.tokens_out, d.tok_logprob, d.q_logprob = _p(tokens_out), _p(tok_logprob), _p(q_logprob)
    d.seq_logprob, d.seq_q_logprob, d.topk_idx, d.topk_val = _p(seq_logprob), _p(seq_q_logprob), _p(topk_idx), _p(topk_val)
    d.ws, d.ws_bytes = _p(ws), ws.numel() * ws.element_size()
    return d


def sample_step(*a, **kw):
    d = sample_step_desc(*a, **kw)
    _lib.check(_lib.lib().univl_sample_step(_BYREF(d), _stream()), "sample_step")


def decode_constrain_desc(x, V, t, *, prefix_in=None, prefix_out=None, src=None, last=None, done=None, done_stride=1, ngram=0, min_len=0,
                          eos=-1, eos_dev=None, params_dev=None, suppress=None, Tmax=None):
    """x: [R, ld] fp32 view of one position's score rows (row stride ld >= V), edited in place; the rest as in include/univl_hip.h:
    UnivlDecodeConstrain.  prefix_in / prefix_out: [R, Tmax] int32; src: int32 [R]; last: int64 [R]; done: uint8 [ceil(R / done_stride)];
    params_dev: int32 [2] device {ngram, min_len}; eos_dev: int32 device word; suppress: int32 device ids (None: an empty list).  Tmax
    is taken from the prefix arrays (give it when there are none).  Shapes and dtypes are checked here; the argument RANGE is the
    library's to refuse."""
    _require_gpu(x, prefix_in, prefix_out, src, last, done, eos_dev, params_dev, suppress)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    R = x.shape[0]
    for h in (prefix_in, prefix_out):
        if h is not None:
            assert h.dtype == torch.int32 and h.dim() == 2 and h.is_contiguous() and h.shape[0] == R
            assert Tmax is None or Tmax == h.shape[1]
            Tmax = h.shape[1]
    assert Tmax is not None, "decode_constrain: Tmax is needed without prefix arrays"
    assert src is None or (src.dtype == torch.int32 and src.numel() == R and src.is_contiguous())
    assert last is None or (last.dtype == torch.int64 and last.numel() == R and last.is_contiguous())
    assert done is None or (done.dtype in (torch.uint8, torch.bool) and done_stride >= 1 and done.numel() * done_stride >= R)
    assert eos_dev is None or eos_dev.dtype == torch.int32
    assert params_dev is None or (params_dev.dtype == torch.int32 and params_dev.numel() == 2 and params_dev.is_contiguous())
    assert suppress is None or (suppress.dtype == torch.int32 and suppress.dim() == 1 and suppress.is_contiguous())
    d = _lib.DecodeConstrain()
    d.x, d.ld, d.R, d.V, d.t, d.Tmax = _p(x), x.stride(0), R, V, t, Tmax
    d.prefix_in, d.prefix_out, d.src, d.last = _p(prefix_in), _p(prefix_out), _p(src), _p(last)
    d.done, d.done_stride, d.ngram, d.min_len, d.eos = _p(done), int(done_stride), int(ngram), int(min_len), int(eos)
    d.eos_dev, d.params_dev = _p(eos_dev), _p(params_dev)
    d.suppress, d.n_suppress = (_p(suppress), suppress.numel()) if suppress is not None and suppress.numel() else (None, 0)
    return d


def decode_constrain(*a, **kw):
    d = decode_constrain_desc(*a, **kw)
    _lib.check(_lib.lib().univl_decode_constrain(_BYREF(d), _stream()), "decode_constrain")


def caption_overlap(sym, length, hyp_row, ref_begin, ref_rows, n_refs, *, tables=None, bleu=False, status=None):
    """N-gram overlap statistics per item (include/univl_hip.h: univl_caption_overlap), one launch, nothing read on the host.
    sym: [rows, T] int32 (row stride >= T), length: [rows] int32; hyp_row [items], ref_begin [items + 1], ref_rows [n_refs] int32 device
    tensors; n_refs: the HOST's statement of ref_begin[items].  tables: None, or (df_keys int64 storage of the uint64 keys, df_cnt int32,
    df_begin: five host ints, n_docs) -- then CIDEr is computed.  bleu: also the sentence BLEU-4 of every item.  status: an int32 device
    word the flags are OR-ed into (default: a fresh zero).  Returns a dict of device tensors: guess / correct [items, 4] int32, hyp_len /
    ref_len [items] int32, lcs [n_refs] int32, rouge_l [items] fp64, cider / bleu [items] fp64 or None, status [1] int32."""
    _require_gpu(sym, length, hyp_row, ref_begin, ref_rows, status)
    assert sym.dtype == torch.int32 and sym.dim() == 2 and sym.stride(1) == 1
    rows, T = sym.shape
    items, dev = hyp_row.numel(), sym.device
    for h, n in ((length, rows), (hyp_row, items), (ref_begin, items + 1), (ref_rows, int(n_refs))):
        assert h.dtype == torch.int32 and h.is_contiguous() and h.numel() == n
    d = _lib.CaptionOverlap()
    d.sym, d.ld, d.len, d.rows, d.T, d.items, d.n_refs = _p(sym), sym.stride(0), _p(length), rows, T, items, int(n_refs)
    d.hyp_row, d.ref_begin, d.ref_rows = _p(hyp_row), _p(ref_begin), _p(ref_rows)
    out = dict(guess=torch.empty(items, 4, dtype=torch.int32, device=dev), correct=torch.empty(items, 4, dtype=torch.int32, device=dev),
               hyp_len=torch.empty(items, dtype=torch.int32, device=dev), ref_len=torch.empty(items, dtype=torch.int32, device=dev),
               lcs=torch.zeros(int(n_refs), dtype=torch.int32, device=dev), rouge_l=torch.empty(items, dtype=torch.float64, device=dev),
               cider=None, bleu=torch.empty(items, dtype=torch.float64, device=dev) if bleu else None,
               status=_status_word(status, dev))
    if tables is not None:
        df_keys, df_cnt, df_begin, n_docs = tables
        _require_gpu(df_keys, df_cnt)
        assert len(df_begin) == 5 and df_keys.dtype == torch.int64 and df_cnt.dtype == torch.int32
        assert df_keys.is_contiguous() and df_cnt.is_contiguous() and df_keys.numel() == df_cnt.numel() == int(df_begin[4])
        d.df_keys, d.df_cnt, d.n_docs = _p(df_keys), _p(df_cnt), int(n_docs)
        for n in range(5):
            d.df_begin[n] = int(df_begin[n])
        out["cider"] = torch.empty(items, dtype=torch.float64, device=dev)
    d.guess, d.correct, d.hyp_len, d.ref_len, d.lcs = (_p(out[k]) for k in ("guess", "correct", "hyp_len", "ref_len", "lcs"))
    d.rouge_l, d.cider, d.bleu, d.status = _p(out["rouge_l"]), _p(out["cider"]), _p(out["bleu"]), _p(out["status"])
    _lib.check(_lib.lib().univl_caption_overlap(_BYREF(d), _stream()), "caption_overlap")
    return out


def ngram_df(sym, length, ref_begin, ref_rows, n_refs, *, capacity=None, status=None):
    """The document-frequency tables of caption_overlap(tables=...) from token rows (include/univl_hip.h: univl_ngram_df); nothing is
    read on the host.  sym: [rows, T] int32 (row stride >= T), length: [rows] int32; document i = rows ref_rows[ref_begin[i] ..
    ref_begin[i + 1]); ref_begin [items + 1], ref_rows [n_refs] int32 device tensors; n_refs: the HOST's statement of ref_begin[items].
    capacity: the length of the returned arrays (default n_refs * 4 T, which always suffices).  status: an int32 device word the flags
    are OR-ed into (default: a fresh zero).  Returns (df_keys [capacity] int64 storage of the uint64 keys, df_cnt [capacity] int32,
    df_begin [5] int32 ON THE DEVICE, status [1] int32); entries at and past df_begin[4] are not written."""
    _require_gpu(sym, length, ref_begin, ref_rows, status)
    assert sym.dtype == torch.int32 and sym.dim() == 2 and sym.stride(1) == 1
    rows, T = sym.shape
    items, dev, n_refs = ref_begin.numel() - 1, sym.device, int(n_refs)
    for h, n in ((length, rows), (ref_begin, items + 1), (ref_rows, n_refs)):
        assert h.dtype == torch.int32 and h.is_contiguous() and h.numel() == n
    if capacity is None:
        capacity = n_refs * 4 * T
    df_keys = torch.empty(max(int(capacity), 0), dtype=torch.int64, device=dev)
    df_cnt = torch.empty(max(int(capacity), 0), dtype=torch.int32, device=dev)
    df_begin = torch.empty(5, dtype=torch.int32, device=dev)
    status = _status_word(status, dev)
    d = _lib.NgramDf()
    d.sym, d.ld, d.len, d.rows, d.T, d.items, d.n_refs = _p(sym), sym.stride(0), _p(length), rows, T, items, n_refs
    d.ref_begin, d.ref_rows = _p(ref_begin), _p(ref_rows)
    d.df_keys, d.df_cnt, d.df_begin, d.status, d.capacity = _p(df_keys), _p(df_cnt), _p(df_begin), _p(status), int(capacity)
    _workspace(d, _lib.lib().univl_ngram_df_ws_bytes(n_refs, T), dev)
    _lib.check(_lib.lib().univl_ngram_df(_BYREF(d), _stream()), "ngram_df")      # refuses what the workspace query refused, with its message
    return df_keys, df_cnt, df_begin, status


def consensus_pick(score):
    """score: [n_inst, n_samp] fp64 device tensor -> (pick [n_inst] int32, best [n_inst] fp64): the arg-max of every row, equal scores
    to the lower index (include/univl_hip.h: univl_consensus_pick)."""
    _require_gpu(score)
    assert score.dtype == torch.float64 and score.dim() == 2 and score.is_contiguous()
    n, ns = score.shape
    pick = torch.empty(n, dtype=torch.int32, device=score.device)
    best = torch.empty(n, dtype=torch.float64, device=score.device)
    _lib.check(_lib.lib().univl_consensus_pick(_p(score), n, ns, _p(pick), _p(best), _stream()), "consensus_pick")
    return pick, best


def caption_advantage(reward, baseline=None, scale=1.0, status=None):
    """reward: [n, ns] fp64 device tensor -> (weight [n, ns] fp32, status [1] int32), include/univl_hip.h: univl_caption_advantage.
    baseline None: the leave-one-out mean of the video's other samples (ns >= 2); else [n] fp64 on the device.  status: an int32 device
    word the non-finite flag is OR-ed into (default: a fresh zero).  Nothing is read on the host."""
    _require_gpu(reward, baseline, status)
    assert reward.dtype == torch.float64 and reward.dim() == 2 and reward.is_contiguous()
    n, ns = reward.shape
    assert baseline is None or (baseline.dtype == torch.float64 and baseline.is_contiguous() and baseline.numel() == n)
    weight = torch.empty(n, ns, dtype=torch.float32, device=reward.device)
    status = _status_word(status, reward.device)
    _lib.check(_lib.lib().univl_caption_advantage(_p(reward), _p(baseline), n, ns, _lib.ADV_LOO if baseline is None else _lib.ADV_GIVEN,
                                                  float(scale), _p(weight), _p(status), _stream()), "caption_advantage")
    return weight, status


def beam_backtrack(hist_parents, hist_tokens, scores, length, n_best):
    """Walk the n_best best beams of every instance back through the history (include/univl_hip.h: univl_beam_backtrack).
    Returns (hyp [n, n_best, Tmax] int32, -1 padded; hyp_scores [n, n_best] fp32)."""
    _require_gpu(hist_parents, hist_tokens, scores, length)
    Tmax, n, n_bm = hist_parents.shape
    assert hist_parents.dtype == torch.int32 and hist_tokens.dtype == torch.int32 and hist_tokens.shape == hist_parents.shape
    assert hist_parents.is_contiguous() and hist_tokens.is_contiguous() and scores.is_contiguous()
    assert scores.dtype == torch.float32 and scores.shape == (n, n_bm) and length.dtype == torch.int32 and length.numel() == n
    hyp = torch.empty(n, n_best, Tmax, dtype=torch.int32, device=scores.device)
    hs = torch.empty(n, n_best, dtype=torch.float32, device=scores.device)
    _lib.check(_lib.lib().univl_beam_backtrack(_p(hist_parents), _p(hist_tokens), _p(scores), _p(length), n, n_bm, int(n_best), Tmax,
                                               _p(hyp), _p(hs), _stream()), "beam_backtrack")
    return hyp, hs


def beam_captions(hyp, length, eos, pad, *, eos_dev=None, out=None):
    """The reference's caption cut on the device (include/univl_hip.h: univl_beam_captions).  hyp: [n, n_best, Tmax] int32 as
    beam_backtrack returns it, length: [n] int32; eos / pad: token ids, negative for none; eos_dev: optional int32 device word read
    instead of eos; out: the cap_tokens buffer (hyp itself for the cut in place; default a new tensor).
    Returns (cap_tokens [n, n_best, Tmax] int32, -1 past the cut; cap_len [n, n_best] int32)."""
    _require_gpu(hyp, length, eos_dev, out)
    assert hyp.dtype == torch.int32 and hyp.dim() == 3 and hyp.is_contiguous()
    n, n_best, Tmax = hyp.shape
    assert length.dtype == torch.int32 and length.numel() == n and length.is_contiguous()
    assert eos_dev is None or eos_dev.dtype == torch.int32
    cap = torch.empty_like(hyp) if out is None else out
    assert cap.dtype == torch.int32 and cap.shape == hyp.shape and cap.is_contiguous()
    cap_len = torch.empty(n, n_best, dtype=torch.int32, device=hyp.device)
    _lib.check(_lib.lib().univl_beam_captions(_p(hyp), _p(length), n, n_best, Tmax, int(eos), int(pad), _p(eos_dev), _p(cap), _p(cap_len),
                                              _stream()), "beam_captions")
    return cap, cap_len


def rank_counts(sim):
    """sim: [n, n] fp32 device tensor (row stride >= n).  Returns (gt, eq) int32 [n]."""
    _require_gpu(sim)
    n = sim.shape[0]
    assert sim.shape[1] == n and sim.dtype == torch.float32 and sim.stride(1) == 1
    gt = torch.empty(n, dtype=torch.int32, device=sim.device)
    eq = torch.empty(n, dtype=torch.int32, device=sim.device)
    _lib.check(_lib.lib().univl_rank_counts(_p(sim), n, sim.stride(0), _p(gt), _p(eq), _stream()), "rank_counts")
    return gt, eq


def sim_topk(q, g, k, *, target=None, slices=0):
    """The k best rows of g for every row of q by inner product, without the [Nq, Ng] matrix (include/univl_hip.h: univl_sim_topk).
    q: [Nq, 768], g: [Ng, 768] fp32 row-major views (row stride >= 768, rows 16-byte aligned); 0 <= k <= TOPK_MAX; target: optional
    [Nq] int32 gallery rows; slices: 0 = the library chooses.  Returns (scores [Nq, k] fp32 descending, indices [Nq, k] int32; equal
    scores by lower index first, -inf / -1 past the gallery's end), followed by (gt, eq) int32 [Nq] -- the rank counts against
    target -- when target is given.  k = 0: only (gt, eq)."""
    return _sim_topk(_lib.SimTopk(), "sim_topk", q, g, k, target, slices)


def _sim_topk(d, what, q, g, k, target, slices):
    """sim_topk and sim_topk_norm: d is the descriptor (SimTopk's fields; the caller has set the ones past them), what the entry point."""
    _require_gpu(q, g, target)
    _row_views(q, g)
    d.q, d.ldq, d.g, d.ldg = _p(q), _ld(q), _p(g), _ld(g)
    d.Nq, d.Ng, d.H, d.k, d.slices = q.shape[0], g.shape[0], q.shape[1], int(k), int(slices)
    if g.shape[1] != q.shape[1]:
        raise RuntimeError("%s: q is %d wide, g %d" % (what, q.shape[1], g.shape[1]))
    dev = q.device
    _workspace(d, _lib.lib().univl_sim_topk_workspace(d.Nq, d.Ng, d.k, d.slices), dev)
    idx = score = gt = eq = None
    if d.k > 0:
        idx = torch.empty(d.Nq, d.k, dtype=torch.int32, device=dev)
        score = torch.empty(d.Nq, d.k, dtype=torch.float32, device=dev)
        d.idx, d.score = _p(idx), _p(score)
    if target is not None:
        assert target.dtype == torch.int32 and target.numel() == d.Nq and target.is_contiguous()
        gt = torch.empty(d.Nq, dtype=torch.int32, device=dev)
        eq = torch.empty(d.Nq, dtype=torch.int32, device=dev)
        d.target, d.gt, d.eq = _p(target), _p(gt), _p(eq)
    _lib.check(getattr(_lib.lib(), "univl_" + what)(_BYREF(d), _stream()), what)     # refuses what the workspace query refused, with its message
    if d.k == 0:
        return gt, eq
    return (score, idx) if target is None else (score, idx, gt, eq)


def sim_topk_norm(q, g, k, col_bias, *, row_gate=None, target=None, slices=0):
    """sim_topk on the query-bank normalised score s'(i, j) = s(i, j) - col_bias[j] where row_gate[i] != 0 (everywhere when row_gate
    is None), s(i, j) untouched where it is 0 (include/univl_hip.h: univl_sim_topk_norm).  col_bias: [Ng] fp32 (sim_colstat), row_gate:
    optional [Nq] int32 (hub_gate).  Arguments and results otherwise as sim_topk's; the scores returned are s'."""
    _require_gpu(col_bias, row_gate)
    assert col_bias.dtype == torch.float32 and col_bias.numel() == g.shape[0] and col_bias.is_contiguous()
    assert row_gate is None or (row_gate.dtype == torch.int32 and row_gate.numel() == q.shape[0] and row_gate.is_contiguous())
    d = _lib.SimTopkNorm()
    d.col_bias, d.row_gate = _p(col_bias), _p(row_gate)
    return _sim_topk(d, "sim_topk_norm", q, g, k, target, slices)


def sim_colstat(bank, g, beta=20.0, *, out=None):
    """The column term of query-bank normalisation, c[j] = log-sum-exp over the bank rows b of beta * s(b, j), divided by beta, without
    the [Nb, Ng] matrix (include/univl_hip.h: univl_sim_colstat).  bank: [Nb, 768], g: [Ng, 768] fp32 row-major views as sim_topk's;
    beta: finite, > 0; out: optional [Ng] fp32 to write.  Returns c [Ng] fp32."""
    _require_gpu(bank, g, out)
    _row_views(bank, g)
    if g.shape[1] != bank.shape[1]:
        raise RuntimeError("sim_colstat: bank is %d wide, g %d" % (bank.shape[1], g.shape[1]))
    d = _lib.SimColstat()
    d.bank, d.ldb, d.g, d.ldg = _p(bank), _ld(bank), _p(g), _ld(g)
    d.Nb, d.Ng, d.H, d.beta = bank.shape[0], g.shape[0], bank.shape[1], float(beta)
    c = torch.empty(d.Ng, dtype=torch.float32, device=g.device) if out is None else out
    assert c.dtype == torch.float32 and c.numel() == d.Ng and c.is_contiguous()
    d.c = _p(c)
    _workspace(d, _lib.lib().univl_sim_colstat_workspace(d.Nb, d.Ng), g.device)
    _lib.check(_lib.lib().univl_sim_colstat(_BYREF(d), _stream()), "sim_colstat")
    return c


def hub_flags(idx, Ng, *, out=None):
    """hub[j] = 1 for every gallery row j that idx names (int32, any shape: the bank rows' best lists from sim_topk; -1 is skipped).
    out: an [Ng] int32 set to add to; default a new one, zeroed.  Returns hub [Ng] int32."""
    _require_gpu(idx, out)
    assert idx.dtype == torch.int32 and idx.is_contiguous()
    hub = torch.zeros(int(Ng), dtype=torch.int32, device=idx.device) if out is None else out
    assert hub.dtype == torch.int32 and hub.numel() == int(Ng) and hub.is_contiguous()
    _lib.check(_lib.lib().univl_hub_flags(_p(idx), idx.numel(), int(Ng), _p(hub), _stream()), "hub_flags")
    return hub


def hub_gate(top1, hub):
    """gate[i] = 1 where hub[top1[i]] is set.  top1: [Nq] int32, or sim_topk's [Nq, k] indices, whose first column is taken in place;
    hub: [Ng] int32 (hub_flags).  Returns gate [Nq] int32, the row_gate of sim_topk_norm."""
    _require_gpu(top1, hub)
    assert top1.dtype == torch.int32 and hub.dtype == torch.int32 and hub.is_contiguous() and top1.dim() in (1, 2)
    ld = top1.stride(0) if top1.shape[0] > 1 else 1
    gate = torch.empty(top1.shape[0], dtype=torch.int32, device=top1.device)
    _lib.check(_lib.lib().univl_hub_gate(_p(top1), ld, top1.shape[0], _p(hub), hub.numel(), _p(gate), _stream()), "hub_gate")
    return gate


def _moment_gallery(frames, mask, normalize, desc=_lib.Moment):
    """The gallery side of a Moment, StepAlign or FrameSegment descriptor (window_norms, moment_localize, step_align, frame_segment)."""
    _require_gpu(frames, mask)
    assert frames.dtype == torch.float32 and frames.dim() == 3 and frames.stride(2) == 1 and frames.stride(1) == frames.shape[2]
    assert mask.dtype == torch.int64 and mask.shape == frames.shape[:2] and mask.is_contiguous()
    d = desc()
    d.N, d.F, d.H, d.normalize = frames.shape[0], frames.shape[1], frames.shape[2], 1 if normalize else 0
    d.frames, d.ld_row, d.mask = _p(frames), frames.stride(0) if d.N > 1 else d.F * d.H, _p(mask)     # one row: its stride means nothing
    return d


def window_norms(frames, mask, *, out=None):
    """|u(s, L)| of every window of every gallery row, u the sum of frames s .. s + L - 1 (include/univl_hip.h: univl_window_norms).
    frames: [N, F, 768] fp32 (frames contiguous, rows 16-byte aligned), F <= MOMENT_F_MAX; mask: [N, F] int64, 0 = not a frame; out:
    optional [N, F, F] fp32 to write.  Returns the table [N, F, F] fp32 indexed (s, L - 1): 0 where the window holds a masked frame
    or runs past the row's end.  It depends on the videos alone: compute it once per row, for models that normalise."""
    d = _moment_gallery(frames, mask, True)
    t = torch.empty(d.N, d.F, d.F, dtype=torch.float32, device=frames.device) if out is None else out
    _require_gpu(t)
    assert t.dtype == torch.float32 and t.shape == (d.N, d.F, d.F) and t.is_contiguous()
    d.wnorm = _p(t)
    _lib.check(_lib.lib().univl_window_norms(_BYREF(d), _stream()), "window_norms")
    return t


def _moment_table(who, d, wnorm, normalize):
    """d.wnorm of a localiser: the table window_norms made of the same gallery, which a normalising model needs."""
    if normalize:
        if wnorm is None:
            raise RuntimeError("%s: normalize=True needs wnorm (window_norms)" % who)
        assert wnorm.dtype == torch.float32 and wnorm.shape == (d.N, d.F, d.F) and wnorm.is_contiguous()
        d.wnorm = _p(wnorm)


def moment_localize(q, frames, mask, rows, lmin, lmax, *, wnorm=None, normalize=True):
    """The best window of frames of gallery row rows[i, j] for query row i, every window scored in one launch (include/univl_hip.h:
    univl_moment_localize).  q: [Nq, 768] fp32 row-major view (row stride >= 768, rows 16-byte aligned); frames, mask: as
    window_norms'; rows: [Nq, K] int32 contiguous gallery rows (sim_topk's indices, say); 1 <= lmin <= lmax <= F: the window lengths
    searched; wnorm: window_norms' table of the same gallery, needed when normalize; normalize: False for use_mil models (the score
    is then the mean's inner product).  Returns (start, length, score), [Nq, K] int32, int32, fp32: the window with the largest score,
    equal scores by lower start, then by smaller length; (-1, 0, -inf) where no window lies inside the valid frames or the row id is
    outside the gallery (the -1 of sim_topk)."""
    d = _moment_gallery(frames, mask, normalize)
    _require_gpu(q, rows, wnorm)
    _row_views(q)
    assert rows.dtype == torch.int32 and rows.dim() == 2 and rows.shape[0] == q.shape[0] and rows.is_contiguous()
    if q.shape[1] != frames.shape[2]:
        raise RuntimeError("moment_localize: q is %d wide, the frames %d" % (q.shape[1], frames.shape[2]))
    _moment_table("moment_localize", d, wnorm, normalize)
    d.q, d.ldq, d.rows, d.Nq, d.K, d.lmin, d.lmax = _p(q), _ld(q), _p(rows), rows.shape[0], rows.shape[1], int(lmin), int(lmax)
    start = torch.empty(d.Nq, d.K, dtype=torch.int32, device=q.device)
    length = torch.empty(d.Nq, d.K, dtype=torch.int32, device=q.device)
    score = torch.empty(d.Nq, d.K, dtype=torch.float32, device=q.device)
    d.start, d.length, d.score = _p(start), _p(length), _p(score)
    _lib.check(_lib.lib().univl_moment_localize(_BYREF(d), _stream()), "moment_localize")
    return start, length, score


def moment_nbest(q, frames, mask, rows, lmin, lmax, n_best, nms=(1, 2), *, wnorm=None, normalize=True):
    """The n_best windows of gallery row rows[i, j] for query row i after greedy temporal non-maximum suppression, in one launch
    (include/univl_hip.h: univl_moment_nbest).  Arguments as moment_localize's; 1 <= n_best <= MOMENT_NBEST_MAX; nms = (num, den),
    integers with 1 <= den <= 1024 and 0 <= num <= den: a window dies when its temporal IoU with a pick exceeds num / den, decided
    in integers (den * inter > num * union).  (1, 1) is the plain top n_best, (0, 1) gives disjoint windows.  Returns (start, length,
    score), [Nq, K, n_best] int32, int32, fp32: slot 0 is moment_localize's triple bit for bit, the scores of a pair never increase
    from slot to slot, and the slots past the last surviving window -- all of them for a row id outside the gallery -- are
    (-1, 0, -inf)."""
    d = _moment_gallery(frames, mask, normalize, _lib.MomentNbest)
    _require_gpu(q, rows, wnorm)
    _row_views(q)
    assert rows.dtype == torch.int32 and rows.dim() == 2 and rows.shape[0] == q.shape[0] and rows.is_contiguous()
    if q.shape[1] != frames.shape[2]:
        raise RuntimeError("moment_nbest: q is %d wide, the frames %d" % (q.shape[1], frames.shape[2]))
    _moment_table("moment_nbest", d, wnorm, normalize)
    d.q, d.ldq, d.rows, d.Nq, d.K, d.lmin, d.lmax = _p(q), _ld(q), _p(rows), rows.shape[0], rows.shape[1], int(lmin), int(lmax)
    d.M, d.iou_num, d.iou_den = int(n_best), int(nms[0]), int(nms[1])
    M = max(d.M, 0)                                   # a bad n_best is the library's to refuse, with its message
    start = torch.empty(d.Nq, d.K, M, dtype=torch.int32, device=q.device)
    length = torch.empty(d.Nq, d.K, M, dtype=torch.int32, device=q.device)
    score = torch.empty(d.Nq, d.K, M, dtype=torch.float32, device=q.device)
    d.start, d.length, d.score = _p(start), _p(length), _p(score)
    _lib.check(_lib.lib().univl_moment_nbest(_BYREF(d), _stream()), "moment_nbest")
    return start, length, score


def step_align(q, counts, frames, mask, rows, lmin, lmax, wnorm=None, normalize=True):
    """Lays ordered lists of step vectors over gallery rows (include/univl_hip.h: univl_step_align): for list i and gallery row
    rows[i, c], the windows (start, length) of its first counts[i] steps -- each of lmin .. lmax valid frames, in order, never
    overlapping -- whose moment_localize scores have the largest sum.  q: [Nl, K, 768] fp32 (vectors contiguous, K <= STEP_K_MAX; slots
    past counts[i] are padding and never read); counts: [Nl] int32; frames, mask, wnorm, normalize: as moment_localize's; rows: [Nl, C]
    int32.  Returns (start, length, score [Nl, C, K] int32, int32, fp32; total [Nl, C] fp32): padding slots are (-1, 0, -inf); a pair
    with no alignment, a row id outside the gallery or a count outside [1, K] is (-1, 0, -inf) in every slot with total -inf."""
    d = _moment_gallery(frames, mask, normalize, _lib.StepAlign)
    _require_gpu(q, counts, rows, wnorm)
    assert q.dtype == torch.float32 and q.dim() == 3 and q.stride(2) == 1
    Nl, K = q.shape[:2]
    ldq = q.stride(1) if K > 1 else q.stride(0) if Nl > 1 else q.shape[2]           # the stride of a dimension of one means nothing
    assert Nl == 1 or q.stride(0) == K * ldq, "the lists of q must lie K rows apart"
    assert counts.dtype == torch.int32 and counts.shape == (q.shape[0],) and counts.is_contiguous()
    assert rows.dtype == torch.int32 and rows.dim() == 2 and rows.shape[0] == q.shape[0] and rows.is_contiguous()
    if q.shape[2] != frames.shape[2]:
        raise RuntimeError("step_align: q is %d wide, the frames %d" % (q.shape[2], frames.shape[2]))
    _moment_table("step_align", d, wnorm, normalize)
    d.Nl, d.C, d.K, d.lmin, d.lmax = Nl, rows.shape[1], K, int(lmin), int(lmax)
    d.q, d.ldq, d.counts, d.rows = _p(q), ldq, _p(counts), _p(rows)
    start = torch.empty(d.Nl, d.C, d.K, dtype=torch.int32, device=q.device)
    length = torch.empty(d.Nl, d.C, d.K, dtype=torch.int32, device=q.device)
    score = torch.empty(d.Nl, d.C, d.K, dtype=torch.float32, device=q.device)
    total = torch.empty(d.Nl, d.C, dtype=torch.float32, device=q.device)
    d.start, d.length, d.score, d.total = _p(start), _p(length), _p(score), _p(total)
    _lib.check(_lib.lib().univl_step_align(_BYREF(d), _stream()), "step_align")
    return start, length, score, total


def frame_segment(q, counts, frames, mask, rows, switch_penalty, background=None, wnorm=None, normalize=True):
    """Labels every frame of gallery rows out of sets of label vectors (include/univl_hip.h: univl_frame_segment): for set i and gallery
    row rows[i, c], the labelling of the row's valid frames -- each frame one of the set's first counts[i] labels or the background --
    with the largest sum of frame scores minus switch_penalty per change of label between neighbouring valid frames.  A frame's score
    for a label is moment_localize's score of that one-frame window, bit for bit; for the background it is `background` (None: -inf, no
    background label).  q: [Nl, K, 768] fp32 (vectors contiguous, K <= SEGMENT_K_MAX; slots past counts[i] are padding and never read);
    counts: [Nl] int32; frames, mask, wnorm, normalize: as moment_localize's; rows: [Nl, C] int32; switch_penalty: finite, >= 0;
    background: a number or -inf.  Returns (label [Nl, C, F] int32: k, -1 for the background, -2 on a masked frame; score [Nl, C, F]
    fp32: the chosen label's frame score, -inf on a masked frame; total [Nl, C] fp32: the objective; nseg [Nl, C] int32: the runs of
    equal non-background labels).  A row id outside the gallery, a count outside [1, K] or a row without a valid frame is -2 / -inf on
    every frame with total -inf and nseg 0."""
    d = _moment_gallery(frames, mask, normalize, _lib.FrameSegment)
    _require_gpu(q, counts, rows, wnorm)
    assert q.dtype == torch.float32 and q.dim() == 3 and q.stride(2) == 1
    Nl, K = q.shape[:2]
    ldq = q.stride(1) if K > 1 else q.stride(0) if Nl > 1 else q.shape[2]           # the stride of a dimension of one means nothing
    assert Nl == 1 or q.stride(0) == K * ldq, "the sets of q must lie K rows apart"
    assert counts.dtype == torch.int32 and counts.shape == (q.shape[0],) and counts.is_contiguous()
    assert rows.dtype == torch.int32 and rows.dim() == 2 and rows.shape[0] == q.shape[0] and rows.is_contiguous()
    if q.shape[2] != frames.shape[2]:
        raise RuntimeError("frame_segment: q is %d wide, the frames %d" % (q.shape[2], frames.shape[2]))
    _moment_table("frame_segment", d, wnorm, normalize)
    d.Nl, d.C, d.K = Nl, rows.shape[1], K
    d.switch_penalty, d.background = float(switch_penalty), float("-inf") if background is None else float(background)
    d.q, d.ldq, d.counts, d.rows = _p(q), ldq, _p(counts), _p(rows)
    label = torch.empty(d.Nl, d.C, d.F, dtype=torch.int32, device=q.device)
    score = torch.empty(d.Nl, d.C, d.F, dtype=torch.float32, device=q.device)
    total = torch.empty(d.Nl, d.C, dtype=torch.float32, device=q.device)
    nseg = torch.empty(d.Nl, d.C, dtype=torch.int32, device=q.device)
    d.label, d.score, d.total, d.nseg = _p(label), _p(score), _p(total), _p(nseg)
    _lib.check(_lib.lib().univl_frame_segment(_BYREF(d), _stream()), "frame_segment")
    return label, score, total, nseg


def video_align(frames, mask, ref, rows, tau, local=False):
    """A monotone alignment of the valid frames of gallery row ref[p] (the exemplar) and gallery row rows[p, c], for every p and c in
    one launch (include/univl_hip.h: univl_video_align).  frames, mask: as window_norms'; ref: [P] int32; rows: [P, C] int32
    contiguous; tau: finite, subtracted from every cosine; local: False lays the whole of one video over the whole of the other (with
    tau = 1 classic DTW under the cosine distance), True finds the best common segment.  The cell score is ALWAYS the cosine of the two
    frames minus tau -- the model defines no video-video score, so there is no normalize switch and no norm table.  Returns (score
    [P, C] fp32, path_len [P, C] int32, path_a, path_b [P, C, 2 F] int32: the path's cells first to last as frame indices, -1 past
    path_len; match [P, C, F] int32: for every frame of the candidate the exemplar frame it is matched with, -1 a valid frame the path
    does not visit, -2 a masked frame; match_score [P, C, F] fp32: that cell's score, -inf where match < 0).  A row id outside the
    gallery or a video without a valid frame gives (-inf, 0, -1, -1, -2, -inf) throughout."""
    d = _lib.VideoAlign()
    _require_gpu(frames, mask, ref, rows)
    assert frames.dtype == torch.float32 and frames.dim() == 3 and frames.stride(2) == 1 and frames.stride(1) == frames.shape[2]
    assert mask.dtype == torch.int64 and mask.shape == frames.shape[:2] and mask.is_contiguous()
    assert ref.dtype == torch.int32 and ref.dim() == 1 and ref.is_contiguous()
    assert rows.dtype == torch.int32 and rows.dim() == 2 and rows.shape[0] == ref.shape[0] and rows.is_contiguous()
    d.N, d.F, d.H = frames.shape
    d.frames, d.ld_row, d.mask = _p(frames), frames.stride(0) if d.N > 1 else d.F * d.H, _p(mask)     # one row: its stride means nothing
    d.P, d.C = rows.shape
    d.tau, d.local = float(tau), int(local)
    d.ref, d.rows = _p(ref), _p(rows)
    dev = frames.device
    score = torch.empty(d.P, d.C, dtype=torch.float32, device=dev)
    path_len = torch.empty(d.P, d.C, dtype=torch.int32, device=dev)
    path_a = torch.empty(d.P, d.C, 2 * d.F, dtype=torch.int32, device=dev)
    path_b = torch.empty(d.P, d.C, 2 * d.F, dtype=torch.int32, device=dev)
    match = torch.empty(d.P, d.C, d.F, dtype=torch.int32, device=dev)
    match_score = torch.empty(d.P, d.C, d.F, dtype=torch.float32, device=dev)
    d.score, d.path_len, d.path_a, d.path_b, d.match, d.match_score = (_p(t) for t in (score, path_len, path_a, path_b, match, match_score))
    _lib.check(_lib.lib().univl_video_align(_BYREF(d), _stream()), "video_align")
    return score, path_len, path_a, path_b, match, match_score


class AdamTables:
    """Device copies of a UnivlSeg[] and a chunk table (adam_tables); keeps the tensors alive for the descriptors that point at them."""

    def __init__(self, segs, chunk_seg, chunk_off, chunk_len):
        self.segs, self.chunk_seg, self.chunk_off, self.chunk_len = segs, chunk_seg, chunk_off, chunk_len
        self.nseg, self.nchunk = segs.numel() // C.sizeof(_lib.Seg), chunk_seg.numel()


def adam_tables(segs, chunks, device="cuda"):
    """segs: [(offset, numel, lr, weight_decay, max_grad_norm, active), ...] -> a device UnivlSeg[]; chunks: [(seg, offset, len), ...]
    -> the chunk_seg / chunk_off / chunk_len arrays, as given (include/univl_hip.h: a tensor's chunks are listed contiguously; nothing
    here checks or rearranges the lists -- the explicit form of optimization._Tables, for tests and tools)."""
    arr = (_lib.Seg * len(segs))()
    for s, (off, numel, lr, wd, mgn, active) in enumerate(segs):
        arr[s].offset, arr[s].numel = int(off), int(numel)
        arr[s].lr, arr[s].weight_decay, arr[s].max_grad_norm, arr[s].active = lr, wd, mgn, int(active)
    return AdamTables(torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device),
                      torch.tensor([c[0] for c in chunks], dtype=torch.int32, device=device),
                      torch.tensor([c[1] for c in chunks], dtype=torch.int64, device=device),
                      torch.tensor([c[2] for c in chunks], dtype=torch.int32, device=device))


def adam_desc(tb, p, g, m, v, *, sumsq, step, seg_scalars, p16=None, p16_lo=None, coef=None, b1=0.9, b2=0.999, eps=1e-6, warmup=-1.0,
              t_total=-1, schedule=0, row_flags=None, flag_seg=0, row_len=0):
    """UnivlAdam over the flat buffers p / g / m / v (and the optional shadow pair) with the tables of adam_tables.  The caller keeps
    every tensor alive while the descriptor is used."""
    _require_gpu(p, g, m, v, p16, p16_lo, sumsq, step, seg_scalars, coef, row_flags)
    d = _lib.Adam()
    d.p, d.g, d.m, d.v, d.p16, d.p16_lo = _p(p), _p(g), _p(m), _p(v), _p(p16), _p(p16_lo)
    d.segs, d.nseg = _p(tb.segs), tb.nseg
    d.chunk_seg, d.chunk_off, d.chunk_len, d.nchunk = _p(tb.chunk_seg), _p(tb.chunk_off), _p(tb.chunk_len), tb.nchunk
    d.sumsq, d.coef, d.step, d.seg_scalars = _p(sumsq), _p(coef), _p(step), _p(seg_scalars)
    d.b1, d.b2, d.eps, d.warmup, d.t_total, d.schedule = b1, b2, eps, warmup, int(t_total), int(schedule)
    d.row_flags, d.flag_seg, d.row_len = _p(row_flags), int(flag_seg), int(row_len)
    return d


def grad_sumsq(g, tb, sumsq):
    """sumsq[s] += the sum of squares of segment s of g, over the chunks of tb (univl_grad_sumsq)."""
    _lib.check(_lib.lib().univl_grad_sumsq(_p(g), _p(tb.segs), tb.nseg, _p(tb.chunk_seg), _p(tb.chunk_off), _p(tb.chunk_len), tb.nchunk,
                                           _p(sumsq), _stream()), "grad_sumsq")


def clip_coef(sumsq, tb, max_norm, coef):
    """coef[0] <- min(1, max_norm / (total norm + 1e-6)), coef[1] <- total norm over the active segments (univl_clip_coef)."""
    _lib.check(_lib.lib().univl_clip_coef(_p(sumsq), _p(tb.segs), tb.nseg, float(max_norm), _p(coef), _stream()), "clip_coef")


def scale_grads(g, tb, coef):
    """g *= coef[0] over the chunks of tb (univl_scale_grads)."""
    _lib.check(_lib.lib().univl_scale_grads(_p(g), _p(tb.segs), _p(tb.chunk_seg), _p(tb.chunk_off), _p(tb.chunk_len), tb.nchunk, _p(coef),
                                            _stream()), "scale_grads")


def bert_adam(desc):
    _lib.check(_lib.lib().univl_bert_adam(_BYREF(desc), _stream()), "bert_adam")


def bert_adam_range(desc, chunk_begin, chunk_count, do_prep=False, max_blocks=0):
    _lib.check(_lib.lib().univl_bert_adam_range(_BYREF(desc), int(chunk_begin), int(chunk_count), int(bool(do_prep)), int(max_blocks),
                                                _stream()), "bert_adam_range")


def gemm_rider(gemm, adam, chunk_begin, chunk_count, max_blocks=0):
    """A forward product with chunks [chunk_begin, +chunk_count) of a prepared BertAdam update (univl_gemm_rider)."""
    _lib.check(_lib.lib().univl_gemm_rider(_BYREF(gemm), _BYREF(adam), int(chunk_begin), int(chunk_count), int(max_blocks), _stream()),
               "gemm_rider")


def cast_bf16(src, dst):
    _lib.check(_lib.lib().univl_cast_bf16(_p(src), _p(dst), src.numel(), _stream()), "cast_bf16")


def cast_bf16_pair(src, hi, lo):
    """hi <- bf16(src), lo <- bf16(src - hi); hi may be None (only the lo half is written)."""
    _lib.check(_lib.lib().univl_cast_bf16_pair(_p(src), _p(hi), _p(lo), src.numel(), _stream()), "cast_bf16_pair")


def cast_f32(src16, dst):
    _lib.check(_lib.lib().univl_cast_f32(_p(src16), _p(dst), src16.numel(), _stream()), "cast_f32")


def stamp(out):
    """out: one int64 / uint64 device word <- the device wall clock when this node runs (measurement, include/univl_hip.h)."""
    _lib.check(_lib.lib().univl_stamp(_p(out), _stream()), "stamp")


def bump_counter(ctr):
    _lib.check(_lib.lib().univl_bump_counter(_p(ctr), _stream()), "bump_counter")


def pair_concat_fwd(seq, vis, amask, vmask, tidx, vidx, P, W, F, out, out_mask):
    _lib.check(_lib.lib().univl_pair_concat_fwd(_p(seq), _p(vis), _p(amask), _p(vmask), _p(tidx), _p(vidx), P, W, F, _p(out),
                                                _p(out_mask), _stream()), "pair_concat_fwd")


def pair_concat_bwd(dout, tidx, vidx, P, W, F, dseq, dvis):
    _lib.check(_lib.lib().univl_pair_concat_bwd(_p(dout), _p(tidx), _p(vidx), P, W, F, _p(dseq), _p(dvis), _stream()), "pair_concat_bwd")


def postype_fwd(pos, type_emb, W, S, out):
    _lib.check(_lib.lib().univl_postype_fwd(_p(pos), _p(type_emb), W, S, _p(out), _stream()), "postype_fwd")


def postype_bwd(dtable, W, S, dpos, dtype_emb):
    _lib.check(_lib.lib().univl_postype_bwd(_p(dtable), W, S, _p(dpos), _p(dtype_emb), _stream()), "postype_bwd")


def tanh_fwd(x, y):
    _lib.check(_lib.lib().univl_tanh_fwd(_p(x), _p(y), x.numel(), _stream()), "tanh_fwd")


def tanh_bwd(dy, y, dx):
    _lib.check(_lib.lib().univl_tanh_bwd(dtype_code(dx.dtype), _p(dy), _p(y), _p(dx), y.numel(), _stream()), "tanh_bwd")


def gelu_bwd(dg, u, du):
    _lib.check(_lib.lib().univl_gelu_bwd(dtype_code(du.dtype), _p(dg), _p(u), _p(du), u.numel(), _stream()), "gelu_bwd")


def simdense_fwd(x, w, b, out):
    _lib.check(_lib.lib().univl_simdense_fwd(_p(x), _p(w), _p(b), x.shape[0], _p(out), _stream()), "simdense_fwd")


def simdense_bwd(ds, x, w, dx, dw, db):
    _lib.check(_lib.lib().univl_simdense_bwd(_p(ds), _p(x), _p(w), x.shape[0], _p(dx), _p(dw), _p(db), _stream()), "simdense_bwd")


def ce_loss(logits, labels, V, scratch2, loss, dlogits, ignore_index=-1):
    """logits: [rows, ld] fp32 view; dlogits: [rows, lddl] compute-type view."""
    _lib.check(_lib.lib().univl_ce_loss(dtype_code(dlogits.dtype), _p(logits), logits.stride(0), _p(labels), logits.shape[0], V,
                                        ignore_index, _p(scratch2), _p(loss), _p(dlogits), dlogits.stride(0), _stream()), "ce_loss")


def vocab_head_desc(cls, x, table, bias, labels, V, ignore_index=-1):
    """The leading fields that UnivlVocabCE and UnivlVocabScore share (cls: _lib.VocabCE or _lib.VocabScore): x [rows, K] and table
    [V(+pad), K] in the compute type, bias [V] fp32 or None, labels [rows] int64; slots = the 128-column tiles of a row, the second
    dimension of `partial`.  The caller fills the rest."""
    d = cls()
    d.dtype, (d.rows, d.K), d.V = dtype_code(x.dtype), x.shape, V
    d.x, d.ldx, d.table, d.ldt = _p(x), x.stride(0), _p(table), table.stride(0)
    d.bias, d.labels, d.ignore_index, d.slots = _p(bias), _p(labels), ignore_index, (V + 127) // 128
    return d


def vocab_ce_desc(x, table, bias, labels, dlogits, V, ignore_index=-1):
    """K16 descriptor (include/univl_hip.h: UnivlVocabCE) + the buffers it owns: x [rows, K], table [V(+pad), K] in the compute type,
    dlogits [rows, lddl] in the compute type.  Returns (desc, buffers) -- keep `buffers` alive as long as the descriptor is used."""
    d = vocab_head_desc(_lib.VocabCE, x, table, bias, labels, V, ignore_index)
    rows, dev = d.rows, x.device
    b = dict(partial=torch.empty(rows, d.slots, 2, device=dev), label_logit=torch.zeros(rows, device=dev), lse=torch.empty(rows, device=dev),
             rowloss=torch.empty(rows, device=dev), scratch=torch.zeros(2, device=dev), loss=torch.zeros(1, device=dev),
             keep=(x, table, bias, labels, dlogits))
    d.partial, d.label_logit, d.lse, d.rowloss = _p(b["partial"]), _p(b["label_logit"]), _p(b["lse"]), _p(b["rowloss"])
    d.scratch2, d.loss, d.gout = _p(b["scratch"]), _p(b["loss"]), None
    d.dlogits, d.lddl = _p(dlogits), dlogits.stride(0)
    return d, b


def vocab_ce_fwd(desc):
    _lib.check(_lib.lib().univl_vocab_ce_fwd(C.byref(desc), _stream()), "vocab_ce_fwd")


def vocab_ce_bwd(desc):
    _lib.check(_lib.lib().univl_vocab_ce_bwd(C.byref(desc), _stream()), "vocab_ce_bwd")


def vocab_ce_weighted_desc(x, table, bias, labels, dlogits, V, seq_weight, seq_len, ignore_index=-1):
    """Descriptor of the weighted form of K16 (include/univl_hip.h: UnivlVocabCEW) + the buffers it owns: vocab_ce_desc's operands plus
    seq_weight [rows / seq_len] fp32 on the device, caption c owning rows [c * seq_len, (c + 1) * seq_len).  Returns (desc, buffers).
    Shapes and dtypes are checked here; the argument RANGE is the library's to refuse."""
    _require_gpu(x, table, bias, labels, dlogits, seq_weight)
    assert seq_weight.dtype == torch.float32 and seq_weight.is_contiguous()
    assert seq_len < 1 or seq_weight.numel() * seq_len >= x.shape[0]
    d = vocab_head_desc(_lib.VocabCEW, x, table, bias, labels, V, ignore_index)
    rows, dev = d.rows, x.device
    b = dict(partial=torch.empty(rows, max(d.slots, 1), 2, device=dev), label_logit=torch.zeros(rows, device=dev),
             lse=torch.empty(rows, device=dev), rowloss=torch.empty(rows, device=dev), scratch=torch.zeros(2, device=dev),
             loss=torch.zeros(1, device=dev), keep=(x, table, bias, labels, dlogits, seq_weight))
    d.partial, d.label_logit, d.lse, d.rowloss = _p(b["partial"]), _p(b["label_logit"]), _p(b["lse"]), _p(b["rowloss"])
    d.scratch2, d.loss, d.gout = _p(b["scratch"]), _p(b["loss"]), None
    d.dlogits, d.lddl = _p(dlogits), dlogits.stride(0)
    d.seq_weight, d.seq_len = _p(seq_weight), int(seq_len)
    return d, b


def vocab_ce_weighted_fwd(desc):
    _lib.check(_lib.lib().univl_vocab_ce_weighted_fwd(C.byref(desc), _stream()), "vocab_ce_weighted_fwd")


def vocab_ce_weighted_bwd(desc):
    _lib.check(_lib.lib().univl_vocab_ce_weighted_bwd(C.byref(desc), _stream()), "vocab_ce_weighted_bwd")


def vocab_ce_smooth_desc(x, table, bias, labels, dlogits, V, smoothing, seq_weight=None, seq_len=None, ignore_index=-1):
    """Descriptor of the smoothed form of K16 (include/univl_hip.h: UnivlVocabCES) + the buffers it owns: vocab_ce_desc's operands, the
    label smoothing eps and, optionally, vocab_ce_weighted_desc's seq_weight [rows / seq_len] (None: every weight 1, seq_len is not
    looked at).  partial_sum [rows, slots] is allocated whatever eps is.  Returns (desc, buffers).  Shapes and dtypes are checked here;
    the argument RANGE -- eps in [0, 1) included -- is the library's to refuse."""
    _require_gpu(x, table, bias, labels, dlogits, seq_weight)
    if seq_weight is not None:
        assert seq_weight.dtype == torch.float32 and seq_weight.is_contiguous()
        assert seq_len is not None and (seq_len < 1 or seq_weight.numel() * seq_len >= x.shape[0])
    d = vocab_head_desc(_lib.VocabCES, x, table, bias, labels, V, ignore_index)
    rows, dev = d.rows, x.device
    b = dict(partial=torch.empty(rows, max(d.slots, 1), 2, device=dev), partial_sum=torch.empty(rows, max(d.slots, 1), device=dev),
             label_logit=torch.zeros(rows, device=dev), lse=torch.empty(rows, device=dev), rowloss=torch.empty(rows, device=dev),
             scratch=torch.zeros(2, device=dev), loss=torch.zeros(1, device=dev), keep=(x, table, bias, labels, dlogits, seq_weight))
    d.partial, d.label_logit, d.lse, d.rowloss = _p(b["partial"]), _p(b["label_logit"]), _p(b["lse"]), _p(b["rowloss"])
    d.scratch2, d.loss, d.gout = _p(b["scratch"]), _p(b["loss"]), None
    d.dlogits, d.lddl = _p(dlogits), dlogits.stride(0)
    d.seq_weight, d.seq_len = _p(seq_weight), int(seq_len) if seq_weight is not None else 0
    d.smoothing, d.partial_sum = float(smoothing), _p(b["partial_sum"])
    return d, b


def vocab_ce_smooth_fwd(desc):
    _lib.check(_lib.lib().univl_vocab_ce_smooth_fwd(C.byref(desc), _stream()), "vocab_ce_smooth_fwd")


def vocab_ce_smooth_bwd(desc):
    _lib.check(_lib.lib().univl_vocab_ce_smooth_bwd(C.byref(desc), _stream()), "vocab_ce_smooth_bwd")


def vocab_score_desc(x, table, bias, labels, V, seq_len, ignore_index=-1, out=None):
    """Descriptor of the scoring form of K16 (include/univl_hip.h: UnivlVocabScore) + the buffers it owns: x [rows, K], table [V(+pad), K]
    in the compute type, bias [V] fp32 or None, labels [rows] int64; rows = n_seq * seq_len.  out: optional dict of caller-owned output
    tensors (any of token_logprob, top_token, top_logprob, lse [rows]; seq_logprob, seq_tokens, seq_correct [n_seq]).  Returns
    (desc, buffers) -- keep `buffers` alive as long as the descriptor is used.  Shapes and dtypes are checked here; the argument RANGE
    is the library's to refuse."""
    _require_gpu(x, table, bias, labels)
    assert x.dim() == 2 and table.dim() == 2 and x.stride(1) == 1 and table.stride(1) == 1 and table.dtype == x.dtype
    assert labels.dtype == torch.int64 and labels.is_contiguous()
    assert bias is None or (bias.dtype == torch.float32 and bias.is_contiguous())
    rows, K = x.shape
    assert labels.numel() == rows and table.shape[1] == K and table.shape[0] >= V
    d = vocab_head_desc(_lib.VocabScore, x, table, bias, labels, V, ignore_index)
    d.slots, d.seq_len = max(d.slots, 1), seq_len      # V < 1 is the library's to refuse: the buffers still get a shape
    n_seq = rows // seq_len if seq_len > 0 else 0
    dev = x.device
    f, i = torch.float32, torch.int32
    b = dict(partial=torch.empty(rows, d.slots, 2, device=dev), partial_top=torch.empty(rows, d.slots, device=dev, dtype=i),
             label_logit=torch.zeros(rows, device=dev), keep=(x, table, bias, labels))
    for name, n, dt in (("token_logprob", rows, f), ("top_token", rows, i), ("top_logprob", rows, f), ("lse", rows, f),
                        ("seq_logprob", n_seq, f), ("seq_tokens", n_seq, i), ("seq_correct", n_seq, i)):
        t = (out or {}).get(name)
        if t is None:
            t = torch.empty(n, device=dev, dtype=dt)
        _require_gpu(t)
        assert t.dtype == dt and t.numel() == n and t.is_contiguous(), name
        b[name] = t
    d.partial, d.partial_top, d.label_logit = _p(b["partial"]), _p(b["partial_top"]), _p(b["label_logit"])
    d.token_logprob, d.top_token, d.top_logprob, d.lse = _p(b["token_logprob"]), _p(b["top_token"]), _p(b["top_logprob"]), _p(b["lse"])
    d.seq_logprob, d.seq_tokens, d.seq_correct = _p(b["seq_logprob"]), _p(b["seq_tokens"]), _p(b["seq_correct"])
    return d, b


def vocab_score(desc):
    _lib.check(_lib.lib().univl_vocab_score(C.byref(desc), _stream()), "vocab_score")


def mfm_nce_loss(logits, vmask, labels, scratch2, loss, dlogits):
    n = logits.shape[0]
    _lib.check(_lib.lib().univl_mfm_nce_loss(_p(logits), logits.stride(0), _p(vmask), _p(labels), n, _p(scratch2), _p(loss),
                                             _p(dlogits), dlogits.stride(0), _stream()), "mfm_nce_loss")


def colsum(x, out):
    """out[c] += sum_r x[r, c]; x: [rows, ld] view in the compute type."""
    _lib.check(_lib.lib().univl_colsum(dtype_code(x.dtype), _p(x), x.stride(0), x.shape[0], x.shape[1], _p(out), _stream()), "colsum")


def scale_ct(x, s):
    _lib.check(_lib.lib().univl_scale_ct_by_device_scalar(dtype_code(x.dtype), _p(x), x.numel(), _p(s), _stream()), "scale_ct")
