// The fused BertAdam update (modules/optimization.py:103-168), stated once for every kernel that applies it: adam_elem is the element
// update of adam_apply_kernel<NT> (optim.hip, which includes this header) and of adam_chunk below; adam_chunk is one chunk of the update
// as a device function, for the kernels that carry optimizer work beside their own (gemm.hip: gemm_adam_kernel, gemm_adam_rect_kernel,
// gemm_ln_kernel, attn_fwd_qkv_kernel), with adam_apply_kernel's walk and non-temporal policy; NTH = threads of the calling workgroup.
#pragma once
#include <type_traits>
#include "common.h"
#include "univl_hip.h"

// The update kernels take their 16-byte vector path from a chunk's element offset alone (off & 3), so the flat buffers themselves must sit
// on those boundaries: p / g / m / v 16-byte aligned, p16 / p16_lo (where given) 8-byte aligned.  Every entry point that carries chunks
// refuses a descriptor that does not (UNIVL_EINVAL, before any launch).
static inline bool adam_bases_aligned(const UnivlAdam* a) {
    return aligned16(a->p) && aligned16(a->g) && aligned16(a->m) && aligned16(a->v) && ((((uintptr_t)a->p16 | (uintptr_t)a->p16_lo) & 7) == 0);
}

// What every kernel that walks chunks of an update reads (univl_bert_adam / _range also need sumsq, step and nseg for the scalar kernel).
static inline bool adam_tables_present(const UnivlAdam* a) {
    return a->p && a->g && a->m && a->v && a->segs && a->chunk_seg && a->chunk_off && a->chunk_len && a->seg_scalars && a->nchunk > 0;
}

// The check of a chunk range [begin, begin + count) of a prepared update, for every entry point `who` that applies or carries one, before
// any launch.  none_ok: the entry point runs without an update too (count == 0; the descriptor may then be NULL and is not looked at).
static inline int adam_range_check(const char* who, const UnivlAdam* a, int32_t begin, int32_t count, bool none_ok) {
    if (none_ok && count == 0) return UNIVL_OK;
    UNIVL_CHECK_ARG(a != nullptr, UNIVL_EINVAL, "%s: null descriptor", who);
    UNIVL_CHECK_ARG(adam_tables_present(a) && begin >= 0 && count >= 0 && count <= a->nchunk - begin, UNIVL_EINVAL,
                    "%s: chunks [%d, +%d) of %d", who, begin, count, a->nchunk);
    UNIVL_CHECK_ARG(adam_bases_aligned(a), UNIVL_EINVAL, "%s: p / g / m / v must be 16-byte aligned, p16 / p16_lo 8-byte aligned", who);
    return UNIVL_OK;
}

// A checked range as the kernels take it: the descriptor by value (the zero descriptor when nothing rides), chunks [c0, c1), and the
// workgroups that walk them (one per chunk, at most max_blocks where that is > 0).
struct AdamRange {
    UnivlAdam adam;
    int c0, c1, blocks;
};
static inline AdamRange adam_range(const UnivlAdam* a, int32_t begin, int32_t count, int32_t max_blocks) {
    AdamRange r = {};
    r.c0 = r.c1 = begin;
    if (count > 0) {
        r.adam = *a;
        r.c1 = begin + count;
        r.blocks = (max_blocks > 0 && max_blocks < count) ? max_blocks : count;
    }
    return r;
}

// One element of the update, for EVERY kernel that applies it (adam_apply_kernel in optim.hip, adam_chunk below).  The association is pinned
// with explicit fused multiply-adds: left to the compiler's contraction, `m * b1 + (1 - b1) * gr` became fma(1 - b1, gr, m * b1) in one
// kernel and fma(b1, m, (1 - b1) * gr) in another (likewise v), and the launch forms that promise the same bits differed in the last
// bit of m and v wherever the moments were not zero (tests/test_optim_gpu.py compares them on non-zero moments).
__device__ __forceinline__ void adam_elem(float& p, const float g, float& m, float& v, const float gs, const float lr, const float wd,
                                          const float b1, const float b2, const float eps) {
    const float gr = g * gs;
    m = __builtin_fmaf(1.0f - b1, gr, m * b1);
    v = __builtin_fmaf((1.0f - b2) * gr, gr, v * b2);
    const float upd = __builtin_fmaf(wd, p, m / (sqrtf(v) + eps));
    p = __builtin_fmaf(-lr, upd, p);
}
// ... and of a row nobody ever touched (UnivlAdam.row_flags): what adam_elem gives for g = m = v = 0
__device__ __forceinline__ float adam_elem_decay_only(const float p, const float lr, const float wd) { return __builtin_fmaf(-lr, wd * p, p); }

bool univl_adam_nt();      // optim.hip: UNIVL_ADAM_NT (default 1): non-temporal loads / stores of the 28 fp32 bytes per parameter
// f(std::bool_constant<NT>) with the switch's value: the one place that picks the <NT> instantiation of a kernel that applies the update
template <typename F> static inline void adam_with_nt(F&& f) {
    if (univl_adam_nt()) f(std::true_type{});
    else f(std::false_type{});
}

template <bool NT> __device__ __forceinline__ f32x4_t adam_ld4(const float* p, int i) {
    const f32x4_t* q = reinterpret_cast<const f32x4_t*>(p) + i;
    if (NT) return __builtin_nontemporal_load(q);
    return *q;
}
template <bool NT> __device__ __forceinline__ void adam_st4(float* p, int i, f32x4_t v) {
    f32x4_t* q = reinterpret_cast<f32x4_t*>(p) + i;
    if (NT) __builtin_nontemporal_store(v, q);
    else *q = v;
}

// LO: the instantiation also keeps the lo half of the shadow pair (UnivlAdam.p16_lo).  The rider kernel of the 64 x 128 tile is built for
// <= 80 VGPRs (three workgroups per unit) and spilled two more with it: it instantiates LO = false and the host keeps an update that carries
// p16_lo out of that kernel (univl_gemm_rider).
template <bool NT, int NTH, bool LO = true>
__device__ __forceinline__ void adam_chunk(const UnivlAdam& a, int c) {
    const int seg = a.chunk_seg[c];
    const UnivlSeg sg = a.segs[seg];
    if (!sg.active) return;
    const float gs = a.seg_scalars[2 * seg], lr = a.seg_scalars[2 * seg + 1], wd = sg.weight_decay;
    const float b1 = a.b1, b2 = a.b2, eps = a.eps;
    const int64_t off = a.chunk_off[c];
    const int len = a.chunk_len[c];
    float* p = a.p + off; const float* g = a.g + off; float* m = a.m + off; float* v = a.v + off;
    __bf16* p16 = a.p16 ? reinterpret_cast<__bf16*>(a.p16) + off : nullptr;
    __bf16* p16lo = (LO && a.p16 && a.p16_lo) ? reinterpret_cast<__bf16*>(a.p16_lo) + off : nullptr;      // lo half of the shadow pair
    const int nv = ((off & 3) == 0) ? len / 4 : 0;
    auto update = [&](int i, f32x4_t pp, const f32x4_t gg, f32x4_t mm, f32x4_t vv) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = pp[e], me = mm[e], ve = vv[e];
            adam_elem(pe, gg[e], me, ve, gs, lr, wd, b1, b2, eps);
            pp[e] = pe; mm[e] = me; vv[e] = ve;
        }
        adam_st4<NT>(p, i, pp);
        adam_st4<NT>(m, i, mm);
        adam_st4<NT>(v, i, vv);
        if (p16) {
            bf16x4_t w;
            w[0] = (__bf16)pp[0]; w[1] = (__bf16)pp[1]; w[2] = (__bf16)pp[2]; w[3] = (__bf16)pp[3];
            reinterpret_cast<bf16x4_t*>(p16)[i] = w;
            if (p16lo) {
                bf16x4_t l;
                l[0] = (__bf16)(pp[0] - (float)w[0]); l[1] = (__bf16)(pp[1] - (float)w[1]);
                l[2] = (__bf16)(pp[2] - (float)w[2]); l[3] = (__bf16)(pp[3] - (float)w[3]);
                reinterpret_cast<bf16x4_t*>(p16lo)[i] = l;
            }
        }
    };
    int i = threadIdx.x;
    for (; i + NTH < nv; i += 2 * NTH) {
        const f32x4_t p0 = adam_ld4<NT>(p, i), p1 = adam_ld4<NT>(p, i + NTH);
        const f32x4_t g0 = adam_ld4<NT>(g, i), g1 = adam_ld4<NT>(g, i + NTH);
        const f32x4_t m0 = adam_ld4<NT>(m, i), m1 = adam_ld4<NT>(m, i + NTH);
        const f32x4_t v0 = adam_ld4<NT>(v, i), v1 = adam_ld4<NT>(v, i + NTH);
        update(i, p0, g0, m0, v0);
        update(i + NTH, p1, g1, m1, v1);
    }
    for (; i < nv; i += NTH) update(i, adam_ld4<NT>(p, i), adam_ld4<NT>(g, i), adam_ld4<NT>(m, i), adam_ld4<NT>(v, i));
    for (int j = nv * 4 + threadIdx.x; j < len; j += NTH) {
        float pi = p[j], mi = m[j], vi = v[j];
        adam_elem(pi, g[j], mi, vi, gs, lr, wd, b1, b2, eps);
        p[j] = pi; m[j] = mi; v[j] = vi;
        if (p16) p16[j] = (__bf16)pi;
        if (p16lo) p16lo[j] = (__bf16)(pi - (float)(__bf16)pi);
    }
}
