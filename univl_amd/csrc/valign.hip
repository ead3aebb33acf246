// Video-to-video alignment on the device (include/univl_hip.h: univl_video_align): a monotone alignment of the valid frames of two
// gallery rows -- classic DTW under the cosine distance with local = 0, tau = 1; the best common segment (Smith-Waterman without gaps
// scored apart) with local = 1.  The neighbours of this file (moment.hip) ask a TEXT about a video; this one asks a video about a video,
// and its product is matrix-shaped on both sides: up to 128 x 128 frame pairs of depth 768.
//
// One workgroup of 256 threads per (exemplar, candidate) pair, one launch, no workspace, no host read, no atomics, capturable:
//   compact    wave 0 lists the valid frames of a, wave 1 those of b (ballots); everything after works on POSITIONS i < Ta, j < Tb and
//              turns them back into frame indices only when it writes.
//   gram       G(i, j) = x_{f_i} . y_{g_j} by v_mfma_f32_32x32x2_f32: the 4 x 4 grid of 32 x 32 tiles is dealt to the four waves by
//              (tile row & 1, tile column & 1), so a wave holds at most 2 x 2 tiles (64 accumulator registers) and the tiles that lie
//              wholly past Ta or Tb are never computed -- at Ta, Tb <= 64 every wave has one tile.  Both rows travel through LDS in K
//              slabs of 32 columns (24 slabs), the next slab's global loads in flight in registers during the products.  A slab row
//              keeps its even columns in words 0 .. 15 and its odd ones in 16 .. 31: the MFMA takes k = lane >> 5 from the upper
//              half-wave, so a lane's operands of four consecutive MFMAs are ONE 16-byte LDS read.  Accumulators start at 0 and an MFMA
//              adds its two products in ascending k, one rounding each: G is bit for bit the fmaf chain over k = 0 .. 767.
//   norms      thread t < 128 owns position t of a, thread 128 + t position t of b: the same chain over x * x from the same slabs,
//              carried in one register across the slabs, then sqrtf.
//   table      every thread turns its accumulators into e(i, j) = G / (max(na_i, 1e-12) * max(nb_j, 1e-12)) - tau and stores them
//              to the LDS table, which overlays the slabs (dead by then).  PITCH 136 floats: cell (i, d - i) of anti-diagonal d lies at
//              word 135 i + d, and 135 is odd, so 64 consecutive rows of a diagonal hit 64 different banks; and 4 x 136 = 32 (mod 64),
//              so the two half-waves of an accumulator register (rows r and r + 4, 32 columns each) store to disjoint banks as well.
//   programme  ONE wave, two rows per lane (lane l owns positions l and l + 64 of a), no barrier: on anti-diagonal d a lane computes
//              cells (l, d - l) and (l + 64, d - l - 64).  Left is the lane's own previous value, up comes from lane l - 1 by one
//              cross-lane read per row (lane 0's upper row takes lane 63's lower), diagonal is the up of the diagonal before.  Ta + Tb
//              - 1 <= 255 steps of two LDS reads, two cross-lane moves and a few compares.  The two predecessor bits of a cell are
//              gathered 16 cells to a word in a register and stored when the word is full: 4 KB for the whole table.  With local
//              every row keeps its best cell (first j among equals), reduced at the end under (H descending, i ascending).
//   walk       lane 0 walks the predecessor bits back from the end cell (at most 255 dependent LDS reads) into a byte list; then all
//              threads write the path forward, the first thread of every column notes where the column's run begins, and thread j
//              folds its column's run into match / match_score.  Masked frames of b are written by the lanes that read the mask.
//
// PURITY.  G, na, nb are functions of the two frames alone (the tile a cell falls in decides who computes it, not what), e of those
// and tau, the programme of e alone: nothing depends on the grid, the pair's place, its company, C or deterministic mode; and since
// a * b == b * a, e_ab(i, j) == e_ba(j, i) bit for bit.
#include <float.h>
#include <limits.h>
#include <stddef.h>
#include "common.h"
#include "univl_hip.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;

constexpr int VA_H = 768;                        // frame width (the hidden size)
constexpr int VA_FM = UNIVL_MOMENT_F_MAX;
constexpr int VA_KS = 32;                        // columns per slab
constexpr int VA_SP = 36;                        // slab pitch in floats: rows 144 B apart, 16-byte reads of 16 rows hit 16 different 4-bank groups
constexpr int VA_TP = 136;                       // table pitch in floats (see above)
constexpr size_t VA_LDS = (size_t)VA_FM * VA_TP * sizeof(float);          // 69 632 B; the two slabs (36 864 B) overlay it
static_assert(2 * VA_FM * VA_SP * sizeof(float) <= VA_LDS, "the slabs overlay the table");
static_assert(VA_FM == 128, "two rows per lane, 4 x 4 tiles of 32");

extern __shared__ __attribute__((aligned(16))) unsigned char va_smem[];

struct VaArgs {
    const float* frames; long ld_row;
    const int64_t* mask;
    const int32_t* ref; const int32_t* rows;
    int N, F, C, local;
    float tau;
    float* score; int32_t* path_len; int32_t* path_a; int32_t* path_b; int32_t* match; float* match_score;
};

// one cell of the programme.  has_d / has_u / has_l: which predecessors exist; the order diagonal, up, left decides among equals.
// code: 0 diagonal, 1 up, 2 left, 3 the cell starts a path
__device__ __forceinline__ float va_cell(float e, bool has_d, bool has_u, bool has_l, float hd, float hu, float hl, int local, unsigned& code) {
    float pm = 0.f;
    code = 3;
    if (has_d) { pm = hd; code = 0; }
    if (has_u && (code == 3 || hu > pm)) { pm = hu; code = 1; }
    if (has_l && (code == 3 || hl > pm)) { pm = hl; code = 2; }
    if (code == 3 || (local && pm <= 0.f)) { code = 3; return e; }
    return e + pm;
}

__global__ __launch_bounds__(256) void video_align_kernel(VaArgs a) {
    __shared__ int vfa[VA_FM], vfb[VA_FM];           // the valid frames of a and b, ascending
    __shared__ float na[VA_FM], nb[VA_FM];           // their norms, by position
    __shared__ unsigned pred[VA_FM * 8];             // two bits per cell, row i's cells 16 j' .. 16 j' + 15 in word 8 i + j'      4 KB
    __shared__ unsigned char pi[2 * VA_FM], pj[2 * VA_FM];   // the path, LAST cell first
    __shared__ int colstart[VA_FM];                  // where column j's run of the forward path begins, -1: not visited
    __shared__ int cnt[2];
    __shared__ int s_len;
    __shared__ float s_score;
    float* tab = reinterpret_cast<float*>(va_smem);
    float* sa = tab;
    float* sb = tab + VA_FM * VA_SP;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, F = a.F;
    const long p = blockIdx.x;
    const int ra = a.ref[p / a.C], rb = a.rows[p];
    int32_t* path_a = a.path_a + p * 2 * F;
    int32_t* path_b = a.path_b + p * 2 * F;
    int32_t* match = a.match + p * F;
    float* match_score = a.match_score + p * F;
    auto nothing = [&]() {                                                // 2 F <= 256: a thread per path slot
        if (tid < 2 * F) { path_a[tid] = -1; path_b[tid] = -1; }
        if (tid < F) { match[tid] = -2; match_score[tid] = -INFINITY; }
        if (tid == 0) { a.score[p] = -INFINITY; a.path_len[p] = 0; }
    };
    if (ra < 0 || ra >= a.N || rb < 0 || rb >= a.N) {                     // block-uniform: nothing of the gallery is read
        nothing();
        return;
    }

    // ---- compact: wave 0 the frames of a, wave 1 those of b
    if (tid < VA_FM) colstart[tid] = -1;
    if (wave < 2) {
        const int64_t* m = a.mask + (long)(wave ? rb : ra) * F;
        int* vf = wave ? vfb : vfa;
        const bool v0 = lane < F && m[lane] != 0, v1 = lane + 64 < F && m[lane + 64] != 0;
        const unsigned long long b0 = __ballot(v0), b1 = __ballot(v1), below = (1ull << lane) - 1;
        if (v0) vf[__popcll(b0 & below)] = lane;
        if (v1) vf[__popcll(b0) + __popcll(b1 & below)] = lane + 64;
        if (lane == 0) cnt[wave] = __popcll(b0) + __popcll(b1);
        if (wave == 1) {                                                  // a masked frame of b: no other thread writes it
            if (lane < F && !v0) { match[lane] = -2; match_score[lane] = -INFINITY; }
            if (lane + 64 < F && !v1) { match[lane + 64] = -2; match_score[lane + 64] = -INFINITY; }
        }
    }
    __syncthreads();
    const int Ta = cnt[0], Tb = cnt[1];
    if (Ta == 0 || Tb == 0) {                                             // block-uniform
        nothing();
        return;
    }

    // ---- gram and norms
    const float* xa = a.frames + (long)ra * a.ld_row;
    const float* xb = a.frames + (long)rb * a.ld_row;
    const int ta32 = (Ta + 31) & ~31, tb32 = (Tb + 31) & ~31;
    // the loader's share of a slab: items tid + 256 it, item = 8 row + c4 (a row is eight 16-byte pieces); rows past the last tile
    // that is computed are not loaded, rows past T inside it repeat the last valid frame (a valid address, a value nobody reads)
    int offa[4], offb[4];
    bool lda[4], ldb[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int item = tid + 256 * it, row = item >> 3, c4 = item & 7;
        lda[it] = row < ta32;
        ldb[it] = row < tb32;
        offa[it] = vfa[min(row, Ta - 1)] * VA_H + 4 * c4;
        offb[it] = vfb[min(row, Tb - 1)] * VA_H + 4 * c4;
    }
    f32x4_t ga[4], gb[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) { ga[it] = f32x4_t{0.f, 0.f, 0.f, 0.f}; gb[it] = ga[it]; }
    auto gload = [&](int k0) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            if (lda[it]) ga[it] = *reinterpret_cast<const f32x4_t*>(xa + offa[it] + k0);
            if (ldb[it]) gb[it] = *reinterpret_cast<const f32x4_t*>(xb + offb[it] + k0);
        }
    };
    auto sstore = [&]() {                                                 // columns 4 c4 .. + 3: the even ones to word 2 c4, the odd to 16 + 2 c4
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int item = tid + 256 * it, at = (item >> 3) * VA_SP + 2 * (item & 7);
            if (lda[it]) {
                *reinterpret_cast<f32x2_t*>(sa + at) = f32x2_t{ga[it][0], ga[it][2]};
                *reinterpret_cast<f32x2_t*>(sa + at + 16) = f32x2_t{ga[it][1], ga[it][3]};
            }
            if (ldb[it]) {
                *reinterpret_cast<f32x2_t*>(sb + at) = f32x2_t{gb[it][0], gb[it][2]};
                *reinterpret_cast<f32x2_t*>(sb + at + 16) = f32x2_t{gb[it][1], gb[it][3]};
            }
        }
    };
    // the wave's tiles: rows 32 (wr + 2 ti), columns 32 (wc + 2 tj)
    const int wr = wave >> 1, wc = wave & 1, r = lane & 31, h = lane >> 5;
    const bool ta0 = 32 * wr < Ta, ta1 = 32 * (wr + 2) < Ta, tb0 = 32 * wc < Tb, tb1 = 32 * (wc + 2) < Tb;
    const float* fa0 = sa + (32 * wr + r) * VA_SP + 16 * h;
    const float* fa1 = fa0 + 64 * VA_SP;
    const float* fb0 = sb + (32 * wc + r) * VA_SP + 16 * h;
    const float* fb1 = fb0 + 64 * VA_SP;
    f32x16_t c00, c01, c10, c11;
#pragma unroll
    for (int i = 0; i < 16; ++i) { c00[i] = 0.f; c01[i] = 0.f; c10[i] = 0.f; c11[i] = 0.f; }
    // the norm this thread carries
    const int nrow = tid & 127;
    const bool nmine = nrow < (tid < 128 ? Ta : Tb);
    const float* nsrc = (tid < 128 ? sa : sb) + nrow * VA_SP;
    float n2 = 0.f;

    gload(0);
    for (int k0 = 0; k0 < VA_H; k0 += VA_KS) {
        if (k0) __syncthreads();                                          // the slab before is read
        sstore();
        __syncthreads();
        if (k0 + VA_KS < VA_H) gload(k0 + VA_KS);
        if (nmine) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4_t ev = *reinterpret_cast<const f32x4_t*>(nsrc + 4 * q);
                const f32x4_t od = *reinterpret_cast<const f32x4_t*>(nsrc + 16 + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    n2 = fmaf(ev[e], ev[e], n2);
                    n2 = fmaf(od[e], od[e], n2);
                }
            }
        }
        if (ta0 && tb0) {                                                 // wave-uniform: a wave without a tile only loads and waits
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4_t A0 = *reinterpret_cast<const f32x4_t*>(fa0 + 4 * q), A1 = A0, B0 = *reinterpret_cast<const f32x4_t*>(fb0 + 4 * q), B1 = B0;
                if (ta1) A1 = *reinterpret_cast<const f32x4_t*>(fa1 + 4 * q);
                if (tb1) B1 = *reinterpret_cast<const f32x4_t*>(fb1 + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    c00 = __builtin_amdgcn_mfma_f32_32x32x2f32(A0[e], B0[e], c00, 0, 0, 0);
                    if (tb1) c01 = __builtin_amdgcn_mfma_f32_32x32x2f32(A0[e], B1[e], c01, 0, 0, 0);
                    if (ta1) c10 = __builtin_amdgcn_mfma_f32_32x32x2f32(A1[e], B0[e], c10, 0, 0, 0);
                    if (ta1 && tb1) c11 = __builtin_amdgcn_mfma_f32_32x32x2f32(A1[e], B1[e], c11, 0, 0, 0);
                }
            }
        }
    }
    __syncthreads();                                                      // the last slab is read: the table may overlay it
    if (nmine) (tid < 128 ? na : nb)[nrow] = sqrtf(n2);
    __syncthreads();
    {
        const float tau = a.tau;
        auto store_tile = [&](const f32x16_t& c, int i0, int j0) {        // C layout: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
            const int j = j0 + r;
            if (j >= Tb) return;
            const float dj = fmaxf(nb[j], 1e-12f);
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int i = i0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                if (i < Ta) tab[i * VA_TP + j] = c[reg] / (fmaxf(na[i], 1e-12f) * dj) - tau;
            }
        };
        if (ta0 && tb0) store_tile(c00, 32 * wr, 32 * wc);
        if (ta0 && tb1) store_tile(c01, 32 * wr, 32 * (wc + 2));
        if (ta1 && tb0) store_tile(c10, 32 * (wr + 2), 32 * wc);
        if (ta1 && tb1) store_tile(c11, 32 * (wr + 2), 32 * (wc + 2));
    }
    __syncthreads();

    // ---- programme and walk: wave 0
    if (wave == 0) {
        const int local = a.local;
        const int r0 = lane, r1 = lane + 64, prev = (lane + 63) & 63;
        const bool on0 = r0 < Ta, on1 = r1 < Ta;
        float h0 = 0.f, h1 = 0.f;                    // the rows' cells of the diagonal before
        float d0 = 0.f, d1 = 0.f;                    // the up values of the diagonal before: this one's diagonal predecessors
        float best0 = -INFINITY, best1 = -INFINITY, hend = -INFINITY;
        int bj0 = 0, bj1 = 0;
        unsigned w0 = 0, w1 = 0;
        const float* t0 = tab + r0 * VA_TP - r0;     // cell (r0, d - r0) at t0[d]
        const float* t1 = tab + r1 * VA_TP - r1;
        const int nd = Ta + Tb - 1;
        for (int d = 0; d < nd; ++d) {
            const float s0 = __shfl(h0, prev, 64), s1 = __shfl(h1, prev, 64);
            const float u0 = s0, u1 = lane ? s1 : s0;                     // row 64 sits under row 63: lane 63's lower row
            const int j0 = d - r0, j1 = d - r1;
            if (on0 && j0 >= 0 && j0 < Tb) {
                unsigned code;
                const float H = va_cell(t0[d], r0 > 0 && j0 > 0, r0 > 0, j0 > 0, d0, u0, h0, local, code);
                h0 = H;
                w0 |= code << (2 * (j0 & 15));
                if ((j0 & 15) == 15 || j0 == Tb - 1) { pred[r0 * 8 + (j0 >> 4)] = w0; w0 = 0; }
                if (H > best0) { best0 = H; bj0 = j0; }
                if (r0 == Ta - 1 && j0 == Tb - 1) hend = H;
            }
            if (on1 && j1 >= 0 && j1 < Tb) {
                unsigned code;
                const float H = va_cell(t1[d], j1 > 0, true, j1 > 0, d1, u1, h1, local, code);
                h1 = H;
                w1 |= code << (2 * (j1 & 15));
                if ((j1 & 15) == 15 || j1 == Tb - 1) { pred[r1 * 8 + (j1 >> 4)] = w1; w1 = 0; }
                if (H > best1) { best1 = H; bj1 = j1; }
                if (r1 == Ta - 1 && j1 == Tb - 1) hend = H;
            }
            d0 = u0;
            d1 = u1;
        }
        // the end cell: (Ta - 1, Tb - 1), or with local the largest H, then the lowest i, then the lowest j (key = 128 i + j)
        float v;
        int key;
        if (local) {
            v = on0 ? best0 : -INFINITY;
            key = on0 ? VA_FM * r0 + bj0 : INT_MAX;
            if (on1 && best1 > v) { v = best1; key = VA_FM * r1 + bj1; }  // equal: the lower row stays
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float v2 = __shfl_xor(v, o, 64);
                const int k2 = __shfl_xor(key, o, 64);
                if (v2 > v || (v2 == v && k2 < key)) { v = v2; key = k2; }
            }
        } else {
            const int owner = (Ta - 1) & 63;
            v = __shfl(hend, owner, 64);
            key = VA_FM * (Ta - 1) + Tb - 1;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");            // the lanes' words of pred, read by lane 0
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
            int i = key >> 7, j = key & 127, n = 0;
            while (n < 2 * VA_FM) {
                pi[n] = (unsigned char)i;
                pj[n] = (unsigned char)j;
                ++n;
                const unsigned code = (pred[i * 8 + (j >> 4)] >> (2 * (j & 15))) & 3u;
                if (code == 3) break;
                if (code != 2) --i;
                if (code != 1) --j;
            }
            s_len = n;
            s_score = v;
        }
    }
    __syncthreads();

    // ---- the path forward, and what every frame of b is matched with
    const int len = s_len;
    if (tid < 2 * F) {
        if (tid < len) {
            const int i = pi[len - 1 - tid], j = pj[len - 1 - tid];
            path_a[tid] = vfa[i];
            path_b[tid] = vfb[j];
            if (tid == 0 || pj[len - tid] != j) colstart[j] = tid;        // the first cell of column j
        } else {
            path_a[tid] = -1;
            path_b[tid] = -1;
        }
    }
    __syncthreads();
    if (tid < Tb) {
        int bi = -1;
        float be = -INFINITY;
        const int t0 = colstart[tid];
        if (t0 >= 0) {
            for (int t = t0; t < len && pj[len - 1 - t] == tid; ++t) {    // a's positions ascend along the run: the lowest among equals stays
                const int i = pi[len - 1 - t];
                const float e = tab[i * VA_TP + tid];
                if (bi < 0 || e > be) { be = e; bi = i; }
            }
        }
        const int g = vfb[tid];
        match[g] = bi < 0 ? -1 : vfa[bi];
        match_score[g] = bi < 0 ? -INFINITY : be;
    }
    if (tid == 0) { a.score[p] = s_score; a.path_len[p] = len; }
}

}  // namespace

extern "C" int univl_video_align_sizeof(void) { return (int)sizeof(UnivlVideoAlign); }

extern "C" int univl_video_align(const UnivlVideoAlign* d, hipStream_t stream) {
    UNIVL_ON_STREAM_DEVICE(stream);
    const char* who = "univl_video_align";
    // the gallery side, as univl_moment_localize asks it
    UNIVL_CHECK_ARG(d != nullptr, UNIVL_EINVAL, "%s: null descriptor", who);
    UNIVL_CHECK_ARG(d->H == VA_H, UNIVL_EINVAL, "%s: H=%d (must be 768)", who, d->H);
    UNIVL_CHECK_ARG(d->F >= 1 && d->F <= UNIVL_MOMENT_F_MAX, UNIVL_EINVAL, "%s: F=%d (1 <= F <= %d)", who, d->F, UNIVL_MOMENT_F_MAX);
    UNIVL_CHECK_ARG(d->N >= 1 && d->N <= INT_MAX / 16, UNIVL_EINVAL, "%s: N=%d (>= 1)", who, d->N);
    UNIVL_CHECK_ARG(d->frames && d->mask, UNIVL_EINVAL, "%s: null pointer (frames, mask)", who);
    UNIVL_CHECK_ARG(d->ld_row >= (int64_t)d->F * VA_H, UNIVL_EINVAL, "%s: ld_row=%lld (>= F * 768)", who, (long long)d->ld_row);
    UNIVL_CHECK_ARG(rows768_aligned(d->frames, d->ld_row), UNIVL_EALIGN, "%s: rows of frames must be 16-byte aligned", who);
    // the pairs
    UNIVL_CHECK_ARG(d->local == 0 || d->local == 1, UNIVL_EINVAL, "%s: local=%d (0 or 1)", who, d->local);
    UNIVL_CHECK_ARG(d->tau >= -FLT_MAX && d->tau <= FLT_MAX, UNIVL_EINVAL, "%s: tau=%g (finite)", who, (double)d->tau);
    UNIVL_CHECK_ARG(d->P >= 1 && d->C >= 1 && (int64_t)d->P * d->C * 2 * d->F <= INT_MAX, UNIVL_EINVAL,
                    "%s: P=%d C=%d (both >= 1, P * C * 2 F < 2^31)", who, d->P, d->C);
    UNIVL_CHECK_ARG(d->ref && d->rows && d->score && d->path_len && d->path_a && d->path_b && d->match && d->match_score, UNIVL_EINVAL,
                    "%s: null pointer (ref, rows, score, path_len, path_a, path_b, match, match_score)", who);
    VaArgs a;
    a.frames = d->frames; a.ld_row = (long)d->ld_row; a.mask = d->mask; a.ref = d->ref; a.rows = d->rows;
    a.N = d->N; a.F = d->F; a.C = d->C; a.local = d->local; a.tau = d->tau;
    a.score = d->score; a.path_len = d->path_len; a.path_a = d->path_a; a.path_b = d->path_b; a.match = d->match; a.match_score = d->match_score;
    static bool attr_done[UNIVL_MAX_DEVICES] = {};
    univl_allow_lds(video_align_kernel, VA_LDS, attr_done);
    hipLaunchKernelGGL(video_align_kernel, dim3((unsigned)(d->P * d->C)), dim3(256), VA_LDS, stream, a);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}
