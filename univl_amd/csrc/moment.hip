// Moment search on the device (include/univl_hip.h: univl_window_norms, univl_moment_localize, univl_moment_nbest, univl_step_align,
// univl_frame_segment): the best-matching window of frames of a gallery video for a pooled text vector, every window of the video
// scored in ONE launch -- or its n best windows after temporal non-maximum suppression -- for an ORDERED list of step vectors, the best
// in-order, non-overlapping windows of all of them at once -- and, from the video's side, the label (or none) of every frame out of a
// SET of label vectors.
//
// A window (s, L) covers frames s .. s + L - 1 of a row; u(s, L) is the sum of its frame vectors.  The score is the model's own --
// the masked mean over the window, L2-normalised unless use_mil, dotted with the query -- written without the mean:
//   normalising   (q . u) / max(|u|, 1e-12 L)          use_mil   (q . u) / L
//
// Five kernels, no host read, no LDS staging of frames, no float atomics, capturable:
//   norms      |u(s, L)| of every window of a row, a [F][F] table indexed (s, L - 1).  It depends on the video alone, so an index
//              computes it once per row.  ONE WAVE OWNS A START s: lane l keeps the 12 columns 4 l + 256 j + c (j < 3, c < 4) of the
//              running sum u(s, .) in registers, adds frame s + L - 1 to it (three 16-byte loads per lane, the next frame's already in
//              flight) and squares what it holds: 12 fmaf in column order, then the xor butterfly over the wave.  The frames of a row
//              are read F / 2 times over, from L2: a row is 144 KB at 48 frames and 393 KB at 128, more than the LDS holds, and a
//              column slice of it in LDS would need one cross-lane reduction per window AND slice instead of one per window.  A wave
//              takes start `slot` and then start F - 1 - slot, F + 1 steps in all, so the waves of a row finish together.
//   localize   one workgroup of 256 threads per (query, candidate) pair.  Wave w computes the frame products d_f = q . x_f of frames
//              w, w + 4, .. (the lane split and reduction tree of the norms kernel; four frames in flight per wave) into LDS.  Thread s
//              < F then owns start s: it grows the numerator d_s + .. + d_{s + L - 1} one frame at a time, stops at the first masked
//              frame or past lmax, divides by the table entry (or by L) and keeps its best window, the shortest among equals.  The F
//              starts' bests are reduced under the total order (score descending, start ascending, length ascending), so the shape of
//              that reduction cannot matter.
//   nbest      the same workgroup per pair, but SEVERAL windows of it: greedy temporal NMS over localize's own candidates.  Thread s
//              visits its windows as localize does and STORES every score in LDS -- length-major and triangular, row L holding the
//              F - L + 1 starts of length L, so that neighbouring threads touch neighbouring words; lengths lmin .. lmax only: at most
//              8 256 floats -- so the norm table is read once per window, not once per round.  A round: every thread walks its own
//              stored scores, marks what the previous pick suppresses (NaN: no live score equals it; the IoU test is in integers) and
//              keeps its best survivor; the F bests are reduced by localize's reduction, which EVERY wave runs on a double-buffered
//              copy, so all threads know the pick after ONE barrier per round.  No thread reads another's scores.  36 KB of LDS.
//   align     one workgroup of 256 threads per (step list, candidate) pair.  The same frame products for every step vector of the list,
//              d[k][f], into LDS: a wave holds four frames in registers and walks the list, so the row is read once per pair.  Then the
//              suffix programme of the contract, step n - 1 down to step 0: thread s < F grows start s's numerators exactly as localize
//              does, adds G[k+1][s + L] and keeps A[k][s] and its length; wave 0 scans A[k] from the right into G[k][t] and the lowest
//              start >= t that attains it; thread 0 walks forward from (k, t) = (0, 0) and writes the windows, re-growing each chosen
//              window's numerator (at most F additions in all).  Only the lengths and first starts are kept per step (one byte each):
//              26 KB of LDS, of which the products are 16.  Two barriers per step.
//   segment   one workgroup of 256 threads per (label set, candidate) pair.  The same frame products for every label vector, then every
//              thread turns its share of them into frame scores e(k, f) in place -- localize's visit of window (f, 1) -- and wave 0 runs
//              the suffix programme of the contract over the valid frames, last to first: lane y holds V[.][y], every lane the
//              background's value, so 64 labels and the background fit one wave; a frame costs one max butterfly, two ballots (who
//              attains the maximum, who stays) and one add.  The stay words and first maxima stay in registers, frame t's in lane
//              t & 63; the forward walk reads them by lane index.  Two barriers in all.  34 KB of LDS, of which the scores are 32 (pitch
//              129: the wave reads a column).
//
// PURITY.  |u(s, L)| is a function of the row's frames s .. s + L - 1 alone, d_f of (q, x_f) alone, a numerator of d_s .. d_{s+L-1}
// in ascending order: no value depends on the grid, the pair's place in the launch, the other pairs or deterministic mode.  Every sum
// is built BY EXTENSION from its start; nothing is a difference of prefix sums.
#include <float.h>
#include <limits.h>
#include <stddef.h>
#include "common.h"
#include "univl_hip.h"

namespace {

constexpr int MM_H = 768;                    // frame width (the hidden size)
constexpr int MM_NO_WINDOW = INT_MAX;        // the key of "no candidate window": sorts after every (start, length)

// the lane's 12 columns of one frame: 4 lane + 256 j + c
__device__ __forceinline__ void load12(f32x4_t (&x)[3], const float* frame, int lane) {
#pragma unroll
    for (int j = 0; j < 3; ++j) x[j] = *reinterpret_cast<const f32x4_t*>(frame + 4 * lane + 256 * j);
}

// sum over the wave's 768 columns of a * b: the lane's 12 products as one fmaf chain in column order, then the xor butterfly -- the
// ONLY reduction over columns in this file, so that every value built on it has one fixed order
__device__ __forceinline__ float dot768(const f32x4_t (&a)[3], const f32x4_t (&b)[3]) {
    float p = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int c = 0; c < 4; ++c) p = fmaf(a[j][c], b[j][c], p);
    }
    return wave_sum(p);
}

// table row s of one gallery row: |u(s, L)| for L = 1 .. F - s while every frame of the window is valid, 0 from the first window that
// holds a masked frame on, 0 for the lengths past the row's end
__device__ __forceinline__ void norms_from(const float* __restrict__ x, const int64_t* __restrict__ m, float* __restrict__ t, int F, int s,
                                           int lane) {
    f32x4_t u[3], cur[3], nxt[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) u[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    load12(cur, x + (long)s * MM_H, lane);
    int e = s;
    for (; e < F; ++e) {
        if (m[e] == 0) break;                                             // wave-uniform
        load12(nxt, x + (long)min(e + 1, F - 1) * MM_H, lane);            // the next frame (the last one again at the end: a valid address)
#pragma unroll
        for (int j = 0; j < 3; ++j) u[j] += cur[j];
        const float n2 = dot768(u, u);
        if (lane == 0) t[e - s] = sqrtf(n2);
#pragma unroll
        for (int j = 0; j < 3; ++j) cur[j] = nxt[j];
    }
    for (int c = e - s + lane; c < F; c += 64) t[c] = 0.f;
}

__global__ __launch_bounds__(256) void window_norms_kernel(const float* __restrict__ frames, long ld_row, const int64_t* __restrict__ mask,
                                                           float* __restrict__ wnorm, int F, int bpr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x / bpr, slot = (blockIdx.x % bpr) * 4 + wave;
    if (slot >= (F + 1) / 2) return;                                      // wave-uniform; the kernel has no barrier
    const float* x = frames + (long)row * ld_row;
    const int64_t* m = mask + (long)row * F;
    float* t = wnorm + (long)row * F * F;
    norms_from(x, m, t + (long)slot * F, F, slot, lane);
    const int s2 = F - 1 - slot;
    if (s2 != slot) norms_from(x, m, t + (long)s2 * F, F, s2, lane);
}

// The frame products of one gallery row x for n query rows: d[k * ldd + f] = q_k . x_f, k < n, f < F.  Wave w takes frames w, w + 4, ..,
// four of them in flight, and walks the query rows over what it holds: every frame is read once.  Each product is one dot768.
__device__ __forceinline__ void frame_products(const float* __restrict__ q, long ldq, int n, const float* __restrict__ x, int F, float* d, int ldd,
                                               int lane, int wave) {
    f32x4_t q0[3], qv[3];
    load12(q0, q, lane);                                                  // the first query row, often the only one, stays in registers
    for (int f0 = wave; f0 < F; f0 += 16) {
        f32x4_t xv[4][3];
#pragma unroll
        for (int r = 0; r < 4; ++r) load12(xv[r], x + (long)min(f0 + 4 * r, F - 1) * MM_H, lane);
        for (int k = 0; k < n; ++k) {
            if (k) {
                load12(qv, q + k * ldq, lane);
            } else {
#pragma unroll
                for (int j = 0; j < 3; ++j) qv[j] = q0[j];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float s = dot768(qv, xv[r]);
                if (lane == 0 && f0 + 4 * r < F) d[k * ldd + f0 + 4 * r] = s;
            }
        }
    }
}

// The candidate windows of start s, shortest first: visit(L, score) for every lmin <= L <= lmax whose frames s .. s + L - 1 are all valid.
// d: one query's frame products; t: the start's row of the norm table (unused with normalize = 0).  The numerator d_s + .. + d_{s+L-1} is
// grown one frame at a time, in this order and no other.
template <typename Visit>
__device__ __forceinline__ void windows_from(const float* d, const int* valid, const float* __restrict__ t, int F, int s, int lmin, int lmax,
                                             int normalize, Visit visit) {
    float num = 0.f;
    for (int e = s; e < F && e - s < lmax && valid[e]; ++e) {
        num += d[e];
        const int L = e - s + 1;
        if (L < lmin) continue;
        const float den = normalize ? fmaxf(t[L - 1], 1e-12f * (float)L) : (float)L;
        visit(L, num / den);
    }
}

struct LocArgs {
    const float* q; long ldq;
    const float* frames; long ld_row;
    const int64_t* mask;
    const float* wnorm;
    const int32_t* rows;
    int N, F, K, lmin, lmax, normalize;
    int32_t* start; int32_t* length; float* score;
};

// (score, key) order of the contract: larger score first, then the lower key = 256 start + length
__device__ __forceinline__ void keep_better(float& v, int& k, float v2, int k2) {
    if (v2 > v || (v2 == v && k2 < k)) { v = v2; k = k2; }
}

// the first under that order of the UNIVL_MOMENT_F_MAX starts' bests (bv, bk), in every lane of the calling wave: lane l folds starts
// l and l + 64, then the xor butterfly.  The order is total, so the shape of the reduction cannot matter.
__device__ __forceinline__ void best_start(const float* bv, const int* bk, int lane, float& v, int& k) {
    v = bv[lane];
    k = bk[lane];
    keep_better(v, k, bv[lane + 64], bk[lane + 64]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(v, o, 64);
        const int k2 = __shfl_xor(k, o, 64);
        keep_better(v, k, v2, k2);
    }
}

__global__ __launch_bounds__(256) void moment_localize_kernel(LocArgs a) {
    __shared__ float d[UNIVL_MOMENT_F_MAX];          // frame products
    __shared__ int valid[UNIVL_MOMENT_F_MAX];
    __shared__ float bv[UNIVL_MOMENT_F_MAX];         // every start's best window
    __shared__ int bk[UNIVL_MOMENT_F_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, F = a.F;
    const long p = blockIdx.x;
    const int cand = a.rows[p];
    if (cand < 0 || cand >= a.N) {                                        // block-uniform: nothing of the gallery is read
        if (tid == 0) { a.start[p] = -1; a.length[p] = 0; a.score[p] = -INFINITY; }
        return;
    }
    frame_products(a.q + (p / a.K) * a.ldq, a.ldq, 1, a.frames + (long)cand * a.ld_row, F, d, 0, lane, wave);
    if (tid < UNIVL_MOMENT_F_MAX) valid[tid] = (tid < F && a.mask[(long)cand * F + tid] != 0) ? 1 : 0;
    __syncthreads();

    if (tid < UNIVL_MOMENT_F_MAX) {
        float best = -INFINITY;
        int key = MM_NO_WINDOW;
        if (tid < F) {
            const int s = tid;
            const float* t = a.normalize ? a.wnorm + ((long)cand * F + s) * F : nullptr;
            windows_from(d, valid, t, F, s, a.lmin, a.lmax, a.normalize, [&](int L, float sc) {
                if (key == MM_NO_WINDOW || sc > best) { best = sc; key = 256 * s + L; }      // the shortest among equals stays
            });
        }
        bv[tid] = best; bk[tid] = key;
    }
    __syncthreads();
    if (wave == 0) {
        float v;
        int k;
        best_start(bv, bk, lane, v, k);
        if (lane == 0) {
            const bool none = k == MM_NO_WINDOW;
            a.start[p] = none ? -1 : k >> 8;
            a.length[p] = none ? 0 : k & 255;
            a.score[p] = none ? -INFINITY : v;
        }
    }
}

struct NbestArgs {
    LocArgs loc;                                     // start, length, score: [Nq, K, M]
    int M, iou_num, iou_den;
};

// does the pick (ps, pl) suppress the live window (s, L)?  Frames, in integers; the pick itself dies whatever the threshold
__device__ __forceinline__ bool suppressed(int s, int L, int ps, int pl, int num, int den) {
    const int inter = max(0, min(s + L, ps + pl) - max(s, ps));
    return (s == ps && L == pl) || den * inter > num * (L + pl - inter);
}

__global__ __launch_bounds__(256) void moment_nbest_kernel(NbestArgs b) {
    constexpr int FM = UNIVL_MOMENT_F_MAX;
    __shared__ float d[FM];                          // frame products
    __shared__ int valid[FM];
    __shared__ float bv[2][FM];                      // every start's best live window, of this round and of the one before
    __shared__ int bk[2][FM];
    __shared__ float sc[FM * (FM + 1) / 2];          // every window's score, length-major: row L holds starts 0 .. F - L       33 KB
    const LocArgs& a = b.loc;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, F = a.F, M = b.M;
    const long p = blockIdx.x;
    const int cand = a.rows[p];
    int32_t* start = a.start + p * M;
    int32_t* length = a.length + p * M;
    float* score = a.score + p * M;
    if (cand < 0 || cand >= a.N) {                                        // block-uniform: nothing of the gallery is read
        if (tid < M) { start[tid] = -1; length[tid] = 0; score[tid] = -INFINITY; }
        return;
    }
    frame_products(a.q + (p / a.K) * a.ldq, a.ldq, 1, a.frames + (long)cand * a.ld_row, F, d, 0, lane, wave);
    if (tid < FM) valid[tid] = (tid < F && a.mask[(long)cand * F + tid] != 0) ? 1 : 0;
    __syncthreads();

    // thread s owns start s: its windows are lengths lmin .. lend, word sc[row(L) + s] with row(lmin) = 0, row(L + 1) = row(L) + F - L + 1.
    // No other thread reads or writes them, so the rounds need no barrier for sc and nothing of it has to be cleared.
    const int s = tid, lmin = a.lmin;
    float best = -INFINITY;
    int key = MM_NO_WINDOW, lend = 0;
    if (s < F) {
        const float* t = a.normalize ? a.wnorm + ((long)cand * F + s) * F : nullptr;
        int at = s;
        windows_from(d, valid, t, F, s, lmin, a.lmax, a.normalize, [&](int L, float w) {
            sc[at] = w;
            at += F - L + 1;
            lend = L;
            if (key == MM_NO_WINDOW || w > best) { best = w; key = 256 * s + L; }        // moment_localize_kernel's fold: slot 0 is its triple
        });
    }
    for (int m = 0;; ++m) {
        if (tid < FM) { bv[m & 1][tid] = best; bk[m & 1][tid] = key; }
        __syncthreads();                                                  // one barrier per round: the round after next writes this buffer again
        float v;
        int k;
        best_start(bv[m & 1], bk[m & 1], lane, v, k);                     // every wave: all threads know the pick
        if (k == MM_NO_WINDOW) {                                          // block-uniform: nothing is alive
            if (tid >= m && tid < M) { start[tid] = -1; length[tid] = 0; score[tid] = -INFINITY; }
            return;
        }
        const int ps = k >> 8, pl = k & 255;
        if (tid == 0) { start[m] = ps; length[m] = pl; score[m] = v; }
        if (m + 1 == M) return;
        // the walk: what the pick suppresses dies (NaN: no live score equals it), the best survivor stays, the shortest among equals
        best = -INFINITY;
        key = MM_NO_WINDOW;
        // (no branch but the store's, so that the loop unrolls and several reads of sc are in flight; a dead window may die again)
#pragma unroll 4
        for (int L = lmin, at = s; L <= lend; at += F - L + 1, ++L) {
            const float w = sc[at];
            const bool kill = suppressed(s, L, ps, pl, b.iou_num, b.iou_den);
            if (kill) sc[at] = NAN;
            const bool take = !kill && w == w && (key == MM_NO_WINDOW || w > best);
            best = take ? w : best;
            key = take ? 256 * s + L : key;
        }
    }
}

struct AlignArgs {
    const float* q; long ldq;
    const float* frames; long ld_row;
    const int64_t* mask;
    const float* wnorm;
    const int32_t* counts; const int32_t* rows;
    int N, F, C, K, lmin, lmax, normalize;
    int32_t* start; int32_t* length; float* score; float* total;
};

// suffix maximum with its first position: the pair at the lower index keeps its place unless the other value is strictly larger
__device__ __forceinline__ void keep_first_max(float& v, int& i, float v2, int i2) {
    if (v2 > v) { v = v2; i = i2; }
}

__global__ __launch_bounds__(256) void step_align_kernel(AlignArgs a) {
    constexpr int FM = UNIVL_MOMENT_F_MAX, KM = UNIVL_STEP_K_MAX;
    __shared__ float d[KM * FM];                     // d[k][f] = q_k . x_f                                      16 KB
    __shared__ int valid[FM];
    __shared__ float A[FM];                          // A[k][.] of the step at hand
    __shared__ float G[2][FM + 1];                   // G[k][.] and G[k + 1][.], t = 0 .. FM
    __shared__ unsigned char len[KM * FM];           // the length behind A[k][s]                                  4 KB
    __shared__ unsigned char first[KM * FM];         // the lowest s >= t with A[k][s] == G[k][t]                  4 KB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, F = a.F, K = a.K;
    const long p = blockIdx.x, list = p / a.C;
    const int cand = a.rows[p], n = a.counts[list];
    int32_t* start = a.start + p * K;
    int32_t* length = a.length + p * K;
    float* score = a.score + p * K;
    if (cand < 0 || cand >= a.N || n < 1 || n > K) {                      // block-uniform: nothing of the gallery or of q is read
        if (tid < K) { start[tid] = -1; length[tid] = 0; score[tid] = -INFINITY; }
        if (tid == 0) a.total[p] = -INFINITY;
        return;
    }
    frame_products(a.q + list * K * a.ldq, a.ldq, n, a.frames + (long)cand * a.ld_row, F, d, FM, lane, wave);
    if (tid < FM) valid[tid] = (tid < F && a.mask[(long)cand * F + tid] != 0) ? 1 : 0;
    if (tid <= FM) { G[n & 1][tid] = 0.f; G[(n & 1) ^ 1][tid] = -INFINITY; }       // T_n = 0 wherever the last window ends
    __syncthreads();

    const float* trow = a.normalize && tid < F ? a.wnorm + ((long)cand * F + tid) * F : nullptr;
    for (int k = n - 1; k >= 0; --k) {
        const float* gn = G[(k + 1) & 1];
        float* gk = G[k & 1];
        if (tid < FM) {
            float best = -INFINITY;                                       // no window, or none with steps k + 1 .. after it
            int bl = 0;
            if (tid < F) {
                windows_from(d + k * FM, valid, trow, F, tid, a.lmin, a.lmax, a.normalize, [&](int L, float w) {
                    const float v = w + gn[tid + L];
                    if (v > best) { best = v; bl = L; }                   // the shortest among equals stays
                });
            }
            A[tid] = best; len[k * FM + tid] = (unsigned char)bl;
        }
        __syncthreads();
        if (wave == 0) {                                                  // lane l holds starts l and l + 64
            float v0 = A[lane], v1 = A[lane + 64];
            int i0 = lane, i1 = lane + 64;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const float u0 = __shfl_down(v0, o, 64), u1 = __shfl_down(v1, o, 64);
                const int j0 = __shfl_down(i0, o, 64), j1 = __shfl_down(i1, o, 64);
                if (lane + o < 64) { keep_first_max(v0, i0, u0, j0); keep_first_max(v1, i1, u1, j1); }
            }
            keep_first_max(v0, i0, __shfl(v1, 0, 64), __shfl(i1, 0, 64)); // the upper half follows every start of the lower
            gk[lane] = v0; gk[lane + 64] = v1;
            first[k * FM + lane] = (unsigned char)i0; first[k * FM + lane + 64] = (unsigned char)i1;
            if (lane == 0) gk[FM] = -INFINITY;                            // a step that would begin past the last frame
        }
        __syncthreads();
    }

    const float tot = G[0][0];
    const bool ok = tot > -INFINITY;                                      // all or nothing
    if (tid < K && (tid >= n || !ok)) { start[tid] = -1; length[tid] = 0; score[tid] = -INFINITY; }
    if (tid == 0) {
        a.total[p] = ok ? tot : -INFINITY;
        for (int k = 0, t = 0; ok && k < n; ++k) {
            const int s = first[k * FM + t], L = len[k * FM + s];
            const float* tr = a.normalize ? a.wnorm + ((long)cand * F + s) * F : nullptr;
            float w = 0.f;
            windows_from(d + k * FM, valid, tr, F, s, L, L, a.normalize, [&](int, float sc) { w = sc; });
            start[k] = s; length[k] = L; score[k] = w;
            t = s + L;
        }
    }
}

struct SegArgs {
    const float* q; long ldq;
    const float* frames; long ld_row;
    const int64_t* mask;
    const float* wnorm;
    const int32_t* counts; const int32_t* rows;
    int N, F, C, K, normalize;
    float lambda, bg;
    int32_t* label; float* score; float* total; int32_t* nseg;
};

__global__ __launch_bounds__(256) void frame_segment_kernel(SegArgs a) {
    constexpr int FM = UNIVL_MOMENT_F_MAX, KM = UNIVL_SEGMENT_K_MAX;
    constexpr int LD = FM + 1;                       // odd pitch: wave 0 reads a COLUMN of e (lane y, frame f) from 64 different banks
    __shared__ float e[KM * LD];                     // d[k][f] = q_k . x_f, then e(k, f) in place                  32.25 KB
    __shared__ float w1[FM];                         // the one-frame entries of the row's norm table
    __shared__ int valid[FM];
    __shared__ int vf[FM];                           // vf[t] = f_t, the t-th valid frame
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, F = a.F;
    const long p = blockIdx.x, set = p / a.C;
    const int cand = a.rows[p], n = a.counts[set];
    int32_t* label = a.label + p * F;
    float* score = a.score + p * F;
    if (cand < 0 || cand >= a.N || n < 1 || n > a.K) {                    // block-uniform: nothing of the gallery or of q is read
        if (tid < F) { label[tid] = -2; score[tid] = -INFINITY; }
        if (tid == 0) { a.total[p] = -INFINITY; a.nseg[p] = 0; }
        return;
    }
    frame_products(a.q + set * a.K * a.ldq, a.ldq, n, a.frames + (long)cand * a.ld_row, F, e, LD, lane, wave);
    if (tid < FM) {
        const int ok = (tid < F && a.mask[(long)cand * F + tid] != 0) ? 1 : 0;
        valid[tid] = ok;
        w1[tid] = (ok && a.normalize) ? a.wnorm[((long)cand * F + tid) * F] : 0.f;
        if (tid < F && !ok) { label[tid] = -2; score[tid] = -INFINITY; }  // a masked frame: no other thread writes it
    }
    __syncthreads();

    // e(k, f) over d[k][f] in place: the visit univl_moment_localize makes of window (f, 1), so the score is its score bit for bit
    for (int i = tid; i < n * F; i += 256) {
        const int k = i / F, f = i - k * F;
        float* row = e + k * LD;
        windows_from(row, valid, w1 + f, F, f, 1, 1, a.normalize, [&](int, float w) { row[f] = w; });
    }
    unsigned long long b0 = 0, b1 = 0;                                    // the valid frames, as wave 0 sees them
    if (wave == 0) {
        const int v0 = valid[lane], v1 = valid[lane + 64];
        b0 = __ballot(v0);
        b1 = __ballot(v1);
        const unsigned long long below = (1ull << lane) - 1;
        if (v0) vf[__popcll(b0 & below)] = lane;
        if (v1) vf[__popcll(b0) + __popcll(b1 & below)] = lane + 64;
    }
    __syncthreads();
    if (wave != 0) return;
    const int T = __popcll(b0) + __popcll(b1);
    if (T == 0) {                                                         // wave-uniform: nothing to label
        if (lane == 0) { a.total[p] = -INFINITY; a.nseg[p] = 0; }
        return;
    }

    // The suffix programme.  Lane y < n holds V[.][y]; every lane carries the background's V[.][n].  Frame t leaves two words behind,
    // in lane t & 63 (w0, m0 for t < 64, w1, m1 above): the ballot of stay[t][.] and a[t] + 128 * stay[t][n].
    const bool mine = lane < n;
    const float* col = e + lane * LD;                                     // read by the lanes y < n alone
    const float lambda = a.lambda, bg = a.bg;
    float V = mine ? col[vf[T - 1]] : -INFINITY, Vb = bg, M;
    int arg;
    unsigned long long s0 = 0, s1 = 0;
    int m0 = 0, m1 = 0;
    // M[t] and a[t]: the maximum over the wave is exact, so the lowest lane that holds it is the lowest label that attains it -- the
    // (value, index) fold of keep_first_max, with one value per exchange; the background enters last and only if strictly larger
    auto top = [&]() {
        M = wave_max(V);
        const unsigned long long at = __ballot(mine && V == M);
        arg = at ? __ffsll(at) - 1 : n;                                   // (no lane: NaN input, unspecified -- but never an index outside e)
        if (Vb > M) { M = Vb; arg = n; }
    };
    auto keep = [&](int t, unsigned long long word, int m) {
        if (lane == (t & 63)) {
            if (t < 64) { s0 = word; m0 = m; } else { s1 = word; m1 = m; }
        }
    };
    top();
    keep(T - 1, 0ull, arg);
    float enext = (mine && T >= 2) ? col[vf[T - 2]] : 0.f;
    for (int t = T - 2; t >= 0; --t) {
        const float ecur = enext;
        if (mine && t > 0) enext = col[vf[t - 1]];                        // the next frame's score is in flight during this one's fold
        const float thr = M - lambda;
        const bool sb = Vb >= thr;                                        // a tie stays
        const unsigned long long word = __ballot(mine && V >= thr);
        V = mine ? ecur + fmaxf(V, thr) : -INFINITY;
        Vb = bg + fmaxf(Vb, thr);
        top();
        keep(t, word, arg | (sb ? 128 : 0));
    }

    // the walk, wave-uniform: lane t & 63 keeps y_t
    int y = 0, prev = -1, runs = 0, y0 = 0, y1 = 0, pm = 0;
    unsigned long long pw = 0;
    for (int t = 0; t < T; ++t) {
        const unsigned long long word = t < 64 ? __shfl(s0, t, 64) : __shfl(s1, t - 64, 64);
        const int m = t < 64 ? __shfl(m0, t, 64) : __shfl(m1, t - 64, 64);
        const bool stay = t > 0 && (y == n ? (pm >> 7) & 1 : (int)((pw >> y) & 1));
        if (!stay) y = m & 127;
        runs += (y != n && y != prev) ? 1 : 0;
        prev = y; pw = word; pm = m;
        if (lane == (t & 63)) {
            if (t < 64) y0 = y; else y1 = y;
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int t = lane + 64 * h, yy = h ? y1 : y0;
        if (t < T) {
            const int f = vf[t];
            label[f] = yy == n ? -1 : yy;
            score[f] = yy == n ? bg : e[yy * LD + f];
        }
    }
    if (lane == 0) { a.total[p] = M; a.nseg[p] = runs; }
}

// the checks every entry point shares: the descriptor itself and its gallery side (UnivlMoment, UnivlStepAlign and UnivlFrameSegment
// name it alike)
template <typename D>
int check_gallery(const char* who, const D* d) {
    UNIVL_CHECK_ARG(d != nullptr, UNIVL_EINVAL, "%s: null descriptor", who);
    UNIVL_CHECK_ARG(d->H == MM_H, UNIVL_EINVAL, "%s: H=%d (must be 768)", who, d->H);
    UNIVL_CHECK_ARG(d->F >= 1 && d->F <= UNIVL_MOMENT_F_MAX, UNIVL_EINVAL, "%s: F=%d (1 <= F <= %d)", who, d->F, UNIVL_MOMENT_F_MAX);
    UNIVL_CHECK_ARG(d->N >= 1 && d->N <= INT_MAX / 16, UNIVL_EINVAL, "%s: N=%d (>= 1)", who, d->N);
    UNIVL_CHECK_ARG(d->normalize == 0 || d->normalize == 1, UNIVL_EINVAL, "%s: normalize=%d (0 or 1)", who, d->normalize);
    UNIVL_CHECK_ARG(d->frames && d->mask, UNIVL_EINVAL, "%s: null pointer (frames, mask)", who);
    UNIVL_CHECK_ARG(d->ld_row >= (int64_t)d->F * MM_H, UNIVL_EINVAL, "%s: ld_row=%lld (>= F * 768)", who, (long long)d->ld_row);
    UNIVL_CHECK_ARG(rows768_aligned(d->frames, d->ld_row), UNIVL_EALIGN, "%s: rows of frames must be 16-byte aligned", who);
    return UNIVL_OK;
}

// what the two localisers ask of the lengths searched, the norm table and the query rows
template <typename D>
int check_search(const char* who, const D* d) {
    UNIVL_CHECK_ARG(d->lmin >= 1 && d->lmin <= d->lmax && d->lmax <= d->F, UNIVL_EINVAL, "%s: lmin=%d lmax=%d (1 <= lmin <= lmax <= F=%d)", who,
                    d->lmin, d->lmax, d->F);
    UNIVL_CHECK_ARG(!d->normalize || d->wnorm != nullptr, UNIVL_EINVAL, "%s: null pointer (wnorm with normalize)", who);
    UNIVL_CHECK_ARG(rows768_pitch(d->ldq), UNIVL_EINVAL, "%s: ldq=%lld (>= 768)", who, (long long)d->ldq);
    UNIVL_CHECK_ARG(rows768_aligned(d->q, d->ldq), UNIVL_EALIGN, "%s: rows of q must be 16-byte aligned", who);
    return UNIVL_OK;
}

}  // namespace

extern "C" int univl_moment_sizeof(void) { return (int)sizeof(UnivlMoment); }

extern "C" int univl_window_norms(const UnivlMoment* d, hipStream_t stream) {
    UNIVL_ON_STREAM_DEVICE(stream);
    const int rc = check_gallery("univl_window_norms", d);
    if (rc != UNIVL_OK) return rc;
    UNIVL_CHECK_ARG(d->wnorm != nullptr, UNIVL_EINVAL, "univl_window_norms: null pointer (wnorm)");
    const int bpr = ((d->F + 1) / 2 + 3) / 4;                             // four waves per block, a wave per pair of starts
    hipLaunchKernelGGL(window_norms_kernel, dim3((unsigned)d->N * bpr), dim3(256), 0, stream, d->frames, (long)d->ld_row, d->mask, d->wnorm, d->F,
                       bpr);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}

extern "C" int univl_moment_localize(const UnivlMoment* d, hipStream_t stream) {
    UNIVL_ON_STREAM_DEVICE(stream);
    const char* who = "univl_moment_localize";
    int rc = check_gallery(who, d);
    if (rc != UNIVL_OK) return rc;
    UNIVL_CHECK_ARG(d->Nq >= 1 && d->K >= 1 && (int64_t)d->Nq * d->K <= INT_MAX, UNIVL_EINVAL, "%s: Nq=%d K=%d (both >= 1, Nq * K < 2^31)", who,
                    d->Nq, d->K);
    UNIVL_CHECK_ARG(d->q && d->rows && d->start && d->length && d->score, UNIVL_EINVAL, "%s: null pointer (q, rows, start, length, score)", who);
    rc = check_search(who, d);
    if (rc != UNIVL_OK) return rc;
    LocArgs a;
    a.q = d->q; a.ldq = (long)d->ldq; a.frames = d->frames; a.ld_row = (long)d->ld_row; a.mask = d->mask; a.wnorm = d->wnorm; a.rows = d->rows;
    a.N = d->N; a.F = d->F; a.K = d->K; a.lmin = d->lmin; a.lmax = d->lmax; a.normalize = d->normalize;
    a.start = d->start; a.length = d->length; a.score = d->score;
    hipLaunchKernelGGL(moment_localize_kernel, dim3((unsigned)(d->Nq * d->K)), dim3(256), 0, stream, a);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}

extern "C" int univl_moment_nbest_sizeof(void) { return (int)sizeof(UnivlMomentNbest); }

extern "C" int univl_moment_nbest(const UnivlMomentNbest* d, hipStream_t stream) {
    UNIVL_ON_STREAM_DEVICE(stream);
    const char* who = "univl_moment_nbest";
    int rc = check_gallery(who, d);
    if (rc != UNIVL_OK) return rc;
    UNIVL_CHECK_ARG(d->M >= 1 && d->M <= UNIVL_MOMENT_NBEST_MAX, UNIVL_EINVAL, "%s: M=%d (1 <= M <= %d)", who, d->M, UNIVL_MOMENT_NBEST_MAX);
    UNIVL_CHECK_ARG(d->iou_den >= 1 && d->iou_den <= 1024, UNIVL_EINVAL, "%s: iou_den=%d (1 <= iou_den <= 1024)", who, d->iou_den);
    UNIVL_CHECK_ARG(d->iou_num >= 0 && d->iou_num <= d->iou_den, UNIVL_EINVAL, "%s: iou_num=%d (0 <= iou_num <= iou_den=%d)", who, d->iou_num,
                    d->iou_den);
    UNIVL_CHECK_ARG(d->Nq >= 1 && d->K >= 1 && (int64_t)d->Nq * d->K * d->M <= INT_MAX, UNIVL_EINVAL,
                    "%s: Nq=%d K=%d (both >= 1, Nq * K * M < 2^31)", who, d->Nq, d->K);
    UNIVL_CHECK_ARG(d->q && d->rows && d->start && d->length && d->score, UNIVL_EINVAL, "%s: null pointer (q, rows, start, length, score)", who);
    rc = check_search(who, d);
    if (rc != UNIVL_OK) return rc;
    NbestArgs b;
    LocArgs& a = b.loc;
    a.q = d->q; a.ldq = (long)d->ldq; a.frames = d->frames; a.ld_row = (long)d->ld_row; a.mask = d->mask; a.wnorm = d->wnorm; a.rows = d->rows;
    a.N = d->N; a.F = d->F; a.K = d->K; a.lmin = d->lmin; a.lmax = d->lmax; a.normalize = d->normalize;
    a.start = d->start; a.length = d->length; a.score = d->score;
    b.M = d->M; b.iou_num = d->iou_num; b.iou_den = d->iou_den;
    hipLaunchKernelGGL(moment_nbest_kernel, dim3((unsigned)(d->Nq * d->K)), dim3(256), 0, stream, b);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}

extern "C" int univl_step_align_sizeof(void) { return (int)sizeof(UnivlStepAlign); }

extern "C" int univl_frame_segment_sizeof(void) { return (int)sizeof(UnivlFrameSegment); }

extern "C" int univl_frame_segment(const UnivlFrameSegment* d, hipStream_t stream) {
    UNIVL_ON_STREAM_DEVICE(stream);
    const char* who = "univl_frame_segment";
    const int rc = check_gallery(who, d);
    if (rc != UNIVL_OK) return rc;
    UNIVL_CHECK_ARG(d->K >= 1 && d->K <= UNIVL_SEGMENT_K_MAX, UNIVL_EINVAL, "%s: K=%d (1 <= K <= %d)", who, d->K, UNIVL_SEGMENT_K_MAX);
    UNIVL_CHECK_ARG(d->Nl >= 1 && d->C >= 1 && (int64_t)d->Nl * d->C <= INT_MAX, UNIVL_EINVAL, "%s: Nl=%d C=%d (both >= 1, Nl * C < 2^31)", who,
                    d->Nl, d->C);
    UNIVL_CHECK_ARG(d->switch_penalty >= 0.f && d->switch_penalty <= FLT_MAX, UNIVL_EINVAL, "%s: switch_penalty=%g (finite, >= 0)", who,
                    (double)d->switch_penalty);
    UNIVL_CHECK_ARG(d->background <= FLT_MAX, UNIVL_EINVAL, "%s: background=%g (a number or -inf)", who, (double)d->background);
    UNIVL_CHECK_ARG(d->q && d->counts && d->rows && d->label && d->score && d->total && d->nseg, UNIVL_EINVAL,
                    "%s: null pointer (q, counts, rows, label, score, total, nseg)", who);
    UNIVL_CHECK_ARG(!d->normalize || d->wnorm != nullptr, UNIVL_EINVAL, "%s: null pointer (wnorm with normalize)", who);
    UNIVL_CHECK_ARG(rows768_pitch(d->ldq), UNIVL_EINVAL, "%s: ldq=%lld (>= 768)", who, (long long)d->ldq);
    UNIVL_CHECK_ARG(rows768_aligned(d->q, d->ldq), UNIVL_EALIGN, "%s: rows of q must be 16-byte aligned", who);
    SegArgs a;
    a.q = d->q; a.ldq = (long)d->ldq; a.frames = d->frames; a.ld_row = (long)d->ld_row; a.mask = d->mask; a.wnorm = d->wnorm;
    a.counts = d->counts; a.rows = d->rows;
    a.N = d->N; a.F = d->F; a.C = d->C; a.K = d->K; a.normalize = d->normalize;
    a.lambda = d->switch_penalty; a.bg = d->background;
    a.label = d->label; a.score = d->score; a.total = d->total; a.nseg = d->nseg;
    hipLaunchKernelGGL(frame_segment_kernel, dim3((unsigned)(d->Nl * d->C)), dim3(256), 0, stream, a);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}

extern "C" int univl_step_align(const UnivlStepAlign* d, hipStream_t stream) {
    UNIVL_ON_STREAM_DEVICE(stream);
    const char* who = "univl_step_align";
    int rc = check_gallery(who, d);
    if (rc != UNIVL_OK) return rc;
    UNIVL_CHECK_ARG(d->K >= 1 && d->K <= UNIVL_STEP_K_MAX, UNIVL_EINVAL, "%s: K=%d (1 <= K <= %d)", who, d->K, UNIVL_STEP_K_MAX);
    UNIVL_CHECK_ARG(d->Nl >= 1 && d->C >= 1 && (int64_t)d->Nl * d->C <= INT_MAX, UNIVL_EINVAL, "%s: Nl=%d C=%d (both >= 1, Nl * C < 2^31)", who,
                    d->Nl, d->C);
    UNIVL_CHECK_ARG(d->q && d->counts && d->rows && d->start && d->length && d->score && d->total, UNIVL_EINVAL,
                    "%s: null pointer (q, counts, rows, start, length, score, total)", who);
    rc = check_search(who, d);
    if (rc != UNIVL_OK) return rc;
    AlignArgs a;
    a.q = d->q; a.ldq = (long)d->ldq; a.frames = d->frames; a.ld_row = (long)d->ld_row; a.mask = d->mask; a.wnorm = d->wnorm;
    a.counts = d->counts; a.rows = d->rows;
    a.N = d->N; a.F = d->F; a.C = d->C; a.K = d->K; a.lmin = d->lmin; a.lmax = d->lmax; a.normalize = d->normalize;
    a.start = d->start; a.length = d->length; a.score = d->score; a.total = d->total;
    hipLaunchKernelGGL(step_align_kernel, dim3((unsigned)(d->Nl * d->C)), dim3(256), 0, stream, a);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}
