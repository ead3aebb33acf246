// K16: the tied vocabulary classifier fused with an ONLINE log-softmax cross entropy -- in training the [tokens, 30522]
// logits never exist in memory.  Included by gemm.hip (needs Tile / tile_mma / gemm_acc_only / pair_tile / smem_raw).
//
// Reference: BertLMPredictionHead.forward (module_bert.py:327-330: h . E_word^T + bias, E_word the tied 30522 x 768 table), its decoder
// copy (module_decoder.py:180-183), and CrossEntropyLoss(ignore_index=-1) on the result (modeling.py:253, 275).
//
// Forward  (vocab_ce_kernel<T, false, TOP>): the product is walked in 128 x 128 tiles (the K loop of gemm_tile, gemm_acc_only); a tile's
//   epilogue reduces its logits to one (max, sum of exp(logit - max)) pair per row -- 16-lane shuffles inside a wave, LDS across the waves
//   of the column direction -- and writes it to partial[row][column tile]; the one lane that owns (row, label[row]) stores that logit.
//   TOP = false, training: vocab_ce_rows_kernel then folds a row's 239 pairs into its log-sum-exp (a wave per row, fixed order) and
//   vocab_ce_loss_kernel sums lse - label logit over the rows that count (one workgroup, fixed order: the loss is bit-reproducible in
//   every mode).
//   TOP = true, scoring (vocab_score.h): the column of the maximum travels beside it through every level, under the order of ranked.h
//   (of equal logits the LOWER column), into partial_top[row][column tile]; vocab_score_rows_kernel folds the triples.  The pairs, and so
//   lse, are the same bits in both forms.
// Backward (vocab_ce_kernel<T, true>): the same product again; the epilogue turns a logit into
//   (exp(logit - lse[row]) - [col == label[row]]) * gout / n_valid   (0 on ignored rows)
//   and stores it in the compute type: the matrix autograd calls dlogits, which the two existing backward products consume
//   (dh = dlogits . E, dE += dlogits^T . h).  What K16 removes per step at 512 tokens: the 62 MB fp32 logits (written by the product, read
//   by the loss kernel), the loss kernel's 31 MB dlogits write + the scale pass over them; what it adds: one more product.
// Weighted (univl_vocab_ce_weighted_fwd / _bwd, WEIGHTED = true): caption c = row / seq_len carries one fp32 weight w.  The forward's tile
//   kernel is the unweighted instantiation itself (lse is the same bits); vocab_ce_rows_weighted_kernel stores w * (lse - label logit) and
//   vocab_ce_loss_kernel sums that, still divided by the number of counting rows.  The backward instantiation vocab_ce_kernel<T, true, false,
//   WGN, true> loads w once per row of the tile (16 loads per thread, each lane of a row's 16-lane group the same address) and uses
//   w * (gout / n_valid) where the unweighted code uses gout / n_valid: with w = 1.0f the same bits.  A row of weight 0 is stored as zeros
//   like an ignored one.  No LDS, no barrier, no new tile walk; the unweighted instantiations do not see the weight.
// Smoothed (univl_vocab_ce_smooth_fwd / _bwd, SMOOTH = true): CrossEntropyLoss(label_smoothing = eps) -- the target is (1 - eps) on the label
//   plus eps / V on every column -- with the weighted form's optional weight per caption (null seq_weight: 1).  The loss needs one more
//   number per row, the sum S of its V logits.  Forward vocab_ce_kernel<T, false, false, WGN, false, true>: the (max, sum exp) path of the
//   epilogue is the training one, statement for statement (lse and the label logit are the same bits); beside it a lane sums its valid
//   logits in ascending column order (a column >= V adds 0, not -inf), the 16-lane xor steps follow, lane 0 leaves the sum in the third
//   [WGN][128] plane of the freed stages (the plane TOP keeps its columns in: the two forms never meet), and the thread that folds a row's
//   column waves adds them in ascending order into partial_sum[row][column tile].  vocab_ce_rows_smooth_kernel folds the pairs exactly as
//   the training row fold does, sums the slots of partial_sum lane-strided and then by the xor steps, and stores
//   w * fma(1 - eps, lse - label logit, eps * (lse - S / V)); vocab_ce_loss_kernel sums that as ever.  Backward vocab_ce_kernel<T, true,
//   false, WGN, true, true>: (exp(logit - lse) - (1 - eps) [col == label] - eps / V) * (w * (gout / n_valid)), one more subtract per
//   element.  Every sum is in a fixed order and there is no atomic: bit-reproducible in every mode, and a row's outputs do not depend on
//   the number of row tiles.  At eps = 0 the entry points launch the plain / the weighted form itself (gemm.hip), so those bits are theirs
//   by construction.  The training, weighted and scoring instantiations read neither partial_sum nor smoothing: `if constexpr (SMOOTH)`
//   around every use, and their instructions are unchanged.
#pragma once
#include "ranked.h"

struct VocabCeArgs {
    const void* X; long ldx;            // [rows, K] head output (compute type), K-major
    const void* E; long lde;            // [V, K] tied word table (compute type), K-major
    const float* bias;                  // [V] or null
    int rows, V, K;
    const int64_t* labels; int ignore;
    float* partial; int slots;          // [rows, slots, 2]
    int* partial_top;                   // [rows, slots]     (TOP)
    float* label_logit;                 // [rows]
    const float* lse;                   // [rows]            (backward)
    const float* scal;                  // scal[0] = n_valid (backward)
    const float* gout;                  // device scalar or null (= 1)
    void* dl; long lddl;                // [rows, lddl] compute type (backward)
    int nx, ny;
    const float* seq_weight; int seq_len;  // [rows / seq_len]  (WEIGHTED backward; SMOOTH: null = every weight 1)
    float* partial_sum;                 // [rows, slots]     (SMOOTH forward)
    float smoothing;                    // eps               (SMOOTH backward)
};

// One more (value, column) for a running maximum (m, c), offered in ASCENDING column order: the strict > keeps the lower column of equal
// values, and an empty maximum (-inf over no valid column) keeps RANK_NONE.  Without TOP there is no column and the maximum is fmaxf's.
template <bool TOP>
__device__ __forceinline__ void vocab_max_take(float& m, int& c, float v, int j) {
    if constexpr (TOP) { if (v > m) { m = v; c = j; } }
    else m = fmaxf(m, v);
}
// the maximum of every aligned group of W lanes, with its column under `better`
template <bool TOP, int W>
__device__ __forceinline__ void vocab_max_lanes(float& m, int& c) {
    if constexpr (TOP) wave_best<W>(m, c);
    else {
#pragma unroll
        for (int o = 1; o < W; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    }
}

template <typename T, bool BWD, bool TOP, int WGN, bool WEIGHTED = false, bool SMOOTH = false>
__global__ __launch_bounds__(128 * WGN, 2) void vocab_ce_kernel(VocabCeArgs a) {
    static_assert(!(BWD && TOP), "the arg-max column belongs to the forward");
    static_assert(BWD || !WEIGHTED, "the weighted forward is the unweighted tile kernel: the weight enters in the row fold");
    static_assert(!(SMOOTH && TOP), "the row sum and the arg-max column share the third LDS plane");
    static_assert(!(SMOOTH && BWD) || WEIGHTED, "the smoothed backward is a weighted one (null seq_weight: every weight 1)");
    constexpr int BM = 128, BN = 128, WGM = 2, NC = 2;
    constexpr int WM = BM / WGM, WN = BN / WGN, MI = WM / 16, NI = WN / 16;
    int bx, by, bz;
    pair_tile((int)blockIdx.x, a.nx * a.ny, a.nx, a.ny, 1, UNIVL_GEMM_XCD_MAP, 8, bx, by, bz);
    const int m0 = by * BM, n0 = bx * BN;
    f32x4_t acc[MI][NI];
    gemm_acc_only<T, false, false, BM, BN, NC, WGM, WGN>(reinterpret_cast<const T*>(a.X), a.ldx, reinterpret_cast<const T*>(a.E), a.lde, a.rows, a.V,
                                                         a.K, m0, n0, acc, smem_raw);
    // (the K loop ends with a barrier: the stages are free)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, i = lane & 15;
    const int wm0 = (wave / WGN) * WM, wn0 = (wave % WGN) * WN, wn = wave % WGN;
    int col[NI];
    bool vcol[NI];
    float bv[NI];
#pragma unroll
    for (int b = 0; b < NI; ++b) {
        col[b] = n0 + wn0 + 16 * b + i;
        vcol[b] = col[b] < a.V;
        bv[b] = (a.bias && vcol[b]) ? a.bias[col[b]] : 0.0f;
    }
    if constexpr (!BWD) {
        float* red = reinterpret_cast<float*>(smem_raw);          // [WGN][BM][2]
        int* redc = reinterpret_cast<int*>(red + WGN * BM * 2);   // [WGN][BM]   (TOP)
        float* reds = red + WGN * BM * 2;                         // [WGN][BM]   (SMOOTH: the same plane, never both)
#pragma unroll
        for (int ma = 0; ma < MI; ++ma)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rl = wm0 + 16 * ma + 4 * g + r, row = m0 + rl;
                const long lab = row < a.rows ? (long)a.labels[row] : -2;       // a label outside [0, V) matches no column
                float v[NI], m = -INFINITY;
                [[maybe_unused]] float t = 0.0f;                               // SMOOTH: the sum of the logits, a column >= V adds 0
                int c = RANK_NONE;
#pragma unroll
                for (int b = 0; b < NI; ++b) {
                    v[b] = vcol[b] ? acc[ma][b][r] + bv[b] : -INFINITY;
                    vocab_max_take<TOP>(m, c, v[b], col[b]);
                    if (vcol[b] && (long)col[b] == lab) a.label_logit[row] = v[b];
                    if constexpr (SMOOTH) t += vcol[b] ? v[b] : 0.0f;            // the lane's columns, ascending
                }
                vocab_max_lanes<TOP, 16>(m, c);
                float s = 0.0f;
                if (m > -INFINITY) {
#pragma unroll
                    for (int b = 0; b < NI; ++b) s += __expf(v[b] - m);     // exp(-inf) = 0 for the columns beyond V
                }
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o, 64);
                if constexpr (SMOOTH) {
#pragma unroll
                    for (int o = 1; o < 16; o <<= 1) t += __shfl_xor(t, o, 64);
                }
                if (i == 0) {
                    red[(wn * BM + rl) * 2] = m; red[(wn * BM + rl) * 2 + 1] = s;
                    if constexpr (TOP) redc[wn * BM + rl] = c;
                    if constexpr (SMOOTH) reds[wn * BM + rl] = t;
                }
            }
        __syncthreads();
        if (tid < BM && m0 + tid < a.rows) {
            float m = -INFINITY;
            int c = RANK_NONE;
#pragma unroll
            for (int w = 0; w < WGN; ++w) {                                     // ascending column waves
                int cw = 0;
                if constexpr (TOP) cw = redc[w * BM + tid];
                vocab_max_take<TOP>(m, c, red[(w * BM + tid) * 2], cw);
            }
            float s = 0.0f;
#pragma unroll
            for (int w = 0; w < WGN; ++w) {
                const float mw = red[(w * BM + tid) * 2];
                if (mw > -INFINITY) s += red[(w * BM + tid) * 2 + 1] * __expf(mw - m);
            }
            const long at = (long)(m0 + tid) * a.slots + bx;
            a.partial[at * 2] = m;
            a.partial[at * 2 + 1] = s;
            if constexpr (TOP) a.partial_top[at] = c;
            if constexpr (SMOOTH) {
                float t = 0.0f;
#pragma unroll
                for (int w = 0; w < WGN; ++w) t += reds[w * BM + tid];          // ascending column waves
                a.partial_sum[at] = t;
            }
        }
    } else {
        const float nvalid = a.scal[0];
        const float up = a.gout ? a.gout[0] : 1.0f;
        T* dl = reinterpret_cast<T*>(a.dl);
#pragma unroll
        for (int ma = 0; ma < MI; ++ma)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm0 + 16 * ma + 4 * g + r;
                if (row >= a.rows) continue;
                const long lab = (long)a.labels[row];
                bool counts = lab != (long)a.ignore && nvalid > 0.0f;
                float sc = counts ? up / nvalid : 0.0f;
                if constexpr (WEIGHTED) {
                    float w;
                    if constexpr (SMOOTH) w = a.seq_weight ? a.seq_weight[row / a.seq_len] : 1.0f;
                    else w = a.seq_weight[row / a.seq_len];
                    counts = counts && w != 0.0f;              // a zero weight: the row is stored as an ignored one, exact zeros
                    sc = counts ? w * sc : 0.0f;               // w * (gout / n_valid): at w = 1.0f the unweighted bits
                }
                const float l = counts ? a.lse[row] : 0.0f;
                // SMOOTH: the target is (1 - eps) on the label and eps / V on every column; an ignored row is (0 - 0 - 0) * 0
                [[maybe_unused]] float hot = 0.0f, uni = 0.0f;
                if constexpr (SMOOTH) {
                    if (counts) { hot = 1.0f - a.smoothing; uni = a.smoothing / (float)a.V; }
                }
#pragma unroll
                for (int b = 0; b < NI; ++b) {
                    if (!vcol[b]) continue;
                    const float p = counts ? __expf(acc[ma][b][r] + bv[b] - l) : 0.0f;
                    if constexpr (SMOOTH) dl[(long)row * a.lddl + col[b]] = from_f32<T>((p - ((long)col[b] == lab ? hot : 0.0f) - uni) * sc);
                    else dl[(long)row * a.lddl + col[b]] = from_f32<T>((p - ((long)col[b] == lab ? 1.0f : 0.0f)) * sc);
                }
            }
    }
}

// The row fold of both forms, by one wave: the row's `slots` pairs (with TOP: triples) in slot order -> in every lane the maximum m, the sum
// s of exp(logit - m) over the row, and with TOP the maximum's column c.  p / pc: the row's slots (pc is not read without TOP).
template <bool TOP>
__device__ __forceinline__ void vocab_row_fold(const float* p, const int* pc, int slots, int lane, float& m, float& s, int& c) {
    m = -INFINITY;
    c = RANK_NONE;
    for (int j = lane; j < slots; j += 64) {                   // ascending slots = ascending columns
        int cj = 0;
        if constexpr (TOP) cj = pc[j];
        vocab_max_take<TOP>(m, c, p[2 * j], cj);
    }
    vocab_max_lanes<TOP, 64>(m, c);
    s = 0.0f;
    for (int j = lane; j < slots; j += 64) {
        const float mj = p[2 * j];
        if (mj > -INFINITY) s += p[2 * j + 1] * expf(mj - m);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
}

// a wave per row: lse[row]; rowloss[row] = lse - label logit (0 on ignored rows); WEIGHTED: times seq_weight[row / seq_len]
template <bool WEIGHTED>
__device__ __forceinline__ void vocab_ce_rows_body(const float* partial, int pitch, int slots, const float* label_logit, const int64_t* labels, int ignore,
                                                   int rows, float* lse, float* rowloss, const float* seq_weight, int seq_len) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float m, s;
    int c;
    vocab_row_fold<false>(partial + (long)row * pitch * 2, nullptr, slots, lane, m, s, c);     // `slots` written column tiles of `pitch` reserved ones
    if (lane == 0) {
        const float l = m + logf(s);
        lse[row] = l;
        float nll = ((long)labels[row] != (long)ignore) ? l - label_logit[row] : 0.0f;
        if constexpr (WEIGHTED) {
            if ((long)labels[row] != (long)ignore) nll = seq_weight[row / seq_len] * nll;
        }
        rowloss[row] = nll;
    }
}

__global__ __launch_bounds__(256) void vocab_ce_rows_kernel(const float* partial, int pitch, int slots, const float* label_logit, const int64_t* labels,
                                                            int ignore, int rows, float* lse, float* rowloss) {
    vocab_ce_rows_body<false>(partial, pitch, slots, label_logit, labels, ignore, rows, lse, rowloss, nullptr, 1);
}

__global__ __launch_bounds__(256) void vocab_ce_rows_weighted_kernel(const float* partial, int pitch, int slots, const float* label_logit,
                                                                     const int64_t* labels, int ignore, int rows, float* lse, float* rowloss,
                                                                     const float* seq_weight, int seq_len) {
    vocab_ce_rows_body<true>(partial, pitch, slots, label_logit, labels, ignore, rows, lse, rowloss, seq_weight, seq_len);
}

// The smoothed row fold, a wave per row: lse as vocab_ce_rows_body (the same fold on the same pairs: the same bits), then the row's sum of
// logits S from its `slots` partial sums -- lane-strided over ascending slots, then the xor steps -- and
//   rowloss = w * fma(1 - eps, lse - label logit, eps * (lse - S / V))     (0 on ignored rows; w = 1 without seq_weight)
__global__ __launch_bounds__(256) void vocab_ce_rows_smooth_kernel(const float* partial, const float* partial_sum, int pitch, int slots,
                                                                   const float* label_logit, const int64_t* labels, int ignore, int rows, int V,
                                                                   float eps, float* lse, float* rowloss, const float* seq_weight, int seq_len) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float m, s;
    int c;
    vocab_row_fold<false>(partial + (long)row * pitch * 2, nullptr, slots, lane, m, s, c);
    const float* ps = partial_sum + (long)row * pitch;
    float t = 0.0f;
    for (int j = lane; j < slots; j += 64) t += ps[j];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) t += __shfl_xor(t, o, 64);
    if (lane == 0) {
        const float l = m + logf(s);
        lse[row] = l;
        float out = 0.0f;
        if ((long)labels[row] != (long)ignore) {
            const float w = seq_weight ? seq_weight[row / seq_len] : 1.0f;
            out = w * __fmaf_rn(1.0f - eps, l - label_logit[row], eps * (l - t / (float)V));
        }
        rowloss[row] = out;
    }
}

__device__ __forceinline__ float vocab_block_sum(float v, float* red) {      // 256 threads, fixed order
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// one workgroup: n_valid and the loss, both summed in row order (CrossEntropyLoss: mean over the rows that count, NaN if none does)
__global__ __launch_bounds__(256) void vocab_ce_loss_kernel(const float* rowloss, const int64_t* labels, int ignore, int rows, float* scal, float* loss) {
    __shared__ float red[4];
    float c = 0.0f, t = 0.0f;
    for (int r = threadIdx.x; r < rows; r += 256) {
        c += ((long)labels[r] != (long)ignore) ? 1.0f : 0.0f;
        t += rowloss[r];
    }
    c = vocab_block_sum(c, red);
    t = vocab_block_sum(t, red);
    if (threadIdx.x == 0) {
        scal[0] = c;
        scal[1] = t;
        loss[0] = c > 0.0f ? t / c : NAN;
    }
}

template <typename T, bool BWD, bool TOP, int WGN, bool WEIGHTED, bool SMOOTH>
static int vocab_ce_launch_as(const VocabCeArgs& a, hipStream_t stream) {
    constexpr int NC = 2, BK = NC * Mma<T>::CH, NT = 128 * WGN;
    constexpr size_t smem_k = 2 * (Tile<T, false, 128, BK, NT>::BYTES + Tile<T, false, 128, BK, NT>::BYTES);
    constexpr size_t smem_r = (size_t)WGN * 128 * ((TOP || SMOOTH) ? 3 : 2) * sizeof(float);
    constexpr size_t smem = smem_k > smem_r ? smem_k : smem_r;
    static bool done[UNIVL_MAX_DEVICES] = {};
    if (smem > 48 * 1024) univl_allow_lds(vocab_ce_kernel<T, BWD, TOP, WGN, WEIGHTED, SMOOTH>, smem, done);
    hipLaunchKernelGGL((vocab_ce_kernel<T, BWD, TOP, WGN, WEIGHTED, SMOOTH>), dim3(a.nx * a.ny), dim3(NT), smem, stream, a);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}

// the tile kernel of one form (training forward, backward, weighted backward, scoring forward, smoothed forward, smoothed backward) for
// the descriptor's dtype
template <bool BWD, bool TOP, bool WEIGHTED = false, bool SMOOTH = false>
static int vocab_ce_launch(int dtype, const VocabCeArgs& a, hipStream_t stream) {
    return dtype == UNIVL_BF16 ? vocab_ce_launch_as<__bf16, BWD, TOP, 4, WEIGHTED, SMOOTH>(a, stream)
                               : vocab_ce_launch_as<float, BWD, TOP, 2, WEIGHTED, SMOOTH>(a, stream);
}
