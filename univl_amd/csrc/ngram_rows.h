// Token rows as packed n-gram words in LDS: what csrc/metric.hip (overlap statistics) and csrc/ngram_df.hip (document-frequency
// tables) both start from.  A row table is sym [rows, ld] int32 with lengths len [rows] (include/univl_hip.h: UnivlCaptionOverlap).
#pragma once
#include "common.h"
#include "univl_hip.h"

constexpr int NGRAM_MT = UNIVL_OVERLAP_TMAX;       // 128: two positions per lane of a wave

// the bits of a packed word that an n-gram (n = 1 .. 4) occupies
__device__ __forceinline__ uint64_t mask_n(int n) { return n == 4 ? ~0ULL : ((1ULL << (16 * n)) - 1ULL); }

// Stages row `row` (clamped into the table) into s[0 .. NGRAM_MT + 3] (symbol + 1, 0 past the length) and k[0 .. NGRAM_MT) (packed
// words);  returns the clamped length.  Only positions below the length are read from memory.  Whole wave; ends with a barrier.
// Args: anything with sym, ld, len, rows, T.
template <typename Args>
__device__ __forceinline__ int stage_row(const Args& a, int row, uint32_t* s, uint64_t* k, int lane, int& flags) {
    if (row < 0 || row >= a.rows) { flags |= UNIVL_OVERLAP_BAD_ROW; row = row < 0 ? 0 : a.rows - 1; }
    int L = a.len[row];
    if (L < 0 || L > a.T) { flags |= UNIVL_OVERLAP_BAD_LEN; L = L < 0 ? 0 : a.T; }
    const int32_t* x = a.sym + (long)row * a.ld;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int p = lane + 64 * h;
        uint32_t v = 0;
        if (p < L) {
            int c = x[p];
            if (c < 0 || c > UNIVL_OVERLAP_SYM_MAX) { flags |= UNIVL_OVERLAP_BAD_SYM; c = c < 0 ? 0 : UNIVL_OVERLAP_SYM_MAX; }
            v = (uint32_t)c + 1u;
        }
        s[p] = v;
    }
    if (lane < 4) s[NGRAM_MT + lane] = 0;
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int p = lane + 64 * h;
        k[p] = (uint64_t)s[p] | ((uint64_t)s[p + 1] << 16) | ((uint64_t)s[p + 2] << 32) | ((uint64_t)s[p + 3] << 48);
    }
    __syncthreads();
    return L;
}
