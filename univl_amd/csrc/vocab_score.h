// The scoring form of K16: teacher-forced scoring on the tied vocabulary classifier -- the forward of K16 (vocab_ce.h) with the row's arg-max kept beside its
// online log-softmax statistics, and per-caption sums instead of one batch mean.  The [rows, 30522] logits never exist in memory.
// Included by gemm.hip after vocab_ce.h (needs Tile / gemm_acc_only / pair_tile / smem_raw / univl_allow_lds).
//
// Reference: BertLMPredictionHead.forward (module_bert.py:327-330, decoder copy module_decoder.py:180-183), then what a caller of
// decoder_caption(get_logits=True) does with the logits: log_softmax, gather at the labels, arg-max (modeling.py:409-428, :253).
//
// vocab_score_kernel<T, WGN>: vocab_ce_kernel<T, false, WGN>'s walk (128 x 128 tiles, gemm_acc_only); a tile's epilogue reduces its logits
//   to one (max, sum of exp(logit - max), column of the max) triple per row -- 16-lane shuffles inside a wave, LDS across the waves of the
//   column direction -- and writes it to slot [row][column tile]; the one lane that owns (row, label[row]) stores that logit.  Equal
//   logits: the LOWER column wins at every level (a strict > in ascending column order, (value, column) order in the shuffles).
// vocab_score_rows_kernel: a wave per row folds the row's slots in slot order -> lse, token_logprob, top_token, top_logprob.
// vocab_score_segments_kernel: a wave per caption; seq_logprob is the plain left-to-right fp32 sum of the caption's token_logprob.
// Every reduction is in fixed order: bit-reproducible in every mode, no float atomics.
#pragma once

struct VocabScoreArgs {
    const void* X; long ldx;            // [rows, K] head output (compute type), K-major
    const void* E; long lde;            // [V, K] tied word table (compute type), K-major
    const float* bias;                  // [V] or null
    int rows, V, K;
    const int64_t* labels;
    float* partial; int* partial_top; int slots;    // [rows, slots, 2], [rows, slots]
    float* label_logit;                 // [rows]
    int nx, ny;
};

constexpr int VOCAB_NO_COLUMN = 0x7fffffff;     // the column of an empty maximum (-inf over no valid column)

// (value, column) order of the arg-max: the larger value, at equal values the lower column
__device__ __forceinline__ void vocab_top_take(float& m, int& c, float om, int oc) {
    if (om > m || (om == m && oc < c)) { m = om; c = oc; }
}

template <typename T, int WGN>
__global__ __launch_bounds__(128 * WGN, 2) void vocab_score_kernel(VocabScoreArgs a) {
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
    float* red = reinterpret_cast<float*>(smem_raw);              // [WGN][BM][2]
    int* redc = reinterpret_cast<int*>(red + WGN * BM * 2);       // [WGN][BM]
#pragma unroll
    for (int ma = 0; ma < MI; ++ma)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rl = wm0 + 16 * ma + 4 * g + r, row = m0 + rl;
            const long lab = row < a.rows ? (long)a.labels[row] : -2;       // a label outside [0, V) matches no column
            float v[NI], m = -INFINITY;
            int c = VOCAB_NO_COLUMN;
#pragma unroll
            for (int b = 0; b < NI; ++b) {                                  // ascending columns: the strict > keeps the lower one
                v[b] = vcol[b] ? acc[ma][b][r] + bv[b] : -INFINITY;
                if (v[b] > m) { m = v[b]; c = col[b]; }
                if (vcol[b] && (long)col[b] == lab) a.label_logit[row] = v[b];
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                const float om = __shfl_xor(m, o, 64);
                const int oc = __shfl_xor(c, o, 64);
                vocab_top_take(m, c, om, oc);
            }
            float s = 0.0f;
            if (m > -INFINITY) {
#pragma unroll
                for (int b = 0; b < NI; ++b) s += __expf(v[b] - m);         // exp(-inf) = 0 for the columns beyond V
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o, 64);
            if (i == 0) { red[(wn * BM + rl) * 2] = m; red[(wn * BM + rl) * 2 + 1] = s; redc[wn * BM + rl] = c; }
        }
    __syncthreads();
    if (tid < BM && m0 + tid < a.rows) {
        float m = -INFINITY;
        int c = VOCAB_NO_COLUMN;
#pragma unroll
        for (int w = 0; w < WGN; ++w) {                                     // ascending column waves
            const float mw = red[(w * BM + tid) * 2];
            if (mw > m) { m = mw; c = redc[w * BM + tid]; }
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
        a.partial_top[at] = c;
    }
}

// a wave per row: fold the row's `slots` triples in slot order -> lse, the arg-max column and its log-probability, the label's
// log-probability (0 where the row does not count: label == ignore or outside [0, V))
__global__ __launch_bounds__(256) void vocab_score_rows_kernel(const float* partial, const int* partial_top, int pitch, int slots, const float* label_logit,
                                                               const int64_t* labels, int ignore, int V, int rows, float* lse, float* token_logprob,
                                                               int* top_token, float* top_logprob) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* p = partial + (long)row * pitch * 2;          // `slots` written column tiles of `pitch` reserved ones
    const int* pc = partial_top + (long)row * pitch;
    float m = -INFINITY;
    int c = VOCAB_NO_COLUMN;
    for (int j = lane; j < slots; j += 64) {                   // ascending slots = ascending columns
        const float mj = p[2 * j];
        if (mj > m) { m = mj; c = pc[j]; }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float om = __shfl_xor(m, o, 64);
        const int oc = __shfl_xor(c, o, 64);
        vocab_top_take(m, c, om, oc);
    }
    float s = 0.0f;
    for (int j = lane; j < slots; j += 64) {
        const float mj = p[2 * j];
        if (mj > -INFINITY) s += p[2 * j + 1] * expf(mj - m);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) {
        const float ls = logf(s);                              // s >= 1: the max's own term
        const long lab = (long)labels[row];
        const bool counts = lab != (long)ignore && lab >= 0 && lab < (long)V;
        lse[row] = m + ls;
        top_token[row] = c;
        top_logprob[row] = -ls;                                // max - lse without the cancellation
        token_logprob[row] = counts ? (label_logit[row] - m) - ls : 0.0f;
    }
}

// a wave per caption s over rows [s * seq_len, (s + 1) * seq_len): seq_logprob = ((t0 + t1) + t2) + ... in row order (ignored rows hold
// an exact 0), seq_tokens = counting rows, seq_correct = counting rows whose arg-max is the label
__global__ __launch_bounds__(256) void vocab_score_segments_kernel(const float* token_logprob, const int* top_token, const int64_t* labels, int ignore, int V,
                                                                   int n_seq, int seq_len, float* seq_logprob, int* seq_tokens, int* seq_correct) {
    const int seq = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (seq >= n_seq) return;
    const long r0 = (long)seq * seq_len;
    float t = 0.0f;
    int n = 0, ok = 0;
    for (int base = 0; base < seq_len; base += 64) {
        const int j = base + lane, left = seq_len - base < 64 ? seq_len - base : 64;
        float v = 0.0f;
        if (j < seq_len) {
            v = token_logprob[r0 + j];
            const long lab = (long)labels[r0 + j];
            const bool counts = lab != (long)ignore && lab >= 0 && lab < (long)V;
            n += counts ? 1 : 0;
            ok += (counts && (long)top_token[r0 + j] == lab) ? 1 : 0;
        }
        for (int k = 0; k < left; ++k) t += __shfl(v, k, 64);             // every lane keeps the same running sum
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        n += __shfl_xor(n, o, 64);
        ok += __shfl_xor(ok, o, 64);
    }
    if (lane == 0) {
        seq_logprob[seq] = t;
        seq_tokens[seq] = n;
        seq_correct[seq] = ok;
    }
}

template <typename T, int WGN>
static int vocab_score_launch(const VocabScoreArgs& a, hipStream_t stream) {
    constexpr int NC = 2, BK = NC * Mma<T>::CH, NT = 128 * WGN;
    constexpr size_t smem_k = 2 * (Tile<T, false, 128, BK, NT>::BYTES + Tile<T, false, 128, BK, NT>::BYTES);
    constexpr size_t smem_r = (size_t)WGN * 128 * 3 * sizeof(float);
    constexpr size_t smem = smem_k > smem_r ? smem_k : smem_r;
    static bool done[UNIVL_MAX_DEVICES] = {};
    if (smem > 48 * 1024) univl_allow_lds(vocab_score_kernel<T, WGN>, smem, done);
    hipLaunchKernelGGL((vocab_score_kernel<T, WGN>), dim3(a.nx * a.ny), dim3(NT), smem, stream, a);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}
