// The scoring form of K16: teacher-forced scoring on the tied vocabulary classifier -- the forward of K16 (vocab_ce.h) with the row's arg-max kept beside its
// online log-softmax statistics, and per-caption sums instead of one batch mean.  The [rows, 30522] logits never exist in memory.
// Included by gemm.hip after vocab_ce.h, whose tile kernel (vocab_ce_kernel<T, false, true, WGN>) and row fold (vocab_row_fold<true>) it uses.
//
// Reference: BertLMPredictionHead.forward (module_bert.py:327-330, decoder copy module_decoder.py:180-183), then what a caller of
// decoder_caption(get_logits=True) does with the logits: log_softmax, gather at the labels, arg-max (modeling.py:409-428, :253).
//
// The tile kernel leaves one (max, sum of exp(logit - max), column of the max) triple per row and column tile.  Equal logits: the LOWER
//   column wins at every level (a strict > in ascending column order, `better` of ranked.h in the shuffles); the column of an empty
//   maximum (-inf over no valid column) is RANK_NONE.
// vocab_score_rows_kernel: a wave per row folds the row's slots in slot order -> lse, token_logprob, top_token, top_logprob.
// vocab_score_segments_kernel: a wave per caption; seq_logprob is the plain left-to-right fp32 sum of the caption's token_logprob.
// Every reduction is in fixed order: bit-reproducible in every mode, no float atomics.
#pragma once

// a wave per row: lse, the arg-max column and its log-probability, the label's log-probability (0 where the row does not count:
// label == ignore or outside [0, V))
__global__ __launch_bounds__(256) void vocab_score_rows_kernel(const float* partial, const int* partial_top, int pitch, int slots, const float* label_logit,
                                                               const int64_t* labels, int ignore, int V, int rows, float* lse, float* token_logprob,
                                                               int* top_token, float* top_logprob) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float m, s;
    int c;
    vocab_row_fold<true>(partial + (long)row * pitch * 2, partial_top + (long)row * pitch, slots, lane, m, s, c);
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
