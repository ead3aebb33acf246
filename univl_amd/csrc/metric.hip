// N-gram overlap statistics of token rows on the device (include/univl_hip.h: univl_caption_overlap, univl_consensus_pick): what
// BLEU, ROUGE_L and CIDEr are made of, for hypotheses against references or for sampled captions against each other.
//
//   overlap  one wave (64 threads) per item.  Lane j owns hypothesis positions j and j + 64.  A row is staged in LDS as symbols + 1
//            (0 past its length), and every position's packed key of the four symbols that start there as one 64-bit word; the key
//            of an n-gram is that word under a mask of 16 n bits.  A symbol + 1 is never 0, so a masked word that runs past the row's
//            end holds a zero field and equals no n-gram: validity of the OTHER position needs no test.  Counts are taken by every
//            lane reading the same LDS word (a broadcast read) per position of the other row and comparing it, for n = 1 .. 4 at
//            once, with its own two keys; "matches before my position == 0" is the first-occurrence flag that marks the distinct
//            n-grams.  The longest common subsequence is the bit-vector recurrence V <- (V + (V & M)) | (V & ~M) over the hypothesis
//            positions, M being a ballot of `hyp[lane] == token` per reference token, two 64-bit words with carry; the zero bits of
//            V are the length.
//   pick     one thread per instance: arg-max of a short fp64 row, equal scores to the lower index.
//
// Integers are exact.  The fp64 values are formed from the integers at the end of every reference and of the item: products and
// logarithms per lane, summed down a fixed butterfly of the lanes, then a fixed left-to-right chain over n and over the references.
// No float atomics (the one atomic is an integer OR into the status word), no dependence on the number of items.
#include <math.h>
#include "common.h"
#include "ngram_rows.h"     // mask_n, stage_row: rows as packed n-gram words in LDS (shared with ngram_df.hip)
#include "univl_hip.h"

namespace {

constexpr int MT = NGRAM_MT;                 // 128: two positions per lane

struct OverlapArgs {
    const int32_t* sym; long ld;
    const int32_t* len;
    int rows, T, n_refs;
    const int32_t* hyp_row; const int32_t* ref_begin; const int32_t* ref_rows;
    const uint64_t* df_keys; const int32_t* df_cnt;
    int df_begin[5];
    int n_docs;
    int32_t* guess; int32_t* correct; int32_t* hyp_len; int32_t* ref_len; int32_t* lcs;
    double* rouge_l; double* cider; double* bleu;
    int32_t* status;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);     // a + b == b + a: every lane ends with the same bits
    return v;
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// document frequency of an n-gram: binary search in the n-th segment of the sorted key table; 0 when absent
__device__ __forceinline__ int df_of(const OverlapArgs& a, int n, uint64_t key) {
    int lo = a.df_begin[n - 1], hi = a.df_begin[n];
    const int end = hi;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a.df_keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < end && a.df_keys[lo] == key) ? a.df_cnt[lo] : 0;
}

__global__ __launch_bounds__(64) void caption_overlap_kernel(OverlapArgs a) {
    __shared__ uint32_t hs[MT + 4], rs[MT + 4];
    __shared__ uint64_t hk[MT], rk[MT];
    const int item = blockIdx.x, lane = threadIdx.x;
    const bool tfidf = a.cider != nullptr;
    int flags = 0;
    int rb = a.ref_begin[item], re = a.ref_begin[item + 1];
    if (rb < 0 || re > a.n_refs || re <= rb) {                         // an item without references, or offsets outside the list
        flags |= UNIVL_OVERLAP_BAD_REFS;
        rb = rb < 0 ? 0 : (rb > a.n_refs ? a.n_refs : rb);
        re = re > a.n_refs ? a.n_refs : re;
        if (re < rb) re = rb;
    }
    const int L = stage_row(a, a.hyp_row[item], hs, hk, lane, flags);
    // ---- my two positions of the hypothesis: symbols (for the match ballots), keys, counts within the hypothesis, first flags
    uint32_t hsym[2];
    uint64_t hkey[4][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int p = lane + 64 * h;
        hsym[h] = hs[p];
        const uint64_t w = hk[p];
#pragma unroll
        for (int n = 1; n <= 4; ++n) hkey[n - 1][h] = p + n <= L ? (w & mask_n(n)) : 0ULL;     // 0 equals no n-gram
    }
    int hcnt[4][2] = {}, hbefore[4][2] = {};
    for (int q = 0; q < L; ++q) {
        const uint64_t w = hk[q];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const uint64_t g = w & mask_n(n + 1);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int eq = g == hkey[n][h] ? 1 : 0;
                hcnt[n][h] += eq;
                hbefore[n][h] += (q < lane + 64 * h) ? eq : 0;
            }
        }
    }
    bool hfirst[4][2];
    double hw[4][2] = {}, hnorm[4] = {}, hidf[4][2] = {};
    const double log_docs = tfidf ? log((double)a.n_docs) : 0.0;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        double sq = 0.0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            hfirst[n][h] = hkey[n][h] != 0ULL && hbefore[n][h] == 0;
            if (tfidf && hfirst[n][h]) {
                const int df = df_of(a, n + 1, hkey[n][h]);
                hidf[n][h] = log_docs - log((double)(df < 1 ? 1 : df));
                hw[n][h] = (double)hcnt[n][h] * hidf[n][h];
                sq += hw[n][h] * hw[n][h];
            }
        }
        if (tfidf) hnorm[n] = sqrt(wave_sum_f64(sq));
    }
    // ---- the references, in list order
    int rmax[4][2] = {};
    int best_len = 0, best_diff = 0, lcs_max = 0;
    double recall = 0.0, cider_sum = 0.0;
    for (int r = rb; r < re; ++r) {
        __syncthreads();                                               // the previous reference's words are no longer read
        const int Lr = stage_row(a, a.ref_rows[r], rs, rk, lane, flags);
        const int diff = Lr > L ? Lr - L : L - Lr;
        if (r == rb || diff < best_diff || (diff == best_diff && Lr < best_len)) { best_diff = diff; best_len = Lr; }
        uint64_t rkey[4][2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int p = lane + 64 * h;
            const uint64_t w = rk[p];
#pragma unroll
            for (int n = 1; n <= 4; ++n) rkey[n - 1][h] = p + n <= Lr ? (w & mask_n(n)) : 0ULL;
        }
        int rcnt[4][2] = {}, scnt[4][2] = {}, sbefore[4][2] = {};
        uint64_t v0 = ~0ULL, v1 = ~0ULL;
        for (int q = 0; q < Lr; ++q) {
            const uint64_t w = rk[q];
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const uint64_t g = w & mask_n(n + 1);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    rcnt[n][h] += g == hkey[n][h] ? 1 : 0;
                    if (tfidf) {
                        const int eq = g == rkey[n][h] ? 1 : 0;
                        scnt[n][h] += eq;
                        sbefore[n][h] += (q < lane + 64 * h) ? eq : 0;
                    }
                }
            }
            const uint32_t c = (uint32_t)(w & 0xFFFFULL);                // the token at q (+ 1); positions past L hold 0 and never match
            const uint64_t m0 = __ballot(hsym[0] == c), m1 = __ballot(hsym[1] == c);
            const uint64_t u0 = v0 & m0, u1 = v1 & m1;
            const uint64_t s0 = v0 + u0;
            const uint64_t s1 = v1 + u1 + (s0 < v0 ? 1ULL : 0ULL);
            v0 = s0 | (v0 & ~m0);
            v1 = s1 | (v1 & ~m1);
        }
        const int l = __popcll(~v0) + __popcll(~v1);
        if (lane == 0) a.lcs[r] = l;
        lcs_max = l > lcs_max ? l : lcs_max;
        const double rec = (double)l / (double)(Lr < 1 ? 1 : Lr);
        recall = rec > recall ? rec : recall;
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int h = 0; h < 2; ++h) rmax[n][h] = rcnt[n][h] > rmax[n][h] ? rcnt[n][h] : rmax[n][h];
        if (tfidf) {
            const double d = (double)((L > 1 ? L - 1 : 0) - (Lr > 1 ? Lr - 1 : 0));
            const double penalty = exp(-(d * d) / (2.0 * 6.0 * 6.0));
            double vals = 0.0;
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                double dot = 0.0, sq = 0.0;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (hfirst[n][h]) {
                        const double wr = (double)rcnt[n][h] * hidf[n][h];
                        dot += fmin(hw[n][h], wr) * wr;
                    }
                    if (rkey[n][h] != 0ULL && sbefore[n][h] == 0) {
                        const int df = df_of(a, n + 1, rkey[n][h]);
                        const double w = (double)scnt[n][h] * (log_docs - log((double)(df < 1 ? 1 : df)));
                        sq += w * w;
                    }
                }
                dot = wave_sum_f64(dot);
                const double rnorm = sqrt(wave_sum_f64(sq));
                if (hnorm[n] != 0.0 && rnorm != 0.0) dot /= hnorm[n] * rnorm;
                vals += dot * penalty;
            }
            cider_sum += vals / 4.0;
        }
    }
    // ---- the item's results
    int corr[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        int c = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (hfirst[n][h]) c += hcnt[n][h] < rmax[n][h] ? hcnt[n][h] : rmax[n][h];
        corr[n] = wave_sum_i32(c);
    }
    if (flags) atomicOr(a.status, flags);
    if (lane != 0) return;
    const int R = re - rb;
    double bl = 1.0;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int gs = L - n > 0 ? L - n : 0;
        a.guess[item * 4 + n] = gs;
        a.correct[item * 4 + n] = corr[n];
        bl *= ((double)corr[n] + 1e-15) / ((double)gs + 1e-9);
    }
    a.hyp_len[item] = L;
    a.ref_len[item] = best_len;
    const double p = (double)lcs_max / (double)(L < 1 ? 1 : L), q = recall, b2 = 1.2 * 1.2;
    a.rouge_l[item] = (p != 0.0 && q != 0.0) ? ((1.0 + b2) * p * q) / (q + b2 * p) : 0.0;
    if (tfidf) a.cider[item] = R > 0 ? 10.0 * (cider_sum / (double)R) : 0.0;
    if (a.bleu != nullptr) {
        double b = sqrt(sqrt(bl));
        const double ratio = ((double)L + 1e-15) / ((double)best_len + 1e-9);
        if (ratio < 1.0) b *= exp(1.0 - 1.0 / ratio);
        a.bleu[item] = b;
    }
}

__global__ __launch_bounds__(64) void consensus_pick_kernel(const double* score, int n_inst, int n_samp, int32_t* pick, double* best) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_inst) return;
    const double* s = score + (long)i * n_samp;
    int at = 0;
    double v = s[0];
    for (int k = 1; k < n_samp; ++k)
        if (s[k] > v || (v != v && s[k] == s[k])) { v = s[k]; at = k; }   // strictly greater: equal scores stay with the lower index; a number beats a NaN
    pick[i] = at;
    if (best != nullptr) best[i] = v;
}

__device__ __forceinline__ bool finite_f64(double v) { return v - v == 0.0; }      // false for NaN and both infinities

// one thread per video: rewards -> fp32 weights (include/univl_hip.h: univl_caption_advantage)
__global__ __launch_bounds__(64) void caption_advantage_kernel(const double* reward, const double* baseline, int n, int ns, int kind, double scale,
                                                               float* weight, int32_t* status) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const double* r = reward + (long)i * ns;
    float* w = weight + (long)i * ns;
    bool bad = false, have = true;
    double sum = 0.0, b = 0.0;
    int m = 0;
    if (kind == UNIVL_ADV_LOO) {
        for (int s = 0; s < ns; ++s)                                // left to right over the finite rewards
            if (finite_f64(r[s])) { sum += r[s]; ++m; }
        have = m >= 2;
        bad = m < ns;
    } else {
        b = baseline[i];
        have = finite_f64(b);
        bad = !have;
    }
    for (int s = 0; s < ns; ++s) {
        const double x = r[s];
        float out = 0.0f;
        if (!finite_f64(x)) bad = true;
        else if (have) {
            const double adv = kind == UNIVL_ADV_LOO ? x - (sum - x) / (double)(m - 1) : x - b;
            out = (float)(adv * scale);
            if (!(out - out == 0.0f)) { out = 0.0f; bad = true; }
        }
        w[s] = out;
    }
    if (bad) atomicOr(status, UNIVL_ADV_NONFINITE);
}

}  // namespace

extern "C" int univl_caption_advantage(const double* reward, const double* baseline, int32_t n, int32_t ns, int32_t baseline_kind, double scale,
                                       float* weight, int32_t* status, hipStream_t stream) {
    UNIVL_ON_STREAM_DEVICE(stream);
    UNIVL_CHECK_ARG(baseline_kind == UNIVL_ADV_LOO || baseline_kind == UNIVL_ADV_GIVEN, UNIVL_EINVAL, "univl_caption_advantage: baseline_kind %d",
                    baseline_kind);
    UNIVL_CHECK_ARG(reward && weight && status && (baseline_kind == UNIVL_ADV_LOO || baseline), UNIVL_EINVAL,
                    "univl_caption_advantage: null pointer");
    UNIVL_CHECK_ARG(n >= 1 && ns >= (baseline_kind == UNIVL_ADV_LOO ? 2 : 1), UNIVL_EINVAL,
                    "univl_caption_advantage: n=%d ns=%d (n >= 1; ns >= 1, and >= 2 for the leave-one-out baseline)", n, ns);
    hipLaunchKernelGGL(caption_advantage_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, reward, baseline, n, ns, baseline_kind, scale, weight,
                       status);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}

extern "C" int univl_caption_overlap_sizeof(void) { return (int)sizeof(UnivlCaptionOverlap); }

extern "C" int univl_caption_overlap(const UnivlCaptionOverlap* d, hipStream_t stream) {
    UNIVL_ON_STREAM_DEVICE(stream);
    UNIVL_CHECK_ARG(d != nullptr, UNIVL_EINVAL, "univl_caption_overlap: null descriptor");
    UNIVL_CHECK_ARG(d->T >= 1 && d->T <= UNIVL_OVERLAP_TMAX && d->ld >= d->T && d->rows >= 1 && d->items >= 1 && d->n_refs >= d->items,
                    UNIVL_EINVAL, "univl_caption_overlap: rows=%d T=%d ld=%lld items=%d n_refs=%d (1 <= T <= %d, T <= ld, rows >= 1, "
                    "1 <= items <= n_refs: every item has a reference)", d->rows, d->T, (long long)d->ld, d->items, d->n_refs,
                    UNIVL_OVERLAP_TMAX);
    UNIVL_CHECK_ARG(d->sym && d->len && d->hyp_row && d->ref_begin && d->ref_rows && d->guess && d->correct && d->hyp_len && d->ref_len &&
                    d->lcs && d->rouge_l && d->status, UNIVL_EINVAL, "univl_caption_overlap: null pointer");
    if (d->cider != nullptr) {
        bool ok = d->n_docs >= 1 && d->df_begin[0] == 0;
        for (int n = 0; n < 4; ++n) ok = ok && d->df_begin[n + 1] >= d->df_begin[n];
        ok = ok && (d->df_begin[4] == 0 || (d->df_keys != nullptr && d->df_cnt != nullptr));
        UNIVL_CHECK_ARG(ok, UNIVL_EINVAL, "univl_caption_overlap: cider needs n_docs >= 1 and the document-frequency tables "
                        "(df_begin = 0 <= ... non-decreasing, df_keys / df_cnt of df_begin[4] entries); n_docs=%d", d->n_docs);
    }
    OverlapArgs a;
    a.sym = d->sym; a.ld = (long)d->ld; a.len = d->len; a.rows = d->rows; a.T = d->T; a.n_refs = d->n_refs;
    a.hyp_row = d->hyp_row; a.ref_begin = d->ref_begin; a.ref_rows = d->ref_rows;
    a.df_keys = d->df_keys; a.df_cnt = d->df_cnt;
    for (int n = 0; n < 5; ++n) a.df_begin[n] = d->cider != nullptr ? d->df_begin[n] : 0;
    a.n_docs = d->n_docs;
    a.guess = d->guess; a.correct = d->correct; a.hyp_len = d->hyp_len; a.ref_len = d->ref_len; a.lcs = d->lcs;
    a.rouge_l = d->rouge_l; a.cider = d->cider; a.bleu = d->bleu; a.status = d->status;
    hipLaunchKernelGGL(caption_overlap_kernel, dim3(d->items), dim3(64), 0, stream, a);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}

extern "C" int univl_consensus_pick(const double* score, int32_t n_inst, int32_t n_samp, int32_t* pick, double* best, hipStream_t stream) {
    UNIVL_ON_STREAM_DEVICE(stream);
    UNIVL_CHECK_ARG(score && pick, UNIVL_EINVAL, "univl_consensus_pick: null pointer");
    UNIVL_CHECK_ARG(n_inst >= 1 && n_samp >= 1, UNIVL_EINVAL, "univl_consensus_pick: n_inst=%d n_samp=%d (both >= 1)", n_inst, n_samp);
    hipLaunchKernelGGL(consensus_pick_kernel, dim3((n_inst + 63) / 64), dim3(64), 0, stream, score, n_inst, n_samp, pick, best);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}
