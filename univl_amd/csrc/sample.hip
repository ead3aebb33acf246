// One position of ancestral caption sampling on the device (include/univl_hip.h: univl_sample_step): top-k / temperature / top-p
// over the RAW logits of every row, the draw, and the row's bookkeeping, as two launches with no host involvement.
//
//   scan    grid (rows, slices), 256 threads = 4 waves.  A workgroup reads one column slice of one row once, with 16-byte loads, four
//           per lane in flight.  Each wave keeps a running top-64 list with ONE ENTRY PER LANE, sorted best first (the list of
//           csrc/ranked.h: every value is tested against the list's k-th entry first, the few that pass are inserted by ballot and
//           popcount), and each lane an online (max, sum of exponentials) pair over the columns it read, in the order it read them.
//           The lanes' pairs fold down a fixed tree to lane 0, the waves' lists and pairs merge through LDS in ascending wave order,
//           and the slice's k best and its pair go to the workspace.  The log-softmax of the row is never formed.
//   select  one wave per row: the slices' lists and pairs merge in ascending slice order; then weights, the cumulative chain, the
//           nucleus, the draw and the outputs (contract steps 2 to 6).
//
// Order of candidates everywhere: larger value first, equal values by LOWER column first (`better`, ranked.h).  Nothing here depends on the
// number of rows, on what other rows hold or on deterministic mode: a workgroup sees one row, every reduction has a fixed order, and
// there are no atomics.  The slice count is a function of V alone.  The sum of exponentials is carried in fp64 (fp32 terms), and the
// two logarithms of the outputs are taken in fp64 and rounded once, so tok_logprob / q_logprob are within an fp32 rounding of the
// values the contract's formulas give in exact arithmetic on the fp32 weights.
#include <math.h>
#include "common.h"
#include "ranked.h"
#include "univl_hip.h"

namespace {

constexpr int SP_WAVES = 4;
constexpr int SP_SLICE_COLS = 2048;          // a row gets one slice per this many columns, at most UNIVL_SAMPLE_SLICES

// (m, s): max and sum over the columns seen so far of exp(x - m).  Equal arguments take the factor 1 without an exponential, so
// that a pair of (-inf, 0) -- no column yet -- folds away instead of producing inf - inf.
__device__ __forceinline__ void pair_add(float& m, double& s, float x) {
    if (x > m) { s = s * (double)expf(m - x) + 1.0; m = x; }
    else s += x == m ? 1.0 : (double)expf(x - m);
}

__device__ __forceinline__ void pair_merge(float& m, double& s, float m2, double s2) {
    const float M = fmaxf(m, m2);
    const double a = m == M ? 1.0 : (double)expf(m - M), b = m2 == M ? 1.0 : (double)expf(m2 - M);
    s = s * a + s2 * b;
    m = M;
}

struct ScanArgs {
    const float* x; long ld;
    int V, k, chunk, vec, S;
    const uint8_t* done;
    double* ws_sum; float* ws_max; float* ws_val; int* ws_idx;      // [R][S], [R][S], [R][S][k], [R][S][k]
};

__global__ __launch_bounds__(256) void sample_scan_kernel(ScanArgs a) {
    __shared__ float sh_v[SP_WAVES][64];
    __shared__ int sh_i[SP_WAVES][64];
    __shared__ float sh_m[SP_WAVES];
    __shared__ double sh_s[SP_WAVES];
    const int row = blockIdx.x, slice = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (a.done[row]) return;                                          // frozen row: the select kernel does not read its slots
    const float* x = a.x + (long)row * a.ld;
    const int c0 = slice * a.chunk, c1 = min(a.V, c0 + a.chunk);      // chunk is a multiple of 4; columns >= V are never read as candidates
    float lv = -INFINITY, pm = -INFINITY;
    int li = RANK_NONE;
    double ps = 0.0;
    if (a.vec) {
        // a wave takes 256 consecutive columns per step; the loop bounds are wave-uniform (list_offer needs whole waves)
        for (int cb = c0 + 256 * wave; cb < c1; cb += 4 * 1024) {
            f32x4_t q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int cu = cb + u * 1024 + 4 * lane;
                q[u] = cu < c1 ? *reinterpret_cast<const f32x4_t*>(x + cu) : f32x4_t{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (cb + u * 1024 >= c1) break;                       // wave-uniform
                const int cu = cb + u * 1024 + 4 * lane;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool ok = cu + e < c1;
                    if (ok) pair_add(pm, ps, q[u][e]);
                    list_offer(lv, li, a.k, q[u][e], cu + e, ok, lane);
                }
            }
        }
    } else {
        for (int cb = c0 + 64 * wave; cb < c1; cb += 256) {
            const bool ok = cb + lane < c1;
            const float v = ok ? x[cb + lane] : 0.f;
            if (ok) pair_add(pm, ps, v);
            list_offer(lv, li, a.k, v, cb + lane, ok, lane);
        }
    }
    // the lanes' pairs: a fixed tree whose root is lane 0 (the other lanes' results are not used)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_down(pm, o, 64);
        const double s2 = __shfl_down(ps, o, 64);
        pair_merge(pm, ps, m2, s2);
    }
    sh_v[wave][lane] = lv;
    sh_i[wave][lane] = li;
    if (lane == 0) { sh_m[wave] = pm; sh_s[wave] = ps; }
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < SP_WAVES; ++w) {
        const int j = sh_i[w][lane];
        list_offer(lv, li, a.k, sh_v[w][lane], j, lane < a.k && j != RANK_NONE, lane);
        pair_merge(pm, ps, sh_m[w], sh_s[w]);                         // every lane folds the same words; lane 0's is the one kept
    }
    const long slot = (long)row * a.S + slice;
    if (lane < a.k) { a.ws_val[slot * a.k + lane] = lv; a.ws_idx[slot * a.k + lane] = li; }
    if (lane == 0) { a.ws_max[slot] = pm; a.ws_sum[slot] = ps; }
}

struct SelectArgs {
    const double* ws_sum; const float* ws_max; const float* ws_val; const int* ws_idx;
    int k, S, t, Tmax, eos;
    float inv_T, top_p;
    uint64_t seed;
    const float* sampling_dev; const uint64_t* seed_dev; const int32_t* eos_dev;
    uint8_t* done; int32_t* length; int64_t* ids;
    int32_t* tokens_out; float* tok_logprob; float* q_logprob; float* seq_logprob; float* seq_q_logprob;
    int32_t* topk_idx; float* topk_val;
};

__global__ __launch_bounds__(64) void sample_select_kernel(SelectArgs a) {
    const int row = blockIdx.x, lane = threadIdx.x, k = a.k;
    if (a.done[row]) return;                                          // frozen: nothing of the row is written
    // step 1: the k best of the row, lane j holding (x_j, col_j), and the row's (max, sum exp)
    float lv = -INFINITY, pm = -INFINITY;
    int li = RANK_NONE;
    double ps = 0.0;
    for (int s = 0; s < a.S; ++s) {
        const long slot = (long)row * a.S + s;
        const float v = lane < k ? a.ws_val[slot * k + lane] : -INFINITY;
        const int j = lane < k ? a.ws_idx[slot * k + lane] : RANK_NONE;
        list_offer(lv, li, k, v, j, j != RANK_NONE, lane);
        pair_merge(pm, ps, a.ws_max[slot], a.ws_sum[slot]);
    }
    const float inv_T = a.sampling_dev ? a.sampling_dev[0] : a.inv_T, top_p = a.sampling_dev ? a.sampling_dev[1] : a.top_p;
    // step 2: two separately rounded fp32 operations, then expf
    const float x0 = __shfl(lv, 0, 64);
    const float w = lane < k ? expf(__fmul_rn(__fsub_rn(lv, x0), inv_T)) : 0.f;
    // step 3: one left-to-right fp32 chain; lane j keeps c_j, the lanes past k keep c_{k-1}
    float run = 0.f, c = 0.f;
    for (int j = 0; j < k; ++j) {
        const float wj = __shfl(w, j, 64);
        run = j == 0 ? wj : __fadd_rn(run, wj);
        if (lane == j) c = run;
    }
    if (lane >= k) c = run;
    // step 4: the c_j are non-decreasing, so the entries below the threshold are a prefix
    int m = k;
    if (!(top_p >= 1.f)) {
        const float thr = __fmul_rn(top_p, run);
        m = __popcll(__ballot(lane < k && c < thr)) + 1;
        m = m > k ? k : m;
    }
    const float cm = __shfl(c, m - 1, 64);
    // step 5
    const uint64_t seed = a.seed_dev ? *a.seed_dev : a.seed;
    const uint32_t r32 = mix32((seed * 0x9E3779B97F4A7C15ULL) ^ ((uint64_t)a.t * 0xD1B54A32D192ED03ULL + (uint64_t)row));
    const float u = (float)(r32 >> 8) * (1.0f / 16777216.0f);
    const float tau = __fmul_rn(u, cm);
    int js = __popcll(__ballot(lane < m && !(c > tau)));
    js = js > m - 1 ? m - 1 : js;                                     // tau < c_{m-1} for finite weights; NaN rows must stay in range
    const float xs = __shfl(lv, js, 64), wsel = __shfl(w, js, 64);
    const int cs = __shfl(li, js, 64);
    // step 6
    if (a.topk_idx != nullptr && lane < k) a.topk_idx[(long)row * k + lane] = li == RANK_NONE ? -1 : li;
    if (a.topk_val != nullptr && lane < k) a.topk_val[(long)row * k + lane] = lv;
    if (lane == 0) {
        const int token = cs == RANK_NONE ? 0 : cs;                     // fewer than k comparable candidates (NaN rows: unspecified result)
        const float tok_lp = (float)((double)__fsub_rn(xs, pm) - log(ps));
        const float q_lp = (float)log((double)wsel / (double)cm);
        const long at = (long)row * a.Tmax + a.t;
        a.tokens_out[at] = token;
        a.tok_logprob[at] = tok_lp;
        a.q_logprob[at] = q_lp;
        a.ids[row] = token;
        a.seq_logprob[row] = __fadd_rn(a.seq_logprob[row], tok_lp);
        a.seq_q_logprob[row] = __fadd_rn(a.seq_q_logprob[row], q_lp);
        a.length[row] += 1;
        if (token == (a.eos_dev ? *a.eos_dev : a.eos)) a.done[row] = 1;
    }
}

int slices_for(int V) {
    const int s = (V + SP_SLICE_COLS - 1) / SP_SLICE_COLS;
    return s < 1 ? 1 : (s > UNIVL_SAMPLE_SLICES ? UNIVL_SAMPLE_SLICES : s);
}

}  // namespace

extern "C" int univl_sample_step(const UnivlSampleStep* d, hipStream_t stream) {
    UNIVL_ON_STREAM_DEVICE(stream);
    UNIVL_CHECK_ARG(d != nullptr, UNIVL_EINVAL, "univl_sample_step: null descriptor");
    UNIVL_CHECK_ARG(d->R >= 1 && d->k >= 1 && d->k <= UNIVL_SAMPLE_KMAX && d->V >= 1 && d->k <= d->V && d->ld >= d->V &&
                    d->V <= INT_MAX - 16 * 1024, UNIVL_EINVAL, "univl_sample_step: R=%d k=%d V=%d ld=%lld (R >= 1, 1 <= k <= %d, k <= V <= ld)",
                    d->R, d->k, d->V, (long long)d->ld, UNIVL_SAMPLE_KMAX);
    UNIVL_CHECK_ARG(d->t >= 0 && d->t < d->Tmax, UNIVL_EINVAL, "univl_sample_step: position t=%d of Tmax=%d", d->t, d->Tmax);
    UNIVL_CHECK_ARG(d->sampling_dev != nullptr || (isfinite(d->inv_T) && d->inv_T > 0.f && d->top_p > 0.f), UNIVL_EINVAL,
                    "univl_sample_step: inv_T=%g top_p=%g (inv_T finite and > 0, top_p > 0)", (double)d->inv_T, (double)d->top_p);
    UNIVL_CHECK_ARG(d->x && d->done && d->length && d->ids && d->tokens_out && d->tok_logprob && d->q_logprob && d->seq_logprob &&
                    d->seq_q_logprob && d->ws, UNIVL_EINVAL, "univl_sample_step: null pointer");
    const int64_t need = (int64_t)d->R * UNIVL_SAMPLE_SLICES * (8 * (int64_t)d->k + 16);
    UNIVL_CHECK_ARG(d->ws_bytes >= need && aligned16(d->ws), UNIVL_EINVAL,
                    "univl_sample_step: workspace of %lld bytes, 16-byte aligned, needed (R * UNIVL_SAMPLE_SLICES * (8 k + 16)); got %lld",
                    (long long)need, (long long)d->ws_bytes);
    const int S = slices_for(d->V);
    const int64_t slots = (int64_t)d->R * S;
    ScanArgs a;
    a.x = d->x; a.ld = (long)d->ld; a.V = d->V; a.k = d->k; a.S = S;
    a.chunk = slice_chunk(d->V, S); a.vec = rows_vec4(d->x, d->ld);
    a.done = d->done;
    a.ws_sum = static_cast<double*>(d->ws);
    a.ws_max = reinterpret_cast<float*>(a.ws_sum + slots);
    a.ws_val = a.ws_max + slots;
    a.ws_idx = reinterpret_cast<int*>(a.ws_val + slots * d->k);
    hipLaunchKernelGGL(sample_scan_kernel, dim3(d->R, S), dim3(256), 0, stream, a);
    UNIVL_LAUNCH_CHECK();
    SelectArgs s;
    s.ws_sum = a.ws_sum; s.ws_max = a.ws_max; s.ws_val = a.ws_val; s.ws_idx = a.ws_idx;
    s.k = d->k; s.S = S; s.t = d->t; s.Tmax = d->Tmax; s.eos = d->eos;
    s.inv_T = d->inv_T; s.top_p = d->top_p; s.seed = d->seed;
    s.sampling_dev = d->sampling_dev; s.seed_dev = d->seed_dev; s.eos_dev = d->eos_dev;
    s.done = d->done; s.length = d->length; s.ids = d->ids;
    s.tokens_out = d->tokens_out; s.tok_logprob = d->tok_logprob; s.q_logprob = d->q_logprob;
    s.seq_logprob = d->seq_logprob; s.seq_q_logprob = d->seq_q_logprob;
    s.topk_idx = d->topk_idx; s.topk_val = d->topk_val;
    hipLaunchKernelGGL(sample_select_kernel, dim3(d->R), dim3(64), 0, stream, s);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}
