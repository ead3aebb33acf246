// Beam bookkeeping of caption decoding on the device (include/univl_hip.h: univl_beam_step, univl_beam_backtrack, univl_beam_captions).
//
// univl_beam_step is Beam.advance (modules/beam.py:63-87) for every instance of a batch at one position, as two launches:
//   phase 1  grid (rows, slices), 256 threads: a workgroup scans one slice of one row of the log-probabilities with 16-byte loads, each
//            thread keeping a SORTED top-n_bm of value = lp + the row's accumulated score in registers; the workgroup then takes n_bm
//            rounds of (value, index) arg-max over the threads' heads (wave shuffles + one LDS word pair per wave) and leaves its n_bm
//            best (value, column) pairs in the workspace.  The score is added HERE, before any comparison, so that ties the fp32 sum
//            creates between different log-probabilities of a row are seen by the tie rule like any other tie.
//   phase 2  one wave per instance: the n_bm best of the (1 or n_bm) x slices x n_bm pairs, then parents / tokens / state / history.
// Order of candidates everywhere: larger value first, equal values by LOWER flat index b * V + v first (`better`, ranked.h).
//
// The select kernels of the three steps are built from the same stages, each a function below: write_frozen, stage_pairs,
// best_rounds, write_winner; the walk-backs from clamp_len and walk_back.  On the host step_args states the common argument rule.
//
// univl_beam_group_step is Diverse Beam Search (Vijayakumar et al.: beam groups, Hamming diversity) on the same two launches.  The G
// groups of width k' = n_bm / G of an instance are the pseudo-instances i * G + g of an ordinary search of width k': `done`, `length`
// and the history are laid out that way, and phase 1 is the scan above with the frozen test reading done[row / k'] (its `stride`) while
// every row still keeps a top-n_bm.  Phase 2 (beam_group_select_kernel) takes the groups of an instance in order inside one wave.
// WHY THE PER-ROW TOP-n_bm IS ENOUGH.  A group ranks its candidates by value - lambda * c(v), c(v) = the number of beams of earlier live
// groups that chose v at this position, and keeps the k' best.  lambda >= 0, so the penalty only lowers a candidate (rounding is
// monotone: fl(value - p) <= value), and it touches at most (G - 1) k' distinct tokens.  Take a candidate x of row b outside that row's
// unpenalised top-n_bm: n_bm candidates of row b stand in front of it in the order above, at least n_bm - (G - 1) k' = k' of them
// unpenalised, and each of those k' still stands in front of x after the penalty (its ranked value is its value, x's is at most x's
// value, the index decides a tie as before).  So x is not among the group's k' best: a row's penalised top-k' lies inside its
// unpenalised top-n_bm, which lies inside the union of its slices' top-n_bm.  With lambda < 0 the argument fails (a candidate far down
// a row could be lifted past the list), which is why a negative penalty is refused.
//
// univl_beam_pool_step / univl_beam_pool_finish are beam search with a pool of finished hypotheses, a length penalty and an
// early-stopping switch, on the same two launches per position (include/univl_hip.h states the rule).  Live beams never hold the end
// token: phase 1 is the scan above with the end column left out (beam_scan_kernel<NB, true>), and phase 2 (beam_pool_select_kernel,
// which carries the sufficiency argument) reads the n_bm end-column values itself.  Keys are raw * w[len] with w a HOST-filled table:
// no powf on the device.  With no end token (eos < 0) the step is univl_beam_step bit for bit.
#include <cmath>

#include "common.h"
#include "ranked.h"
#include "univl_hip.h"

namespace {

template <int NB>
__device__ __forceinline__ void keep(float (&tv)[NB], int (&ti)[NB], float v, int i) {
    if (!better(v, i, tv[NB - 1], ti[NB - 1])) return;
    tv[NB - 1] = v; ti[NB - 1] = i;
#pragma unroll
    for (int j = NB - 1; j > 0; --j) {
        if (better(tv[j], ti[j], tv[j - 1], ti[j - 1])) {
            const float fv = tv[j]; tv[j] = tv[j - 1]; tv[j - 1] = fv;
            const int fi = ti[j]; ti[j] = ti[j - 1]; ti[j - 1] = fi;
        }
    }
}

// ws_val / ws_idx: [rows][slices][NB]; idx is the COLUMN within the row (RANK_NONE: empty)
// SKIP (univl_beam_pool_step): the end column is not a candidate of the scan; phase 2 reads it itself.  Without SKIP the two
// arguments behind it are not read and the code is the one the plain and the group step always had.
template <int NB, bool SKIP>
__global__ __launch_bounds__(256) void beam_scan_kernel(const float* __restrict__ lp, long ld, int V, int first_step, const float* __restrict__ scores,
                                                        const uint8_t* __restrict__ done, int stride, int chunk, int vec,
                                                        float* __restrict__ ws_val, int* __restrict__ ws_idx, int eos,
                                                        const int32_t* __restrict__ eos_dev) {
    __shared__ float red_v[2][4];
    __shared__ int red_i[2][4];
    // stride: rows per entry of done -- n_bm for univl_beam_step (an instance), k' for univl_beam_group_step (a group)
    const int inst = first_step ? (int)blockIdx.x : (int)blockIdx.x / stride;
    if (done[inst]) return;                                   // frozen instance: phase 2 does not read its slots
    const int row = first_step ? inst * stride : (int)blockIdx.x, slice = blockIdx.y, tid = threadIdx.x;
    const float add = first_step ? 0.f : scores[row];
    const int skip = SKIP ? (eos_dev ? *eos_dev : eos) : -1;  // never a column when negative
    const float* x = lp + (long)row * ld;
    const int c0 = slice * chunk, c1 = min(V, c0 + chunk);    // chunk is a multiple of 4
    float tv[NB];
    int ti[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) { tv[k] = -INFINITY; ti[k] = RANK_NONE; }
    if (vec) {
        // four 16-byte loads in flight per thread; columns >= V of the last word (padding up to ld) are never candidates
        for (int c = c0 + 4 * tid; c < c1; c += 4 * 1024) {
            f32x4_t q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int cu = c + u * 1024;
                q[u] = cu < c1 ? *reinterpret_cast<const f32x4_t*>(x + cu) : f32x4_t{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int cu = c + u * 1024;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (cu + e < c1 && !(SKIP && cu + e == skip)) keep<NB>(tv, ti, first_step ? q[u][e] : q[u][e] + add, cu + e);
            }
        }
    } else {
        for (int c = c0 + tid; c < c1; c += 256)
            if (!(SKIP && c == skip)) keep<NB>(tv, ti, first_step ? x[c] : x[c] + add, c);
    }
    // NB rounds: the best head of the workgroup; its owner (columns are unique to a thread) moves on to its next entry
    const int wave = tid >> 6;
    float* out_v = ws_val + ((long)row * gridDim.y + slice) * NB;
    int* out_i = ws_idx + ((long)row * gridDim.y + slice) * NB;
#pragma unroll
    for (int r = 0; r < NB; ++r) {
        float v = tv[0];
        int i = ti[0];
        wave_best(v, i);
        if ((tid & 63) == 0) { red_v[r & 1][wave] = v; red_i[r & 1][wave] = i; }
        __syncthreads();                                      // the other buffer is rewritten only after the NEXT barrier
        v = red_v[r & 1][0]; i = red_i[r & 1][0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (better(red_v[r & 1][w], red_i[r & 1][w], v, i)) { v = red_v[r & 1][w]; i = red_i[r & 1][w]; }
        if (tid == 0) { out_v[r] = v; out_i[r] = i; }
        if (i != RANK_NONE && ti[0] == i) {
#pragma unroll
            for (int k = 0; k + 1 < NB; ++k) { tv[k] = tv[k + 1]; ti[k] = ti[k + 1]; }
            tv[NB - 1] = -INFINITY; ti[NB - 1] = RANK_NONE;
        }
    }
}

struct BeamOut {
    float* scores; uint8_t* done; int32_t* length; int64_t* tokens; int32_t* src;
    int32_t* hist_parents; int32_t* hist_tokens; float* hist_scores;
};

__device__ __forceinline__ int clamp_len(int len, int Tmax) { return len < 0 ? 0 : (len > Tmax ? Tmax : len); }

// ---- the stages of phase 2; one wave, `lane` its thread.  A unit is what freezes together: an instance, or a group of one.
// A frozen unit of `width` beams from state slot s0: the state stays, the history row repeats it under identity parents.
__device__ __forceinline__ void write_frozen(const BeamOut& o, long hist_row, long s0, int width, int lane) {
    if (lane < width) {
        o.src[s0 + lane] = (int32_t)(s0 + lane);
        o.hist_parents[hist_row + s0 + lane] = lane;
        o.hist_tokens[hist_row + s0 + lane] = (int32_t)o.tokens[s0 + lane];
        o.hist_scores[hist_row + s0 + lane] = o.scores[s0 + lane];
    }
}

// The ncand workspace pairs from `at` on (per_row per row, the first of them the instance's beam b0) into LDS as (value, flat index
// b * V + column); also(c, value, column) sees every pair on its way (the group step's ranked value).
template <class Also>
__device__ __forceinline__ void stage_pairs(const float* ws_val, const int* ws_idx, long at, int ncand, int per_row,
                                            int b0, int V, float* cv, int* ci, int lane, Also also) {
    for (int c = lane; c < ncand; c += 64) {
        const int col = ws_idx[at + c];
        const float v = ws_val[at + c];
        cv[c] = v;
        also(c, v, col);
        ci[c] = col == RANK_NONE ? RANK_NONE : (b0 + c / per_row) * V + col;
    }
}

// n rounds of the wave's best (key, index) among the staged pairs; the lane that owns a round's winner (flat indices are unique: one
// owner) retires its slot.  take(r, v, i, at, own): what the kernel does with round r's winner (v, i), which every lane holds; `own`
// is true in the owner, whose slot it was at `at`.  i == RANK_NONE: nothing comparable was left.
template <class Take>
__device__ __forceinline__ void best_rounds(int n, float* key, int* ci, int ncand, int lane, Take take) {
    for (int r = 0; r < n; ++r) {
        float v = -INFINITY;
        int i = RANK_NONE, at = -1;
        for (int c = lane; c < ncand; c += 64)
            if (better(key[c], ci[c], v, i)) { v = key[c]; i = ci[c]; at = c; }
        const int mine = i;
        wave_best(v, i);
        const bool own = i != RANK_NONE && mine == i;
        if (own) { key[at] = -INFINITY; ci[at] = RANK_NONE; }
        take(r, v, i, at, own);
    }
}

// Winner (v, i) into slot `lane` of the unit whose first state slot is s0 and whose first beam within the instance is b0; the
// history's parent is local to the unit.  Returns the token.  Fewer comparable candidates than slots (NaN rows: unspecified result)
// must still leave in-range indices behind: an empty winner stands for column 0 of the slot's own row.
// (The pointer parameters of these stages carry no __restrict__ and the sums are spelled s0 + lane on purpose: with either changed
// the plain kernel's instructions change.)
__device__ __forceinline__ int write_winner(const BeamOut& o, long hist_row, long s0, int b0, int lane, float v, int i, int V) {
    const int flat = i == RANK_NONE ? (b0 + lane) * V : i, parent = flat / V, token = flat % V;
    o.scores[s0 + lane] = v;
    o.tokens[s0 + lane] = token;
    o.src[s0 + lane] = (int32_t)(s0 - b0 + parent);
    o.hist_parents[hist_row + s0 + lane] = parent - b0;
    o.hist_tokens[hist_row + s0 + lane] = token;
    o.hist_scores[hist_row + s0 + lane] = v;
    return token;
}

// one wave per instance; at most 8 x 8 x 8 = 512 pairs
__global__ __launch_bounds__(64) void beam_select_kernel(const float* __restrict__ ws_val, const int* __restrict__ ws_idx, int n_bm, int V, int slices,
                                                         int first_step, int eos, const int32_t* __restrict__ eos_dev, long hist_row, BeamOut o) {
    __shared__ float cv[512];
    __shared__ int ci[512];
    __shared__ float win_v[8];
    __shared__ int win_i[8];
    const int inst = blockIdx.x, lane = threadIdx.x;
    const long s0 = (long)inst * n_bm;                        // first row / state slot of the instance
    if (o.done[inst]) { write_frozen(o, hist_row, s0, n_bm, lane); return; }
    const int per_row = slices * n_bm, ncand = (first_step ? 1 : n_bm) * per_row;
    stage_pairs(ws_val, ws_idx, s0 * per_row, ncand, per_row, 0, V, cv, ci, lane, [](int, float, int) {});
    __syncthreads();
    best_rounds(n_bm, cv, ci, ncand, lane, [&](int r, float v, int i, int, bool) {
        if (lane == 0) { win_v[r] = v; win_i[r] = i; }
        __syncthreads();
    });
    if (lane < n_bm) {
        const int token = write_winner(o, hist_row, s0, 0, lane, win_v[lane], win_i[lane], V);
        if (lane == 0) {
            o.length[inst] += 1;
            if (token == (eos_dev ? *eos_dev : eos)) o.done[inst] = 1;               // beam.py:84: the TOP beam emitted EOS
        }
    }
}

// Row e of hyp: the len tokens that end in beam b of the instance at position len - 1, walked back through the history; -1 past them.
__device__ __forceinline__ void walk_back(const int32_t* __restrict__ hp, const int32_t* __restrict__ ht, int n_inst, int inst, int n_bm, int b,
                                          int len, int Tmax, int32_t* __restrict__ out) {
    for (int j = len; j < Tmax; ++j) out[j] = -1;
    for (int j = len - 1; j >= 0; --j) {
        b = b < 0 ? 0 : (b >= n_bm ? n_bm - 1 : b);            // a corrupt history (or pool) must not walk out of the arrays
        const long at = ((long)j * n_inst + inst) * n_bm + b;
        out[j] = ht[at];
        b = hp[at];
    }
}

__global__ __launch_bounds__(64) void beam_backtrack_kernel(const int32_t* __restrict__ hp, const int32_t* __restrict__ ht, const float* __restrict__ scores,
                                                            const int32_t* __restrict__ length, int n_inst, int n_bm, int n_best, int Tmax,
                                                            int32_t* __restrict__ hyp, float* __restrict__ hyp_scores) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= n_inst * n_best) return;
    const int inst = e / n_best, k = e % n_best;
    walk_back(hp, ht, n_inst, inst, n_bm, k, clamp_len(length[inst], Tmax), Tmax, hyp + (long)e * Tmax);
    hyp_scores[e] = scores[(long)inst * n_bm + k];
}

// The cut of main_task_caption.py:555-560 on the rows the walk-back wrote: one wave per hypothesis row, four rows per workgroup.
// Pass 1 reads 64 tokens at a time and takes the first matching lane from a ballot; pass 2 rewrites the row.  hyp and cap_tokens
// may be the same buffer (no __restrict__): every lane reads the word it is about to write, and a row belongs to one wave.
__global__ __launch_bounds__(256) void beam_captions_kernel(const int32_t* hyp, const int32_t* __restrict__ length, int rows, int n_best, int Tmax,
                                                            int eos, int pad, const int32_t* __restrict__ eos_dev, int32_t* cap_tokens,
                                                            int32_t* __restrict__ cap_len) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;                                  // whole waves leave: the ballots below see full rows only
    const int len = clamp_len(length[row / n_best], Tmax);
    const int end = eos_dev ? *eos_dev : eos;
    const int32_t* in = hyp + (long)row * Tmax;
    int32_t* out = cap_tokens + (long)row * Tmax;
    int cut = len;
    for (int j0 = 0; j0 < len; j0 += 64) {
        const int j = j0 + lane;
        const int tok = j < len ? in[j] : -1;
        const bool hit = j < len && ((end >= 0 && tok == end) || (pad >= 0 && tok == pad));
        const unsigned long long m = __ballot(hit);
        if (m) { cut = j0 + __ffsll(m) - 1; break; }          // m is wave-uniform: all lanes leave together
    }
    for (int j = lane; j < Tmax; j += 64) {
        const int tok = j < cut ? in[j] : -1;
        out[j] = tok;
    }
    if (lane == 0) cap_len[row] = cut;
}

// Phase 2 of univl_beam_group_step: one wave per instance, its G groups in order.  A group stages the (value, flat index) pairs of
// its own k' rows (at most 8 x 8 x 8 = 512 for G = 1) together with their ranked value, takes k' rounds of wave_best on `ranked`,
// re-sorts the k' winners by their unpenalised value and appends their tokens to pen_tok, the list the later stages count c(v) in
// (at most n_bm - k' entries when it is read; a token chosen by several beams stands there once per beam, so the count is the
// number of matches).  A frozen group writes its frozen rows and appends nothing.  Single wave, fixed order, no atomics.
__device__ __forceinline__ float ranked_value(float value, float lambda, int c) {
#pragma clang fp contract(off)                                // two roundings: the product, then the difference
    const float p = lambda * (float)c;
    return value - p;
}

__global__ __launch_bounds__(64) void beam_group_select_kernel(const float* __restrict__ ws_val, const int* __restrict__ ws_idx, int n_bm, int n_groups,
                                                               int V, int slices, int first_step, int eos, const int32_t* __restrict__ eos_dev,
                                                               float diversity, const float* __restrict__ diversity_dev, long hist_row, BeamOut o) {
    __shared__ float cv[512];                                 // unpenalised value: what is stored
    __shared__ float rk[512];                                 // ranked value: what is selected by
    __shared__ int ci[512];
    __shared__ float win_v[8], srt_v[8];
    __shared__ int win_i[8], srt_i[8];
    __shared__ int pen_tok[8];
    const int inst = blockIdx.x, lane = threadIdx.x, kp = n_bm / n_groups;
    const float lambda = diversity_dev ? *diversity_dev : diversity;
    const int end = eos_dev ? *eos_dev : eos;
    const int per_row = slices * n_bm;
    int npen = 0;                                             // wave-uniform
    for (int g = 0; g < n_groups; ++g) {
        const int grp = inst * n_groups + g, b0 = g * kp;     // the pseudo-instance; the group's first beam within the instance
        const long s0 = (long)inst * n_bm + b0;               // its first row / state slot
        if (o.done[grp]) { write_frozen(o, hist_row, s0, kp, lane); continue; }          // wave-uniform
        const int ncand = (first_step ? 1 : kp) * per_row;
        stage_pairs(ws_val, ws_idx, s0 * per_row, ncand, per_row, b0, V, cv, ci, lane, [&](int c, float v, int col) {
            int cnt = 0;
            for (int j = 0; j < npen; ++j) cnt += pen_tok[j] == col ? 1 : 0;
            rk[c] = ranked_value(v, lambda, cnt);
        });
        // a lane reads back only the slots it wrote (c = lane mod 64): no barrier until the winners are exchanged
        best_rounds(kp, rk, ci, ncand, lane, [&](int r, float, int i, int at, bool own) {
            if (own) { win_v[r] = cv[at]; win_i[r] = i; }      // selected by the ranked value, stored with the unpenalised one
            else if (i == RANK_NONE && lane == 0) { win_v[r] = -INFINITY; win_i[r] = RANK_NONE; }
        });
        __syncthreads();
        if (lane < kp) {                                      // place among the k' winners by (value, flat index); slot order settles empty ones
            const float mv = win_v[lane];
            const int mi = win_i[lane];
            int place = 0;
            for (int j = 0; j < kp; ++j)
                if (j != lane && (better(win_v[j], win_i[j], mv, mi) || (!better(mv, mi, win_v[j], win_i[j]) && j < lane))) ++place;
            srt_v[place] = mv; srt_i[place] = mi;
        }
        __syncthreads();
        if (lane < kp) {
            const int token = write_winner(o, hist_row, s0, b0, lane, srt_v[lane], srt_i[lane], V);
            pen_tok[npen + lane] = token;
            if (lane == 0) {
                o.length[grp] += 1;
                if (token == end) o.done[grp] = 1;
            }
        }
        npen += kp;
        __syncthreads();                                      // pen_tok is read, and win / srt rewritten, by the next stage
    }
}

// ---- the pooled search (univl_beam_pool_step, univl_beam_pool_finish)
struct BeamPool {
    const float* w; const int32_t* params;
    float* key; float* raw; int32_t* end_t; int32_t* beam; uint8_t* fin; int32_t* count;
};

// pool order: larger key first, then smaller end_t, then smaller beam
__device__ __forceinline__ bool pool_before(float ka, int ea, int ba, float kb, int eb, int bb) {
    return ka > kb || (ka == kb && (ea < eb || (ea == eb && ba < bb)));
}

// An instance's pool in the LDS of its one wave; slots are in arrival order, a replacement takes the slot of the entry it displaces.
struct PoolLds {
    float key[UNIVL_BEAM_MAX], raw[UNIVL_BEAM_MAX];
    int end_t[UNIVL_BEAM_MAX], beam[UNIVL_BEAM_MAX], fin[UNIVL_BEAM_MAX];
};

__device__ __forceinline__ int pool_last(const PoolLds& q, int cnt) {
    int last = 0;
    for (int j = 1; j < cnt; ++j)
        if (pool_before(q.key[last], q.end_t[last], q.beam[last], q.key[j], q.end_t[j], q.beam[j])) last = j;
    return last;
}

// one lane: append while there is room, else replace the last entry in pool order if the new one stands in front of it
__device__ __forceinline__ void pool_offer(PoolLds& q, int& cnt, int cap, float key, float raw, int end_t, int beam, int fin) {
    int slot = cnt;
    if (cnt < cap) {
        ++cnt;
    } else {
        slot = pool_last(q, cnt);
        if (!pool_before(key, end_t, beam, q.key[slot], q.end_t[slot], q.beam[slot])) return;
    }
    q.key[slot] = key; q.raw[slot] = raw; q.end_t[slot] = end_t; q.beam[slot] = beam; q.fin[slot] = fin;
}

__device__ __forceinline__ int pool_load(PoolLds& q, const BeamPool& p, long s0, int inst, int n_bm, int lane) {
    if (lane < n_bm) {
        q.key[lane] = p.key[s0 + lane]; q.raw[lane] = p.raw[s0 + lane]; q.end_t[lane] = p.end_t[s0 + lane];
        q.beam[lane] = p.beam[s0 + lane]; q.fin[lane] = p.fin[s0 + lane];
    }
    const int cnt = p.count[inst];
    return cnt < 0 ? 0 : (cnt > n_bm ? n_bm : cnt);
}

// Phase 2 of univl_beam_pool_step: one wave per instance.  The workspace holds each (row, slice)'s top-n_bm NON-END candidates
// (beam_scan_kernel<NB, SKIP>); the wave reads the (1 or n_bm) end-column values itself.
// WHY THAT IS ENOUGH.  Live beams: the first n_bm non-end candidates of the instance.  A non-end candidate x of row b outside that
// row's non-end top-n_bm has n_bm non-end candidates of its own row in front of it, so it is not among the instance's first n_bm; a
// row's non-end top-n_bm lies inside the union of its slices' non-end top-n_bm.  Finishing: a row has ONE end column, and ALL of them
// are read here, so none can be missed.  The rank of an end candidate e among all candidates is
//   #(non-end candidates in front of e) + #(end candidates in front of e);
// the second count is taken over the end values read here; for the first, the non-end candidates in front of e are a PREFIX of the
// non-end order, so counting over the n_bm live winners gives min(true count, n_bm) -- exact whenever rank < n_bm can still hold.
// A value of -inf (a column univl_decode_constrain masked) or NaN is not a candidate: `v > -inf` is false for both.
__global__ __launch_bounds__(64) void beam_pool_select_kernel(const float* __restrict__ ws_val, const int* __restrict__ ws_idx,
                                                              const float* __restrict__ lp, long ld, int n_bm, int V, int slices, int first_step,
                                                              int eos, const int32_t* __restrict__ eos_dev, int t, int Tmax, long hist_row,
                                                              BeamOut o, BeamPool p) {
    __shared__ float cv[512];
    __shared__ int ci[512];
    __shared__ float win_v[8], ev[8];
    __shared__ int win_i[8], ord[8];
    __shared__ PoolLds q;
    __shared__ int cnt_s;
    const int inst = blockIdx.x, lane = threadIdx.x;
    const long s0 = (long)inst * n_bm;                        // first row / state slot / pool slot of the instance
    if (o.done[inst]) { write_frozen(o, hist_row, s0, n_bm, lane); return; }          // the pool is untouched too
    const int end = eos_dev ? *eos_dev : eos, nrows = first_step ? 1 : n_bm;
    const bool has_end = end >= 0 && end < V;
    const int per_row = slices * n_bm, ncand = nrows * per_row;
    stage_pairs(ws_val, ws_idx, s0 * per_row, ncand, per_row, 0, V, cv, ci, lane, [](int, float, int) {});
    if (lane < 8) {                                           // the end candidates, formed as the scan forms a candidate
        float v = -INFINITY;
        if (has_end && lane < nrows) {
            const float x = lp[(s0 + lane) * ld + end];
            v = first_step ? x : x + o.scores[s0 + lane];
        }
        ev[lane] = v;
    }
    int cnt = pool_load(q, p, s0, inst, n_bm, lane);
    __syncthreads();
    best_rounds(n_bm, cv, ci, ncand, lane, [&](int r, float v, int i, int, bool) {        // the live beams: beam_select_kernel's rounds
        if (lane == 0) { win_v[r] = v; win_i[r] = i; }
        __syncthreads();
    });
    // lane b: the rank of end candidate b; the taken ones, in candidate order, into ord[]
    bool taken = false;
    if (lane < nrows) {
        const float v = ev[lane];
        const int fi = lane * V + end;
        if (v > -INFINITY) {
            int ahead = 0, ends_ahead = 0;
            for (int j = 0; j < n_bm; ++j) ahead += (win_i[j] != RANK_NONE && better(win_v[j], win_i[j], v, fi)) ? 1 : 0;
            for (int j = 0; j < nrows; ++j) ends_ahead += (j != lane && ev[j] > -INFINITY && better(ev[j], j * V + end, v, fi)) ? 1 : 0;
            taken = ahead + ends_ahead < n_bm;                // every end candidate in front of a taken one is taken: ends_ahead is its place
            if (taken) ord[ends_ahead] = lane;
        }
    }
    const int ntaken = __popcll(__ballot(taken));
    __syncthreads();
    if (lane < n_bm) write_winner(o, hist_row, s0, 0, lane, win_v[lane], win_i[lane], V);
    if (lane == 0) {
        const float wl = p.w[t + 1];                          // len = t + 1 <= Tmax
        for (int k = 0; k < ntaken; ++k) {
            const int b = ord[k];
            pool_offer(q, cnt, n_bm, ev[b] * wl, ev[b], t, b, 1);
        }
        o.length[inst] += 1;
        if (cnt == n_bm) {
            const int lmax = clamp_len(p.params[1], Tmax + 1);
            if (p.params[0] != 0 || win_v[0] * p.w[lmax] <= q.key[pool_last(q, cnt)]) o.done[inst] = 1;
        }
        p.count[inst] = cnt;
        cnt_s = cnt;
    }
    __syncthreads();
    if (ntaken && lane < cnt_s) {
        p.key[s0 + lane] = q.key[lane]; p.raw[s0 + lane] = q.raw[lane]; p.end_t[s0 + lane] = q.end_t[lane];
        p.beam[s0 + lane] = q.beam[lane]; p.fin[s0 + lane] = (uint8_t)q.fin[lane];
    }
}

struct PoolHyp {
    int32_t* tokens; float* raw; float* key; int32_t* len; uint8_t* fin;
};

// univl_beam_pool_finish: one wave per instance.  The live beams of an instance that is not done are offered (in LDS: the pool arrays
// themselves are only read), the pool is ranked in pool order and lane k < n_best writes hypothesis k.
__global__ __launch_bounds__(64) void beam_pool_finish_kernel(int n_inst, int n_bm, int n_best, int Tmax, int eos, const int32_t* __restrict__ eos_dev,
                                                              const float* __restrict__ scores, const uint8_t* __restrict__ done,
                                                              const int32_t* __restrict__ length, const int32_t* __restrict__ hp,
                                                              const int32_t* __restrict__ ht, BeamPool p, PoolHyp h) {
    __shared__ PoolLds q;
    __shared__ int cnt_s, srt[8];
    const int inst = blockIdx.x, lane = threadIdx.x;
    const long s0 = (long)inst * n_bm;
    int cnt = pool_load(q, p, s0, inst, n_bm, lane);
    __syncthreads();
    if (lane == 0) {
        if (!done[inst]) {
            const int len = clamp_len(length[inst], Tmax);
            const float wl = p.w[len];
            for (int b = 0; b < n_bm; ++b) pool_offer(q, cnt, n_bm, scores[s0 + b] * wl, scores[s0 + b], len, b, 0);
        }
        cnt_s = cnt;
    }
    __syncthreads();
    cnt = cnt_s;
    if (lane < cnt) {
        int place = 0;
        for (int j = 0; j < cnt; ++j)
            place += (j != lane && pool_before(q.key[j], q.end_t[j], q.beam[j], q.key[lane], q.end_t[lane], q.beam[lane])) ? 1 : 0;
        // (end_t, beam) is unique in a pool; equal entries (a corrupt pool) must still leave every srt slot written
        for (int j = 0; j < lane; ++j)
            place += (q.key[j] == q.key[lane] && q.end_t[j] == q.end_t[lane] && q.beam[j] == q.beam[lane]) ? 1 : 0;
        srt[place] = lane;
    }
    __syncthreads();
    if (lane >= n_best) return;
    const long e = (long)inst * n_best + lane;
    int32_t* out = h.tokens + e * Tmax;
    if (lane >= cnt) {                                        // an idle slot
        for (int j = 0; j < Tmax; ++j) out[j] = -1;
        h.raw[e] = -INFINITY; h.key[e] = -INFINITY; h.len[e] = 0; h.fin[e] = 0;
        return;
    }
    const int s = srt[lane], fin = q.fin[s] ? 1 : 0, ntok = clamp_len(q.end_t[s], Tmax);
    walk_back(hp, ht, n_inst, inst, n_bm, q.beam[s], ntok, Tmax, out);
    if (fin && ntok < Tmax) out[ntok] = eos_dev ? *eos_dev : eos;        // the end token that finished it: the row holds len tokens
    h.raw[e] = q.raw[s]; h.key[e] = q.key[s]; h.fin[e] = (uint8_t)fin;
    h.len[e] = fin && ntok < Tmax ? ntok + 1 : ntok;
}

// what the entry points hand to phase 1; n_units x stride = rows, done has n_units entries; eos / eos_dev: read by the SKIP form only
struct Scan {
    const float* lp; long ld; int V, first_step; const float* scores; const uint8_t* done; int n_units, stride;
    int eos = -1; const int32_t* eos_dev = nullptr;
};

template <int NB, bool SKIP>
void launch_scan(const Scan& a, int slices, int chunk, int vec, float* ws_val, int* ws_idx, hipStream_t stream) {
    const unsigned rows = a.first_step ? a.n_units : a.n_units * a.stride;
    hipLaunchKernelGGL((beam_scan_kernel<NB, SKIP>), dim3(rows, slices), dim3(256), 0, stream, a.lp, a.ld, a.V, a.first_step, a.scores, a.done,
                       a.stride, chunk, vec, ws_val, ws_idx, a.eos, a.eos_dev);
}

// Phase 1 with a sorted top-n_bm per (row, slice); returns the slices used.  ws: [rows][slices][n_bm] values, then as many indices.
template <bool SKIP = false>
int scan_rows(const Scan& a, int n_bm, void* ws, float** ws_val, int** ws_idx, hipStream_t stream) {
    const int64_t rows = (int64_t)a.n_units * a.stride;
    // slices: enough workgroups for the whole chip (~4 per CU at 80 rows), but at least 1024 columns each
    const int64_t scanned = a.first_step ? a.n_units : rows;
    int slices = (int)((1024 + scanned - 1) / scanned);
    const int by_len = (a.V + 1023) / 1024;
    slices = slices > by_len ? by_len : slices;
    slices = slices < 1 ? 1 : (slices > UNIVL_BEAM_SLICES ? UNIVL_BEAM_SLICES : slices);
    const int chunk = slice_chunk(a.V, slices), vec = rows_vec4(a.lp, a.ld);
    *ws_val = static_cast<float*>(ws);
    *ws_idx = reinterpret_cast<int*>(*ws_val + rows * slices * n_bm);
    switch (n_bm) {
        case 1: launch_scan<1, SKIP>(a, slices, chunk, vec, *ws_val, *ws_idx, stream); break;
        case 2: launch_scan<2, SKIP>(a, slices, chunk, vec, *ws_val, *ws_idx, stream); break;
        case 3: launch_scan<3, SKIP>(a, slices, chunk, vec, *ws_val, *ws_idx, stream); break;
        case 4: launch_scan<4, SKIP>(a, slices, chunk, vec, *ws_val, *ws_idx, stream); break;
        case 5: launch_scan<5, SKIP>(a, slices, chunk, vec, *ws_val, *ws_idx, stream); break;
        case 6: launch_scan<6, SKIP>(a, slices, chunk, vec, *ws_val, *ws_idx, stream); break;
        case 7: launch_scan<7, SKIP>(a, slices, chunk, vec, *ws_val, *ws_idx, stream); break;
        default: launch_scan<8, SKIP>(a, slices, chunk, vec, *ws_val, *ws_idx, stream); break;
    }
    return slices;
}

// The range that every descriptor entry point shares.
template <class D>
bool beam_dims_ok(const D* d) {
    return d->n_inst >= 1 && d->n_bm >= 1 && d->n_bm <= UNIVL_BEAM_MAX && (int64_t)d->n_inst * d->n_bm <= INT_MAX / 2;
}

// What a step entry point works with once step_args has accepted its descriptor; `scan` is the plain step's, the caller adjusts it.
struct Step {
    int64_t rows; long hist_row; int first_step; BeamOut o; Scan scan;
};

// The argument rule of UnivlBeamStep's fields, which UnivlBeamGroupStep and UnivlBeamPoolStep begin with in its order; `who` is the
// entry point's name.  UNIVL_OK, or UNIVL_EINVAL with the error text set.
template <class D>
int step_args(const char* who, const D* d, Step* s) {
    UNIVL_CHECK_ARG(d != nullptr, UNIVL_EINVAL, "%s: null descriptor", who);
    UNIVL_CHECK_ARG(beam_dims_ok(d) && d->V >= 1 && d->n_bm <= d->V && d->ld >= d->V && d->V <= INT_MAX / UNIVL_BEAM_MAX, UNIVL_EINVAL,
                    "%s: n_inst=%d n_bm=%d V=%d ld=%lld (1 <= n_bm <= %d, n_bm <= V <= ld)", who, d->n_inst, d->n_bm, d->V, (long long)d->ld,
                    UNIVL_BEAM_MAX);
    UNIVL_CHECK_ARG(d->t >= 0 && d->t < d->Tmax, UNIVL_EINVAL, "%s: history row t=%d of Tmax=%d", who, d->t, d->Tmax);
    UNIVL_CHECK_ARG(d->lp && d->scores && d->done && d->length && d->tokens && d->src && d->hist_parents && d->hist_tokens && d->hist_scores &&
                    d->ws, UNIVL_EINVAL, "%s: null pointer", who);
    const int64_t rows = (int64_t)d->n_inst * d->n_bm;
    const int64_t need = rows * UNIVL_BEAM_SLICES * d->n_bm * 8;
    UNIVL_CHECK_ARG(d->ws_bytes >= need && aligned16(d->ws), UNIVL_EINVAL,
                    "%s: workspace of %lld bytes, 16-byte aligned, needed (n_inst * n_bm * UNIVL_BEAM_SLICES * n_bm * 8); got %lld", who,
                    (long long)need, (long long)d->ws_bytes);
    const int first_step = d->first_step ? 1 : 0;
    *s = Step{rows, (long)d->t * rows, first_step,
              BeamOut{d->scores, d->done, d->length, d->tokens, d->src, d->hist_parents, d->hist_tokens, d->hist_scores},
              Scan{d->lp, (long)d->ld, d->V, first_step, d->scores, d->done, d->n_inst, d->n_bm}};
    return UNIVL_OK;
}

BeamPool pool_of(const UnivlBeamPoolStep* d) {
    return BeamPool{d->w, d->params, d->pool_key, d->pool_raw, d->pool_end_t, d->pool_beam, d->pool_finished, d->pool_count};
}

}  // namespace

extern "C" int univl_beam_step(const UnivlBeamStep* d, hipStream_t stream) {
    UNIVL_ON_STREAM_DEVICE(stream);
    Step s;
    if (const int rc = step_args("univl_beam_step", d, &s)) return rc;
    float* ws_val;
    int* ws_idx;
    const int slices = scan_rows(s.scan, d->n_bm, d->ws, &ws_val, &ws_idx, stream);
    UNIVL_LAUNCH_CHECK();
    hipLaunchKernelGGL(beam_select_kernel, dim3(d->n_inst), dim3(64), 0, stream, ws_val, ws_idx, d->n_bm, d->V, slices, s.first_step, d->eos,
                       d->eos_dev, s.hist_row, s.o);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}

extern "C" int univl_beam_group_step_sizeof(void) { return (int)sizeof(UnivlBeamGroupStep); }

extern "C" int univl_beam_group_step(const UnivlBeamGroupStep* d, hipStream_t stream) {
    UNIVL_ON_STREAM_DEVICE(stream);
    Step s;
    if (const int rc = step_args("univl_beam_group_step", d, &s)) return rc;
    UNIVL_CHECK_ARG(d->n_groups >= 1 && d->n_groups <= d->n_bm && d->n_bm % d->n_groups == 0, UNIVL_EINVAL,
                    "univl_beam_group_step: n_groups=%d does not divide n_bm=%d (1 <= n_groups <= n_bm)", d->n_groups, d->n_bm);
    UNIVL_CHECK_ARG(d->diversity_dev != nullptr || (std::isfinite(d->diversity) && d->diversity >= 0.f), UNIVL_EINVAL,
                    "univl_beam_group_step: diversity=%g, expected finite and >= 0 (the per-row top-n_bm lists hold every winner only then)",
                    (double)d->diversity);
    s.scan.n_units = d->n_inst * d->n_groups;                 // a group freezes on its own
    s.scan.stride = d->n_bm / d->n_groups;
    float* ws_val;
    int* ws_idx;
    const int slices = scan_rows(s.scan, d->n_bm, d->ws, &ws_val, &ws_idx, stream);
    UNIVL_LAUNCH_CHECK();
    hipLaunchKernelGGL(beam_group_select_kernel, dim3(d->n_inst), dim3(64), 0, stream, ws_val, ws_idx, d->n_bm, d->n_groups, d->V, slices,
                       s.first_step, d->eos, d->eos_dev, d->diversity, d->diversity_dev, s.hist_row, s.o);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}

extern "C" int univl_beam_pool_step_sizeof(void) { return (int)sizeof(UnivlBeamPoolStep); }

extern "C" int univl_beam_pool_step(const UnivlBeamPoolStep* d, hipStream_t stream) {
    UNIVL_ON_STREAM_DEVICE(stream);
    Step s;
    if (const int rc = step_args("univl_beam_pool_step", d, &s)) return rc;
    UNIVL_CHECK_ARG(d->w && d->params && d->pool_key && d->pool_raw && d->pool_end_t && d->pool_beam && d->pool_finished && d->pool_count,
                    UNIVL_EINVAL, "univl_beam_pool_step: null pointer (w, params or a pool array)");
    s.scan.eos = d->eos;                                      // the scan leaves the end column out
    s.scan.eos_dev = d->eos_dev;
    float* ws_val;
    int* ws_idx;
    const int slices = scan_rows<true>(s.scan, d->n_bm, d->ws, &ws_val, &ws_idx, stream);
    UNIVL_LAUNCH_CHECK();
    hipLaunchKernelGGL(beam_pool_select_kernel, dim3(d->n_inst), dim3(64), 0, stream, ws_val, ws_idx, d->lp, (long)d->ld, d->n_bm, d->V, slices,
                       s.first_step, d->eos, d->eos_dev, d->t, d->Tmax, s.hist_row, s.o, pool_of(d));
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}

extern "C" int univl_beam_pool_finish(const UnivlBeamPoolStep* d, int32_t n_best, int32_t* hyp, float* hyp_raw, float* hyp_key, int32_t* hyp_len,
                                      uint8_t* hyp_finished, hipStream_t stream) {
    UNIVL_ON_STREAM_DEVICE(stream);
    UNIVL_CHECK_ARG(d != nullptr, UNIVL_EINVAL, "univl_beam_pool_finish: null descriptor");
    UNIVL_CHECK_ARG(beam_dims_ok(d) && n_best >= 1 && n_best <= d->n_bm && d->Tmax >= 1, UNIVL_EINVAL,
                    "univl_beam_pool_finish: n_inst=%d n_bm=%d n_best=%d Tmax=%d (1 <= n_best <= n_bm <= %d)", d->n_inst, d->n_bm, n_best, d->Tmax,
                    UNIVL_BEAM_MAX);
    UNIVL_CHECK_ARG(d->scores && d->done && d->length && d->hist_parents && d->hist_tokens && d->w && d->pool_key && d->pool_raw &&
                    d->pool_end_t && d->pool_beam && d->pool_finished && d->pool_count && hyp && hyp_raw && hyp_key && hyp_len && hyp_finished,
                    UNIVL_EINVAL, "univl_beam_pool_finish: null pointer");
    PoolHyp h{hyp, hyp_raw, hyp_key, hyp_len, hyp_finished};
    hipLaunchKernelGGL(beam_pool_finish_kernel, dim3(d->n_inst), dim3(64), 0, stream, d->n_inst, d->n_bm, n_best, d->Tmax, d->eos, d->eos_dev,
                       d->scores, d->done, d->length, d->hist_parents, d->hist_tokens, pool_of(d), h);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}

extern "C" int univl_beam_backtrack(const int32_t* hist_parents, const int32_t* hist_tokens, const float* scores, const int32_t* length,
                                    int32_t n_inst, int32_t n_bm, int32_t n_best, int32_t Tmax, int32_t* hyp, float* hyp_scores,
                                    hipStream_t stream) {
    UNIVL_ON_STREAM_DEVICE(stream);
    UNIVL_CHECK_ARG(hist_parents && hist_tokens && scores && length && hyp && hyp_scores, UNIVL_EINVAL, "univl_beam_backtrack: null pointer");
    UNIVL_CHECK_ARG(n_inst >= 1 && n_bm >= 1 && n_bm <= UNIVL_BEAM_MAX && n_best >= 1 && n_best <= n_bm && Tmax >= 1 &&
                    (int64_t)n_inst * n_best <= INT_MAX / 2, UNIVL_EINVAL,
                    "univl_beam_backtrack: n_inst=%d n_bm=%d n_best=%d Tmax=%d (1 <= n_best <= n_bm <= %d)", n_inst, n_bm, n_best, Tmax, UNIVL_BEAM_MAX);
    const int total = n_inst * n_best;
    hipLaunchKernelGGL(beam_backtrack_kernel, dim3((total + 63) / 64), dim3(64), 0, stream, hist_parents, hist_tokens, scores, length, n_inst,
                       n_bm, n_best, Tmax, hyp, hyp_scores);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}

extern "C" int univl_beam_captions(const int32_t* hyp, const int32_t* length, int32_t n_inst, int32_t n_best, int32_t Tmax, int32_t eos,
                                   int32_t pad, const int32_t* eos_dev, int32_t* cap_tokens, int32_t* cap_len, hipStream_t stream) {
    UNIVL_ON_STREAM_DEVICE(stream);
    UNIVL_CHECK_ARG(hyp && length && cap_tokens && cap_len, UNIVL_EINVAL, "univl_beam_captions: null pointer");
    UNIVL_CHECK_ARG(n_inst >= 1 && n_best >= 1 && n_best <= UNIVL_BEAM_MAX && Tmax >= 1 && (int64_t)n_inst * n_best <= INT_MAX / 2, UNIVL_EINVAL,
                    "univl_beam_captions: n_inst=%d n_best=%d Tmax=%d (1 <= n_best <= %d, Tmax >= 1)", n_inst, n_best, Tmax, UNIVL_BEAM_MAX);
    const int rows = n_inst * n_best;
    hipLaunchKernelGGL(beam_captions_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, hyp, length, rows, n_best, Tmax, eos, pad, eos_dev,
                       cap_tokens, cap_len);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}
