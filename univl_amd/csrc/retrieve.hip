// Retrieval search on the device (include/univl_hip.h: univl_sim_topk): the k best gallery rows of every query row by inner product,
// and optionally the two rank counts of univl_rank_counts against an arbitrary target column, without the [Nq, Ng] score matrix.
//
// Two launches, no host read, capturable:
//   scan   grid (query tiles, gallery slices), 512 threads = 8 waves.  The query tile (16 or 32 rows x 768 fp32, pitch 772) is staged into
//          LDS once; the workgroup then walks its slice of the gallery in tiles of 128 rows.  Wave w owns gallery rows 16 w .. 16 w + 15 of
//          the tile and reads them STRAIGHT from global memory into MFMA operand fragments (lane (i, g) reads 16 bytes of row i at
//          k = 16 c + 4 g: a 64-byte piece per row and instruction, eight chunks = 512 contiguous bytes per row in flight, double buffered
//          in registers), the query fragments come from LDS.  One tile's scores go through a [queries][128] LDS buffer (two of them, so
//          that one barrier per tile is enough) to the wave that owns the query: waves keep 2 or 4 queries each, a query's running top-64
//          list is ONE ENTRY PER LANE of that wave, sorted.  Every score is compared with the query's current k-th entry first; the few
//          that pass are inserted one by one (ballot -> position, one shuffle to shift the tail).  The slice's k best and its counts go to
//          the workspace.
//   merge  one wave per query: the same insert over the slices' lists, then idx / score / gt / eq.
//
// SCORE CONTRACT.  s(i, j) is one accumulator chain: 48 chunks of 16 contraction indices in ascending order, 4 x v_mfma_f32_16x16x4_f32
// per chunk, starting from zero.  Neither the tile position of the row, the slice, the number of query blocks (16 / 32 row tiles run the
// same chain) nor deterministic mode enters it, and the target's score is computed by the same chain on gathered rows -- so equality of
// scores is meaningful (tie rule, eq) and pieces of a gallery searched separately merge exactly.  No float atomics anywhere.
// Order everywhere: larger score first, equal scores by LOWER gallery index first (`better`, ranked.h).
//
// QUERY-BANK NORMALISATION (univl_sim_colstat, univl_sim_topk_norm, univl_hub_flags, univl_hub_gate; contract in univl_hip.h).  The scan
// is templated on NORM: the NORM instantiation subtracts a per-column term from the scores of the gated queries where they leave the LDS
// score buffer, univl_sim_topk is the other instantiation.  The column term comes from the same tile loop (tile_scores) with the roles
// swapped -- gallery tile in LDS, bank rows streamed -- and a running (max, sum of exp) pair per gallery row instead of a ranked list;
// its reductions run in a fixed order and its slices depend on the bank size alone, so c_j is as pure as the scores are.
#include <float.h>
#include <stddef.h>
#include <string.h>
#include "common.h"
#include "ranked.h"
#include "univl_hip.h"

namespace {

constexpr int RT_H = 768;                   // contraction width (the pooled hidden size)
constexpr int RT_PITCH = RT_H + 4;          // LDS pitch of a query row: the 16 rows of a fragment read land in distinct banks
constexpr int RT_TILE = 128;                // gallery rows per tile = 8 waves x 16
constexpr int RT_SCP = RT_TILE + 4;         // pitch of the score buffer
constexpr int RT_WGS = 256;                 // workgroups the automatic slice count aims for (one per compute unit)

struct ScanArgs {
    const float* q; long ldq;
    const float* g; long ldg;
    int Nq, Ng, k, tiles, tps, S;          // tiles of the gallery, tiles per slice, slices
    const int32_t* target;
    float* ws_val; int32_t* ws_idx; int32_t* ws_cnt;     // [Nq][S][k], [Nq][S][k], [Nq][S][2]
    const float* bias; const int32_t* gate;              // NORM only: [Ng] column term, optional [Nq] gates
};

__device__ __forceinline__ void load8(f32x4_t (&f)[8], const float* p) {
#pragma unroll
    for (int c = 0; c < 8; ++c) f[c] = *reinterpret_cast<const f32x4_t*>(p + 16 * c);
}

// One tile's scores, the chain of the SCORE CONTRACT: the wave's 16 streamed rows (`cur` holds their first 8 chunks, gp points at
// them) against NB blocks of 16 rows kept in LDS at ls.  On return cur holds the first 8 chunks of the rows at gpn (the next tile).
// The GALLERY row is the MFMA's first operand and the QUERY row its second, whichever of the two is streamed: LDS_FIRST = false is the
// search (gallery streamed, queries in LDS), true the column term (gallery in LDS, bank rows streamed as the queries they are).
// acc[b] (lane (i, g), register r) = first-operand row 4 g + r, second-operand row i of the 16 x 16 block b.
template <int NB, bool LDS_FIRST>
__device__ __forceinline__ void tile_scores(f32x4_t (&acc)[NB], f32x4_t (&cur)[8], const float* gp, const float* gpn, const float* ls, int i,
                                            int gg) {
    f32x4_t nxt[8];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kg = 0; kg < RT_H / 128; ++kg) {
        load8(nxt, kg + 1 < RT_H / 128 ? gp + 128 * (kg + 1) : gpn);       // the next 8 chunks (of the next tile after the last group)
#pragma unroll
        for (int c = 0; c < 8; ++c) {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const f32x4_t lf = *reinterpret_cast<const f32x4_t*>(ls + (16 * b + i) * RT_PITCH + 128 * kg + 16 * c + 4 * gg);
                acc[b] = LDS_FIRST ? Mma<float>::mma(lf, cur[c], acc[b]) : Mma<float>::mma(cur[c], lf, acc[b]);
            }
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) cur[c] = nxt[c];
    }
}

// NQB: blocks of 16 queries per workgroup.  NORM: the scores are s'(i, j) = gate_i ? s(i, j) - bias_j : s(i, j) (univl_sim_topk_norm);
// the subtraction happens where a score leaves the LDS score buffer, and once more on the target's score.
template <int NQB, bool NORM>
__global__ __launch_bounds__(512) void sim_topk_scan_kernel(ScanArgs a) {
    constexpr int QT = 16 * NQB, NQW = QT / 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char rt_smem[];
    float* qs = reinterpret_cast<float*>(rt_smem);                   // [QT][RT_PITCH]
    float* sc = qs + QT * RT_PITCH;                                   // [2][QT][RT_SCP]
    float* tsc = sc + 2 * QT * RT_SCP;                                // [QT] target scores
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, gg = lane >> 4;
    const int q0 = blockIdx.x * QT, slice = blockIdx.y;

    for (int e = tid; e < QT * (RT_H / 4); e += 512) {
        const int r = e / (RT_H / 4), c4 = e % (RT_H / 4);
        f32x4_t v = {0.f, 0.f, 0.f, 0.f};
        if (q0 + r < a.Nq) v = *reinterpret_cast<const f32x4_t*>(a.q + (long)(q0 + r) * a.ldq + 4 * c4);
        *reinterpret_cast<f32x4_t*>(qs + r * RT_PITCH + 4 * c4) = v;
    }
    __syncthreads();

    // s(query, target[query]) by the chain of the main loop: wave w takes query block w against the gathered target rows; the
    // diagonal of its 16 x 16 tile sits in lane i + 16 (i / 4), register i % 4
    if (a.target != nullptr) {
        if (wave < NQB) {
            const int tq = q0 + 16 * wave + i;
            int tr = tq < a.Nq ? a.target[tq] : 0;
            tr = tr < 0 ? 0 : (tr >= a.Ng ? a.Ng - 1 : tr);          // a target out of range must not read outside the gallery
            const float* gp = a.g + (long)tr * a.ldg + 4 * gg;
            const float* qp = qs + (16 * wave + i) * RT_PITCH + 4 * gg;
            f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
            for (int c = 0; c < RT_H / 16; ++c)
                acc = Mma<float>::mma(*reinterpret_cast<const f32x4_t*>(gp + 16 * c), *reinterpret_cast<const f32x4_t*>(qp + 16 * c), acc);
            if (gg == (i >> 2)) {
                const int r = i & 3;
                float ts = r == 0 ? acc[0] : (r == 1 ? acc[1] : (r == 2 ? acc[2] : acc[3]));
                if constexpr (NORM) {
                    if (tq < a.Nq && (a.gate == nullptr || a.gate[tq] != 0)) ts = ts - a.bias[tr];
                }
                tsc[16 * wave + i] = ts;
            }
        }
        __syncthreads();
    }

    float lv[NQW], tv[NQW];
    int li[NQW], cgt[NQW], ceq[NQW];
#pragma unroll
    for (int u = 0; u < NQW; ++u) {
        lv[u] = -INFINITY; li[u] = RANK_NONE; cgt[u] = 0; ceq[u] = 0;
        tv[u] = a.target != nullptr ? tsc[wave * NQW + u] : 0.f;
    }
    [[maybe_unused]] bool gated[NQW];                                                      // NORM: this query's scores take the bias
    if constexpr (NORM) {
#pragma unroll
        for (int u = 0; u < NQW; ++u) {
            const int qrow = q0 + wave * NQW + u;
            gated[u] = qrow < a.Nq && (a.gate == nullptr || a.gate[qrow] != 0);
        }
    }

    const int t0 = slice * a.tps, t1 = min(a.tiles, t0 + a.tps);
    const long last = a.Ng - 1;
    // rows past the gallery's end read its last row (a valid address); their scores are never offered or counted
    const float* gp = a.g + min((long)t0 * RT_TILE + 16 * wave + i, last) * a.ldg + 4 * gg;
    f32x4_t cur[8];
    load8(cur, gp);
    for (int t = t0; t < t1; ++t) {
        const float* gpn = a.g + min((long)(t + 1) * RT_TILE + 16 * wave + i, last) * a.ldg + 4 * gg;
        const int j0 = t * RT_TILE;
        [[maybe_unused]] float cb[2];                                                      // NORM: the bias of this lane's two columns of the tile
        if constexpr (NORM) {
#pragma unroll
            for (int h = 0; h < 2; ++h) cb[h] = a.bias[min((long)j0 + 64 * h + lane, last)];
        }
        f32x4_t acc[NQB];
        tile_scores<NQB, false>(acc, cur, gp, gpn, qs, i, gg);
        gp = gpn;
        // accumulator (lane (i, g), register r) = gallery row 16 w + 4 g + r of the tile, query 16 b + i
        float* scb = sc + (t & 1) * QT * RT_SCP;
#pragma unroll
        for (int b = 0; b < NQB; ++b) *reinterpret_cast<f32x4_t*>(scb + (16 * b + i) * RT_SCP + 16 * wave + 4 * gg) = acc[b];
        __syncthreads();             // the other buffer is rewritten only after the NEXT barrier
#pragma unroll
        for (int u = 0; u < NQW; ++u) {
            const float* row = scb + (wave * NQW + u) * RT_SCP;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float s = row[64 * h + lane];
                if constexpr (NORM) s = gated[u] ? s - cb[h] : s;
                const bool ok = j0 + 64 * h + lane < a.Ng;
                if (a.target != nullptr) {
                    cgt[u] += (ok && s > tv[u]) ? 1 : 0;
                    ceq[u] += (ok && s == tv[u]) ? 1 : 0;
                }
                if (a.k > 0) list_offer_run(lv[u], li[u], a.k, s, j0 + 64 * h, ok, lane);
            }
        }
    }

#pragma unroll
    for (int u = 0; u < NQW; ++u) {
        const int qrow = q0 + wave * NQW + u;
        if (qrow >= a.Nq) continue;                                   // wave-uniform
        const long slot = (long)qrow * a.S + slice;
        if (lane < a.k) { a.ws_val[slot * a.k + lane] = lv[u]; a.ws_idx[slot * a.k + lane] = li[u]; }
        if (a.target != nullptr) {
            const int ngt = wave_sum_i(cgt[u]), neq = wave_sum_i(ceq[u]);
            if (lane == 0) { a.ws_cnt[slot * 2] = ngt; a.ws_cnt[slot * 2 + 1] = neq; }
        }
    }
}

__global__ __launch_bounds__(64) void sim_topk_merge_kernel(const float* __restrict__ ws_val, const int32_t* __restrict__ ws_idx,
                                                            const int32_t* __restrict__ ws_cnt, int S, int k, int counts,
                                                            int32_t* __restrict__ idx, float* __restrict__ score, int32_t* __restrict__ gt,
                                                            int32_t* __restrict__ eq) {
    const int row = blockIdx.x, lane = threadIdx.x;
    if (k > 0) {
        float lv = -INFINITY;
        int li = RANK_NONE;
        for (int s = 0; s < S; ++s) {
            const long at = ((long)row * S + s) * k + lane;
            const float v = lane < k ? ws_val[at] : -INFINITY;
            const int j = lane < k ? ws_idx[at] : RANK_NONE;
            list_offer_as<true, true>(lv, li, k, v, j, j != RANK_NONE, lane);      // COPY: see ranked.h
        }
        if (lane < k) {
            idx[(long)row * k + lane] = li == RANK_NONE ? -1 : li;
            score[(long)row * k + lane] = li == RANK_NONE ? -INFINITY : lv;
        }
    }
    if (counts) {
        int ngt = 0, neq = 0;
        for (int s = lane; s < S; s += 64) { ngt += ws_cnt[((long)row * S + s) * 2]; neq += ws_cnt[((long)row * S + s) * 2 + 1]; }
        ngt = wave_sum_i(ngt); neq = wave_sum_i(neq);
        if (lane == 0) { gt[row] = ngt; eq[row] = neq; }
    }
}

// tiles per slice, then the slices that leaves, for `want` slices of `tiles` tiles: no empty slice, one tile each where want > tiles
void slice_plan(int tiles, int want, int& tps, int& S) { tps = (tiles + want - 1) / want; S = (tiles + tps - 1) / tps; }
bool rows_ok(int n) { return n >= 1 && n <= INT_MAX - 2 * RT_TILE; }     // the scans index up to two tiles past the last row, in int

struct Plan { int nqb, qtiles, tiles, tps, S; };

Plan make_plan(int Nq, int Ng, int slices) {
    Plan p;
    p.nqb = Nq <= 16 ? 1 : 2;
    p.qtiles = (Nq + 16 * p.nqb - 1) / (16 * p.nqb);
    p.tiles = (Ng + RT_TILE - 1) / RT_TILE;
    // automatic: query tiles x slices fills the chip once -- a workgroup owns a compute unit's LDS, so a second round would only queue
    int want = slices > 0 ? slices : (RT_WGS + p.qtiles - 1) / p.qtiles;
    want = want > UNIVL_TOPK_SLICES_MAX ? UNIVL_TOPK_SLICES_MAX : want;
    slice_plan(p.tiles, want, p.tps, p.S);
    return p;
}

template <int NQB, bool NORM>
void launch_scan(const ScanArgs& a, const Plan& p, hipStream_t stream) {
    constexpr size_t smem = ((size_t)16 * NQB * RT_PITCH + (size_t)2 * 16 * NQB * RT_SCP + 16 * NQB) * sizeof(float);
    static bool done[UNIVL_MAX_DEVICES] = {};
    univl_allow_lds(sim_topk_scan_kernel<NQB, NORM>, smem, done);
    hipLaunchKernelGGL((sim_topk_scan_kernel<NQB, NORM>), dim3(p.qtiles, p.S), dim3(512), smem, stream, a);
}

// univl_sim_topk (bias == nullptr, `who` names it in the messages) and univl_sim_topk_norm: one set of checks, one plan, two
// instantiations of the scan
template <bool NORM>
int sim_topk_run(const char* who, const UnivlSimTopk* d, const float* bias, const int32_t* gate, hipStream_t stream) {
    UNIVL_CHECK_ARG(d->H == RT_H, UNIVL_EINVAL, "%s: H=%d (must be 768)", who, d->H);
    UNIVL_CHECK_ARG(d->Nq >= 1 && rows_ok(d->Ng), UNIVL_EINVAL, "%s: Nq=%d Ng=%d (both >= 1)", who, d->Nq, d->Ng);
    UNIVL_CHECK_ARG(d->k >= 0 && d->k <= UNIVL_TOPK_MAX, UNIVL_EINVAL, "%s: k=%d (0 <= k <= %d)", who, d->k, UNIVL_TOPK_MAX);
    UNIVL_CHECK_ARG(d->k > 0 || d->target != nullptr, UNIVL_EINVAL, "%s: k = 0 asks for the rank counts only and needs target", who);
    UNIVL_CHECK_ARG(d->slices >= 0 && d->slices <= UNIVL_TOPK_SLICES_MAX, UNIVL_EINVAL, "%s: slices=%d (0 = automatic, at most %d)", who,
                    d->slices, UNIVL_TOPK_SLICES_MAX);
    UNIVL_CHECK_ARG(d->q && d->g && d->ws, UNIVL_EINVAL, "%s: null pointer (q, g, ws)", who);
    UNIVL_CHECK_ARG(!NORM || bias != nullptr, UNIVL_EINVAL, "%s: null pointer (col_bias)", who);
    UNIVL_CHECK_ARG(d->k == 0 || (d->idx && d->score), UNIVL_EINVAL, "%s: null pointer (idx, score)", who);
    UNIVL_CHECK_ARG(d->target == nullptr || (d->gt && d->eq), UNIVL_EINVAL, "%s: null pointer (gt, eq with target)", who);
    UNIVL_CHECK_ARG(rows768_pitch(d->ldq) && rows768_pitch(d->ldg), UNIVL_EINVAL, "%s: ldq=%lld ldg=%lld (both >= 768)", who, (long long)d->ldq,
                    (long long)d->ldg);
    UNIVL_CHECK_ARG(rows768_aligned(d->q, d->ldq) && rows768_aligned(d->g, d->ldg) && aligned16(d->ws), UNIVL_EALIGN,
                    "%s: rows of q and g and the workspace must be 16-byte aligned", who);
    const Plan p = make_plan(d->Nq, d->Ng, d->slices);
    const int64_t need = univl_sim_topk_workspace(d->Nq, d->Ng, d->k, d->slices);       // THE formula; its own refusals are the checks above
    UNIVL_CHECK_ARG(d->ws_bytes >= need, UNIVL_EINVAL, "%s: workspace of %lld bytes needed (univl_sim_topk_workspace), got %lld", who,
                    (long long)need, (long long)d->ws_bytes);
    ScanArgs a;
    a.q = d->q; a.ldq = (long)d->ldq; a.g = d->g; a.ldg = (long)d->ldg;
    a.Nq = d->Nq; a.Ng = d->Ng; a.k = d->k; a.tiles = p.tiles; a.tps = p.tps; a.S = p.S;
    a.target = d->target;
    a.bias = bias; a.gate = gate;
    const int64_t slots = (int64_t)d->Nq * p.S;
    a.ws_val = static_cast<float*>(d->ws);
    a.ws_idx = reinterpret_cast<int32_t*>(a.ws_val + slots * d->k);
    a.ws_cnt = a.ws_idx + slots * d->k;
    if (p.nqb == 1) launch_scan<1, NORM>(a, p, stream);
    else launch_scan<2, NORM>(a, p, stream);
    UNIVL_LAUNCH_CHECK();
    hipLaunchKernelGGL(sim_topk_merge_kernel, dim3(d->Nq), dim3(64), 0, stream, a.ws_val, a.ws_idx, a.ws_cnt, p.S, d->k, d->target != nullptr ? 1 : 0,
                       d->idx, d->score, d->gt, d->eq);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}

// ------------------------------------------------------------------------------------------- the column term (univl_sim_colstat)
// A (max, sum of exp) pair stands for log-sum-exp over some bank rows: m = their largest score, l = sum exp(beta (s - m)).  The three
// functions below are the ONLY arithmetic between the scores and c_j; contraction is off in them, so that the same operations run
// wherever they are inlined.
__device__ __forceinline__ float lse_term(float beta, float s, float m) {
#pragma clang fp contract(off)
    const float x = beta * (s - m);
    return expf(x);
}
// (M, L) <- (M, L) joined with (m, l), the pair on the left covering the EARLIER bank rows
__device__ __forceinline__ void lse_fold(float& M, float& L, float m, float l, float beta) {
#pragma clang fp contract(off)
    const float n = fmaxf(M, m);
    const float a = L * lse_term(beta, M, n);
    const float b = l * lse_term(beta, m, n);
    M = n;
    L = a + b;
}
__device__ __forceinline__ float lse_value(float M, float L, float beta) {
#pragma clang fp contract(off)
    const float t = logf(L) / beta;
    return M + t;
}

constexpr int CS_QT = 32, CS_NQW = CS_QT / 8;        // gallery rows per workgroup (two blocks of 16), gallery rows per wave

struct ColArgs {
    const float* bank; long ldb;
    const float* g; long ldg;
    int Nb, Ng, tiles, tps, S;            // tiles of the bank, tiles per slice, slices
    float beta;
    float* ws_m; float* ws_l;             // [S][Ng] each
};

// sim_topk_scan_kernel with the roles swapped: the gallery tile (32 rows) is staged into LDS, wave w streams bank rows 16 w .. 16 w + 15
// of every 128-row bank tile of the slice, the tile's scores go through the LDS score buffer to the wave that owns the gallery row.
// That wave reduces the tile's 128 scores to one pair (two per lane, then the xor butterfly: a fixed tree) and folds it into the row's
// running pair, tiles in ascending order.
__global__ __launch_bounds__(512) void sim_colstat_scan_kernel(ColArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rt_smem[];
    float* gs = reinterpret_cast<float*>(rt_smem);                   // [CS_QT][RT_PITCH]
    float* sc = gs + CS_QT * RT_PITCH;                                // [2][CS_QT][RT_SCP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, gg = lane >> 4;
    const int g0 = blockIdx.x * CS_QT, slice = blockIdx.y;

    for (int e = tid; e < CS_QT * (RT_H / 4); e += 512) {
        const int r = e / (RT_H / 4), c4 = e % (RT_H / 4);
        f32x4_t v = {0.f, 0.f, 0.f, 0.f};
        if (g0 + r < a.Ng) v = *reinterpret_cast<const f32x4_t*>(a.g + (long)(g0 + r) * a.ldg + 4 * c4);
        *reinterpret_cast<f32x4_t*>(gs + r * RT_PITCH + 4 * c4) = v;
    }
    __syncthreads();

    float M[CS_NQW], L[CS_NQW];
#pragma unroll
    for (int u = 0; u < CS_NQW; ++u) { M[u] = -INFINITY; L[u] = 0.f; }

    const int t0 = slice * a.tps, t1 = min(a.tiles, t0 + a.tps);
    const long last = a.Nb - 1;
    // rows past the bank's end read its last row (a valid address); their scores enter no pair
    const float* bp = a.bank + min((long)t0 * RT_TILE + 16 * wave + i, last) * a.ldb + 4 * gg;
    f32x4_t cur[8];
    load8(cur, bp);
    for (int t = t0; t < t1; ++t) {
        const float* bpn = a.bank + min((long)(t + 1) * RT_TILE + 16 * wave + i, last) * a.ldb + 4 * gg;
        f32x4_t acc[2];
        tile_scores<2, true>(acc, cur, bp, bpn, gs, i, gg);
        bp = bpn;
        // accumulator (lane (i, g), register r) = gallery row 16 b + 4 g + r of the workgroup, bank row 16 w + i of the tile
        float* scb = sc + (t & 1) * CS_QT * RT_SCP;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
#pragma unroll
            for (int r = 0; r < 4; ++r) scb[(16 * b + 4 * gg + r) * RT_SCP + 16 * wave + i] = acc[b][r];
        }
        __syncthreads();             // the other buffer is rewritten only after the NEXT barrier
        const int j0 = t * RT_TILE;
        const bool ok0 = j0 + lane < a.Nb, ok1 = j0 + 64 + lane < a.Nb;
#pragma unroll
        for (int u = 0; u < CS_NQW; ++u) {
            const float* row = scb + (wave * CS_NQW + u) * RT_SCP;
            const float s0 = row[lane], s1 = row[64 + lane];
            const float m = wave_max(fmaxf(ok0 ? s0 : -INFINITY, ok1 ? s1 : -INFINITY));
            const float e0 = ok0 ? lse_term(a.beta, s0, m) : 0.f, e1 = ok1 ? lse_term(a.beta, s1, m) : 0.f;
            const float l = wave_sum(e0 + e1);
            if (t == t0) { M[u] = m; L[u] = l; }                      // wave-uniform
            else lse_fold(M[u], L[u], m, l, a.beta);
        }
    }

#pragma unroll
    for (int u = 0; u < CS_NQW; ++u) {
        const int grow = g0 + wave * CS_NQW + u;
        if (grow < a.Ng && lane == 0) { a.ws_m[(long)slice * a.Ng + grow] = M[u]; a.ws_l[(long)slice * a.Ng + grow] = L[u]; }
    }
}

__global__ __launch_bounds__(256) void sim_colstat_merge_kernel(const float* __restrict__ ws_m, const float* __restrict__ ws_l, int S, int Ng,
                                                                float beta, float* __restrict__ c) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= Ng) return;
    float M = ws_m[j], L = ws_l[j];
    for (int s = 1; s < S; ++s) lse_fold(M, L, ws_m[(long)s * Ng + j], ws_l[(long)s * Ng + j], beta);
    c[j] = lse_value(M, L, beta);
}

struct ColPlan { int gtiles, tiles, tps, S; };

// the slices are a function of Nb ALONE (the purity of c_j: include/univl_hip.h)
ColPlan make_col_plan(int Nb, int Ng) {
    ColPlan p;
    p.gtiles = (Ng + CS_QT - 1) / CS_QT;
    p.tiles = (Nb + RT_TILE - 1) / RT_TILE;
    slice_plan(p.tiles, UNIVL_COLSTAT_SLICES, p.tps, p.S);
    return p;
}

__global__ __launch_bounds__(256) void hub_flags_kernel(const int32_t* __restrict__ idx, long n, int Ng, int32_t* __restrict__ hub) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int j = idx[e];
    if (j >= 0 && j < Ng) hub[j] = 1;
}

__global__ __launch_bounds__(256) void hub_gate_kernel(const int32_t* __restrict__ top1, long ld, int Nq, const int32_t* __restrict__ hub, int Ng,
                                                       int32_t* __restrict__ gate) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Nq) return;
    const int j = top1[(long)q * ld];
    gate[q] = (j >= 0 && j < Ng && hub[j] != 0) ? 1 : 0;
}

}  // namespace

extern "C" int64_t univl_sim_topk_workspace(int32_t Nq, int32_t Ng, int32_t k, int32_t slices) {
    if (Nq < 1 || !rows_ok(Ng) || k < 0 || k > UNIVL_TOPK_MAX || slices < 0 || slices > UNIVL_TOPK_SLICES_MAX) {
        univl_set_error("univl_sim_topk_workspace: Nq=%d Ng=%d k=%d slices=%d", Nq, Ng, k, slices);
        return UNIVL_EINVAL;
    }
    return (int64_t)Nq * make_plan(Nq, Ng, slices).S * (8 * (int64_t)k + 8);       // [Nq][S] slots: k values, k indices, two counts
}

extern "C" int univl_sim_topk(const UnivlSimTopk* d, hipStream_t stream) {
    UNIVL_ON_STREAM_DEVICE(stream);
    UNIVL_CHECK_ARG(d != nullptr, UNIVL_EINVAL, "univl_sim_topk: null descriptor");
    return sim_topk_run<false>("univl_sim_topk", d, nullptr, nullptr, stream);
}

extern "C" int univl_sim_topk_norm_sizeof(void) { return (int)sizeof(UnivlSimTopkNorm); }

extern "C" int univl_sim_topk_norm(const UnivlSimTopkNorm* d, hipStream_t stream) {
    static_assert(offsetof(UnivlSimTopkNorm, col_bias) == sizeof(UnivlSimTopk) && offsetof(UnivlSimTopkNorm, ws_bytes) == offsetof(UnivlSimTopk, ws_bytes),
                  "UnivlSimTopkNorm begins with UnivlSimTopk's fields");
    UNIVL_ON_STREAM_DEVICE(stream);
    UNIVL_CHECK_ARG(d != nullptr, UNIVL_EINVAL, "univl_sim_topk_norm: null descriptor");
    UnivlSimTopk base;                                                // the common fields, copied: no access through another struct type
    memcpy(&base, d, sizeof(base));
    return sim_topk_run<true>("univl_sim_topk_norm", &base, d->col_bias, d->row_gate, stream);
}

extern "C" int univl_sim_colstat_sizeof(void) { return (int)sizeof(UnivlSimColstat); }

extern "C" int64_t univl_sim_colstat_workspace(int32_t Nb, int32_t Ng) {
    if (!rows_ok(Nb) || !rows_ok(Ng)) {
        univl_set_error("univl_sim_colstat_workspace: Nb=%d Ng=%d", Nb, Ng);
        return UNIVL_EINVAL;
    }
    return 8 * (int64_t)make_col_plan(Nb, Ng).S * Ng;
}

extern "C" int univl_sim_colstat(const UnivlSimColstat* d, hipStream_t stream) {
    UNIVL_ON_STREAM_DEVICE(stream);
    UNIVL_CHECK_ARG(d != nullptr, UNIVL_EINVAL, "univl_sim_colstat: null descriptor");
    UNIVL_CHECK_ARG(d->H == RT_H, UNIVL_EINVAL, "univl_sim_colstat: H=%d (must be 768)", d->H);
    UNIVL_CHECK_ARG(rows_ok(d->Nb) && rows_ok(d->Ng), UNIVL_EINVAL, "univl_sim_colstat: Nb=%d Ng=%d (both >= 1)", d->Nb, d->Ng);
    UNIVL_CHECK_ARG(d->beta > 0.f && d->beta <= FLT_MAX, UNIVL_EINVAL, "univl_sim_colstat: beta=%g (finite, > 0)", (double)d->beta);
    UNIVL_CHECK_ARG(d->bank && d->g && d->c && d->ws, UNIVL_EINVAL, "univl_sim_colstat: null pointer (bank, g, c, ws)");
    UNIVL_CHECK_ARG(rows768_pitch(d->ldb) && rows768_pitch(d->ldg), UNIVL_EINVAL, "univl_sim_colstat: ldb=%lld ldg=%lld (both >= 768)",
                    (long long)d->ldb, (long long)d->ldg);
    UNIVL_CHECK_ARG(rows768_aligned(d->bank, d->ldb) && rows768_aligned(d->g, d->ldg) && aligned16(d->ws), UNIVL_EALIGN,
                    "univl_sim_colstat: rows of bank and g and the workspace must be 16-byte aligned");
    const ColPlan p = make_col_plan(d->Nb, d->Ng);
    const int64_t need = univl_sim_colstat_workspace(d->Nb, d->Ng);                       // THE formula; its own refusals are the checks above
    UNIVL_CHECK_ARG(d->ws_bytes >= need, UNIVL_EINVAL, "univl_sim_colstat: workspace of %lld bytes needed (univl_sim_colstat_workspace), got %lld",
                    (long long)need, (long long)d->ws_bytes);
    ColArgs a;
    a.bank = d->bank; a.ldb = (long)d->ldb; a.g = d->g; a.ldg = (long)d->ldg;
    a.Nb = d->Nb; a.Ng = d->Ng; a.tiles = p.tiles; a.tps = p.tps; a.S = p.S; a.beta = d->beta;
    a.ws_m = static_cast<float*>(d->ws);
    a.ws_l = a.ws_m + (int64_t)p.S * d->Ng;
    constexpr size_t smem = ((size_t)CS_QT * RT_PITCH + (size_t)2 * CS_QT * RT_SCP) * sizeof(float);
    static bool done[UNIVL_MAX_DEVICES] = {};
    univl_allow_lds(sim_colstat_scan_kernel, smem, done);
    hipLaunchKernelGGL(sim_colstat_scan_kernel, dim3(p.gtiles, p.S), dim3(512), smem, stream, a);
    UNIVL_LAUNCH_CHECK();
    hipLaunchKernelGGL(sim_colstat_merge_kernel, dim3((d->Ng + 255) / 256), dim3(256), 0, stream, a.ws_m, a.ws_l, p.S, d->Ng, d->beta, d->c);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}

extern "C" int univl_hub_flags(const int32_t* idx, int64_t n, int32_t Ng, int32_t* hub, hipStream_t stream) {
    UNIVL_ON_STREAM_DEVICE(stream);
    UNIVL_CHECK_ARG(idx && hub && n >= 1 && Ng >= 1, UNIVL_EINVAL, "univl_hub_flags: idx, hub, n=%lld or Ng=%d", (long long)n, Ng);
    hipLaunchKernelGGL(hub_flags_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, idx, (long)n, Ng, hub);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}

extern "C" int univl_hub_gate(const int32_t* top1, int64_t ld, int32_t Nq, const int32_t* hub, int32_t Ng, int32_t* gate, hipStream_t stream) {
    UNIVL_ON_STREAM_DEVICE(stream);
    UNIVL_CHECK_ARG(top1 && hub && gate && ld >= 1 && Nq >= 1 && Ng >= 1, UNIVL_EINVAL, "univl_hub_gate: top1, hub, gate, ld=%lld, Nq=%d or Ng=%d",
                    (long long)ld, Nq, Ng);
    hipLaunchKernelGGL(hub_gate_kernel, dim3((Nq + 255) / 256), dim3(256), 0, stream, top1, (long)ld, Nq, hub, Ng, gate);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}
