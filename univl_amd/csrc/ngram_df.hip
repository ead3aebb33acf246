// Document-frequency tables of n-grams on the device (include/univl_hip.h: univl_ngram_df): the tables univl_caption_overlap reads
// for CIDEr, built from the token rows themselves.  No host read, no synchronisation; the launches of one call are ordered by the
// stream, and a kernel reads what an earlier one counted from device words in the workspace's head.
//
//   emit     one wave (64 threads) per document.  Its reference rows are staged one after the other as packed words (ngram_rows.h;
//            lane j owns positions j and j + 64).  A position's n-gram of reference r is emitted when it is valid and no equal key
//            stands at an earlier position of r or anywhere in a reference r' < r of the document: every lane compares its own keys,
//            n = 1 .. 4 at once, with the word every lane reads from the same LDS address (a broadcast read).  The emitted keys of all
//            four n go into one buffer: eight ballots, their popcounts, ONE integer atomic on the device cursor per reference row.
//   sort     LSD radix sort of the 64-bit keys, 8 passes of 8 bits, ping-pong between two buffers.  A pass is: per-tile digit
//            histogram (LDS atomics, integers); one exclusive scan over [256 digits][tiles], digit-major; a STABLE scatter -- a
//            workgroup walks its tile of UNIVL_NGRAM_DF_TILE keys in ascending order, 256 at a time; a lane's rank among the lanes
//            of its wave with the same digit comes from eight ballots ANDed into a peer mask and a popcount under the lower-lane
//            mask; the four waves are chained in order through LDS counts.  Keys are compared and bucketed as UNSIGNED numbers.
//   fold     head flags (key[i] != key[i - 1]) counted per tile, the same scan, then a compaction that writes each distinct key and
//            the position its run starts at; the last kernel turns starts into run lengths and finds df_begin by three lower-bound
//            searches in the distinct keys.
//
// The result is a function of the multiset of (document, key) pairs: the order in which the cursor hands out slots does not reach
// the output.  Integers only.  Every kernel bounds what it counted by what the host allocated, and every store is range-checked.
#include "common.h"
#include "ngram_rows.h"
#include "univl_hip.h"

namespace {

constexpr int MT = NGRAM_MT;
constexpr int TILE = UNIVL_NGRAM_DF_TILE;    // keys per workgroup and pass
constexpr int WG = 256;                      // threads of the sort and fold kernels
constexpr int STEPS = TILE / WG;
constexpr int SCAN_THREADS = 1024;
// device words at the head of the workspace (zeroed by the call)
constexpr int CTL_EMITTED = 0;               // the emit cursor: (document, key) pairs counted, may exceed what was stored
constexpr int CTL_DISTINCT = 1;              // distinct keys
constexpr int CTL_WORDS = 16;

struct RowTable {
    const int32_t* sym; long ld;
    const int32_t* len;
    int rows, T, n_refs;
    const int32_t* ref_begin; const int32_t* ref_rows;
};

__device__ __forceinline__ int stored_keys(const int32_t* ctl, int n_max) {
    const int n = ctl[CTL_EMITTED];
    return n < 0 ? 0 : (n > n_max ? n_max : n);
}

__global__ __launch_bounds__(64) void df_emit_kernel(RowTable a, uint64_t* keys, int n_max, int32_t* ctl, int32_t* status) {
    __shared__ uint32_t cs[MT + 4], os[MT + 4];
    __shared__ uint64_t ck[MT], ok[MT];
    const int doc = blockIdx.x, lane = threadIdx.x;
    int flags = 0;
    int rb = a.ref_begin[doc], re = a.ref_begin[doc + 1];
    if (rb < 0 || rb > a.n_refs || re < rb || re > a.n_refs) {         // offsets outside the list or decreasing; an empty document is fine
        flags |= UNIVL_OVERLAP_BAD_REFS;
        rb = rb < 0 ? 0 : (rb > a.n_refs ? a.n_refs : rb);
        re = re > a.n_refs ? a.n_refs : re;
        if (re < rb) re = rb;
    }
    for (int r = rb; r < re; ++r) {
        __syncthreads();                                               // the previous reference's words are no longer read
        const int L = stage_row(a, a.ref_rows[r], cs, ck, lane, flags);
        uint64_t key[4][2];
        bool dup[4][2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int p = lane + 64 * h;
            const uint64_t w = ck[p];
#pragma unroll
            for (int n = 1; n <= 4; ++n) {
                key[n - 1][h] = p + n <= L ? (w & mask_n(n)) : 0ULL;   // 0 equals no n-gram
                dup[n - 1][h] = false;
            }
        }
        for (int q = 0; q < L; ++q) {                                  // earlier positions of this row
            const uint64_t w = ck[q];
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const uint64_t g = w & mask_n(n + 1);
#pragma unroll
                for (int h = 0; h < 2; ++h) dup[n][h] = dup[n][h] || (q < lane + 64 * h && g == key[n][h]);
            }
        }
        for (int e = rb; e < r; ++e) {                                 // every position of the document's earlier rows
            __syncthreads();
            const int Le = stage_row(a, a.ref_rows[e], os, ok, lane, flags);
            for (int q = 0; q < Le; ++q) {
                const uint64_t w = ok[q];
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const uint64_t g = w & mask_n(n + 1);
#pragma unroll
                    for (int h = 0; h < 2; ++h) dup[n][h] = dup[n][h] || g == key[n][h];
                }
            }
        }
        // ---- one slot range for the row: eight ballots, one atomic
        int before[4][2], total = 0;
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint64_t m = __ballot(key[n][h] != 0ULL && !dup[n][h]);
                before[n][h] = total + __popcll(m & ((1ULL << lane) - 1ULL));
                total += __popcll(m);
            }
        int base = 0;
        if (lane == 0 && total > 0) base = atomicAdd(&ctl[CTL_EMITTED], total);
        base = __shfl(base, 0, 64);
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const long at = (long)base + before[n][h];
                if (key[n][h] != 0ULL && !dup[n][h] && at >= 0 && at < n_max) keys[at] = key[n][h];
            }
    }
    if (flags) atomicOr(status, flags);
}

// hist[digit * tiles + tile] = the number of the tile's keys with that digit
__global__ __launch_bounds__(WG) void df_hist_kernel(const uint64_t* keys, int n_max, const int32_t* ctl, int shift, int32_t* hist) {
    __shared__ int h[256];
    const int n = stored_keys(ctl, n_max), tiles = (n + TILE - 1) / TILE, tile = blockIdx.x, t = threadIdx.x;
    if (tile >= tiles) return;
    h[t] = 0;
    __syncthreads();
#pragma unroll 4
    for (int s = 0; s < STEPS; ++s) {
        const int i = tile * TILE + s * WG + t;
        if (i < n) atomicAdd(&h[(int)((keys[i] >> shift) & 255ULL)], 1);
    }
    __syncthreads();
    hist[t * tiles + tile] = h[t];
}

// x[0 .. total) <- its exclusive prefix sums, total = rows * tiles (rows == 256) or tiles (rows == 1); *sum (optional) <- the sum.
// One workgroup; a thread owns a contiguous piece.
__global__ __launch_bounds__(SCAN_THREADS) void df_scan_kernel(int32_t* x, int rows, int n_max, const int32_t* ctl, int32_t* sum) {
    __shared__ int wave_total[SCAN_THREADS / 64];
    const int n = stored_keys(ctl, n_max), tiles = (n + TILE - 1) / TILE;
    const long total = (long)rows * tiles;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const long piece = (total + SCAN_THREADS - 1) / SCAN_THREADS;
    const long lo = t * piece < total ? t * piece : total, hi = lo + piece < total ? lo + piece : total;
    int mine = 0;
    for (long i = lo; i < hi; ++i) mine += x[i];
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wave_total[w] = incl;
    __syncthreads();
    int run = incl - mine;
    for (int k = 0; k < w; ++k) run += wave_total[k];
    for (long i = lo; i < hi; ++i) {
        const int v = x[i];
        x[i] = run;
        run += v;
    }
    if (sum != nullptr && t == SCAN_THREADS - 1) *sum = run;          // the last thread ends on the whole sum (its piece may be empty)
}

__global__ __launch_bounds__(WG) void df_scatter_kernel(const uint64_t* in, uint64_t* out, int n_max, const int32_t* ctl, int shift,
                                                        const int32_t* offs) {
    __shared__ int base[256];
    __shared__ int wcnt[WG / 64][256];
    const int n = stored_keys(ctl, n_max), tiles = (n + TILE - 1) / TILE, tile = blockIdx.x, t = threadIdx.x;
    if (tile >= tiles) return;
    const int lane = t & 63, w = t >> 6;
    base[t] = offs[t * tiles + tile];
#pragma unroll
    for (int k = 0; k < WG / 64; ++k) wcnt[k][t] = 0;
    __syncthreads();
    for (int s = 0; s < STEPS; ++s) {
        const int i = tile * TILE + s * WG + t;
        const bool valid = i < n;
        const uint64_t key = valid ? in[i] : 0ULL;
        const int d = (int)((key >> shift) & 255ULL);
        uint64_t peer = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const uint64_t m = __ballot((d >> b) & 1);
            peer &= ((d >> b) & 1) ? m : ~m;
        }
        const int rank = __popcll(peer & ((1ULL << lane) - 1ULL));
        if (valid && rank == 0) wcnt[w][d] = __popcll(peer);
        __syncthreads();
        if (valid) {
            int at = base[d] + rank;
            for (int k = 0; k < w; ++k) at += wcnt[k][d];
            if (at >= 0 && at < n) out[at] = key;
        }
        __syncthreads();
        int add = 0;
#pragma unroll
        for (int k = 0; k < WG / 64; ++k) { add += wcnt[k][t]; wcnt[k][t] = 0; }
        base[t] += add;
        __syncthreads();
    }
}

__device__ __forceinline__ bool is_head(const uint64_t* keys, int i, int n) { return i < n && (i == 0 || keys[i] != keys[i - 1]); }

// heads[tile] = the number of positions of the tile whose key differs from the one before
__global__ __launch_bounds__(WG) void df_heads_kernel(const uint64_t* keys, int n_max, const int32_t* ctl, int32_t* heads) {
    __shared__ int wsum[WG / 64];
    const int n = stored_keys(ctl, n_max), tiles = (n + TILE - 1) / TILE, tile = blockIdx.x, t = threadIdx.x;
    if (tile >= tiles) return;
    int c = 0;
    for (int s = 0; s < STEPS; ++s) c += is_head(keys, tile * TILE + s * WG + t, n) ? 1 : 0;
    c = wave_sum_i(c);
    if ((t & 63) == 0) wsum[t >> 6] = c;
    __syncthreads();
    if (t == 0) {
        int all = 0;
        for (int k = 0; k < WG / 64; ++k) all += wsum[k];
        heads[tile] = all;
    }
}

// the u-th distinct key -> df_keys[u] (u < capacity) and the position its run starts at -> start[u] (u <= capacity)
__global__ __launch_bounds__(WG) void df_compact_kernel(const uint64_t* keys, int n_max, const int32_t* ctl, const int32_t* offs,
                                                        uint64_t* df_keys, int32_t* start, int capacity) {
    __shared__ int wsum[WG / 64];
    const int n = stored_keys(ctl, n_max), tiles = (n + TILE - 1) / TILE, tile = blockIdx.x, t = threadIdx.x;
    if (tile >= tiles) return;
    const int lane = t & 63, w = t >> 6;
    int run = offs[tile];
    for (int s = 0; s < STEPS; ++s) {
        const int i = tile * TILE + s * WG + t;
        const bool head = is_head(keys, i, n);
        const uint64_t m = __ballot(head);
        if (lane == 0) wsum[w] = __popcll(m);
        __syncthreads();
        int u = run + __popcll(m & ((1ULL << lane) - 1ULL)), all = 0;
#pragma unroll
        for (int k = 0; k < WG / 64; ++k) {
            u += k < w ? wsum[k] : 0;
            all += wsum[k];
        }
        if (head && u >= 0 && u <= capacity) {
            start[u] = i;
            if (u < capacity) df_keys[u] = keys[i];
        }
        run += all;
        __syncthreads();
    }
}

// run lengths, df_begin, the overflow flag
__global__ __launch_bounds__(WG) void df_finish_kernel(int n_max, const int32_t* ctl, const uint64_t* df_keys, const int32_t* start,
                                                       int capacity, int32_t* df_cnt, int32_t* df_begin, int32_t* status) {
    const int n = stored_keys(ctl, n_max), distinct = ctl[CTL_DISTINCT];
    const int kept = distinct < capacity ? distinct : capacity;
    const int u = blockIdx.x * WG + threadIdx.x;
    if (u < kept) df_cnt[u] = (u + 1 < distinct ? start[u + 1] : n) - start[u];
    if (u != 0) return;
    if (distinct > capacity || ctl[CTL_EMITTED] > n_max) atomicOr(status, UNIVL_NGRAM_DF_OVERFLOW);
    df_begin[0] = 0;
    for (int k = 1; k < 4; ++k) {                                      // the first key of k + 1 symbols or more
        const uint64_t bound = 1ULL << (16 * k);
        int lo = 0, hi = kept;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (df_keys[mid] < bound) lo = mid + 1; else hi = mid;
        }
        df_begin[k] = lo;
    }
    df_begin[4] = kept;
}

long key_bound(int n_refs, int T) { return 4L * T * n_refs; }
long tiles_of(long n) { return (n + TILE - 1) / TILE; }

}  // namespace

extern "C" int univl_ngram_df_sizeof(void) { return (int)sizeof(UnivlNgramDf); }

extern "C" int univl_ngram_df_tile(void) { return TILE; }

extern "C" int64_t univl_ngram_df_ws_bytes(int32_t n_refs, int32_t T) {
    if (n_refs < 1 || T < 1 || T > UNIVL_OVERLAP_TMAX || key_bound(n_refs, T) > 0x7FFFFFFFL) return -1;
    const long N = key_bound(n_refs, T);
    return (int64_t)(4 * CTL_WORDS + 16 * N + 1024 * tiles_of(N));
}

extern "C" int univl_ngram_df(const UnivlNgramDf* d, hipStream_t stream) {
    UNIVL_ON_STREAM_DEVICE(stream);
    UNIVL_CHECK_ARG(d != nullptr, UNIVL_EINVAL, "univl_ngram_df: null descriptor");
    UNIVL_CHECK_ARG(d->T >= 1 && d->T <= UNIVL_OVERLAP_TMAX && d->ld >= d->T && d->rows >= 1 && d->items >= 1 && d->n_refs >= 1 &&
                    d->capacity >= 1, UNIVL_EINVAL, "univl_ngram_df: rows=%d T=%d ld=%lld items=%d n_refs=%d capacity=%d (1 <= T <= %d, "
                    "T <= ld, rows, items, n_refs, capacity >= 1)", d->rows, d->T, (long long)d->ld, d->items, d->n_refs, d->capacity,
                    UNIVL_OVERLAP_TMAX);
    UNIVL_CHECK_ARG(d->sym && d->len && d->ref_begin && d->ref_rows && d->df_keys && d->df_cnt && d->df_begin && d->status && d->ws,
                    UNIVL_EINVAL, "univl_ngram_df: null pointer");
    const int64_t need = univl_ngram_df_ws_bytes(d->n_refs, d->T);
    UNIVL_CHECK_ARG(need > 0 && d->ws_bytes >= need, UNIVL_EINVAL, "univl_ngram_df: workspace of %lld bytes, %lld needed for n_refs=%d T=%d "
                    "(n_refs * 4 T keys must stay below 2^31)", (long long)d->ws_bytes, (long long)need, d->n_refs, d->T);
    UNIVL_CHECK_ARG(aligned16(d->ws), UNIVL_EALIGN, "univl_ngram_df: the workspace must be 16-byte aligned");
    const int N = (int)key_bound(d->n_refs, d->T), tiles = (int)tiles_of(N);
    int32_t* ctl = static_cast<int32_t*>(d->ws);
    uint64_t* buf_a = reinterpret_cast<uint64_t*>(ctl + CTL_WORDS);
    uint64_t* buf_b = buf_a + N;
    int32_t* hist = reinterpret_cast<int32_t*>(buf_b + N);
    hipError_t e = hipMemsetAsync(ctl, 0, 4 * CTL_WORDS, stream);
    if (e != hipSuccess) { univl_set_error("univl_ngram_df: hipMemsetAsync: %s", hipGetErrorString(e)); return (int)e; }
    RowTable a;
    a.sym = d->sym; a.ld = (long)d->ld; a.len = d->len; a.rows = d->rows; a.T = d->T; a.n_refs = d->n_refs;
    a.ref_begin = d->ref_begin; a.ref_rows = d->ref_rows;
    hipLaunchKernelGGL(df_emit_kernel, dim3(d->items), dim3(64), 0, stream, a, buf_a, N, ctl, d->status);
    UNIVL_LAUNCH_CHECK();
    uint64_t* in = buf_a;
    uint64_t* out = buf_b;
    for (int shift = 0; shift < 64; shift += 8) {                      // an even number of passes: the sorted keys end in buf_a
        hipLaunchKernelGGL(df_hist_kernel, dim3(tiles), dim3(WG), 0, stream, in, N, ctl, shift, hist);
        hipLaunchKernelGGL(df_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, hist, 256, N, ctl, (int32_t*)nullptr);
        hipLaunchKernelGGL(df_scatter_kernel, dim3(tiles), dim3(WG), 0, stream, in, out, N, ctl, shift, hist);
        UNIVL_LAUNCH_CHECK();
        uint64_t* t = in; in = out; out = t;
    }
    int32_t* start = reinterpret_cast<int32_t*>(buf_b);               // free again: N + 1 words fit in N keys
    hipLaunchKernelGGL(df_heads_kernel, dim3(tiles), dim3(WG), 0, stream, buf_a, N, ctl, hist);
    hipLaunchKernelGGL(df_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, hist, 1, N, ctl, ctl + CTL_DISTINCT);
    hipLaunchKernelGGL(df_compact_kernel, dim3(tiles), dim3(WG), 0, stream, buf_a, N, ctl, hist, d->df_keys, start, d->capacity);
    const int kept_max = d->capacity < N ? d->capacity : N;
    hipLaunchKernelGGL(df_finish_kernel, dim3((kept_max + WG - 1) / WG), dim3(WG), 0, stream, N, ctl, d->df_keys, start, d->capacity,
                       d->df_cnt, d->df_begin, d->status);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}
