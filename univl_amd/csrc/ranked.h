// Ranked candidates on the device: the one statement of the order that the beam step (beam.hip), the sample step (sample.hip), the retrieval
// search (retrieve.hip) and the arg-max of the vocabulary head (vocab_ce.h) share, and of the wave-wide mechanisms built on it.
// Included after common.h.  Device code, except the last two functions: slice_chunk and rows_vec4 are HOST-side launch rules of the
// beam and sample scans (rows_vec4 uses common.h's aligned16).
//
// Order of candidates everywhere: larger value first, equal values by LOWER index first (`better`).  A comparison with a NaN value is
// false both ways: NaN candidates are never taken, what a row of them returns is unspecified but in range.
// RANK_NONE is the index of an empty slot; with the value -inf it loses against every real candidate of any value.
#pragma once
#include <limits.h>
#include <type_traits>

constexpr int RANK_NONE = INT_MAX;

__device__ __forceinline__ bool better(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

// the best (v, i) of every aligned group of W lanes, left in all of them
template <int W = 64>
__device__ __forceinline__ void wave_best(float& v, int& i) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) {
        const float w = __shfl_xor(v, o, 64);
        const int j = __shfl_xor(i, o, 64);
        if (better(w, j, v, i)) { v = w; i = j; }
    }
}

// A wave-wide list with ONE ENTRY PER LANE, sorted best first: (lv, li) is this lane's entry, the first k lanes are the list.
// Inserts the wave-uniform candidate; the last entry falls off.
__device__ __forceinline__ void list_insert(float& lv, int& li, float cv, int ci, int lane) {
    const int pos = __popcll(__ballot(better(lv, li, cv, ci)));      // the entries that stay in front of it are a prefix
    const float uv = __shfl_up(lv, 1, 64);
    const int ui = __shfl_up(li, 1, 64);
    if (lane == pos) { lv = cv; li = ci; }
    else if (lane > pos) { lv = uv; li = ui; }
}

// Offers every lane's candidate with ok != 0 to the list: tested against the k-th entry BEFORE any insert, and again when its turn
// comes, so that the few that pass cost an insert and the rest one comparison.  Called by whole waves only.
// OWN: lane b brings its own index i; otherwise the candidates are numbered i + b and no index is shuffled.
// COPY: the loop runs on a copy of the entry, written back at the end.  Same result; it is the form in which the compiler keeps
// list_insert's update as two selects in sim_topk_merge_kernel, where through the references it emits two branches (+17 instructions,
// +1.7 us at 64 queries x 128 slices).  The scan kernels get their shortest code without it.
template <bool OWN, bool COPY = false>
__device__ __forceinline__ void list_offer_as(float& lv_, int& li_, int k, float v, int i, bool ok, int lane) {
    std::conditional_t<COPY, float, float&> lv = lv_;
    std::conditional_t<COPY, int, int&> li = li_;
    float kv = __shfl(lv, k - 1, 64);
    int ki = __shfl(li, k - 1, 64);
    unsigned long long m = __ballot(ok && better(v, OWN ? i : i + lane, kv, ki));
    while (m) {                                                       // wave-uniform
        const int b = __ffsll((long long)m) - 1;
        m &= m - 1;
        const float cv = __shfl(v, b, 64);
        const int ci = OWN ? __shfl(i, b, 64) : i + b;
        if (better(cv, ci, kv, ki)) {
            list_insert(lv, li, cv, ci, lane);
            kv = __shfl(lv, k - 1, 64);
            ki = __shfl(li, k - 1, 64);
        }
    }
    if constexpr (COPY) { lv_ = lv; li_ = li; }
}
__device__ __forceinline__ void list_offer(float& lv, int& li, int k, float v, int i, bool ok, int lane) {
    list_offer_as<true>(lv, li, k, v, i, ok, lane);
}
// the candidates of a contiguous run: lane b offers (v, base + b)
__device__ __forceinline__ void list_offer_run(float& lv, int& li, int k, float v, int base, bool ok, int lane) {
    list_offer_as<false>(lv, li, k, v, base, ok, lane);
}

// A row of V fp32 columns scanned in S slices with 16-byte loads (beam and sample scans): columns per slice, a multiple of 4 ...
static inline int slice_chunk(int V, int S) { return ((V + 3) / 4 + S - 1) / S * 4; }
// ... and whether the loads may be used: then every row starts 16-byte aligned and ld >= roundup4(V)
static inline int rows_vec4(const void* p, long long ld) { return (aligned16(p) && ld % 4 == 0) ? 1 : 0; }
