// Decoding constraints on the device (include/univl_hip.h: univl_decode_constrain): n-gram blocking, a minimum length and a suppress
// list as -inf stores into the score rows of one position, in ONE launch between the vocabulary classifier (or the log-softmax behind
// it) and the selection kernel.
//
//   grid ceil(R / 4), 256 threads = 4 waves, one wave per row.  A row's work is a few dozen loads and a handful of stores, so the launch
//   is bound by its own latency, not by any rate: what matters is that it is one launch with no dependence on the host.
//   The prefix update rides in the same kernel.  A wave copies its own row only (from the row src names, of the OTHER array), and it
//   reads the prefix it blocks on through `tok` below -- from prefix_in and last, never back from what it has just stored -- so no store
//   of this launch is read by this launch, within a wave or across waves, and nothing needs a fence.
//   Every store to x is the same word (-inf), so two lanes that ban the same column do not race on a value.
#include <math.h>
#include "common.h"
#include "univl_hip.h"

namespace {

constexpr int CN_WAVES = 4;

struct ConstrainArgs {
    float* x; long ld;
    int R, V, t, Tmax;
    const int32_t* prefix_in; int32_t* prefix_out; const int32_t* src; const int64_t* last;
    const uint8_t* done; int done_stride;
    int ngram, min_len, eos;
    const int32_t* eos_dev; const int32_t* params_dev; const int32_t* suppress; int n_suppress;
};

__global__ __launch_bounds__(64 * CN_WAVES) void decode_constrain_kernel(ConstrainArgs a) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * CN_WAVES + (threadIdx.x >> 6);
    if (row >= a.R) return;                                           // wave-uniform
    const int t = a.t;
    const bool update = a.last != nullptr && t > 0;
    // the row's prefix p[0 .. t): the parent's first t-1 tokens and the newest one, or the row of prefix_in as it stands
    const int32_t* p = a.prefix_in;
    int newest = 0;
    if (update) {
        int sr = a.src != nullptr ? a.src[row] : row;
        sr = sr < 0 ? 0 : (sr >= a.R ? a.R - 1 : sr);
        p += (long)sr * a.Tmax;
        newest = (int)a.last[row];
        int32_t* out = a.prefix_out + (long)row * a.Tmax;
        for (int j = lane; j < t - 1; j += 64) out[j] = p[j];
        if (lane == 0) out[t - 1] = newest;
    } else if (p != nullptr) {
        p += (long)row * a.Tmax;
    }
    if (a.done != nullptr && a.done[row / a.done_stride]) return;     // the row of x stays as it is
    auto tok = [&](int j) { return update && j == t - 1 ? newest : p[j]; };
    float* x = a.x + (long)row * a.ld;
    const int V = a.V;
    int n = a.params_dev != nullptr ? a.params_dev[0] : a.ngram;
    const int min_len = a.params_dev != nullptr ? a.params_dev[1] : a.min_len;
    n = n < 0 ? 0 : (n > UNIVL_NGRAM_BLOCK_MAX ? UNIVL_NGRAM_BLOCK_MAX : n);
    if (n >= 1 && p != nullptr) {
        const int s0 = t - n + 1;                                     // where the last n-1 tokens begin
        for (int j = lane; j < s0; j += 64) {
            bool same = true;
            for (int k = 0; k < n - 1; ++k) same = same && tok(j + k) == tok(s0 + k);
            const int v = tok(j + n - 1);
            if (same && v >= 0 && v < V) x[v] = -INFINITY;
        }
    }
    if (lane == 0) {
        const int eos = a.eos_dev != nullptr ? *a.eos_dev : a.eos;
        if (t < min_len && eos >= 0 && eos < V) x[eos] = -INFINITY;
    }
    for (int i = lane; i < a.n_suppress; i += 64) {
        const int v = a.suppress[i];
        if (v >= 0 && v < V) x[v] = -INFINITY;
    }
}

bool overlap(const void* a, const void* b, int64_t bytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + (uintptr_t)bytes && pb < pa + (uintptr_t)bytes;
}

}  // namespace

extern "C" int univl_decode_constrain_sizeof(void) { return (int)sizeof(UnivlDecodeConstrain); }

extern "C" int univl_decode_constrain(const UnivlDecodeConstrain* d, hipStream_t stream) {
    UNIVL_ON_STREAM_DEVICE(stream);
    UNIVL_CHECK_ARG(d != nullptr, UNIVL_EINVAL, "univl_decode_constrain: null descriptor");
    UNIVL_CHECK_ARG(d->R >= 1 && d->V >= 1 && d->V <= d->ld, UNIVL_EINVAL, "univl_decode_constrain: R=%d V=%d ld=%lld (R >= 1, 1 <= V <= ld)",
                    d->R, d->V, (long long)d->ld);
    UNIVL_CHECK_ARG(d->t >= 0 && d->t < d->Tmax, UNIVL_EINVAL, "univl_decode_constrain: position t=%d of Tmax=%d", d->t, d->Tmax);
    UNIVL_CHECK_ARG(d->ngram >= 0 && d->ngram <= UNIVL_NGRAM_BLOCK_MAX && d->min_len >= 0 && d->n_suppress >= 0, UNIVL_EINVAL,
                    "univl_decode_constrain: ngram=%d min_len=%d n_suppress=%d (0 <= ngram <= %d, min_len >= 0, n_suppress >= 0)", d->ngram,
                    d->min_len, d->n_suppress, UNIVL_NGRAM_BLOCK_MAX);
    UNIVL_CHECK_ARG(d->done == nullptr || d->done_stride >= 1, UNIVL_EINVAL, "univl_decode_constrain: done_stride=%d", d->done_stride);
    const bool update = d->last != nullptr && d->t > 0;
    const bool reads = d->t > 0 && (update || d->ngram > 0 || d->params_dev != nullptr);
    UNIVL_CHECK_ARG(d->x != nullptr && (!reads || d->prefix_in != nullptr) && (!update || d->prefix_out != nullptr) &&
                    (d->n_suppress == 0 || d->suppress != nullptr), UNIVL_EINVAL, "univl_decode_constrain: null pointer");
    UNIVL_CHECK_ARG(!(update && d->src != nullptr && overlap(d->prefix_in, d->prefix_out, (int64_t)d->R * d->Tmax * 4)), UNIVL_EINVAL,
                    "univl_decode_constrain: prefix_in and prefix_out overlap while src is given");
    ConstrainArgs a;
    a.x = d->x; a.ld = (long)d->ld; a.R = d->R; a.V = d->V; a.t = d->t; a.Tmax = d->Tmax;
    a.prefix_in = d->prefix_in; a.prefix_out = d->prefix_out; a.src = d->src; a.last = d->last;
    a.done = d->done; a.done_stride = d->done_stride;
    a.ngram = d->ngram; a.min_len = d->min_len; a.eos = d->eos;
    a.eos_dev = d->eos_dev; a.params_dev = d->params_dev; a.suppress = d->suppress; a.n_suppress = d->n_suppress;
    hipLaunchKernelGGL(decode_constrain_kernel, dim3((d->R + CN_WAVES - 1) / CN_WAVES), dim3(64 * CN_WAVES), 0, stream, a);
    UNIVL_LAUNCH_CHECK();
    return UNIVL_OK;
}
