/* libunivl_hip.so -- C ABI of the MI355X (gfx950) kernels behind the UniVL hot path.
 *
 * The reference (microsoft/UniVL) has NO native layer: its "operator API" is the Python class
 * modules/modeling.py::UniVL and all arithmetic is delegated to PyTorch ATen.  Each entry
 * point below therefore replaces an ATen op SEQUENCE at a cited call site of the reference; the Python host
 * (univl_amd/) mirrors the reference's module surface and calls these through ctypes.
 *
 * Contract (SURVEY.md section 8b "C-ABI"):
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller (PyTorch's caching
 *     allocator on the Python side).  The library never allocates, frees or synchronises on the hot path.
 *   - every call only ENQUEUES work on `stream` (a hipStream_t) and returns 0 on success, <0 for an argument error (UNIVL_E*), >0 for a hipError_t; univl_last_error() describes it.
 *   - the DEVICE is the one `stream` belongs to (hipStreamGetDevice), not the calling thread's current device: the
 *     reference's evaluation fan-out calls the model from one thread per GPU (util.py:21-60) and autograd's backward
 *     threads carry their own current device.  The null stream means the current device.
 *   - re-entrant; no global mutable state besides the thread-local error string, per-device "large LDS enabled" flags and the
 *     deterministic-mode switch below (with its per-device scratch ring -- the one thing the library allocates, and only when asked).
 *   - dtype: UNIVL_F32 (parity mode, exact-fp32 MFMA) or UNIVL_BF16 (production: bf16 operands, fp32
 *     accumulate, fp32 LayerNorm/softmax/residual stream).
 *   - RNG for dropout is (seed, offset) supplied by the caller; offsets distinguish call sites.  The effective
 *     seed is seed + *seed_dev when seed_dev (a device pointer) is given, so that a captured hipGraph draws a
 *     fresh mask on every replay (univl_bump_counter advances the device word inside the graph).
 */
#ifndef UNIVL_HIP_H
#define UNIVL_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

#define UNIVL_DT_F32 0
#define UNIVL_DT_BF16 1

const char* univl_last_error(void);
int univl_version(void);
/* sizeof of ABI struct #which (0 Gemm, 1 LayerNorm, 2 Attention, 3 EmbedText, 4 Pool, 5 Seg, 6 Adam, 7 VocabCE, 8 BeamStep, 9 SimTopk, 10 VocabScore) -- lets a
 * foreign-language binding verify its struct mirrors at load time */
int univl_struct_size(int which);
/* The same table, continued: 0 .. 10 as univl_struct_size, 11 SampleStep; -1 past the end.  univl_struct_size itself stays at the
 * eleven structs it has always listed -- bindings pin the -1 it returns for the first index past them -- and descriptors added from
 * here on are numbered in this table only. */
int univl_abi_sizeof(int which);
/* number of CUs / name of the current device, for host-side launch heuristics; returns 0 or hipError_t */
int univl_device_info(int* cu_count, char* name, int name_len);
/* univl_init(device): optional, idempotent.  Checks that `device` exists and is a gfx950 part (the only code object in the
 * library), returns 0 / UNIVL_EUNSUPPORTED / hipError_t.  Nothing needs to be initialised before the first call into the
 * library; a host that wants the failure at start-up instead of at the first launch calls this once per GPU
 * (where the reference calls torch.cuda.set_device, main_task_retrieval.py:121).  univl_destroy() releases what the
 * library opened lazily (the RCCL handle of univl_allreduce_bucket); device memory is never owned by the library. */
int univl_init(int device);
/* Clears n <= UNIVL_ZERO_MAX device buffers (16-byte aligned) with one launch; ptrs / bytes are HOST arrays read at call time. */
#define UNIVL_ZERO_MAX 16
int univl_zero_many(void* const* ptrs, const int64_t* bytes, int32_t n, hipStream_t stream);
/* n <= UNIVL_ZERO_MAX device-to-device copies (dst[i] <- src[i], bytes[i] each; non-overlapping) with one launch: the input
 * staging of UniVL.forward (modeling.py:192-202 hands over input_ids / token_type_ids / attention_mask / video / video_mask) and
 * the loss hand-off as ONE kernel node of the captured step instead of one memcpy node each.  16-byte aligned pairs move as
 * 16-byte words, others bytewise.  srcs / dsts / bytes are HOST arrays read at call time. */
int univl_copy_many(const void* const* srcs, void* const* dsts, const int64_t* bytes, int32_t n, hipStream_t stream);
int univl_destroy(void);
/* Deterministic mode.  By default every floating-point sum that several workgroups contribute to -- split-K slices, the column sums
 * behind LayerNorm / bias gradients, embedding and pair-concat scatter-adds, gradient-norm partials, loss accumulators -- is taken
 * with fp32 atomics, whose order (and therefore the last bits of the result) differs from run to run, as it does for the reference's
 * own CUDA kernels (index_add_ / embedding backward).  univl_set_deterministic(1) makes every later launch take these sums in a
 * FIXED order: no split-K, "last workgroup to arrive adds the partials in workgroup order" for column sums, gather-style kernels
 * ("the first source of a destination row sums all its sources in source order") for the scatters.  Two runs on the same inputs
 * are then bit-identical, at a cost of a few extra launches -- the parity tests run in this mode, production does not.  The call
 * allocates a scratch ring on the CURRENT device (UNIVL_DET_ARENA_MB, default 1024) and must therefore be made outside any stream
 * capture, once per device; plans / graphs built before a switch keep the mode they were built in.  Returns 0 or UNIVL_EINVAL. */
int univl_set_deterministic(int on);
int univl_get_deterministic(void);
/* Data-parallel gradient exchange for hosts that own an RCCL communicator themselves (the Python host goes through
 * torch.distributed's "nccl" backend = RCCL, main_task_retrieval.py:23,197-198, instead): in-place all-reduce of
 * buf[0..n) (dtype UNIVL_DT_F32 / UNIVL_DT_BF16) over `comm` (an ncclComm_t) on the side stream `side`,
 * op = average if `average` else sum.  Only enqueues.  RCCL is resolved at first use (the copy already loaded into
 * the process, else librccl.so); UNIVL_EUNSUPPORTED if it cannot be found, >0 = ncclResult_t + 1000. */
int univl_allreduce_bucket(void* buf, size_t n, int dtype, int average, void* comm, hipStream_t side);

/* ------------------------------------------------------------------------------------------------ GEMM
 * C[M,N] = epi( alpha * A_op[M,K] . B_op[N,K]^T ).   trans_x = 0: operand stored [rows][K] (row-major, ld);
 * trans_x = 1: operand stored [K][rows].  Replaces nn.Linear forward (module_bert.py:172-174,207,233,246 and
 * the Visual/Cross/Decoder copies), its autograd dgrad (trans_b=1) and wgrad (trans_a=trans_b=1), the tied
 * vocabulary classifier (module_bert.py:327-330), torch.matmul of the similarity (modeling.py:389) and torch.mm
 * of the MFM logits (modeling.py:285). */
#define UNIVL_GEMM_ACCUM 1        /* C32 (and dbias) += result                                             */
#define UNIVL_GEMM_GELU_FWD 2     /* aux <- pre-activation (T), result <- gelu(result)  (until_module.py:28) */
#define UNIVL_GEMM_GELU_BWD 4     /* result *= gelu'(aux)                                                  */
#define UNIVL_GEMM_ATOMIC 8       /* internal: split-K atomics                                             */
#define UNIVL_GEMM_DBIAS_ATOMIC 16 /* dbias accumulated with atomics (several row tiles share a bias)       */
#define UNIVL_GEMM_XCD_MAP 64      /* internal: XCD-aware workgroup -> tile map (always on since round 4) */
#define UNIVL_GEMM_PROBE_NOSTORE 128 /* internal, only in the -DUNIVL_TRACE measurement build (UNIVL_GEMM_PROBE=1 there): the epilogue computes but does not store; the product library never sets or tests it */
#define UNIVL_GEMM_PROBE_NT_B 256   /* internal, only in the -DUNIVL_TRACE measurement build (UNIVL_GEMM_NT_B=1 there): non-temporal LDS-DMA of the B operand */
#define UNIVL_GEMM_AUX_F32 512     /* aux holds the GELU pre-activation in fp32 (ldaux in floats) instead of the compute type: removes the one
                                    * non-operand rounding between FFN1 and its GELU' (A/B measurement of DESIGN.md section 2; costs 2 x the
                                    * bytes of that buffer both ways) */
#define UNIVL_GEMM_NT_OUT 32       /* fp32 output written with non-temporal stores: a weight gradient is read next by the optimizer, a whole backward later */
typedef struct UnivlGemm {
    int32_t dtype, trans_a, trans_b;
    int32_t M, N, K;
    const void* A; int64_t lda;
    const void* B; int64_t ldb;
    float* C32;            /* optional fp32 output                      */
    void* C16;             /* optional output in the compute type       */
    int64_t ldc;
    const float* bias;     /* optional [N]                              */
    const float* R;        /* optional fp32 residual [M,ldr]            */
    int64_t ldr;
    void* aux;             /* GELU pre-activation buffer (compute type) */
    int64_t ldaux;
    float* dbias;          /* optional, wgrad only: [M] sums of A_op rows over K */
    float alpha;
    int32_t flags;
    int32_t ksplit;        /* >1: split the contraction over gridDim.z, fp32 atomics into pre-zeroed C32 */
    int32_t tile;          /* 0 auto; 64 (64x64), 128 (128x128);
                            * 256 (256x256 on the 8-phase body, csrc/gemm256.h: bf16, M and N multiples of 256, K slices multiples of
                            *      128, not (T-major A, K-major B), no in-tile dbias -- else 128);
                            * 12864 / 64128 (128x64 / 64x128; bf16, K-major A, no sumsq / dbias, univl_gemm only -- else 128) */
    /* optional, no split-K: every wave stores the sum of squares of the FINAL values it wrote to
     *   sumsq[(m0 / sumsq_rows) * sumsq_stride + (((m0 % sumsq_rows) / tile) * tiles_x + tile_x) * waves + wave]
     * (sumsq_rows = 0: the whole output is one tensor).  Partial sums, no atomics: thousands of workgroups adding to one
     * address serialise in L2.  univl_sumsq_finish folds them into per-tensor sums.  Lets the weight-gradient GEMMs
     * produce the gradient norms clip_grad_norm_ (main_task_retrieval.py:347) and BertAdam's per-parameter clip
     * (optimization.py:135-136) need, instead of a separate 4 B/param pass.  sumsq_rows must be a multiple of 128.
     * At most rows x N / 1024 partial sums per tensor. */
    float* sumsq; int32_t sumsq_rows; int32_t sumsq_stride;
    int32_t stages;        /* LDS pipeline depth: 0 or 2 (double buffer, the only form since round 4; the field keeps the ABI layout) */
    int32_t waves;         /* waves per workgroup on the 64 / 128 tiles: 0 auto, 4, 8 (bf16, else 4) */
    /* Round 6, bf16 only -- operand PAIRS.  A bf16 operand carries 8 mantissa bits; x = hi + lo with hi = bf16(x), lo = bf16(x - hi)
     * carries 16.  A_lo / B_lo (optional, same layout and leading dimension as A / B) hold the lo halves; the product then walks the
     * contraction once per term in a FIXED order --  A.B,  A.B_lo (if B_lo),  A_lo.B (if A_lo)  -- into the same fp32 accumulators
     * (the lo.lo term is below fp32 resolution of the sum and is dropped).  ksplit divides that concatenated contraction.  A paired
     * product runs on the 64 x 64 tile whatever `tile` says (the only body that carries the term walk), needs K-major A and K a
     * multiple of 128, and is carried by univl_gemm, univl_gemm_rider, univl_gemm_ln and univl_attention_fwd_fused; univl_gemm_pair /
     * univl_gemm_group / univl_attention_bwd_fused return UNIVL_EUNSUPPORTED for it.  The plans pair the forward products'
     * operands up to 768 tokens, where the matrix pipe is idle (what it buys in gradient error).
     * C16_lo (optional): the epilogue also stores lo = bf16(result - bf16(result)) there (same ldc) -- the A_lo of the next product. */
    const void* A_lo; const void* B_lo; void* C16_lo;
} UnivlGemm;
int univl_gemm(const UnivlGemm* desc, hipStream_t stream);
/* n (1..UNIVL_GEMM_GROUP_MAX) independent problems with the same dtype / trans_a / trans_b in ONE launch: the four
 * weight-gradient GEMMs autograd runs for one transformer layer (the wgrad halves of the nn.Linear backward of
 * module_bert.py:172-174,207,233,246).  Members must not alias each other's outputs. */
#define UNIVL_GEMM_GROUP_MAX 4
int univl_gemm_group(const UnivlGemm* descs, int32_t n, hipStream_t stream);
/* The same with at most max_blocks workgroups (0: one per tile): the kernel then walks its tiles.  A launch that is not on
 * the critical path -- a layer's weight gradients -- can run beside the next layer's latency-bound kernels on another
 * stream without taking the compute units away from them. */
int univl_gemm_group_limited(const UnivlGemm* d, int n, int max_blocks, hipStream_t stream);
/* One launch for a dgrad product (dY . W: A K-major, B T-major) and the weight-gradient product that consumes the
 * same upstream gradient (dY^T . X: both T-major) -- the two halves of one nn.Linear backward (e.g. module_bert.py:233, 246): the
 * weight-gradient tiles fill the compute units the latency-bound dgrad leaves idle.  bf16, 64 x 64 tiles only (returns
 * UNIVL_EUNSUPPORTED otherwise -- callers fall back to univl_gemm + univl_gemm_group); dry_run != 0 validates without launching. */
int univl_gemm_pair(const UnivlGemm* dgrad, const UnivlGemm* wgrad, int32_t dry_run, hipStream_t stream);
/* Host-side evaluation of the kernels' workgroup -> tile maps (no device work; lets a CPU test prove they are bijections):
 * what 0: plain-grid map, in out[0..2] = hardware block index, out = the tile that block computes;
 * what 1: out[0] <- position of linear workgroup out[0] in the XCD-grouped tile list of nx tiles;
 * what 2: out[0..2] <- tile number out[0] of an nx x ny x nz problem (a grouped launch's member);
 * what 3: out[0..2] <- the tile local workgroup out[0] of one half of a pair / rider launch computes;
 * what 4: the rider launch of the 64 x 128 tile (round 5), whose update workgroups are spread through the grid in groups of 8: workgroup
 *         out[0] of nx + ny (nx tile slots, ny update workgroups, both multiples of 8) -> out[1] = 1 and out[0] = its update index, or
 *         out[1] = 0 and out[0] = its tile slot (congruent to the workgroup id modulo 8). */
int univl_gemm_tile_map(int32_t what, int32_t nx, int32_t ny, int32_t nz, int32_t gm, int32_t* out);

/* Host-side evaluation of the LDS maps of the 256 x 256 product body (csrc/gemm256.h; no device work -- lets a CPU test prove that the
 * LDS-DMA image and the fragment reads agree and are bank-conflict free):
 * what 0: out[0..1] <- (row, k) of the first of the 8 elements at lane-linear LDS piece idx (0..1023) of a half-tile image;
 * what 1: out[0..7] <- LDS byte offsets of the fragment reads of lane idx (0..63) for the 32-row block at arg (0, 32, 64, 96):
 *         K-major (trans 0) out[0..3] per 16-deep k step, out[4..7] = -1; T-major (trans 1) two transpose reads per k step. */
int univl_gemm256_layout(int32_t what, int32_t trans, int32_t idx, int32_t arg, int32_t* out);

/* ------------------------------------------------------------------------------------------ LayerNorm
 * TF-style LayerNorm (until_module.py:40-53: biased variance, eps inside the sqrt) fused with what surrounds it
 * in the reference:  out = dropout_post( LN( dropout_pre(x) + residual + pos[row % period] ) ).
 *   BertSelfOutput/BertOutput (module_bert.py:207-211,246-250): x = dense output, residual, p_pre.
 *   Visual/Cross embeddings  (module_visual.py:118-131, module_cross.py:123-138): pos (+type via residual), p_post.
 *   NormalizeVideo (modeling.py:88-92): x is float64 (x_f64 = 1), no residual/dropout. */
typedef struct UnivlLayerNorm {
    int32_t dtype;         /* type of out16 / dxd16                                                       */
    int32_t rows, N;       /* N in {768, 1024}                                                             */
    int32_t x_f64;         /* forward input is float64                                                     */
    const void* x;         /* fwd: [rows,N] fp32 (or f64)                                                  */
    const float* residual; /* fwd: optional [rows,N]                                                       */
    const float* pos;      /* fwd: optional [period,N] added to row (row % period)                         */
    int32_t pos_period;
    const float* gamma; const float* beta;
    float eps;
    float* y;              /* fwd out / bwd in: pre-LN sum [rows,N] (may alias x)                          */
    float* stats;          /* fwd out / bwd in: [rows,2] = mean, rstd                                      */
    float* out32;          /* fwd: optional fp32 output                                                    */
    void* out16;           /* fwd: optional output in compute type                                         */
    float p_pre, p_post;
    uint64_t seed, off_pre, off_post;
    const uint64_t* seed_dev;
    /* backward */
    const float* dout;     /* [rows,N] grad wrt out                                                        */
    float* dx32;           /* optional: grad wrt the pre-LN sum (= grad of residual / pos inputs)           */
    float* dxd32;          /* optional: grad wrt x (dropout_pre backward applied), fp32                    */
    void* dxd16;           /* optional: same in compute type (operand of the following dgrad/wgrad)        */
    float* dgamma; float* dbeta;   /* [N], accumulated (atomics; fixed order in deterministic mode)        */
    float* dbias;          /* optional [N]: column sums of the grad wrt x (bias grad of the producing GEMM) */
    float* dpos;           /* optional [period,N], accumulated (atomics; fixed order in deterministic mode)*/
    void* out16_lo;        /* fwd, optional, bf16: lo half of the output pair (UnivlGemm.A_lo of the products that read out16) */
} UnivlLayerNorm;
int univl_layernorm_fwd(const UnivlLayerNorm* d, hipStream_t stream);
int univl_layernorm_bwd(const UnivlLayerNorm* d, hipStream_t stream);

/* ------------------------------------------------------------------------------------------- attention
 * softmax(Q K^T / sqrt(d) + mask) -> dropout -> .V   (module_bert.py:181-197 and its three copies).  The additive
 * mask is built in-kernel from the {0,1} key mask exactly as module_bert.py:429-437 ((1-m)*-10000, added AFTER
 * the scaling) and, with `causal`, as module_decoder.py:389-396 (((1-answer_mask)+triu(1))>0)*-10000.
 * Head h of row r lives at  ptr + r*ld + h*64.  d is fixed to 64.  Forward saves the row log-sum-exp. */
typedef struct UnivlAttention {
    int32_t dtype;
    int32_t B, H, Sq, Sk;
    const void* q; int64_t ldq;
    const void* k; int64_t ldk;
    const void* v; int64_t ldv;
    const int64_t* key_mask;  /* optional [B,Sk], 1 = attend */
    int32_t causal;
    void* out; int64_t ldo;   /* [B*Sq, ldo] compute type */
    float* lse;               /* [B,H,Sq] */
    float p_drop; uint64_t seed, offset;
    const uint64_t* seed_dev;
    /* backward */
    const void* dout; int64_t lddo;
    void* dq; int64_t lddq;
    void* dk; int64_t lddk;
    void* dv; int64_t lddv;
    /* optional batch strides (elements) of k and v: 0 = Sk*ld (densely packed rows).  A key/value cache of capacity
     * Tmax >= Sk per sequence (incremental caption decoding, main_task_caption.py:434-470) passes Tmax*ld.  Rows >= Sk of a
     * sequence's slots are never read.  The strides cover READS only: univl_attention_bwd reads k and v at bsk / bsv and
     * writes dk and dv densely, batch row b at row b*Sk of [B*Sk, lddk] / [B*Sk, lddv] -- the gradient of the prefix, not a
     * cache-shaped buffer (tests/test_attention_edges_gpu.py pins both).
     * Bias semantics at the edges: a key that is masked AND (causal) ahead of the query carries ONE -10000, so a fully
     * masked batch row is softmax(raw scores) over all Sk real keys, causal or not; causal is key > q for any Sq, Sk. */
    int64_t bsk, bsv;
    void* out_lo;             /* fwd, optional, bf16: lo half of the output pair, [B*Sq, ldo] (UnivlGemm.A_lo of the output projection) */
} UnivlAttention;
int univl_attention_fwd(const UnivlAttention* d, hipStream_t stream);
int univl_attention_bwd(const UnivlAttention* d, hipStream_t stream);

/* univl_attention_bwd with the dgrad of the attention-output projection (dctx = dY . W_o: the dense of BertSelfOutput, module_bert.py:207,
 * differentiated) computed INSIDE the launch: every workgroup first multiplies the 64 x 64 block of dctx that belongs to its own (batch
 * row, head) -- sequences of at most 64 positions, head width 64 -- and runs the attention backward on it from LDS; dctx never goes
 * through global memory (at->dout is not written) and one launch leaves the backward chain.  dq / dk / dv are bit-identical to
 * univl_gemm(odgrad) + univl_attention_bwd(at).  owgrad (optional): the weight gradient of the same projection (dY^T . ctx), riding
 * as extra workgroups like in univl_gemm_pair.  bf16 only; UNIVL_EUNSUPPORTED where the launch does not carry the pair; dry_run != 0
 * validates without launching. */
int univl_attention_bwd_fused(const UnivlAttention* at, const UnivlGemm* odgrad, const UnivlGemm* owgrad, int32_t dry_run, hipStream_t stream);

/* univl_attention_fwd with the query / key / value projection (module_bert.py:172-174) computed INSIDE the launch: every workgroup
 * multiplies the 64 x 192 block of q | k | v that belongs to its (batch row, head), stores it to the qkv buffer (bit-identical to
 * univl_gemm(qkv)) and attends on it from LDS -- self-attention over at most 128 positions (65 .. 128: two workgroups per (batch row,
 * head), one per block of 64 queries, each multiplying the whole sequence's q | k | v), bf16; the projection may carry operand pairs (A_lo / B_lo).  adam / chunk_*: BertAdam chunks
 * riding in the launch like in univl_gemm_rider (NULL / 0: none).  UNIVL_EUNSUPPORTED where the launch does not carry the pair. */
int univl_attention_fwd_fused(const UnivlAttention* at, const UnivlGemm* qkv, const struct UnivlAdam* adam, int32_t chunk_begin,
                              int32_t chunk_count, int32_t max_blocks, int32_t dry_run, hipStream_t stream);

/* ------------------------------------------------------------------------------------- text embeddings
 * BertEmbeddings / DecoderEmbeddings (module_bert.py:132-146, module_decoder.py:309-320):
 * gather word + position (+ token type) -> LayerNorm -> dropout.  Backward scatter-adds into the tables. */
typedef struct UnivlEmbedText {
    int32_t dtype;
    int32_t B, S, N;
    const int64_t* ids; const int64_t* type_ids;   /* type_ids optional */
    const float* word; const float* pos; const float* type;   /* type optional */
    const float* gamma; const float* beta; float eps;
    float* y; float* stats; float* out32; void* out16;
    float p_post; uint64_t seed, off_post;
    const uint64_t* seed_dev;
    const float* dout;
    float* dword; float* dpos; float* dtype_emb; float* dgamma; float* dbeta;   /* dpos may be NULL when drows is given */
    /* optional [B*S, N]: store each token's word-table gradient row here INSTEAD of scatter-adding it into dword.  Under
     * data parallelism the dense table gradient (30522 x 768 fp32 = 94 MB, at most B*S non-zero rows) is then exchanged
     * as (ids, rows) and rebuilt by univl_embed_scatter on every rank. */
    float* drows;
    void* out16_lo;           /* fwd, optional, bf16: lo half of the output pair */
} UnivlEmbedText;
int univl_embed_text_fwd(const UnivlEmbedText* d, hipStream_t stream);
int univl_embed_text_bwd(const UnivlEmbedText* d, hipStream_t stream);
/* Sparse bookkeeping of the word-embedding gradient (retrieval configurations: the token gather is the table's only
 * gradient source, so at most B*W of its 30522 rows are non-zero).  list[0 .. meta[0]) holds the rows written since the
 * last clear; meta[1] != 0 means "treat every row as listed" (list overflow, or a dense writer).  univl_rows_zero clears
 * the listed rows (instead of a 94 MB memset), univl_rows_append records the rows of a backward (reset != 0 starts a new
 * list), univl_rows_sumsq adds the sum of squares of the listed rows (each row once) to *out (instead of streaming the
 * whole table for its gradient norm).  cap <= 8192.  `ever` (optional, [rows_total] bytes): sticky "this row has been written at
 * least once" flags for UnivlAdam.row_flags -- univl_rows_append sets the flag of every id it is given (all flags on overflow). */
int univl_rows_zero(float* table, int64_t rows_total, const int64_t* list, const int32_t* meta, hipStream_t stream);
int univl_rows_append(const int64_t* ids, int32_t n, int64_t* list, int32_t cap, int32_t* meta, int32_t reset, uint8_t* ever,
                      int64_t rows_total, hipStream_t stream);
int univl_rows_sumsq(const float* table, int64_t rows_total, const int64_t* list, const int32_t* meta, float* out, hipStream_t stream);
/* out[s, c] += sum of rows[r, c] over r = s, s + period, s + 2 period, ... < n_rows (ascending, fixed order): the gradient of a
 * [period, n] position table from per-token gradient rows (UnivlEmbedText.drows, UnivlLayerNorm.dx32) -- used instead of the fused
 * kernels' scatter-add (dpos) from 32 rows per position on, where B atomics per table element dominate those kernels. */
int univl_rows_gather_sum(const float* rows, int32_t n_rows, int32_t period, int32_t n, float* out, hipStream_t stream);
/* dword[ids[t]] += scale * rows[t] for t < n (fp32 atomics; rows [n, 768]): the second half of the sparse exchange */
int univl_embed_scatter(const int64_t* ids, const float* rows, int64_t n, float scale, float* dword, hipStream_t stream);

/* ------------------------------------------------------------------------- pooling / similarity / loss
 * _mean_pooling_for_similarity + F.normalize (modeling.py:327-339, 385-388): masked mean over tokens
 * (skip_first: position 0 excluded for text; zero-count guard), optional L2 normalisation (eps 1e-12). */
typedef struct UnivlPool {
    int32_t B, S, N;
    const float* x; int64_t ldx_row;   /* x[(b*S+s)*ldx_row + c] */
    const int64_t* mask;
    int32_t skip_first, normalize;
    float* mean;        /* [B,N] saved pre-normalisation mean */
    float* out;         /* [B,N] */
    const float* dout;  /* bwd: [B,N] */
    float* dx;          /* bwd: [B,S,N] */
    int32_t accumulate; /* bwd: dx += instead of dx = */
    /* bwd, optional: take the upstream gradient from the similarity matrix's instead of `dout` -- torch.matmul(text, video.t())
     * of modeling.py:389 backward folded in: dout[b, :] = gscale[0] * sum_k dsim[b, k] * other[k, :] (transpose = 0: this side
     * indexes the ROWS of dsim) or sum_k dsim[k, b] * other[k, :] (transpose = 1: the columns); `other` = the other modality's
     * pooled (normalised) [n_other, N] matrix, dsim rows ldsim floats apart, gscale a device scalar (NULL: 1). */
    const float* dsim; int64_t ldsim; const float* other; int32_t n_other; int32_t transpose; const float* gscale;
} UnivlPool;
int univl_pool_fwd(const UnivlPool* d, hipStream_t stream);
int univl_pool_bwd(const UnivlPool* d, hipStream_t stream);
/* The text and the video pooling of one similarity head in ONE launch each way (the two descriptors of modeling.py:327-339). */
int univl_pool_pair_fwd(const UnivlPool* a, const UnivlPool* b, hipStream_t stream);
int univl_pool_pair_bwd(const UnivlPool* a, const UnivlPool* b, hipStream_t stream);

/* MaxMarginRankingLoss (until_module.py:245-251): loss = mean(w * (relu(m + x - diag_col) + relu(m + x - diag_row))).
 * `sim` and `dsim` are [n, ld] row-major (ld >= n).  Writes the scalar loss and d loss / d x (for an upstream
 * gradient of 1). */
int univl_maxmargin_loss(const float* sim, int32_t n, int32_t ld, float margin, const float* weight, float* loss,
                         float* dsim, hipStream_t stream);
/* CrossEn (until_module.py:186-191): mean(-diag(log_softmax(x, -1))) and its gradient. */
int univl_crossen_loss(const float* sim, int32_t n, int32_t ld, float* loss, float* dsim, hipStream_t stream);
/* MILNCELoss (until_module.py:201-221) for batch_size x n_pair blocks; n = batch_size*n_pair. */
int univl_milnce_loss(const float* sim, int32_t batch_size, int32_t n_pair, int32_t ld, float* loss, float* dsim,
                      hipStream_t stream);
/* Retrieval metrics (metrics.py:8-20): for every row i of the [n, ld] similarity matrix, gt[i] = #{j : x[i][j] > x[i][i]}
 * and eq[i] = #{j : x[i][j] == x[i][i]} (>= 1).  The rank positions `ind` of compute_metrics are range(gt, gt + eq)
 * per row: R@k / median rank follow on the host from 2n integers instead of an n x n sort. */
int univl_rank_counts(const float* sim, int32_t n, int64_t ld, int32_t* gt, int32_t* eq, hipStream_t stream);
/* x[0..n) *= s[0] with s on the device (applies loss.backward()'s upstream gradient without a host sync) */
int univl_scale_by_device_scalar(float* x, int64_t n, const float* s, hipStream_t stream);

/* --------------------------------------------------------------------- cross encoder / classifier helpers
 * pair_concat: out[p, :, :] = cat(seq[tidx[p]], vis[vidx[p]]) and out_mask likewise -- torch.cat of
 * UniVL._get_cross_output (modeling.py:315-325) for an explicit list of (text row, video row) pairs (the repeat/view
 * expansion of _cross_similarity modeling.py:352-366, or tidx = vidx = arange for the caption / pretrain path).
 * Backward scatter-adds d out into dseq / dvis (fp32 atomics; callers zero or pre-fill them). */
int univl_pair_concat_fwd(const float* seq, const float* vis, const int64_t* amask, const int64_t* vmask,
                          const int32_t* tidx, const int32_t* vidx, int32_t P, int32_t W, int32_t F, float* out,
                          int64_t* out_mask, hipStream_t stream);
int univl_pair_concat_bwd(const float* dout, const int32_t* tidx, const int32_t* vidx, int32_t P, int32_t W, int32_t F,
                          float* dseq, float* dvis, hipStream_t stream);
/* CrossEmbeddings (module_cross.py:123-138): table[s] = position[s] + token_type[s >= W] for s < S = W + F; the
 * LayerNorm kernel then adds it with period S.  Backward accumulates into dpos / dtype with atomics. */
int univl_postype_fwd(const float* pos, const float* type, int32_t W, int32_t S, float* out, hipStream_t stream);
int univl_postype_bwd(const float* dtable, int32_t W, int32_t S, float* dpos, float* dtype, hipStream_t stream);
/* nn.Tanh of CrossPooler (module_cross.py:281-287) */
int univl_tanh_fwd(const float* x, float* y, int64_t n, hipStream_t stream);
int univl_tanh_bwd(int32_t dtype, const float* dy, const float* y, void* dx, int64_t n, hipStream_t stream);   /* dx in compute type */
/* du (compute type) = dg (fp32) * gelu'(u): BertPredictionHeadTransform backward (module_bert.py:299-311) */
int univl_gelu_bwd(int32_t dtype, const float* dg, const void* u, void* du, int64_t n, hipStream_t stream);
/* similarity_dense = nn.Linear(768, 1) on the pooled cross output (modeling.py:167,371) and its backward
 * (dx written, dw/db accumulated with atomics) */
/* out[c] += sum_r x[r, c] over a [rows, ld] matrix in the compute type (atomics) */
int univl_colsum(int32_t dtype, const void* x, int64_t ld, int32_t rows, int32_t n, float* out, hipStream_t stream);
/* dst[r, 0:copy_bytes) = src[idx[r], 0:copy_bytes) for r < rows; rows are row_stride bytes apart in both buffers, all
 * byte counts multiples of 16 (beam re-ordering of the decoder's key/value cache: Beam.get_current_origin, beam.py:54) */
int univl_gather_rows(const void* src, void* dst, const int32_t* idx, int32_t rows, int64_t row_stride, int64_t copy_bytes,
                      hipStream_t stream);
/* x[r, 0:n) <- log_softmax(x[r, 0:n)) in place, fp32 rows ld apart (torch.nn.functional.log_softmax of
 * main_task_caption.py:454 over the vocabulary) */
int univl_log_softmax_rows(float* x, int32_t rows, int32_t n, int64_t ld, hipStream_t stream);
/* ---------------------------------------------------------------------------------- caption beam search
 * Beam.advance (modules/beam.py:63-87) for ALL instances of a batch at one position, entirely in device memory: two launches, no
 * host involvement, capturable.  Per instance i that is not done:
 *   candidate(b, v) = lp[i * n_bm + b, v] + scores[i, b]   (one fp32 addition; at the first step only b = 0 counts and nothing is
 *                     added, beam.py:69), v < V -- columns V .. ld-1 of lp are padding and are never candidates;
 *   the n_bm largest candidates, sorted descending.  TIE RULE: candidates of equal fp32 value are ordered by LOWER flat index
 *   b * V + v first (torch.topk leaves this open; here it is part of the contract).  Behaviour on NaN values: unspecified;
 *   parent = flat / V, token = flat % V;  scores[i, :] <- the kept values, tokens[i * n_bm + k] <- token (int64: the ids the next
 *   position's univl_embed_text_fwd reads), src[i * n_bm + k] <- i * n_bm + parent (int32: the row index univl_gather_rows reads),
 *   row t of the three history arrays [Tmax, n_inst, n_bm] <- parent / token / kept value;
 *   length[i] += 1;  done[i] <- 1 if the TOP beam's token == eos (beam.py:84).
 * An instance whose done[i] != 0 is FROZEN: scores, tokens, length and done stay as they are, src and the history's parents are
 * the identity, and the history's tokens / scores repeat the state.
 * Range: 1 <= n_bm <= UNIVL_BEAM_MAX, n_bm <= V <= ld, any n_inst >= 1, 0 <= t < Tmax; otherwise UNIVL_EINVAL. */
#define UNIVL_BEAM_MAX 8
#define UNIVL_BEAM_SLICES 8          /* most column slices a row is scanned in (sizes the workspace) */
typedef struct {
    const float* lp; int64_t ld;     /* [n_inst * n_bm, ld] fp32 log-probabilities (what univl_log_softmax_rows leaves)         */
    int32_t n_inst, n_bm, V;
    int32_t first_step;              /* != 0: only beam 0's row is read and no score is added                                     */
    int32_t eos;                     /* token that ends an instance when its top beam emits it (-1: none)                         */
    const int32_t* eos_dev;          /* optional device word read INSTEAD of eos: a captured hipGraph serves calls with different */
                                     /* end tokens (the pattern of seed_dev above); NULL: eos                                     */
    int32_t t, Tmax;                 /* history row written by this call, rows of the history arrays                              */
    float* scores;                   /* [n_inst, n_bm]   read and written                                                         */
    uint8_t* done;                   /* [n_inst]         read and written                                                         */
    int32_t* length;                 /* [n_inst]         read and written                                                         */
    int64_t* tokens;                 /* [n_inst * n_bm]  written (read for frozen instances)                                      */
    int32_t* src;                    /* [n_inst * n_bm]  written                                                                  */
    int32_t* hist_parents; int32_t* hist_tokens; float* hist_scores;     /* [Tmax, n_inst, n_bm] each; row t written             */
    void* ws; int64_t ws_bytes;      /* 16-byte aligned scratch of >= n_inst * n_bm * UNIVL_BEAM_SLICES * n_bm * 8 bytes          */
} UnivlBeamStep;
int univl_beam_step(const UnivlBeamStep* d, hipStream_t stream);
/* Diverse Beam Search (Vijayakumar et al.; elsewhere `num_beam_groups` + `diversity_penalty`): the n_bm beams of an instance are
 * n_groups = G groups of width k' = n_bm / G, and a group is penalised for the tokens that EARLIER groups chose at the same position
 * (Hamming diversity).  Two launches, no host involvement, capturable, the workspace of univl_beam_step.
 * LAYOUT: done and length are [n_inst * G], one entry per (instance, group); group g of instance i owns beams b in [g k', (g+1) k'),
 * i.e. rows i * n_bm + b.  The history arrays [Tmax, n_inst, n_bm] are, byte for byte, [Tmax, n_inst * G, k'], and the parents written
 * into them are LOCAL to the group: to univl_beam_backtrack, univl_beam_captions, univl_gather_rows and univl_decode_constrain
 * (done_stride = k') the call is an ordinary search on n_inst * G pseudo-instances of width k'.
 * Per instance i the groups g = 0 .. G-1 are handled IN ORDER.  A group with done[i G + g] != 0 is FROZEN exactly as a frozen instance
 * of univl_beam_step (state untouched, src and the history's parents the identity, the history's tokens / scores repeat the state) and
 * contributes NO tokens to the penalty of later groups.  A live group:
 *   value(b, v)  = lp[i * n_bm + b, v] + scores[i, b]   (one fp32 addition; at the first step only the group's first beam counts and
 *                  nothing is added), v < V;
 *   c(v)         = the number of beams of EARLIER LIVE groups of instance i whose token chosen at this position is v;
 *   ranked(b, v) = value - p, p = lambda * (float)c(v): the product rounded to fp32 once, the subtraction rounded separately (no fma
 *                  across them); c = 0 subtracts +0;
 *   the k' candidates with the largest `ranked` (TIE RULE of univl_beam_step: equal fp32 values by LOWER flat index b * V + v first),
 *   then RE-SORTED by their unpenalised value, descending, same tie rule.  scores / the history's scores get the UNPENALISED value:
 *   the penalty orders the selection and does not accumulate, so scores stay the model's log-probabilities, beam 0 of a group is its
 *   best, and hypothesis scores are comparable across groups.  tokens, src (i * n_bm + parent) and the history row as univl_beam_step
 *   writes them;  length[i G + g] += 1;  done[i G + g] <- 1 if the group's TOP beam's token == eos.
 * lambda = *diversity_dev when that optional device word is given (the pattern of eos_dev: one capture serves every penalty; a
 * negative or non-finite word there is the caller's error, indices stay in range), else `diversity`.
 * IDENTITIES: n_groups == 1 is univl_beam_step bit for bit; diversity == 0 with any G is univl_beam_step called with
 * (n_inst * G, k') on the same buffers, bit for bit.  NaN values: unspecified, every index written stays in range.
 * Range: that of univl_beam_step, and 1 <= n_groups <= n_bm, n_bm % n_groups == 0, diversity finite and >= 0 (unless diversity_dev);
 * otherwise UNIVL_EINVAL and nothing is launched.  The struct is in neither numbered size table: univl_beam_group_step_sizeof states
 * its size. */
typedef struct {
    const float* lp; int64_t ld;     /* the fields of UnivlBeamStep, in its order ...                                             */
    int32_t n_inst, n_bm, V;
    int32_t first_step;              /* != 0: only the first beam's row of every group is read and no score is added              */
    int32_t eos;
    const int32_t* eos_dev;
    int32_t t, Tmax;
    float* scores;                   /* [n_inst, n_bm]       read and written                                                     */
    uint8_t* done;                   /* [n_inst * n_groups]  read and written                                                     */
    int32_t* length;                 /* [n_inst * n_groups]  read and written                                                     */
    int64_t* tokens;
    int32_t* src;
    int32_t* hist_parents; int32_t* hist_tokens; float* hist_scores;
    void* ws; int64_t ws_bytes;      /* as UnivlBeamStep.ws                                                                       */
    int32_t n_groups;                /* ... then G                                                                                */
    float diversity;                 /* lambda                                                                                    */
    const float* diversity_dev;      /* optional device word read INSTEAD of diversity; NULL: diversity                           */
} UnivlBeamGroupStep;
int univl_beam_group_step_sizeof(void);
int univl_beam_group_step(const UnivlBeamGroupStep* d, hipStream_t stream);
/* Beam search with a POOL OF FINISHED HYPOTHESES, a length penalty and an early-stopping switch (elsewhere `length_penalty`,
 * `early_stopping`).  Two launches per position, no host involvement, capturable, the workspace of univl_beam_step; one more launch
 * (univl_beam_pool_finish) after the last position.  Per instance i that is not done, at position t:
 *   CANDIDATES  candidate(b, v) = lp[i * n_bm + b, v] + scores[i, b], exactly as univl_beam_step forms it (one fp32 addition; at the
 *               first step only b = 0 counts and nothing is added), ordered by larger value first, then LOWER flat index b * V + v.
 *               A candidate whose value is -inf is not a candidate (a minimum length of univl_decode_constrain masks the end column
 *               that way); NaN values: unspecified, every index written stays in range.
 *   LIVE BEAMS  the first n_bm candidates with v != eos, in that order: scores, tokens, src and history row t are written exactly as
 *               univl_beam_step writes them.  A live beam never holds the end token.  The caller's condition: n_bm finite non-end
 *               columns per live row.
 *   FINISHING   every candidate with v == eos whose rank among ALL candidates (the number of candidates in front of it) is < n_bm
 *               is offered to the pool, in candidate order, as the entry
 *                 raw = the candidate's value, len = t + 1 (the end token counts), key = raw * w[len] (one fp32 multiplication),
 *                 end_t = t, beam = b, finished = 1;
 *               its tokens are the walk-back from history row end_t - 1 at `beam`: end_t tokens, the empty caption at t = 0.
 *   w           a device table of Tmax + 2 floats that the HOST fills: w[L] = (float)pow((double)L, -alpha), w[0] = 1.  There is no
 *               powf on the device, so a host reference reproduces every key bit for bit.
 *   POOL ORDER  larger key first, then smaller end_t, then smaller beam.  The pool holds at most n_bm entries per instance: a new entry
 *               is appended while there is room (slot pool_count[i]); otherwise it replaces, in that entry's slot, the LAST entry in
 *               pool order if it stands in front of it, and is dropped if it does not.  Slots are therefore in arrival order, not sorted.
 *   AFTER THE OFFERS  length[i] += 1;  done[i] <- 1 when the pool holds n_bm entries AND (params[0] != 0 [early_stopping] OR
 *               scores[i, 0] * w[Lmax] <= the key of the last pool entry), with scores[i, 0] the NEW best live score and
 *               Lmax = params[1] clamped to [0, Tmax + 1], the call's max_len: for alpha >= 0 and log-probabilities <= 0 that
 *               product is the best key a live beam can still reach.
 * Done instances and idle slots are FROZEN exactly as univl_beam_step freezes them; their pool is untouched too.
 * IDENTITY: with no end token (eos < 0 or >= V) the step is univl_beam_step bit for bit and the pool is not written.
 * univl_beam_pool_finish(d, n_best, ...) reads the same descriptor (lp, ws, t, tokens and src are not looked at): for every instance
 * that is NOT done the live beams b = 0 .. n_bm-1 are offered in order (raw = scores[i, b], len = length[i], key = raw * w[len],
 * end_t = length[i], beam = b, finished = 0) -- in the kernel's own memory, the pool arrays are only read -- then the pool is sorted in
 * pool order and its first n_best entries are written out: hyp [n_inst, n_best, Tmax] int32 (the walk-back, every parent clamped into
 * [0, n_bm) as univl_beam_backtrack does; for a finished entry FOLLOWED BY THE END TOKEN at index end_t, so that the row holds `len`
 * tokens as a plain search's row holds the end token its top beam emitted; then -1), hyp_raw, hyp_key, hyp_len (`len`) and the
 * finished byte, [n_inst, n_best] each.  A slot with fewer pool entries than n_best is an idle one: -1 tokens, -inf, -inf, length 0,
 * finished 0.
 * Range: that of univl_beam_step (the finish: 1 <= n_best <= n_bm <= UNIVL_BEAM_MAX, Tmax >= 1), w, params and every pool array
 * non-NULL; otherwise UNIVL_EINVAL and nothing is launched.  The struct is in neither numbered size table:
 * univl_beam_pool_step_sizeof states its size. */
typedef struct {
    const float* lp; int64_t ld;     /* the fields of UnivlBeamStep, in its order ...                                             */
    int32_t n_inst, n_bm, V;
    int32_t first_step;
    int32_t eos;
    const int32_t* eos_dev;
    int32_t t, Tmax;
    float* scores;
    uint8_t* done;
    int32_t* length;
    int64_t* tokens;
    int32_t* src;
    int32_t* hist_parents; int32_t* hist_tokens; float* hist_scores;
    void* ws; int64_t ws_bytes;      /* as UnivlBeamStep.ws                                                                       */
    const float* w;                  /* ... then [Tmax + 2] device floats, the length weights (host-filled)                       */
    const int32_t* params;           /* int32 [2] device words {early_stopping, Lmax}: one capture serves every mode and max_len   */
    float* pool_key; float* pool_raw;                          /* [n_inst, n_bm] each, read and written                           */
    int32_t* pool_end_t; int32_t* pool_beam;                   /* [n_inst, n_bm]                                                  */
    uint8_t* pool_finished;                                    /* [n_inst, n_bm]                                                  */
    int32_t* pool_count;                                       /* [n_inst] entries held, 0 before position 0                      */
} UnivlBeamPoolStep;
int univl_beam_pool_step_sizeof(void);
int univl_beam_pool_step(const UnivlBeamPoolStep* d, hipStream_t stream);
int univl_beam_pool_finish(const UnivlBeamPoolStep* d, int32_t n_best, int32_t* hyp, float* hyp_raw, float* hyp_key, int32_t* hyp_len,
                           uint8_t* hyp_finished, hipStream_t stream);
/* Beam.get_hypothesis (beam.py:108-116) for the n_best best beams of every instance (beams are sorted after univl_beam_step, so
 * beam k is the k-th best): hyp[i, k, 0 .. length[i]) <- the tokens found by walking the history back from (row length[i] - 1,
 * beam k) through the parents, the rest of hyp[i, k, :] (Tmax entries) <- -1;  hyp_scores[i, k] <- scores[i, k].
 * 1 <= n_best <= n_bm <= UNIVL_BEAM_MAX, otherwise UNIVL_EINVAL. */
int univl_beam_backtrack(const int32_t* hist_parents, const int32_t* hist_tokens, const float* scores, const int32_t* length,
                         int32_t n_inst, int32_t n_bm, int32_t n_best, int32_t Tmax, int32_t* hyp, float* hyp_scores,
                         hipStream_t stream);
/* The caption cut of main_task_caption.py:555-560 (first "[SEP]", then first "[PAD]") on the rows univl_beam_backtrack writes:
 * for row r = i * n_best + k of hyp [n_inst * n_best, Tmax], with len = length[i] clamped to [0, Tmax],
 *   cap_len[r] <- the smallest j < len with hyp[r, j] == eos or hyp[r, j] == pad, else len (the reference's two successive cuts);
 *   cap_tokens[r, 0 .. cap_len[r]) <- hyp[r, 0 .. cap_len[r]), the rest of cap_tokens[r, :] (Tmax entries) <- -1.
 * eos / pad: a negative id means "none".  eos_dev: optional device word read INSTEAD of eos (as UnivlBeamStep.eos_dev; NULL: eos).
 * cap_tokens MAY ALIAS hyp (the cut in place); otherwise the buffers must not overlap.  One launch, capturable.
 * 1 <= n_best <= UNIVL_BEAM_MAX, n_inst >= 1, Tmax >= 1, otherwise UNIVL_EINVAL. */
int univl_beam_captions(const int32_t* hyp, const int32_t* length, int32_t n_inst, int32_t n_best, int32_t Tmax, int32_t eos, int32_t pad,
                        const int32_t* eos_dev, int32_t* cap_tokens, int32_t* cap_len, hipStream_t stream);
/* ---------------------------------------------------------------------------------------- caption sampling
 * One position of ancestral sampling (top-k, temperature, top-p) for R independent rows, entirely in device memory: two launches, no
 * host involvement, capturable.  It reads the RAW logits x [R, ld] fp32 that the vocabulary classifier leaves -- no
 * univl_log_softmax_rows in front of it; only columns < V are candidates, columns V .. ld-1 are padding and never are.
 * Per row r with done[r] == 0 at position t:
 *   1. TOP-K: the k largest x[r, v], descending, x_0 >= ... >= x_{k-1} at columns col_j.  TIE RULE (the one univl_beam_step,
 *      univl_sim_topk and univl_vocab_score fix): equal fp32 values are ordered by LOWER column first.
 *   2. WEIGHTS: w_j = expf((x_j - x_0) * inv_T), inv_T = 1 / temperature computed by the host in fp32; the subtraction and the
 *      multiplication are two separately rounded fp32 operations (no fma across them).
 *   3. CUMULATIVE SUMS: c_0 = w_0, c_j = c_{j-1} + w_j, ONE left-to-right fp32 chain.
 *   4. NUCLEUS: m = the smallest count with c_{m-1} >= top_p * c_{k-1} (one fp32 product); top_p >= 1 means m = k exactly.
 *   5. DRAW: r32 = mix32((seed * 0x9E3779B97F4A7C15) ^ (t * 0xD1B54A32D192ED03 + r)) -- the generator and keying of the dropout masks
 *      (offset t, index r; 64-bit wrap-around arithmetic, mix32 = the murmur3 finaliser's low word), u = (r32 >> 8) * 2^-24,
 *      tau = u * c_{m-1} (fp32), j* = the first j < m with c_j > tau.
 *   6. OUTPUTS: tokens_out[r, t] = ids[r] = col_{j*};
 *      tok_logprob[r, t] = (x_{j*} - max) - log(sum_v exp(x_v - max)), max and the sum over all V columns: the model's own
 *      log-probability at temperature 1, formed as written (an fp32 difference, then the logarithm subtracted), never as a difference
 *      of two numbers of the size of the log-sum-exp;   q_logprob[r, t] = log(w_{j*} / c_{m-1}), the proposal's log-probability;
 *      seq_logprob[r] += tok_logprob, seq_q_logprob[r] += q_logprob (one fp32 addition each, so over positions each is the same
 *      left-to-right fp32 sum a host forms from the [R, Tmax] arrays);  length[r] += 1;  done[r] <- 1 if col_{j*} == eos.
 * A row with done[r] != 0 is FROZEN: nothing of it is written and ids[r] stays.  done is per ROW here.
 * The two logarithms of step 6 are evaluated in fp64 and rounded to fp32 once; the sum of exponentials (fp32 terms) is carried in
 * fp64.  Behaviour on NaN logits: unspecified, but every index written stays in range.
 * REPRODUCIBILITY: every reduction has a fixed order and there are no atomics; a row's outputs are a pure function of its V logits,
 * k, inv_T, top_p, seed, t and r -- not of R, of other rows, of deterministic mode or of how the row was cut into column slices
 * (the slice count depends on V alone).
 * inv_T / top_p / seed / eos may each come from DEVICE words instead (sampling_dev, seed_dev, eos_dev), so that one captured hipGraph
 * serves every temperature, nucleus, seed and end token; the library cannot range-check device words, that is then the caller's.
 * Range: R >= 1, 1 <= k <= min(UNIVL_SAMPLE_KMAX, V), V <= ld, 0 <= t < Tmax, and without sampling_dev inv_T finite and > 0 and
 * top_p > 0; otherwise, for a NULL pointer (the optional ones apart) or a short workspace, UNIVL_EINVAL and nothing is launched. */
#define UNIVL_SAMPLE_KMAX 64
#define UNIVL_SAMPLE_SLICES 8        /* most column slices a row is scanned in (sizes the workspace) */
typedef struct UnivlSampleStep {
    const float* x; int64_t ld;      /* [R, ld] fp32 raw logits                                                                   */
    int32_t R, V, k;
    int32_t t, Tmax;                 /* column of the [R, Tmax] outputs written by this call; the offset of the draw              */
    int32_t eos;                     /* token that ends a row (-1: none)                                                          */
    float inv_T, top_p;
    uint64_t seed;
    const float* sampling_dev;       /* optional device {inv_T, top_p} read INSTEAD of the two fields                             */
    const uint64_t* seed_dev;        /* optional device word read INSTEAD of seed                                                 */
    const int32_t* eos_dev;          /* optional device word read INSTEAD of eos (as UnivlBeamStep.eos_dev)                       */
    uint8_t* done;                   /* [R]        read and written                                                               */
    int32_t* length;                 /* [R]        read and written                                                               */
    int64_t* ids;                    /* [R]        written: the ids the next position's univl_embed_text_fwd reads                */
    int32_t* tokens_out; float* tok_logprob; float* q_logprob;       /* [R, Tmax] each; column t written                         */
    float* seq_logprob; float* seq_q_logprob;                         /* [R] each, read and written                               */
    int32_t* topk_idx; float* topk_val;                               /* optional [R, k] each: the list of step 1 (written)      */
    void* ws; int64_t ws_bytes;      /* 16-byte aligned scratch of >= R * UNIVL_SAMPLE_SLICES * (8 * k + 16) bytes                */
} UnivlSampleStep;
int univl_sample_step(const UnivlSampleStep* d, hipStream_t stream);
/* ---------------------------------------------------------------------------------------- decoding constraints
 * No repeated n-gram, a minimum length and a list of ids that are never emitted, applied to the score rows x [R, ld] fp32 of ONE
 * position IN PLACE, entirely in device memory: one launch, no host involvement, no atomics, no workspace, capturable.  It goes
 * between the launches that exist: behind univl_log_softmax_rows and in front of univl_beam_step (rows of log-probabilities), or
 * behind the vocabulary classifier and in front of univl_sample_step (rows of raw logits).  One wave handles one row, its lanes
 * stride over the prefix positions.  Every edit is x[r, v] = -inf by a plain vector store, so edits commute and there is no
 * arithmetic to round; only columns v < V are ever written, columns V .. ld-1 are padding and stay bit-identical.
 * PREFIX: p[0 .. t) are the tokens row r has emitted at positions 0 .. t-1 (the begin token is not among them), kept as rows of
 * [R, Tmax] int32 arrays.  With last != NULL and t > 0 the launch first brings them up to date from the beam state
 *   prefix_out[r, 0 .. t-1) = prefix_in[src[r], 0 .. t-1),   prefix_out[r, t-1] = (int32) last[r]
 * (src: the row each beam continues from, what univl_beam_step writes and univl_gather_rows reads; NULL: the identity.  last: the
 * tokens array of univl_beam_step.  A src entry outside [0, R) is clamped to that range, nothing is read out of it), and p is that
 * row of prefix_out; the two arrays are used with alternating roles from position to position and must not overlap unless src ==
 * NULL.  With last == NULL nothing is written to a prefix, prefix_out may be NULL and prefix_in must already hold t tokens per row:
 * the tokens_out array of univl_sample_step is that array.
 * A row with done[r / done_stride] != 0 keeps its row of x untouched; its prefix is still brought up to date, so that the buffers
 * stay defined.  done_stride: n_bm for beams (done is per instance), 1 for the sampler (per row); done may be NULL (no row is done).
 * Per live row, with n = ngram:
 *   1. N-GRAM BLOCKING (n >= 1): for every j in [0, t-n+1) with p[j .. j+n-1) == p[t-n+1 .. t), x[r, p[j+n-1]] = -inf: a token that
 *      would complete an n-gram the row already holds.  n == 1: every prefix token.  t < n-1: nothing.
 *   2. MINIMUM LENGTH: if t < min_len and eos >= 0, x[r, eos] = -inf.
 *   3. SUPPRESS LIST: x[r, v] = -inf for every v in suppress[0 .. n_suppress); duplicates are allowed.
 * Ids outside [0, V) -- in a prefix, as eos, in the list -- are skipped, never written through.
 * eos_dev: optional device word read INSTEAD of eos (as UnivlBeamStep.eos_dev).  params_dev: optional device words {ngram, min_len}
 * read INSTEAD of the two fields, so that one captured hipGraph serves every setting of them (the pattern and the caveat of
 * UnivlSampleStep.sampling_dev: the library cannot range-check device words, the caller does; an order outside
 * [0, UNIVL_NGRAM_BLOCK_MAX] is clamped into it).
 * The kernel does NOT check that a finite candidate remains: at least n_bm (univl_beam_step) or k (univl_sample_step) finite columns
 * per live row are the caller's responsibility; otherwise the selection kernels' ordering of -inf applies and is meaningless.
 * Range: R >= 1, 1 <= V <= ld, 0 <= t < Tmax, 0 <= ngram <= UNIVL_NGRAM_BLOCK_MAX, min_len >= 0, n_suppress >= 0, done_stride >= 1
 * with done; x, prefix_in whenever a prefix is read (t > 0 and last, ngram or params_dev given), prefix_out whenever one is written
 * (t > 0 and last given), suppress with n_suppress > 0 must not be NULL; prefix_in and prefix_out must not overlap while src is
 * given; otherwise UNIVL_EINVAL and nothing is launched.  The struct is in neither numbered size table:
 * univl_decode_constrain_sizeof states its size. */
#define UNIVL_NGRAM_BLOCK_MAX 4
typedef struct UnivlDecodeConstrain {
    float* x; int64_t ld;            /* [R, ld] fp32 score rows, edited in place                                                  */
    int32_t R, V;
    int32_t t, Tmax;                 /* the position whose token is about to be chosen; columns of the prefix arrays              */
    const int32_t* prefix_in;        /* [R, Tmax] int32                                                                           */
    int32_t* prefix_out;             /* [R, Tmax] int32, columns 0 .. t-1 written when last is given                              */
    const int32_t* src;              /* optional [R]: the row of prefix_in each row continues from (NULL: the identity)           */
    const int64_t* last;             /* optional [R]: the token each row emitted at position t-1 (NULL: prefix_in is up to date)  */
    const uint8_t* done;             /* optional [ceil(R / done_stride)]                                                          */
    int32_t done_stride;
    int32_t ngram;                   /* 0: off; 1 .. UNIVL_NGRAM_BLOCK_MAX: the blocked order                                     */
    int32_t min_len;                 /* 0: off                                                                                    */
    int32_t eos;                     /* the end token of the minimum length (negative: none)                                      */
    const int32_t* eos_dev;          /* optional device word read INSTEAD of eos                                                  */
    const int32_t* params_dev;       /* optional device {ngram, min_len} read INSTEAD of the two fields                           */
    const int32_t* suppress;         /* [n_suppress] int32 ids on the device                                                      */
    int32_t n_suppress, reserved;    /* reserved: 0                                                                               */
} UnivlDecodeConstrain;
int univl_decode_constrain_sizeof(void);
int univl_decode_constrain(const UnivlDecodeConstrain* d, hipStream_t stream);
/* ---------------------------------------------------------------------------------------- caption metrics
 * N-gram overlap statistics of token rows, per item, in one launch with no host involvement (capturable): the integers BLEU is made
 * of, the longest common subsequences and ROUGE_L, and, given document-frequency tables, CIDEr.  An ITEM is one hypothesis row and a
 * list of reference rows of the same table sym [rows, ld] int32 (T columns used) with lengths len [rows]; items may share rows:
 *   hypothesis of item i = row hyp_row[i];  references = rows ref_rows[ref_begin[i] .. ref_begin[i + 1]), n_refs = ref_begin[items].
 * Only the first len[row] symbols of a row are read.  An n-gram (n = 1 .. 4) is compared through its exact 64-bit key
 * sum_{j < n} (s_j + 1) << 16 j, so keys of different n never meet.  With L = len of the hypothesis, per item i:
 *   guess[i, n-1]   = max(0, L - n + 1)
 *   correct[i, n-1] = sum over the hypothesis' distinct n-grams g of min(count_hyp(g), max over the references of count_ref(g))
 *   hyp_len[i] = L;  ref_len[i] = the reference length l that minimises (|l - L|, l)   (bleu_scorer's "closest")
 *   lcs[ref_begin[i] + r] = length of the longest common subsequence of the hypothesis and reference r
 *   rouge_l[i] = (1 + b^2) p q / (q + b^2 p) with b = 1.2, p = max_r lcs_r / max(L, 1), q = max_r (lcs_r / max(len_r, 1)); 0 when p or q is 0
 *   bleu[i] (optional) = the sentence form of BLEU-4 on the item's own counts: (prod_n (correct_n + 1e-15) / (guess_n + 1e-9))^(1/4),
 *      times exp(1 - 1 / ratio) when ratio = (L + 1e-15) / (ref_len + 1e-9) < 1
 *   cider[i] (optional; needs the tables) = 10 x mean over the references of the mean over n of val_n, where with
 *      idf(g) = log(n_docs) - log(max(1, df(g))), df(g) looked up by binary search (0 when absent), the tf-idf vectors of the hypothesis
 *      and of the reference over their distinct n-grams and their Euclidean norms:  val_n = sum over the hypothesis' distinct g of
 *      min(tf_h idf, tf_r idf) * (tf_r idf), divided by norm_h norm_r when both are non-zero, times exp(-d^2 / (2 * 6^2)),
 *      d = max(L - 1, 0) - max(len_r - 1, 0)   (cider_scorer's "length" is the bigram count).
 * TABLES: df_keys (ascending uint64) / df_cnt (int32) hold the four per-n tables one after the other, the n-th in entries
 * df_begin[n-1] .. df_begin[n) (HOST words; the keys' construction makes the whole array ascending too).
 * The integers are exact.  The fp64 values are sums in a fixed order (no atomics on them); they do not depend on the number of items.
 * RANGE: 1 <= T <= UNIVL_OVERLAP_TMAX, T <= ld, rows >= 1, 1 <= items <= n_refs, cider only with n_docs >= 1 and consistent df_begin;
 * otherwise, or for a NULL pointer (the optional ones apart), UNIVL_EINVAL and nothing is launched.  What is DATA ON THE DEVICE is
 * clamped and flagged instead, nothing is read out of range: the bits below are OR-ed into *status (the caller clears it) when a length
 * is outside [0, T], a symbol read is outside [0, UNIVL_OVERLAP_SYM_MAX], a row index is outside [0, rows), or an item's reference
 * offsets leave [0, n_refs] or give it no reference; the outputs of such an item are then those of the clamped data. */
#define UNIVL_OVERLAP_TMAX 128
#define UNIVL_OVERLAP_SYM_MAX 65534
#define UNIVL_OVERLAP_BAD_LEN 1
#define UNIVL_OVERLAP_BAD_SYM 2
#define UNIVL_OVERLAP_BAD_ROW 4
#define UNIVL_OVERLAP_BAD_REFS 8
typedef struct UnivlCaptionOverlap {
    const int32_t* sym; int64_t ld;  /* [rows, ld] int32 symbols                                                                  */
    const int32_t* len;              /* [rows]                                                                                    */
    int32_t rows, T, items, n_refs;
    const int32_t* hyp_row;          /* [items]                                                                                   */
    const int32_t* ref_begin;        /* [items + 1]                                                                               */
    const int32_t* ref_rows;         /* [n_refs]                                                                                  */
    const uint64_t* df_keys;         /* [df_begin[4]] or NULL                                                                     */
    const int32_t* df_cnt;           /* [df_begin[4]] or NULL                                                                     */
    int32_t df_begin[5];
    int32_t n_docs;
    int32_t* guess; int32_t* correct;            /* [items, 4] each                                                               */
    int32_t* hyp_len; int32_t* ref_len;          /* [items] each                                                                  */
    int32_t* lcs;                    /* [n_refs]                                                                                  */
    double* rouge_l;                 /* [items]                                                                                   */
    double* cider;                   /* [items] or NULL                                                                           */
    double* bleu;                    /* [items] or NULL                                                                           */
    int32_t* status;                 /* one word, bits OR-ed in                                                                   */
} UnivlCaptionOverlap;
/* sizeof(UnivlCaptionOverlap), for a binding's load-time check.  (The two numbered size tables above keep the lengths bindings pin.) */
int univl_caption_overlap_sizeof(void);
int univl_caption_overlap(const UnivlCaptionOverlap* d, hipStream_t stream);
/* pick[i] = the index of the largest of score[i, 0 .. n_samp) (fp64), equal scores resolving to the LOWER index (the tie rule of
 * univl_beam_step); best[i] (optional) = that score.  A NaN is never the larger one.  n_inst, n_samp >= 1, otherwise UNIVL_EINVAL. */
int univl_consensus_pick(const double* score, int32_t n_inst, int32_t n_samp, int32_t* pick, double* best, hipStream_t stream);
/* Rewards -> per-caption training weights (the advantage of self-critical sequence training), on the device.  reward [n, ns] fp64, in
 * the layout univl_caption_overlap writes rouge_l / bleu in; weight [n, ns] fp32 (the seq_weight of UnivlVocabCEW).
 *   baseline_kind UNIVL_ADV_LOO   (baseline = NULL): the leave-one-out mean of the video's other samples,
 *       A[i, s] = r[i, s] - (S_i - r[i, s]) / (m_i - 1),  S_i the left-to-right sum of the video's finite rewards, m_i their number
 *       (m_i = ns when every reward is finite).  Needs ns >= 2, otherwise UNIVL_EINVAL.
 *   baseline_kind UNIVL_ADV_GIVEN (baseline [n] fp64, e.g. the reward of the greedy or beam caption):  A[i, s] = r[i, s] - b[i].
 * weight[i, s] = (float)(A[i, s] * scale): fp64 throughout, rounded once.  A non-finite reward gives weight 0 for that sample, leaves
 * the other samples' baseline without it, and sets bit 0 (UNIVL_ADV_NONFINITE) of *status; so does a non-finite b[i] (every weight of
 * the video 0), a video left with m_i < 2 under LOO (its weights 0) and a product that is not finite in fp32: no NaN or infinity is ever
 * written.  One thread per video, sums in sample order: bit-reproducible; the one atomic is the integer OR into the status word.
 * n, ns >= 1, no NULL pointer but baseline under LOO; otherwise UNIVL_EINVAL. */
#define UNIVL_ADV_LOO 0
#define UNIVL_ADV_GIVEN 1
#define UNIVL_ADV_NONFINITE 1
int univl_caption_advantage(const double* reward, const double* baseline, int32_t n, int32_t ns, int32_t baseline_kind, double scale,
                            float* weight, int32_t* status, hipStream_t stream);
/* The document-frequency TABLES of UnivlCaptionOverlap, built on the device from token rows: no host read, no synchronisation,
 * capturable.  The row table is UnivlCaptionOverlap's (sym [rows, ld] int32, len [rows], T <= UNIVL_OVERLAP_TMAX, symbols in
 * [0, UNIVL_OVERLAP_SYM_MAX]).  A DOCUMENT i < items is the set of rows ref_rows[ref_begin[i] .. ref_begin[i + 1]); documents may
 * share rows; an empty document contributes nothing.  With the n-gram keys of UnivlCaptionOverlap (n = 1 .. 4),
 *   df(g) = the number of documents in which g occurs at least once, in any of the document's rows, at a position p with p + n <= len.
 * Written:
 *   df_keys [capacity] uint64   every key with df >= 1 exactly once, ascending as UNSIGNED 64-bit numbers (the four per-n tables one
 *                               after the other: keys of a larger n are larger numbers)
 *   df_cnt  [capacity] int32    the matching df
 *   df_begin [5] int32          DEVICE words: the n-grams are entries df_begin[n-1] .. df_begin[n)
 * Entries at and past df_begin[4] are left as they were.  The result is a function of the multiset of (document, key) pairs: integer
 * atomics order the intermediate buffers, never the outputs, which are bit-reproducible.  No float arithmetic.
 * LAUNCHES (csrc/ngram_df.hip), every grid sized from n_refs, T and capacity, the true counts read from device words:
 *   emit   one wave per document: a row's n-gram is emitted unless an equal key stands earlier in the row or in an earlier row of
 *          the document; one integer atomic on a device cursor per row hands out the slots
 *   sort   LSD radix sort of the 64-bit keys, 8 passes of 8 bits: per-tile histogram, one scan over [256][tiles], a stable scatter
 *          over tiles of UNIVL_NGRAM_DF_TILE keys
 *   fold   head flags, the same scan, compaction to (key, run start), run lengths and the three lower-bound searches of df_begin
 * CAPACITY: the caller's statement of df_keys' / df_cnt's length; n_refs * 4 T always suffices.  With more distinct keys than that,
 * bit UNIVL_NGRAM_DF_OVERFLOW is OR-ed into *status, nothing is written at or past capacity, every df_begin entry is <= capacity, and
 * the contents are otherwise unspecified.
 * WORKSPACE: 64 + 16 N + 1024 ceil(N / UNIVL_NGRAM_DF_TILE) bytes with N = 4 T n_refs (the control words, two key buffers, the
 * histograms), 16-byte aligned (UNIVL_EALIGN); univl_ngram_df_ws_bytes evaluates this on the host (-1 for arguments univl_ngram_df
 * would refuse; N must stay below 2^31).
 * RANGE: 1 <= T <= UNIVL_OVERLAP_TMAX, T <= ld, rows, items, n_refs, capacity >= 1, no NULL pointer, ws_bytes as above; otherwise
 * UNIVL_EINVAL and nothing is launched.  DATA ON THE DEVICE is clamped and flagged as in univl_caption_overlap, with the same
 * UNIVL_OVERLAP_BAD_LEN / _SYM / _ROW / _REFS bits OR-ed into *status (the caller clears it) and nothing read out of range; _REFS:
 * a document's offsets leave [0, n_refs] or decrease (it is then the clamped range, empty when decreasing).  Offsets that are not
 * monotone can make documents overlap and list more than n_refs rows in all: what no longer fits N keys is dropped and
 * UNIVL_NGRAM_DF_OVERFLOW is set as well. */
#define UNIVL_NGRAM_DF_OVERFLOW 16
#define UNIVL_NGRAM_DF_TILE 4096
typedef struct UnivlNgramDf {
    const int32_t* sym; int64_t ld;  /* [rows, ld] int32 symbols                                                                  */
    const int32_t* len;              /* [rows]                                                                                    */
    int32_t rows, T, items, n_refs;
    const int32_t* ref_begin;        /* [items + 1]                                                                               */
    const int32_t* ref_rows;         /* [n_refs]                                                                                  */
    uint64_t* df_keys;               /* [capacity] written                                                                        */
    int32_t* df_cnt;                 /* [capacity] written                                                                        */
    int32_t* df_begin;               /* [5] device words, written                                                                 */
    int32_t* status;                 /* one word, bits OR-ed in                                                                   */
    int32_t capacity, reserved;      /* reserved: 0                                                                               */
    void* ws; int64_t ws_bytes;      /* see WORKSPACE                                                                             */
} UnivlNgramDf;
/* sizeof(UnivlNgramDf) (in neither numbered size table) and the scatter tile, for a binding's load-time check */
int univl_ngram_df_sizeof(void);
int univl_ngram_df_tile(void);
int64_t univl_ngram_df_ws_bytes(int32_t n_refs, int32_t T);
int univl_ngram_df(const UnivlNgramDf* d, hipStream_t stream);
/* ---------------------------------------------------------------------------------------- retrieval search
 * The k best gallery rows of every query row by inner product -- torch.matmul(text, video.t()) of modeling.py:389 followed by a
 * row-wise top-k -- WITHOUT the [Nq, Ng] score matrix: the 768-deep product's epilogue keeps a running top-k per query and never
 * writes the tile (the pattern of univl_vocab_ce_fwd).  Two launches, no host read, capturable:
 *   scan   grid (query tiles of 16 / 32 rows, gallery slices), 512 threads: the query tile stays in LDS, gallery tiles of 128 rows are
 *          streamed from global memory into f32 MFMA operands (fp32 accumulate); every score is tested against the query's current
 *          k-th entry before any insert; a slice's sorted k best and its partial counts go to the workspace;
 *   merge  one wave per query row over the slices' lists.
 * Outputs, per query row i:  idx[i, 0..k) / score[i, 0..k) = the k best gallery rows, sorted by DESCENDING score.  TIE RULE (the one
 * univl_beam_step fixes, part of the contract): equal fp32 scores are ordered by LOWER gallery index first.  With Ng < k the entries
 * Ng .. k-1 are idx = -1, score = -inf.  Behaviour on NaN values: unspecified.
 * Rank counts (optional): with target ([Nq] int32, each in [0, Ng); a value outside is not refused -- the device cannot report it --
 * but CLAMPED to that range, so the counts are then those of row 0 or Ng - 1 and nothing is read outside the gallery) also
 *   gt[i] = #{j : s(i, j) > s(i, target[i])},   eq[i] = #{j : s(i, j) == s(i, target[i])}  (>= 1: the target itself)
 * -- the two counts of univl_rank_counts for an ARBITRARY ground-truth column, so several queries may share a gallery row and
 * Nq != Ng is allowed.  k = 0 produces the counts only (idx / score may be NULL) and needs target.
 * SCORE CONTRACT: s(i, j) is a pure function of the 768 values of q_i and g_j -- one fixed fp32 accumulation chain.  Its bits do not
 * depend on Nq, Ng, the row's position in a tile, the slice count or deterministic mode; there are no float atomics and no
 * order-dependent reduction across workgroups.  Equality of scores is therefore meaningful (tie rule, eq), and a gallery searched in
 * pieces merges exactly: sort the pieces' results by (score descending, global index ascending).
 * Range: H == 768 (as univl_pool_fwd), Nq >= 1, Ng >= 1, 0 <= k <= UNIVL_TOPK_MAX, ldq / ldg >= H, 0 <= slices <=
 * UNIVL_TOPK_SLICES_MAX; otherwise, for a NULL pointer, for k == 0 without target or for a workspace that is too small, UNIVL_EINVAL.
 * Rows of q and g (base and leading dimension) and the workspace must be 16-byte aligned (UNIVL_EALIGN).
 * WORKSPACE: Nq * S * (8 * k + 8) bytes, S = the number of slices the call uses:  with T = ceil(Ng / 128) gallery tiles and
 * QT = ceil(Nq / (Nq <= 16 ? 16 : 32)) query tiles,  want = slices ? slices : ceil(256 / QT)  (query tiles x slices fills the 256
 * compute units once),  want = min(want, UNIVL_TOPK_SLICES_MAX, T),  S = ceil(T / ceil(T / want)).  univl_sim_topk_workspace
 * evaluates this on the host (no device work; < 0 for arguments univl_sim_topk would refuse). */
#define UNIVL_TOPK_MAX 64
#define UNIVL_TOPK_SLICES_MAX 256
typedef struct UnivlSimTopk {
    const float* q; int64_t ldq;     /* [Nq, ldq] fp32 queries                                                                    */
    const float* g; int64_t ldg;     /* [Ng, ldg] fp32 gallery                                                                    */
    int32_t Nq, Ng, H, k;            /* H must be 768; k = 0: rank counts only                                                    */
    int32_t slices;                  /* 0: the library chooses; 1 .. UNIVL_TOPK_SLICES_MAX: forced (capped at the tile count)     */
    int32_t reserved;                /* 0                                                                                          */
    int32_t* idx; float* score;      /* [Nq, k] each, written (k > 0)                                                             */
    const int32_t* target;           /* optional [Nq]: the ground-truth gallery row of every query                                */
    int32_t* gt; int32_t* eq;        /* [Nq] each, written when target is given                                                   */
    void* ws; int64_t ws_bytes;      /* 16-byte aligned scratch, see WORKSPACE                                                    */
} UnivlSimTopk;
int univl_sim_topk(const UnivlSimTopk* d, hipStream_t stream);
int64_t univl_sim_topk_workspace(int32_t Nq, int32_t Ng, int32_t k, int32_t slices);
/* ---------------------------------------------------------------------------------------- query-bank normalised search
 * Search-time normalisation against hubness (QB-Norm's dynamic inverted softmax, dual-softmax inference): a gallery row that a BANK of
 * other queries already claims strongly is marked down.  With s(a, g) the score of univl_sim_topk (its SCORE CONTRACT, the same
 * accumulator chain), a bank of Nb >= 1 rows b and a finite beta > 0:
 *   column term       c_j = m_j + log(sum_b exp(beta * (s(b, j) - m_j))) / beta,   m_j = max_b s(b, j)      (never overflows)
 *   normalised score  s'(i, j) = gate_i ? s(i, j) - c_j : s(i, j)                  (ONE fp32 subtraction; ranking by s' is ranking
 *                     by exp(beta s(i, j)) / sum_b exp(beta s(b, j)))
 *   hub set           hub[j] = 1 iff j is among the hub_k best gallery rows of some bank row (raw score, TIE RULE of univl_sim_topk)
 *   dynamic gate      gate_i = hub[raw top-1 of query i]                            (static: every gate is 1)
 * univl_sim_colstat computes c[Ng] without the [Nb, Ng] matrix.  Two launches, no host read, capturable:
 *   scan   grid (gallery tiles of 32 rows, bank slices), 512 threads: univl_sim_topk's scan with the roles swapped -- the gallery
 *          tile stays in LDS, bank tiles of 128 rows are streamed into the MFMA operands, and instead of a ranked list every gallery
 *          row keeps a running (max, sum of exp) pair: one partial per bank tile, reduced over its 128 rows in a fixed tree, folded
 *          into the running pair in ascending tile order; a slice's pair goes to the workspace;
 *   merge  one thread per gallery row folds the slices' pairs in ascending order and writes c.
 * PURITY: the bits of c_j depend on g_j, the bank (its rows and their order) and beta, and on nothing else -- not on Ng, the row's
 * place in the gallery or a tile, or deterministic mode; there are no float atomics.  The slice rule is a function of Nb alone:
 * T = ceil(Nb / 128) bank tiles, ceil(T / UNIVL_COLSTAT_SLICES) tiles per slice, S = ceil(T / that) slices.  A gallery normalised
 * in pieces is therefore the gallery normalised whole, element for element, and s' is a pure function of (q_i, g_j, bank, beta,
 * gate_i): the tie rule, eq and the exact merging of gallery pieces hold for the normalised search as they do for the plain one.
 * Range: H == 768, Nb >= 1, Ng >= 1, beta finite and > 0, ldb / ldg >= H, rows 16-byte aligned (UNIVL_EALIGN), workspace of
 * univl_sim_colstat_workspace(Nb, Ng) = 8 * S * Ng bytes (host only; < 0 for arguments univl_sim_colstat would refuse). */
#define UNIVL_COLSTAT_SLICES 32
typedef struct UnivlSimColstat {
    const float* bank; int64_t ldb;  /* [Nb, ldb] fp32 bank rows                                                                  */
    const float* g; int64_t ldg;     /* [Ng, ldg] fp32 gallery                                                                    */
    int32_t Nb, Ng, H;               /* H must be 768                                                                             */
    float beta;                      /* finite, > 0                                                                               */
    float* c;                        /* [Ng] written                                                                              */
    void* ws; int64_t ws_bytes;      /* 16-byte aligned scratch, univl_sim_colstat_workspace                                      */
} UnivlSimColstat;
int univl_sim_colstat_sizeof(void);
int univl_sim_colstat(const UnivlSimColstat* d, hipStream_t stream);
int64_t univl_sim_colstat_workspace(int32_t Nb, int32_t Ng);
/* univl_sim_topk on s': UnivlSimTopk's fields with UnivlSimTopk's meaning, range, workspace and refusals, then the column term and the
 * gates.  Everything univl_sim_topk states about s holds for s': the sorted lists with the tie rule, the -1 / -inf padding, gt / eq
 * against target, whose score is s(i, target[i]) - c[target[i]] by the same subtraction, k == 0, the bit-exact merging of gallery
 * pieces (each piece with its piece of col_bias).  The same scan kernel (its NORM instantiation; univl_sim_topk is the other one):
 * the bias is read once per tile and lane where the scores leave the LDS score buffer.  A NULL col_bias is UNIVL_EINVAL. */
typedef struct UnivlSimTopkNorm {
    const float* q; int64_t ldq;
    const float* g; int64_t ldg;
    int32_t Nq, Ng, H, k;
    int32_t slices;
    int32_t reserved;
    int32_t* idx; float* score;
    const int32_t* target;
    int32_t* gt; int32_t* eq;
    void* ws; int64_t ws_bytes;      /* univl_sim_topk_workspace(Nq, Ng, k, slices)                                               */
    const float* col_bias;           /* ... then [Ng] fp32: c_j (any finite values: the kernel subtracts what it is given)        */
    const int32_t* row_gate;         /* optional [Nq] int32: 0 leaves the query's scores untouched; NULL: every gate is 1         */
} UnivlSimTopkNorm;
int univl_sim_topk_norm_sizeof(void);
int univl_sim_topk_norm(const UnivlSimTopkNorm* d, hipStream_t stream);
/* hub[idx[e]] = 1 for every e < n with 0 <= idx[e] < Ng (plain stores of 1; duplicates and the -1 padding of univl_sim_topk are
 * harmless).  hub is NOT cleared: the caller zeroes it, so that several lists may be scattered into one set. */
int univl_hub_flags(const int32_t* idx, int64_t n, int32_t Ng, int32_t* hub, hipStream_t stream);
/* gate[i] = hub[top1[i * ld]] != 0 for i < Nq (0 for an index outside [0, Ng)): top1 is the first column of univl_sim_topk's idx. */
int univl_hub_gate(const int32_t* top1, int64_t ld, int32_t Nq, const int32_t* hub, int32_t Ng, int32_t* gate, hipStream_t stream);
/* ---------------------------------------------------------------------------------------- moment search
 * WHERE in a retrieved video a text matches: the best window of frames.  The model defines the score -- _mean_pooling_for_similarity
 * over the window, F.normalize unless use_mil, the inner product with the pooled text (modeling.py:377-391 with the video mask narrowed
 * to the window); here every window of a video is scored in one launch.
 * For a query vector q, gallery row v with frames x_0 .. x_{F-1} (768 wide) and mask m, a window (s, L) covers frames s .. s + L - 1.
 *   candidate   iff lmin <= L <= lmax, 0 <= s, s + L <= F and every frame in it has m != 0: a padded tail or a hole in the mask never
 *               lies inside a window
 *   u(s, L)     = x_s + .. + x_{s + L - 1}
 *   score       normalize = 1:  (q . u) / max(|u|, 1e-12 * L)     -- univl_pool_fwd's normalised value (eps 1e-12 on the mean) dotted with q
 *               normalize = 0:  (q . u) / L                       -- use_mil models
 *   ORDER       larger score first; equal scores by lower s; then by smaller L
 *   result      per pair: start (int32), length (int32), score (fp32); (-1, 0, -inf) for a pair without a candidate window and for a
 *               candidate id outside [0, N) -- the -1 padding of univl_sim_topk among them; such a pair reads nothing of the gallery
 * univl_window_norms writes |u(s, L)| of every window of N rows into wnorm [N][F][F] fp32, indexed (s, L - 1): 0 from the first window
 * of a start that holds a frame with m == 0 on, 0 past the row's end (s + L > F).  Independent of lmin / lmax and of any query: it
 * depends on the video alone and is computed once per row.  Not needed with normalize = 0.  One wave owns a start and extends u frame
 * by frame in registers (12 columns per lane); the frames are read from L2, never staged (a row of 128 frames is 393 KB).
 * univl_moment_localize scores, for each of the P = Nq * K pairs (query row p / K, gallery row rows[p]), every candidate window and
 * reduces them to the best under ORDER.  One workgroup per pair: the F frame products d_f = q . x_f, then one thread per start grows
 * the numerators d_s + .. + d_{s + L - 1} and divides by the table entry (or L).  One launch each, no host read, capturable.
 * PURITY: the score is a function of q, the row's frames and mask, (s, L) and normalize only -- not of the pair's position in the
 * launch, the grid, the other pairs, N, or deterministic mode; |u(s, L)| likewise of frames s .. s + L - 1 alone.  Equal scores are
 * therefore meaningful.  Every reduction runs in a fixed order (768 columns: 12 per lane as one fmaf chain in column order, then the xor
 * butterfly of the wave); there are no float atomics.  q . u and |u| are built BY EXTENSION from the window's start, never as a
 * difference of prefix sums: LayerNorm outputs have |x_f|^2 near 768, and a summed-area table in fp32 loses about 1e-4 relative on a
 * one-frame window.
 * Range: H == 768, 1 <= F <= UNIVL_MOMENT_F_MAX, N >= 1, ld_row >= F * 768, normalize 0 or 1; localize also 1 <= lmin <= lmax <= F,
 * Nq >= 1, K >= 1, ldq >= 768; otherwise, or for a NULL pointer, UNIVL_EINVAL.  Rows of frames and q (base and leading dimension)
 * must be 16-byte aligned (UNIVL_EALIGN).  Behaviour on NaN values: unspecified. */
#define UNIVL_MOMENT_F_MAX 128
typedef struct UnivlMoment {
    const float* frames; int64_t ld_row; /* [N, F, 768] fp32 frames of the gallery rows, ld_row floats between rows               */
    const int64_t* mask;                 /* [N, F] int64, contiguous: 0 = not a frame                                             */
    float* wnorm;                        /* [N, F, F] fp32: written by univl_window_norms, read by univl_moment_localize           */
    int32_t N, F, H;                     /* H must be 768                                                                         */
    int32_t normalize;                   /* 1: divide by max(|u|, 1e-12 L); 0: by L (wnorm may be NULL)                           */
    /* univl_moment_localize only */
    const float* q; int64_t ldq;         /* [Nq, ldq] fp32 pooled queries                                                         */
    const int32_t* rows;                 /* [Nq, K] candidate gallery rows; outside [0, N): (-1, 0, -inf)                          */
    int32_t Nq, K;
    int32_t lmin, lmax;
    int32_t* start; int32_t* length;     /* [Nq, K] each, written                                                                 */
    float* score;                        /* [Nq, K] written                                                                       */
} UnivlMoment;
int univl_moment_sizeof(void);
int univl_window_norms(const UnivlMoment* d, hipStream_t stream);
int univl_moment_localize(const UnivlMoment* d, hipStream_t stream);
/* ---------------------------------------------------------------------------------------- n-best moments with temporal NMS
 * SEVERAL windows per (query, gallery row) pair: greedy non-maximum suppression over univl_moment_localize's own candidates, on the
 * device, for "R@n, IoU = m" tables and for texts that match a video in more than one place.  Candidate windows, their scores and
 * ORDER (larger score first, then lower start, then smaller length) are exactly univl_moment_localize's.  For each pair, with every
 * candidate alive at first, for m = 0 .. M - 1:
 *   pick        the first live candidate under ORDER goes to slot m
 *   suppress    the pick dies, and so does every live window w with  iou_den * inter(w, pick) > iou_num * union(w, pick);  inter and
 *               union are counted in frames, in integers: no float enters a suppression decision
 *   empty       when nothing is alive, slot m and all later slots are (-1, 0, -inf)
 * A row id outside [0, N) gives (-1, 0, -inf) in all M slots, decided for the whole workgroup before anything of the gallery is read.
 * Consequences: slot 0 is univl_moment_localize's triple bit for bit, and M = 1 is univl_moment_localize; iou_num == iou_den
 * suppresses nothing but the pick itself, so the result is the plain top-M windows under ORDER; iou_num == 0 yields pairwise
 * disjoint windows; the scores of a pair's slots never increase from slot to slot.
 * One workgroup of 256 threads per pair, one launch, no workspace, no host read, no atomics, capturable.  The frame products and
 * the visit of a start's windows are univl_moment_localize's device functions (the numerator grown by extension, the same
 * denominator: that is what makes slot 0 bit-identical); thread s < F stores every score in LDS instead of folding it -- length-major
 * and triangular, row L holding the F - L + 1 starts of length L, lengths lmin .. lmax only: at most 8 256 floats (33 KB) -- so the
 * norm table is read once per window, not once per round.  A round is one walk per thread over its own stored scores (it marks what
 * the previous pick suppresses with NaN, which no live score equals, and keeps its best survivor) and the reduction of the F bests
 * that univl_moment_localize runs, under the same total order.
 * PURITY: a pair's result is a function of its q row, the gallery row (frames, mask, table rows), (lmin, lmax), normalize and
 * (M, iou_num, iou_den) only -- not of its place in the launch, the other pairs, N, or deterministic mode; the first M slots do not
 * depend on M.
 * Range: 1 <= M <= UNIVL_MOMENT_NBEST_MAX, 1 <= iou_den <= 1024, 0 <= iou_num <= iou_den; everything else as for
 * univl_moment_localize; otherwise, or for a NULL pointer, UNIVL_EINVAL; rows of frames and q 16-byte aligned (UNIVL_EALIGN); all
 * before any launch.  Behaviour on NaN or infinite values: unspecified. */
#define UNIVL_MOMENT_NBEST_MAX 16
typedef struct UnivlMomentNbest {
    const float* frames; int64_t ld_row; /* [N, F, 768] fp32 frames of the gallery rows, ld_row floats between rows               */
    const int64_t* mask;                 /* [N, F] int64, contiguous: 0 = not a frame                                             */
    const float* wnorm;                  /* [N, F, F] fp32 from univl_window_norms (may be NULL with normalize = 0)               */
    int32_t N, F, H;                     /* H must be 768                                                                         */
    int32_t normalize;
    const float* q; int64_t ldq;         /* [Nq, ldq] fp32 pooled queries                                                         */
    const int32_t* rows;                 /* [Nq, K] candidate gallery rows; outside [0, N): (-1, 0, -inf) in every slot            */
    int32_t Nq, K;
    int32_t lmin, lmax;
    int32_t M;                           /* windows per pair                                                                      */
    int32_t iou_num, iou_den;            /* w dies iff iou_den * inter > iou_num * union                                          */
    int32_t reserved;
    int32_t* start; int32_t* length;     /* [Nq, K, M] each, written                                                              */
    float* score;                        /* [Nq, K, M] written                                                                    */
} UnivlMomentNbest;
int univl_moment_nbest_sizeof(void);
int univl_moment_nbest(const UnivlMomentNbest* d, hipStream_t stream);
/* ---------------------------------------------------------------------------------------- ordered step alignment
 * WHERE every step of an ORDERED list of texts happens in a video (action step localisation; with lmin = lmax = 1 the dynamic
 * programme of CrossTask: one frame per step, frames strictly increasing).  The gallery side -- frames, ld_row, mask, wnorm, N, F, H,
 * normalize -- is UnivlMoment's, and so is the score of one window for one step vector.
 * For list i (its counts[i] = n step vectors q[i, 0 .. n - 1]; K is only the padding of a list) and gallery row v = rows[i, c]:
 *   alignment   n windows (s_k, L_k), k < n, each a candidate window of univl_moment_localize (lmin <= L_k <= lmax, every frame valid
 *               by the mask), with s_k + L_k <= s_{k+1}: in order, never overlapping.  Gaps may hold anything, masked frames too
 *   w_k         the score of (s_k, L_k) for q[i, k], bit for bit univl_moment_localize's: the numerator grown by extension over the
 *               same frame products, divided by max(wnorm, 1e-12 L) or by L
 *   total       T_n = 0, T_k = w_k + T_{k+1} in fp32, the total is T_0: summed from the last step to the first
 *   result      the alignment of largest total.  EQUAL totals are decided by this suffix programme, which is the contract:
 *                 A[k][s] = max over L of w(k, s, L) + G[k+1][s + L], lengths ascending, a later one only if strictly larger
 *                 G[k][t] = max over s >= t of A[k][s],   G[n][.] = 0
 *                 walk from k = 0, t = 0: s_k = the lowest s >= t with A[k][s] == G[k][t], L_k its length, t = s_k + L_k
 *               i.e. the lexicographically smallest (s_0, L_0, s_1, L_1, ..) among the alignments whose every suffix total T_k is the
 *               largest one from its frame on (where the sums are exact: among all alignments of equal total)
 *   outputs     start, length (int32), score (fp32) [Nl, C, K]; total (fp32) [Nl, C].  Slots k >= n: (-1, 0, -inf).  No alignment
 *               (ALL OR NOTHING): every slot (-1, 0, -inf), total -inf.  A row outside [0, N) or counts[i] outside [1, K]: the same,
 *               decided for the whole workgroup before anything of the gallery or of q is read.  q rows k >= counts[i] are never read
 * One workgroup of 256 threads per (list, candidate): the frame products d[k][f] = q_k . x_f into LDS (a wave keeps four frames in
 * registers and walks the list's vectors: the row's frames are read once per pair), then for k = n - 1 .. 0 thread s < F grows start
 * s's numerators, adds G[k+1][s + L] and keeps A[k][s] with its length; one wave turns A[k] into G[k] and the first start that
 * attains it (a suffix scan in registers); one thread walks forward.  The [K, F, F] window scores are never stored.  LDS: 16 KB of
 * products, 8 KB of lengths and first starts, 2 KB of A, G and the mask.  One launch, no host read, no atomics, capturable.
 * PURITY: a pair's result is a function of its n vectors, the row's frames, mask and table rows, (lmin, lmax) and normalize only --
 * not of its place in the launch, the other pairs, K, C or deterministic mode.  With n = 1 the triple and the total are
 * univl_moment_localize's triple, bit for bit (the total up to the sign of a zero).
 * Range: UnivlMoment's for the gallery side and (lmin, lmax); 1 <= K <= UNIVL_STEP_K_MAX, Nl >= 1, C >= 1, Nl * C < 2^31,
 * ldq >= 768 (a list's vectors are ldq floats apart, lists K * ldq); otherwise, or for a NULL pointer, UNIVL_EINVAL; rows of frames
 * and q 16-byte aligned (UNIVL_EALIGN).  Behaviour on NaN values: unspecified. */
#define UNIVL_STEP_K_MAX 32
typedef struct UnivlStepAlign {
    const float* frames; int64_t ld_row; /* [N, F, 768] fp32 frames of the gallery rows, ld_row floats between rows               */
    const int64_t* mask;                 /* [N, F] int64, contiguous: 0 = not a frame                                             */
    const float* wnorm;                  /* [N, F, F] fp32 from univl_window_norms (may be NULL with normalize = 0)               */
    int32_t N, F, H;                     /* H must be 768                                                                         */
    int32_t normalize;
    const float* q; int64_t ldq;         /* [Nl, K, ldq] fp32 pooled step vectors                                                 */
    const int32_t* counts;               /* [Nl] on the device: the steps of list i are its first counts[i] vectors               */
    const int32_t* rows;                 /* [Nl, C] candidate gallery rows                                                        */
    int32_t Nl, C, K;
    int32_t lmin, lmax, reserved;
    int32_t* start; int32_t* length;     /* [Nl, C, K] each, written                                                              */
    float* score;                        /* [Nl, C, K] written                                                                    */
    float* total;                        /* [Nl, C] written                                                                       */
} UnivlStepAlign;
int univl_step_align_sizeof(void);
int univl_step_align(const UnivlStepAlign* d, hipStream_t stream);
/* ---------------------------------------------------------------------------------------- frame-wise segmentation
 * WHICH of a SET of texts, if any, every frame of a video shows (action segmentation; COIN's frame accuracy is counted over such
 * labels): the question of the three entries above asked from the video's side.  No order among the labels, a label may occur in
 * several runs or not at all, and a background label stands for "none of these".  The gallery side -- frames, ld_row, mask, wnorm, N,
 * F, H, normalize -- is UnivlMoment's.
 * For label set i (its counts[i] = n label vectors q[i, 0 .. n - 1]; K is only the padding of a set) and gallery row v = rows[i, c],
 * let f_0 < .. < f_{T-1} be the frames of v with mask != 0; a hole in the mask is simply skipped, the frames on its two sides are
 * neighbours.  lambda = switch_penalty, b = background.
 *   e(k, t)     k < n: the score univl_moment_localize gives window (f_t, 1) for q[i, k], bit for bit -- one frame product divided by
 *               max(wnorm[v][f_t][0], 1e-12), or by 1 with normalize = 0.  The background label has index n and e(n, t) = b; b = -inf
 *               means there is no background label
 *   objective   the labelling y_0 .. y_{T-1} of largest  sum_t e(y_t, t) - lambda * #{t >= 1 : y_t != y_{t-1}}
 *   result      EQUAL objectives and the fp32 order of the sums are decided by this suffix programme, which is the contract (all
 *               of it additions, subtractions and comparisons in fp32; y ranges over 0 .. n, labels before the background):
 *                 V[T-1][y] = e(y, T-1);   M[t] = max over y of V[t][y];   a[t] = the lowest y with V[t][y] == M[t]
 *                 V[t][y]   = e(y, t) + max(V[t+1][y], M[t+1] - lambda)
 *                 stay[t][y] = V[t+1][y] >= M[t+1] - lambda                                        -- a tie stays
 *                 walk forward: y_0 = a[0];  y_{t+1} = y_t if stay[t][y_t], else a[t+1];  total = M[0]
 *   outputs     label (int32) [Nl, C, F]: k for a label, -1 for the background, -2 on a masked frame; score (fp32) [Nl, C, F]: e(y_t, t)
 *               of the label chosen, -inf on a masked frame; total (fp32) [Nl, C]; nseg (int32) [Nl, C]: the maximal runs of equal
 *               NON-background labels over the valid frames in order.  All of them are written for every pair.
 *   nothing to label   a row outside [0, N), counts[i] outside [1, K], or a row without a valid frame: label -2 and score -inf on all
 *               F frames, total -inf, nseg 0.  The first two are decided for the whole workgroup before anything of the gallery or of
 *               q is read.  q rows k >= counts[i] are never read
 * Consequences: lambda = 0 is the arg-max of every frame by itself -- among equal scores the lowest label and the background last,
 * except that a label which is among the equals of the next frame too is kept (a tie stays); a lambda larger than every difference of
 * two sums of scores gives one label for the whole video; with n = 1 and b = -inf every valid frame gets label 0.
 * One workgroup of 256 threads per (set, candidate): the frame products d[k][f] = q_k . x_f into LDS as univl_step_align makes them,
 * turned into e(k, f) in place by univl_moment_localize's own visit of window (f, 1); then ONE wave runs the programme over the valid
 * frames from the last to the first -- lane y holds V[.][y] and every lane the background's value, so UNIVL_SEGMENT_K_MAX labels and
 * the background fit one wave; a frame costs one max butterfly over the wave, one ballot for a[t] (the maximum is exact, so the lowest
 * lane that holds it is the lowest label that attains it), one ballot for stay[t][.] and one addition -- and walks forward.  The stay
 * words (64 bits and the background's bit per frame) and a[.] never leave the registers.  LDS: 33 KB of scores (pitch 129 floats, so
 * that the wave reads a column from 64 banks), 1.5 KB of one-frame norms, mask and valid-frame list.  One launch, no workspace, no
 * host read, no atomics, capturable.
 * PURITY: a pair's result is a function of its n vectors, the row's frames, mask and table, lambda, b and normalize only -- not of its
 * place in the launch, the other pairs, K, C or deterministic mode.
 * Range: UnivlMoment's for the gallery side; 1 <= K <= UNIVL_SEGMENT_K_MAX, Nl >= 1, C >= 1, Nl * C < 2^31, ldq >= 768 (a set's vectors
 * are ldq floats apart, sets K * ldq), switch_penalty finite and >= 0, background a number or -inf (not NaN, not +inf); otherwise, or
 * for a NULL pointer (wnorm may be NULL with normalize = 0), UNIVL_EINVAL; rows of frames and q 16-byte aligned (UNIVL_EALIGN); all
 * before any launch.  Behaviour on NaN values in q or the frames: unspecified (no access leaves the buffers). */
#define UNIVL_SEGMENT_K_MAX 64
typedef struct UnivlFrameSegment {
    const float* frames; int64_t ld_row; /* [N, F, 768] fp32 frames of the gallery rows, ld_row floats between rows               */
    const int64_t* mask;                 /* [N, F] int64, contiguous: 0 = not a frame                                             */
    const float* wnorm;                  /* [N, F, F] fp32 from univl_window_norms (may be NULL with normalize = 0)               */
    int32_t N, F, H;                     /* H must be 768                                                                         */
    int32_t normalize;
    const float* q; int64_t ldq;         /* [Nl, K, ldq] fp32 pooled label vectors                                                */
    const int32_t* counts;               /* [Nl] on the device: the labels of set i are its first counts[i] vectors               */
    const int32_t* rows;                 /* [Nl, C] candidate gallery rows                                                        */
    int32_t Nl, C, K;
    float switch_penalty, background;    /* lambda >= 0, finite; b: the score of the background label on every frame, or -inf     */
    int32_t reserved;
    int32_t* label;                      /* [Nl, C, F] written: k, -1 background, -2 masked                                       */
    float* score;                        /* [Nl, C, F] written                                                                    */
    float* total;                        /* [Nl, C] written                                                                       */
    int32_t* nseg;                       /* [Nl, C] written                                                                       */
} UnivlFrameSegment;
int univl_frame_segment_sizeof(void);
int univl_frame_segment(const UnivlFrameSegment* d, hipStream_t stream);
/* ---------------------------------------------------------------------------------------- video-to-video alignment
 * A monotone alignment of the frames of TWO gallery rows (csrc/valign.hip): lay an annotated exemplar over another video of the
 * same task and carry its frame labels across (local = 0), or find the segment two videos share (local = 1).  The four entries
 * above ask a text about a video; this one needs no text at all.  The gallery side -- frames, ld_row, mask, N, F, H -- is
 * UnivlMoment's; no norm table is read.
 * THE SCORE IS ALWAYS THE COSINE OF TWO FRAMES, whatever the model's use_mil says: the model defines no video-video score, so there
 * is no normalize switch here.
 * For pair (a, b) = (ref[p], rows[p, c]) let f_0 < .. < f_{Ta-1} be the frames of a with mask != 0 and g_0 < .. < g_{Tb-1} those of
 * b; a hole in a mask is simply skipped.  Every index written is a FRAME index (f_i, g_j), never a position.
 *   e(i, j)     G(i, j) / (max(na_i, 1e-12f) * max(nb_j, 1e-12f)) - tau, where G(i, j) is the fp32 fmaf chain over k = 0 .. 767,
 *               ascending from 0, of x_{f_i}[k] * y_{g_j}[k], and na_i, nb_j are sqrtf of the same chain over x * x.  These bits are
 *               the contract whatever computes them (here the exact f32 MFMA, whose result is that chain), so e_ab(i, j) ==
 *               e_ba(j, i) and no value depends on the pair's place in the launch, its company, C or deterministic mode
 *   programme   additions and comparisons only.  The predecessors of (i, j) are taken in the order diagonal (i-1, j-1), up (i-1, j),
 *               left (i, j-1); Pm is the largest H among those that exist, among equals the first in that order.
 *                 local = 0   H(0, 0) = e(0, 0), otherwise H(i, j) = e(i, j) + Pm; the end cell is (Ta-1, Tb-1); the path walks the
 *                             recorded predecessors back to (0, 0).  With tau = 1 this is classic DTW under the cosine distance
 *                 local = 1   a cell with no predecessor, or with Pm <= 0, starts a path: H = e; otherwise H = e + Pm; the end cell
 *                             is the largest H, then the lowest i, then the lowest j; the path walks back to its starting cell
 *                             (Smith-Waterman without gaps scored apart; tau is what makes a poor cell negative)
 *   outputs     all written for every pair.  score [P, C]: H at the end cell; path_len [P, C]; path_a, path_b [P, C, 2 F] int32: the
 *               path's cells first to last as frame indices, -1 past path_len (a path holds at most Ta + Tb - 1 < 2 F cells);
 *               match [P, C, F] int32: for frame g of b the a frame of the path cell in its column with the largest e, the lowest i
 *               among equals; -1 for a valid frame the path does not visit (only with local), -2 for a masked frame; match_score
 *               [P, C, F]: that cell's e, -inf where match < 0
 *   nothing to align   ref[p] or rows[p, c] outside [0, N), or either video without a valid frame: score -inf, path_len 0, paths
 *               -1, match -2 and match_score -inf on ALL F frames.  A row out of range is decided for the whole workgroup before
 *               anything of the gallery is read
 * One workgroup of 256 threads per pair; dynamic LDS: the 128 x 128 table of e at a pitch of 136 floats (69 632 B; the K slabs of the
 * Gram phase overlay it), 7 KB static.  One launch, no workspace, no host read, no atomics, capturable.
 * Range: UnivlMoment's for the gallery side; P >= 1, C >= 1, P * C * 2 F < 2^31, tau finite, local 0 or 1; otherwise, or for a NULL
 * pointer, UNIVL_EINVAL; rows of frames 16-byte aligned (UNIVL_EALIGN); all before any launch.  Behaviour on NaN or infinite values
 * in the frames: unspecified (no access leaves the buffers). */
typedef struct UnivlVideoAlign {
    const float* frames; int64_t ld_row; /* [N, F, 768] fp32 frames of the gallery rows, ld_row floats between rows               */
    const int64_t* mask;                 /* [N, F] int64, contiguous: 0 = not a frame                                             */
    int32_t N, F, H;                     /* H must be 768                                                                         */
    int32_t local;                       /* 0: end to end; 1: the best common segment                                             */
    const int32_t* ref;                  /* [P] exemplar gallery rows                                                             */
    const int32_t* rows;                 /* [P, C] candidate gallery rows                                                         */
    int32_t P, C;
    float tau;                           /* subtracted from every cosine                                                          */
    int32_t reserved;
    float* score;                        /* [P, C] written                                                                        */
    int32_t* path_len;                   /* [P, C] written                                                                        */
    int32_t* path_a;                     /* [P, C, 2 F] written                                                                   */
    int32_t* path_b;                     /* [P, C, 2 F] written                                                                   */
    int32_t* match;                      /* [P, C, F] written                                                                     */
    float* match_score;                  /* [P, C, F] written                                                                     */
} UnivlVideoAlign;
int univl_video_align_sizeof(void);
int univl_video_align(const UnivlVideoAlign* d, hipStream_t stream);
/* out[seg[e]] = sum(partials[start[e] .. start[e] + count[e])) for e < n: folds the per-wave partial sums written by the
 * weight-gradient GEMMs (UnivlGemm.sumsq) into the per-tensor sums of squares */
int univl_sumsq_finish(const float* partials, const int32_t* seg, const int32_t* start, const int32_t* count, int32_t n,
                       float* out, hipStream_t stream);
/* x (compute type) *= s[0], s on the device */
int univl_scale_ct_by_device_scalar(int32_t dtype, void* x, int64_t n, const float* s, hipStream_t stream);
int univl_simdense_fwd(const float* x, const float* w, const float* b, int32_t rows, float* out, hipStream_t stream);
int univl_simdense_bwd(const float* ds, const float* x, const float* w, int32_t rows, float* dx, float* dw, float* db,
                       hipStream_t stream);
/* CrossEntropyLoss(ignore_index) over [rows, V] fp32 logits (modeling.py:168,252-254,275): loss = mean over rows with
 * label != ignore_index; dlogits (compute type, [rows, lddl]) = (softmax - onehot) / n_valid.  scratch2: 2 floats. */
int univl_ce_loss(int32_t dtype, const float* logits, int64_t ld, const int64_t* labels, int32_t rows, int32_t V,
                  int32_t ignore_index, float* scratch2, float* loss, void* dlogits, int64_t lddl, hipStream_t stream);
/* K16: the tied vocabulary classifier fused with an ONLINE log-softmax cross entropy -- BertLMPredictionHead.forward's last line
 * (module_bert.py:327-330: h . E_word^T + bias; decoder copy module_decoder.py:180-183) and CrossEntropyLoss(ignore_index) on it
 * (modeling.py:253, 275) without the [rows, V] logits ever existing in memory.
 *   univl_vocab_ce_fwd: walks the product in 128 x 128 tiles; a tile's epilogue leaves one (max, sum exp(logit - max)) pair per row in
 *     partial[row][column tile] and the label's logit in label_logit[row]; two small kernels fold them (fixed order: bit-reproducible)
 *     into lse[rows], rowloss[rows], scratch2[0] = number of rows whose label != ignore_index, loss = mean over those rows (NaN if none).
 *   univl_vocab_ce_bwd: the same product again; the epilogue stores dlogits[row, col] = (exp(logit - lse[row]) - [col == label]) *
 *     gout / n_valid in the compute type (0 on ignored rows) -- the operand of the two backward products (dh = dlogits . E,
 *     dE += dlogits^T . h), which are ordinary univl_gemm calls.  Call after univl_vocab_ce_fwd with the same descriptor.
 * x [rows, K] and table [V, K] in the compute type, K-major, K a multiple of 64 (bf16) / 32 (fp32); slots >= ceil(V / 128);
 * partial holds rows * slots * 2 floats; dlogits rows are lddl >= V elements apart (columns >= V are left untouched). */
typedef struct UnivlVocabCE {
    int32_t dtype, rows, V, K;
    const void* x; int64_t ldx;
    const void* table; int64_t ldt;
    const float* bias;             /* [V] or null */
    const int64_t* labels;         /* [rows] */
    int32_t ignore_index, slots;
    float* partial;                /* [rows, slots, 2] */
    float* label_logit;            /* [rows] */
    float* lse;                    /* [rows] */
    float* rowloss;                /* [rows] */
    float* scratch2;               /* [0] n_valid, [1] sum of the row losses */
    float* loss;                   /* [1] */
    const float* gout;             /* backward: upstream gradient of the loss, one float on the device; null = 1 */
    void* dlogits; int64_t lddl;   /* backward output */
} UnivlVocabCE;
int univl_vocab_ce_fwd(const UnivlVocabCE* desc, hipStream_t stream);
int univl_vocab_ce_bwd(const UnivlVocabCE* desc, hipStream_t stream);
/* K16 weighted form: the same classifier + online log-softmax cross entropy with one fp32 weight per CAPTION -- what self-critical
 * sequence training, minimum-risk training and importance- or confidence-weighted fine-tuning need.  rows = n_seq * seq_len: caption c
 * owns rows [c * seq_len, (c + 1) * seq_len), the convention of UnivlVocabScore.  A row COUNTS when label != ignore_index; with
 * nll_r = lse_r - logit_r[label_r] on counting rows and w_r = seq_weight[r / seq_len]:
 *   univl_vocab_ce_weighted_fwd:
 *     lse[rows]      as univl_vocab_ce_fwd: the same bits on the same operands (the tile walk is the unweighted kernel itself);
 *     rowloss[r]   = w_r * nll_r, 0 on ignored rows;
 *     scratch2[0]  = n_valid, the number of counting rows, independent of the weights;  scratch2[1] = the sum of rowloss;
 *     loss         = (sum_r rowloss[r]) / n_valid, summed in the fixed order of the unweighted loss kernel; NaN when no row counts.
 *   univl_vocab_ce_weighted_bwd:
 *     dlogits[r, col] = (exp(logit - lse_r) - [col == label_r]) * (w_r * (gout / n_valid)) in the compute type; ignored rows and rows whose
 *     weight is 0.0f are exact zeros; columns >= V stay untouched.  Call after the weighted forward with the same descriptor.
 * Weights may be negative or zero.  With every weight 1.0f all outputs (loss, lse, rowloss, scratch2, dlogits) are bit-identical to
 * univl_vocab_ce_fwd / _bwd.  Behaviour on non-finite weights: unspecified.  Every reduction is in fixed order, there are no atomics.
 * Range: as univl_vocab_ce_fwd / _bwd, plus seq_len >= 1 dividing rows and seq_weight != NULL; otherwise UNIVL_EINVAL.
 * The struct is in neither numbered size table: univl_vocab_ce_weighted_sizeof states its size. */
typedef struct UnivlVocabCEW {
    int32_t dtype, rows, V, K;
    const void* x; int64_t ldx;
    const void* table; int64_t ldt;
    const float* bias;             /* [V] or null */
    const int64_t* labels;         /* [rows] */
    int32_t ignore_index, slots;
    float* partial;                /* [rows, slots, 2] */
    float* label_logit;            /* [rows] */
    float* lse;                    /* [rows] */
    float* rowloss;                /* [rows] */
    float* scratch2;               /* [0] n_valid, [1] sum of the weighted row losses */
    float* loss;                   /* [1] */
    const float* gout;             /* backward: upstream gradient of the loss, one float on the device; null = 1 */
    void* dlogits; int64_t lddl;   /* backward output */
    const float* seq_weight;       /* [rows / seq_len] fp32, on the device */
    int32_t seq_len, reserved;     /* reserved: 0 */
} UnivlVocabCEW;
int univl_vocab_ce_weighted_sizeof(void);
int univl_vocab_ce_weighted_fwd(const UnivlVocabCEW* desc, hipStream_t stream);
int univl_vocab_ce_weighted_bwd(const UnivlVocabCEW* desc, hipStream_t stream);
/* K16 smoothed form: torch.nn.CrossEntropyLoss(ignore_index, label_smoothing = eps) on x . table^T + bias, with the optional fp32 weight
 * per caption of the weighted form -- the target of a counting row is (1 - eps) on its label plus eps / V on every one of the V columns.
 * seq_weight may be NULL: seq_len is then ignored and every weight is 1.  With w_r = seq_weight[r / seq_len] (or 1), S_r = the sum of the
 * row's V logits and nll_r = lse_r - logit_r[label_r] on counting rows:
 *   univl_vocab_ce_smooth_fwd:
 *     lse[rows], label_logit[rows]  as univl_vocab_ce_fwd: the same bits on the same operands (the tile epilogue's (max, sum exp) path and
 *                    the row fold are the unsmoothed ones);
 *     partial_sum[r][column tile] = the tile's share of S_r (columns >= V add 0): per lane over its ascending columns, the 16-lane xor
 *                    steps, the column waves in ascending order; the row fold sums the slots lane-strided, then the xor steps;
 *     rowloss[r]   = w_r * fma(1 - eps, nll_r, eps * (lse_r - S_r / V)) in fp32: S_r / V, the difference, the product with eps and
 *                    1 - eps are each rounded, the sum of the two terms is one fused multiply-add, the weight multiplies last;
 *                    0 on ignored rows;
 *     scratch2[0]  = n_valid, independent of weights and eps;  scratch2[1] = the sum of rowloss;
 *     loss         = (sum_r rowloss[r]) / n_valid in the fixed order of the unsmoothed loss kernel; NaN when no row counts.
 *   univl_vocab_ce_smooth_bwd:
 *     dlogits[r, col] = (exp(logit - lse_r) - (1 - eps) * [col == label_r] - eps / V) * (w_r * (gout / n_valid)) in the compute type; ignored
 *     rows and rows whose weight is 0.0f are exact zeros; columns >= V stay untouched.  Call after the smoothed forward with the same
 *     descriptor.  The two backward products that consume dlogits are the ones of univl_vocab_ce_bwd.
 * With smoothing == 0 both entry points ARE the unsmoothed ones -- univl_vocab_ce_fwd / _bwd without weights, univl_vocab_ce_weighted_fwd /
 * _bwd with them: the same launches on the same arguments, every output (loss, lse, rowloss, scratch2, dlogits) bit-identical, partial_sum
 * neither read nor written.  Every reduction is in fixed order, there are no atomics: bit-reproducible in every mode, and a row's outputs
 * do not depend on how many rows the problem has.
 * Range: as univl_vocab_ce_fwd / _bwd, plus smoothing finite in [0, 1), partial_sum != NULL when smoothing > 0 (rows * slots floats), and
 * with seq_weight != NULL a seq_len >= 1 dividing rows; otherwise UNIVL_EINVAL.
 * The struct is in neither numbered size table: univl_vocab_ce_smooth_sizeof states its size. */
typedef struct UnivlVocabCES {
    int32_t dtype, rows, V, K;
    const void* x; int64_t ldx;
    const void* table; int64_t ldt;
    const float* bias;             /* [V] or null */
    const int64_t* labels;         /* [rows] */
    int32_t ignore_index, slots;
    float* partial;                /* [rows, slots, 2] */
    float* label_logit;            /* [rows] */
    float* lse;                    /* [rows] */
    float* rowloss;                /* [rows] */
    float* scratch2;               /* [0] n_valid, [1] sum of the row losses */
    float* loss;                   /* [1] */
    const float* gout;             /* backward: upstream gradient of the loss, one float on the device; null = 1 */
    void* dlogits; int64_t lddl;   /* backward output */
    const float* seq_weight;       /* [rows / seq_len] fp32, on the device; null = every weight 1 */
    int32_t seq_len, reserved;     /* reserved: 0 */
    float smoothing;               /* eps in [0, 1) */
    int32_t reserved2;             /* 0 */
    float* partial_sum;            /* [rows, slots]; may be null when smoothing == 0 */
} UnivlVocabCES;
int univl_vocab_ce_smooth_sizeof(void);
int univl_vocab_ce_smooth_fwd(const UnivlVocabCES* desc, hipStream_t stream);
int univl_vocab_ce_smooth_bwd(const UnivlVocabCES* desc, hipStream_t stream);
/* K16 scoring form: teacher-forced SCORING on the tied vocabulary classifier -- the forward of K16 with the questions an evaluation asks of the
 * logits answered in the product's epilogue: for x [rows, K] . table [V, K]^T + bias (module_bert.py:327-330, decoder copy
 * module_decoder.py:180-183) and labels [rows], what log_softmax + gather + arg-max over the [rows, V] logits would give
 * (a caller of decoder_caption with get_logits, modeling.py:409-428; the label convention of modeling.py:253) -- and the logits are
 * never written.  Forward only.  rows = n_seq * seq_len: caption s owns rows [s * seq_len, (s + 1) * seq_len).
 * A row COUNTS when label != ignore_index and 0 <= label < V; any other label is treated as ignored and reads nothing out of range.
 * Outputs:
 *   lse[row]           = logsumexp of the row's logits
 *   token_logprob[row] = logit[label] - lse[row]; 0 where the row does not count
 *   top_token[row], top_logprob[row] = the row's arg-max column and max - lse[row].  TIE RULE (the one univl_beam_step and
 *                        univl_sim_topk fix, part of the contract): equal fp32 logits resolve to the LOWER column
 *   seq_logprob[s]     = ((t0 + t1) + t2) + ... over the caption's token_logprob in ascending row order, one fp32 chain
 *   seq_tokens[s]      = the caption's counting rows;  seq_correct[s] = those whose top_token equals the label
 * Three launches, no host read, capturable: the 128 x 128 tile walk of K16 (a tile's epilogue leaves one (max, sum exp(logit - max),
 * column of the max) triple per row in slot [row][column tile]: 16-lane shuffles in a wave, LDS across the column waves), a wave per
 * row that folds the slots in slot order, a wave per caption for the sums.  Every reduction is in fixed order -- results are
 * bit-reproducible in every mode -- and there are no float atomics.  Behaviour on NaN logits: unspecified.
 * Range: rows >= 1, V >= 1, K a multiple of 64 (bf16) / 32 (fp32), seq_len >= 1 dividing rows, slots >= ceil(V / 128), ldx / ldt >= K,
 * x and table 16-byte aligned with 16-byte row pitches, no NULL pointer but bias; otherwise UNIVL_EINVAL. */
typedef struct UnivlVocabScore {
    int32_t dtype, rows, V, K;
    const void* x; int64_t ldx;    /* [rows, K] compute type, K-major */
    const void* table; int64_t ldt;/* [V, K] compute type, K-major */
    const float* bias;             /* [V] or null */
    const int64_t* labels;         /* [rows] */
    int32_t ignore_index, slots;
    int32_t seq_len, reserved;     /* reserved: 0 */
    float* partial;                /* scratch [rows, slots, 2] */
    int32_t* partial_top;          /* scratch [rows, slots] */
    float* label_logit;            /* scratch [rows] */
    float* token_logprob;          /* [rows] */
    int32_t* top_token;            /* [rows] */
    float* top_logprob;            /* [rows] */
    float* lse;                    /* [rows] */
    float* seq_logprob;            /* [rows / seq_len] */
    int32_t* seq_tokens;           /* [rows / seq_len] */
    int32_t* seq_correct;          /* [rows / seq_len] */
} UnivlVocabScore;
int univl_vocab_score(const UnivlVocabScore* desc, hipStream_t stream);
/* masked-frame NCE of UniVL._calculate_mfm_loss (modeling.py:285-297) on the [n,n] logits matrix */
int univl_mfm_nce_loss(const float* logits, int64_t ld, const int64_t* vmask, const int64_t* labels, int32_t n,
                       float* scratch2, float* loss, float* dlogits, int64_t lddl, hipStream_t stream);

/* -------------------------------------------------------------------------------------------- optimizer
 * Fused multi-tensor BertAdam (modules/optimization.py:103-168) + clip_grad_norm_ (main_task_retrieval.py:347)
 * over FLAT parameter / gradient / moment buffers.  `segs` describes the parameter tensors (device array). */
typedef struct UnivlSeg {
    int64_t offset, numel;      /* element range in the flat buffers                                     */
    float lr, weight_decay;     /* group hyper-parameters (main_task_retrieval.py:185-190)               */
    float max_grad_norm;        /* per-parameter clip of optimization.py:135-136 (<=0: off)              */
    int32_t active;             /* 0: parameter has no gradient this step (skipped, as `p.grad is None`) */
} UnivlSeg;
/* sumsq[s] = sum of squares of segment s of g (fp32 atomics; sumsq must be zeroed by the caller). */
int univl_grad_sumsq(const float* g, const UnivlSeg* segs, int32_t nseg, const int32_t* chunk_seg,
                     const int64_t* chunk_off, const int32_t* chunk_len, int32_t nchunk, float* sumsq,
                     hipStream_t stream);
/* total-norm clip coefficient: coef[0] = min(1, max_norm / (sqrt(sum_active sumsq) + 1e-6)), coef[1] = total norm */
int univl_clip_coef(const float* sumsq, const UnivlSeg* segs, int32_t nseg, float max_norm, float* coef, hipStream_t stream);
/* g *= coef[0] over all active segments (in-place form of clip_grad_norm_) */
int univl_scale_grads(float* g, const UnivlSeg* segs, const int32_t* chunk_seg, const int64_t* chunk_off,
                      const int32_t* chunk_len, int32_t nchunk, const float* coef, hipStream_t stream);
/* Alignment: the kernels pick their 16-byte vector path from a chunk's element offset alone (offset % 4 == 0), so p / g / m / v must be
 * 16-byte aligned and p16 / p16_lo (where given) 8-byte aligned.  univl_bert_adam, univl_bert_adam_range, univl_gemm_rider and the
 * launches that carry chunks (univl_gemm_ln, univl_attention_fwd_fused) return UNIVL_EINVAL otherwise, before any launch. */
typedef struct UnivlAdam {
    float* p; const float* g; float* m; float* v;   /* flat fp32 buffers, 16-byte aligned                 */
    void* p16;                   /* optional bf16 shadow of p (same offsets, 8-byte aligned), rewritten by the step */
    const UnivlSeg* segs; int32_t nseg;
    const int32_t* chunk_seg; const int64_t* chunk_off; const int32_t* chunk_len; int32_t nchunk;
    const float* sumsq;          /* per-segment sum of squares of the UNSCALED g                          */
    const float* coef;           /* optional global clip coefficient still to be applied (deferred clip)  */
    int32_t* step;               /* [nseg] per-parameter step counters (state['step'])                    */
    float b1, b2, eps;
    float warmup; int32_t t_total;   /* warmup_linear schedule (optimization.py:38-43), t_total -1: constant */
    float* seg_scalars;          /* scratch [nseg*2]                                                       */
    int32_t schedule;            /* 0 warmup_linear, 1 warmup_cosine, 2 warmup_constant (optimization.py:26-50) */
    /* Optional "rows nobody ever touched" shortcut for ONE row-structured tensor (the 30522 x 768 word table: at most B*W of its
     * rows receive a gradient per step, 15 % of all parameters).  row_flags[r] != 0 <=> row r of segment flag_seg has ever held a
     * non-zero gradient, moment or second moment (kept by univl_rows_append; the host sets every flag where it cannot know).  A
     * chunk of that segment whose rows are all unflagged has g = m = v = 0 exactly, so its BertAdam update is p -= lr * (wd * p)
     * -- the same bits the full formula gives (0 / (sqrt(0) + e) = 0) at 10 instead of 30 bytes per parameter.  The segment's
     * chunks must start on row boundaries.  NULL: off. */
    const uint8_t* row_flags; int32_t flag_seg; int32_t row_len;
    void* p16_lo;                /* optional: lo half of the shadow pair, bf16(p - bf16(p)), same offsets (UnivlGemm.B_lo)   */
} UnivlAdam;
int univl_bert_adam(const UnivlAdam* d, hipStream_t stream);
/* The same update over chunks [chunk_begin, chunk_begin + chunk_count) of the chunk table only; do_prep != 0 first runs the
 * per-tensor scalar kernel (once per step, before the first range).  max_blocks > 0 caps the grid (the kernel then walks
 * the range), which leaves compute units to kernels running concurrently on other streams: the pipelined training step
 * applies the update layer by layer next to the following forward pass (univl_amd/graphed.py). */
int univl_bert_adam_range(const UnivlAdam* d, int32_t chunk_begin, int32_t chunk_count, int32_t do_prep, int32_t max_blocks,
                          hipStream_t stream);
/* (Round 3: validated bit-exact against the sequential loop and the default of the captured step.)  A forward product (both operands K-major, bf16, 64 x 64 tiles) and chunks [chunk_begin, +chunk_count) of a
 * prepared BertAdam update (univl_bert_adam_range with do_prep ran before) in ONE launch: the update of step t rides with the
 * forward of step t + 1 (univl_amd/graphed.py).  Products the kernel does not carry are launched the ordinary way, followed by
 * the chunk range as its own launch -- same result.  max_blocks > 0 caps the workgroups given to the update. */
int univl_gemm_rider(const UnivlGemm* gemm, const UnivlAdam* adam, int32_t chunk_begin, int32_t chunk_count, int32_t max_blocks,
                     hipStream_t stream);
/* Round 5: the launch also carries products on the 64 x 128 tile (what univl_gemm picks from 1536 rows on).  Host-side question, no
 * device work: 1 if univl_gemm_rider carries chunks INSIDE this product's launch, 0 if it would enqueue the update behind the product
 * (the 128 x 128 and 256 x 256 tiles, transposed operands, fp32); negative: the descriptor's validation error.  A host spreads a
 * layer's chunks over the products that answer 1 (engine.EncoderStack.build_forward). */
int univl_gemm_rider_fits(const UnivlGemm* gemm);
/* K8 / K10 of the survey (module_bert.py:207-211, 246-250: dense -> dropout -> + input -> LayerNorm; the copies in module_visual.py /
 * module_cross.py): a forward product whose fp32 output is the input x of a LayerNorm, with that LayerNorm finished INSIDE the product's
 * launch -- each 64-row block of the output is normalised by the last workgroups to contribute to it (agent-scope release / acquire around
 * a per-block arrival counter), instead of by a second launch behind a kernel boundary.  Same arithmetic per row as univl_layernorm_fwd
 * (the same device function); the product's sums meet in hardware order exactly as in any split-K product, so the entry point refuses
 * deterministic mode.  Optionally also carries BertAdam chunks like univl_gemm_rider (adam may be NULL with chunk_count 0).
 *   gemm: bf16, both operands K-major, fp32 output C32 == ln->x with ldc = N = 768, no C16 / GELU / ACCUM / sumsq, at most 1024 rows
 *         (16 row blocks: the fold's last arrivals spin for the block's later ones, and the spinners must stay far below the resident slots);
 *   ln:   rows == gemm->M, N == 768, fp32 x, dtype bf16 (residual / dropout / y / stats / out32 / out16 as for univl_layernorm_fwd);
 *   counters: 2 * ceil(M / 64) int32 device words owned by this call site, ZERO before its first launch (the launch leaves them zero).
 * Returns UNIVL_EUNSUPPORTED for anything else (callers then enqueue univl_gemm / univl_gemm_rider + univl_layernorm_fwd);
 * dry_run != 0 validates without launching. */
int univl_gemm_ln(const UnivlGemm* gemm, const UnivlLayerNorm* ln, int32_t* counters, const UnivlAdam* adam, int32_t chunk_begin,
                  int32_t chunk_count, int32_t max_blocks, int32_t dry_run, hipStream_t stream);
/* The backward twin: univl_gemm_pair whose dgrad product's fp32 output is the upstream gradient of a LayerNorm backward (ln->dout ==
 * dgrad->C32, e.g. the FFN1 dgrad in front of BertSelfOutput's LayerNorm, module_bert.py:207-211 differentiated), with that LayerNorm
 * backward (dx32 / dxd16 rows, dgamma / dbeta / dbias column sums) finished inside the launch by the dgrad's last workgroups per 64-row
 * block.  At most 1024 rows (the rectangular dgrad body of 384+ rows only beside a 128 x 64 weight-gradient body), N = 768, C32 pre-zeroed (the dgrad's contributions become fp32 atomics), no position
 * rows (ln->dpos NULL); counters as for univl_gemm_ln; UNIVL_EUNSUPPORTED otherwise and in deterministic mode. */
int univl_gemm_pair_ln(const UnivlGemm* dgrad, const UnivlGemm* wgrad, const UnivlLayerNorm* ln, int32_t* counters, int32_t dry_run,
                       hipStream_t stream);
/* Large-LDS opt-in of the rider kernels on the stream's device; call once outside any stream capture before the first captured rider. */
int univl_gemm_rider_prime(hipStream_t stream);
/* *ctr += 1 (device word; used for per-replay dropout seeds) */
int univl_bump_counter(uint64_t* ctr, hipStream_t stream);
/* p16 <- bf16(p) over n elements */
int univl_cast_bf16(const float* p, void* p16, int64_t n, hipStream_t stream);
/* the shadow PAIR: p16 <- bf16(p), p16_lo <- bf16(p - p16) over n elements (p16 may be NULL: only the lo half is written) */
int univl_cast_bf16_pair(const float* p, void* p16, void* p16_lo, int64_t n, hipStream_t stream);
/* p <- fp32(p16) over n elements (the bf16 gradient exchange brings its buckets back into the fp32 gradient buffer) */
int univl_cast_f32(const void* p16, float* p, int64_t n, hipStream_t stream);

/* ------------------------------------------------------------------------------------- hardware probes */
int univl_probe_layouts(float* out, int32_t n_out, hipStream_t stream);
/* Measurement node: *out = the device's constant-rate wall clock (wall_clock64, 100 MHz on gfx950) when a one-thread kernel enqueued on
 * `stream` runs.  Placed between the nodes of a captured step it gives GPU-side start / end times of the step's branches WITHOUT a
 * profiler attached (scripts/probe_branches.py: rocprofv3 changes how the two branches of the step graph overlap). */
int univl_stamp(uint64_t* out, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
