/*
 * teal_hip.h — C ABI of libteal_hip.so, the MI355X (gfx950) implementation of TEAL's
 * activation-sparsity decode hot path.
 *
 * Every entry point replaces one piece of the reference's Triton path; citations are
 * into the reference tree (FasterDecoding/TEAL @ 2024-10-22):
 *
 *   teal_sparse_gemv       <- kernels/sparse_gemv.py:87-142  splitk_sparse_gemv()  + :50-83 kernel
 *                             (+ the init_to_zero("Y") pre-hook launch, :8-12, which disappears)
 *   teal_sparse_qkv_gemv   <- kernels/sparse_gemv.py:196-237 qkv_gemv()            + :152-194 kernel
 *   teal_compact           <- kernels/sparse_gemv.py:75      idx = tl.abs(x0) > threshold
 *                             (exposed standalone so index sets can be tested bit-exactly)
 *   teal_dense_gemv        <- kernels/sparse_gemv.py:301-307 DenseGEMV / torch.matmul(x, W.T) at S == 1
 *   teal_sparse_gateup_silu <- gpt-fast/model.py:258-259       silu(gemv1(x, w1)) * gemv1(x, w3)
 *   teal_fused_gemv        <- gpt-fast/model.py:158-161,289-291 residual adds + RMSNorm, :258-259 silu * up,
 *                             folded into the GEMV launch as producers
 *   teal_decode_attention* <- gpt-fast/model.py:170-186       RoPE, kv_cache.update, SDPA at S == 1
 *                             (TEAL_OUT_QKV_ROPE + teal_decode_attention_split_roped: RoPE and the cache append in the wqkv
 *                             projection's epilogue, :170-178, SDPA in the attention launch)
 *   teal_sample_topk       <- gpt-fast/generate.py:49-66      logits_to_probs + multinomial_sample_one
 *   teal_sparse_qkv_gemv_i8 <- gpt-fast/quantize.py:339-357   WeightOnlyInt8Linear.forward on the masked x
 *   teal_sparse_qkv_gemv_i4 <- gpt-fast/quantize.py:58-162,483-526 group-quantised int4 linear on the masked x
 *   teal_cmp_flag_gemv     <- scripts/benchmark_gemv.py:32-107,170-172 the Deja Vu comparator of the kernel benchmark
 *   teal_prefill_*         <- kernels/sparse_gemv.py:271,298 (dense matmul when S > 1) + gpt-fast/model.py:107-121,158-186,258-259:
 *                             the prompt pass of a short prompt, counted by the reference's tokens/sec (generate.py:458,487-496)
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types, no exceptions across the boundary.
 *   - All pointers are DEVICE pointers owned by the caller (PyTorch); the library borrows them for
 *     the duration of the stream-ordered launch and never allocates.  Library state: the properties of each device,
 *     cached the first time it is used (teal_init(); immutable), and a host-side registry of the workspaces prepared by
 *     teal_workspace_init() (which device memory holds a valid header; mutex-protected).  Nothing else: no entry point
 *     of libteal_hip.so changes how a later call behaves, and what a call did is reported through its own arguments
 *     (teal_gemv_out_t.desc).  The tuning / phase-stamp switches of the last section exist only in the DIAGNOSTICS
 *     build of the same sources, libteal_hip_diag.so (-DTEAL_DIAGNOSTICS), which the product path never loads.
 *     No device memory belongs to the library: the arrival counters of the single-launch split-K GEMVs and the scratch of the
 *     multi-workgroup sampler live in the header of the CALLER's workspace, so two streams, two captured graphs or two
 *     devices can only collide if the caller hands them the same workspace.
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream).  Every call is
 *     asynchronous, allocation-free and hipGraph-capture safe.
 *   - dtype: 0 = fp16, 1 = bf16 (x, weights and y share it; int8 weights carry scales in that dtype).
 *   - Weight layout: the reference's "column major" weight[N, Z] with strides (1, N), i.e. the
 *     memory image is W^T row-major [Z][N]: element (m, n) at wT[m * N + n]
 *     (kernels/sparse_gemv.py:68,106).  N % 8 == 0 (16-byte rows), 1 <= Z <= 65536.
 *   - Keep rule: row m is kept iff float32(|x[m]|) > float32(tau)  (strict; kernels/sparse_gemv.py:75).
 *     In the GEMV entry points a NaN x[m] additionally propagates NaN into every output column of its
 *     threshold group, as the reference's `0 * NaN` on masked rows does.
 *   - Arithmetic: fp32 multiply-accumulate over the kept rows, ONE rounding to dtype at the end
 *     (the reference rounds through fp16 atomics, kernels/sparse_gemv.py:83); no atomics, results are
 *     bit-reproducible run to run.
 *   - Return value: 0 on success, negative TEAL_ERR_* otherwise (teal_strerror()).
 */
#ifndef TEAL_HIP_H
#define TEAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TEAL_OK 0
#define TEAL_ERR_ARG (-1)       /* null pointer / non-positive size */
#define TEAL_ERR_DTYPE (-2)     /* dtype not 0 (fp16) / 1 (bf16) */
#define TEAL_ERR_SHAPE (-3)     /* N % 8 != 0, Z > 65536, bad N_q / N_kv */
#define TEAL_ERR_ALIGN (-4)     /* pointer not 16-byte aligned */
#define TEAL_ERR_WORKSPACE (-5) /* workspace too small (teal_workspace_bytes) */
#define TEAL_ERR_LAUNCH (-6)    /* hipGetLastError() after the launch */
#define TEAL_ERR_NO_DEVICE (-7) /* no HIP device / teal_init failed */
#define TEAL_ERR_CONFIG (-8)    /* invalid tuning override */

#define TEAL_F16 0
#define TEAL_BF16 1

int teal_version(void);
const char* teal_strerror(int code);

/* Cache the immutable properties of the CURRENT device (CU count, per-kernel attributes).  Call once per device
 * before any launch that may happen during stream capture (every entry point does it lazily otherwise).  Returns the
 * CU count (> 0) or a negative error. */
int teal_init(void);

/* Bytes of workspace a GEMV with N output columns may need: the library's header (arrival counters, sampler scratch)
 * plus an upper bound of the fp32 split-K slabs over all launch geometries (the deepest split x two N-column
 * segments).  Does not depend on Z — accepted for symmetry with the GEMV entry points.  The caller allocates once and
 * reuses; distinct streams need distinct workspaces. */
size_t teal_workspace_bytes(int Z, int N);

/* Prepare a workspace: zero its header (asynchronously on `stream`) and remember the pointer.  Once per allocation,
 * before the first launch that uses it and not under stream capture.  A prepared workspace lets a split-K GEMV with a
 * rounded output run as ONE launch (per-tile arrival tickets; the last slice to arrive sums the partials in slice
 * order) and a large-vocabulary sampler as several workgroups; every launch re-arms what it used, so a graph that was
 * captured with the workspace can be replayed indefinitely.  An unprepared workspace (plain memory of
 * teal_workspace_bytes) is still valid everywhere: 16-bit weights give the SAME bits from GEMV + ordered reduce launch (the
 * same slices summed in the same order) and the sampler the same tokens from a single workgroup; int8 / int4 weights pick
 * their split-K factor by whether tickets are available, so there the two ways agree to the tolerance of the fp32
 * summation order (one ulp of the 16-bit output), not bit for bit.  If a launch is aborted (device reset), prepare again.  teal_workspace_release() forgets the
 * pointer; call it before freeing the memory. */
int teal_workspace_init(void* ws, size_t ws_bytes, void* stream);
int teal_workspace_release(void* ws);

/* idx_out[0..count) = ascending m with float32(|x[m]|) > float32(tau); *count_out = count.
 * idx_out must hold Z int32.  (kernels/sparse_gemv.py:75) */
int teal_compact(const void* x, float tau, int Z, int dtype, int32_t* idx_out, int32_t* count_out,
                 void* stream);

/* y[n] = sum_{m kept} wT[m*N + n] * x[m]            (kernels/sparse_gemv.py:87-142) */
int teal_sparse_gemv(const void* x, const void* wT, void* y, float tau, int Z, int N, int dtype,
                     void* ws, size_t ws_bytes, void* stream);

/* Same on the fused wqkv weight with a threshold per column range:
 * columns [0,N_q) tau_q, [N_q,N_q+N_kv) tau_k, [N_q+N_kv,N) tau_v   (kernels/sparse_gemv.py:196-237;
 * N_q = N - 2*kv_size, N_kv = kv_size there).  N_q and N_kv must be multiples of 8. */
int teal_sparse_qkv_gemv(const void* x, const void* wT, void* y, float tau_q, float tau_k,
                         float tau_v, int Z, int N, int N_q, int N_kv, int dtype, void* ws,
                         size_t ws_bytes, void* stream);

/* Same with an explicit row stride `ld >= N` (elements, multiple of 8) of the W^T image, i.e. weight[N, Z]
 * with strides (1, ld).  A stride that is NOT a multiple of 1024 bytes (ld = N + 64) makes consecutive
 * rows start in different 128-byte DRAM-channel residues, so a workgroup's column tile rotates over all
 * channels instead of hammering one. */
int teal_sparse_qkv_gemv_ld(const void* x, const void* wT, int ld, void* y, float tau_q, float tau_k,
                            float tau_v, int Z, int N, int N_q, int N_kv, int dtype, void* ws,
                            size_t ws_bytes, void* stream);

/* int8 weight-only variant of teal_sparse_qkv_gemv_ld (the reference ships int8 only for its
 * dense path, gpt-fast/quantize.py:339-357, and lists quantised TEAL as missing, README.md:110).  wqT = int8 image of
 * W^T, row-major [Z][ld] bytes (ld % 8 == 0, ld >= N); scale[N] in the activation dtype.  N_kv = 0, N_q = N: one
 * threshold (tau_q). */
int teal_sparse_qkv_gemv_i8(const void* x, const void* wqT, const void* scale, void* y, float tau_q, float tau_k,
                            float tau_v, int Z, int N, int N_q, int N_kv, int ld, int dtype, void* ws, size_t ws_bytes,
                            void* stream);

/* y = x @ W^T with every row kept (prefill-free decode of un-sparsified layers, e.g. lm_head).
 * (kernels/sparse_gemv.py:301-307) */
int teal_dense_gemv(const void* x, const void* wT, void* y, int Z, int N, int dtype, void* ws,
                    size_t ws_bytes, void* stream);

/* int4 group-quantised weight-only variant (the reference ships int4-g32/64/128/256 for its dense
 * path only: gpt-fast/quantize.py:58-162 group q-params / quantise / dequantise, :483-526 WeightOnlyInt4Linear over a
 * CUDA-only packed layout).  w[n][m] = (q - 8) * scale[m / G][n] + zero[m / G][n], q in 0..15.
 *   wq               nibble image of W^T by ROW PAIRS: [Z / 2][ldb] BYTES (ldb >= N, ldb % 8 == 0, 8-byte aligned; for speed
 *                    ldb % 128 == 0 and a 128-byte aligned base, so that a tile's 128-byte segment is ONE memory line); the
 *                    32-bit word g of pair-row p holds columns 4g .. 4g+3 of row 2p in its low half (nibble j = column
 *                    4g + j) and of row 2p + 1 in its high half — two rows of a column unpack into one half2 for a packed
 *                    dot product; a pair is fetched when either of its rows is kept
 *   scales_and_zeros bf16 [Z / G][N][2] = {scale, zero}, exactly the reference's tensor (quantize.py:79-93)
 * N, N_q, N_kv multiples of 128; Z a multiple of G; x / y fp16 or bf16 (dtype).  N_kv = 0, N_q = N: one threshold.
 * One launch (split-K over 32-row units folded in by arrival tickets); fp32 accumulation, scale / zero applied once per
 * (unit, column), one rounding. */
int teal_sparse_qkv_gemv_i4(const void* x, const void* wq, const void* scales_and_zeros, void* y, float tau_q, float tau_k,
                            float tau_v, int Z, int N, int N_q, int N_kv, int ldb, int groupsize, int dtype, void* ws,
                            size_t ws_bytes, void* stream);

/* ---- fusions around the path ------------------------------------------ */

/* h[n] = silu(gate[n]) * up[n] with gate = sparse_gemv(x, w1T, tau_gate), up = sparse_gemv(x, w3T,
 * tau_up), both [Z][N]; gate/up are rounded to dtype before the activation and the product, as the
 * unfused reference sequence does (gpt-fast/model.py:258-259).  One launch, one shared read of x. */
int teal_sparse_gateup_silu(const void* x, const void* w1T, const void* w3T, void* h, float tau_gate,
                            float tau_up, int Z, int N, int dtype, void* ws, size_t ws_bytes,
                            void* stream);

/* ---- fused decode step: producers/consumers folded into the GEMV launch - */

#define TEAL_IN_PLAIN 0      /* x given as is */
#define TEAL_IN_RESID_NORM 1 /* x = RMSNorm(resid + round(sum slabs)) * w   (model.py:158-161, 289-291) */
#define TEAL_IN_SILU_MUL 2   /* x = silu(gate) * up, gate|up contiguous [2Z] (model.py:258-259) */
#define TEAL_IN_MASKED 3     /* x given together with its keep masks (one uint64 per 64 elements, bit i =
                              * element 64*c+i kept) as emitted by the producing launch: the consumer skips
                              * the compare/ballot phase.  The masks must be those of tau[0]. */
#define TEAL_IN_ATTN_MERGE 4 /* x = attention output merged from the split-KV partials per head written by
                              * teal_decode_attention_split(y = NULL, nsplit = 4 or 8): x points at the fp32
                              * partials [Z/head_dim][nsplit][head_dim + 2]; att_head_dim = head_dim,
                              * att_nsplit = nsplit (0 means 4); Z <= 16384 (nsplit 4) / 8192 (nsplit 8).  A split whose
                              * weight is zero (an empty split: sum == 0) is skipped whatever its o holds, as in the merge launch */
#define TEAL_OUT_ROUNDED 0   /* y rounded to dtype (runs the ordered slab reduce when split-K is used) */
#define TEAL_OUT_SLABS 1     /* leave the fp32 split-K slabs for the next launch's RESID_NORM producer.
                              * Which rows slab k (of *nslabs_out = split) sums — part of the ABI: both kernels follow it, and so
                              * does the partial that a TEAL_OUT_ROUNDED / TEAL_OUT_SLAB_SUM launch folds in slice order.  The
                              * vector is cut into chunks of 64 activations, chunk c = elements 64 c .. 64 c + 63; a round is 16
                              * chunks.  While split <= the vector's rounds (ceil(ceil(Z / 64) / 16)) and a slice's lists fit
                              * the LDS (always, for the lean kernel):
                              *   element-wise producers (PLAIN, SILU_MUL, MASKED, ATTN_MERGE): chunk c belongs to slice c mod
                              *     split (and, inside its workgroup, to wave (c div split) mod 16);
                              *   RESID_NORM (every workgroup holds the whole vector, wave w the chunks w + 16 k): chunk
                              *     w + 16 k belongs to slice (k + w) mod split.
                              * Otherwise (general kernel only: more slices than rounds, or lists beyond the LDS) the kept rows
                              * of a column tile form ONE ascending list of `total` entries and slice k sums entries
                              * [total * k / split, total * (k + 1) / split) (integer division).
                              * Slab k holds the fp32 sum of its kept rows only; a slice that keeps nothing writes +0.0.
                              * int4 weights (weight_bits = 4) cut the vector into UNITS of 32 activations instead, unit u =
                              * elements 32 u .. 32 u + 31, whatever the producer: unit u belongs to slice u mod split and,
                              * inside its workgroup, to wave (u div split) mod 16, so a wave's j-th unit is
                              * slice + split * (wave + 16 j); a wave walks its units in passes of 2 (when it owns at most two)
                              * or 4 consecutive j.  Scale and zero of unit u are those of group (32 u) div groupsize. */
#define TEAL_OUT_QKV_ROPE 3  /* nseg == 3 = q | k | v of ONE fused wqkv image, RESID_NORM input: when the launch needs no
                              * split-K (and the lean kernel takes it: *nslabs_out = 0), its epilogue applies RoPE to q and
                              * to the new k row and appends k, v to the caches (gpt-fast/model.py:170-178): y[0] = rotated
                              * q [ncols[0]], rounded exactly as teal_decode_attention* would have; follow it with
                              * teal_decode_attention_split_roped.  Otherwise (*nslabs_out >= 1) the launch behaved as
                              * TEAL_OUT_SLABS (slabs required) and teal_decode_attention_split_slabs finishes the job */
#define TEAL_OUT_SLAB_SUM 4  /* nseg == 1: `slabs` (plain memory, fp32 [ncols]) receives the UNROUNDED sum over the row slices,
                              * added in slice order by the last slice of each tile to arrive (arrival tickets: `ws` must be a
                              * prepared workspace when the launch uses split-K) — bit-identical to summing the TEAL_OUT_SLABS
                              * slabs in slice order.  *nslabs_out = 1; the consumer is a RESID_NORM producer with nslabs = 1,
                              * slabs_interleaved = 0.  Tensor parallelism: the [ncols] fp32 vector is what the ranks all-reduce
                              * (gpt-fast/tp.py:120-121,139-140) instead of [ncols][4..8] slabs.  16-bit and int8 weights; shapes
                              * outside the lean kernel return TEAL_ERR_CONFIG without launching */
#define TEAL_OUT_PAIR_SILU 2 /* nseg == 2 (gate, up of equal shape): every workgroup streams the same column tile
                              * of both matrices and stores h = silu(gate) * up to y[0] (model.py:258-259); optional
                              * mask_out[ncols/64] = keep masks of h against mask_tau for a TEAL_IN_MASKED consumer */

typedef struct teal_gemv_in {
    int mode;                 /* TEAL_IN_* */
    const void* x;            /* PLAIN: [Z];  SILU_MUL: gate[Z] followed by up[Z] */
    const void* resid_in;     /* RESID_NORM: residual stream [Z] (or a [rows][Z] table with row_index) */
    const int32_t* row_index; /* RESID_NORM, optional: device int32; row = row_index[0] (embedding lookup) */
    const float* slabs;       /* RESID_NORM, optional: fp32 [nslabs][Z] partial sums folded into the residual */
    int nslabs;
    const void* norm_weight;  /* RESID_NORM: RMSNorm weight [Z] */
    float eps;
    void* resid_out;          /* RESID_NORM, optional: updated residual [Z]; must not alias resid_in */
    const void* masks;        /* MASKED: uint64 [ceil(Z/64)] keep masks of x */
    int att_head_dim;         /* ATTN_MERGE: head_dim */
    int att_nsplit;           /* ATTN_MERGE: partials per head, 4 or 8 (0 = 4) */
    int slabs_interleaved;    /* RESID_NORM: slabs are [Z][(nslabs+3)&~3] (as written by a producer with
                               * slabs_interleaved = 1) instead of planar [nslabs][Z]; nslabs <= 8 */
    int gate_activated;       /* SILU_MUL: the gate half already holds round(silu(gate)) — written by a launch with
                               * act_seg0 = 1 — so x = round(gate * up): the same roundings as the unfused sequence
                               * (model.py:258-259), the activation computed once per column instead of in every consumer
                               * workgroup's prologue.  16-bit and int8 weights (not the int4 kernel) */
} teal_gemv_in_t;

typedef struct teal_gemv_out {
    int nseg;            /* 1..3 column segments, each with its own threshold (q|k|v, gate|up, ...) */
    const void* w[3];    /* weight image of the segment: row-major [Z][ld] */
    int ld[3];           /* row stride (elements) */
    int col0[3];         /* first column of the segment inside a row */
    int ncols[3];        /* columns in the segment */
    float tau[3];        /* keep threshold of the segment */
    void* y[3];          /* ROUNDED: output of the segment [ncols] */
    int mode;            /* TEAL_OUT_* */
    float* slabs;        /* SLABS: destination, fp32 [nslabs][sum ncols]; plain memory, NOT a prepared workspace */
    size_t slabs_bytes;
    void* mask_out;      /* PAIR_SILU, optional: uint64 [ceil(ncols/64)] keep masks of h */
    float mask_tau;      /* PAIR_SILU: threshold of the consumer (the down projection) */
    int slabs_interleaved; /* SLABS: write slabs[col][slice] with row stride (nslabs+3)&~3 so that the consumer
                            * fetches every partial of an element with one 16-byte load */
    int weight_bits;       /* 0 or 16: fp16/bf16 weights (the activation dtype); 8: int8 weight-only quantisation
                            * (gpt-fast/quantize.py:339-357): w[i] = int8 image of W^T, row-major [Z][ld] BYTES, and
                            * scale[i] = per-output-column scales in the activation dtype (element 0 = column col0[i]);
                            * y = round(fp32(sum q*x) * fp32(scale)) — one rounding, where the reference's
                            * F.linear(x, w.to(dtype)) * scales rounds twice */
    const void* scale[3];  /* int8: see above.  int4 (weight_bits = 4, gpt-fast/quantize.py:58-162, 483-526): w[i] = packed image
                            * of W^T by row pairs, [Z / 2][ld BYTES] (see teal_sparse_qkv_gemv_i4); scale[i] = the
                            * reference's scales_and_zeros tensor of that image, bf16 [Z / groupsize][scale_ld[i]][2]; col0
                            * addresses both.  ncols multiples of 128; in modes PLAIN, RESID_NORM (interleaved slabs, <= 8),
                            * SILU_MUL, ATTN_MERGE; out modes ROUNDED and SLABS */
    int scale_ld[3];       /* int4 only: columns per group row of scale[i] (the image's N) */
    int groupsize;         /* int4 only: 32, 64, 128 or 256 rows per quantisation group; Z a multiple */
    /* TEAL_OUT_QKV_ROPE only (zero otherwise): */
    const void* rope;          /* (cos, sin) table [rope_max_seq][rope_head_dim / 2][2], activation dtype */
    const int32_t* rope_pos;   /* device int32: position of the token being decoded (clamped to the cache) */
    void* k_cache;             /* [ncols[1] / rope_head_dim][rope_max_seq][rope_head_dim] */
    void* v_cache;
    int rope_head_dim;         /* 64 or 128 */
    int rope_max_seq;
    int act_seg0;              /* TEAL_OUT_ROUNDED: y[0] = round(silu(round(sum))) for segment 0 (the gate projection of an
                                * unpaired gate | up launch, model.py:258); the other segments are stored as usual.  16-bit
                                * and int8 weights (not the int4 kernel) */
    char* desc;                /* optional HOST buffer: receives the kernel template instantiation and grid of the launch THIS
                                * call made, NUL-terminated (as rocprofv3 prints it; e.g. to name the kernel in a benchmark
                                * record) — per call, no library state */
    int desc_bytes;            /* capacity of desc (160 is enough) */
} teal_gemv_out_t;

/* One launch: [fused producer] -> mask + compaction -> gathered GEMV over every segment.
 * *nslabs_out receives the split-K factor used (the number of slabs written in SLABS mode). */
int teal_fused_gemv(const teal_gemv_in_t* in, const teal_gemv_out_t* out, int Z, int dtype, void* ws,
                    size_t ws_bytes, int* nslabs_out, void* stream);

/* Single-token attention between gemv1 and gemv2 (gpt-fast/model.py:170-186): RoPE(q, k_new) with the
 * (cos, sin) table rope[max_pos][head_dim/2][2], KV-cache append at *pos, softmax(q K^T / sqrt(d)) V.
 * qkv = [q | k | v] as produced by the fused wqkv GEMV; caches are [n_kv_head][max_seq][head_dim];
 * y = [n_head * head_dim].  head_dim 64 or 128.  A position >= max_seq is clamped to the last cache slot (no
 * out-of-bounds write; the output of such a step is meaningless). */
int teal_decode_attention(const void* qkv, const void* rope, const int32_t* pos, void* k_cache, void* v_cache,
                          void* y, int n_head, int n_kv_head, int head_dim, int max_seq, int dtype, void* stream);

/* Same, also emitting the keep masks of y against mask_tau (uint64 [n_head*head_dim/64]) for a
 * TEAL_IN_MASKED wo projection. */
int teal_decode_attention_masked(const void* qkv, const void* rope, const int32_t* pos, void* k_cache, void* v_cache,
                                 void* y, void* mask_out, float mask_tau, int n_head, int n_kv_head, int head_dim,
                                 int max_seq, int dtype, void* stream);

/* Long-context form (flash-decoding): the cached positions of every head are split over `nsplit` workgroups
 * that write un-normalised partials {max, sum, o[head_dim]} (fp32, n_head*nsplit*(head_dim+2) floats), then
 * a merge launch rescales, sums, rounds once and emits the masks.  Use when max_seq is in the thousands:
 * one workgroup per head would leave most CUs idle while n_head of them stream the whole KV cache.
 * nsplit <= 64.  Grouped-query shapes (n_head / n_kv_head = 8 with max_seq >= 2048, = 4 with max_seq >= 4096) run as ONE workgroup per
 * (KV head, split) that serves all query heads of the group, so every K/V row is read once instead of once per query
 * head; choose nsplit so that n_kv_head * nsplit is about the CU count (32 for 8 KV heads).  Same partial format. */
int teal_decode_attention_split(const void* qkv, const void* rope, const int32_t* pos, void* k_cache, void* v_cache,
                                void* y, void* mask_out, float mask_tau, int n_head, int n_kv_head, int head_dim,
                                int max_seq, int nsplit, void* partials, size_t partials_bytes, int dtype, void* stream);
/* Same, with the qkv projection taken from the fp32 split-K slabs of a TEAL_OUT_SLABS launch (slabs_interleaved = 1,
 * layout [col][(nslabs + 3) & ~3], nslabs <= 8): the kernel sums each element's partials in slice order and rounds
 * once — exactly what the ordered reduce launch would have written — so a narrow (GQA) wqkv can be row-sliced over
 * all CUs without a reduce launch between projection and attention. */
int teal_decode_attention_split_slabs(const float* qkv_slabs, int qkv_nslabs, const void* rope, const int32_t* pos,
                                      void* k_cache, void* v_cache, void* y, void* mask_out, float mask_tau, int n_head,
                                      int n_kv_head, int head_dim, int max_seq, int nsplit, void* partials,
                                      size_t partials_bytes, int dtype, void* stream);
/* General form: exactly one of qkv (rounded projection) / qkv_slabs (+ qkv_nslabs) is given.  Same launches and results as
 * teal_decode_attention_split / _split_slabs.  `ws` / `ws_bytes` are accepted and unused (round 3 folded the merge launch into
 * the split launch through arrival counters in a prepared workspace: bit-identical y, measured no faster — equal at 4-8
 * splits, slower at 16-32 — and removed in round 5). */
int teal_decode_attention_split_ws(const void* qkv, const float* qkv_slabs, int qkv_nslabs, const void* rope,
                                   const int32_t* pos, void* k_cache, void* v_cache, void* y, void* mask_out,
                                   float mask_tau, int n_head, int n_kv_head, int head_dim, int max_seq, int nsplit,
                                   void* partials, size_t partials_bytes, int dtype, void* ws, size_t ws_bytes, void* stream);
/* After a TEAL_OUT_QKV_ROPE projection that reported *nslabs_out = 0: q = the rotated, rounded query [n_head * head_dim];
 * the token's k / v rows are already in the caches.  Always the per-query-head split kernel (no grouped-query form); same
 * partials, merge and results as teal_decode_attention_split_ws. */
int teal_decode_attention_split_roped(const void* q, const int32_t* pos, const void* k_cache, const void* v_cache, void* y,
                                      void* mask_out, float mask_tau, int n_head, int n_kv_head, int head_dim, int max_seq,
                                      int nsplit, void* partials, size_t partials_bytes, int dtype, void* ws, size_t ws_bytes,
                                      void* stream);
/* y == NULL: only the partials are written (no merge launch); with nsplit 4 or 8 a TEAL_IN_ATTN_MERGE wo
 * projection merges them in its own prologue (nsplit 4 or 8) — one launch less per layer, and 4 CUs per head pull the KV
 * cache instead of one (a single CU sustains ~50 GB/s, which bounds the one-workgroup-per-head kernel). */

/* ---- fused top-k sampler, teal_amd/csrc/teal_sampler.hip --------------------------------------- */

/* Sampling step of the decode loop (gpt-fast/generate.py:49-66): logits / temperature, top-k filter
 * (ties at the pivot kept), softmax, exponential-race multinomial.  rng_state = device uint64[2]
 * {seed, draw counter}; the kernel bumps the counter so hipGraph replays draw fresh numbers.
 * top_k <= 0 or >= vocab disables the filter.  token_out = device int32[1] (may be the buffer the next
 * decode step reads its token from).  Optional in-graph loop-carried state, so that one graph replay
 * IS one decode step with no host-side glue: pos_inout[0] += 1; history[draw counter] = token.
 * teal_sample_topk_ws with a prepared workspace (teal_workspace_init): vocabularies of 8193..131072 entries (multiple
 * of 8) with an active filter run as one workgroup per 8192 logits: local top-k candidates -> workspace header -> the
 * last workgroup to arrive picks the token; same tokens as the single-workgroup kernels, which serve every other case
 * (no / unprepared workspace, other shapes). */
int teal_sample_topk(const void* logits, int vocab, int dtype, int top_k, float temperature, void* rng_state,
                     int32_t* token_out, int32_t* pos_inout, int32_t* history, int history_len, void* stream);
int teal_sample_topk_ws(const void* logits, int vocab, int dtype, int top_k, float temperature, void* rng_state,
                        int32_t* token_out, int32_t* pos_inout, int32_t* history, int history_len, void* ws,
                        size_t ws_bytes, void* stream);


/* ---- dense prompt pass for short prompts (T <= 16 tokens), teal_amd/csrc/teal_prefill.hip ----- */

/* The reference's prefill is dense (its ops run torch.matmul when the sequence is longer than one token,
 * kernels/sparse_gemv.py:271,298; the rest is the stock model, gpt-fast/model.py:107-121,158-186,258-259,289-291) and its
 * tokens/sec counts it (gpt-fast/generate.py:458,487-496).  These entry points make one layer of that pass seven launches over
 * the decode step's own weight images.  Every hand-over is TRANSPOSED, [feature][R] with R = 8 for T <= 8 and R = 16 for
 * 9 <= T <= 16 (every call of one pass takes the same T, hence the same R; "[..][8]" below reads "[..][R]"): the tokens of a
 * feature in one or two 16-byte words (16-bit activations: xt, ht, yt) or R / 4 of them (fp32 slabs [slice][feature][R]); token
 * slots >= T of the 16-bit vectors are written as zero; of the slabs, which are written in token pairs, slot T of an odd T is zero (a
 * TEAL_PREFILL_IN_XT launch takes xt's slot T as given: zero from every producer here) and slots >= 2 * ceil(T / 2) are left
 * untouched (consumers ignore them).  1 <= T <= 16.
 * Floating-point results: fp32 sums, the rounding points of the module path's 16-bit tensors. */

/* What a GEMM launch builds its activations from (every workgroup builds the rows of its own slice, once, while staging them) */
#define TEAL_PREFILL_IN_XT 0        /* xt [Z][8] as given */
#define TEAL_PREFILL_IN_NORM 1      /* x = RMSNorm(h) * norm_w from the residual rows xt = ht [Z][8] and the per-workgroup sums of squares
                                     * sumsq [nwg][8] a teal_prefill_resid_norm call left in its scratch (nwg = Z / 256 rounded up) */
#define TEAL_PREFILL_IN_SILU_MUL 2  /* x = round(round(silu(round(gate))) * round(up)) from the slabs [gu_split][2 Z][8] of a gate | up launch */
typedef struct teal_prefill_in {
    int mode;
    const void* xt;
    const float* sumsq;
    int nwg;
    const void* norm_w;
    float eps;
    const float* gu_slabs;
    int gu_split;
} teal_prefill_in_t;

/* slabs[slice][n][s] = sum over the slice's rows m of W^T[m][n] * x[m][s]: w0T [Z][ld0] (n0 columns) and, optionally, w1T [Z][ld1]
 * (n1 columns, output columns n0 ..: gate | up in one launch).  Z, n0, n1 multiples of 256.  *split_out = slices written (<= 16;
 * the consumer sums them in slice order and rounds once); slabs must hold 16 * (n0 + n1) * R floats and must not be the buffer a
 * TEAL_PREFILL_IN_SILU_MUL launch reads. */
int teal_prefill_gemm(const teal_prefill_in_t* in, const void* w0T, int ld0, int n0, const void* w1T, int ld1, int n1, float* slabs,
                      size_t slabs_bytes, int Z, int T, int dtype, int* split_out, void* stream);
/* h = (embedding rows of tokens[0..T) | ht_in) + round(sum of `split` slabs) (split 0: nothing to add); x = RMSNorm(h) * norm_w.
 * Exactly one of tokens (+ emb [vocab][dim]) / ht_in is given; with neither xt_out nor x_last only the first of the two launches runs
 * (h and the sums of squares: a TEAL_PREFILL_IN_NORM GEMM normalises while it stages).  Outputs: ht_out [dim][8] (required; must not alias ht_in's
 * words of other columns — the same buffer is fine), xt_out [dim][8] and x_last [dim] (optional) = the normalised vector of
 * token T - 1 as a plain vector (input of the lm_head GEMV).  sumsq_scratch: (dim / 256 rounded up) * R floats of caller memory
 * (the per-workgroup sums of squares between the two launches this call makes).  dim <= 16384. */
int teal_prefill_resid_norm(const void* emb, const int32_t* tokens, int T, const void* ht_in, const float* slabs, int split,
                            const void* norm_w, float eps, int dim, void* ht_out, void* xt_out, void* x_last, float* sumsq_scratch,
                            int dtype, void* stream);
/* q | k | v from the slabs [split][(n_head + 2 n_kv_head) * head_dim][8] of the wqkv launch: RoPE(q, k) at positions 0 .. T-1,
 * cache rows 0 .. T-1 written, causal softmax(q K^T / sqrt(d)) V -> yt [n_head * head_dim][8].  head_dim 64 or 128. */
int teal_prefill_attention(const float* qkv_slabs, int split, const void* rope, void* k_cache, void* v_cache, void* yt, int T, int n_head,
                           int n_kv_head, int head_dim, int max_seq, int dtype, void* stream);

/* ---- speculative decoding: the dense verify pass and the accept step, teal_amd/csrc/teal_speculative.hip ---------- */

/* A round (gpt-fast/generate.py:98-217): k draft tokens d1 .. dk from the sparse decode step, then ONE dense prompt-pass-shaped
 * pass over the T = k + 1 tokens [x0, d1 .. dk] at positions p0 .. p0+k (teal_prefill_gemm / teal_prefill_resid_norm with this
 * attention), the lm_head of every row (teal_prefill_gemm over the column-major lm_head image), then teal_spec_accept. */

/* Bytes of `partials` teal_verify_attention may need (any cache length). */
size_t teal_verify_attention_ws_bytes(int T, int n_head, int head_dim);
/* q | k | v of T <= 16 tokens from the slabs [split][(n_head + 2 n_kv_head) * head_dim][R] of a teal_prefill_gemm launch: RoPE(q, k) at
 * positions p0 + t, cache rows p0 .. p0+T-1 written, query t attends causally to rows 0 .. p0+t -> yt [n_head * head_dim][R] (slots
 * >= T zero), the input of the wo GEMM.  p0 = *pos is read on the DEVICE (a captured round replays at any position), clamped to
 * [0, max_seq - T].  Split-KV over the context (every K / V row a workgroup loads serves all T x (n_head / n_kv_head) query rows
 * of its KV head) and a merge launch; the T new rows are rebuilt from the slabs by every workgroup that needs them — no row written
 * by the launch is read back by it.  head_dim 64 or 128, max_seq >= T.  Two launches. */
int teal_verify_attention(const float* qkv_slabs, int split, const void* rope, const int32_t* pos, void* k_cache, void* v_cache, void* yt,
                          float* partials, size_t partials_bytes, int T, int n_head, int n_kv_head, int head_dim, int max_seq, int dtype,
                          void* stream);

/* Bytes of `scratch` teal_spec_accept needs (the rounded target rows and per-row statistics). */
size_t teal_spec_accept_scratch_bytes(int vocab, int k);
/* The accept / reject step of one round, on the device (gpt-fast/generate.py:123-146).
 *   logit_slabs   [split][vocab][R] lm_head slabs of the T = k + 1 verified rows (teal_prefill_gemm, R = 8 for T <= 8 else 16): row t
 *                 is summed in slice order and rounded ONCE to 16 bits (the module path's logits) -> q_t
 *   draft_logits  [k][vocab] 16-bit: the draft's logits row that drew d_{i+1} -> p_i
 *   tokens        int32 [T]: tokens[0] = the round's input token x0, tokens[1 .. k] = d1 .. dk; tokens[0] <- the next round's input
 * Distributions: prob(v) = exp((x_v - max x) / temperature) / Z over the top_k largest logits (ties at the pivot kept; top_k <= 0 or
 * >= vocab: all) — the fused sampler's weights (teal_sample_topk), normalised.  With (seed, c) = rng_state[0], rng_state[1] at entry and
 * U(h) = ((h >> 8) + 0.5) / 2^24, hash3 as in the sampler:
 *   u_i      = U(hash3(seed, c, i)),  i < k
 *   accept d_{i+1} while p_i(d_{i+1}) > 0 and u_i <= min(1, q_i(d_{i+1}) / p_i(d_{i+1}))   (fp32); n = accepted count
 *   key_v    = U(hash3(seed, c + 1, v)),  v < vocab
 *   token    = argmax_v w_v / -log(key_v) (ties: lowest v), w = max(q_n - p_n, 0) if n < k (q_n if that is zero everywhere), else q_k
 *   rng_state[1] = c + 2.
 * Outputs: out_seq[*out_len ..] <- d1 .. dn, token (entries past out_cap dropped), *out_len += n + 1; *spec_pos += n + 1 and, if
 * given, *pos_out = the same (the draft engine's position); *n_acc = n and hist[n] += 1 if given.  vocab 8 .. 131072, a multiple of
 * 8; 1 <= k <= 15.  Three launches: round the target rows, per-row statistics (2k + 1 workgroups), the decision (one workgroup). */
int teal_spec_accept(const float* logit_slabs, int split, const void* draft_logits, int vocab, int k, int dtype, int top_k, float temperature,
                     void* rng_state, int32_t* tokens, int32_t* spec_pos, int32_t* pos_out, int32_t* out_seq, int out_cap, int32_t* out_len,
                     int32_t* n_acc, int32_t* hist, void* scratch, size_t scratch_bytes, void* stream);

/* ---- batched decode: up to 8 TEAL-sparse sequences per step, teal_amd/csrc/teal_batched.hip -------------------------- */

/* A step of B <= 8 sequences runs the prompt pass's chain (teal_prefill_resid_norm with T = B, the hand-over [feature][8]: slot b =
 * sequence b) with these GEMM and attention launches.  TEAL's rule per sequence: y_b = W (x_b * [float32(|x_b|) > float32(tau)]),
 * the mask taken on the 16-bit activation the module path holds. */

/* Threshold segments of one GEMM launch: column ranges [col_end[s - 1], col_end[s]) over the launch's n0 + n1 output columns
 * (col_end[-1] = 0, ascending, multiples of 8, col_end[nseg - 1] = n0 + n1), one tau each (q / k / v of wqkv; gate / up). */
typedef struct teal_batched_segs {
    int nseg;
    int col_end[3];
    float tau[3];
} teal_batched_segs_t;

/* slabs[slice][n][8] (fp32) = sum over the slice's rows m that sequence b keeps under its column's segment threshold of
 * W^T[m][n] * x_b[m], b < B <= 8; inputs, weights and the slab contract as teal_prefill_gemm (Z, n0, n1 multiples of 256).  Slots are
 * written in pairs: slots B .. 2 * ceil(B / 2) - 1 are exactly zero whatever the hand-over holds there, slots >= 2 * ceil(B / 2) and
 * the slabs of slices >= *split_out are left untouched (every consumer reads slots < B only; tests/test_exact_gemm_gpu.py pins
 * this).  Every weight row that some sequence keeps (the union) is read once; no other row is loaded.  counts (optional, int32
 * [16][3][9]): slice k's row counts under segment s — counts[k][s][b] rows kept by sequence b, counts[k][s][8] rows of the union —
 * written for slices k < *split_out (sum them over k; entries of absent segments are not written). */
int teal_batched_sparse_gemm(const teal_prefill_in_t* in, const teal_batched_segs_t* segs, const void* w0T, int ld0, int n0, const void* w1T,
                             int ld1, int n1, float* slabs, size_t slabs_bytes, int Z, int B, int32_t* counts, int dtype, int* split_out,
                             void* stream);
/* y[b][n] (16-bit, row stride N) = the `split` slabs [slice][N][8] of column n summed in slice order and rounded once, b < B. */
int teal_batched_round_rows(const float* slabs, int split, int N, int B, void* y, int dtype, void* stream);
/* Bytes of `partials` teal_batched_decode_attention may need (any cache length). */
size_t teal_batched_decode_attention_ws_bytes(int B, int n_head, int head_dim);
/* One decode token per sequence: q | k | v of sequence b from slot b of the wqkv slabs [split][(n_head + 2 n_kv_head) * head_dim][8],
 * RoPE at p_b = clamp(pos[b], 0, max_seq - 1) (pos: int32 [B] on the DEVICE, positions may differ), the K / V row p_b written to
 * sequence b's cache, attention over its rows 0 .. p_b -> yt [n_head * head_dim][8] (slots >= B zero).  Caches [B][n_kv_head][max_seq]
 * [head_dim] (setup_caches(max_batch_size=B)).  head_dim 64 or 128, GQA or MHA, B <= 8.  Two launches (split-KV, merge). */
int teal_batched_decode_attention(const float* qkv_slabs, int split, const void* rope, const int32_t* pos, void* k_cache, void* v_cache,
                                  void* yt, float* partials, size_t partials_bytes, int B, int n_head, int n_kv_head, int head_dim,
                                  int max_seq, int dtype, void* stream);

/* ---- continuous batching: slots that drop out of the batched step on the device, teal_amd/csrc/teal_batched.hip ------------
 * A slot is one running request.  The slot state is ONE int32 buffer of TEAL_SLOT_WORDS words per engine, at a fixed address (a
 * captured step holds it): TEAL_SLOT_ACTIVE (bit b: slot b runs), TEAL_SLOT_STEP (steps retired so far), and per slot b the words
 * TEAL_SLOT_BUDGET + b (tokens it may still produce), TEAL_SLOT_PRODUCED + b (tokens produced), TEAL_SLOT_EOS + b (EOS id, -1: none)
 * and TEAL_SLOT_FINISH + b (the step on which it stopped).  The host writes a slot's words between steps (admission) and reads
 * the whole buffer back in one copy. */
#define TEAL_SLOT_ACTIVE 0
#define TEAL_SLOT_STEP 1
#define TEAL_SLOT_BUDGET 8
#define TEAL_SLOT_PRODUCED 16
#define TEAL_SLOT_EOS 24
#define TEAL_SLOT_FINISH 32
#define TEAL_SLOT_WORDS 40

/* teal_batched_sparse_gemm with the slots whose bit of active[0] (device int32) is clear left out: read once per workgroup, such a
 * slot's activation is +0 (whatever its hand-over holds, NaN and Inf included) and never kept, so it adds nothing to the union,
 * to the kept counts or to any other slot's sums, and its slab columns are exactly 0.  On the active slots the results are
 * bit-identical to teal_batched_sparse_gemm of the compacted batch. */
int teal_batched_sparse_gemm_slots(const teal_prefill_in_t* in, const teal_batched_segs_t* segs, const void* w0T, int ld0, int n0,
                                   const void* w1T, int ld1, int n1, float* slabs, size_t slabs_bytes, int Z, int B, const int32_t* active,
                                   int32_t* counts, int dtype, int* split_out, void* stream);
/* teal_batched_sparse_gemm_slots with a threshold per slot: taus (device fp32 [3][8], segment-major and slot-minor, 32-byte
 * aligned) — slot b keeps row m under segment s iff its bit of active[0] is set and float32(|x_b[m]|) > taus[s][b].  segs->tau is
 * ignored; segs->col_end and nseg hold as before, rows of taus past nseg - 1 are not consulted.  Read once per workgroup together
 * with active[0].  An inactive slot's column is never consulted: whatever it holds (a finished request's level, NaN) changes
 * nothing.  The union, the dealing of rows, the sums' order and the counts are those of teal_batched_sparse_gemm_slots: with every
 * column equal to segs->tau the outputs are the same words.  taus null: TEAL_ERR_ARG; misaligned: TEAL_ERR_ALIGN. */
int teal_batched_sparse_gemm_slot_taus(const teal_prefill_in_t* in, const teal_batched_segs_t* segs, const void* w0T, int ld0, int n0,
                                       const void* w1T, int ld1, int n1, float* slabs, size_t slabs_bytes, int Z, int B,
                                       const int32_t* active, const float* taus, int32_t* counts, int dtype, int* split_out, void* stream);
/* teal_batched_decode_attention where the workgroups of a slot whose bit of active[0] is clear exit at once: no cache row written,
 * no partials, yt slot zero.  Same grid and nsplit as the unmasked launch at the same B (nsplit never depends on the active set). */
int teal_batched_decode_attention_slots(const float* qkv_slabs, int split, const void* rope, const int32_t* pos, const int32_t* active,
                                        void* k_cache, void* v_cache, void* yt, float* partials, size_t partials_bytes, int B, int n_head,
                                        int n_kv_head, int head_dim, int max_seq, int dtype, void* stream);
/* One launch after the B samplers of a step: every slot b < B that is active and in slot_mask counts its token (tokens[b]), spends
 * one unit of budget and stops — bit cleared, TEAL_SLOT_FINISH + b = the current step — when tokens[b] is its EOS id, when its
 * budget is spent, or when its next position pos[b] would be max_seq (pos[b] is then set to max_seq - 1: a slot's position never
 * passes the cache).  count_step != 0: TEAL_SLOT_STEP += 1 (the decode step; an admission's first draw passes 0). */
int teal_batched_retire(int32_t* slot_state, const int32_t* tokens, int32_t* pos, int B, int slot_mask, int max_seq, int count_step,
                        void* stream);
/* (teal_amd/csrc/teal_sampler.hip) teal_sample_topk_ws predicated on bit `slot` of active[0] (device int32): set, exactly
 * teal_sample_topk_ws; clear, nothing changes —
 * token, position, rng_state, history and the workspace's ticket and scratch stay as they were (every workgroup of the
 * multi-workgroup form exits before the ticket). */
int teal_sample_topk_slot(const void* logits, int vocab, int dtype, int top_k, float temperature, void* rng_state, int32_t* token_out,
                          int32_t* pos_inout, int32_t* history, int history_len, void* ws, size_t ws_bytes, const int32_t* active, int slot,
                          void* stream);

/* ---- token log-probabilities, teal_amd/csrc/teal_logprob.hip ---------------------------------------------------------------
 * For a row of `vocab` 16-bit logits l and a token t:  lp(t) = (l[t] - m) - log sum_v exp(l[v] - m),  m = max_v l[v],  in fp32
 * (expf / logf).  The MODEL's distribution: temperature 1, no top-k filter, whatever the sampler was told.  A logit of -inf
 * contributes 0; NaN logits, +inf logits and a row that is all -inf are outside the contract; a token outside 0 .. vocab-1 gives
 * NaN.  One workgroup per row, no workspace: a row's results depend only on that row's logits and token (not on B, the slot or
 * the other rows) and replays are bit-identical.
 * Both: vocab a multiple of 8 in 8..131072 (else TEAL_ERR_SHAPE); null required pointers TEAL_ERR_ARG; a row base (or, B > 1, a
 * stride) off 16 bytes TEAL_ERR_ALIGN; every check comes before any HIP call. */

/* One launch after the B samplers of a step (before teal_batched_retire).  Row r < B serves slot slot0 + r.
 *   c = rng_state[r][1]   (uint64 [B][2]: the draw counter the sampler has just bumped)
 *   i = c - 1
 *   t = tokens[r]
 * If 0 <= i < lp_len:
 *   lp[r * lp_len + i] = lp(t)
 *   if top_n > 0: top_ids / top_lp[(r * lp_len + i) * top_n + j], j < top_n, are the ids and logprobs of the top_n largest logits
 *     of the row, by descending logit, equal logits (-0 = +0) by ascending id.
 * Otherwise nothing is written.
 * active != NULL: a row whose bit (slot0 + r) of active[0] (device int32) is clear writes nothing.
 * logits_stride is in elements.  TEAL_ERR_ARG also: top_n outside 0..8 (top_ids / top_lp required when > 0), B outside 1..8,
 * slot0 < 0 or slot0 + B > 32, lp_len <= 0. */
int teal_token_logprobs(const void* logits, size_t logits_stride, int vocab, int dtype, int B, const int32_t* tokens,
                        const void* rng_state, float* lp, int lp_len, int top_n, int32_t* top_ids, float* top_lp,
                        const int32_t* active, int slot0, void* stream);
/* Teacher forcing: takes the sampler's place in a scoring loop (one graph replay = one position).
 *   p = pos_inout[0]
 *   j = p + 1
 * If 0 <= j < n_targets:
 *   t = targets[j]
 *   lp[j] = lp(t) from `logits`
 *   token_out[0] = t
 *   pos_inout[0] = j
 * Otherwise nothing changes, so replaying past the end is harmless. */
int teal_score_step(const void* logits, int vocab, int dtype, const int32_t* targets, int n_targets, int32_t* token_out,
                    int32_t* pos_inout, float* lp, void* stream);

/* ---- per-request logit processors, teal_amd/csrc/teal_logit_adjust.hip -----------------------------------------------------
 * One launch between a step's logits and its samplers: repetition, frequency and presence penalty and a logit bias, per row.
 * For element v of row r, with w = state[r][v] (bit 31: v occurs in the request's prompt; low 31 bits n: how often v was
 * generated), {theta, alpha_p, alpha_f, reserved} = params[r] and b = bias[r] (or no bias):
 *   x = float(logits[r][v])
 *   if w != 0:   x = x > 0 ? x / theta : x * theta
 *   if n > 0:    x = x - alpha_f * float(n);  x = x - alpha_p
 *   if bias:     x = x + float(b[v])
 *   out[r][v] = round-to-nearest-even(min(max(x, -MAXF), MAXF)),  MAXF = the dtype's largest finite value
 * every operation a separately rounded fp32 operation (no fused multiply-add).  `out` never holds an infinity: a logit of -inf
 * leaves as -MAXF.  NaN logits are outside the contract.  theta = 1, alphas 0, no bias: out equals logits as values (with a bias
 * row, -0 leaves as +0).
 * count_token != 0: before element t = tokens[r] is adjusted, the count of state[r][t] goes up by one (it stays at 2^31 - 1); a
 * token outside 0 .. vocab-1 counts nothing.  No other state word is written; no atomics, no workspace: replays are bit-identical.
 * Row r < B serves slot slot0 + r.  active != NULL: a row whose bit (slot0 + r) of active[0] (device int32) is clear changes
 * nothing — no count, its `out` row untouched.  state: int32 [B][vocab]; params: fp32 [B][4]; bias: [B][vocab] of the dtype, or
 * NULL; strides in elements.  `out` must not overlap `logits` (the logprob launch goes on reading the raw rows): TEAL_ERR_ARG.
 * vocab a multiple of 8 in 8..131072 (else TEAL_ERR_SHAPE); B outside 1..8, slot0 < 0, slot0 + B > 32 or a null required pointer
 * TEAL_ERR_ARG; TEAL_ERR_DTYPE; a row base (or, B > 1, a stride) off 16 bytes TEAL_ERR_ALIGN; every check comes before any HIP
 * call. */
int teal_logit_adjust(const void* logits, size_t logits_stride, int vocab, int dtype, int B, const int32_t* tokens, int count_token,
                      int32_t* state, const float* params, const void* bias, void* out, size_t out_stride, const int32_t* active,
                      int slot0, void* stream);

/* ---- per-request sampling, teal_amd/csrc/teal_sample_rows.hip -----------------------------------------------------------------
 * One launch in the place of a step's B teal_sample_topk* launches: row r < B (one workgroup each) draws a token from its row of
 * `vocab` 16-bit logits under its own four 32-bit words params[r] = {fp32 temperature, int32 top_k, fp32 top_p, fp32 min_p}, read
 * from device memory, so a captured launch serves any mix of settings.  The filters apply in this order:
 *   1. temperature   inv = 1 / max(temperature, 1e-5);  mx = the row's largest logit;  t_i = fl(fl(x_i - mx) * inv)
 *                    (fp32, one rounding per operation: what teal_sample_topk* compute).
 *   2. top_k         0 < top_k < vocab: every logit not below the top_k-th largest VALUE stays, ties at the pivot included; any
 *                    other top_k: no filter.  The surviving set is K1.  (teal_sample_topk*'s filter.)
 *   3. top_p         over K1, with w_i = exp(t_i), Z = the sum of w over K1 and A(v) = the mass of the members of K1 whose value is
 *                    strictly greater than v: a logit of value v stays iff A(v) < top_p * Z.  (The nucleus of the renormalised
 *                    top-k set, decided by value: equal logits stay or go together, the maximum always stays.)  top_p >= 1: no
 *                    filter, and no sum is formed.  top_p <= 0 or not finite is the caller's error.
 *   4. min_p         a logit stays iff exp(t_i) >= min_p: its probability is at least min_p times the largest one's (renormalising
 *                    does not change that ratio).  min_p == 0: no filter.  min_p outside [0, 1) is the caller's error.
 *   5. the race      among the logits that pass all three: argmax_i expf(t_i) / -logf(u_i), u_i = ((hash3(seed, ctr, i) >> 8) + 0.5)
 *                    / 2^24 — teal_sample_topk*'s fp32 expression and random stream, the smallest index winning exact ties; then
 *                    tokens[r] = token, history[r][c] = token if c < history_len (c: the draw counter before), the draw counter
 *                    goes up by one and pos[r] by one where `pos` is given.
 * Every filter has the form "value >= threshold" and the maximum passes all of them: the kept sets are nested, and kept_out[r]
 * (optional) — how many logits entered the race — identifies the set.  With top_p = 1 and min_p = 0 a row draws the very token
 * teal_sample_topk_slot draws from the same logits, temperature, top_k and rng state (bit-equal scores).
 * Rounding: the masses are summed as 64-bit fixed-point integers (trunc(expf(t_i) * 2^40)), A and Z are within about
 * (E + 2) * 2^-24 * Z of exact for an expf good to E ulps, and top_p * Z is formed in fp64; a decision closer than 1e-5 * Z to a
 * boundary (or, min_p, exp(t) within 1e-5 * min_p of min_p) may fall either way against exact arithmetic.  Integer sums do not
 * depend on their order: a row's token and kept count depend only on that row's logits, parameters and rng state — not on B, the
 * slot, the other rows or the replay.  NaN logits and a row that is all -inf are outside the contract.
 * Row r serves slot slot0 + r.  active != NULL: a row whose bit (slot0 + r) of active[0] (device int32) is clear changes nothing.
 * rng_state: uint64 [B][2] = {seed, draw counter}; tokens, pos (or NULL), kept_out (or NULL): int32 [B]; history: int32
 * [B][history_len] or NULL; logits_stride in elements.
 * vocab a multiple of 8 in 8..131072 (else TEAL_ERR_SHAPE); B outside 1..8, slot0 < 0, slot0 + B > 32, history_len < 0 with a
 * history or a null required pointer TEAL_ERR_ARG; TEAL_ERR_DTYPE; a row base (or, B > 1, a stride) off 16 bytes TEAL_ERR_ALIGN;
 * every check comes before any HIP call. */
int teal_sample_rows(const void* logits, size_t logits_stride, int vocab, int dtype, int B, const void* params, void* rng_state,
                     int32_t* tokens, int32_t* pos, int32_t* history, int history_len, int32_t* kept_out, const int32_t* active,
                     int slot0, void* stream);

/* ---- per-request stop conditions of continuous batching, teal_amd/csrc/teal_stop.hip ------------------------------------------
 * The retire launch with stop ids, stop sequences, a minimum length and a finish reason.  It takes the place of the plain retire
 * launch after a step's samplers (and after an admission's first draw) while an engine has the feature on: one launch for one.
 * slot_state, tokens, pos, B, slot_mask, max_seq and count_step mean what they mean for the plain retire launch; the slot-state
 * layout is untouched.
 * history: int32 [B][history_stride]; entry c of row b is the token of draw c of the request now in slot b — the samplers write it
 * before this launch, and a row restarts at 0 on admission.  stops: int32 [8][TEAL_STOP_WORDS], row b for slot b:
 *   TEAL_STOP_MIN      min_new_tokens: no stop id, EOS id or stop sequence fires while fewer tokens than this are produced
 *                      (<= 1: always armed)
 *   TEAL_STOP_NIDS     stop ids in use, 0..16 (device data: a value above 16 is read as 16, one below 0 as 0)
 *   TEAL_STOP_NSEQ     stop sequences in use, 0..8 (above 8 is read as 8, below 0 as 0)
 *   TEAL_STOP_REASON   out: TEAL_FINISH_* — why the slot stopped.  The host writes TEAL_FINISH_RUNNING at admission
 *   TEAL_STOP_MATCH    out: the token id for STOP_TOKEN, the sequence's index for STOP_SEQUENCE, -1 otherwise
 *   words 5..7         reserved, never written
 *   TEAL_STOP_IDS      + i, i < 16: the stop ids
 *   TEAL_STOP_SEQLEN   + q, q < 8: the length of sequence q, 1..8 (any other value: the sequence never matches)
 *   TEAL_STOP_SEQ      + 8 q + j: token j of sequence q
 * The rule, for every slot b < B that is active and in slot_mask, with n = PRODUCED[b] before the launch, t = tokens[b], p = pos[b]:
 *   BUDGET[b] -= 1;  PRODUCED[b] = n + 1
 *   armed      = n + 1 >= MIN
 *   hit_id     = armed and ((EOS[b] >= 0 and t == EOS[b]) or t == IDS[i] for some i < NIDS)
 *   hit_seq q  = armed and q < NSEQ and len = SEQLEN[q] in 1..8 and len <= n + 1 and SEQ[q][len-1] == t
 *                and SEQ[q][j] == history[b][n - len + 1 + j] for every j < len - 1
 *   the slot stops when hit_id, some hit_seq, BUDGET <= 0 or p >= max_seq holds; the reason is the first of STOP_TOKEN,
 *   STOP_SEQUENCE (the lowest q), LENGTH, CACHE that holds.  On a stop FINISH[b] = STEP, REASON and MATCH are written, the slot's
 *   bit is cleared and pos[b] is pulled back to max_seq - 1 if it passed it.  count_step != 0: STEP += 1.
 * A sequence is matched against tokens this request generated only: len <= n + 1 keeps every history index at 0 or above, and the
 * prompt is never looked at.  A slot that is inactive or outside slot_mask changes nothing: no state word, no word of its stops
 * row, no position.  With a slot's MIN, NIDS and NSEQ all 0, slot_state and pos leave bit-identical to the plain retire launch's.
 * The caller's contract: n < history_stride for every slot served (the engines' rows hold max_seq + 1 entries); a history entry
 * at or past history_stride is never read and counts as a mismatch.  A matched sequence of 8 tokens ends at entry n and starts at
 * n - 7, hence history_stride >= 8.
 * One workgroup, no atomics, no workspace; replays are bit-identical.
 * TEAL_ERR_ARG: a null pointer, B outside 1..8, max_seq < 1, history_stride < 8; every check comes before any HIP call. */
#define TEAL_STOP_MIN 0
#define TEAL_STOP_NIDS 1
#define TEAL_STOP_NSEQ 2
#define TEAL_STOP_REASON 3
#define TEAL_STOP_MATCH 4
#define TEAL_STOP_IDS 8
#define TEAL_STOP_SEQLEN 24
#define TEAL_STOP_SEQ 32
#define TEAL_STOP_WORDS 96
#define TEAL_STOP_MAX_IDS 16
#define TEAL_STOP_MAX_SEQS 8
#define TEAL_STOP_MAX_SEQ_LEN 8
#define TEAL_FINISH_RUNNING 0
#define TEAL_FINISH_STOP_TOKEN 1
#define TEAL_FINISH_STOP_SEQUENCE 2
#define TEAL_FINISH_LENGTH 3
#define TEAL_FINISH_CACHE 4
int teal_batched_retire_stops(int32_t* slot_state, const int32_t* tokens, int32_t* pos, const int32_t* history, int history_stride,
                              int32_t* stops, int B, int slot_mask, int max_seq, int count_step, void* stream);

/* ---- constrained decoding, teal_amd/csrc/teal_constrain.hip -------------------------------------------------------------------
 * Per-request token automata stepped on the device: one launch behind the logit processors (it reads their rows when they are
 * on) and in front of the samplers (they read its `out`).  Logprobs and dumps go on reading the model's raw logits.
 * A token automaton has S >= 1 states, state 0 the start.  State s has edges(s): (token, next) pairs, tokens strictly ascending in
 * 0 .. vocab-1, next in -1 .. S-1; default(s) in -1 .. S-1; accept(s) in {0, 1}.  delta(s, t) = the `next` of the edge that names
 * t, if there is one, else default(s); t is ALLOWED in s iff delta(s, t) >= 0 (an edge with next = -1 is an exception to a
 * non-negative default: "anything but these").
 * Its image, S + edges words of int32 in `arena`: S header rows {edge_begin, edge_end, default, accept} — word offsets relative to
 * the image, edge_end - edge_begin = 2 * the state's edges — then the edges as (token, next) word pairs.  table: int32 [B][4] =
 * {base, S, 0, 0}: base the image's word offset in `arena`, or -1: row r is unconstrained.  Any number of rows may share an image.
 * The rule, for row r with EOS id e = eos[r] (-1: none), about to make draw c = rng_state[r][1] (before the sampler runs), fed
 * t = tokens[r], the request's latest token:
 *   1. state    c == 0: s_c = 0.  c > 0: p = trace[r][c-1] & 0x3FFFFFFF, clamped into 0 .. S-1, and
 *                 t == e:              s_c = p     (the EOS id never moves the automaton: an EOS drawn and ignored below a minimum)
 *                 delta(p, t) >= 0:    s_c = delta(p, t)
 *                 else:                s_c = p, with bit 30 (TEAL_CONSTRAIN_VIOLATION) set in the trace word — the fed token was
 *                                      banned; cannot happen for a token drawn under the mask
 *               trace[r][c] = s_c (| bit 30).
 *   2. mask     out[r][v] = logits[r][v], the same 16 bits, if v is allowed in s_c, or if v == e and accept(s_c); every other entry
 *               becomes -MAXF, the dtype's most negative finite value — never an infinity, as with teal_logit_adjust.  The EOS id is
 *               banned in a non-accepting state whatever default(s_c) says; edges may not name it.
 *   3. unconstrained rows (base < 0): out[r] is a bit-for-bit copy of logits[r] (-0, infinities, NaN payloads); trace[r][c] = 0.
 *   4. inactive rows (active != NULL and bit slot0 + r of active[0] clear) change nothing: `out` row untouched, no trace word.
 * Guarantee: a banned token enters the samplers' race with weight expf((-MAXF - mx) / T), exactly 0 when the largest allowed logit
 * mx is above -MAXF / 2 and T <= 100 (fp16: the exponent is then at most about -327; expf reaches 0 near -104), and the row's
 * maximum is an allowed token with weight 1 — a banned token never wins.  Callers refuse a constrained request with T > 100.
 * The host validates images (sorted tokens inside the vocabulary, next / default in range, no edge on the EOS id, no dead end);
 * the device only keeps a damaged image's reads inside `arena`.  The caller's contract: c < trace_len (a counter past it writes no
 * word and starts from state 0), as for the stop launch's history.
 * Grid (ceil(vocab / 8192), B), 1024 threads, 16-byte loads and stores.  Every workgroup of a row recomputes s_c (uniform), builds
 * a bitmap of its 8192 entries in LDS from the state's default and its sub-range of the sorted edges (LDS bit atomics: order does
 * not matter) and applies it; workgroup x == 0 alone writes trace[r][c].  No workgroup reads a word the launch writes; no
 * workspace; replays from the same state are bit-identical.
 * rng_state: uint64 [B][2] = {seed, draw counter} (read only); tokens, eos: int32 [B]; trace: int32 [B][trace_len]; strides in
 * elements.  The checks of teal_logit_adjust, before any HIP call, and TEAL_ERR_ARG also for trace_len < 1, arena_words == 0 and
 * an `out` that overlaps `logits`. */
#define TEAL_CONSTRAIN_VIOLATION (1 << 30)
#define TEAL_CONSTRAIN_STATE_MASK 0x3FFFFFFF
int teal_constrain_logits(const void* logits, size_t logits_stride, int vocab, int dtype, int B, const int32_t* tokens,
                          const void* rng_state, const int32_t* eos, const int32_t* table, const int32_t* arena, size_t arena_words,
                          int32_t* trace, int trace_len, void* out, size_t out_stride, const int32_t* active, int slot0, void* stream);

/* ---- teacher-forced tokens of continuous batching, teal_amd/csrc/teal_force.hip -------------------------------------------------
 * One launch after a draw's sampler launch or launches, before the logprob launch (teal_token_logprobs) and before retire.  Row
 * r < B serves slot slot0 + r.
 *   c = rng_state[r][1]          (uint64: the draw counter the sampler has just bumped)
 *   i = c - 1
 *   n = min(forced_len[r], forced_stride)
 *   if (active == NULL or bit slot0 + r of active[0] is set) and 0 <= i < n:
 *       t = forced[r * forced_stride + i]
 *       tokens[r] = t
 *       if history != NULL and i < history_len:  history[r * history_len + i] = t
 *   otherwise nothing is written
 * The sampler has already moved pos, the counter and the history entry, so the launch leaves exactly the words a sampler that had
 * drawn t would have left, and everything behind it sees t as the drawn token: teal_token_logprobs reports lp(t) of the model's
 * raw row, the retire launch (plain or with stop conditions) counts t and matches it, the next step is fed t, and the next
 * step's logit processors count it.  The ids are not checked against a vocabulary here: that is the admission's.
 * forced: int32 [B][forced_stride]; forced_len: int32 [B]; rng_state: uint64 [B][2]; tokens: int32 [B]; history: int32
 * [B][history_len] or NULL.  A null required pointer, B outside 1..8, slot0 < 0 or slot0 + B > 32, forced_stride <= 0 or
 * history_len < 0 with a history: TEAL_ERR_ARG, every check before any HIP call.  One wave, lane r serving row r; two dependent
 * load rounds at most ({active word, counter, length}, then the table entry); no atomics, no workspace: replays are
 * bit-identical. */
int teal_force_tokens(const int32_t* forced, int forced_stride, const int32_t* forced_len, const void* rng_state, int32_t* tokens,
                      int32_t* history, int history_len, int B, const int32_t* active, int slot0, void* stream);

/* ---- shared prompt prefixes of continuous batching, teal_amd/csrc/teal_prefix.hip ------------------------------------
 * A prefix is a token sequence whose K / V rows (every layer) are computed once and kept in a device store; a request that names
 * it is admitted by copying those rows into its slot's caches and running a prompt pass over its own tokens only. */

/* Rows 0 .. rows-1 of every head of n_tensors cache tensors in ONE launch: for every tensor t < n_tensors, head h < n_heads and row
 * r < rows the row_bytes bytes at dst[t] + h * dst_head_stride + r * row_bytes become those at src[t] + h * src_head_stride +
 * r * row_bytes (16-byte loads and stores); no other byte is written.  src_table / dst_table: DEVICE arrays of n_tensors 64-bit
 * addresses, each row 0 of head 0 of one tensor (K and V of every layer: n_tensors = 2 L), 16-byte aligned — the caller's contract,
 * they are read on the device only (no host synchronisation; a captured launch follows the tables' contents at replay).  rows == 0
 * launches nothing.  TEAL_ERR_ARG: a null table, n_tensors / n_heads / row_bytes <= 0, rows < 0; TEAL_ERR_ALIGN: row_bytes or a head
 * stride not a multiple of 16; TEAL_ERR_SHAPE: a head stride smaller than rows * row_bytes, n_tensors or n_heads above 65535. */
int teal_kv_copy_rows(const void* src_table, const void* dst_table, int n_tensors, int n_heads, int rows, int row_bytes,
                      size_t src_head_stride, size_t dst_head_stride, void* stream);

/* ---- fp8 KV cache of continuous batching, teal_amd/csrc/teal_kv8.hip ---------------------------------------------------
 * A cached K or V row of one KV head is hd bytes of OCP e4m3fn codes and one fp32 scale word that holds an exact power of two; a
 * cache is two tensors, codes [n_kv][max_seq][hd] uint8 and scales [n_kv][max_seq] fp32.  The rule, for a row x[0 .. hd) of 16-bit
 * values widened exactly to fp32 (tests/kv8_rule.py restates it in integers):
 *   a = max |x_d|;  e = 0 if a == 0, else the smallest integer with a * 2^-e <= 448, then clamped below at -100;  scale = 2^e;
 *   code_d = RNE_e4m3fn(x_d * 2^-e): subnormals down to 2^-9, ties to even, the sign kept (-0 -> 0x80).  The product is exact in
 *   fp32 wherever it does not underflow (and there the code is +-0 either way); |x_d * 2^-e| <= 448, so nothing saturates.
 *   Dequantisation is float(code_d) * scale, exact in fp32.
 * A row that holds NaN or Inf is outside the contract: its codes and scale are unspecified, and no byte outside the row is touched. */

/* For every tensor t < n_tensors, head h < n_heads and row r < rows: the head_dim 16-bit values at src[t] + ((h * src_head_rows + r)
 * * head_dim) elements become head_dim codes at code[t] + (h * dst_head_rows + r) * head_dim bytes and one scale word at scale[t] +
 * (h * dst_head_rows + r) floats, by the rule above.  No other byte is written.  One launch covers all tensors (K and V of every
 * layer: n_tensors = 2 L).  The three tables are DEVICE arrays of n_tensors 64-bit addresses (teal_kv_copy_rows' conventions: row 0 of
 * head 0 of one tensor each, 16-byte aligned by the caller's contract, read on the device only — no host synchronisation).  rows == 0
 * launches nothing.  TEAL_ERR_ARG: a null table, n_tensors / n_heads <= 0, rows < 0; TEAL_ERR_DTYPE; TEAL_ERR_SHAPE: head_dim not
 * 64 / 128, rows above a head's rows on either side, n_tensors or n_heads above 65535; TEAL_ERR_ALIGN: a table off 8 bytes. */
int teal_kv8_quantize_rows(const void* src_table, const void* code_table, const void* scale_table, int n_tensors, int n_heads, int head_dim,
                           int rows, size_t src_head_rows, size_t dst_head_rows, int dtype, void* stream);
/* teal_batched_decode_attention_slots on fp8 caches: k_codes / v_codes [B][n_kv][max_seq][hd] uint8 (16-byte aligned), k_scales /
 * v_scales [B][n_kv][max_seq] fp32.  The same grid, plan, partials layout and merge launch; the kernel is the same chunked split-KV
 * body with its cache format set.  Cached rows r < pos[b] enter as float(code) * scale; the new row is attended unquantised (the
 * launch that makes a row sees it exactly, like the prompt pass) and its codes and scale are stored by the rule for later launches.
 * So yt holds the words teal_batched_decode_attention_slots leaves on 16-bit caches that hold the dequantised values, whenever
 * those are representable in the dtype.  An inactive slot writes nothing and its yt slot is zero.  TEAL_ERR_ARG also for null scales. */
int teal_batched_decode_attention_slots_kv8(const float* qkv_slabs, int split, const void* rope, const int32_t* pos, const int32_t* active,
                                            void* k_codes, void* v_codes, float* k_scales, float* v_scales, void* yt, float* partials,
                                            size_t partials_bytes, int B, int n_head, int n_kv_head, int head_dim, int max_seq, int dtype,
                                            void* stream);

/* ---- benchmark comparator (scripts/benchmark_gemv.py only; not on the decode path) ----------- */

/* The Deja Vu gather GEMV the reference's kernel benchmark plots next to TEAL's (scripts/benchmark_gemv.py:32-107,170-172),
 * restated for CDNA4: flags[m] = |x[m]| > tau by a launch of its own, y32 zeroed, then a (row block, column tile) grid adds
 * fp32 partial sums of the flagged rows into y32 with atomics.  y32: fp32 [N]; flags: Z bytes of scratch.  Three launches. */
int teal_cmp_flag_gemv(const void* x, const void* wT, int ld, float* y32, unsigned char* flags, float tau, int Z, int N,
                       int dtype, void* stream);

/* ---- diagnostics build only (libteal_hip_diag.so = these sources with -DTEAL_DIAGNOSTICS) ------------------------
 * Process-global switches, NOT thread-safe, for benchmarks, phase-stamp probes and the parity tests that force the general
 * kernel or a launch geometry.  libteal_hip.so exports none of them. */
#ifdef TEAL_DIAGNOSTICS

/* Override the launch geometry picked from (Z, N, CU count): lanes per row segment (8/16/32/64) and split-K factor
 * (>= 1); waves per workgroup and unroll depth are fixed at 16 and 4 (the other values of round 1 were sweep-only
 * and are no longer built: pass 0 or the fixed value).  0 = automatic.  Process-global; meant for benchmark sweeps only. */
int teal_set_tuning(int lanes_per_row, int waves, int split, int unroll);

/* Wave-local compaction (default on): each wave streams the rows it ballots itself instead of an even share
 * of a workgroup-wide list; removes every barrier between the activation and the first weight load. */
int teal_set_wave_local(int on);

/* Diagnostics: kernel template instantiation and grid of the most recent GEMV launch of this process (host-side
 * string; e.g. for naming the kernel in a benchmark record). */
const char* teal_last_launch_desc(void);

/* Lean kernel for qualifying shapes (default on; 0 forces the general kernel everywhere: A/B and parity tests). */
int teal_set_fast(int on);

/* Diagnostics: when set (device pointer to >= 32 * workgroups uint64 — 32 stamps per workgroup of the launch), every
 * GEMV workgroup stores 100 MHz wall-clock stamps of its phases, row w of the buffer = workgroup w:
 *   [0] kernel entry, [1] kernel arguments in registers, [2] activation ready, [3] row list ready, [4] first weight
 *   batch consumed (wave 0), [5] wave 0 done streaming, [6] past the reduce barrier, [7] done,
 *   [12] hardware id << 32 | XCC id, [13] waves << 32 | workgroups, [16 + w] end of stream of wave w (w < 16).
 * The attention, sampler and int4 launches (the latter with fp16 activations only) stamp rows of the same width with their own
 * phase meanings (scripts/attn_phase.py, scripts/sampler_phase.py, scripts/int4_phase.py).  NULL (default) disables.
 * Process-global. */
int teal_set_phase_buffer(void* dev_u64);
/* > 0: consecutive GEMV / attention launches stamp consecutive regions of `u64_per_launch` uint64 of the phase buffer
 * (so that a chain of launches can be timed against each other): u64_per_launch >= 32 * the largest launch's
 * workgroups, and the buffer must hold u64_per_launch * (launches between two teal_set_phase_stride calls) uint64;
 * 0 (default): every launch stamps the start of the buffer. */
int teal_set_phase_stride(size_t u64_per_launch);

/* Probe of the epilogues' row-group reduction (teal_common.h: row_reduce_scatter) against the shuffle butterfly it replaces,
 * on caller-supplied bit patterns.  in: uint32 [nwaves][64 lanes][8 accumulators], read as floats; lanes_per_row 8 or 16.
 *   scatter: uint32 [nwaves][64][2] — lane 16 r + i (i < lanes_per_row) holds the totals of accumulators r and 4 + r over the
 *            lanes l with l % lanes_per_row == i;
 *   shuffle: uint32 [nwaves][64][8] — `v += __shfl_xor(v, off)` for off = lanes_per_row .. 32: lane i holds every total. */
int teal_probe_row_reduce(const void* in_u32, void* scatter_u32, void* shuffle_u32, int nwaves, int lanes_per_row, void* stream);
#endif /* TEAL_DIAGNOSTICS */

/* ---- introspection (pure functions of their arguments; teal_get_config also of the device's CU count) - */

/* The geometry of a plain rounded 16-bit GEMV of this shape BEFORE any adjustment for the output kind or the weight width
 * (slab, pair and int8 launches choose their own: ask teal_fused_gemv_plan): out[0..5) = {lanes_per_row, waves, split,
 * unroll, workgroups}.  `nseg` is ignored. */
int teal_get_config(int Z, int N, int nseg, int* out);

/* What teal_fused_gemv(in, out, Z, dtype, ws, ws_bytes, nslabs_out, stream) returns, reports in *nslabs_out and writes to
 * out->desc on a device with num_cu CUs — from the launch's own plan (teal_amd/csrc/teal_gemv_plan.h), host only: no device is
 * needed, nothing is launched and no data pointer is dereferenced (their nullness, alignment and identities are all that
 * matters, so any values with those properties serve).  The caller's workspace is described instead of passed: ws_bytes (0 =
 * none) and ws_prepared (it went through teal_workspace_init); it counts as 16-byte aligned.  out->slabs counts as plain
 * memory.  Never TEAL_ERR_NO_DEVICE or TEAL_ERR_LAUNCH; TEAL_ERR_ARG also for num_cu <= 0.  The diagnostics build honours its
 * switches as a launch does. */
int teal_fused_gemv_plan(const teal_gemv_in_t* in, const teal_gemv_out_t* out, int Z, int dtype, int ws_prepared,
                         size_t ws_bytes, int num_cu, int* nslabs_out);

/* The launch teal_decode_attention_split* makes for this shape (teal_amd/csrc/teal_attention.hip; host only, no device needed):
 * out[0] = 1: the shape takes the grouped-query kernel (n_head / n_kv_head = 8 or 4 from its cache length on; never when
 * `roped`, i.e. through teal_decode_attention_split_roped); out[1] = threads per workgroup; out[2] = dynamic LDS bytes of that
 * launch at this nsplit; out[3] = the LDS limit it has to fit.  For the grouped kernel that is what a device grants after
 * teal_init(): above it the launch falls back to the per-query-head kernel.  Otherwise it is 64 KiB, and the launch
 * refuses a share above it (TEAL_ERR_SHAPE).  The query itself reports either case through out[2] > out[3].
 * TEAL_ERR_ARG: out == NULL; TEAL_ERR_SHAPE: the arguments the launch refuses (head_dim not 64 / 128, n_head not a positive
 * multiple of n_kv_head, max_seq < 1, nsplit outside 1..64). */
int teal_decode_attention_split_plan(int n_head, int n_kv_head, int head_dim, int max_seq, int nsplit, int roped, int* out);

#ifdef __cplusplus
}
#endif
#endif /* TEAL_HIP_H */
