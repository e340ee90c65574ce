// teal_slab.h — what the three dense slab-chain passes share: the prompt pass (teal_prefill.hip), the verify / suffix pass
// (teal_speculative.hip) and the batched / slot step (teal_batched.hip).
//
// The hand-over layout between the launches of a layer is TRANSPOSED: [feature][KR], KR = rows_for(rows) token (or sequence)
// slots per feature — 16-bit activations as KR / 8 16-byte words, fp32 split-K slabs [slice][column][KR] as KR / 4 of them.  A
// GEMM deals its 16-row groups to `split` slices (slab_gemm_split) and leaves one slab per slice; every consumer sums a column's
// slabs in slice order and rounds once (slab_column / rounded_row): what a projection's 16-bit output tensor holds.  What a GEMM
// builds its activations from while staging is a SlabProd, filled from the C ABI's teal_prefill_in_t by slab_prod_fill.
// The attention of the two passes that attend a cache (verify, batched) reads its new rows from the wqkv slabs in this layout:
// teal_chunked_attention.h, which includes this header.
#pragma once
#include "teal_producers.h"

#include <limits.h>

namespace teal {

typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int kSlabMaxSplit = 16;  // most slices (slabs) of a GEMM launch
constexpr int rows_for(const int T) { return T <= 8 ? 8 : 16; }

// What a GEMM's staging loop builds a row's KR activations from (PROD): 0 = xt itself; 1 = RMSNorm of the residual rows ht with the
// per-workgroup sums of squares the resid launch left (every wave adds them itself) and the norm weight; 2 = silu(gate) * up from
// the slabs of the gate | up launch.  Folding these into the staging removes a launch each: every workgroup builds only the rows
// of its own slice (a 16th of the vector in the narrow projections), once.
struct SlabProd {
    const uint16_t* xt;       // PROD 0: [Z][KR];  PROD 1: the residual rows ht [Z][KR]
    const float* sumsq;       // PROD 1: [nwg][KR]
    const uint16_t* norm_w;   // PROD 1: [Z]
    const float* gu;          // PROD 2: slabs [gu_split][2 Z][KR] of the gate | up launch
    float eps;
    int nwg, gu_split, rows;  // rows: the tokens (prompt, verify) or sequences (batched) of the pass; slots past them are zero
};

// the producer of a launch that writes `out_slabs`, from the C ABI's description (TEAL_ERR_ARG: a missing or misaligned pointer,
// nwg or gu_split out of range, or gate | up slabs that are the launch's own output)
inline int slab_prod_fill(const teal_prefill_in_t* in, const float* out_slabs, const int max_split, const int rows, SlabProd* pr) {
    *pr = {};
    pr->rows = rows;
    switch (in->mode) {
        case TEAL_PREFILL_IN_XT:
            if (!in->xt || !aligned16(in->xt)) return TEAL_ERR_ARG;
            pr->xt = reinterpret_cast<const uint16_t*>(in->xt);
            break;
        case TEAL_PREFILL_IN_NORM:
            if (!in->xt || !aligned16(in->xt) || !in->sumsq || !aligned16(in->sumsq) || !in->norm_w || in->nwg < 1 || in->nwg > 64) return TEAL_ERR_ARG;
            pr->xt = reinterpret_cast<const uint16_t*>(in->xt);
            pr->sumsq = in->sumsq; pr->nwg = in->nwg; pr->norm_w = reinterpret_cast<const uint16_t*>(in->norm_w); pr->eps = in->eps;
            break;
        case TEAL_PREFILL_IN_SILU_MUL:
            if (!in->gu_slabs || !aligned16(in->gu_slabs) || in->gu_split < 1 || in->gu_split > max_split) return TEAL_ERR_ARG;
            if (in->gu_slabs == out_slabs) return TEAL_ERR_ARG;  // the launch reads its producer's slabs while it writes its own
            pr->gu = in->gu_slabs; pr->gu_split = in->gu_split;
            break;
        default: return TEAL_ERR_ARG;
    }
    return TEAL_OK;
}

// slices of a GEMM of `tiles` 256-column tiles over Z rows: never more workgroups than CUs (a 16-wave workgroup owns its CU: 86
// tiles x 3 = 258 workgroups ran 62 us, x 2 = 172 run 38), every wave keeping at least one full pair of batches of a dense slice
// (split <= Z / 256), and among the candidates the one whose waves stream the fewest 8-row batches (ties: the fewer slabs)
inline int slab_gemm_split(const int num_cu, const int tiles, const int Z, const int max_split) {
    const int ngroups = Z >> 4;
    int smax = num_cu / tiles;
    if (smax > Z / 256) smax = Z / 256;
    if (smax > max_split) smax = max_split;
    if (smax < 1) smax = 1;
    int split = 1, best = INT_MAX;
    for (int c = 1; c <= smax; ++c) {
        const int batches = ((ngroups + c - 1) / c + 7) / 8;
        if (batches < best) { best = batches; split = c; }
    }
    return split;
}

// 1 / rms per token from the per-workgroup sums of squares sumsq [nwg][KR] (lane = producing workgroup, nwg <= 64; the total in
// workgroup order)
template <int KR>
__device__ __forceinline__ void rstd_rows(const float* __restrict__ sumsq, const int nwg, const int lane, const int Z, const float eps,
                                          float (&rstd)[KR]) {
    f32x4 pw[KR / 4];
#pragma unroll
    for (int w = 0; w < KR / 4; ++w) pw[w] = lane < nwg ? *reinterpret_cast<const f32x4*>(sumsq + (size_t)lane * KR + 4 * w) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KR; ++s) rstd[s] = rsqrtf(wave_sum_f(pw[s >> 2][s & 3]) / (float)Z + eps);
}

// sum of `split` slabs [slice][n_total][KR] of column `col` in slice order, rounded once to the activation dtype
template <bool BF16, int KR>
__device__ __forceinline__ void slab_column(const float* __restrict__ slabs, const int split, const size_t n_total, const size_t col,
                                            float (&out)[KR]) {
    f32x4 acc[KR / 4];
#pragma unroll
    for (int w = 0; w < KR / 4; ++w) acc[w] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < split; ++s) {
        const float* p = slabs + ((size_t)s * n_total + col) * KR;
#pragma unroll
        for (int w = 0; w < KR / 4; ++w) acc[w] += *reinterpret_cast<const f32x4*>(p + 4 * w);
    }
#pragma unroll
    for (int w = 0; w < KR / 4; ++w)
#pragma unroll
        for (int s = 0; s < 4; ++s) out[4 * w + s] = bits_to_float(float_to_bits<BF16>(acc[w][s]), BF16);
}

// The same sum, for the prompt-pass kernels only.  There are two because this is the LOOKAHEAD variant: it keeps the loads of UU
// slices in flight together, where slab_column asks for one slice at a time.  Same order of additions, same bits.
template <bool BF16, int KR>
__device__ __forceinline__ void rounded_row(const float* __restrict__ slabs, const int split, const size_t n_total, const size_t col,
                                            float (&out)[KR]) {
    constexpr int NW = KR / 4, UU = KR == 8 ? 4 : 2;  // 16-byte words per row; slices whose loads are in flight together
    f32x4 acc[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) acc[w] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < split; k0 += UU) {  // (clamped: a repeated slice is not added); slice order kept
        f32x4 v[UU][NW];
#pragma unroll
        for (int u = 0; u < UU; ++u) {
            const float* p = slabs + ((size_t)min(k0 + u, split - 1) * n_total + col) * KR;
#pragma unroll
            for (int w = 0; w < NW; ++w) v[u][w] = *reinterpret_cast<const f32x4*>(p + 4 * w);
        }
#pragma unroll
        for (int u = 0; u < UU; ++u) {
            if (k0 + u < split) {
#pragma unroll
                for (int w = 0; w < NW; ++w) acc[w] += v[u][w];
            }
        }
    }
#pragma unroll
    for (int w = 0; w < NW; ++w)
#pragma unroll
        for (int s = 0; s < 4; ++s) out[4 * w + s] = bits_to_float(float_to_bits<BF16>(acc[w][s]), BF16);
}

// word w of a feature's row: slots 8 w .. 8 w + 7 as one 16-byte word of 16-bit values (slot 2 j in the low half of lane j)
template <bool BF16, int KR>
__device__ __forceinline__ u32x4 pack_row(const float (&v)[KR], const int w = 0) {
    u32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        r[j] = (uint32_t)float_to_bits<BF16>(v[8 * w + 2 * j]) | ((uint32_t)float_to_bits<BF16>(v[8 * w + 2 * j + 1]) << 16);
    return r;
}

template <bool BF16, int KR>
__device__ __forceinline__ void unpack_row(const u32x4 p, float (&x)[KR], const int w = 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { x[8 * w + 2 * j] = bits_to_float(p[j] & 0xFFFFu, BF16); x[8 * w + 2 * j + 1] = bits_to_float(p[j] >> 16, BF16); }
}

// a feature's KR slots to and from memory: KR / 8 16-byte words
template <bool BF16, int KR>
__device__ __forceinline__ void store_row(uint16_t* __restrict__ p, const float (&v)[KR]) {
#pragma unroll
    for (int w = 0; w < KR / 8; ++w) *reinterpret_cast<u32x4*>(p + 8 * w) = pack_row<BF16>(v, w);
}

template <bool BF16, int KR>
__device__ __forceinline__ void load_row(const uint16_t* __restrict__ p, float (&x)[KR]) {
#pragma unroll
    for (int w = 0; w < KR / 8; ++w) unpack_row<BF16>(*reinterpret_cast<const u32x4*>(p + 8 * w), x, w);
}

}  // namespace teal
