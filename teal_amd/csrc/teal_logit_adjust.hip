// teal_logit_adjust.hip — per-request logit processors and their C-ABI entry point (include/teal_hip.h): one launch between a
// step's logits and its samplers.
//
// For element v of a row of 16-bit logits l, the request's state word w[v] (bit 31: v occurs in the prompt; low 31 bits n: how
// often v was generated), its parameters {theta, alpha_p, alpha_f} and an optional bias row b:
//
//   x = float(l[v])
//   w[v] != 0:   x = x > 0 ? x / theta : x * theta            repetition penalty (prompt or generated)
//   n > 0:       x = x - alpha_f * float(n);  x = x - alpha_p    frequency, then presence penalty
//   bias:        x = x + float(b[v])
//   out[v] = round-to-nearest-even(min(max(x, -MAXF), MAXF))     MAXF: the dtype's largest finite value — never an infinity
//
// Every operation is ONE correctly rounded fp32 operation: rn_mul / rn_sub / rn_add / rn_div below keep the library's
// -ffp-contract=on from folding a product into the subtraction behind it (tests/logit_rule.py restates the rule in numpy, and
// the tests compare bit for bit).  NaN logits are outside the contract.
//
// Counting: with count_token != 0 the thread that owns element tokens[r] adds 1 to that word's count (saturating at 2^31 - 1)
// before it adjusts the element, and stores that one word back.  No other state word is written and no element has two
// writers, so there are no atomics and replays are bit-identical.
//
// A pure streaming pass: grid (ceil(vocab / 8192), B), 1024 threads, 8 consecutive elements per thread — one 16-byte load of
// the logits and of the bias, two of the state, one 16-byte store; no LDS, no workspace.  Rows are predicated on the slot
// engine's active word: an inactive row counts nothing and leaves its `out` row alone.
#include "teal_common.h"

// one rounding per operation, whatever the contraction setting the library is built with (the intrinsics below say so too)
#pragma clang fp contract(off)

namespace teal {

__device__ __forceinline__ float rn_mul(const float a, const float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float rn_sub(const float a, const float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float rn_add(const float a, const float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float rn_div(const float a, const float b) { return __fdiv_rn(a, b); }

// round to nearest even to the dtype.  The value comes out of the clamp's v_min_f32, not out of a multiply-add, so there is no
// fused multiply-add for the compiler to fold the conversion into (what float_to_bits guards against with its compiler barrier).
template <bool BF16>
__device__ __forceinline__ uint32_t round16(const float x) {
    if (BF16) return __builtin_bit_cast(uint16_t, (__bf16)x);
    return __builtin_bit_cast(uint16_t, (_Float16)x);
}

constexpr int kAdjustPerWg = 8192;  // elements a workgroup of 1024 threads covers

template <bool BF16, bool BIAS>
__global__ __launch_bounds__(1024) void logit_adjust_kernel(const uint16_t* __restrict__ logits, const size_t stride, const int V,
                                                             const int* __restrict__ tokens, const int count_token,
                                                             int* __restrict__ state, const float* __restrict__ params,
                                                             const uint16_t* __restrict__ bias, uint16_t* __restrict__ out,
                                                             const size_t out_stride, const int* __restrict__ active, const int slot0) {
    const int r = blockIdx.y;
    if (active && !((active[0] >> (slot0 + r)) & 1)) return;
    const int e0 = (blockIdx.x * 1024 + threadIdx.x) * 8;
    if (e0 >= V) return;  // (V % 8 == 0: a thread's 8 elements are inside the row or all outside)
    const u32x4 lv = *reinterpret_cast<const u32x4*>(logits + (size_t)r * stride + e0);
    int* const srow = state + (size_t)r * V + e0;
    const u32x4 s0 = *reinterpret_cast<const u32x4*>(srow), s1 = *reinterpret_cast<const u32x4*>(srow + 4);
    u32x4 bv = {0u, 0u, 0u, 0u};
    if (BIAS) bv = *reinterpret_cast<const u32x4*>(bias + (size_t)r * V + e0);
    const float theta = params[4 * r], alpha_p = params[4 * r + 1], alpha_f = params[4 * r + 2];
    const int tok = count_token ? tokens[r] : -1;  // (an id outside 0 .. V-1 is no thread's element)
    const float maxf = BF16 ? __uint_as_float(0x7F7F0000u) : 65504.0f;
    u32x4 ov;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        uint32_t w = j < 4 ? s0[j] : s1[j - 4];
        if (e0 + j == tok) {
            if ((w & 0x7FFFFFFFu) != 0x7FFFFFFFu) ++w;
            srow[j] = (int)w;
        }
        const uint32_t lb = (j & 1) ? (lv[j >> 1] >> 16) : (lv[j >> 1] & 0xFFFFu);
        float x = bits_to_float(lb, BF16);
        if (w != 0u) x = x > 0.0f ? rn_div(x, theta) : rn_mul(x, theta);
        const uint32_t n = w & 0x7FFFFFFFu;
        if (n != 0u) {
            x = rn_sub(x, rn_mul(alpha_f, (float)n));
            x = rn_sub(x, alpha_p);
        }
        if (BIAS) x = rn_add(x, bits_to_float((j & 1) ? (bv[j >> 1] >> 16) : (bv[j >> 1] & 0xFFFFu), BF16));
        x = fminf(fmaxf(x, -maxf), maxf);
        const uint32_t ob = round16<BF16>(x);
        if (j & 1) ov[j >> 1] |= ob << 16; else ov[j >> 1] = ob;
    }
    *reinterpret_cast<u32x4*>(out + (size_t)r * out_stride + e0) = ov;
}

}  // namespace teal

using namespace teal;

extern "C" {

int teal_logit_adjust(const void* logits, size_t logits_stride, int vocab, int dtype, int B, const int32_t* tokens, int count_token,
                      int32_t* state, const float* params, const void* bias, void* out, size_t out_stride, const int32_t* active,
                      int slot0, void* stream) {
    if (!logits || !tokens || !state || !params || !out) return TEAL_ERR_ARG;
    if (B < 1 || B > 8 || slot0 < 0 || slot0 + B > 32) return TEAL_ERR_ARG;
    if (dtype != TEAL_F16 && dtype != TEAL_BF16) return TEAL_ERR_DTYPE;
    if (vocab < 8 || vocab > 16 * kAdjustPerWg || (vocab & 7)) return TEAL_ERR_SHAPE;
    if (!aligned16(logits) || !aligned16(out) || !aligned16(state) || (bias && !aligned16(bias))) return TEAL_ERR_ALIGN;
    if (B > 1 && ((logits_stride & 7) || (out_stride & 7))) return TEAL_ERR_ALIGN;
    {   // `out` must not alias `logits`: the logprob launch behind the samplers reads the raw rows
        const uintptr_t l0 = reinterpret_cast<uintptr_t>(logits), o0 = reinterpret_cast<uintptr_t>(out);
        const uintptr_t l1 = l0 + ((size_t)(B - 1) * logits_stride + (size_t)vocab) * 2, o1 = o0 + ((size_t)(B - 1) * out_stride + (size_t)vocab) * 2;
        if (l0 < o1 && o0 < l1) return TEAL_ERR_ARG;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    auto* lg = reinterpret_cast<const uint16_t*>(logits);
    auto* bs = reinterpret_cast<const uint16_t*>(bias);
    auto* o = reinterpret_cast<uint16_t*>(out);
    const dim3 grid((vocab + kAdjustPerWg - 1) / kAdjustPerWg, B);
#define TEAL_ADJUST(KERNEL) \
    hipLaunchKernelGGL((KERNEL), grid, dim3(1024), 0, st, lg, logits_stride, vocab, tokens, count_token, state, params, bs, o, out_stride, active, slot0)
    if (dtype == TEAL_BF16) {
        if (bias) TEAL_ADJUST((logit_adjust_kernel<true, true>)); else TEAL_ADJUST((logit_adjust_kernel<true, false>));
    } else {
        if (bias) TEAL_ADJUST((logit_adjust_kernel<false, true>)); else TEAL_ADJUST((logit_adjust_kernel<false, false>));
    }
#undef TEAL_ADJUST
    return hipGetLastError() == hipSuccess ? TEAL_OK : TEAL_ERR_LAUNCH;
}

}  // extern "C"
