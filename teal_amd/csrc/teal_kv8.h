// teal_kv8.h — the fp8 KV-cache row format of continuous batching (include/teal_hip.h, "fp8 KV cache"): the device side of
// the rule, typed once for the two places that write a row (teal_kv8_quantize_rows and the batched attention's single writer) and
// the one that reads it (the staging loop of teal_chunked_attention.h).
//
// A row x[0 .. hd) of one KV head, 16-bit values widened exactly to fp32, is hd OCP e4m3fn codes and one fp32 scale 2^e:
//   a = max |x_d|;  e = 0 if a == 0, else the smallest integer with a * 2^-e <= 448, clamped below at -100;
//   code_d = RNE_e4m3fn(x_d * 2^-e)   (the product is exact where it does not underflow; |.| <= 448: nothing saturates);
//   x'_d = float(code_d) * 2^e        (exact in fp32).
// gfx950 converts e4m3fn in hardware both ways (v_cvt_pk_fp8_f32: round to nearest even, subnormals down to 2^-9, the sign kept;
// v_cvt_pk_f32_fp8), so the rule costs a multiply and half a conversion per element.
#pragma once
#include "teal_common.h"

namespace teal {

template <bool KV8>
using kv_elem_t = std::conditional_t<KV8, uint8_t, uint16_t>;  // what a cache pointer points at

constexpr int kKv8MinExp = -100;

// e of the rule for a = max |x_d| (finite, >= 0).  a = m * 2^k, 1 <= m < 2: a * 2^-e <= 448 = 1.75 * 2^8 first holds at e = k - 8 when
// m <= 1.75 and at e = k - 7 otherwise.  (A bf16 subnormal widens to an fp32 subnormal: exponent field 0 reads as k = -127 and the
// clamp takes it, as it takes the true e < -100.)
__device__ __forceinline__ int kv8_scale_exp(const float amax) {
    const uint32_t b = __float_as_uint(amax);
    if (b == 0u) return 0;
    const int k = (int)(b >> 23) - 127;
    return max(k - ((b & 0x7FFFFFu) <= 0x600000u ? 8 : 7), kKv8MinExp);
}

// One row written by LANES consecutive lanes of a wave (LANES = hd / 8, a power of two; all of them active): each holds 8 of the
// row's values and stores their 8 codes with one 8-byte store; the row's first lane stores the scale word.  Nothing else is written.
template <int LANES>
__device__ __forceinline__ void kv8_store_row(const float (&x)[8], uint8_t* __restrict__ codes, float* __restrict__ scale, const bool first) {
    float a = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) a = fmaxf(a, fabsf(x[j]));
#pragma unroll
    for (int d = 1; d < LANES; d <<= 1) a = fmaxf(a, __shfl_xor(a, d));
    const int e = kv8_scale_exp(a);
    const float inv = __uint_as_float((uint32_t)(127 - e) << 23);  // 2^-e, e in -100 .. 120
    u32x2 w;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        int v = 0;
        v = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * q] * inv, x[4 * q + 1] * inv, v, false);
        v = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * q + 2] * inv, x[4 * q + 3] * inv, v, true);
        w[q] = (uint32_t)v;
    }
    *reinterpret_cast<u32x2*>(codes) = w;
    if (first) *scale = __uint_as_float((uint32_t)(e + 127) << 23);
}

// 16 codes (one 16-byte load, in memory order) times their row's scale
__device__ __forceinline__ void kv8_dequant16(const u32x4 w, const float scale, float (&out)[16]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], false);
        const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], true);
        out[4 * j] = lo[0] * scale; out[4 * j + 1] = lo[1] * scale;
        out[4 * j + 2] = hi[0] * scale; out[4 * j + 3] = hi[1] * scale;
    }
}

}  // namespace teal
