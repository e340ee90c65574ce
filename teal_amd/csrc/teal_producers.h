// teal_producers.h — the rounding chains of the fused producers and epilogues, ONE copy for every kernel that fuses one: the
// lean and the general GEMV (teal_gemv_fast.h, teal_gemv_kernel.h), the int4 GEMV, the split-K reduce and gate|up epilogue
// launches (teal_kernels.hip), the prompt pass and the batched step (through teal_slab.h) and the attention launches (RoPE).
// The decode step, the batched step, the prompt pass and the int4 path are specified to round like the module path and to
// agree among themselves bit for bit (tests/test_soak.py, test_engine_parity.py, the exact-integer probes); a chain that is
// typed once cannot drift.  (Still typed at their sites, because as functions they changed some kernel's instructions: the
// ordered sum of an element's interleaved slabs, the deposit half of the RMS reduce, the split-K ticket tail —
// profiles/producer_chains_refactor.txt.)
//
// Rule of this header: no expression of the form a * b + c.  The GEMV units compile with `#pragma clang fp contract(off)`, the
// others with -ffp-contract=on; a helper means the same in both, so a fused multiply-add is an explicit fmaf().
// Operands that a chain uses LATE (the norm weight, the up half) may be handed over as 16-bit patterns (uint32_t): they are
// then converted where the chain uses them, which is where the inline code converted them (late16).
#pragma once
#include "teal_common.h"

namespace teal {

// the one expression the chains are made of: a value as the module path's 16-bit tensor holds it
template <bool BF16>
__device__ __forceinline__ float round16(const float v) { return bits_to_float(float_to_bits<BF16>(v), BF16); }

template <bool BF16>
__device__ __forceinline__ float late16(const float v) { return v; }
template <bool BF16>
__device__ __forceinline__ float late16(const uint32_t b16) { return bits_to_float(b16, BF16); }

// RoPE of one (even, odd) pair (gpt-fast/model.py:apply_rotary_emb: x0 * cos - x1 * sin, x1 * cos + x0 * sin): the qkv
// projection's epilogue (teal_gemv_fast.h, ROPE) and the attention launches must agree bit for bit.
__device__ __forceinline__ float rope_even(float x0, float x1, float c, float s) { return fmaf(x0, c, -(x1 * s)); }
__device__ __forceinline__ float rope_odd(float x0, float x1, float c, float s) { return fmaf(x1, c, x0 * s); }

// h = h + round(sum of the projection's split-K slabs), rounded (gpt-fast/model.py:158-161: the residual adds)
template <bool BF16>
__device__ __forceinline__ float resid_add(const float r, const float slab_sum) { return round16<BF16>(r + round16<BF16>(slab_sum)); }

// round(a * b) of two 16-bit values: the second rounding of the RMSNorm and silu * up chains below.  A site whose guard
// ("this slot exists, else +0") sits between a chain's two roundings calls the chain's halves around it.
template <bool BF16, class B>
__device__ __forceinline__ uint16_t mul_bits(const float a16, const B b) { return float_to_bits<BF16>(a16 * late16<BF16>(b)); }

// x = round(round(h * rstd) * w) (gpt-fast/model.py:289-291: RMSNorm's `_norm(x.float()).type_as(x) * weight`); norm_scale is
// its first rounding
template <bool BF16>
__device__ __forceinline__ float norm_scale(const float h, const float rstd) { return round16<BF16>(h * rstd); }
template <bool BF16, class W>
__device__ __forceinline__ uint16_t norm_bits(const float h, const float rstd, const W w) {
    return mul_bits<BF16>(norm_scale<BF16>(h, rstd), w);
}

// silu(g) of a gate value that is a 16-bit value already, in fp32 (gpt-fast/model.py:258: F.silu(self.w1(x))), and rounded
__device__ __forceinline__ float silu32(const float g16) { return g16 / (1.0f + expf(-g16)); }
template <bool BF16>
__device__ __forceinline__ float silu16(const float g16) { return round16<BF16>(silu32(g16)); }

// round(round(silu(g)) * u) (gpt-fast/model.py:258-259: F.silu(self.w1(x)) * self.w3(x))
template <bool BF16, class U>
__device__ __forceinline__ uint16_t silu_mul_bits(const float g16, const U u) { return mul_bits<BF16>(silu16<BF16>(g16), u); }

// round(silu(round(sum))): the gate projection's output with the activation applied where it is computed (model.py:258)
template <bool BF16>
__device__ __forceinline__ uint16_t silu_bits(const float sum) { return float_to_bits<BF16>(silu32(round16<BF16>(sum))); }

// 1 / rms of the workgroup's vector (gpt-fast/model.py:289: torch.rsqrt(torch.mean(x * x) + eps)), second half: lane 0 of
// every wave has deposited wave_sum_f of its lanes' partial sums of squares in sumsq[wave] and the caller's barrier (with its
// phase stamps) has passed; every wave folds the WAVES deposits in wave order.  (The deposit — one predicated store — stays at
// the sites: as a function it moved the kernels' branches.)
template <int WAVES>
__device__ __forceinline__ float rms_rstd(const float* sumsq, const int lane, const int Z, const float eps) {
    float tot = (lane < WAVES) ? sumsq[lane] : 0.0f;
    tot = wave_sum_f(tot);
    return rsqrtf(tot / (float)Z + eps);
}

// ---- the split-KV merge producer (flash-decoding; gpt-fast/model.py:186 hands y = softmax(q k^T) v to wo): a head's NS
//      partials {max, sum, o[]} -> o = sum_q o_q * e^(m_q - M) * (1 / L), L = sum_q l_q e^(m_q - M) -------------------------
template <int CTRL>
__device__ __forceinline__ float dpp_f(const float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

// Lane j holds {max, sum} of split j % NS of a chunk; the bits of its normalised weight e^(m - M) / L, formed inside the
// group of NS lanes: quad_perm [1,0,3,2], quad_perm [2,3,0,1] and, for eight, row_half_mirror (lane i <-> 7 - i)
template <int NS>
__device__ __forceinline__ int merge_weight(const float2 st) {
    float M = fmaxf(st.x, dpp_f<0xB1>(st.x));
    M = fmaxf(M, dpp_f<0x4E>(M));
    if constexpr (NS == 8) M = fmaxf(M, dpp_f<0x141>(M));
    const float f = st.y > 0.0f ? expf(st.x - M) : 0.0f;
    float Ls = st.y * f;
    Ls += dpp_f<0xB1>(Ls);
    Ls += dpp_f<0x4E>(Ls);
    if constexpr (NS == 8) Ls += dpp_f<0x141>(Ls);
    return __float_as_int(f / Ls);
}

// A split that contributes nothing (empty: sum 0; or e^(m - M) underflowed) is skipped, as merge_head does (teal_attention.hip:
// `if (ls > 0)`): whatever its o holds, NaN included, stays out of the sum.  Every lane holds the weight of a (chunk, split) the
// wave uses, so one ballot tells whether any split is skipped at all: the usual case, none, keeps the unguarded chain
// (wave-uniform branch).
__device__ __forceinline__ bool merge_all_live(const int cw) { return __ballot(__int_as_float(cw) > 0.0f) == ~0ull; }

// the merged, rounded activation of chunk k from its NS partial outputs and the weights of lanes NS k .. NS k + NS - 1
template <bool BF16, int NS>
__device__ __forceinline__ uint16_t merge_bits(const float (&ov)[NS], const int cw, const int k, const bool all_live) {
    float Os = 0.0f;
    if (all_live) {
#pragma unroll
        for (int q = 0; q < NS; ++q) Os = fmaf(ov[q], __int_as_float(__builtin_amdgcn_readlane(cw, NS * k + q)), Os);
    } else {
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            const float wq = __int_as_float(__builtin_amdgcn_readlane(cw, NS * k + q));
            if (wq > 0.0f) Os = fmaf(ov[q], wq, Os);
        }
    }
    return float_to_bits<BF16>(Os);
}

}  // namespace teal
