// teal_draw.h — the sampler's random stream, selection and draw: ONE copy of each rule that the fused sampler (teal_sampler.hip), the
// per-request sampler (teal_sample_rows.hip) and the speculative accept step (teal_speculative.hip) share.  A draw is the exponential
// race  argmax_i expf((x_i - max) * inv_temp) / -logf(u_i),  u_i = uniform01(hash3(seed, ctr, i)),  over the kept logits; the lower
// index wins an exact tie and thread 0 files the winner.  Internal header.
#pragma once
#include "teal_common.h"

namespace teal {

// ---- selection: order-preserving 16-bit keys and the bin that holds the k-th largest ----
__device__ __forceinline__ uint32_t order_key16(uint32_t b, bool bf16) {
    (void)bf16;  // fp16 and bf16 share sign-magnitude ordering
    const uint32_t k = (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
    // -0.0 (the only pattern that keys 0x7FFF) is the VALUE +0.0 and takes its key: a pivot on zero keeps both zeros, as
    // `logits < pivot` does (tests/test_sampler_rule.py).  Written on the key: mapping the pattern first costs the
    // 16-vector window kernel 14 more spilled VGPRs.
    return k + (k == 0x7FFFu ? 1u : 0u);
}

// the 16-bit pattern of a key: the inverse of order_key16 (-0.0 has no key of its own and comes back as +0.0)
__device__ __forceinline__ uint32_t key_bits16(const uint32_t k) { return (k & 0x8000u) ? (k ^ 0x8000u) : (~k & 0xFFFFu); }

// whist[16][256] (one sub-histogram per wave) -> hist[256], by threads 0..255.  The barriers on both sides are the caller's.
template <typename T>
__device__ __forceinline__ void merge_whist(const T (*whist)[256], T* hist, const int tid) {
    if (tid < 256) {
        T a = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) a += whist[w][tid];
        hist[tid] = a;
    }
}

// sel[0] = the bin b in which the `need`-th largest key falls, sel[1] = its rank inside that bin.  One wave does
// it without workgroup barriers (lane l owns bins 4l..4l+3, suffix sums over lanes by shuffles): the Hillis-Steele
// scan over 1024 threads it replaces cost 18 barriers per call, and barriers were most of this kernel's time.
// All threads must call this; hist[] must be complete (barrier before), sel[] is valid after the trailing barrier.
__device__ __forceinline__ void select_bin(const unsigned int* hist, unsigned int* sel, const unsigned int need, const int tid) {
    if (tid < 64) {
        const unsigned int h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
        const unsigned int own = h0 + h1 + h2 + h3;
        unsigned int incl = own;  // keys in this lane's bins and all higher lanes'
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned int t = (unsigned int)__shfl_down((int)incl, d);
            if (tid + d < 64) incl += t;
        }
        // keys in strictly higher bins, for each of the four bins (highest first)
        const unsigned int a3 = incl - own, a2 = a3 + h3, a1 = a2 + h2, a0 = a1 + h1;
        if (a3 + h3 >= need && a3 < need) { sel[0] = 4u * tid + 3u; sel[1] = need - a3; }
        if (a2 + h2 >= need && a2 < need) { sel[0] = 4u * tid + 2u; sel[1] = need - a2; }
        if (a1 + h1 >= need && a1 < need) { sel[0] = 4u * tid + 1u; sel[1] = need - a1; }
        if (a0 + h0 >= need && a0 < need) { sel[0] = 4u * tid; sel[1] = need - a0; }
        if (tid == 0 && incl < need) { sel[0] = 0u; sel[1] = need; }  // fewer keys than requested: keep all
    }
    __syncthreads();
}

// ---- the random stream: counter-based, one 32-bit word per (seed, draw counter, index) ----
__device__ __forceinline__ uint32_t hash3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t h = a * 0x9E3779B1u ^ (b + 0x7F4A7C15u) * 0x85EBCA77u ^ (c + 0x165667B1u) * 0xC2B2AE3Du;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

// the word's top 24 bits, centred in their cell: ((h >> 8) + 0.5) * 2^-24, evaluated in fp32
__device__ __forceinline__ float uniform01(const uint32_t h) { return ((float)(h >> 8) + 0.5f) * (1.0f / 16777216.0f); }

// ---- the race ----
// the score of index i, whose unnormalised weight is pnum = expf((x_i - max) * inv_temp): pnum / q_i, q_i = -logf(u_i) ~ Exp(1)
// (the softmax normaliser is common to all i and cannot change the argmax)
__device__ __forceinline__ float race_score(const float pnum, const uint32_t seed, const uint32_t ctr, const int i) {
    return pnum / (-logf(uniform01(hash3(seed, ctr, (uint32_t)i))));
}

// (s, i) takes the lead from (best, besti): the larger score, on an exact tie the lower index
__device__ __forceinline__ void race_take(float& best, int& besti, const float s, const int i) {
    if (s > best || (s == best && i < besti)) { best = s; besti = i; }
}

// The rest of a draw is written out in each kernel, because as functions these two pieces changed the kernels' instructions
// (profiles/sampler_draw_refactor.txt).  Every copy must read:
//   the block reduce   six __shfl_xor steps (32 .. 1) of race_take on (best, besti); a barrier; lane 0 of each wave deposits its
//                      pair in fred[wave] / ired[wave]; a barrier; thread 0 scans waves 1 .. 15 with race_take's comparison
//   the commit         by thread 0: the token word; the history entry filed under the draw counter, if the counter is below
//                      history_len; counter + 1; position + 1, if a position is kept

}  // namespace teal
