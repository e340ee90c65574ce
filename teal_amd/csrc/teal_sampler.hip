// teal_sampler.hip — the fused top-k sampler and its C-ABI entry points (include/teal_hip.h).
//   gpt-fast/generate.py:49-66  logits_to_probs + multinomial_sample_one -> sample_topk*_kernel
#include "teal_common.h"

namespace teal {

// ------------------------------------------------------------------------------------------------
// Fused sampler (gpt-fast/generate.py:49-66): logits / T -> keep the top-k -> softmax -> exponential-
// race multinomial (argmax p_i / q_i, q_i ~ Exp(1)), no host sync.  One workgroup; the k-th largest
// logit is found EXACTLY by a two-pass radix select on the 16-bit keys (ties at the pivot are all
// kept, as `logits < pivot -> -inf` does).  Randomness: counter-based hash of (seed, draw counter,
// index); the draw counter lives on the device and is bumped by the kernel, so hipGraph replays
// draw fresh numbers.  Token streams are not pinned by the reference (they depend on torch's RNG).
// ------------------------------------------------------------------------------------------------
// (order_key16, hash3 and select_bin live in teal_common.h: the speculative accept kernel draws from the same stream)

template <bool BF16>
__device__ __forceinline__ void sample_full(const uint16_t* __restrict__ logits, const int V, const int top_k,
                                            const float inv_temp, unsigned long long* __restrict__ rng_state,
                                            int* __restrict__ token_out, int* __restrict__ pos_inout,
                                            int* __restrict__ history, const int history_len) {
    __shared__ unsigned int hist[256];
    __shared__ unsigned int whist[16][256];  // per-wave sub-histograms: logits cluster in a few bins, a single
                                             // shared histogram serialises on LDS atomics
    __shared__ float fred[16];
    __shared__ int ired[16];
    __shared__ unsigned int sel[2];
    __shared__ unsigned int suf[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool filter = top_k > 0 && top_k < V;
    const int V8 = V >> 3;  // 16-byte vectors (vocab sizes are multiples of 8; the tail is handled scalar)
    const u32x4* lv = reinterpret_cast<const u32x4*>(logits);
    uint32_t pivot_key = 0;  // keep keys >= pivot_key
    float mx = -INFINITY;
    for (int i = tid; i < 16 * 256; i += 1024) (&whist[0][0])[i] = 0;
    __syncthreads();
    // pass 1: high-byte histogram of the order-preserving 16-bit keys + global max
    for (int i = tid; i < V8; i += 1024) {
        const u32x4 w = lv[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t lo = w[j] & 0xFFFFu, hi = w[j] >> 16;
            mx = fmaxf(mx, fmaxf(bits_to_float(lo, BF16), bits_to_float(hi, BF16)));
            if (filter) {
                atomicAdd(&whist[wave][order_key16(lo, BF16) >> 8], 1u);
                atomicAdd(&whist[wave][order_key16(hi, BF16) >> 8], 1u);
            }
        }
    }
    for (int i = (V8 << 3) + tid; i < V; i += 1024) {
        mx = fmaxf(mx, bits_to_float(logits[i], BF16));
        if (filter) atomicAdd(&whist[wave][order_key16(logits[i], BF16) >> 8], 1u);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
    if (lane == 0) fred[wave] = mx;
    __syncthreads();
    if (tid < 256) {
        unsigned int a = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) a += whist[w][tid];
        hist[tid] = a;
    }
    __syncthreads();
    mx = fred[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) mx = fmaxf(mx, fred[w]);
    if (filter) {
        // suffix counts over the 256 bins (parallel scan), then the bin holding the top_k-th key
        select_bin(hist, suf, sel, (unsigned int)top_k, tid);
        __syncthreads();
        const unsigned int hb = sel[0], need2 = sel[1];
        __syncthreads();
        for (int i = tid; i < 16 * 256; i += 1024) (&whist[0][0])[i] = 0;
        __syncthreads();
        // pass 2: low-byte histogram inside the selected high-byte bin
        for (int i = tid; i < V8; i += 1024) {
            const u32x4 w = lv[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t k0 = order_key16(w[j] & 0xFFFFu, BF16), k1 = order_key16(w[j] >> 16, BF16);
                if ((k0 >> 8) == hb) atomicAdd(&whist[wave][k0 & 0xFFu], 1u);
                if ((k1 >> 8) == hb) atomicAdd(&whist[wave][k1 & 0xFFu], 1u);
            }
        }
        for (int i = (V8 << 3) + tid; i < V; i += 1024) {
            const uint32_t k = order_key16(logits[i], BF16);
            if ((k >> 8) == hb) atomicAdd(&whist[wave][k & 0xFFu], 1u);
        }
        __syncthreads();
        if (tid < 256) {
            unsigned int a = 0;
#pragma unroll
            for (int w = 0; w < 16; ++w) a += whist[w][tid];
            hist[tid] = a;
        }
        __syncthreads();
        select_bin(hist, suf, sel, need2, tid);
        if (tid == 0) sel[0] = (hb << 8) | sel[0];
        __syncthreads();
        pivot_key = sel[0];
    }
    // exponential race: argmax_i exp((x_i - max)/T) / q_i  over the kept set (the softmax
    // normaliser is common to all i and cannot change the argmax)
    const uint32_t seed = (uint32_t)rng_state[0], ctr = (uint32_t)rng_state[1];
    float best = -1.0f;
    int besti = 0x7FFFFFFF;
    auto consider = [&](const uint32_t b, const int i) {
        if (filter && order_key16(b, BF16) < pivot_key) return;
        const float pnum = expf((bits_to_float(b, BF16) - mx) * inv_temp);
        const float u = ((float)(hash3(seed, ctr, (uint32_t)i) >> 8) + 0.5f) * (1.0f / 16777216.0f);
        const float scv = pnum / (-logf(u));
        if (scv > best || (scv == best && i < besti)) { best = scv; besti = i; }
    };
    for (int i = tid; i < V8; i += 1024) {
        const u32x4 w = lv[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            consider(w[j] & 0xFFFFu, i * 8 + 2 * j);
            consider(w[j] >> 16, i * 8 + 2 * j + 1);
        }
    }
    for (int i = (V8 << 3) + tid; i < V; i += 1024) consider(logits[i], i);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float ob = __shfl_xor(best, d);
        const int oi = __shfl_xor(besti, d);
        if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
    }
    __syncthreads();
    if (lane == 0) { fred[wave] = best; ired[wave] = besti; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w)
            if (fred[w] > best || (fred[w] == best && ired[w] < besti)) { best = fred[w]; besti = ired[w]; }
        token_out[0] = besti;
        const unsigned long long c = rng_state[1];
        if (history && (long long)c < (long long)history_len) history[c] = besti;
        rng_state[1] = c + 1ull;
        if (pos_inout) pos_inout[0] = pos_inout[0] + 1;
    }
}

template <bool BF16>
__global__ __launch_bounds__(1024) void sample_topk_kernel(const uint16_t* __restrict__ logits, const int V,
                                                            const int top_k, const float inv_temp,
                                                            unsigned long long* __restrict__ rng_state,
                                                            int* __restrict__ token_out, int* __restrict__ pos_inout,
                                                            int* __restrict__ history, const int history_len) {
    sample_full<BF16>(logits, V, top_k, inv_temp, rng_state, token_out, pos_inout, history, history_len);
}

// the slot-predicated forms (teal_sample_topk_slot): bit `slot` of active[0] clear -> the whole launch exits before it reads or
// writes anything else
__device__ __forceinline__ bool slot_off(const int* __restrict__ active, const int slot) { return !((active[0] >> slot) & 1); }

template <bool BF16>
__global__ __launch_bounds__(1024) void sample_topk_slot_kernel(const uint16_t* __restrict__ logits, const int V,
                                                                 const int top_k, const float inv_temp,
                                                                 unsigned long long* __restrict__ rng_state,
                                                                 int* __restrict__ token_out, int* __restrict__ pos_inout,
                                                                 int* __restrict__ history, const int history_len,
                                                                 const int* __restrict__ active, const int slot) {
    if (slot_off(active, slot)) return;
    sample_full<BF16>(logits, V, top_k, inv_temp, rng_state, token_out, pos_inout, history, history_len);
}


// ------------------------------------------------------------------------------------------------
// Register-resident sampler for vocab % 8 == 0, vocab <= NV * 8192 (Llama-2: NV = 4, Llama-3: NV = 16).
// Phase stamps of the generic kernel above (scripts/sampler_phase.py): its time is the high-byte histogram
// pass — every key does an LDS atomic, and bf16 logits fall into 4-5 of the 256 high-byte bins (sign + 7
// exponent bits), so the atomics serialise: 45 of 72 us at vocab 128256 — plus dependent global loads in
// every pass and in the last thread's epilogue.  Here:
//   * every thread loads its NV vectors ONCE and keeps the order-preserving keys in registers;
//   * the k-th largest key is found in a WINDOW below the maximum: bin = (kmax - key) >> SH for the keys
//     within 256 << SH of kmax, everything further away does no atomic at all.  The top-k of a peaked
//     distribution sits within ~2 octaves of the maximum (SH = 0 for bf16, 3 for fp16), i.e. a few per cent of
//     the vocabulary, spread over 256 bins.  If the window holds fewer than k keys it is widened (SH += 3, up
//     to 8 where it covers every key) and the pass repeated; a bin wider than one key is resolved by a second
//     histogram of the low SH bits of its (few) members.  Exact: same pivot, ties kept, same tokens as the
//     generic kernel (tests/test_engine.py).
// ------------------------------------------------------------------------------------------------
template <bool BF16, int NV>
__device__ __forceinline__ void sample_window_body(const uint16_t* __restrict__ logits, const int V, const int top_k, const float inv_temp,
                                                   unsigned long long* __restrict__ rng_state, int* __restrict__ token_out,
                                                   int* __restrict__ pos_inout, int* __restrict__ history, const int history_len,
                                                   unsigned long long* __restrict__ phase) {
    auto stamp_s = [&](const int i) { if (phase && threadIdx.x == 0) phase[i] = wall_clock64(); };
    stamp_s(0);
    __shared__ unsigned int hist[256];
    __shared__ unsigned int whist[16][256];
    __shared__ float fred[16];
    __shared__ int ired[16];
    __shared__ unsigned int sel[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool filter = top_k > 0 && top_k < V;
    const int V8 = V >> 3;
    const u32x4* lv = reinterpret_cast<const u32x4*>(logits);
    u32x4 kv[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) kv[v] = lv[min(v * 1024 + tid, V8 - 1)];
    // everything the epilogue needs from memory is requested now, not by the last thread at the very end
    const unsigned long long seed64 = rng_state[0], ctr64 = rng_state[1];
    const int pos0 = pos_inout ? pos_inout[0] : 0;
    for (int i = tid; i < 16 * 256; i += 1024) (&whist[0][0])[i] = 0;
    uint32_t kmax = 0u;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const bool ok = v * 1024 + tid < V8;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t k0 = order_key16(kv[v][j] & 0xFFFFu, BF16), k1 = order_key16(kv[v][j] >> 16, BF16);
            kv[v][j] = ok ? (k0 | (k1 << 16)) : 0u;  // vectors past the vocabulary: key 0, never considered (index check)
            kmax = ok ? max(kmax, max(k0, k1)) : kmax;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, d));
    if (lane == 0) ired[wave] = (int)kmax;
    __syncthreads();
    kmax = (uint32_t)ired[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) kmax = max(kmax, (uint32_t)ired[w]);
    auto key_bits = [](const uint32_t k) -> uint32_t { return (k & 0x8000u) ? (k ^ 0x8000u) : (~k & 0xFFFFu); };  // order_key16^-1
    const float mx = bits_to_float(key_bits(kmax), BF16);
    stamp_s(1);
    auto merge_hist = [&]() {  // whist[16][256] -> hist[256]; barriers on both sides
        __syncthreads();
        if (tid < 256) {
            unsigned int a = 0;
#pragma unroll
            for (int w = 0; w < 16; ++w) a += whist[w][tid];
            hist[tid] = a;
        }
        __syncthreads();
    };
    uint32_t pivot_key = 0u;  // keep keys >= pivot_key
    if (filter) {
        for (int sh = BF16 ? 0 : 3;; sh += 3) {
            if (sh > 8) sh = 8;  // 256 << 8 covers every key
            // window pass: bin 255 = kmax, bin 255 - d = keys (d << sh) .. below it
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                if (v * 1024 + tid < V8) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t d0 = (kmax - (kv[v][j] & 0xFFFFu)) >> sh, d1 = (kmax - (kv[v][j] >> 16)) >> sh;
                        if (d0 < 256u) atomicAdd(&whist[wave][255u - d0], 1u);
                        if (d1 < 256u) atomicAdd(&whist[wave][255u - d1], 1u);
                    }
                }
            }
            merge_hist();
            unsigned int inwin = 0;  // keys inside the window (workgroup-uniform)
            {
                unsigned int a = (tid < 256) ? hist[tid] : 0u;
                a = (unsigned int)wave_sum_f((float)a);  // <= 131072: exact in fp32
                if (lane == 0) fred[wave] = (float)a;
                __syncthreads();
                inwin = (unsigned int)(fred[0] + fred[1] + fred[2] + fred[3]);
            }
            if (inwin >= (unsigned int)top_k || sh == 8) {
                select_bin(hist, nullptr, sel, (unsigned int)top_k, tid);
                const unsigned int d = 255u - sel[0], need2 = sel[1];
                __syncthreads();
                if (sh == 0) {
                    pivot_key = kmax - d;
                } else {
                    // resolve the bin: histogram of the low `sh` bits of its members (bin 255 = largest key)
                    for (int i = tid; i < 16 * 256; i += 1024) (&whist[0][0])[i] = 0;
                    __syncthreads();
                    const uint32_t lowmask = (1u << sh) - 1u;
#pragma unroll
                    for (int v = 0; v < NV; ++v) {
                        if (v * 1024 + tid < V8) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const uint32_t e0 = kmax - (kv[v][j] & 0xFFFFu), e1 = kmax - (kv[v][j] >> 16);
                                if ((e0 >> sh) == d) atomicAdd(&whist[wave][255u - (e0 & lowmask)], 1u);
                                if ((e1 >> sh) == d) atomicAdd(&whist[wave][255u - (e1 & lowmask)], 1u);
                            }
                        }
                    }
                    merge_hist();
                    select_bin(hist, nullptr, sel, need2, tid);
                    pivot_key = kmax - ((d << sh) | (255u - sel[0]));
                    __syncthreads();
                }
                break;
            }
            for (int i = tid; i < 16 * 256; i += 1024) (&whist[0][0])[i] = 0;  // widen the window and count again
            __syncthreads();
        }
    }
    stamp_s(2);
    // exponential race over the kept set (see sample_topk_kernel)
    const uint32_t seed = (uint32_t)seed64, ctr = (uint32_t)ctr64;
    float best = -1.0f;
    int besti = 0x7FFFFFFF;
    auto consider = [&](const uint32_t key, const int i) {
        if (key < pivot_key) return;
        const float pnum = expf((bits_to_float(key_bits(key), BF16) - mx) * inv_temp);
        const float u = ((float)(hash3(seed, ctr, (uint32_t)i) >> 8) + 0.5f) * (1.0f / 16777216.0f);
        const float scv = pnum / (-logf(u));
        if (scv > best || (scv == best && i < besti)) { best = scv; besti = i; }
    };
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int i = v * 1024 + tid;
        if (i < V8) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                consider(kv[v][j] & 0xFFFFu, i * 8 + 2 * j);
                consider(kv[v][j] >> 16, i * 8 + 2 * j + 1);
            }
        }
    }
    stamp_s(3);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float ob = __shfl_xor(best, d);
        const int oi = __shfl_xor(besti, d);
        if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
    }
    __syncthreads();
    if (lane == 0) { fred[wave] = best; ired[wave] = besti; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w)
            if (fred[w] > best || (fred[w] == best && ired[w] < besti)) { best = fred[w]; besti = ired[w]; }
        token_out[0] = besti;
        if (history && (long long)ctr64 < (long long)history_len) history[ctr64] = besti;
        rng_state[1] = ctr64 + 1ull;
        if (pos_inout) pos_inout[0] = pos0 + 1;
    }
    stamp_s(4);
}

template <bool BF16, int NV>
__global__ __launch_bounds__(1024) void sample_topk_window_kernel(const uint16_t* __restrict__ logits, const int V,
                                                                   const int top_k, const float inv_temp,
                                                                   unsigned long long* __restrict__ rng_state,
                                                                   int* __restrict__ token_out, int* __restrict__ pos_inout,
                                                                   int* __restrict__ history, const int history_len,
                                                                   unsigned long long* __restrict__ phase) {
    sample_window_body<BF16, NV>(logits, V, top_k, inv_temp, rng_state, token_out, pos_inout, history, history_len, phase);
}

template <bool BF16, int NV>
__global__ __launch_bounds__(1024) void sample_topk_window_slot_kernel(const uint16_t* __restrict__ logits, const int V,
                                                                        const int top_k, const float inv_temp,
                                                                        unsigned long long* __restrict__ rng_state,
                                                                        int* __restrict__ token_out, int* __restrict__ pos_inout,
                                                                        int* __restrict__ history, const int history_len,
                                                                        const int* __restrict__ active, const int slot) {
    if (slot_off(active, slot)) return;
    sample_window_body<BF16, NV>(logits, V, top_k, inv_temp, rng_state, token_out, pos_inout, history, history_len, nullptr);
}

// ------------------------------------------------------------------------------------------------
// Multi-workgroup sampler (vocab % 8 == 0, vocab <= 16 x 8192, 0 < top_k < vocab): the single workgroup above spends
// its time in NV sequential passes over its registers (14 us at 32 k, 37 us at 128 k logits).  Here workgroup g owns
// 8192 logits (one 16-byte vector per thread) and
//   stage A  bounds ITS k-th largest key from below with one pass of the same window select (the lower edge of the
//            histogram bin that holds it) and appends every key >= that bound, with its index, to a candidate list
//            in global memory (write-through stores), then takes an arrival ticket;
//   stage B  (the last workgroup to arrive) reads the <= G x kSampCap candidates, finds the global pivot among them,
//            and runs the exponential race over the candidates that survive it.
// Exact: a key >= the global pivot P is >= its chunk's pivot (the k-th largest of a subset is <= the k-th largest of
// the whole) and so >= the chunk's bound: the union of the candidate sets contains every key >= P, hence its k-th
// largest is P; the race
// uses the same counter-based random numbers by vocabulary index and the same tie-break as the single-workgroup
// kernels, so the tokens are identical (tests/test_engine.py).  A chunk with more than kSampCap candidates (top_k
// beyond the cap, or massive ties) raises an overflow flag and the last arriver runs the generic two-pass select over
// the whole vocabulary instead.
// ------------------------------------------------------------------------------------------------
// k-th largest of the keys this workgroup's threads hold (NK per thread, absent entries flagged in `valid` bits): the
// window select of sample_topk_window_kernel.  All 1024 threads call; returns the pivot key (keep keys >= pivot).
// COARSE: return the lower edge of the histogram bin that holds the k-th largest key instead of resolving the bin — a
// bound BELOW the exact pivot (a superset of the top-k, by up to one bin of 1 << sh keys), one pass cheaper.
template <bool BF16, int NK, bool COARSE = false>
__device__ __forceinline__ uint32_t window_pivot(const uint32_t (&keys)[NK], const uint32_t valid, const uint32_t kmax,
                                                 const unsigned int top_k, unsigned int* hist, unsigned int (*whist)[256],
                                                 float* fred, unsigned int* sel, const int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    auto merge_hist = [&]() {
        __syncthreads();
        if (tid < 256) {
            unsigned int a = 0;
#pragma unroll
            for (int w = 0; w < 16; ++w) a += whist[w][tid];
            hist[tid] = a;
        }
        __syncthreads();
    };
    uint32_t pivot_key = 0u;
    for (int i = tid; i < 16 * 256; i += 1024) (&whist[0][0])[i] = 0;
    __syncthreads();
    for (int sh = BF16 ? 0 : 3;; sh += 3) {
        if (sh > 8) sh = 8;  // 256 << 8 covers every key
#pragma unroll
        for (int j = 0; j < NK; ++j) {
            const uint32_t d = (kmax - keys[j]) >> sh;
            if (((valid >> j) & 1u) && d < 256u) atomicAdd(&whist[wave][255u - d], 1u);
        }
        merge_hist();
        unsigned int inwin = 0;
        {
            unsigned int a = (tid < 256) ? hist[tid] : 0u;
            a = (unsigned int)wave_sum_f((float)a);  // <= 131072: exact in fp32
            if (lane == 0) fred[wave] = (float)a;
            __syncthreads();
            inwin = (unsigned int)(fred[0] + fred[1] + fred[2] + fred[3]);
        }
        if (inwin >= top_k || sh == 8) {
            select_bin(hist, nullptr, sel, top_k, tid);
            const unsigned int d = 255u - sel[0], need2 = sel[1];
            __syncthreads();
            if (sh == 0) {
                pivot_key = kmax - d;
            } else if (COARSE) {
                const uint32_t span = ((d + 1u) << sh) - 1u;  // kmax - key <= span for every key of bins 0..d
                pivot_key = span >= kmax ? 0u : kmax - span;
            } else {
                for (int i = tid; i < 16 * 256; i += 1024) (&whist[0][0])[i] = 0;
                __syncthreads();
                const uint32_t lowmask = (1u << sh) - 1u;
#pragma unroll
                for (int j = 0; j < NK; ++j) {
                    const uint32_t e = kmax - keys[j];
                    if (((valid >> j) & 1u) && (e >> sh) == d) atomicAdd(&whist[wave][255u - (e & lowmask)], 1u);
                }
                merge_hist();
                select_bin(hist, nullptr, sel, need2, tid);
                pivot_key = kmax - ((d << sh) | (255u - sel[0]));
                __syncthreads();
            }
            break;
        }
        for (int i = tid; i < 16 * 256; i += 1024) (&whist[0][0])[i] = 0;  // widen the window and count again
        __syncthreads();
    }
    return pivot_key;
}

__device__ __forceinline__ uint32_t block_max_u32(uint32_t v, int* ired, const int tid) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d));
    __syncthreads();  // ired may still be read from a previous use
    if (lane == 0) ired[wave] = (int)v;
    __syncthreads();
    v = (uint32_t)ired[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) v = max(v, (uint32_t)ired[w]);
    return v;
}

template <bool BF16>
__device__ __forceinline__ void sample_multi_body(const uint16_t* __restrict__ logits, const int V, const int top_k, const float inv_temp,
                                                  unsigned long long* __restrict__ rng_state, int* __restrict__ token_out,
                                                  int* __restrict__ pos_inout, int* __restrict__ history, const int history_len,
                                                  unsigned char* __restrict__ slot) {
    __shared__ unsigned int hist[256];
    __shared__ unsigned int whist[16][256];
    __shared__ float fred[16];
    __shared__ int ired[16];
    __shared__ unsigned int sel[2];
    __shared__ unsigned int lcnt;
    __shared__ unsigned int lflag;
    __shared__ unsigned int gcount[kSampMaxGroups];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = blockIdx.x, G = gridDim.x;
    const int V8 = V >> 3;
    unsigned long long* cand = reinterpret_cast<unsigned long long*>(slot);
    unsigned int* counts = reinterpret_cast<unsigned int*>(slot + (size_t)kSampMaxGroups * kSampCap * 8);
    unsigned int* ticket = counts + kSampMaxGroups;
    // ---- stage A: this workgroup's 8192 logits -------------------------------------------------------------
    const int vi = g * 1024 + tid;
    const bool ok = vi < V8;
    const u32x4 raw = reinterpret_cast<const u32x4*>(logits)[min(vi, V8 - 1)];
    // what the last arriver's epilogue needs from memory is requested now
    const unsigned long long seed64 = rng_state[0], ctr64 = rng_state[1];
    const int pos0 = pos_inout ? pos_inout[0] : 0;
    if (tid == 0) lcnt = 0u;
    uint32_t keys[8];
    uint32_t kmax = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        keys[2 * j] = order_key16(raw[j] & 0xFFFFu, BF16);
        keys[2 * j + 1] = order_key16(raw[j] >> 16, BF16);
        if (ok) kmax = max(kmax, max(keys[2 * j], keys[2 * j + 1]));
    }
    kmax = block_max_u32(kmax, ired, tid);
    const unsigned int chunk_keys = (unsigned int)(min(V8 - g * 1024, 1024) * 8);
    // fewer keys in the chunk than requested: every key is a candidate (and overflows the cap: generic path)
    const uint32_t lpivot = chunk_keys <= (unsigned int)top_k ? 0u
                            : window_pivot<BF16, 8, true>(keys, ok ? 0xFFu : 0u, kmax, (unsigned int)top_k, hist, whist, fred, sel, tid);
    __syncthreads();
    if (ok) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (keys[j] >= lpivot) {
                const unsigned int s = atomicAdd(&lcnt, 1u);
                if (s < (unsigned int)kSampCap)
                    __hip_atomic_store(&cand[(size_t)g * kSampCap + s], ((unsigned long long)keys[j] << 32) | (unsigned int)(vi * 8 + j),
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    __syncthreads();
    if (tid == 0) __hip_atomic_store(&counts[g], lcnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // arrival ticket (see gemv_fast_kernel): the stores above are write-through and complete before the increment
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        lflag = (t == (unsigned)G - 1u) ? 1u : 0u;
    }
    __syncthreads();
    if (lflag == 0u) return;
    // ---- stage B: the last arriver ---------------------------------------------------------------------------
    if (tid == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm for the next launch / replay
    constexpr int NC = kSampMaxGroups * kSampCap / 1024;  // candidate slots per thread
    unsigned long long craw[NC];  // requested together with the counts (one round trip); slots past a count are stale
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int sidx = j * 1024 + tid;
        craw[j] = sidx / kSampCap < G ? __hip_atomic_load(&cand[sidx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    }
    if (tid < kSampMaxGroups) gcount[tid] = tid < G ? __hip_atomic_load(&counts[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    __syncthreads();
    bool overflow = false;
#pragma unroll
    for (int q = 0; q < kSampMaxGroups; ++q) overflow |= gcount[q] > (unsigned int)kSampCap;
    if (overflow) {  // workgroup-uniform
        sample_full<BF16>(logits, V, top_k, inv_temp, rng_state, token_out, pos_inout, history, history_len);
        return;
    }
    uint32_t ck[NC], ci[NC], cvalid = 0u;
    uint32_t gmax = 0u;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int sidx = j * 1024 + tid, gq = sidx / kSampCap, jj = sidx % kSampCap;
        ck[j] = 0u; ci[j] = 0u;
        if (gq < G && (unsigned int)jj < gcount[gq]) {
            ck[j] = (uint32_t)(craw[j] >> 32); ci[j] = (uint32_t)craw[j];
            cvalid |= 1u << j;
            gmax = max(gmax, ck[j]);
        }
    }
    gmax = block_max_u32(gmax, ired, tid);
    const uint32_t pivot = window_pivot<BF16, NC>(ck, cvalid, gmax, (unsigned int)top_k, hist, whist, fred, sel, tid);
    auto key_bits = [](const uint32_t k) -> uint32_t { return (k & 0x8000u) ? (k ^ 0x8000u) : (~k & 0xFFFFu); };  // order_key16^-1
    const float mx = bits_to_float(key_bits(gmax), BF16);
    const uint32_t seed = (uint32_t)seed64, ctr = (uint32_t)ctr64;
    float best = -1.0f;
    int besti = 0x7FFFFFFF;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        if (((cvalid >> j) & 1u) && ck[j] >= pivot) {
            const int i = (int)ci[j];
            const float pnum = expf((bits_to_float(key_bits(ck[j]), BF16) - mx) * inv_temp);
            const float u = ((float)(hash3(seed, ctr, (uint32_t)i) >> 8) + 0.5f) * (1.0f / 16777216.0f);
            const float scv = pnum / (-logf(u));
            if (scv > best || (scv == best && i < besti)) { best = scv; besti = i; }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float ob = __shfl_xor(best, d);
        const int oi = __shfl_xor(besti, d);
        if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
    }
    __syncthreads();
    if (lane == 0) { fred[wave] = best; ired[wave] = besti; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w)
            if (fred[w] > best || (fred[w] == best && ired[w] < besti)) { best = fred[w]; besti = ired[w]; }
        token_out[0] = besti;
        if (history && (long long)ctr64 < (long long)history_len) history[ctr64] = besti;
        rng_state[1] = ctr64 + 1ull;
        if (pos_inout) pos_inout[0] = pos0 + 1;
    }
}

template <bool BF16>
__global__ __launch_bounds__(1024) void sample_topk_multi_kernel(const uint16_t* __restrict__ logits, const int V,
                                                                  const int top_k, const float inv_temp,
                                                                  unsigned long long* __restrict__ rng_state,
                                                                  int* __restrict__ token_out, int* __restrict__ pos_inout,
                                                                  int* __restrict__ history, const int history_len,
                                                                  unsigned char* __restrict__ slot) {
    sample_multi_body<BF16>(logits, V, top_k, inv_temp, rng_state, token_out, pos_inout, history, history_len, slot);
}

// every workgroup reads the same word and takes the same exit decision, before the ticket
template <bool BF16>
__global__ __launch_bounds__(1024) void sample_topk_multi_slot_kernel(const uint16_t* __restrict__ logits, const int V,
                                                                       const int top_k, const float inv_temp,
                                                                       unsigned long long* __restrict__ rng_state,
                                                                       int* __restrict__ token_out, int* __restrict__ pos_inout,
                                                                       int* __restrict__ history, const int history_len,
                                                                       unsigned char* __restrict__ scratch, const int* __restrict__ active,
                                                                       const int slot) {
    if (slot_off(active, slot)) return;
    sample_multi_body<BF16>(logits, V, top_k, inv_temp, rng_state, token_out, pos_inout, history, history_len, scratch);
}

}  // namespace teal

using namespace teal;

namespace {
// teal_sample_topk_ws (active == nullptr) and teal_sample_topk_slot: the same kernel choice, the slot forms of the same kernels
int sample_launch(const void* logits, int vocab, int dtype, int top_k, float temperature, void* rng_state, int32_t* token_out,
                  int32_t* pos_inout, int32_t* history, int history_len, void* ws, size_t ws_bytes, const int32_t* active, int slot_id,
                  void* stream) {
    if (!logits || !rng_state || !token_out || vocab <= 0) return TEAL_ERR_ARG;
    if (dtype != TEAL_F16 && dtype != TEAL_BF16) return TEAL_ERR_DTYPE;
    if (!aligned16(logits)) return TEAL_ERR_ALIGN;
    const float inv_temp = 1.0f / fmaxf(temperature, 1e-5f);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    auto* lg = reinterpret_cast<const uint16_t*>(logits);
    auto* rs = reinterpret_cast<unsigned long long*>(rng_state);
#define TEAL_SAMPLE(KERNEL) hipLaunchKernelGGL((KERNEL), dim3(1), dim3(1024), 0, st, lg, vocab, top_k, inv_temp, rs, token_out, pos_inout, history, history_len)
#define TEAL_SAMPLE_W(KERNEL) hipLaunchKernelGGL((KERNEL), dim3(1), dim3(1024), 0, st, lg, vocab, top_k, inv_temp, rs, token_out, pos_inout, history, history_len, phase_start_only())
#define TEAL_SAMPLE_S(KERNEL) hipLaunchKernelGGL((KERNEL), dim3(1), dim3(1024), 0, st, lg, vocab, top_k, inv_temp, rs, token_out, pos_inout, history, history_len, active, slot_id)
    const bool bf = dtype == TEAL_BF16;
    if ((vocab & 7) == 0 && vocab > 8192 && vocab <= kSampMaxGroups * 8192 && top_k > 0 && top_k < vocab && ws_prepared(ws, ws_bytes)) {
        // one workgroup per 8192 logits + the last arriver (sample_topk_multi_kernel)
        unsigned char* slot = ws_sampler(ws);  // scratch of the caller's prepared workspace (one per stream)
        const dim3 grid((vocab / 8 + 1023) / 1024), block(1024);
        if (active) {
            if (bf) hipLaunchKernelGGL((sample_topk_multi_slot_kernel<true>), grid, block, 0, st, lg, vocab, top_k, inv_temp, rs, token_out, pos_inout, history, history_len, slot, active, slot_id);
            else hipLaunchKernelGGL((sample_topk_multi_slot_kernel<false>), grid, block, 0, st, lg, vocab, top_k, inv_temp, rs, token_out, pos_inout, history, history_len, slot, active, slot_id);
        } else {
            if (bf) hipLaunchKernelGGL((sample_topk_multi_kernel<true>), grid, block, 0, st, lg, vocab, top_k, inv_temp, rs, token_out, pos_inout, history, history_len, slot);
            else hipLaunchKernelGGL((sample_topk_multi_kernel<false>), grid, block, 0, st, lg, vocab, top_k, inv_temp, rs, token_out, pos_inout, history, history_len, slot);
        }
    } else if ((vocab & 7) == 0 && vocab <= 4 * 8192) {  // register-resident keys, window select: 4 vectors per thread
        if (active) { if (bf) TEAL_SAMPLE_S((sample_topk_window_slot_kernel<true, 4>)); else TEAL_SAMPLE_S((sample_topk_window_slot_kernel<false, 4>)); }
        else if (bf) TEAL_SAMPLE_W((sample_topk_window_kernel<true, 4>)); else TEAL_SAMPLE_W((sample_topk_window_kernel<false, 4>));
    } else if ((vocab & 7) == 0 && vocab <= 16 * 8192) {  // 16 vectors per thread (Llama-3's 128256)
        if (active) { if (bf) TEAL_SAMPLE_S((sample_topk_window_slot_kernel<true, 16>)); else TEAL_SAMPLE_S((sample_topk_window_slot_kernel<false, 16>)); }
        else if (bf) TEAL_SAMPLE_W((sample_topk_window_kernel<true, 16>)); else TEAL_SAMPLE_W((sample_topk_window_kernel<false, 16>));
    } else {  // any size: two full radix passes over memory
        if (active) { if (bf) TEAL_SAMPLE_S((sample_topk_slot_kernel<true>)); else TEAL_SAMPLE_S((sample_topk_slot_kernel<false>)); }
        else if (bf) TEAL_SAMPLE((sample_topk_kernel<true>)); else TEAL_SAMPLE((sample_topk_kernel<false>));
    }
#undef TEAL_SAMPLE
#undef TEAL_SAMPLE_W
#undef TEAL_SAMPLE_S
    return hipGetLastError() == hipSuccess ? TEAL_OK : TEAL_ERR_LAUNCH;
}
}  // namespace

extern "C" {

int teal_sample_topk_ws(const void* logits, int vocab, int dtype, int top_k, float temperature, void* rng_state,
                        int32_t* token_out, int32_t* pos_inout, int32_t* history, int history_len, void* ws, size_t ws_bytes,
                        void* stream) {
    return sample_launch(logits, vocab, dtype, top_k, temperature, rng_state, token_out, pos_inout, history, history_len, ws, ws_bytes,
                         nullptr, 0, stream);
}

int teal_sample_topk_slot(const void* logits, int vocab, int dtype, int top_k, float temperature, void* rng_state, int32_t* token_out,
                          int32_t* pos_inout, int32_t* history, int history_len, void* ws, size_t ws_bytes, const int32_t* active, int slot,
                          void* stream) {
    if (!active || slot < 0 || slot > 31) return TEAL_ERR_ARG;
    return sample_launch(logits, vocab, dtype, top_k, temperature, rng_state, token_out, pos_inout, history, history_len, ws, ws_bytes,
                         active, slot, stream);
}

int teal_sample_topk(const void* logits, int vocab, int dtype, int top_k, float temperature, void* rng_state,
                     int32_t* token_out, int32_t* pos_inout, int32_t* history, int history_len, void* stream) {
    return teal_sample_topk_ws(logits, vocab, dtype, top_k, temperature, rng_state, token_out, pos_inout, history, history_len,
                               nullptr, 0, stream);
}

}  // extern "C"
