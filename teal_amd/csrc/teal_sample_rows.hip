// teal_sample_rows.hip — per-request sampling and its C-ABI entry point (include/teal_hip.h): ONE launch draws the tokens of all
// B rows of a step, each row under its own {temperature, top_k, top_p, min_p}, read from device memory and predicated per slot.
//
// The rule (include/teal_hip.h states it in full, tests/sampling_rule.py restates it on the host).  Every filter keeps the logits
// whose VALUE is not below a threshold, and the maximum passes all of them, so the kept sets are nested and one pivot — the
// largest of the filters' pivots — says which logits enter the race:
//
//   t_i = fl(fl(x_i - max) * inv),  inv = 1 / max(temperature, 1e-5)                  (sample_full's expression)
//   top_k   0 < k < V: every logit not below the k-th largest value (ties kept) -> the set K1
//   top_p   < 1: over K1, w_i = expf(t_i), Z = sum w, A(v) = mass of the values above v: v stays iff A(v) < top_p * Z
//   min_p   > 0: v stays iff expf(t) >= min_p
//   race    argmax expf(t_i) / -logf(u_i) over what stayed — consider()'s fp32 expression of teal_sampler.hip, the same hash3
//           stream, the smallest index winning exact ties, and the same epilogue
//
// How: one workgroup of 1024 threads per row.  A thread loads its NV 16-byte vectors once and keeps the order-preserving 16-bit
// keys in registers (sample_window_body's layout).  With d = kmax - key (0 at the maximum) both selections are the same question,
// "the smallest d whose cumulative weight over d' <= d reaches `need`", asked with weight 1 and need = top_k for the top-k pivot
// and with weight = mass and need = top_p * Z for the top-p pivot (A(v) < top_p * Z for exactly the d up to that one).  It is
// answered exactly by a two-pass radix select: a histogram of d >> 8, the bin where the cumulative weight crosses, then a
// histogram of d & 255 inside that bin.
//
// Masses are summed as 64-bit fixed-point integers, q_i = trunc(expf(t_i) * 2^40) (<= 2^40, a row's total <= 2^57), by integer
// LDS atomics: integer addition is associative, so a row's sums — and with them its kept set and its token — do not depend on
// the order the atomics land in, on B, on the slot or on the replay.  A term loses less than 2^-40 to the truncation (nothing
// at all from 2^-17 up, where fp32's last place is worth at least 2^-40), a row less than 131072 * 2^-40 = 2^-23 against Z >= 1
// (the maximum's own mass is 1); the product top_p * Z is formed in fp64.  So of the 1e-5 * Z margin within which
// tests/sampling_rule.py calls a top-p decision open (about 168 * 2^-24) all but 2 * 2^-24 is left to expf's own error on every
// term at once.  The toolchain documents no bound for expf, so the margin stays where the rule puts it instead of being tightened
// to a guess.
//
// min_p needs no pivot: it is one comparison on the race's own expf(t_i).
#include "teal_common.h"

namespace teal {

typedef unsigned long long u64;

constexpr float kMassScale = 1099511627776.0f;  // 2^40

// hist[256] complete (barrier before) -> the smallest bin b with hist[0] + .. + hist[b] >= need: sel[0] = b, sel[1] = need less
// the weight of the bins below b (what the next level has to reach inside b).  frac >= 0: need = max(1, ceil(frac * total)).  The
// total does not reach need: b = 255 (so does the next level: every key is kept).  One wave, lane l owns bins 4l .. 4l+3 (the
// scheme of select_bin, in prefix order and 64 bits wide).  All threads call; sel[] is valid after the trailing barrier.
__device__ __forceinline__ void select_prefix(const u64* hist, u64* sel, u64 need, const double frac, const int tid) {
    if (tid < 64) {
        const u64 h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
        const u64 own = h0 + h1 + h2 + h3;
        u64 incl = own;  // weight of this lane's bins and all lower lanes'
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u64 t = __shfl_up(incl, d);
            if (tid >= d) incl += t;
        }
        const u64 total = __shfl(incl, 63);
        if (frac >= 0.0) {
            const double want = ceil(frac * (double)total);
            need = want < 1.0 ? 1ull : (u64)want;
        }
        const u64 e0 = incl - own, e1 = e0 + h0, e2 = e1 + h1, e3 = e2 + h2;
        if (e0 < need && e0 + h0 >= need) { sel[0] = 4ull * tid; sel[1] = need - e0; }
        if (e1 < need && e1 + h1 >= need) { sel[0] = 4ull * tid + 1ull; sel[1] = need - e1; }
        if (e2 < need && e2 + h2 >= need) { sel[0] = 4ull * tid + 2ull; sel[1] = need - e2; }
        if (e3 < need && e3 + h3 >= need) { sel[0] = 4ull * tid + 3ull; sel[1] = need - e3; }
        if (tid == 63 && total < need) { sel[0] = 255ull; sel[1] = need - e3; }
    }
    __syncthreads();
}

template <bool BF16, int NV>
__global__ __launch_bounds__(1024) void sample_rows_kernel(const uint16_t* __restrict__ logits, const size_t stride, const int V,
                                                            const uint32_t* __restrict__ params, u64* __restrict__ rng_state,
                                                            int* __restrict__ tokens, int* __restrict__ pos, int* __restrict__ history,
                                                            const int history_len, int* __restrict__ kept_out,
                                                            const int* __restrict__ active, const int slot0) {
    const int r = blockIdx.x;
    if (active && !((active[0] >> (slot0 + r)) & 1)) return;  // (workgroup-uniform: before any barrier, load or store)
    __shared__ u64 hist[256];
    __shared__ u64 whist[16][256];  // per-wave sub-histograms (sample_full's reason: the keys cluster in a few bins)
    __shared__ u64 sel[2];
    __shared__ float fred[16];
    __shared__ int ired[16];
    __shared__ int kred[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V8 = V >> 3;
    const u32x4* lv = reinterpret_cast<const u32x4*>(logits + (size_t)r * stride);
    u32x4 kv[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) kv[v] = lv[min(v * 1024 + tid, V8 - 1)];
    // everything else the row needs from memory is requested now
    const float temperature = __uint_as_float(params[4 * r]);
    const int top_k = (int)params[4 * r + 1];
    const float top_p = __uint_as_float(params[4 * r + 2]), min_p = __uint_as_float(params[4 * r + 3]);
    const u64 seed64 = rng_state[2 * r], ctr64 = rng_state[2 * r + 1];
    const int pos0 = pos ? pos[r] : 0;
    const float inv_temp = __fdiv_rn(1.0f, fmaxf(temperature, 1e-5f));
    uint32_t kmax = 0u;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const bool ok = v * 1024 + tid < V8;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t k0 = order_key16(kv[v][j] & 0xFFFFu, BF16), k1 = order_key16(kv[v][j] >> 16, BF16);
            kv[v][j] = ok ? (k0 | (k1 << 16)) : 0u;  // vectors past the vocabulary are never visited (for_keys)
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
    // f(key, vocabulary index) for every key this thread holds
    auto for_keys = [&](auto f) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int i = v * 1024 + tid;
            if (i < V8) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    f(kv[v][j] & 0xFFFFu, i * 8 + 2 * j);
                    f(kv[v][j] >> 16, i * 8 + 2 * j + 1);
                }
            }
        }
    };
    auto zero_whist = [&]() {  // (the barrier also keeps the previous select's readers of hist / sel ahead of the next writers)
        __syncthreads();
        for (int i = tid; i < 16 * 256; i += 1024) (&whist[0][0])[i] = 0ull;
        __syncthreads();
    };
    auto merge_hist = [&]() {  // whist[16][256] -> hist[256]; barriers on both sides
        __syncthreads();
        if (tid < 256) {
            u64 a = 0ull;
#pragma unroll
            for (int w = 0; w < 16; ++w) a += whist[w][tid];
            hist[tid] = a;
        }
        __syncthreads();
    };
    // the smallest d = kmax - key at which the cumulative weight reaches the need; weight(key, d) == 0: the key takes no part
    auto select_d = [&](auto weight, const u64 need, const double frac) -> uint32_t {
        zero_whist();
        for_keys([&](const uint32_t key, const int) {
            const uint32_t d = kmax - key;
            const u64 q = weight(key, d);
            if (q) atomicAdd(&whist[wave][d >> 8], q);
        });
        merge_hist();
        select_prefix(hist, sel, need, frac, tid);
        const uint32_t hb = (uint32_t)sel[0];
        const u64 need2 = sel[1];
        zero_whist();
        for_keys([&](const uint32_t key, const int) {
            const uint32_t d = kmax - key;
            if ((d >> 8) == hb) {
                const u64 q = weight(key, d);
                if (q) atomicAdd(&whist[wave][d & 0xFFu], q);
            }
        });
        merge_hist();
        select_prefix(hist, sel, need2, -1.0, tid);
        return (hb << 8) | (uint32_t)sel[0];
    };
    uint32_t dmax = 0xFFFFu;  // keep the keys with kmax - key <= dmax
    if (top_k > 0 && top_k < V) dmax = select_d([](const uint32_t, const uint32_t) -> u64 { return 1ull; }, (u64)top_k, -1.0);
    if (top_p < 1.0f) {  // (workgroup-uniform, like every branch around a barrier here)
        const uint32_t dk = dmax;
        const uint32_t dp = select_d([&](const uint32_t key, const uint32_t d) -> u64 {
            if (d > dk) return 0ull;
            return (u64)(expf((bits_to_float(key_bits(key), BF16) - mx) * inv_temp) * kMassScale);
        }, 0ull, (double)top_p);
        dmax = min(dk, dp);
    }
    // exponential race over what stayed: consider() of teal_sampler.hip, term for term
    const uint32_t seed = (uint32_t)seed64, ctr = (uint32_t)ctr64;
    float best = -1.0f;
    int besti = 0x7FFFFFFF, kept = 0;
    for_keys([&](const uint32_t key, const int i) {
        if (kmax - key > dmax) return;
        const float pnum = expf((bits_to_float(key_bits(key), BF16) - mx) * inv_temp);
        if (!(pnum >= min_p)) return;
        ++kept;
        const float u = ((float)(hash3(seed, ctr, (uint32_t)i) >> 8) + 0.5f) * (1.0f / 16777216.0f);
        const float scv = pnum / (-logf(u));
        if (scv > best || (scv == best && i < besti)) { best = scv; besti = i; }
    });
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float ob = __shfl_xor(best, d);
        const int oi = __shfl_xor(besti, d);
        kept += __shfl_xor(kept, d);
        if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
    }
    __syncthreads();
    if (lane == 0) { fred[wave] = best; ired[wave] = besti; kred[wave] = kept; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w) {
            if (fred[w] > best || (fred[w] == best && ired[w] < besti)) { best = fred[w]; besti = ired[w]; }
            kept += kred[w];
        }
        tokens[r] = besti;
        if (history && (long long)ctr64 < (long long)history_len) history[(size_t)r * history_len + ctr64] = besti;
        rng_state[2 * r + 1] = ctr64 + 1ull;
        if (pos) pos[r] = pos0 + 1;
        if (kept_out) kept_out[r] = kept;
    }
}

}  // namespace teal

using namespace teal;

extern "C" {

int teal_sample_rows(const void* logits, size_t logits_stride, int vocab, int dtype, int B, const void* params, void* rng_state,
                     int32_t* tokens, int32_t* pos, int32_t* history, int history_len, int32_t* kept_out, const int32_t* active,
                     int slot0, void* stream) {
    if (!logits || !params || !rng_state || !tokens) return TEAL_ERR_ARG;
    if (B < 1 || B > 8 || slot0 < 0 || slot0 + B > 32 || (history && history_len < 0)) return TEAL_ERR_ARG;
    if (dtype != TEAL_F16 && dtype != TEAL_BF16) return TEAL_ERR_DTYPE;
    if (vocab < 8 || vocab > 16 * 8192 || (vocab & 7)) return TEAL_ERR_SHAPE;
    if (!aligned16(logits)) return TEAL_ERR_ALIGN;
    if (B > 1 && (logits_stride & 7)) return TEAL_ERR_ALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    auto* lg = reinterpret_cast<const uint16_t*>(logits);
    auto* pr = reinterpret_cast<const uint32_t*>(params);
    auto* rs = reinterpret_cast<u64*>(rng_state);
#define TEAL_ROWS(KERNEL) \
    hipLaunchKernelGGL((KERNEL), dim3(B), dim3(1024), 0, st, lg, logits_stride, vocab, pr, rs, tokens, pos, history, history_len, kept_out, active, slot0)
    const bool bf = dtype == TEAL_BF16;
    if (vocab <= 4 * 8192) {  // 4 vectors per thread
        if (bf) TEAL_ROWS((sample_rows_kernel<true, 4>)); else TEAL_ROWS((sample_rows_kernel<false, 4>));
    } else {                  // 16 vectors per thread (Llama-3's 128256)
        if (bf) TEAL_ROWS((sample_rows_kernel<true, 16>)); else TEAL_ROWS((sample_rows_kernel<false, 16>));
    }
#undef TEAL_ROWS
    return hipGetLastError() == hipSuccess ? TEAL_OK : TEAL_ERR_LAUNCH;
}

}  // extern "C"
