// teal_speculative.hip — the verify side of speculative decoding (gpt-fast/generate.py:98-217) for gfx950 / CDNA4, wave64.
//
// One round: k draft steps (the fused decode step, TEAL-sparse), then ONE dense pass over the k + 1 tokens [x0, d1 .. dk] at
// positions p .. p+k through the prompt pass's GEMMs (teal_prefill.hip; the slab layout and its helpers: teal_slab.h), with
//   verify_attention_kernel + verify_merge_kernel   attention of the k + 1 rows against the whole cache (split-KV; the body the
//                                                   batched step shares: teal_chunked_attention.h)
//   spec_round_logits_kernel                        the lm_head slabs of every row, summed and rounded once (the module's logits)
//   spec_row_stats_kernel                           per row: max, top-k pivot, softmax normaliser
//   spec_decide_kernel                              the reference's accept / reject rule (gpt-fast/generate.py:123-146)
// Everything that decides the round stays on the device: the accepted count, the emitted tokens, the next round's position
// and input token.  The draw convention is in include/teal_hip.h (teal_spec_accept).
#include "teal_chunked_attention.h"

namespace teal {

constexpr int kVerifyMaxT = 16;     // the prompt pass's most tokens per pass
constexpr int kVerifyMaxQ = 64;     // query rows (heads of a group x tokens) per workgroup

// Attention of T <= 16 new tokens at positions p0 .. p0+T-1 (p0 read from the device) against cache rows 0 .. p0+t: the chunked
// split-KV body (teal_chunked_attention.h) with the KR token slots of the slabs as its new rows.  Grid (nsplit, n_kv, rep / hq).
template <bool BF16, int HD, int KR>
__global__ __launch_bounds__(256) void verify_attention_kernel(const float* __restrict__ slabs, const int split,
                                                               const int* __restrict__ pos_ptr, const uint16_t* __restrict__ rope,
                                                               uint16_t* __restrict__ k_cache, uint16_t* __restrict__ v_cache,
                                                               float* __restrict__ partials, const int T, const int n_head,
                                                               const int n_kv, const int hq, const int max_seq, const float scale) {
    chunked_attention_body<BF16, HD, kVerifyMaxQ, KR, KR>(slabs, split, pos_ptr[0], rope, k_cache, v_cache, partials, T, 0, T, n_head, n_kv,
                                                          hq, blockIdx.z, max_seq, scale);
}

// token slots >= T are zero
template <bool BF16, int KR>
__global__ __launch_bounds__(128) void verify_merge_kernel(const float* __restrict__ partials, uint16_t* __restrict__ yt, const int T,
                                                           const int hd, const int nsplit) {
    chunked_merge_body<BF16, KR, false>(partials, yt, T, hd, nsplit, nullptr);
}

// ------------------------------------------------------------------------------------------------
// Acceptance.  Row distributions: x (16-bit logits) -> x / temperature -> keep the top_k (ties at the pivot kept) -> softmax,
// evaluated as prob(v) = exp((x_v - max) * inv_temp) / Z over the kept set — the fused sampler's weights, normalised.
// ------------------------------------------------------------------------------------------------
struct RowStats {
    float mx;
    uint32_t pivot;  // keep order_key16(x) >= pivot (0: all)
    float z;
    float pad;
};

__device__ __forceinline__ float uniform01(const uint32_t h) { return ((float)(h >> 8) + 0.5f) * (1.0f / 16777216.0f); }

template <bool BF16>
__device__ __forceinline__ float row_prob(const uint16_t* __restrict__ row, const RowStats& st, const float inv_temp, const int v) {
    const uint32_t b = row[v];
    if (order_key16(b, BF16) < st.pivot) return 0.0f;
    return expf((bits_to_float(b, BF16) - st.mx) * inv_temp) / st.z;
}

// target rows: tl[t][V] = round(sum of the lm_head slabs of token t), t < T (one thread per vocabulary column)
template <bool BF16, int KR>
__global__ __launch_bounds__(256) void spec_round_logits_kernel(const float* __restrict__ slabs, const int split, const int V, const int T,
                                                                uint16_t* __restrict__ tl) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= V) return;
    float r[KR];
    slab_column<BF16, KR>(slabs, split, (size_t)V, (size_t)col, r);
#pragma unroll
    for (int t = 0; t < KR; ++t)
        if (t < T) tl[(size_t)t * V + col] = float_to_bits<BF16>(r[t]);
}

// one workgroup per row: rows 0 .. k are the target's (tl), rows k+1 .. 2k the draft's (dl).  The top-k pivot is the fused
// sampler's exact two-pass radix select on the 16-bit keys.
template <bool BF16>
__global__ __launch_bounds__(1024) void spec_row_stats_kernel(const uint16_t* __restrict__ tl, const uint16_t* __restrict__ dl, const int V,
                                                              const int k, const int top_k, const float inv_temp, RowStats* __restrict__ stats) {
    __shared__ unsigned int hist[256];
    __shared__ unsigned int whist[16][256];
    __shared__ float fred[16];
    __shared__ unsigned int sel[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = blockIdx.x;
    const uint16_t* x = r <= k ? tl + (size_t)r * V : dl + (size_t)(r - k - 1) * V;
    const bool filter = top_k > 0 && top_k < V;
    float mx = -INFINITY;
    for (int i = tid; i < 16 * 256; i += 1024) (&whist[0][0])[i] = 0;
    __syncthreads();
    for (int i = tid; i < V; i += 1024) {
        const uint32_t b = x[i];
        mx = fmaxf(mx, bits_to_float(b, BF16));
        if (filter) atomicAdd(&whist[wave][order_key16(b, BF16) >> 8], 1u);
    }
    mx = wave_max_f(mx);
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
    uint32_t pivot = 0;
    if (filter) {
        select_bin(hist, nullptr, sel, (unsigned int)top_k, tid);
        const unsigned int hb = sel[0], need2 = sel[1];
        __syncthreads();
        for (int i = tid; i < 16 * 256; i += 1024) (&whist[0][0])[i] = 0;
        __syncthreads();
        for (int i = tid; i < V; i += 1024) {
            const uint32_t kk = order_key16(x[i], BF16);
            if ((kk >> 8) == hb) atomicAdd(&whist[wave][kk & 0xFFu], 1u);
        }
        __syncthreads();
        if (tid < 256) {
            unsigned int a = 0;
#pragma unroll
            for (int w = 0; w < 16; ++w) a += whist[w][tid];
            hist[tid] = a;
        }
        __syncthreads();
        select_bin(hist, nullptr, sel, need2, tid);
        pivot = (hb << 8) | sel[0];
        __syncthreads();
    }
    float z = 0.0f;
    for (int i = tid; i < V; i += 1024) {
        const uint32_t b = x[i];
        if (order_key16(b, BF16) >= pivot) z += expf((bits_to_float(b, BF16) - mx) * inv_temp);
    }
    z = wave_sum_f(z);
    __syncthreads();
    if (lane == 0) fred[wave] = z;
    __syncthreads();
    if (tid == 0) {
        float s = 0.0f;
        for (int w = 0; w < 16; ++w) s += fred[w];
        stats[r] = RowStats{mx, pivot, s, 0.0f};
    }
}

// the decision (one workgroup): accepted count n, the token after the accepted drafts, and the round's device state
template <bool BF16>
__global__ __launch_bounds__(1024) void spec_decide_kernel(const uint16_t* __restrict__ tl, const uint16_t* __restrict__ dl,
                                                           const RowStats* __restrict__ stats, const int V, const int k,
                                                           const float inv_temp, unsigned long long* __restrict__ rng_state,
                                                           int* __restrict__ tokens, int* __restrict__ spec_pos, int* __restrict__ pos_out,
                                                           int* __restrict__ out_seq, const int out_cap, int* __restrict__ out_len,
                                                           int* __restrict__ n_acc_out, int* __restrict__ hist_out) {
    __shared__ int n_sh;
    __shared__ float fb[2][16];
    __shared__ int ib[2][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t seed = (uint32_t)rng_state[0], ctr = (uint32_t)rng_state[1];
    if (tid == 0) {
        int n = k;
        for (int i = 0; i < k; ++i) {
            const int d = min(max(tokens[i + 1], 0), V - 1);
            const float q = row_prob<BF16>(tl + (size_t)i * V, stats[i], inv_temp, d);
            const float p = row_prob<BF16>(dl + (size_t)i * V, stats[k + 1 + i], inv_temp, d);
            const float u = uniform01(hash3(seed, ctr, (uint32_t)i));
            if (!(p > 0.0f && u <= fminf(1.0f, q / p))) { n = i; break; }
        }
        n_sh = n;
    }
    __syncthreads();
    const int n = n_sh;
    const uint16_t* qrow = tl + (size_t)n * V;
    const RowStats qs = stats[n];
    const bool resid = n < k;
    const uint16_t* prow = dl + (size_t)(resid ? n : 0) * V;
    const RowStats ps = stats[k + 1 + (resid ? n : 0)];
    // exponential race over max(q - p, 0) (rejection) or q (all accepted); q alone as the fallback of an all-zero residual
    float best = -1.0f, bestq = -1.0f;
    int besti = 0x7FFFFFFF, bestqi = 0x7FFFFFFF;
    for (int v = tid; v < V; v += 1024) {
        const float e = -logf(uniform01(hash3(seed, ctr + 1u, (uint32_t)v)));
        const float q = row_prob<BF16>(qrow, qs, inv_temp, v);
        const float w = resid ? fmaxf(q - row_prob<BF16>(prow, ps, inv_temp, v), 0.0f) : q;
        const float s = w / e, sq = q / e;
        if (s > best) { best = s; besti = v; }  // (v ascending per thread: ties keep the lower index)
        if (sq > bestq) { bestq = sq; bestqi = v; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float ob = __shfl_xor(best, o), obq = __shfl_xor(bestq, o);
        const int oi = __shfl_xor(besti, o), oiq = __shfl_xor(bestqi, o);
        if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
        if (obq > bestq || (obq == bestq && oiq < bestqi)) { bestq = obq; bestqi = oiq; }
    }
    if (lane == 0) { fb[0][wave] = best; ib[0][wave] = besti; fb[1][wave] = bestq; ib[1][wave] = bestqi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w) {
            if (fb[0][w] > best || (fb[0][w] == best && ib[0][w] < besti)) { best = fb[0][w]; besti = ib[0][w]; }
            if (fb[1][w] > bestq || (fb[1][w] == bestq && ib[1][w] < bestqi)) { bestq = fb[1][w]; bestqi = ib[1][w]; }
        }
        const int tok = best > 0.0f ? besti : bestqi;
        const int base = out_len[0], p = spec_pos[0];
        for (int j = 0; j < n; ++j)
            if (base + j < out_cap) out_seq[base + j] = tokens[j + 1];
        if (base + n < out_cap) out_seq[base + n] = tok;
        out_len[0] = base + n + 1;
        tokens[0] = tok;
        spec_pos[0] = p + n + 1;
        if (pos_out) pos_out[0] = p + n + 1;
        if (n_acc_out) n_acc_out[0] = n;
        if (hist_out) hist_out[n] += 1;
        rng_state[1] = rng_state[1] + 2ull;
    }
}

constexpr size_t align256(const size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace teal

using namespace teal;

extern "C" {

size_t teal_verify_attention_ws_bytes(int T, int n_head, int head_dim) {
    return chunked_attention_ws_bytes(n_head, T < 1 ? 1 : T, kAttnMaxSplit, head_dim);
}

int teal_verify_attention(const float* qkv_slabs, int split, const void* rope, const int32_t* pos, void* k_cache, void* v_cache, void* yt,
                          float* partials, size_t partials_bytes, int T, int n_head, int n_kv_head, int head_dim, int max_seq, int dtype,
                          void* stream) {
    const int rc = chunked_attention_check(qkv_slabs, split, rope, pos, k_cache, v_cache, yt, partials, T, kVerifyMaxT, n_head, n_kv_head,
                                           head_dim, max_seq, T, dtype);
    if (rc != TEAL_OK) return rc;
    DeviceCtx* ctx = device_ctx();
    if (!ctx) return TEAL_ERR_NO_DEVICE;
    const ChunkedAttnPlan pl = chunked_attention_plan(ctx->num_cu, n_head / n_kv_head, n_kv_head, T, 1, max_seq, kVerifyMaxQ);
    const int hq = pl.hq, nsplit = pl.nsplit;
    if (partials_bytes < chunked_attention_ws_bytes(n_head, T, nsplit, head_dim)) return TEAL_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const float scale = 1.0f / sqrtf((float)head_dim);
    const dim3 grid(nsplit, n_kv_head, pl.groups);
    auto* rp = reinterpret_cast<const uint16_t*>(rope);
    auto* kc = reinterpret_cast<uint16_t*>(k_cache);
    auto* vc = reinterpret_cast<uint16_t*>(v_cache);
    auto* y = reinterpret_cast<uint16_t*>(yt);
    const int kr = rows_for(T);
#define TEAL_VA(BF, HDV, KRV) do { \
        hipLaunchKernelGGL((verify_attention_kernel<BF, HDV, KRV>), grid, dim3(256), 0, st, qkv_slabs, split, pos, rp, kc, vc, partials, T, \
                           n_head, n_kv_head, hq, max_seq, scale); \
        hipLaunchKernelGGL((verify_merge_kernel<BF, KRV>), dim3(n_head, KRV), dim3(128), 0, st, partials, y, T, head_dim, nsplit); } while (0)
#define TEAL_VA_KR(BF, HDV) do { if (kr == 8) TEAL_VA(BF, HDV, 8); else TEAL_VA(BF, HDV, 16); } while (0)
    if (dtype == TEAL_BF16) { if (head_dim == 128) TEAL_VA_KR(true, 128); else TEAL_VA_KR(true, 64); }
    else { if (head_dim == 128) TEAL_VA_KR(false, 128); else TEAL_VA_KR(false, 64); }
#undef TEAL_VA_KR
#undef TEAL_VA
    return hipGetLastError() == hipSuccess ? TEAL_OK : TEAL_ERR_LAUNCH;
}

size_t teal_spec_accept_scratch_bytes(int vocab, int k) {
    if (vocab <= 0 || k < 1) return 0;
    return align256((size_t)(k + 1) * vocab * sizeof(uint16_t)) + align256((size_t)(2 * k + 1) * sizeof(RowStats));
}

int teal_spec_accept(const float* logit_slabs, int split, const void* draft_logits, int vocab, int k, int dtype, int top_k, float temperature,
                     void* rng_state, int32_t* tokens, int32_t* spec_pos, int32_t* pos_out, int32_t* out_seq, int out_cap, int32_t* out_len,
                     int32_t* n_acc, int32_t* hist, void* scratch, size_t scratch_bytes, void* stream) {
    if (!logit_slabs || !draft_logits || !rng_state || !tokens || !spec_pos || !out_len || !scratch || split < 1 || split > 16 || out_cap < 0 ||
        (out_cap > 0 && !out_seq))
        return TEAL_ERR_ARG;
    if (dtype != TEAL_F16 && dtype != TEAL_BF16) return TEAL_ERR_DTYPE;
    if (vocab < 8 || vocab > 131072 || vocab % 8 || k < 1 || k > kVerifyMaxT - 1) return TEAL_ERR_SHAPE;
    if (!aligned16(logit_slabs) || !aligned16(scratch)) return TEAL_ERR_ALIGN;
    if (scratch_bytes < teal_spec_accept_scratch_bytes(vocab, k)) return TEAL_ERR_WORKSPACE;
    if (!device_ctx()) return TEAL_ERR_NO_DEVICE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const float inv_temp = 1.0f / fmaxf(temperature, 1e-5f);
    const int T = k + 1;
    auto* tl = reinterpret_cast<uint16_t*>(scratch);
    auto* stats = reinterpret_cast<RowStats*>(reinterpret_cast<unsigned char*>(scratch) + align256((size_t)T * vocab * sizeof(uint16_t)));
    auto* dl = reinterpret_cast<const uint16_t*>(draft_logits);
    auto* rs = reinterpret_cast<unsigned long long*>(rng_state);
    const dim3 gr((vocab + 255) / 256);
#define TEAL_SA(BF) do { \
        if (rows_for(T) == 8) hipLaunchKernelGGL((spec_round_logits_kernel<BF, 8>), gr, dim3(256), 0, st, logit_slabs, split, vocab, T, tl); \
        else hipLaunchKernelGGL((spec_round_logits_kernel<BF, 16>), gr, dim3(256), 0, st, logit_slabs, split, vocab, T, tl); \
        hipLaunchKernelGGL((spec_row_stats_kernel<BF>), dim3(2 * k + 1), dim3(1024), 0, st, tl, dl, vocab, k, top_k, inv_temp, stats); \
        hipLaunchKernelGGL((spec_decide_kernel<BF>), dim3(1), dim3(1024), 0, st, tl, dl, stats, vocab, k, inv_temp, rs, tokens, spec_pos, pos_out, \
                           out_seq, out_cap, out_len, n_acc, hist); } while (0)
    if (dtype == TEAL_BF16) TEAL_SA(true); else TEAL_SA(false);
#undef TEAL_SA
    return hipGetLastError() == hipSuccess ? TEAL_OK : TEAL_ERR_LAUNCH;
}

}  // extern "C"
