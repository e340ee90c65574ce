// teal_logprob.hip — token log-probabilities of a logits row and their C-ABI entry points (include/teal_hip.h).
//
//   lp(t) = (l[t] - m) - log sum_v exp(l[v] - m),  m = max_v l[v],  in fp32 over the row's 16-bit logits
//
// This is the MODEL's distribution: temperature 1 and no top-k filter, whatever the sampler that drew the token was told.
// expf / logf as in teal_sampler.hip (no fast intrinsics: the tests' bound of 4 fp32 ulps against the fp64 restatement,
// tests/logprob_rule.py, rests on their 1-ulp error).  A logit of -inf contributes 0; NaN logits, +inf logits and a row that
// is all -inf are outside the contract.
//
// One workgroup of 1024 threads per row, grid B; nothing is shared between workgroups (no atomics, no workspace, no hand-over),
// so a row's results depend on that row's logits and token only — not on B, on the slot or on the other rows — and the
// reduction order is fixed: replays are bit-identical.  The row (64 - 256 KB) comes from L2 right after the lm_head launch, so
// the kernel reads it twice with 16-byte loads, four in flight per thread: a max pass, then the sum pass; each ends in a wave
// butterfly and one step over the 16 wave results in LDS.  (All 16 vectors of a 128 k row held in registers, as the
// register-resident sampler holds them, spilled next to 8 expf chains.)
//
// The top_n alternates (by descending logit, equal logits by ascending id): every thread holds ITS best remaining (key, id) —
// the first is its maximum, which the max pass leaves behind; a round reduces the 1024 candidates to the winner, the thread that
// owned it writes the entry and rescans its own vectors for its next one — one thread rescans per round, the other 1023
// candidates stay valid (they lost to a larger one).
#include "teal_common.h"

namespace teal {

// order_key16 with -0 filed under +0's key (0x7FFF is the key of -0 alone): equal logits, so the lower id comes first
__device__ __forceinline__ uint32_t logit_key(const uint32_t b, const bool bf16) {
    const uint32_t k = order_key16(b, bf16);
    return k + (k == 0x7FFFu ? 1u : 0u);
}
__device__ __forceinline__ float key_logit(const uint32_t k, const bool bf16) {  // logit_key^-1
    return bits_to_float((k & 0x8000u) ? (k ^ 0x8000u) : (~k & 0xFFFFu), bf16);
}

// (key, id) a beats (key, id) b: larger logit, equal logits the lower id
__device__ __forceinline__ bool cand_better(const uint32_t ak, const int ai, const uint32_t bk, const int bi) {
    return ak > bk || (ak == bk && ai < bi);
}

constexpr int kNoCand = 0x7FFFFFFF;

// All 1024 threads of the workgroup call (barriers inside).  lp_out[0] = lp(t) (NaN for a token outside 0 .. V-1); top_n > 0:
// top_ids / top_lp [top_n].  V % 8 == 0.
template <bool BF16>
__device__ __forceinline__ void row_logprob(const uint16_t* __restrict__ logits, const int V, const int t, const int top_n,
                                            float* __restrict__ lp_out, int* __restrict__ top_ids, float* __restrict__ top_lp) {
    __shared__ uint32_t kred[2][16];
    __shared__ int ired[2][16];
    __shared__ float fred[16];
    constexpr int NV = 4;  // 16-byte loads in flight per thread
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V8 = V >> 3;
    const u32x4* lv = reinterpret_cast<const u32x4*>(logits);
    const bool tok_ok = t >= 0 && t < V;
    const uint32_t tbits = (tid == 0 && tok_ok) ? logits[t] : 0u;
    // this thread's best (key, id) among its logits below (pk, pid), NF 16-byte loads in flight; its vectors are tid, tid + 1024,
    // ...: ids ascend, so among equal keys the first seen is the lowest id.  FIRST: nothing is spent yet (the max pass).
    auto scan = [&](auto first, auto nf, const uint32_t pk, const int pid, uint32_t& bk, int& bi) {
        constexpr bool FIRST = decltype(first)::value;
        constexpr int NF = decltype(nf)::value;
        bk = 0u;
        bi = kNoCand;
        for (int i0 = tid; i0 < V8; i0 += NF * 1024) {
            u32x4 w[NF];
#pragma unroll
            for (int v = 0; v < NF; ++v) w[v] = lv[min(i0 + v * 1024, V8 - 1)];
#pragma unroll
            for (int v = 0; v < NF; ++v) {
                if (i0 + v * 1024 < V8) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const uint32_t k = logit_key((j & 1) ? (w[v][j >> 1] >> 16) : (w[v][j >> 1] & 0xFFFFu), BF16);
                        const int id = (i0 + v * 1024) * 8 + j;
                        if ((FIRST || cand_better(pk, pid, k, id)) && (k > bk || bi == kNoCand)) { bk = k; bi = id; }
                    }
                }
            }
        }
    };
    // max pass: (bk, bi) = this thread's largest logit, the first candidate of the alternates
    uint32_t bk;
    int bi;
    scan(std::true_type{}, std::integral_constant<int, NV>{}, 0u, 0, bk, bi);
    uint32_t kmax = bk;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, d));
    if (lane == 0) kred[1][wave] = kmax;
    __syncthreads();
    kmax = kred[1][0];
#pragma unroll
    for (int w = 1; w < 16; ++w) kmax = max(kmax, kred[1][w]);
    const float mx = key_logit(kmax, BF16);
    // sum of exp(l - m): this thread's logits in index order, the wave's 64 sums by butterfly, the 16 waves' by a tree
    float s = 0.0f;
    for (int i0 = tid; i0 < V8; i0 += NV * 1024) {
        u32x4 w[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) w[v] = lv[min(i0 + v * 1024, V8 - 1)];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            if (i0 + v * 1024 < V8) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    s += expf(bits_to_float(w[v][j] & 0xFFFFu, BF16) - mx);
                    s += expf(bits_to_float(w[v][j] >> 16, BF16) - mx);
                }
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 0) fred[wave] = s;
    __syncthreads();
    float part[16];
#pragma unroll
    for (int w = 0; w < 16; ++w) part[w] = fred[w];
#pragma unroll
    for (int n = 8; n >= 1; n >>= 1) {
#pragma unroll
        for (int w = 0; w < n; ++w) part[w] = part[2 * w] + part[2 * w + 1];
    }
    const float lse = logf(part[0]);
    if (tid == 0) lp_out[0] = tok_ok ? (key_logit(logit_key(tbits, BF16), BF16) - mx) - lse : __uint_as_float(0x7FC00000u);
    for (int r = 0; r < top_n; ++r) {
        uint32_t wk = bk;
        int wi = bi;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t ok = (uint32_t)__shfl_xor((int)wk, d);
            const int oi = __shfl_xor(wi, d);
            if (cand_better(ok, oi, wk, wi)) { wk = ok; wi = oi; }
        }
        // (round r writes buffer r & 1 and every thread reads it behind the barrier; the writes of round r + 2 come behind the
        // barrier of round r + 1, which no thread passes before it has read round r's; the max pass's buffer 1 was read before
        // the sum pass's barrier)
        if (lane == 0) { kred[r & 1][wave] = wk; ired[r & 1][wave] = wi; }
        __syncthreads();
        wk = kred[r & 1][0];
        wi = ired[r & 1][0];
#pragma unroll
        for (int w = 1; w < 16; ++w)
            if (cand_better(kred[r & 1][w], ired[r & 1][w], wk, wi)) { wk = kred[r & 1][w]; wi = ired[r & 1][w]; }
        if (bi == wi && wi != kNoCand) {  // the owner of the winner (ids are unique): its entry, then its next candidate
            top_ids[r] = wi;
            top_lp[r] = (key_logit(wk, BF16) - mx) - lse;
            if (r + 1 < top_n) scan(std::false_type{}, std::integral_constant<int, 16>{}, wk, wi, bk, bi);  // (one L2 round trip: <= 16 vectors)
        }
    }
}

// the sampling form: row r of the launch serves slot slot0 + r and files its results under the draw its sampler has just counted
template <bool BF16>
__global__ __launch_bounds__(1024) void token_logprobs_kernel(const uint16_t* __restrict__ logits, const size_t stride, const int V,
                                                               const int* __restrict__ tokens,
                                                               const unsigned long long* __restrict__ rng_state,
                                                               float* __restrict__ lp, const int lp_len, const int top_n,
                                                               int* __restrict__ top_ids, float* __restrict__ top_lp,
                                                               const int* __restrict__ active, const int slot0) {
    const int r = blockIdx.x;
    if (active && !((active[0] >> (slot0 + r)) & 1)) return;
    const unsigned long long c = rng_state[2 * r + 1];
    if (c == 0ull || c > (unsigned long long)lp_len) return;
    const size_t o = (size_t)r * lp_len + (size_t)(c - 1ull);
    row_logprob<BF16>(logits + (size_t)r * stride, V, tokens[r], top_n, lp + o, top_n > 0 ? top_ids + o * top_n : nullptr,
                          top_n > 0 ? top_lp + o * top_n : nullptr);
}

// the teacher-forcing form: in the sampler's place of a scoring loop
template <bool BF16>
__global__ __launch_bounds__(1024) void score_step_kernel(const uint16_t* __restrict__ logits, const int V,
                                                           const int* __restrict__ targets, const int n_targets,
                                                           int* __restrict__ token_out, int* __restrict__ pos_inout,
                                                           float* __restrict__ lp) {
    const long long j = (long long)pos_inout[0] + 1;  // (every thread reads it before the barriers of row_logprob; thread 0
    if (j < 0 || j >= n_targets) return;              //  writes it behind them)
    const int t = targets[j];
    row_logprob<BF16>(logits, V, t, 0, lp + j, nullptr, nullptr);
    if (threadIdx.x == 0) {
        token_out[0] = t;
        pos_inout[0] = (int)j;
    }
}

}  // namespace teal

using namespace teal;

namespace {
int logprob_row_check(const void* logits, int vocab, int dtype) {
    if (dtype != TEAL_F16 && dtype != TEAL_BF16) return TEAL_ERR_DTYPE;
    if (vocab < 8 || vocab > 16 * 8192 || (vocab & 7)) return TEAL_ERR_SHAPE;
    if (!aligned16(logits)) return TEAL_ERR_ALIGN;
    return TEAL_OK;
}
}  // namespace

extern "C" {

int teal_token_logprobs(const void* logits, size_t logits_stride, int vocab, int dtype, int B, const int32_t* tokens,
                        const void* rng_state, float* lp, int lp_len, int top_n, int32_t* top_ids, float* top_lp,
                        const int32_t* active, int slot0, void* stream) {
    if (!logits || !tokens || !rng_state || !lp || top_n < 0 || top_n > 8 || (top_n > 0 && (!top_ids || !top_lp))) return TEAL_ERR_ARG;
    if (B < 1 || B > 8 || slot0 < 0 || slot0 + B > 32 || lp_len <= 0) return TEAL_ERR_ARG;
    const int rc = logprob_row_check(logits, vocab, dtype);
    if (rc != TEAL_OK) return rc;
    if (B > 1 && (logits_stride & 7)) return TEAL_ERR_ALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    auto* lg = reinterpret_cast<const uint16_t*>(logits);
    auto* rs = reinterpret_cast<const unsigned long long*>(rng_state);
#define TEAL_LOGPROBS(KERNEL) \
    hipLaunchKernelGGL((KERNEL), dim3(B), dim3(1024), 0, st, lg, logits_stride, vocab, tokens, rs, lp, lp_len, top_n, top_ids, top_lp, active, slot0)
    if (dtype == TEAL_BF16) TEAL_LOGPROBS(token_logprobs_kernel<true>); else TEAL_LOGPROBS(token_logprobs_kernel<false>);
#undef TEAL_LOGPROBS
    return hipGetLastError() == hipSuccess ? TEAL_OK : TEAL_ERR_LAUNCH;
}

int teal_score_step(const void* logits, int vocab, int dtype, const int32_t* targets, int n_targets, int32_t* token_out,
                    int32_t* pos_inout, float* lp, void* stream) {
    if (!logits || !targets || !token_out || !pos_inout || !lp || n_targets < 1) return TEAL_ERR_ARG;
    const int rc = logprob_row_check(logits, vocab, dtype);
    if (rc != TEAL_OK) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    auto* lg = reinterpret_cast<const uint16_t*>(logits);
#define TEAL_SCORE(KERNEL) hipLaunchKernelGGL((KERNEL), dim3(1), dim3(1024), 0, st, lg, vocab, targets, n_targets, token_out, pos_inout, lp)
    if (dtype == TEAL_BF16) TEAL_SCORE(score_step_kernel<true>); else TEAL_SCORE(score_step_kernel<false>);
#undef TEAL_SCORE
    return hipGetLastError() == hipSuccess ? TEAL_OK : TEAL_ERR_LAUNCH;
}

}  // extern "C"
