// teal_constrain.hip — constrained decoding: per-request token automata stepped on the device, and their C-ABI entry point
// (include/teal_hip.h): one launch between a step's (adjusted) logits and its samplers.
//
// A row's automaton image lives in a shared arena: S header rows {edge_begin, edge_end, default, accept}, then the edges as
// (token, next) word pairs, tokens strictly ascending per state.  delta(s, t) = the edge's `next` if state s names t, else
// default(s); t is allowed in s iff delta(s, t) >= 0.  For row r about to make draw c (its draw counter before the sampler):
//
//   state   c == 0: s = 0.  Else p = trace[r][c-1] & 0x3FFFFFFF (clamped into 0 .. S-1) and t = tokens[r], the token the step
//           was fed: t == eos[r]: s = p;  delta(p, t) >= 0: s = delta(p, t);  else s = p with bit 30 set in the trace word
//           (a violation: cannot happen for a token drawn under the mask).  trace[r][c] = that word.
//   mask    out[r][v] = logits[r][v] (the same 16 bits) if v is allowed in s, or v == eos[r] and accept(s); -MAXF otherwise —
//           the EOS id is banned in a non-accepting state whatever its default says.
//   table[r].base < 0: unconstrained — out[r] is a bit-for-bit copy (-0, infinities and NaN payloads included), trace word 0.
//
// The grid of teal_logit_adjust: (ceil(vocab / 8192), B), 1024 threads, 8 consecutive elements per thread in one 16-byte load and
// one 16-byte store.  Every workgroup of a row recomputes s (a binary search over the previous state's edges: workgroup-uniform,
// scalar loads), fills a 256-word LDS bitmap of its 8192 entries with the state's default, finds its sub-range of the state's
// sorted edges with two lower bounds and lets its threads stride over it, setting or clearing bits with LDS atomics (bit
// operations commute: replays are bit-identical).  No workgroup reads a word the launch writes — trace[r][c-1] is read,
// trace[r][c] written, by workgroup x == 0 alone — so a multi-workgroup row needs no second launch.  All stores are plain vector
// stores; no workspace.
#include "teal_common.h"

namespace teal {

constexpr int kConstrainPerWg = 8192;  // elements a workgroup of 1024 threads covers
constexpr int kViolationBit = 1 << 30;
constexpr int kStateMask = 0x3FFFFFFF;

// first i in 0 .. n with token(i) >= key; edges: (token, next) word pairs
__device__ __forceinline__ int edge_lower_bound(const int* __restrict__ edges, const int n, const int key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (edges[2 * mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// a state's header with its edge range clamped into the arena (the host validates images; this keeps a damaged one in bounds)
struct StateHeader {
    int begin, count, dflt, accept;
};

__device__ __forceinline__ StateHeader load_header(const int* __restrict__ image, const int s, const int S, const long long room) {
    const int* h = image + 4 * (size_t)s;
    long long b = h[0], e = h[1];
    const long long lo = 4ll * S;
    b = b < lo ? lo : (b > room ? room : b);
    e = e < b ? b : (e > room ? room : e);
    return {(int)b, (int)((e - b) >> 1), h[2], h[3]};
}

__global__ __launch_bounds__(1024) void constrain_logits_kernel(const uint16_t* __restrict__ logits, const size_t stride, const int V,
                                                                 const int* __restrict__ tokens, const unsigned long long* __restrict__ rng_state,
                                                                 const int* __restrict__ eos, const int* __restrict__ table,
                                                                 const int* __restrict__ arena, const size_t arena_words,
                                                                 int* __restrict__ trace, const int trace_len, uint16_t* __restrict__ out,
                                                                 const size_t out_stride, const int* __restrict__ active, const int slot0,
                                                                 const uint32_t neg_maxf) {
    __shared__ uint32_t bitmap[kConstrainPerWg / 32];
    const int r = blockIdx.y;
    if (active && !((active[0] >> (slot0 + r)) & 1)) return;  // (workgroup-uniform: before any barrier)
    const int tid = threadIdx.x;
    const int wg0 = blockIdx.x * kConstrainPerWg;
    const int e0 = wg0 + tid * 8;
    const bool inside = e0 < V;  // (V % 8 == 0: a thread's 8 elements are inside the row or all outside)
    const unsigned long long c64 = rng_state[2 * r + 1];
    const bool traced = c64 < (unsigned long long)trace_len;  // (the caller's contract; a counter past it writes no word)
    int* const trow = trace + (size_t)r * trace_len;
    const long long base = table[4 * r];
    const int S = table[4 * r + 1];
    if (base < 0 || S < 1 || (unsigned long long)base + 4ull * S > arena_words) {  // unconstrained: the row's own bits
        if (inside) *reinterpret_cast<u32x4*>(out + (size_t)r * out_stride + e0) = *reinterpret_cast<const u32x4*>(logits + (size_t)r * stride + e0);
        if (blockIdx.x == 0 && tid == 0 && traced) trow[c64] = 0;
        return;
    }
    const int* const image = arena + base;
    const long long room = (long long)(arena_words - (size_t)base);
    const int e = eos[r];
    int s = 0, word = 0;
    if (c64 > 0 && c64 - 1 < (unsigned long long)trace_len) {
        int p = trow[c64 - 1] & kStateMask;
        p = p > S - 1 ? S - 1 : p;
        const int t = tokens[r];
        s = word = p;
        if (t != e) {
            const StateHeader hp = load_header(image, p, S, room);
            const int* pe = image + hp.begin;
            const int i = edge_lower_bound(pe, hp.count, t);
            int d = (i < hp.count && pe[2 * i] == t) ? pe[2 * i + 1] : hp.dflt;
            d = d > S - 1 ? -1 : d;
            if (d >= 0) s = word = d; else word = p | kViolationBit;
        }
    }
    if (blockIdx.x == 0 && tid == 0 && traced) trow[c64] = word;
    const StateHeader hs = load_header(image, s, S, room);
    if (tid < kConstrainPerWg / 32) bitmap[tid] = hs.dflt >= 0 ? 0xFFFFFFFFu : 0u;
    __syncthreads();
    const int* const se = image + hs.begin;
    const int i0 = edge_lower_bound(se, hs.count, wg0), i1 = edge_lower_bound(se, hs.count, wg0 + kConstrainPerWg);
    for (int i = i0 + tid; i < i1; i += 1024) {
        const int bit = se[2 * i] - wg0, next = se[2 * i + 1];  // (0 .. 8191 between the two lower bounds of a sorted list)
        if ((unsigned)bit >= (unsigned)kConstrainPerWg) continue;
        if (next >= 0) atomicOr(&bitmap[bit >> 5], 1u << (bit & 31)); else atomicAnd(&bitmap[bit >> 5], ~(1u << (bit & 31)));
    }
    __syncthreads();
    if (!inside) return;
    uint32_t keep = (bitmap[tid >> 2] >> ((tid & 3) * 8)) & 0xFFu;
    if (e >= e0 && e < e0 + 8) keep = hs.accept ? (keep | (1u << (e - e0))) : (keep & ~(1u << (e - e0)));
    const u32x4 lv = *reinterpret_cast<const u32x4*>(logits + (size_t)r * stride + e0);
    u32x4 ov;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t lo = ((keep >> (2 * j)) & 1u) ? (lv[j] & 0xFFFFu) : neg_maxf;
        const uint32_t hi = ((keep >> (2 * j + 1)) & 1u) ? (lv[j] & 0xFFFF0000u) : (neg_maxf << 16);
        ov[j] = lo | hi;
    }
    *reinterpret_cast<u32x4*>(out + (size_t)r * out_stride + e0) = ov;
}

}  // namespace teal

using namespace teal;

extern "C" {

int teal_constrain_logits(const void* logits, size_t logits_stride, int vocab, int dtype, int B, const int32_t* tokens, const void* rng_state,
                          const int32_t* eos, const int32_t* table, const int32_t* arena, size_t arena_words, int32_t* trace, int trace_len,
                          void* out, size_t out_stride, const int32_t* active, int slot0, void* stream) {
    if (!logits || !tokens || !rng_state || !eos || !table || !arena || !trace || !out) return TEAL_ERR_ARG;
    if (B < 1 || B > 8 || slot0 < 0 || slot0 + B > 32 || trace_len < 1 || arena_words == 0) return TEAL_ERR_ARG;
    if (dtype != TEAL_F16 && dtype != TEAL_BF16) return TEAL_ERR_DTYPE;
    if (vocab < 8 || vocab > 16 * kConstrainPerWg || (vocab & 7)) return TEAL_ERR_SHAPE;
    if (!aligned16(logits) || !aligned16(out)) return TEAL_ERR_ALIGN;
    if (B > 1 && ((logits_stride & 7) || (out_stride & 7))) return TEAL_ERR_ALIGN;
    {   // `out` must not alias `logits`: the logprob launch behind the samplers reads the rows in front of this launch
        const uintptr_t l0 = reinterpret_cast<uintptr_t>(logits), o0 = reinterpret_cast<uintptr_t>(out);
        const uintptr_t l1 = l0 + ((size_t)(B - 1) * logits_stride + (size_t)vocab) * 2, o1 = o0 + ((size_t)(B - 1) * out_stride + (size_t)vocab) * 2;
        if (l0 < o1 && o0 < l1) return TEAL_ERR_ARG;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((vocab + kConstrainPerWg - 1) / kConstrainPerWg, B);
    const uint32_t neg_maxf = dtype == TEAL_BF16 ? 0xFF7Fu : 0xFBFFu;
    hipLaunchKernelGGL(constrain_logits_kernel, grid, dim3(1024), 0, st, reinterpret_cast<const uint16_t*>(logits), logits_stride, vocab, tokens,
                       reinterpret_cast<const unsigned long long*>(rng_state), eos, table, arena, arena_words, trace, trace_len,
                       reinterpret_cast<uint16_t*>(out), out_stride, active, slot0, neg_maxf);
    return hipGetLastError() == hipSuccess ? TEAL_OK : TEAL_ERR_LAUNCH;
}

}  // extern "C"
