// teal_force.hip — teacher-forced tokens of continuous batching: the launch that puts a token a request was told to take in the
// place of the one its sampler has just drawn (teal_amd/gpt_fast/forcing.py, SlotDecodeEngine).
//
// One entry point, teal_force_tokens (the rule: include/teal_hip.h).  It runs behind a draw's sampler launch or launches and in
// front of the logprob and retire launches.  The sampler has already moved the row's position, bumped its draw counter and filed
// its own token under history entry i = counter - 1; the launch overwrites the two words that name the token — tokens[r] and that
// history entry — so what it leaves is what a sampler that had drawn the forced token would have left, and every launch behind it
// (logprobs, retire, the next step's embedding, processors and automaton) sees the forced token as the drawn one.
//
// One wave, lane r serving row r.  Like the retire launch it sits at the end of a step that has streamed the model's weights
// through every cache, so its loads miss and what it costs is the number of loads that wait for one another: round one is every
// word whose address the arguments give — the active word, the row's draw counter and its length, in flight together — and
// round two the one table entry the counter selects.  No branch stands in front of round one (a lane past the last row reads the
// last row's words; the compiler sinks a load below any branch it is allowed to, which made three rounds of the first draft), and
// the one predicate is formed from all three words at once.  Two stores follow, to addresses known from round one.  No atomics,
// no workspace, no LDS; the active word is one scalar load, every other access a plain vector load or store of one lane: replays
// are bit-identical.
#include "teal_common.h"

namespace teal {

constexpr int kForceRows = 8;  // rows of a launch = the slots of a step

__global__ __launch_bounds__(64) void force_tokens_kernel(const int* __restrict__ forced, const int forced_stride,
                                                          const int* __restrict__ forced_len,
                                                          const unsigned long long* __restrict__ rng_state, int* __restrict__ tokens,
                                                          int* __restrict__ history, const int history_len, const int B,
                                                          const int* __restrict__ active, const int slot0) {
    // a lane past the last row reads the last row's words and writes nothing: no branch stands in front of a load
    const int r = min((int)threadIdx.x, B - 1);
    // round one: three loads whose addresses the arguments give (active NULL: some valid word, not consulted)
    const int* act_p = active ? active : forced_len;
    const uint32_t act_w = (uint32_t)act_p[0];
    const unsigned long long c = rng_state[2 * r + 1];
    const int len = forced_len[r];
    const uint32_t act = active ? act_w : 0xFFFFFFFFu;
    const int n = max(min(len, forced_stride), 0);
    // i = c - 1 in 0 .. n-1 (n = 0: no forced token at all); one predicate, formed without a branch
    const bool go = ((int)threadIdx.x < B) & (((act >> (slot0 + r)) & 1u) != 0u) & (c != 0ull) & (c <= (unsigned long long)n);
    const int i = go ? (int)(c - 1ull) : 0;
    if (!go) return;
    // round two: the entry the counter selects
    const int t = forced[(size_t)r * (size_t)forced_stride + (size_t)i];
    tokens[r] = t;
    if (history && i < history_len) history[(size_t)r * (size_t)history_len + (size_t)i] = t;
}

}  // namespace teal

using namespace teal;

extern "C" int teal_force_tokens(const int32_t* forced, int forced_stride, const int32_t* forced_len, const void* rng_state,
                                 int32_t* tokens, int32_t* history, int history_len, int B, const int32_t* active, int slot0,
                                 void* stream) {
    if (!forced || !forced_len || !rng_state || !tokens) return TEAL_ERR_ARG;
    if (B < 1 || B > kForceRows || slot0 < 0 || slot0 + B > 32 || forced_stride <= 0) return TEAL_ERR_ARG;
    if (history && history_len < 0) return TEAL_ERR_ARG;
    hipLaunchKernelGGL(force_tokens_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), forced, forced_stride,
                       forced_len, reinterpret_cast<const unsigned long long*>(rng_state), tokens, history, history_len, B, active, slot0);
    return hipGetLastError() == hipSuccess ? TEAL_OK : TEAL_ERR_LAUNCH;
}
