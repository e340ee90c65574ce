// teal_stop.hip — per-request stop conditions of continuous batching: the retire launch of a step (or of an admission's first draw)
// that also ends a slot on one of up to 16 stop ids or on one of up to 8 stop sequences of up to 8 tokens, holds all of them back
// below the request's min_new_tokens, and records why the slot ended (teal_amd/gpt_fast/stopping.py, SlotDecodeEngine).
//
// One entry point, teal_batched_retire_stops: teal_batched_retire's arguments plus the engines' history rows and the table of stop
// rows (include/teal_hip.h, TEAL_STOP_*).  It takes the old launch's place while the feature is on, so a step has as many launches
// as before; with a slot's MIN, NIDS and NSEQ all 0 the slot state and the positions leave as teal_batched_retire leaves them.
//
// One workgroup (the active word has a single writer) of 8 waves, wave w serving slot w.  Lane 8 q + j compares element j of
// sequence q — the last element against this step's token, the others against the history row — and lanes 0..15 compare the stop
// ids.  The launch sits at the end of a step that has streamed the model's weights through every cache, so its loads miss and what
// it costs is the number of loads that wait for one another: the whole stop row and the slot's words are loaded at once, whatever
// the counts in the row say, and the history needs one more round (seven words behind draw n, handed to the comparing lanes by a
// wave shuffle) — two rounds, as many as the plain retire launch has, with empty tables and with full ones.  Two wave ballots give
// the verdicts; lane 0 writes the slot's words, an LDS word per slot and one barrier hand the stops to thread 0, which writes the
// active word and the step counter.  No atomics, no workspace, every write a plain vector store: replays are bit-identical.
#include "teal_common.h"

namespace teal {

constexpr int kStopSlots = 8;  // rows of the table = the slots of a step
constexpr int kStopThreads = 64 * kStopSlots;

__global__ __launch_bounds__(kStopThreads) void batched_retire_stops_kernel(int* __restrict__ st, const int* __restrict__ tokens,
                                                                            int* __restrict__ pos, const int* __restrict__ history,
                                                                            const int history_stride, int* __restrict__ stops, const int B,
                                                                            const uint32_t mask, const int max_seq, const int count_step) {
    __shared__ int s_stop[kStopSlots];
    const int b = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // (every wave reads both words before the barrier; thread 0 writes them after it)
    const uint32_t act = (uint32_t)st[TEAL_SLOT_ACTIVE];
    const int step = st[TEAL_SLOT_STEP];
    bool stop = false;
    if (b < B && ((mask >> b) & 1u)) {  // wave-uniform, from the arguments alone: no load below waits for the active word
        // Round one — every word whose address the arguments give, in flight together: the slot's state words, its token and
        // position, and the whole stop row (lane l holds sequence word l, lanes 0..15 an id each).  All of them exist whatever the
        // counts say: the table has eight full rows.
        int* row = stops + b * TEAL_STOP_WORDS;
        const int q = lane >> 3, j = lane & 7;
        const int n = st[TEAL_SLOT_PRODUCED + b], budget = st[TEAL_SLOT_BUDGET + b] - 1, eos = st[TEAL_SLOT_EOS + b];
        const int t = tokens[b], p = pos[b];
        const int min_new = row[TEAL_STOP_MIN], nids_w = row[TEAL_STOP_NIDS], nseq_w = row[TEAL_STOP_NSEQ];
        const int id_w = row[TEAL_STOP_IDS + (lane & (TEAL_STOP_MAX_IDS - 1))];
        const int len = row[TEAL_STOP_SEQLEN + q];
        const int seq_w = row[TEAL_STOP_SEQ + lane];
        // Round two — the only loads that wait for data (n): the last seven draws before this one, lane k holding draw n - 1 - k.
        // A draw below 0 does not exist and an entry at or past the row's end is never read: neither can match
        int hist_w = 0, hist_ok = 0;
        if (lane < TEAL_STOP_MAX_SEQ_LEN - 1) {
            const int c = n - 1 - lane;
            hist_ok = c >= 0 && c < history_stride;
            if (hist_ok) hist_w = history[(size_t)b * (size_t)history_stride + c];
        }
        const bool mine = (act >> b) & 1u;
        const int nids = min(max(nids_w, 0), TEAL_STOP_MAX_IDS), nseq = min(max(nseq_w, 0), TEAL_STOP_MAX_SEQS);
        const bool armed = n + 1 >= min_new;
        // stop ids: lanes 0..15, one id each; the slot's EOS word is a stop token too
        const bool hit_id = armed && (__ballot(lane < nids && id_w == t) != 0ull || (eos >= 0 && t == eos));
        // stop sequences: lane 8 q + j holds element j of sequence q.  The sequence ends on this token, draw n; its element j < len - 1
        // is draw n - len + 1 + j, which lane len - 2 - j holds and which is >= 0 because len <= n + 1: only what this request
        // generated can match
        const int src = min(max(len - 2 - j, 0), TEAL_STOP_MAX_SEQ_LEN - 2);
        const int got = __shfl(hist_w, src, 64), got_ok = __shfl(hist_ok, src, 64);  // (every lane takes part)
        const bool live = armed && q < nseq && len >= 1 && len <= TEAL_STOP_MAX_SEQ_LEN && len <= n + 1;
        const bool ok = live && (j >= len || (j == len - 1 ? seq_w == t : (got_ok && seq_w == got)));
        const unsigned long long seq_ok = __ballot(ok);
        int hit_seq = -1;
#pragma unroll
        for (int s = TEAL_STOP_MAX_SEQS - 1; s >= 0; --s)
            if (((seq_ok >> (8 * s)) & 0xFFull) == 0xFFull) hit_seq = s;  // the lowest matching index
        const bool spent = budget <= 0, full = p >= max_seq;
        stop = mine && (hit_id || hit_seq >= 0 || spent || full);
        if (mine && lane == 0) {
            st[TEAL_SLOT_BUDGET + b] = budget;
            st[TEAL_SLOT_PRODUCED + b] = n + 1;
            if (stop) {
                st[TEAL_SLOT_FINISH + b] = step;
                row[TEAL_STOP_REASON] = hit_id ? TEAL_FINISH_STOP_TOKEN : hit_seq >= 0 ? TEAL_FINISH_STOP_SEQUENCE : spent ? TEAL_FINISH_LENGTH
                                                                                                                          : TEAL_FINISH_CACHE;
                row[TEAL_STOP_MATCH] = hit_id ? t : hit_seq;  // (-1 where neither fired)
                if (p > max_seq - 1) pos[b] = max_seq - 1;
            }
        }
    }
    if (lane == 0) s_stop[b] = stop ? 1 : 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t stopped = 0;
#pragma unroll
        for (int s = 0; s < kStopSlots; ++s) stopped |= (uint32_t)s_stop[s] << s;
        st[TEAL_SLOT_ACTIVE] = (int)(act & ~stopped);
        if (count_step) st[TEAL_SLOT_STEP] = step + 1;
    }
}

}  // namespace teal

using namespace teal;

extern "C" int teal_batched_retire_stops(int32_t* slot_state, const int32_t* tokens, int32_t* pos, const int32_t* history,
                                         int history_stride, int32_t* stops, int B, int slot_mask, int max_seq, int count_step,
                                         void* stream) {
    if (!slot_state || !tokens || !pos || !history || !stops) return TEAL_ERR_ARG;
    if (B < 1 || B > kStopSlots || max_seq < 1 || history_stride < TEAL_STOP_MAX_SEQ_LEN) return TEAL_ERR_ARG;
    hipLaunchKernelGGL(batched_retire_stops_kernel, dim3(1), dim3(kStopThreads), 0, reinterpret_cast<hipStream_t>(stream), slot_state,
                       tokens, pos, history, history_stride, stops, B, (uint32_t)slot_mask & 0xFFu, max_seq, count_step ? 1 : 0);
    return hipGetLastError() == hipSuccess ? TEAL_OK : TEAL_ERR_LAUNCH;
}
