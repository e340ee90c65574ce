// teal_chunked_attention.h — the chunked split-KV attention of the two dense passes that attend a cache: the verify / suffix pass
// (teal_speculative.hip: verify_attention_kernel, T <= 16 new tokens of ONE sequence) and the batched / slot step
// (teal_batched.hip: batched_attention_kernel, ONE new token of each of B sequences).  The second is the first at T = 1 with the
// token slot replaced by the sequence slot b, the caches moved to sequence b's and the partial row (h * R + slot) taken with
// R = B: one kernel body, one merge body, one host-side plan and one argument check, each typed here once.  The two units keep
// their __global__ wrappers (symbols, argument lists, launch bounds), the SLOTS early exit and their dispatch.
#pragma once
#include "teal_kv8.h"
#include "teal_slab.h"

namespace teal {

constexpr int kAttnChunk = 32;     // context rows a workgroup stages per round
constexpr int kAttnMaxSplit = 64;  // most splits of the context (partials per query row)
constexpr int kBatchMax = 8;       // sequences per batched launch: one 16-byte word of 16-bit activations per feature
constexpr int kBAttnMaxQ = 16;     // batched step: query heads of one KV head per workgroup

// ------------------------------------------------------------------------------------------------
// Attention of T new rows at positions p0 .. p0+T-1, p0 = clamp(pos, 0, max_seq - T), against the cache rows 0 .. p0+t of ONE
// sequence (k_cache / v_cache: that sequence's [n_kv][max_seq][HD]).  Grid x = split of the context, y = KV head; the workgroup
// serves the hq query heads from h0 = kvh * rep + grp * hq on, for ALL T rows (hq * T <= MAXQ query rows), so every K / V row it
// loads is used hq * T times.  Context rows are dealt in chunks of 32, chunk c to split c mod nsplit.  The new rows are rebuilt by
// every workgroup from the wqkv slabs (RoPE at p0 + t, the module path's rounding points) and read from LDS: the cache stores of
// rows p0 .. p0+T-1 (split 0, group 0 only) are for LATER launches — nothing written in this launch is read back by it.  Each
// workgroup leaves an un-normalised partial {m, l, o[HD]} per query row at partials[((h * R + row slot) * nsplit + sp)];
// chunked_merge_body rescales and sums them in split order.
//   MAXQ  query rows per workgroup: sizes the LDS and the accumulators a thread holds
//   KR    token / sequence slots per slab column (teal_slab.h)
//   NR    new K / V rows held in LDS.  NR = KR: the rows are slots 0 .. T-1 (slab_column).  NR = 1: T is 1 and the one row is
//         slot `slot`; both forms add the slices in order from +0.
//   KV8   the cache format (teal_kv8.h; NR = 1 only).  false: 16-bit rows.  true: k_cache / v_cache are [n_kv][max_seq][HD] e4m3fn
//         codes and k_scales / v_scales the rows' [n_kv][max_seq] power-of-two scales.  Only the staging loop's load and the
//         writer's store know: a cached row reaches ks / vs as float(code) * scale — exact — and the new row is attended from
//         kn / vn unquantised, so everything after the staging loop is the 16-bit launch's on a cache of the dequantised values.
// ------------------------------------------------------------------------------------------------
template <bool BF16, int HD, int MAXQ, int KR, int NR, bool KV8 = false>
__device__ __forceinline__ void chunked_attention_body(const float* __restrict__ slabs, const int split, const int pos,
                                                       const uint16_t* __restrict__ rope, kv_elem_t<KV8>* __restrict__ k_cache,
                                                       kv_elem_t<KV8>* __restrict__ v_cache, float* __restrict__ partials, const int T_rows,
                                                       const int slot, const int R, const int n_head, const int n_kv, const int hq,
                                                       const int grp, const int max_seq, const float scale,
                                                       float* __restrict__ k_scales = nullptr, float* __restrict__ v_scales = nullptr) {
    constexpr bool ONE = NR == 1;
    static_assert(ONE || !KV8, "the fp8 cache is the batched step's: one new row per launch");
    constexpr int C = kAttnChunk, NT = 256, OJ = (MAXQ * HD + NT - 1) / NT, QSTEP = NT / HD;
    __shared__ float qs[MAXQ][HD + 1];
    __shared__ float kn[NR][ONE ? HD : HD + 1];  // (a single row needs no padding against bank conflicts)
    __shared__ float vn[NR][HD];
    __shared__ float ks[C][HD + 1];
    __shared__ float vs[C][HD];
    __shared__ float sc[MAXQ][C + 1];
    __shared__ float mrow[MAXQ], lrow[MAXQ], alph[MAXQ];
    const int tid = threadIdx.x, sp = blockIdx.x, nsplit = gridDim.x, kvh = blockIdx.y;
    const int T = ONE ? 1 : T_rows;
    const int rep = n_head / n_kv, h0 = kvh * rep + grp * hq, NQ = hq * T;
    // (a caller past the cache is clamped into it: the output is then meaningless, the memory stays intact)
    const int p0 = min(max(pos, 0), max_seq - T);
    const int ctx = p0 + T;
    const size_t nq = (size_t)n_head * HD, nkv = (size_t)n_kv * HD, ntot = nq + 2 * nkv;

    // ---- the new rows: q of the group's heads, k and v of the KV head, from the slabs (rounded), then RoPE (rounded)
    const int ncols = (hq + 2) * HD;
    for (int c = tid; c < ncols; c += NT) {
        const int part = c < hq * HD ? 0 : (c < (hq + 1) * HD ? 1 : 2);
        const int d = part == 0 ? c % HD : c - (hq + part - 1) * HD;
        const size_t col = part == 0 ? (size_t)h0 * HD + c : (part == 1 ? nq : nq + nkv) + (size_t)kvh * HD + d;
        if constexpr (ONE) {
            float a = 0.0f;
            for (int s = 0; s < split; ++s) a += slabs[((size_t)s * ntot + col) * KR + slot];
            const float r = bits_to_float(float_to_bits<BF16>(a), BF16);
            if (part == 0) qs[c / HD][d] = r;
            else if (part == 1) kn[0][d] = r;
            else vn[0][d] = r;
        } else {
            float r[KR];
            slab_column<BF16, KR>(slabs, split, ntot, col, r);
#pragma unroll
            for (int t = 0; t < KR; ++t) {
                if (t < T) {
                    if (part == 0) qs[(c / HD) * T + t][d] = r[t];
                    else if (part == 1) kn[t][d] = r[t];
                    else vn[t][d] = r[t];
                }
            }
        }
    }
    if (tid < MAXQ) { mrow[tid] = -INFINITY; lrow[tid] = 0.0f; }
    __syncthreads();
    for (int e = tid; e < (NQ + T) * (HD / 2); e += NT) {  // one (even, odd) pair per thread
        const int row = e / (HD / 2), i = e % (HD / 2);
        const int t = row % T;  // (the k rows follow NQ = hq * T query rows)
        float* x = row < NQ ? &qs[row][0] : &kn[t][0];
        const uint32_t cs = *reinterpret_cast<const uint32_t*>(rope + ((size_t)(p0 + t) * (HD / 2) + i) * 2);
        const float c = bits_to_float(cs & 0xFFFFu, BF16), sn = bits_to_float(cs >> 16, BF16);
        const float x0 = x[2 * i], x1 = x[2 * i + 1];
        x[2 * i] = bits_to_float(float_to_bits<BF16>(rope_even(x0, x1, c, sn)), BF16);
        x[2 * i + 1] = bits_to_float(float_to_bits<BF16>(rope_odd(x0, x1, c, sn)), BF16);
    }
    __syncthreads();
    kv_elem_t<KV8>* kc = k_cache + (size_t)kvh * max_seq * HD;
    kv_elem_t<KV8>* vc = v_cache + (size_t)kvh * max_seq * HD;
    [[maybe_unused]] float* ksc = nullptr;
    [[maybe_unused]] float* vsc = nullptr;
    if constexpr (KV8) { ksc = k_scales + (size_t)kvh * max_seq; vsc = v_scales + (size_t)kvh * max_seq; }
    if (sp == 0 && grp == 0) {  // one writer per (sequence, KV head); rows p0 .. p0+T-1 <= max_seq - 1
        if constexpr (KV8) {  // wave 0 the K row, wave 1 the V row: HD / 8 lanes of 8 codes each
            if (tid < 128 && (tid & 63) < HD / 8) {
                const bool isv = tid >= 64;
                const int d0 = (tid & 63) * 8;
                float x[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = isv ? vn[0][d0 + j] : kn[0][d0 + j];
                kv8_store_row<HD / 8>(x, (isv ? vc : kc) + (size_t)p0 * HD + d0, (isv ? vsc : ksc) + p0, d0 == 0);
            }
        } else {
            for (int e = tid; e < T * HD; e += NT) {
                const int t = e / HD, d = e % HD;
                kc[(size_t)(p0 + t) * HD + d] = float_to_bits<BF16>(kn[t][d]);
                vc[(size_t)(p0 + t) * HD + d] = float_to_bits<BF16>(vn[t][d]);
            }
        }
    }

    // ---- this split's chunks of the context: scores, online softmax, o += p V
    const int d_own = tid % HD;
    float o[OJ];
#pragma unroll
    for (int j = 0; j < OJ; ++j) o[j] = 0.0f;
    const int nchunks = (ctx + C - 1) / C;
    for (int ch = sp; ch < nchunks; ch += nsplit) {
        const int r0 = ch * C;
        __syncthreads();  // the previous chunk's ks / vs / sc are consumed
        constexpr int W = KV8 ? 16 : 8;  // elements of a row per 16-byte load
        for (int e = tid; e < C * (HD / W); e += NT) {
            const int rr = e / (HD / W), seg = e % (HD / W), r = r0 + rr;
            float kf[W], vf[W];
            if (r < p0) {  // cached rows (never the rows this launch writes)
                const u32x4 kw = *reinterpret_cast<const u32x4*>(kc + (size_t)r * HD + seg * W);
                const u32x4 vw = *reinterpret_cast<const u32x4*>(vc + (size_t)r * HD + seg * W);
                if constexpr (KV8) {
                    kv8_dequant16(kw, ksc[r], kf);
                    kv8_dequant16(vw, vsc[r], vf);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        kf[2 * j] = bits_to_float(kw[j] & 0xFFFFu, BF16); kf[2 * j + 1] = bits_to_float(kw[j] >> 16, BF16);
                        vf[2 * j] = bits_to_float(vw[j] & 0xFFFFu, BF16); vf[2 * j + 1] = bits_to_float(vw[j] >> 16, BF16);
                    }
                }
            } else {
                const int t = min(r - p0, T - 1);
#pragma unroll
                for (int j = 0; j < W; ++j) {
                    kf[j] = r < ctx ? kn[t][seg * W + j] : 0.0f;
                    vf[j] = r < ctx ? vn[t][seg * W + j] : 0.0f;
                }
            }
#pragma unroll
            for (int j = 0; j < W; ++j) { ks[rr][seg * W + j] = kf[j]; vs[rr][seg * W + j] = vf[j]; }
        }
        __syncthreads();
        for (int pq = tid; pq < NQ * C; pq += NT) {  // (query row, context row): causal — row r is visible to token t iff r <= p0 + t
            const int qi = pq / C, rr = pq % C, r = r0 + rr, t = qi % T;
            float s = -INFINITY;
            if (r <= p0 + t) {
                float a = 0.0f;
#pragma unroll 16
                for (int j = 0; j < HD; ++j) a = fmaf(qs[qi][j], ks[rr][j], a);
                s = bits_to_float(float_to_bits<BF16>(a * scale), BF16);
            }
            sc[qi][rr] = s;
        }
        __syncthreads();
        if (tid < NQ) {
            const int qi = tid;
            float mx = mrow[qi];
            for (int rr = 0; rr < C; ++rr) mx = fmaxf(mx, sc[qi][rr]);
            float a = 1.0f, l = lrow[qi];
            if (mx != -INFINITY) {
                a = mrow[qi] == -INFINITY ? 0.0f : expf(mrow[qi] - mx);
                l *= a;
                for (int rr = 0; rr < C; ++rr) {
                    const float e = sc[qi][rr] == -INFINITY ? 0.0f : expf(sc[qi][rr] - mx);
                    sc[qi][rr] = e;
                    l += e;
                }
                mrow[qi] = mx;
            } else {
                for (int rr = 0; rr < C; ++rr) sc[qi][rr] = 0.0f;
            }
            lrow[qi] = l;
            alph[qi] = a;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < OJ; ++j) {
            const int qi = tid / HD + j * QSTEP;
            if (qi < NQ) {
                float acc = o[j] * alph[qi];
#pragma unroll 8
                for (int rr = 0; rr < C; ++rr) acc = fmaf(sc[qi][rr], vs[rr][d_own], acc);
                o[j] = acc;
            }
        }
    }
    __syncthreads();
    // partials[((h * R + row slot) * nsplit + sp) * (HD + 2)] = {m, l, o[HD]}
#pragma unroll
    for (int j = 0; j < OJ; ++j) {
        const int qi = tid / HD + j * QSTEP;
        if (qi < NQ) {
            const int h = h0 + qi / T, rs = ONE ? slot : qi % T;
            float* p = partials + (((size_t)h * R + rs) * nsplit + sp) * (HD + 2);
            p[2 + d_own] = o[j];
            if (d_own == 0) { p[0] = mrow[qi]; p[1] = lrow[qi]; }
        }
    }
}

// yt[(h * hd + d) * KR + r] = round(sum_s o_s e^(m_s - M) / sum_s l_s e^(m_s - M)), splits in order.  Grid (n_head, KR) x hd
// threads; slots r >= R are zero, and with SLOTS so are the slots whose `active` bit is clear.
template <bool BF16, int KR, bool SLOTS>
__device__ __forceinline__ void chunked_merge_body(const float* __restrict__ partials, uint16_t* __restrict__ yt, const int R,
                                                   const int hd, const int nsplit, const int* __restrict__ active) {
    const int h = blockIdx.x, r = blockIdx.y, d = threadIdx.x;
    if (d >= hd) return;
    uint16_t* y = yt + ((size_t)h * hd + d) * KR + r;
    if (r >= R || (SLOTS && !((active[0] >> r) & 1))) { *y = 0; return; }
    const float* p = partials + ((size_t)h * R + r) * nsplit * (hd + 2);
    float M = -INFINITY;
    for (int s = 0; s < nsplit; ++s) M = fmaxf(M, p[(size_t)s * (hd + 2)]);
    float L = 0.0f, O = 0.0f;
    for (int s = 0; s < nsplit; ++s) {
        const float* q = p + (size_t)s * (hd + 2);
        const float l = q[1];
        if (l > 0.0f) {
            const float f = expf(q[0] - M);
            L = fmaf(l, f, L);
            O = fmaf(q[2 + d], f, O);
        }
    }
    *y = float_to_bits<BF16>(O / L);
}

// ------------------------------------------------------------------------------------------------
// Host side: what both launchers decide before their dispatch.
// ------------------------------------------------------------------------------------------------
struct ChunkedAttnPlan {
    int hq, groups, nsplit;  // query heads of a KV head per workgroup, workgroups per KV head, splits of the context
};

// hq: the most query heads of a KV head (rep of them) that divide it and fit `cap` query rows at `rows` new rows each.  nsplit:
// about two workgroups per CU at the longest context the cache holds, never more splits than chunks.
inline ChunkedAttnPlan chunked_attention_plan(const int num_cu, const int rep, const int n_kv, const int rows, const int seqs,
                                              const int max_seq, const int cap) {
    ChunkedAttnPlan p{1, 1, 1};
    for (int c = 1; c <= rep; ++c)
        if (rep % c == 0 && c * rows <= cap) p.hq = c;
    p.groups = rep / p.hq;
    const int chunks = (max_seq + kAttnChunk - 1) / kAttnChunk, wg = n_kv * p.groups * seqs;
    p.nsplit = (2 * num_cu + wg - 1) / wg;
    p.nsplit = p.nsplit < 1 ? 1 : (p.nsplit > kAttnMaxSplit ? kAttnMaxSplit : p.nsplit);
    if (p.nsplit > chunks) p.nsplit = chunks;
    return p;
}

// bytes of partials for `rows` query rows per head (tokens x sequences) at nsplit splits
inline size_t chunked_attention_ws_bytes(const int n_head, const int rows, const int nsplit, const int head_dim) {
    return (size_t)n_head * rows * nsplit * (head_dim + 2) * sizeof(float);
}

// the arguments both entry points share: `rows` new tokens (verify) or sequences (batched) of at most max_rows, a cache of at
// least min_seq rows
inline int chunked_attention_check(const float* qkv_slabs, const int split, const void* rope, const int32_t* pos, const void* k_cache,
                                   const void* v_cache, const void* yt, const float* partials, const int rows, const int max_rows,
                                   const int n_head, const int n_kv_head, const int head_dim, const int max_seq, const int min_seq,
                                   const int dtype) {
    if (!qkv_slabs || !rope || !pos || !k_cache || !v_cache || !yt || !partials || split < 1 || split > kSlabMaxSplit) return TEAL_ERR_ARG;
    if (dtype != TEAL_F16 && dtype != TEAL_BF16) return TEAL_ERR_DTYPE;
    if ((head_dim != 64 && head_dim != 128) || n_head <= 0 || n_kv_head <= 0 || n_head % n_kv_head || rows < 1 || rows > max_rows ||
        max_seq < min_seq)
        return TEAL_ERR_SHAPE;
    if (!aligned16(qkv_slabs) || !aligned16(k_cache) || !aligned16(v_cache)) return TEAL_ERR_ALIGN;
    return TEAL_OK;
}

}  // namespace teal
