// teal_stream_attention.h — the stream split-KV body of the batched / slot step: ONE new token of each of B sequences against a long
// cache, shaped like a bandwidth-bound stream where chunked_attention_body (teal_chunked_attention.h, written for T <= 16 new rows)
// stages every cached row through LDS behind three barriers per 32 rows.  Grid, cache layout, slot predication, the partials
// {m, l, o[HD]} at partials[((h * B + b) * nsplit + sp) * (HD + 2)] and the merge (chunked_merge_body) are the chunked launch's;
// the row a launch stores is, word for word, the row the chunked launch stores.  Only the walk over the cached rows is new:
//
//   lanes     a lane owns 8 consecutive features of a cache row; a row is LPR = HD / 8 adjacent lanes (16 at head_dim 128, 8 at 64),
//             so one load instruction of a wave covers 64 / LPR consecutive rows: 1 KB contiguous of a 16-bit cache (16 bytes a
//             lane), 512 bytes of codes plus the rows' scale words of an fp8 cache (8 bytes a lane).  The map of features to
//             lanes is the same in both formats: after the conversion (kv8_dequant8: float(code) * scale, exact) one source.
//   streams   each group of LPR lanes is an independent online-softmax stream held in registers: q (8 features x HQ heads), and
//             per head a running m, l and o[8].  A workgroup of 4 waves is 16 (head_dim 128) or 32 (64) streams.  Per round a
//             stream requests the K and V words of UNR rows, then, in this fixed order: 8 FMAs a head in feature order, a DPP
//             butterfly over the LPR lanes (quad_perm 1, quad_perm 2, row_half_mirror, row_mirror: every lane ends with the same
//             bits), the score round16(dot * scale) — the chunked body's rounding point —, then ONE update of m / l / o over the
//             round's UNR rows in row order (UNR + 1 fp32 expf a head).  No LDS, no barrier, no cross-wave traffic in the loop.
//   dealing   cached rows 0 .. p_b - 1 go out in blocks of U = 4 waves x (64 / LPR) groups x UNR rows; block j belongs to split
//             j mod nsplit.  Inside a block row (w * UNR + u) * (64 / LPR) + g is wave w's group g at unroll step u: a wave's
//             load covers consecutive rows and a wave's round a contiguous UNR KB.  The dealing reads p_b and the launch
//             geometry, never the slot, the active word or a neighbour.  A row at or behind p_b is never loaded (its address is
//             clamped to row p_b - 1) and its score is -inf by selection: NaN there cannot reach a sum.
//   new row   row p_b is attended from LDS, unquantised, by stream 0 of the split that owns the block holding row p_b, after
//             that stream's cached rows.
//   exit      a wave's streams merge through __shfl_xor (LPR, 2 LPR, .. 32), the 4 wave results meet in LDS and are merged in
//             wave order into the workgroup's partial of each head.  An empty stream (m = -inf, l = 0) merges with factor 0 by
//             selection; a split without rows leaves l = 0, which chunked_merge_body skips.
//
// HQ (1, 2, 4, 8) sizes the registers; the launch's hq <= HQ heads are live, the others carry q = 0 and are not stored.  At HQ = 16
// q and o alone would take 256 VGPRs: the plan stops at 8 and splits a wider group over `groups` workgroups.
#pragma once
#include "teal_chunked_attention.h"

namespace teal {

constexpr int kStreamMaxQ = 8;  // query heads of one KV head per workgroup

// rows a stream requests per round: the registers HQ <= 2 leaves free hold twice the loads in flight
constexpr int stream_unroll(const int HQ) { return HQ <= 2 ? 8 : 4; }
// U, the rows of one workgroup round: the unit of the dealing
constexpr int stream_round_rows(const int HD, const int HQ) { return 4 * (64 / (HD / 8)) * stream_unroll(HQ); }
// the HQ a launch at hq heads per workgroup is compiled for
constexpr int stream_hq_class(const int hq) { return hq <= 1 ? 1 : (hq <= 2 ? 2 : (hq <= 4 ? 4 : 8)); }

template <int CTRL>
__device__ __forceinline__ float stream_dpp(const float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

// sum over the LPR lanes of a stream, the same bits in every lane (a + b and b + a are one number at every step)
template <int LPR>
__device__ __forceinline__ float stream_group_sum(float v) {
    v += stream_dpp<0xB1>(v);   // quad_perm [1, 0, 3, 2]
    v += stream_dpp<0x4E>(v);   // quad_perm [2, 3, 0, 1]
    v += stream_dpp<0x141>(v);  // row_half_mirror
    if constexpr (LPR == 16) v += stream_dpp<0x140>(v);  // row_mirror
    return v;
}

template <bool BF16, int HD, int HQ, bool KV8>
__device__ __forceinline__ void stream_attention_body(const float* __restrict__ slabs, const int split, const int pos,
                                                      const uint16_t* __restrict__ rope, kv_elem_t<KV8>* __restrict__ k_cache,
                                                      kv_elem_t<KV8>* __restrict__ v_cache, float* __restrict__ k_scales,
                                                      float* __restrict__ v_scales, float* __restrict__ partials, const int slot,
                                                      const int R, const int n_head, const int n_kv, const int hq, const int grp,
                                                      const int max_seq, const float scale) {
    constexpr int NT = 256, KR = kBatchMax, LPR = HD / 8, GPW = 64 / LPR, UNR = stream_unroll(HQ), U = stream_round_rows(HD, HQ);
    using raw_t = std::conditional_t<KV8, u32x2, u32x4>;  // a lane's 8 features of a row
    __shared__ float qs[HQ][HD];
    __shared__ float kn[HD];
    __shared__ float vn[HD];
    __shared__ float wm[4][HQ], wl[4][HQ];
    __shared__ float wo[4][HQ][HD];
    const int tid = threadIdx.x, sp = blockIdx.x, nsplit = gridDim.x, kvh = blockIdx.y;
    const int lane = tid & 63, w = tid >> 6, g = lane / LPR, seg = lane % LPR;
    const int rep = n_head / n_kv, h0 = kvh * rep + grp * hq;
    const int p0 = min(max(pos, 0), max_seq - 1);  // (a caller past the cache is clamped into it, as in the chunked body)
    const size_t nq = (size_t)n_head * HD, nkv = (size_t)n_kv * HD, ntot = nq + 2 * nkv;

    // ---- the new row, as chunked_attention_body builds it at NR = 1: slices summed in order from +0 and rounded, RoPE rounded
    const int ncols = (hq + 2) * HD;
    for (int c = tid; c < ncols; c += NT) {
        const int part = c < hq * HD ? 0 : (c < (hq + 1) * HD ? 1 : 2);
        const int d = part == 0 ? c % HD : c - (hq + part - 1) * HD;
        const size_t col = part == 0 ? (size_t)h0 * HD + c : (part == 1 ? nq : nq + nkv) + (size_t)kvh * HD + d;
        float a = 0.0f;
        for (int s = 0; s < split; ++s) a += slabs[((size_t)s * ntot + col) * KR + slot];
        const float r = bits_to_float(float_to_bits<BF16>(a), BF16);
        if (part == 0) qs[c / HD][d] = r;
        else if (part == 1) kn[d] = r;
        else vn[d] = r;
    }
    __syncthreads();
    for (int e = tid; e < (hq + 1) * (HD / 2); e += NT) {  // one (even, odd) pair per thread; the k row follows the hq query rows
        const int row = e / (HD / 2), i = e % (HD / 2);
        float* x = row < hq ? &qs[row][0] : &kn[0];
        const uint32_t cs = *reinterpret_cast<const uint32_t*>(rope + ((size_t)p0 * (HD / 2) + i) * 2);
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
    if (sp == 0 && grp == 0) {  // one writer per (sequence, KV head): row p0 <= max_seq - 1, for LATER launches
        if constexpr (KV8) {  // wave 0 the K row, wave 1 the V row: HD / 8 lanes of 8 codes each
            if (tid < 128 && (tid & 63) < HD / 8) {
                const bool isv = tid >= 64;
                const int d0 = (tid & 63) * 8;
                float x[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = isv ? vn[d0 + j] : kn[d0 + j];
                kv8_store_row<HD / 8>(x, (isv ? vc : kc) + (size_t)p0 * HD + d0, (isv ? vsc : ksc) + p0, d0 == 0);
            }
        } else {
            for (int d = tid; d < HD; d += NT) {
                kc[(size_t)p0 * HD + d] = float_to_bits<BF16>(kn[d]);
                vc[(size_t)p0 * HD + d] = float_to_bits<BF16>(vn[d]);
            }
        }
    }

    // ---- the stream's registers
    float q[HQ][8], o[HQ][8], m[HQ], l[HQ];
#pragma unroll
    for (int i = 0; i < HQ; ++i) {
        m[i] = -INFINITY;
        l[i] = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            q[i][j] = i < hq ? qs[i][seg * 8 + j] : 0.0f;
            o[i][j] = 0.0f;
        }
    }
    const auto widen = [](const raw_t wd, [[maybe_unused]] const float sc, float (&x)[8]) {
        if constexpr (KV8) {
            kv8_dequant8(wd, sc, x);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x[2 * j] = bits_to_float(wd[j] & 0xFFFFu, BF16);
                x[2 * j + 1] = bits_to_float(wd[j] >> 16, BF16);
            }
        }
    };

    // ---- this split's blocks of the cached rows 0 .. p0 - 1
    for (int blk = sp; blk * U < p0; blk += nsplit) {
        const int r0 = blk * U + w * (UNR * GPW) + g;  // the stream's rows: r0 + u * GPW
        raw_t kw[UNR], vw[UNR];
        [[maybe_unused]] float kscl[UNR], vscl[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {  // every load of the round before the first use
            const int rc = min(r0 + u * GPW, p0 - 1);
            kw[u] = *reinterpret_cast<const raw_t*>(kc + (size_t)rc * HD + seg * 8);
            vw[u] = *reinterpret_cast<const raw_t*>(vc + (size_t)rc * HD + seg * 8);
            if constexpr (KV8) { kscl[u] = ksc[rc]; vscl[u] = vsc[rc]; }
        }
        float s[HQ][UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            float kf[8];
            widen(kw[u], KV8 ? kscl[u] : 0.0f, kf);
            const bool seen = r0 + u * GPW < p0;
#pragma unroll
            for (int i = 0; i < HQ; ++i) {
                float a = 0.0f;
#pragma unroll
                for (int j = 0; j < 8; ++j) a = fmaf(q[i][j], kf[j], a);
                a = stream_group_sum<LPR>(a);
                s[i][u] = seen ? bits_to_float(float_to_bits<BF16>(a * scale), BF16) : -INFINITY;
            }
        }
        if (r0 < p0) {  // (whole streams: the LPR lanes of a row decide together; a stream's rows ascend with u)
#pragma unroll
            for (int i = 0; i < HQ; ++i) {
                float mn = m[i];
#pragma unroll
                for (int u = 0; u < UNR; ++u) mn = fmaxf(mn, s[i][u]);
                const float a = m[i] == -INFINITY ? 0.0f : expf(m[i] - mn);
                float ls = l[i] * a;
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    const float e = s[i][u] == -INFINITY ? 0.0f : expf(s[i][u] - mn);
                    s[i][u] = e;
                    ls += e;
                }
                m[i] = mn;
                l[i] = ls;
#pragma unroll
                for (int j = 0; j < 8; ++j) o[i][j] *= a;
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                float vf[8];
                widen(vw[u], KV8 ? vscl[u] : 0.0f, vf);
#pragma unroll
                for (int i = 0; i < HQ; ++i) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) o[i][j] = fmaf(s[i][u], vf[j], o[i][j]);
                }
            }
        }
    }

    // ---- the new row, from LDS: every stream forms the score (the butterfly stays wave-wide), the designated one takes it
    {
        const bool mine = sp == (p0 / U) % nsplit && w == 0 && g == 0;
        float kf[8], vf[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { kf[j] = kn[seg * 8 + j]; vf[j] = vn[seg * 8 + j]; }
#pragma unroll
        for (int i = 0; i < HQ; ++i) {
            float a = 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j) a = fmaf(q[i][j], kf[j], a);
            a = stream_group_sum<LPR>(a);
            const float sn = bits_to_float(float_to_bits<BF16>(a * scale), BF16);
            if (mine) {
                const float mn = fmaxf(m[i], sn);
                const float f = m[i] == -INFINITY ? 0.0f : expf(m[i] - mn);
                const float e = expf(sn - mn);
                m[i] = mn;
                l[i] = fmaf(l[i], f, e);
#pragma unroll
                for (int j = 0; j < 8; ++j) o[i][j] = fmaf(e, vf[j], o[i][j] * f);
            }
        }
    }

    // ---- exit: the wave's streams by butterfly, the 4 waves through LDS in wave order
#pragma unroll
    for (int dl = LPR; dl < 64; dl <<= 1) {
#pragma unroll
        for (int i = 0; i < HQ; ++i) {
            const float mo = __shfl_xor(m[i], dl), lo = __shfl_xor(l[i], dl);
            const float mn = fmaxf(m[i], mo);
            const float fa = m[i] == -INFINITY ? 0.0f : expf(m[i] - mn);
            const float fb = mo == -INFINITY ? 0.0f : expf(mo - mn);
            m[i] = mn;
            l[i] = fmaf(l[i], fa, lo * fb);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float oo = __shfl_xor(o[i][j], dl);
                o[i][j] = fmaf(o[i][j], fa, oo * fb);
            }
        }
    }
    if (g == 0) {
#pragma unroll
        for (int i = 0; i < HQ; ++i) {
            if (seg == 0) { wm[w][i] = m[i]; wl[w][i] = l[i]; }
#pragma unroll
            for (int j = 0; j < 8; ++j) wo[w][i][seg * 8 + j] = o[i][j];
        }
    }
    __syncthreads();
    for (int e = tid; e < hq * HD; e += NT) {
        const int i = e / HD, d = e % HD;
        float M = -INFINITY;
#pragma unroll
        for (int x = 0; x < 4; ++x) M = fmaxf(M, wm[x][i]);
        float Ls = 0.0f, Os = 0.0f;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            if (wl[x][i] > 0.0f) {
                const float f = expf(wm[x][i] - M);
                Ls = fmaf(wl[x][i], f, Ls);
                Os = fmaf(wo[x][i][d], f, Os);
            }
        }
        float* p = partials + (((size_t)(h0 + i) * R + slot) * nsplit + sp) * (HD + 2);
        p[2 + d] = Os;
        if (d == 0) { p[0] = M; p[1] = Ls; }
    }
}

}  // namespace teal
