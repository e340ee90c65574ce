// teal_batched.hip — batched decode: up to 8 sequences per fused step, hand-fused for gfx950 / CDNA4, wave64.
//
// TEAL's rule is per token: sequence b's projection is W . (x_b (.) [|x_b| > tau]) (the reference's SparsifyFn masks every
// token's activations element-wise against the site's threshold).  One step of B sequences therefore needs every weight row
// that ANY of them keeps — the union — read once, and each sequence adds only its own kept rows.  The layer is the prompt
// pass's chain over the same transposed hand-over layout [feature][8] (teal_slab.h), with two launches of its own:
//
//   batched_gemm_kernel       the prompt pass's GEMM (256-column tiles, row groups dealt to slices, the slice's activation rows
//                             staged in LDS once, one broadcast LDS read per row for the 8 sequences) plus one step after the
//                             staging: per tile, the slice's UNION row list (wave ballot over the OR of the B per-sequence
//                             compares, prefix sum into LDS).  Waves stream only listed rows; a sequence that does not keep a
//                             listed row sees a zero activation.  Rows outside the union are never loaded.
//   batched_attention_kernel  split-KV attention of B single-token queries, each at its own device position, over its own
//                             [n_kv][max_seq][hd] cache slab (the verify attention's structure, the sequence as a grid
//                             dimension), then batched_merge_kernel.
//
// Rounding points are the module path's (16-bit projection outputs, RoPE, attention output); sums are fp32.
#include "teal_chunked_attention.h"

namespace teal {
namespace {

constexpr int kBPhaseRows = 2048;      // rows a workgroup stages per phase (128 groups of 16)
constexpr int kBChunks = kBPhaseRows / 64;
constexpr int kBCountStride = 9;       // counts[slice][segment][9]: kept per sequence (0 .. 7), union (8)
constexpr int kBTauOff = (kBPhaseRows * 28 + (2 * kBChunks + 1 + 16 * 3 * kBCountStride) * 4 + 15) & ~15;  // LDS: the parked thresholds

struct BSegs {
    int nseg;
    int end[3];   // exclusive end column of each segment over [0, n_total)
    float tau[3];
};
struct BSegsTaus {  // the per-slot form: the threshold table in the place of the three thresholds
    int nseg;
    int end[3];
    const float* taus;  // device fp32 [3][8]: segment-major, slot-minor
};

// ------------------------------------------------------------------------------------------------
// slabs[slice][n][8] (fp32) = sum over the slice's rows m with float32(|x_b[m]|) > tau_seg of W^T[m][n] * x_b[m], sequences b < B.
//   grid (256-column tiles, row slices); rows in groups of 16, group q belongs to slice q mod split (the layout of teal_slab.h).
// Per phase (<= 2048 rows of the slice): stage the rows' 8 activations in LDS, each with a keep mask (bit 8 * ls + b: sequence b
// keeps the row under the threshold of the tile's ls-th segment), then compact the rows with a non-zero mask — the union of the
// tile — into a list in row order (chunks of 64 rows: one ballot each, a prefix sum over the chunk counts).  Wave w streams list
// entries w, w + 16, ...: one 512-byte row segment per load, the row's activations through one broadcast LDS read, and a lane's
// four columns take the mask bits of their own segment (a tile may hold up to three: the narrow k | v of small models).
// counts (optional): the first tile of each segment also writes, per slice, how many of the slice's rows each sequence keeps and
// how many the union holds under that segment's threshold.
// ------------------------------------------------------------------------------------------------
// SLOTS: `active` (device int32, bit b = slot b runs) is read once per workgroup; an inactive slot's activation is +0 and never
// kept, so it adds nothing to the union, the counts or any slab (its own columns are exactly 0).  SLOTS = false is the code of
// teal_batched_sparse_gemm.
// TAUS (with SLOTS only): slot b's threshold under segment s is taus[s][b] (device fp32 [3][8]); sg.tau is not read.  An inactive
// slot's column is never consulted (`live` is false before the compare).  The table's address travels in the segments argument
// (BSegsTaus), so the other instantiations keep their arguments and their code.
template <bool BF16, int NP, int PROD, bool TAUS, bool SLOTS>
__global__ __launch_bounds__(1024) void batched_gemm_kernel(const SlabProd pr, const std::conditional_t<TAUS, BSegsTaus, BSegs> sg,
                                                            const uint16_t* __restrict__ w0, const int ld0,
                                                            const uint16_t* __restrict__ w1, const int ld1, const int tiles0,
                                                            float* __restrict__ slabs, int* __restrict__ counts, const int Z, const int n_total,
                                                            const int* __restrict__ active) {
    static_assert(SLOTS || !TAUS, "per-slot thresholds need the slot form");
    constexpr int WAVES = 16, CPL = 4, BN = 256, U = NP <= 2 ? 8 : 4, PHASE_GROUPS = kBPhaseRows / 16;
    extern __shared__ __align__(16) unsigned char smem[];
    u32x4* xs = reinterpret_cast<u32x4*>(smem);                                     // [kBPhaseRows] activations of the phase's rows
    u32x2* list = reinterpret_cast<u32x2*>(smem + kBPhaseRows * 16);                // [kBPhaseRows] {local row, keep mask}
    uint32_t* msk = reinterpret_cast<uint32_t*>(smem + kBPhaseRows * 24);           // [kBPhaseRows] keep mask per local row
    int* coff = reinterpret_cast<int*>(smem + kBPhaseRows * 28);                    // [kBChunks + 1] list offset per chunk, total
    int* ccnt = coff + kBChunks + 1;                                                // [kBChunks] union rows per chunk
    int* wcnt = ccnt + kBChunks;                                                    // [WAVES][3][9] counts per wave
    float* red = reinterpret_cast<float*>(smem);                                    // epilogue: [WAVES][BN][2]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = blockIdx.x, slice = blockIdx.y, split = gridDim.y;
    const bool second = tile >= tiles0;
    const uint32_t ld = (uint32_t)(second ? ld1 : ld0);
    const int c0 = tile * BN;
    // the segments this tile's columns fall in: sfirst .. slast (local index ls = s - sfirst)
    // (the kernel-argument arrays are read with constant indices only: a dynamic index would copy them to scratch)
    const int e0 = sg.end[0], e1 = sg.end[1];
    const int sfirst = (c0 >= e0 ? 1 : 0) + (c0 >= e1 ? 1 : 0);
    const int slast = (c0 + BN - 1 >= e0 ? 1 : 0) + (c0 + BN - 1 >= e1 ? 1 : 0);
    const int nls = slast - sfirst + 1;
    [[maybe_unused]] float tau[3];
    if constexpr (!TAUS) {
        const float tau_s[3] = {sg.tau[0], sg.tau[1], sg.tau[2]};
#pragma unroll
        for (int i = 0; i < 3; ++i) tau[i] = sfirst + i == 0 ? tau_s[0] : (sfirst + i == 1 ? tau_s[1] : tau_s[2]);
    }
    const int lc = c0 + lane * CPL;  // this lane's four columns: one segment (boundaries are multiples of 8 columns)
    const uint32_t lshift = 8u * (uint32_t)((lc >= e0 ? 1 : 0) + (lc >= e1 ? 1 : 0) - sfirst);
    // segments whose kept counts this tile reports: those that start in it
    uint32_t count_segs = 0;
    if (counts) {
        const int starts[3] = {0, e0, e1};
#pragma unroll
        for (int s = 0; s < 3; ++s)
            if (s < sg.nseg && s >= sfirst && s <= slast && starts[s] / BN == tile) count_segs |= 1u << (s - sfirst);
    }
    int* mycnt = wcnt + wave * 3 * kBCountStride;  // this wave's counts, kept in LDS (registers are the streaming loop's)
    if (count_segs && lane < 3 * kBCountStride) mycnt[lane] = 0;

    uint32_t on = 0xFFu;  // slots that run
    if constexpr (TAUS) {
        // the threshold rows of the tile's segments: three 32-byte scalar loads whose addresses come from the arguments alone, so
        // they are in flight together with the active word's and one wait serves all four.  They are then parked in LDS — a copy
        // per wave, written and read back by the same lanes, so no barrier — and fetched again by each phase's staging: 24 scalar
        // registers held across the streaming loop are registers its pipeline needs.
        float t[3][8];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float* __restrict__ row = sg.taus + 8 * min(sfirst + i, 2);
#pragma unroll
            for (int b = 0; b < 8; ++b) t[i][b] = row[b];
        }
        on = (uint32_t)__builtin_amdgcn_readfirstlane(active[0]) & 0xFFu;
        float* park = reinterpret_cast<float*>(smem + kBTauOff) + wave * 24;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int b = 0; b < 8; ++b) park[i * 8 + b] = t[i][b];
    } else if constexpr (SLOTS) {
        on = (uint32_t)__builtin_amdgcn_readfirstlane(active[0]) & 0xFFu;
    }
    const int ngroups = Z >> 4;
    const int nj = (ngroups - slice + split - 1) / split;  // row groups of this slice
    const uint16_t* wbase = (second ? w1 : w0) + (size_t)(second ? tile - tiles0 : tile) * BN;
    f32x2 acc[CPL][NP];
#pragma unroll
    for (int c = 0; c < CPL; ++c)
#pragma unroll
        for (int p = 0; p < NP; ++p) acc[c][p] = (f32x2){0.0f, 0.0f};
    auto consume = [&](const u32x2 w, u32x4 xv, const uint32_t mk) {
        const uint32_t m8 = (mk >> lshift) & 0xFFu;  // this lane's segment: which sequences keep the row
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t keep = ((m8 >> (2 * q)) & 1u ? 0x0000FFFFu : 0u) | ((m8 >> (2 * q + 1)) & 1u ? 0xFFFF0000u : 0u);
            xv[q] &= keep;  // a dropped activation reads as +0
        }
        f32x2 xp[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) xp[p] = (f32x2){bits_to_float(xv[p] & 0xFFFFu, BF16), bits_to_float(xv[p] >> 16, BF16)};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float wl = bits_to_float(w[j] & 0xFFFFu, BF16), wh = bits_to_float(w[j] >> 16, BF16);
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                acc[2 * j][p] = __builtin_elementwise_fma((f32x2){wl, wl}, xp[p], acc[2 * j][p]);
                acc[2 * j + 1][p] = __builtin_elementwise_fma((f32x2){wh, wh}, xp[p], acc[2 * j + 1][p]);
            }
        }
    };
    for (int jb = 0; jb < nj; jb += PHASE_GROUPS) {
        const int nrows = min(PHASE_GROUPS, nj - jb) * 16;
        if (jb) __syncthreads();  // the previous phase's list and rows are consumed
        [[maybe_unused]] float rstd[8];
        if constexpr (PROD == 1) rstd_rows<8>(pr.sumsq, pr.nwg, lane, Z, pr.eps, rstd);
        // ---- staging: the rows' activations (16-bit, what the module path holds) and their keep masks
        [[maybe_unused]] float tslot[3][8];  // TAUS: [local segment][slot]
        if constexpr (TAUS) {
            const float* park = reinterpret_cast<const float*>(smem + kBTauOff) + wave * 24;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int b = 0; b < 8; ++b) tslot[i][b] = park[i * 8 + b];
        }
        for (int r = tid; r < nrows; r += 1024) {
            const uint32_t m = (uint32_t)(slice + split * (jb + (r >> 4))) * 16u + (uint32_t)(r & 15);
            float x[8];
            if constexpr (PROD == 0) {
                unpack_row<BF16>(*reinterpret_cast<const u32x4*>(pr.xt + (size_t)m * 8), x);
            } else if constexpr (PROD == 1) {  // x = round(round(h * rstd) * w)  (gpt-fast/model.py:289-291)
                const float nw = bits_to_float(pr.norm_w[m], BF16);
                unpack_row<BF16>(*reinterpret_cast<const u32x4*>(pr.xt + (size_t)m * 8), x);
#pragma unroll
                for (int s = 0; s < 8; ++s) x[s] = bits_to_float(norm_bits<BF16>(x[s], rstd[s], nw), BF16);
            } else {  // x = round(round(silu(round(gate))) * round(up))  (gpt-fast/model.py:258-259)
                float gv[8], uv[8];
                slab_column<BF16, 8>(pr.gu, pr.gu_split, (size_t)2 * Z, (size_t)m, gv);
                slab_column<BF16, 8>(pr.gu, pr.gu_split, (size_t)2 * Z, (size_t)Z + m, uv);
#pragma unroll
                for (int s = 0; s < 8; ++s) x[s] = bits_to_float(silu_mul_bits<BF16>(gv[s], uv[s]), BF16);
            }
            uint32_t mk = 0;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                if constexpr (SLOTS) {
                    const bool live = s < pr.rows && ((on >> s) & 1u);
                    x[s] = live ? x[s] : 0.0f;  // slots of absent or inactive sequences: zero, never kept
#pragma unroll
                    for (int i = 0; i < 3; ++i)
                        if (i < nls && live && keep_rule(x[s], TAUS ? tslot[i][s] : tau[i])) mk |= 1u << (8 * i + s);
                } else {
                    x[s] = s < pr.rows ? x[s] : 0.0f;  // slots of absent sequences: zero, never kept
#pragma unroll
                    for (int i = 0; i < 3; ++i)
                        if (i < nls && s < pr.rows && keep_rule(x[s], tau[i])) mk |= 1u << (8 * i + s);
                }
            }
            xs[r] = pack_row<BF16>(x);
            msk[r] = mk;
        }
        __syncthreads();
        // ---- the union row list: chunk counts (and the reported kept counts), prefix sum, compaction in row order
        const int nchunks = (nrows + 63) >> 6;
        for (int c = wave; c < nchunks; c += WAVES) {
            const int r = c * 64 + lane;
            const uint32_t mk = r < nrows ? msk[r] : 0u;
            const unsigned long long ball = __ballot(mk != 0u);
            if (lane == 0) ccnt[c] = __popcll(ball);
            if (count_segs) {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    if (!((count_segs >> i) & 1u)) continue;
                    int n[kBCountStride];
#pragma unroll
                    for (int b = 0; b < 8; ++b) n[b] = __popcll(__ballot((mk >> (8 * i + b)) & 1u));
                    n[8] = __popcll(__ballot(((mk >> (8 * i)) & 0xFFu) != 0u));
                    if (lane == 0) {
#pragma unroll
                        for (int b = 0; b < kBCountStride; ++b) mycnt[i * kBCountStride + b] += n[b];
                    }
                }
            }
        }
        __syncthreads();
        if (wave == 0) {
            const int v = lane < nchunks ? ccnt[lane] : 0;
            const int incl = wave_incl_scan(v, lane);
            if (lane < nchunks) coff[lane] = incl - v;
            if (lane == 63) coff[kBChunks] = incl;
        }
        __syncthreads();
        for (int c = wave; c < nchunks; c += WAVES) {
            const int r = c * 64 + lane;
            const uint32_t mk = r < nrows ? msk[r] : 0u;
            const unsigned long long ball = __ballot(mk != 0u);
            if (mk) list[coff[c] + lane_rank(ball)] = (u32x2){(uint32_t)r, mk};
        }
        __syncthreads();
        const int nlist = coff[kBChunks];
        const int njw = nlist > wave ? (nlist - wave + WAVES - 1) / WAVES : 0;  // this wave's entries: wave + 16 j
        // ---- stream the listed rows: two batches of U rows in flight (the pipeline of prefill_gemm_kernel, teal_prefill.hip)
        // (the list entry is read again where the row is consumed: held across the pipeline it cost 32 scalar registers and
        //  spilled the kernel)
        auto issue = [&](u32x2 (&w)[U], const int j0, auto guard) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = decltype(guard)::value ? min(j0 + u, njw - 1) : j0 + u;
                const uint32_t lr = __builtin_amdgcn_readfirstlane(list[j * WAVES + wave][0]);  // wave-uniform: one broadcast read
                const uint32_t m = (uint32_t)(slice + split * (jb + (int)(lr >> 4))) * 16u + (lr & 15u);
                w[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(wbase + (size_t)m * ld) + (uint32_t)lane);
            }
        };
        auto consume_batch = [&](const u32x2 (&w)[U], const int j0, auto guard) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = decltype(guard)::value ? min(j0 + u, njw - 1) : j0 + u;
                const u32x2 e = list[j * WAVES + wave];
                const uint32_t mk = (decltype(guard)::value && j0 + u >= njw) ? 0u : e[1];  // repeated entries add nothing
                consume(w[u], xs[e[0]], mk);
            }
        };
        constexpr std::false_type full{};
        constexpr std::true_type guarded{};
        u32x2 wa[U], wb[U];
        const int nfull = njw / (2 * U);
        int j0 = 0;
        if (nfull > 0) {
            issue(wa, 0, full);
            __builtin_amdgcn_sched_barrier(0);
            for (int it = 0; it < nfull; ++it, j0 += 2 * U) {
                issue(wb, j0 + U, full);
                __builtin_amdgcn_sched_barrier(0);
                consume_batch(wa, j0, full);
                __builtin_amdgcn_sched_barrier(0);
                if (it + 1 < nfull) issue(wa, j0 + 2 * U, full);
                __builtin_amdgcn_sched_barrier(0);
                consume_batch(wb, j0 + U, full);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (j0 < njw) {  // the partial pair: entries past the wave's last repeat it with an all-zero mask
            issue(wa, j0, guarded);
            const bool two = j0 + U < njw;
            if (two) issue(wb, j0 + U, guarded);
            __builtin_amdgcn_sched_barrier(0);
            consume_batch(wa, j0, guarded);
            if (two) consume_batch(wb, j0 + U, guarded);
        }
    }
    // the 16 waves in fixed order through LDS, one sequence pair per round
    const uint32_t col_base = (uint32_t)tile * BN;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        __syncthreads();
#pragma unroll
        for (int c = 0; c < CPL; ++c) *reinterpret_cast<f32x2*>(red + ((size_t)wave * BN + lane * CPL + c) * 2) = acc[c][p];
        __syncthreads();
        if (tid < BN * 2) {
            const int col = tid >> 1, e = tid & 1;
            float sum = 0.0f;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) sum += red[((size_t)w * BN + col) * 2 + e];
            slabs[((size_t)slice * n_total + col_base + col) * 8 + 2 * p + e] = sum;
        }
    }
    if (count_segs) {  // (workgroup-uniform) the waves' counts, added in wave order: counts[slice][segment][9]
        __syncthreads();
        if (tid < 3 * kBCountStride) {
            const int i = tid / kBCountStride, b = tid % kBCountStride;
            if ((count_segs >> i) & 1u) {
                int s = 0;
                for (int w = 0; w < WAVES; ++w) s += wcnt[(w * 3 + i) * kBCountStride + b];
                counts[((size_t)slice * 3 + sfirst + i) * kBCountStride + b] = s;
            }
        }
    }
}

// y[b][n] = round(sum of `split` slabs [slice][n][8] in slice order), b < B
template <bool BF16>
__global__ __launch_bounds__(256) void batched_round_rows_kernel(const float* __restrict__ slabs, const int split, const int N, const int B,
                                                                 uint16_t* __restrict__ y) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= N) return;
    float r[8];
    slab_column<BF16, 8>(slabs, split, (size_t)N, (size_t)col, r);
#pragma unroll
    for (int b = 0; b < 8; ++b)
        if (b < B) y[(size_t)b * N + col] = float_to_bits<BF16>(r[b]);
}

// ------------------------------------------------------------------------------------------------
// Attention of B single-token queries, sequence b at position p_b = clamp(pos[b], 0, max_seq - 1) against ITS cache rows 0 .. p_b:
// the chunked split-KV body (teal_chunked_attention.h) at T = 1 with the sequence as a grid dimension.  Grid (nsplit, n_kv,
// groups * B): a workgroup serves hq query heads of one KV head of one sequence; its one new row is slot b of the wqkv slabs, its
// caches are sequence b's [n_kv][max_seq][hd], its partials are row (h * B + b).
// ------------------------------------------------------------------------------------------------
// SLOTS: a workgroup of a slot whose `active` bit is clear exits before anything else (no cache row, no partials).
template <bool BF16, int HD, bool SLOTS>
__global__ __launch_bounds__(256) void batched_attention_kernel(const float* __restrict__ slabs, const int split,
                                                                const int* __restrict__ pos_ptr, const uint16_t* __restrict__ rope,
                                                                uint16_t* __restrict__ k_cache, uint16_t* __restrict__ v_cache,
                                                                float* __restrict__ partials, const int B, const int n_head,
                                                                const int n_kv, const int hq, const int groups, const int max_seq,
                                                                const float scale, const int* __restrict__ active) {
    const int b = blockIdx.z / groups, grp = blockIdx.z % groups;
    if constexpr (SLOTS) {
        if (!((active[0] >> b) & 1)) return;  // workgroup-uniform
    }
    const size_t seq_off = (size_t)b * n_kv * max_seq * HD;
    chunked_attention_body<BF16, HD, kBAttnMaxQ, kBatchMax, 1>(slabs, split, pos_ptr[b], rope, k_cache + seq_off, v_cache + seq_off, partials, 1,
                                                               b, B, n_head, n_kv, hq, grp, max_seq, scale);
}

// slots b >= B are zero (SLOTS: so are the slots whose `active` bit is clear)
template <bool BF16, bool SLOTS>
__global__ __launch_bounds__(128) void batched_merge_kernel(const float* __restrict__ partials, uint16_t* __restrict__ yt, const int B,
                                                            const int hd, const int nsplit, const int* __restrict__ active) {
    chunked_merge_body<BF16, kBatchMax, SLOTS>(partials, yt, B, hd, nsplit, active);
}

// ------------------------------------------------------------------------------------------------
// Retirement after the B samplers of one step (or after the first draw of an admission): thread b serves slot b.  An active
// slot in `mask` counts its token, spends one unit of budget, and stops — its bit cleared, the step recorded — on its EOS id,
// on an empty budget, or when its next position would be max_seq (that position is pulled back to max_seq - 1: no later
// launch may address a row past the cache).  Every field is written by plain vector stores; the active mask is assembled with
// a ballot and written by lane 0.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void batched_retire_kernel(int* __restrict__ st, const int* __restrict__ tokens, int* __restrict__ pos,
                                                            const int B, const uint32_t mask, const int max_seq, const int count_step) {
    const int b = threadIdx.x;
    const uint32_t act = (uint32_t)st[TEAL_SLOT_ACTIVE];
    const int step = st[TEAL_SLOT_STEP];
    const bool mine = b < B && ((mask >> b) & 1u) && ((act >> b) & 1u);
    bool stop = false;
    if (mine) {
        const int budget = st[TEAL_SLOT_BUDGET + b] - 1, eos = st[TEAL_SLOT_EOS + b], p = pos[b];
        stop = budget <= 0 || (eos >= 0 && tokens[b] == eos) || p >= max_seq;
        st[TEAL_SLOT_BUDGET + b] = budget;
        st[TEAL_SLOT_PRODUCED + b] = st[TEAL_SLOT_PRODUCED + b] + 1;
        if (stop) {
            st[TEAL_SLOT_FINISH + b] = step;
            if (p > max_seq - 1) pos[b] = max_seq - 1;
        }
    }
    const uint32_t stopped = (uint32_t)__ballot(stop);
    if (b == 0) {
        st[TEAL_SLOT_ACTIVE] = (int)(act & ~stopped);
        if (count_step) st[TEAL_SLOT_STEP] = step + 1;
    }
}

}  // namespace
}  // namespace teal

using namespace teal;

namespace {
// teal_batched_sparse_gemm (active == nullptr), teal_batched_sparse_gemm_slots and teal_batched_sparse_gemm_slot_taus (taus != nullptr)
int batched_gemm_launch(const teal_prefill_in_t* in, const teal_batched_segs_t* segs, const void* w0T, int ld0, int n0, const void* w1T,
                        int ld1, int n1, float* slabs, size_t slabs_bytes, int Z, int B, const int32_t* active, const float* taus, int32_t* counts,
                        int dtype, int* split_out, void* stream) {
    if (!in || !segs || !w0T || !slabs || !split_out || Z <= 0 || n0 <= 0 || n1 < 0 || (n1 > 0 && !w1T)) return TEAL_ERR_ARG;
    if (dtype != TEAL_F16 && dtype != TEAL_BF16) return TEAL_ERR_DTYPE;
    if (B < 1 || B > kBatchMax || (Z & 255) || Z > 65536 || (ld0 & 7) || (ld1 & 7) || ld0 < n0 || (n1 > 0 && ld1 < n1)) return TEAL_ERR_SHAPE;
    const int ntot = n0 + n1;
    if (n0 % 256 || n1 % 256) return TEAL_ERR_SHAPE;
    BSegs sg = {};
    sg.nseg = segs->nseg;
    if (sg.nseg < 1 || sg.nseg > 3) return TEAL_ERR_ARG;
    for (int s = 0; s < sg.nseg; ++s) {
        const int lo = s == 0 ? 0 : segs->col_end[s - 1];
        if (segs->col_end[s] <= lo || (segs->col_end[s] & 7)) return TEAL_ERR_SHAPE;
        sg.end[s] = segs->col_end[s];
        sg.tau[s] = segs->tau[s];
    }
    if (sg.end[sg.nseg - 1] != ntot) return TEAL_ERR_SHAPE;
    for (int s = sg.nseg; s < 3; ++s) { sg.end[s] = ntot; sg.tau[s] = sg.tau[sg.nseg - 1]; }
    const BSegsTaus sgt = {sg.nseg, {sg.end[0], sg.end[1], sg.end[2]}, taus};
    SlabProd pr;
    if (const int rc = slab_prod_fill(in, slabs, kSlabMaxSplit, B, &pr)) return rc;
    if (!aligned16(w0T) || (w1T && !aligned16(w1T)) || !aligned16(slabs)) return TEAL_ERR_ALIGN;
    if (taus && (reinterpret_cast<uintptr_t>(taus) & 31)) return TEAL_ERR_ALIGN;  // each row is one 32-byte scalar load
    DeviceCtx* ctx = device_ctx();
    if (!ctx) return TEAL_ERR_NO_DEVICE;
    constexpr int bn = 256;
    const int tiles = ntot / bn, split = slab_gemm_split(ctx->num_cu, tiles, Z, kSlabMaxSplit);
    if (slabs_bytes < (size_t)split * ntot * 8 * sizeof(float)) return TEAL_ERR_WORKSPACE;
    const dim3 grid(tiles, split), block(1024);
    const size_t lds = taus ? (size_t)kBTauOff + 16 * 24 * sizeof(float)
                            : (size_t)kBPhaseRows * 28 + (size_t)(2 * kBChunks + 1) * sizeof(int) + (size_t)16 * 3 * kBCountStride * sizeof(int);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int np = (B + 1) / 2, tiles0 = n0 / bn;
    auto* a = reinterpret_cast<const uint16_t*>(w0T);
    auto* b = reinterpret_cast<const uint16_t*>(w1T);
    int* cnt = reinterpret_cast<int*>(counts);
#define TEAL_BG(BF, NPV, PR) do { if (taus) hipLaunchKernelGGL((batched_gemm_kernel<BF, NPV, PR, true, true>), grid, block, lds, st, pr, sgt, \
        a, ld0, b, ld1, tiles0, slabs, cnt, Z, ntot, active); \
    else if (active) hipLaunchKernelGGL((batched_gemm_kernel<BF, NPV, PR, false, true>), grid, block, lds, st, pr, sg, a, ld0, b, \
        ld1, tiles0, slabs, cnt, Z, ntot, active); \
    else hipLaunchKernelGGL((batched_gemm_kernel<BF, NPV, PR, false, false>), grid, block, lds, st, pr, sg, a, ld0, b, ld1, tiles0, slabs, cnt, Z, ntot, \
                            nullptr); } while (0)
#define TEAL_BG_PR(BF, NPV) do { if (in->mode == TEAL_PREFILL_IN_NORM) TEAL_BG(BF, NPV, 1); else if (in->mode == TEAL_PREFILL_IN_SILU_MUL) TEAL_BG(BF, NPV, 2); else TEAL_BG(BF, NPV, 0); } while (0)
#define TEAL_BG_NP(BF) do { switch (np) { case 1: TEAL_BG_PR(BF, 1); break; case 2: TEAL_BG_PR(BF, 2); break; case 3: TEAL_BG_PR(BF, 3); break; \
    default: TEAL_BG_PR(BF, 4); } } while (0)
    if (dtype == TEAL_BF16) TEAL_BG_NP(true); else TEAL_BG_NP(false);
#undef TEAL_BG_NP
#undef TEAL_BG_PR
#undef TEAL_BG
    *split_out = split;
    return hipGetLastError() == hipSuccess ? TEAL_OK : TEAL_ERR_LAUNCH;
}
}  // namespace

extern "C" {

int teal_batched_sparse_gemm(const teal_prefill_in_t* in, const teal_batched_segs_t* segs, const void* w0T, int ld0, int n0, const void* w1T,
                             int ld1, int n1, float* slabs, size_t slabs_bytes, int Z, int B, int32_t* counts, int dtype, int* split_out,
                             void* stream) {
    return batched_gemm_launch(in, segs, w0T, ld0, n0, w1T, ld1, n1, slabs, slabs_bytes, Z, B, nullptr, nullptr, counts, dtype, split_out, stream);
}

int teal_batched_sparse_gemm_slots(const teal_prefill_in_t* in, const teal_batched_segs_t* segs, const void* w0T, int ld0, int n0,
                                   const void* w1T, int ld1, int n1, float* slabs, size_t slabs_bytes, int Z, int B, const int32_t* active,
                                   int32_t* counts, int dtype, int* split_out, void* stream) {
    if (!active) return TEAL_ERR_ARG;
    return batched_gemm_launch(in, segs, w0T, ld0, n0, w1T, ld1, n1, slabs, slabs_bytes, Z, B, active, nullptr, counts, dtype, split_out, stream);
}

int teal_batched_sparse_gemm_slot_taus(const teal_prefill_in_t* in, const teal_batched_segs_t* segs, const void* w0T, int ld0, int n0,
                                       const void* w1T, int ld1, int n1, float* slabs, size_t slabs_bytes, int Z, int B,
                                       const int32_t* active, const float* taus, int32_t* counts, int dtype, int* split_out, void* stream) {
    if (!active || !taus) return TEAL_ERR_ARG;
    return batched_gemm_launch(in, segs, w0T, ld0, n0, w1T, ld1, n1, slabs, slabs_bytes, Z, B, active, taus, counts, dtype, split_out, stream);
}

int teal_batched_round_rows(const float* slabs, int split, int N, int B, void* y, int dtype, void* stream) {
    if (!slabs || !y || split < 1 || split > kSlabMaxSplit || N <= 0) return TEAL_ERR_ARG;
    if (dtype != TEAL_F16 && dtype != TEAL_BF16) return TEAL_ERR_DTYPE;
    if (B < 1 || B > kBatchMax) return TEAL_ERR_SHAPE;
    if (!aligned16(slabs)) return TEAL_ERR_ALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((N + 255) / 256);
    auto* yo = reinterpret_cast<uint16_t*>(y);
    if (dtype == TEAL_BF16) hipLaunchKernelGGL((batched_round_rows_kernel<true>), grid, dim3(256), 0, st, slabs, split, N, B, yo);
    else hipLaunchKernelGGL((batched_round_rows_kernel<false>), grid, dim3(256), 0, st, slabs, split, N, B, yo);
    return hipGetLastError() == hipSuccess ? TEAL_OK : TEAL_ERR_LAUNCH;
}

size_t teal_batched_decode_attention_ws_bytes(int B, int n_head, int head_dim) {
    return chunked_attention_ws_bytes(n_head, B < 1 ? 1 : B, kAttnMaxSplit, head_dim);
}

}  // extern "C"

namespace {
// teal_batched_decode_attention (active == nullptr) and teal_batched_decode_attention_slots: the same grid and nsplit either way
int batched_attention_launch(const float* qkv_slabs, int split, const void* rope, const int32_t* pos, const int32_t* active, void* k_cache,
                             void* v_cache, void* yt, float* partials, size_t partials_bytes, int B, int n_head, int n_kv_head, int head_dim,
                             int max_seq, int dtype, void* stream) {
    const int rc = chunked_attention_check(qkv_slabs, split, rope, pos, k_cache, v_cache, yt, partials, B, kBatchMax, n_head, n_kv_head,
                                           head_dim, max_seq, 1, dtype);
    if (rc != TEAL_OK) return rc;
    DeviceCtx* ctx = device_ctx();
    if (!ctx) return TEAL_ERR_NO_DEVICE;
    const ChunkedAttnPlan pl = chunked_attention_plan(ctx->num_cu, n_head / n_kv_head, n_kv_head, 1, B, max_seq, kBAttnMaxQ);
    const int hq = pl.hq, groups = pl.groups, nsplit = pl.nsplit;
    if (partials_bytes < chunked_attention_ws_bytes(n_head, B, nsplit, head_dim)) return TEAL_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const float scale = 1.0f / sqrtf((float)head_dim);
    const dim3 grid(nsplit, n_kv_head, groups * B);
    auto* rp = reinterpret_cast<const uint16_t*>(rope);
    auto* kc = reinterpret_cast<uint16_t*>(k_cache);
    auto* vc = reinterpret_cast<uint16_t*>(v_cache);
    auto* y = reinterpret_cast<uint16_t*>(yt);
#define TEAL_BA(BF, HDV) do { \
        if (active) { \
            hipLaunchKernelGGL((batched_attention_kernel<BF, HDV, true>), grid, dim3(256), 0, st, qkv_slabs, split, pos, rp, kc, vc, partials, \
                               B, n_head, n_kv_head, hq, groups, max_seq, scale, active); \
            hipLaunchKernelGGL((batched_merge_kernel<BF, true>), dim3(n_head, kBatchMax), dim3(128), 0, st, partials, y, B, head_dim, nsplit, \
                               active); \
        } else { \
            hipLaunchKernelGGL((batched_attention_kernel<BF, HDV, false>), grid, dim3(256), 0, st, qkv_slabs, split, pos, rp, kc, vc, partials, \
                               B, n_head, n_kv_head, hq, groups, max_seq, scale, nullptr); \
            hipLaunchKernelGGL((batched_merge_kernel<BF, false>), dim3(n_head, kBatchMax), dim3(128), 0, st, partials, y, B, head_dim, nsplit, \
                               nullptr); \
        } } while (0)
    if (dtype == TEAL_BF16) { if (head_dim == 128) TEAL_BA(true, 128); else TEAL_BA(true, 64); }
    else { if (head_dim == 128) TEAL_BA(false, 128); else TEAL_BA(false, 64); }
#undef TEAL_BA
    return hipGetLastError() == hipSuccess ? TEAL_OK : TEAL_ERR_LAUNCH;
}
}  // namespace

extern "C" {

int teal_batched_decode_attention(const float* qkv_slabs, int split, const void* rope, const int32_t* pos, void* k_cache, void* v_cache,
                                  void* yt, float* partials, size_t partials_bytes, int B, int n_head, int n_kv_head, int head_dim,
                                  int max_seq, int dtype, void* stream) {
    return batched_attention_launch(qkv_slabs, split, rope, pos, nullptr, k_cache, v_cache, yt, partials, partials_bytes, B, n_head,
                                    n_kv_head, head_dim, max_seq, dtype, stream);
}

int teal_batched_decode_attention_slots(const float* qkv_slabs, int split, const void* rope, const int32_t* pos, const int32_t* active,
                                        void* k_cache, void* v_cache, void* yt, float* partials, size_t partials_bytes, int B, int n_head,
                                        int n_kv_head, int head_dim, int max_seq, int dtype, void* stream) {
    if (!active) return TEAL_ERR_ARG;
    return batched_attention_launch(qkv_slabs, split, rope, pos, active, k_cache, v_cache, yt, partials, partials_bytes, B, n_head,
                                    n_kv_head, head_dim, max_seq, dtype, stream);
}

int teal_batched_retire(int32_t* slot_state, const int32_t* tokens, int32_t* pos, int B, int slot_mask, int max_seq, int count_step,
                        void* stream) {
    if (!slot_state || !tokens || !pos || max_seq < 1) return TEAL_ERR_ARG;
    if (B < 1 || B > kBatchMax) return TEAL_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(batched_retire_kernel, dim3(1), dim3(64), 0, st, slot_state, tokens, pos, B, (uint32_t)slot_mask & 0xFFu, max_seq,
                       count_step ? 1 : 0);
    return hipGetLastError() == hipSuccess ? TEAL_OK : TEAL_ERR_LAUNCH;
}

}  // extern "C"
