// teal_kv8.hip — the fp8 KV cache of continuous batching (teal_amd/gpt_fast/batched.py, SlotDecodeEngine(kv_cache="fp8")): a cached
// K or V row of one KV head is hd e4m3fn codes and one power-of-two fp32 scale (teal_kv8.h has the rule).  Two entry points:
//
//   teal_kv8_quantize_rows                   rows 0 .. rows-1 of every head of every 16-bit cache tensor of a staging cache (K and V
//                                            of every layer) into a slot's code and scale tensors, in ONE launch at admission.
//   teal_batched_decode_attention_slots_kv8  teal_batched_decode_attention_slots on such caches: the chunked split-KV body
//                                            (teal_chunked_attention.h) with its cache-format parameter set — the same grid, plan,
//                                            partials and merge; only the staging loop's load and the writer's store differ.
#include "teal_chunked_attention.h"

namespace teal {
namespace {

constexpr int kQuantThreads = 256;

// grid (row blocks, n_heads, n_tensors); hd / 8 consecutive lanes per row, 8 values (one 16-byte load) per lane.  A lane whose row
// is >= rows does nothing: no code past row rows-1 of a head, no scale word past it, nothing between heads, no other tensor.
template <bool BF16, int HD>
__global__ __launch_bounds__(kQuantThreads) void kv8_quantize_rows_kernel(const uint64_t* __restrict__ src_table,
                                                                          const uint64_t* __restrict__ code_table,
                                                                          const uint64_t* __restrict__ scale_table, const int rows,
                                                                          const size_t src_head_rows, const size_t dst_head_rows) {
    constexpr int LANES = HD / 8, RPW = kQuantThreads / LANES;
    const uint32_t h = blockIdx.y, t = blockIdx.z;
    const int r = blockIdx.x * RPW + threadIdx.x / LANES, seg = threadIdx.x % LANES;
    if (r >= rows) return;  // (whole rows: the lanes of a row leave together)
    const auto* src = reinterpret_cast<const uint16_t*>(src_table[t]) + ((size_t)h * src_head_rows + r) * HD + seg * 8;
    auto* codes = reinterpret_cast<uint8_t*>(code_table[t]) + ((size_t)h * dst_head_rows + r) * HD + seg * 8;
    auto* scale = reinterpret_cast<float*>(scale_table[t]) + (size_t)h * dst_head_rows + r;
    const u32x4 w = *reinterpret_cast<const u32x4*>(src);
    float x[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        x[2 * j] = bits_to_float(w[j] & 0xFFFFu, BF16);
        x[2 * j + 1] = bits_to_float(w[j] >> 16, BF16);
    }
    kv8_store_row<LANES>(x, codes, scale, seg == 0);
}

// batched_attention_kernel (teal_batched.hip) with SLOTS on the fp8 caches [B][n_kv][max_seq][HD] codes, [B][n_kv][max_seq] scales
template <bool BF16, int HD>
__global__ __launch_bounds__(256) void batched_attention_kv8_kernel(const float* __restrict__ slabs, const int split,
                                                                    const int* __restrict__ pos_ptr, const uint16_t* __restrict__ rope,
                                                                    uint8_t* __restrict__ k_codes, uint8_t* __restrict__ v_codes,
                                                                    float* __restrict__ k_scales, float* __restrict__ v_scales,
                                                                    float* __restrict__ partials, const int B, const int n_head,
                                                                    const int n_kv, const int hq, const int groups, const int max_seq,
                                                                    const float scale, const int* __restrict__ active) {
    const int b = blockIdx.z / groups, grp = blockIdx.z % groups;
    if (!((active[0] >> b) & 1)) return;  // workgroup-uniform
    const size_t row_off = (size_t)b * n_kv * max_seq;
    chunked_attention_body<BF16, HD, kBAttnMaxQ, kBatchMax, 1, true>(slabs, split, pos_ptr[b], rope, k_codes + row_off * HD,
                                                                     v_codes + row_off * HD, partials, 1, b, B, n_head, n_kv, hq, grp,
                                                                     max_seq, scale, k_scales + row_off, v_scales + row_off);
}

template <bool BF16>
__global__ __launch_bounds__(128) void batched_merge_kv8_kernel(const float* __restrict__ partials, uint16_t* __restrict__ yt, const int B,
                                                                const int hd, const int nsplit, const int* __restrict__ active) {
    chunked_merge_body<BF16, kBatchMax, true>(partials, yt, B, hd, nsplit, active);
}

}  // namespace
}  // namespace teal

using namespace teal;

extern "C" {

int teal_kv8_quantize_rows(const void* src_table, const void* code_table, const void* scale_table, int n_tensors, int n_heads, int head_dim,
                           int rows, size_t src_head_rows, size_t dst_head_rows, int dtype, void* stream) {
    if (!src_table || !code_table || !scale_table || n_tensors <= 0 || n_heads <= 0 || rows < 0) return TEAL_ERR_ARG;
    if (dtype != TEAL_F16 && dtype != TEAL_BF16) return TEAL_ERR_DTYPE;
    if ((head_dim != 64 && head_dim != 128) || n_tensors > 65535 || n_heads > 65535 || (size_t)rows > src_head_rows ||
        (size_t)rows > dst_head_rows)
        return TEAL_ERR_SHAPE;
    if ((reinterpret_cast<uintptr_t>(src_table) | reinterpret_cast<uintptr_t>(code_table) | reinterpret_cast<uintptr_t>(scale_table)) & 7u)
        return TEAL_ERR_ALIGN;
    if (rows == 0) return TEAL_OK;
    const int rpw = kQuantThreads / (head_dim / 8);
    const dim3 grid((rows + rpw - 1) / rpw, n_heads, n_tensors);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    auto* s = reinterpret_cast<const uint64_t*>(src_table);
    auto* c = reinterpret_cast<const uint64_t*>(code_table);
    auto* f = reinterpret_cast<const uint64_t*>(scale_table);
#define TEAL_KQ(BF, HDV) hipLaunchKernelGGL((kv8_quantize_rows_kernel<BF, HDV>), grid, dim3(kQuantThreads), 0, st, s, c, f, rows, src_head_rows, dst_head_rows)
    if (dtype == TEAL_BF16) { if (head_dim == 128) TEAL_KQ(true, 128); else TEAL_KQ(true, 64); }
    else { if (head_dim == 128) TEAL_KQ(false, 128); else TEAL_KQ(false, 64); }
#undef TEAL_KQ
    return hipGetLastError() == hipSuccess ? TEAL_OK : TEAL_ERR_LAUNCH;
}

int teal_batched_decode_attention_slots_kv8(const float* qkv_slabs, int split, const void* rope, const int32_t* pos, const int32_t* active,
                                            void* k_codes, void* v_codes, float* k_scales, float* v_scales, void* yt, float* partials,
                                            size_t partials_bytes, int B, int n_head, int n_kv_head, int head_dim, int max_seq, int dtype,
                                            void* stream) {
    if (!active || !k_scales || !v_scales) return TEAL_ERR_ARG;
    const int rc = chunked_attention_check(qkv_slabs, split, rope, pos, k_codes, v_codes, yt, partials, B, kBatchMax, n_head, n_kv_head,
                                           head_dim, max_seq, 1, dtype);
    if (rc != TEAL_OK) return rc;
    DeviceCtx* ctx = device_ctx();
    if (!ctx) return TEAL_ERR_NO_DEVICE;
    const ChunkedAttnPlan pl = chunked_attention_plan(ctx->num_cu, n_head / n_kv_head, n_kv_head, 1, B, max_seq, kBAttnMaxQ);
    if (partials_bytes < chunked_attention_ws_bytes(n_head, B, pl.nsplit, head_dim)) return TEAL_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const float scale = 1.0f / sqrtf((float)head_dim);
    const dim3 grid(pl.nsplit, n_kv_head, pl.groups * B);
    auto* rp = reinterpret_cast<const uint16_t*>(rope);
    auto* kc = reinterpret_cast<uint8_t*>(k_codes);
    auto* vc = reinterpret_cast<uint8_t*>(v_codes);
    auto* y = reinterpret_cast<uint16_t*>(yt);
#define TEAL_BA8(BF, HDV) do { \
        hipLaunchKernelGGL((batched_attention_kv8_kernel<BF, HDV>), grid, dim3(256), 0, st, qkv_slabs, split, pos, rp, kc, vc, k_scales, v_scales, \
                           partials, B, n_head, n_kv_head, pl.hq, pl.groups, max_seq, scale, active); \
        hipLaunchKernelGGL((batched_merge_kv8_kernel<BF>), dim3(n_head, kBatchMax), dim3(128), 0, st, partials, y, B, head_dim, pl.nsplit, active); \
    } while (0)
    if (dtype == TEAL_BF16) { if (head_dim == 128) TEAL_BA8(true, 128); else TEAL_BA8(true, 64); }
    else { if (head_dim == 128) TEAL_BA8(false, 128); else TEAL_BA8(false, 64); }
#undef TEAL_BA8
    return hipGetLastError() == hipSuccess ? TEAL_OK : TEAL_ERR_LAUNCH;
}

}  // extern "C"
