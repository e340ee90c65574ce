// teal_stream_attention.hip — the batched / slot step's attention through the stream split-KV body (teal_stream_attention.h), an
// opt-in next to the chunked launches of teal_batched.hip and teal_kv8.hip (BatchedDecodeEngine(attention="stream")):
//
//   teal_batched_decode_attention_stream      16-bit caches; active == NULL: every slot (teal_batched_decode_attention's
//                                             contract), else teal_batched_decode_attention_slots'
//   teal_batched_decode_attention_stream_kv8  the fp8 caches of teal_kv8.hip, the same way
//
// Grid (nsplit, n_kv, groups * B) x 256 threads, the partials and the merge launch are the chunked launches'; the plan is
// chunked_attention_plan at a cap of kStreamMaxQ = 8 query heads per workgroup.
#include "teal_stream_attention.h"

namespace teal {
namespace {

// a workgroup of a slot whose `active` bit is clear exits before anything else (no cache row, no partials); active == nullptr: none is
template <bool BF16, int HD, int HQ, bool KV8>
__global__ __launch_bounds__(256) void stream_attention_kernel(const float* __restrict__ slabs, const int split,
                                                               const int* __restrict__ pos_ptr, const uint16_t* __restrict__ rope,
                                                               kv_elem_t<KV8>* __restrict__ k_cache, kv_elem_t<KV8>* __restrict__ v_cache,
                                                               float* __restrict__ k_scales, float* __restrict__ v_scales,
                                                               float* __restrict__ partials, const int B, const int n_head,
                                                               const int n_kv, const int hq, const int groups, const int max_seq,
                                                               const float scale, const int* __restrict__ active) {
    const int b = blockIdx.z / groups, grp = blockIdx.z % groups;
    if (active != nullptr && slot_off(active, b)) return;  // workgroup-uniform
    const size_t row_off = (size_t)b * n_kv * max_seq;
    stream_attention_body<BF16, HD, HQ, KV8>(slabs, split, pos_ptr[b], rope, k_cache + row_off * HD, v_cache + row_off * HD,
                                             KV8 ? k_scales + row_off : nullptr, KV8 ? v_scales + row_off : nullptr, partials, b, B,
                                             n_head, n_kv, hq, grp, max_seq, scale);
}

template <bool BF16, bool SLOTS>
__global__ __launch_bounds__(128) void stream_merge_kernel(const float* __restrict__ partials, uint16_t* __restrict__ yt, const int B,
                                                           const int hd, const int nsplit, const int* __restrict__ active) {
    chunked_merge_body<BF16, kBatchMax, SLOTS>(partials, yt, B, hd, nsplit, active);
}

template <bool BF16, int HD, int HQ, bool KV8>
void launch_one(const dim3 grid, hipStream_t st, const float* slabs, int split, const int32_t* pos, const uint16_t* rope, void* kc, void* vc,
                float* ks, float* vs, float* partials, int B, int n_head, int n_kv, const ChunkedAttnPlan& pl, int max_seq, float scale,
                const int32_t* active) {
    using elem = kv_elem_t<KV8>;
    hipLaunchKernelGGL((stream_attention_kernel<BF16, HD, HQ, KV8>), grid, dim3(256), 0, st, slabs, split, pos, rope,
                       reinterpret_cast<elem*>(kc), reinterpret_cast<elem*>(vc), ks, vs, partials, B, n_head, n_kv, pl.hq, pl.groups, max_seq,
                       scale, active);
}

template <bool BF16, int HD, bool KV8>
void launch_hq(const int hq_class, const dim3 grid, hipStream_t st, const float* slabs, int split, const int32_t* pos, const uint16_t* rope,
               void* kc, void* vc, float* ks, float* vs, float* partials, int B, int n_head, int n_kv, const ChunkedAttnPlan& pl,
               int max_seq, float scale, const int32_t* active) {
#define TEAL_SA(HQV) launch_one<BF16, HD, HQV, KV8>(grid, st, slabs, split, pos, rope, kc, vc, ks, vs, partials, B, n_head, n_kv, pl, max_seq, scale, active)
    switch (hq_class) {
        case 1: TEAL_SA(1); break;
        case 2: TEAL_SA(2); break;
        case 4: TEAL_SA(4); break;
        default: TEAL_SA(8); break;
    }
#undef TEAL_SA
}

// both entries: every refusal before any launch
template <bool KV8>
int stream_attention_launch(const float* qkv_slabs, int split, const void* rope, const int32_t* pos, const int32_t* active, void* k_cache,
                            void* v_cache, float* k_scales, float* v_scales, void* yt, float* partials, size_t partials_bytes, int B,
                            int n_head, int n_kv_head, int head_dim, int max_seq, int dtype, void* stream) {
    if (KV8 && (!k_scales || !v_scales)) return TEAL_ERR_ARG;
    const int rc = chunked_attention_check(qkv_slabs, split, rope, pos, k_cache, v_cache, yt, partials, B, kBatchMax, n_head, n_kv_head,
                                           head_dim, max_seq, 1, dtype);
    if (rc != TEAL_OK) return rc;
    DeviceCtx* ctx = device_ctx();
    if (!ctx) return TEAL_ERR_NO_DEVICE;
    const ChunkedAttnPlan pl = chunked_attention_plan(ctx->num_cu, n_head / n_kv_head, n_kv_head, 1, B, max_seq, kStreamMaxQ);
    if (partials_bytes < chunked_attention_ws_bytes(n_head, B, pl.nsplit, head_dim)) return TEAL_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const float scale = 1.0f / sqrtf((float)head_dim);
    const dim3 grid(pl.nsplit, n_kv_head, pl.groups * B);
    auto* rp = reinterpret_cast<const uint16_t*>(rope);
    auto* y = reinterpret_cast<uint16_t*>(yt);
    const int hc = stream_hq_class(pl.hq);
#define TEAL_SB(BF, HDV) do { \
        launch_hq<BF, HDV, KV8>(hc, grid, st, qkv_slabs, split, pos, rp, k_cache, v_cache, k_scales, v_scales, partials, B, n_head, n_kv_head, \
                                pl, max_seq, scale, active); \
        if (active) hipLaunchKernelGGL((stream_merge_kernel<BF, true>), dim3(n_head, kBatchMax), dim3(128), 0, st, partials, y, B, head_dim, \
                                       pl.nsplit, active); \
        else hipLaunchKernelGGL((stream_merge_kernel<BF, false>), dim3(n_head, kBatchMax), dim3(128), 0, st, partials, y, B, head_dim, \
                                pl.nsplit, nullptr); \
    } while (0)
    if (dtype == TEAL_BF16) { if (head_dim == 128) TEAL_SB(true, 128); else TEAL_SB(true, 64); }
    else { if (head_dim == 128) TEAL_SB(false, 128); else TEAL_SB(false, 64); }
#undef TEAL_SB
    return hipGetLastError() == hipSuccess ? TEAL_OK : TEAL_ERR_LAUNCH;
}

}  // namespace
}  // namespace teal

using namespace teal;

extern "C" {

int teal_batched_decode_attention_stream(const float* qkv_slabs, int split, const void* rope, const int32_t* pos, const int32_t* active,
                                         void* k_cache, void* v_cache, void* yt, float* partials, size_t partials_bytes, int B, int n_head,
                                         int n_kv_head, int head_dim, int max_seq, int dtype, void* stream) {
    return stream_attention_launch<false>(qkv_slabs, split, rope, pos, active, k_cache, v_cache, nullptr, nullptr, yt, partials, partials_bytes,
                                          B, n_head, n_kv_head, head_dim, max_seq, dtype, stream);
}

int teal_batched_decode_attention_stream_kv8(const float* qkv_slabs, int split, const void* rope, const int32_t* pos, const int32_t* active,
                                             void* k_codes, void* v_codes, float* k_scales, float* v_scales, void* yt, float* partials,
                                             size_t partials_bytes, int B, int n_head, int n_kv_head, int head_dim, int max_seq, int dtype,
                                             void* stream) {
    return stream_attention_launch<true>(qkv_slabs, split, rope, pos, active, k_codes, v_codes, k_scales, v_scales, yt, partials,
                                         partials_bytes, B, n_head, n_kv_head, head_dim, max_seq, dtype, stream);
}

}  // extern "C"
