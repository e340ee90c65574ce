// teal_prefix.hip — shared prompt prefixes of continuous batching: the K / V rows of a named token sequence are computed once,
// kept in a device store and copied into a slot's caches at admission (teal_amd/gpt_fast/batched.py, SlotDecodeEngine).
//
// One entry point, teal_kv_copy_rows: rows 0 .. rows-1 of every head of every cache tensor (K and V of every layer) in ONE launch.
// The tensors' base addresses come from two device tables, so an admission builds nothing on the host; within a head the rows are
// contiguous (row stride = row_bytes), so a (tensor, head) pair is one run of rows * row_bytes bytes moved in 16-byte words.
#include "teal_common.h"

namespace teal {

constexpr int kCopyThreads = 256;
constexpr int kCopyWordsPerThread = 4;  // 16 KiB per workgroup: four independent 16-byte loads in flight per lane

// grid (chunks of a head's run, n_heads, n_tensors).  Word w of the run is touched only when w < words: nothing past row rows-1 of
// a head, nothing between heads and no other tensor is written.
__global__ __launch_bounds__(kCopyThreads) void kv_copy_rows_kernel(const uint64_t* __restrict__ src_table, const uint64_t* __restrict__ dst_table,
                                                                    const uint32_t words, const size_t src_head_stride,
                                                                    const size_t dst_head_stride) {
    const uint32_t h = blockIdx.y, t = blockIdx.z;
    const auto* src = reinterpret_cast<const u32x4*>(src_table[t] + (size_t)h * src_head_stride);
    auto* dst = reinterpret_cast<u32x4*>(dst_table[t] + (size_t)h * dst_head_stride);
    const uint32_t w0 = blockIdx.x * (kCopyThreads * kCopyWordsPerThread) + threadIdx.x;
    u32x4 v[kCopyWordsPerThread];
#pragma unroll
    for (int i = 0; i < kCopyWordsPerThread; ++i) {
        const uint32_t w = w0 + i * kCopyThreads;
        if (w < words) v[i] = src[w];
    }
#pragma unroll
    for (int i = 0; i < kCopyWordsPerThread; ++i) {
        const uint32_t w = w0 + i * kCopyThreads;
        if (w < words) dst[w] = v[i];
    }
}

}  // namespace teal

using namespace teal;

extern "C" int teal_kv_copy_rows(const void* src_table, const void* dst_table, int n_tensors, int n_heads, int rows, int row_bytes,
                                 size_t src_head_stride, size_t dst_head_stride, void* stream) {
    if (!src_table || !dst_table || n_tensors <= 0 || n_heads <= 0 || rows < 0 || row_bytes <= 0) return TEAL_ERR_ARG;
    if (n_tensors > 65535 || n_heads > 65535) return TEAL_ERR_SHAPE;
    if (row_bytes & 15) return TEAL_ERR_ALIGN;
    const size_t run = (size_t)rows * (size_t)row_bytes;
    if (src_head_stride < run || dst_head_stride < run || run / 16 > 0x7fffffffu) return TEAL_ERR_SHAPE;
    if ((src_head_stride & 15) || (dst_head_stride & 15)) return TEAL_ERR_ALIGN;
    if (rows == 0) return TEAL_OK;
    const uint32_t words = (uint32_t)(run / 16);
    const uint32_t per_wg = kCopyThreads * kCopyWordsPerThread;
    const dim3 grid((words + per_wg - 1) / per_wg, n_heads, n_tensors);
    hipLaunchKernelGGL(kv_copy_rows_kernel, grid, dim3(kCopyThreads), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const uint64_t*>(src_table), reinterpret_cast<const uint64_t*>(dst_table), words, src_head_stride,
                       dst_head_stride);
    return hipGetLastError() == hipSuccess ? TEAL_OK : TEAL_ERR_LAUNCH;
}
