// teal_kernels.hip — host side of libteal_hip.so: the C-ABI entry points of the sparse GEMV (include/teal_hip.h), which
// turn their arguments into a request, the driver that plans a request and launches what the plan says (run_gemv), and the
// small kernels around it (ordered split-K reduce, gate|up epilogue, standalone compaction).  gfx950 / CDNA4, wave64.
//
//   teal_gemv_plan.h            the launch plan: geometry, kernel choice, wave-local facts — pure host arithmetic
//   teal_gemv_kernel.h          the sparse GEMV kernel template (the hot kernel; design notes there)
//   teal_gemv_w*_*.hip          its instantiations, one translation unit per (weight width, dtype)
//   teal_attention.hip          decode attention, its launch plan and entry points
//   teal_sampler.hip            fused top-k sampler and its entry points
//
// Replaces (reference tree FasterDecoding/TEAL @ 2024-10-22):
//   kernels/sparse_gemv.py:87-142   splitk_sparse_gemv (host wrapper, autotune, grid)  -> plan_gemv + run_gemv
//   kernels/sparse_gemv.py:196-237  qkv_gemv                                           -> teal_sparse_qkv_gemv*
//   kernels/sparse_gemv.py:8-12     init_to_zero("Y") pre-hook memset                  -> gone
#include "teal_producers.h"
#include "teal_gemv_plan.h"

#include <stdlib.h>

#include <mutex>
#include <vector>

namespace teal {

// ------------------------------------------------------------------------------------------------
// Workgroup-wide compaction of x against one threshold.
//   phase A: one ballot per 64-element chunk -> masks[] in LDS
//   phase B: wave 0 turns popcounts into an exclusive prefix (prefix[nch] = total kept)
// `nan_keeps`: GEMV mode — a NaN activation is kept so that it poisons the output like the
// reference's masked `0 * NaN` does; teal_compact uses the pure rule.
// ------------------------------------------------------------------------------------------------
template <int WAVES, bool BF16>
__device__ __forceinline__ void wg_ballot_prefix(const uint16_t* __restrict__ x, const int Z,
                                                 const float tau, const bool nan_keeps,
                                                 unsigned long long* masks, int* prefix) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nch = (Z + 63) >> 6;
    for (int c = wave; c < nch; c += WAVES) {
        const int m = (c << 6) + lane;
        bool k = false;
        if (m < Z) {
            const float v = bits_to_float(x[m], BF16);
            k = keep_rule(v, tau) || (nan_keeps && (v != v));
        }
        const unsigned long long mask = __ballot(k);
        if (lane == 0) masks[c] = mask;
    }
    __syncthreads();
    if (wave == 0) {
        int base = 0;
        for (int g0 = 0; g0 < nch; g0 += 64) {
            const int c = g0 + lane;
            const int v = (c < nch) ? __popcll(masks[c]) : 0;
            int incl = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            if (c < nch) prefix[c] = base + incl - v;
            base += __shfl(incl, 63);
        }
        if (lane == 0) prefix[nch] = base;
    }
    __syncthreads();
}


// y[n] = round(sum_s ws[s][n]) in slice order; one thread per column.
template <bool BF16>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const Params p) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= p.ws_ld) return;
    int s = 0;
    if (p.nseg > 1 && n >= p.seg[1].ws_off) s = 1;
    if (p.nseg > 2 && n >= p.seg[2].ws_off) s = 2;
    float sum = 0.0f;
    for (int k = 0; k < p.split; ++k) sum += p.ws[(size_t)k * p.ws_ld + n];
    reinterpret_cast<uint16_t*>(p.seg[s].y)[n - p.seg[s].ws_off] = (p.act0 && s == 0) ? silu_bits<BF16>(sum) : float_to_bits<BF16>(sum);
}

// h[n] = silu(gate[n]) * up[n] from the fp32 slabs of a 2-segment (gate | up) GEMV.
// gate and up are rounded to dtype first, silu is rounded, then the product is rounded — the same
// roundings the unfused fp16 sequence F.silu(g) * u performs (gpt-fast/model.py:258-259).
template <bool BF16>
__global__ __launch_bounds__(256) void gateup_silu_epilogue_kernel(const Params p, void* h) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int N = p.seg[0].ncols;
    if (n >= N) return;
    float g = 0.0f, u = 0.0f;
    for (int k = 0; k < p.split; ++k) {
        g += p.ws[(size_t)k * p.ws_ld + n];
        u += p.ws[(size_t)k * p.ws_ld + N + n];
    }
    const float g16 = round16<BF16>(g);
    const float u16 = round16<BF16>(u);
    reinterpret_cast<uint16_t*>(h)[n] = silu_mul_bits<BF16>(g16, u16);
}

// Standalone compaction (one workgroup): ascending kept indices + count to global memory.
template <bool BF16>
__global__ __launch_bounds__(1024) void compact_kernel(const uint16_t* __restrict__ x, const int Z,
                                                       const float tau, int32_t* __restrict__ idx_out,
                                                       int32_t* __restrict__ count_out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int nch = (Z + 63) >> 6;
    unsigned long long* masks = reinterpret_cast<unsigned long long*>(smem);
    int* prefix = reinterpret_cast<int*>(masks + nch);
    wg_ballot_prefix<16, BF16>(x, Z, tau, false, masks, prefix);
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    for (int c = wave; c < nch; c += 16) {
        const unsigned long long mask = masks[c];
        if ((mask >> lane) & 1ull) idx_out[prefix[c] + lane_rank(mask)] = (c << 6) + lane;
    }
    if (threadIdx.x == 0) *count_out = prefix[nch];
}


#ifdef TEAL_DIAGNOSTICS
// row_reduce_scatter against the __shfl_xor butterfly it replaces, on raw bit patterns: one wave per workgroup, lane l reads
// in[wave][l][0..8)
template <int LPR>
__global__ __launch_bounds__(64) void row_reduce_probe_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ scatter_out,
                                                              uint32_t* __restrict__ shuffle_out) {
    const int lane = threadIdx.x;
    const size_t base = ((size_t)blockIdx.x * 64 + lane) * 8;
    float v[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = b[j] = __builtin_bit_cast(float, in[base + j]);
    float lo, hi;
    row_reduce_scatter<LPR>(v, lo, hi);
    scatter_out[((size_t)blockIdx.x * 64 + lane) * 2] = __builtin_bit_cast(uint32_t, lo);
    scatter_out[((size_t)blockIdx.x * 64 + lane) * 2 + 1] = __builtin_bit_cast(uint32_t, hi);
#pragma unroll
    for (int off = LPR; off < 64; off <<= 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] += __shfl_xor(b[j], off);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) shuffle_out[base + j] = __builtin_bit_cast(uint32_t, b[j]);
}
#endif


// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------


#ifdef TEAL_DIAGNOSTICS  // libteal_hip_diag.so only (teal_common.h): the product library has no mutable switches
Config g_override = {0, 0, 0, 0};
unsigned long long* g_phase = nullptr;
size_t g_phase_stride = 0;  // > 0: consecutive GEMV launches stamp consecutive regions of this many uint64
int g_phase_seq = 0;
int g_wave_local = 1;
int g_fast = 1;  // lean kernel (teal_gemv_fast.h) where the shape qualifies
char g_last_desc[160] = "";  // template instantiation + grid of the most recent GEMV launch (teal_last_launch_desc)
#endif

// ---- per-device properties (immutable once cached) ---------------------------------------------------------------
constexpr int kMaxDevices = 64;
static DeviceCtx g_dev[kMaxDevices] = {};
static std::mutex g_dev_mu;

DeviceCtx* device_ctx() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (dev < 0 || dev >= kMaxDevices) return nullptr;
    DeviceCtx* c = &g_dev[dev];
    if (c->num_cu > 0) return c;
    std::lock_guard<std::mutex> lk(g_dev_mu);
    if (c->num_cu > 0) return c;
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cu <= 0) {
        (void)hipGetLastError();
        return nullptr;
    }
    c->gqa_lds_ok = attention_device_init();
    c->num_cu = cu;
    return c;
}

// ---- prepared workspaces (teal_workspace_init): host-side registry, keyed by the device pointer -------------------
struct WsEntry { const void* ws; size_t bytes; };
static std::vector<WsEntry> g_ws_reg;
static std::mutex g_ws_mu;

bool ws_prepared(const void* ws, size_t ws_bytes) {
    if (!ws || ws_bytes < kWsHeaderBytes) return false;
    std::lock_guard<std::mutex> lk(g_ws_mu);
    for (const WsEntry& e : g_ws_reg)
        if (e.ws == ws) return true;
    return false;
}


static GemvSwitches current_switches() { return {g_override, g_wave_local, g_fast, phase_stamping()}; }

bool gemv_site(hipStream_t st, GemvSite& site) {
    DeviceCtx* dc = device_ctx();
    if (!dc) return false;
    site = {dc->num_cu, true, st};
    return true;
}

// Common driver: plans the request (teal_gemv_plan.h), reports the description of the launch, and launches what the plan
// says — the GEMV and, for kGemvGeneralReduce, the ordered slab reduce.  Not at a launch site (teal_fused_gemv_plan): the
// plan alone.  desc / desc_bytes: the caller's host buffer (teal_gemv_out_t.desc).
int run_gemv(const GemvRequest& r, const GemvSite& site, char* desc, int desc_bytes, GemvPlan& plan) {
    const int rc = plan_gemv(r, site.num_cu, current_switches(), plan);
    if (plan.desc[0]) publish_desc(plan.desc, desc, desc_bytes, site.launch);
    if (rc != TEAL_OK || !site.launch) return rc;
    const bool bf16 = r.dtype == TEAL_BF16;
    plan.p.phase = plan.f.a.phase = phase_next_region();  // (nullptr in the product library)
    if (plan.family == kGemvLean) {
        const FastLaunch& f = plan.f;
        const hipError_t e = f.w8 ? (bf16 ? launch_fast_w8_bf16(f, site.st) : launch_fast_w8_f16(f, site.st))
                                  : (bf16 ? launch_fast_bf16(f, site.st) : launch_fast_f16(f, site.st));
        return e == hipSuccess ? TEAL_OK : TEAL_ERR_LAUNCH;
    }
    // one translation unit per (weight width, dtype): see teal_common.h
    const Params& p = plan.p;
    const hipError_t e = p.w8 ? (bf16 ? launch_gemv_w8_bf16(p, plan.lds, plan.c.lpr, plan.krt, site.st)
                                      : launch_gemv_w8_f16(p, plan.lds, plan.c.lpr, plan.krt, site.st))
                              : (bf16 ? launch_gemv_w16_bf16(p, plan.lds, plan.c.lpr, plan.krt, site.st)
                                      : launch_gemv_w16_f16(p, plan.lds, plan.c.lpr, plan.krt, site.st));
    if (e != hipSuccess) return TEAL_ERR_LAUNCH;
    if (plan.family == kGemvGeneralReduce) {
        const dim3 grid((p.ws_ld + 255) / 256), block(256);
        if (bf16)
            hipLaunchKernelGGL((splitk_reduce_kernel<true>), grid, block, 0, site.st, p);
        else
            hipLaunchKernelGGL((splitk_reduce_kernel<false>), grid, block, 0, site.st, p);
        if (hipGetLastError() != hipSuccess) return TEAL_ERR_LAUNCH;
    }
    return TEAL_OK;
}

int check_common(const void* x, const void* w, const void* y, int Z, int N, int dtype) {
    if (!x || !w || !y || Z <= 0 || N <= 0) return TEAL_ERR_ARG;
    if (dtype != TEAL_F16 && dtype != TEAL_BF16) return TEAL_ERR_DTYPE;
    if ((N & 7) != 0 || Z > 65536) return TEAL_ERR_SHAPE;
    if (!aligned16(w) || (reinterpret_cast<uintptr_t>(x) & 1u) || (reinterpret_cast<uintptr_t>(y) & 1u))
        return TEAL_ERR_ALIGN;
    if (!device_ctx()) return TEAL_ERR_NO_DEVICE;
    return TEAL_OK;
}

// the legacy entry points: plain x, partials in the caller's workspace, no description buffer
int run_legacy(const Params& p, int dtype, GemvOutKind kind, void* ws, size_t ws_bytes, void* stream, GemvPlan& plan) {
    GemvSite site;
    if (!gemv_site(reinterpret_cast<hipStream_t>(stream), site)) return TEAL_ERR_NO_DEVICE;
    GemvRequest r = {};
    r.p = p;
    r.dtype = dtype;
    r.kind = kind;
    r.want_desc = kDiagnostics;
    r.mem = {ws, ws_bytes, ws_prepared(ws, ws_bytes), nullptr, 0, false};
    return run_gemv(r, site, nullptr, 0, plan);
}

}  // namespace teal

using namespace teal;

extern "C" {


int teal_version(void) { return 100; }

const char* teal_strerror(int code) {
    switch (code) {
        case TEAL_OK: return "ok";
        case TEAL_ERR_ARG: return "bad argument (null pointer or non-positive size)";
        case TEAL_ERR_DTYPE: return "unsupported dtype (0 = fp16, 1 = bf16)";
        case TEAL_ERR_SHAPE: return "unsupported shape (need N % 8 == 0, Z <= 65536, segment sizes % 8 == 0)";
        case TEAL_ERR_ALIGN: return "pointer not sufficiently aligned (weights/workspace 16 B)";
        case TEAL_ERR_WORKSPACE: return "split-K workspace missing or too small (teal_workspace_bytes)";
        case TEAL_ERR_LAUNCH: return "HIP kernel launch failed";
        case TEAL_ERR_NO_DEVICE: return "no HIP device available";
        case TEAL_ERR_CONFIG: return "invalid tuning override";
        default: return "unknown error";
    }
}

int teal_init(void) {
    DeviceCtx* c = device_ctx();
    return c ? c->num_cu : TEAL_ERR_NO_DEVICE;
}

size_t teal_workspace_bytes(int Z, int N) {
    (void)Z;
    if (N <= 0) return 0;
    // the library's header (arrival counters, sampler scratch) + kMaxSplit slabs of N columns; the fused gate|up GEMV
    // uses two segments of N columns
    return kWsHeaderBytes + (size_t)kMaxSplit * (size_t)N * 2 * sizeof(float);
}

int teal_workspace_init(void* ws, size_t ws_bytes, void* stream) {
    if (!ws || ws_bytes < kWsHeaderBytes) return TEAL_ERR_WORKSPACE;
    if (!aligned16(ws)) return TEAL_ERR_ALIGN;
    if (!device_ctx()) return TEAL_ERR_NO_DEVICE;
    if (hipMemsetAsync(ws, 0, kWsHeaderBytes, reinterpret_cast<hipStream_t>(stream)) != hipSuccess) {
        (void)hipGetLastError();
        return TEAL_ERR_LAUNCH;
    }
    std::lock_guard<std::mutex> lk(g_ws_mu);
    // entries that overlap the new range are stale by construction (their memory was freed and handed out again
    // without teal_workspace_release): drop them
    const char* lo = reinterpret_cast<const char*>(ws);
    const char* hi = lo + ws_bytes;
    for (size_t i = 0; i < g_ws_reg.size();) {
        const char* elo = reinterpret_cast<const char*>(g_ws_reg[i].ws);
        if (elo < hi && lo < elo + g_ws_reg[i].bytes) g_ws_reg.erase(g_ws_reg.begin() + i);
        else ++i;
    }
    g_ws_reg.push_back({ws, ws_bytes});
    return TEAL_OK;
}

int teal_workspace_release(void* ws) {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    for (size_t i = 0; i < g_ws_reg.size(); ++i)
        if (g_ws_reg[i].ws == ws) { g_ws_reg.erase(g_ws_reg.begin() + i); return TEAL_OK; }
    return TEAL_ERR_ARG;
}

#ifdef TEAL_DIAGNOSTICS  // exported by libteal_hip_diag.so only
int teal_set_tuning(int lanes_per_row, int waves, int split, int unroll) {
    auto in = [](int v, std::initializer_list<int> ok) {
        for (int o : ok) if (v == o) return true;
        return false;
    };
    if (!in(lanes_per_row, {0, 8, 16, 32, 64}) || !in(waves, {0, 16}) ||
        !in(unroll, {0, 4}) || split < 0 || split > kMaxSplit)
        return TEAL_ERR_CONFIG;
    g_override = {lanes_per_row, waves, split, unroll};
    return TEAL_OK;
}

const char* teal_last_launch_desc(void) { return g_last_desc; }

int teal_set_fast(int on) {
    g_fast = on ? 1 : 0;
    return TEAL_OK;
}

int teal_set_wave_local(int on) {
    g_wave_local = on ? 1 : 0;
    return TEAL_OK;
}

int teal_set_phase_buffer(void* dev_u64) {
    g_phase = reinterpret_cast<unsigned long long*>(dev_u64);
    g_phase_seq = 0;
    return TEAL_OK;
}

int teal_set_phase_stride(size_t u64_per_launch) {
    g_phase_stride = u64_per_launch;
    g_phase_seq = 0;
    return TEAL_OK;
}

int teal_probe_row_reduce(const void* in_u32, void* scatter_u32, void* shuffle_u32, int nwaves, int lanes_per_row, void* stream) {
    if (!in_u32 || !scatter_u32 || !shuffle_u32 || nwaves <= 0 || (lanes_per_row != 8 && lanes_per_row != 16)) return TEAL_ERR_ARG;
    const uint32_t* in = reinterpret_cast<const uint32_t*>(in_u32);
    uint32_t* so = reinterpret_cast<uint32_t*>(scatter_u32);
    uint32_t* sh = reinterpret_cast<uint32_t*>(shuffle_u32);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (lanes_per_row == 8) hipLaunchKernelGGL((row_reduce_probe_kernel<8>), dim3(nwaves), dim3(64), 0, st, in, so, sh);
    else hipLaunchKernelGGL((row_reduce_probe_kernel<16>), dim3(nwaves), dim3(64), 0, st, in, so, sh);
    return hipGetLastError() == hipSuccess ? TEAL_OK : TEAL_ERR_LAUNCH;
}
#endif  // TEAL_DIAGNOSTICS

int teal_get_config(int Z, int N, int nseg, int* out) {
    if (!out || Z <= 0 || N <= 0) return TEAL_ERR_ARG;
    (void)nseg;
    const Config c = default_geometry(Z, N, num_cu_or(256), current_switches());
    out[0] = c.lpr;
    out[1] = c.waves;
    out[2] = c.split;
    out[3] = c.unroll;
    out[4] = ((N + c.lpr * 8 - 1) / (c.lpr * 8)) * c.split;
    return TEAL_OK;
}

int teal_compact(const void* x, float tau, int Z, int dtype, int32_t* idx_out, int32_t* count_out,
                 void* stream) {
    if (!x || !idx_out || !count_out || Z <= 0) return TEAL_ERR_ARG;
    if (dtype != TEAL_F16 && dtype != TEAL_BF16) return TEAL_ERR_DTYPE;
    if (Z > 65536) return TEAL_ERR_SHAPE;
    const int nch = (Z + 63) >> 6;
    const size_t lds = (size_t)nch * 8 + (size_t)(nch + 2) * 4;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint16_t* xp = reinterpret_cast<const uint16_t*>(x);
    if (dtype == TEAL_BF16)
        hipLaunchKernelGGL((compact_kernel<true>), dim3(1), dim3(1024), lds, st, xp, Z, tau, idx_out, count_out);
    else
        hipLaunchKernelGGL((compact_kernel<false>), dim3(1), dim3(1024), lds, st, xp, Z, tau, idx_out, count_out);
    return hipGetLastError() == hipSuccess ? TEAL_OK : TEAL_ERR_LAUNCH;
}

int teal_sparse_qkv_gemv(const void* x, const void* wT, void* y, float tau_q, float tau_k,
                         float tau_v, int Z, int N, int N_q, int N_kv, int dtype, void* ws,
                         size_t ws_bytes, void* stream) {
    return teal_sparse_qkv_gemv_ld(x, wT, N, y, tau_q, tau_k, tau_v, Z, N, N_q, N_kv, dtype, ws, ws_bytes, stream);
}

int teal_sparse_qkv_gemv_ld(const void* x, const void* wT, int ld, void* y, float tau_q, float tau_k,
                            float tau_v, int Z, int N, int N_q, int N_kv, int dtype, void* ws,
                            size_t ws_bytes, void* stream) {
    int rc = check_common(x, wT, y, Z, N, dtype);
    if (rc != TEAL_OK) return rc;
    if (ld < N || (ld & 7)) return TEAL_ERR_SHAPE;
    if (N_q < 0 || N_kv < 0 || N_q + N_kv > N || (N_q & 7) || (N_kv & 7)) return TEAL_ERR_SHAPE;
    Params p = {};
    p.x = x;
    p.Z = Z;
    const int widths[3] = {N_q, N_kv, N - N_q - N_kv};
    const float taus[3] = {tau_q, tau_k, tau_v};
    int col = 0, ns = 0;
    for (int i = 0; i < 3; ++i) {
        if (widths[i] > 0) {
            Seg& sgm = p.seg[ns++];
            sgm.w = wT;
            sgm.y = reinterpret_cast<uint16_t*>(y) + col;
            sgm.tau = taus[i];
            sgm.ld = ld;
            sgm.col0 = col;
            sgm.ncols = widths[i];
        }
        col += widths[i];
    }
    p.nseg = ns;
    GemvPlan plan;
    return run_legacy(p, dtype, kOutRounded, ws, ws_bytes, stream, plan);
}

int teal_sparse_gemv(const void* x, const void* wT, void* y, float tau, int Z, int N, int dtype,
                     void* ws, size_t ws_bytes, void* stream) {
    return teal_sparse_qkv_gemv(x, wT, y, tau, tau, tau, Z, N, N, 0, dtype, ws, ws_bytes, stream);
}

int teal_sparse_qkv_gemv_i8(const void* x, const void* wqT, const void* scale, void* y, float tau_q, float tau_k,
                            float tau_v, int Z, int N, int N_q, int N_kv, int ld, int dtype, void* ws, size_t ws_bytes,
                            void* stream) {
    if (!scale || N_q <= 0 || N_kv < 0 || N_q + 2 * N_kv != N || ld < N) return TEAL_ERR_ARG;
    if ((N_q & 7) || (N_kv & 7) || (ld & 7)) return TEAL_ERR_SHAPE;
    int rc = check_common(x, wqT, y, Z, N, dtype);
    if (rc != TEAL_OK) return rc;
    teal_gemv_in_t in = {};
    in.mode = TEAL_IN_PLAIN;
    in.x = x;
    teal_gemv_out_t out = {};
    out.mode = TEAL_OUT_ROUNDED;
    out.weight_bits = 8;
    const float taus[3] = {tau_q, tau_k, tau_v};
    const int col0[3] = {0, N_q, N_q + N_kv}, ncols[3] = {N_q, N_kv, N_kv};
    out.nseg = N_kv > 0 ? 3 : 1;
    for (int i = 0; i < out.nseg; ++i) {
        out.w[i] = wqT;
        out.ld[i] = ld;
        out.col0[i] = col0[i];
        out.ncols[i] = ncols[i];
        out.tau[i] = taus[i];
        out.y[i] = reinterpret_cast<uint16_t*>(y) + col0[i];
        out.scale[i] = reinterpret_cast<const uint16_t*>(scale) + col0[i];
    }
    return teal_fused_gemv(&in, &out, Z, dtype, ws, ws_bytes, nullptr, stream);
}

int teal_dense_gemv(const void* x, const void* wT, void* y, int Z, int N, int dtype, void* ws,
                    size_t ws_bytes, void* stream) {
    // |x| > -inf keeps every finite and infinite activation; NaN propagates via nan_keeps.
    return teal_sparse_gemv(x, wT, y, -INFINITY, Z, N, dtype, ws, ws_bytes, stream);
}

int teal_sparse_gateup_silu(const void* x, const void* w1T, const void* w3T, void* h, float tau_gate,
                            float tau_up, int Z, int N, int dtype, void* ws, size_t ws_bytes,
                            void* stream) {
    int rc = check_common(x, w1T, h, Z, N, dtype);
    if (rc != TEAL_OK) return rc;
    if (!w3T) return TEAL_ERR_ARG;
    if (!aligned16(w3T)) return TEAL_ERR_ALIGN;
    Params p = {};
    p.x = x;
    p.Z = Z;
    p.nseg = 2;
    p.seg[0].w = w1T; p.seg[0].y = nullptr; p.seg[0].tau = tau_gate; p.seg[0].ld = N; p.seg[0].col0 = 0; p.seg[0].ncols = N;
    p.seg[1].w = w3T; p.seg[1].y = nullptr; p.seg[1].tau = tau_up;   p.seg[1].ld = N; p.seg[1].col0 = 0; p.seg[1].ncols = N;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    GemvPlan plan;
    rc = run_legacy(p, dtype, kOutSlabsEpilogue, ws, ws_bytes, stream, plan);
    if (rc != TEAL_OK) return rc;
    const dim3 grid((N + 255) / 256), block(256);
    if (dtype == TEAL_BF16)
        hipLaunchKernelGGL((gateup_silu_epilogue_kernel<true>), grid, block, 0, st, plan.p, h);
    else
        hipLaunchKernelGGL((gateup_silu_epilogue_kernel<false>), grid, block, 0, st, plan.p, h);
    return hipGetLastError() == hipSuccess ? TEAL_OK : TEAL_ERR_LAUNCH;
}

// teal_fused_gemv and teal_fused_gemv_plan: one body.  `query`: nothing is launched, no device and no registry is asked — the
// request is planned for query->num_cu CUs, the caller's workspace as `mem` describes it, out->slabs plain memory.
static int fused_gemv(const teal_gemv_in_t* in, const teal_gemv_out_t* out, int Z, int dtype, GemvMemory mem, int* nslabs_out,
                      hipStream_t st, const GemvSite* query) {
    if (!in || !out || Z <= 0 || out->nseg < 1 || out->nseg > kMaxSeg) return TEAL_ERR_ARG;
    if (dtype != TEAL_F16 && dtype != TEAL_BF16) return TEAL_ERR_DTYPE;
    if (Z > 65536) return TEAL_ERR_SHAPE;
    GemvSite site;
    if (query) site = *query;
    else if (!gemv_site(st, site)) return TEAL_ERR_NO_DEVICE;
    const bool to_slabs = out->mode == TEAL_OUT_SLABS || out->mode == TEAL_OUT_SLAB_SUM || out->mode == TEAL_OUT_QKV_ROPE;
    if (!query) mem.ws_prepared = ws_prepared(mem.ws, mem.ws_bytes);
    mem.slabs = out->slabs;
    mem.slabs_bytes = out->slabs_bytes;
    mem.slabs_prepared = !query && to_slabs && ws_prepared(out->slabs, out->slabs_bytes);
    if (out->act_seg0 && out->mode != TEAL_OUT_ROUNDED) return TEAL_ERR_ARG;
    if (out->weight_bits == 4) {
        if (out->act_seg0 || in->gate_activated || out->mode == TEAL_OUT_QKV_ROPE || out->mode == TEAL_OUT_SLAB_SUM) return TEAL_ERR_ARG;  // 16-bit / int8 launches only
        return fused_gemv_i4(in, out, Z, dtype, mem, nslabs_out, site);
    }
    int rc = check_producer(in, Z, kProducer16or8);
    if (rc != TEAL_OK) return rc;
    GemvRequest r = {};
    Params& p = r.p;
    p.Z = Z;
    p.in.mode = in->mode;
    p.x = in->mode == TEAL_IN_RESID_NORM ? in->resid_in : in->x;
    switch (in->mode) {
        case TEAL_IN_SILU_MUL:
            p.in.gate_act = in->gate_activated ? 1 : 0;
            break;
        case TEAL_IN_ATTN_MERGE:
            p.in.att = reinterpret_cast<const float*>(in->x);
            p.in.att_hd = in->att_head_dim;
            p.in.att_ns = in->att_nsplit ? in->att_nsplit : 4;
            break;
        case TEAL_IN_MASKED:
            p.in.masks = reinterpret_cast<const unsigned long long*>(in->masks);
            break;
        case TEAL_IN_RESID_NORM:
            p.in.resid_in = in->resid_in;
            p.in.row_index = in->row_index;
            p.in.slabs = in->slabs;
            p.in.nslabs = in->nslabs;
            p.in.slabs_il = in->slabs_interleaved ? 1 : 0;
            p.in.norm_w = in->norm_weight;
            p.in.resid_out = in->resid_out;
            p.in.eps = in->eps;
            break;
        default: break;
    }
    p.nseg = out->nseg;
    for (int i = 0; i < out->nseg; ++i) {
        if (!out->w[i] || out->ncols[i] <= 0 || (out->ncols[i] & 7) || (out->col0[i] & 7) || (out->ld[i] & 7)) return TEAL_ERR_SHAPE;
        if (!aligned16(out->w[i])) return TEAL_ERR_ALIGN;
        if (out->mode == TEAL_OUT_ROUNDED && !out->y[i]) return TEAL_ERR_ARG;
        p.seg[i].w = out->w[i];
        p.seg[i].y = out->y[i];
        p.seg[i].tau = out->tau[i];
        p.seg[i].ld = out->ld[i];
        p.seg[i].col0 = out->col0[i];
        p.seg[i].ncols = out->ncols[i];
        p.seg[i].scale = out->scale[i];
    }
    if (out->weight_bits != 0 && out->weight_bits != 16 && out->weight_bits != 8) return TEAL_ERR_ARG;
    p.w8 = out->weight_bits == 8 ? 1 : 0;
    r.dtype = dtype;
    r.mem = mem;
    r.want_desc = out->desc || kDiagnostics;
    r.interleave = out->slabs_interleaved != 0;
    switch (out->mode) {
        case TEAL_OUT_PAIR_SILU:
            // seg 0 = gate (w1), seg 1 = up (w3), same shape; y[0] receives h = silu(gate) * up
            if (out->nseg != 2 || in->mode != TEAL_IN_RESID_NORM || out->ncols[0] != out->ncols[1] || !out->y[0]) return TEAL_ERR_ARG;
            r.kind = kOutPair;
            p.mask_out = reinterpret_cast<unsigned long long*>(out->mask_out);
            p.mask_tau = out->mask_tau;
            break;
        case TEAL_OUT_SLABS:
            r.kind = kOutSlabs;
            break;
        case TEAL_OUT_SLAB_SUM:
            // one fp32 vector [ncols]: the row slices' partial sums folded in slice order by the last slice of each tile to arrive
            // (arrival tickets in the caller's prepared workspace), NOT rounded — what tensor-parallel ranks all-reduce
            if (out->nseg != 1 || !out->slabs || out->slabs_bytes < (size_t)out->ncols[0] * sizeof(float)) return TEAL_ERR_ARG;
            if (mem.slabs_prepared) return TEAL_ERR_ARG;
            r.kind = kOutSlabSum;
            p.seg[0].y = out->slabs;
            break;
        case TEAL_OUT_ROUNDED:
            r.kind = kOutRounded;
            p.act0 = out->act_seg0 ? 1 : 0;
            break;
        case TEAL_OUT_QKV_ROPE:
            if (out->nseg != 3 || in->mode != TEAL_IN_RESID_NORM || !out->y[0] || !out->rope || !out->rope_pos || !out->k_cache ||
                !out->v_cache || out->rope_max_seq <= 0 || !nslabs_out)
                return TEAL_ERR_ARG;
            r.kind = kOutRope;
            p.rope = reinterpret_cast<const uint16_t*>(out->rope);
            p.rope_pos = out->rope_pos;
            p.kc = reinterpret_cast<uint16_t*>(out->k_cache);
            p.vc = reinterpret_cast<uint16_t*>(out->v_cache);
            p.rope_hd = out->rope_head_dim;
            p.rope_max_seq = out->rope_max_seq;
            break;
        default: return TEAL_ERR_ARG;
    }
    GemvPlan plan;
    rc = run_gemv(r, site, out->desc, out->desc_bytes, plan);
    if (rc == TEAL_OK && nslabs_out) *nslabs_out = plan.nslabs;
    return rc;
}

int teal_fused_gemv(const teal_gemv_in_t* in, const teal_gemv_out_t* out, int Z, int dtype, void* ws,
                    size_t ws_bytes, int* nslabs_out, void* stream) {
    return fused_gemv(in, out, Z, dtype, {ws, ws_bytes, false, nullptr, 0, false}, nslabs_out, reinterpret_cast<hipStream_t>(stream), nullptr);
}

int teal_fused_gemv_plan(const teal_gemv_in_t* in, const teal_gemv_out_t* out, int Z, int dtype, int ws_prepared,
                         size_t ws_bytes, int num_cu, int* nslabs_out) {
    if (num_cu <= 0) return TEAL_ERR_ARG;
    // the caller's workspace stands for itself: a made-up non-null, 16-byte aligned address (only those two facts matter)
    void* ws = ws_bytes ? reinterpret_cast<void*>(uintptr_t(1) << 32) : nullptr;
    const GemvSite query = {num_cu, false, nullptr};
    return fused_gemv(in, out, Z, dtype, {ws, ws_bytes, ws_prepared != 0 && ws_bytes >= kWsHeaderBytes, nullptr, 0, false}, nslabs_out,
                      nullptr, &query);
}


}  // extern "C"
