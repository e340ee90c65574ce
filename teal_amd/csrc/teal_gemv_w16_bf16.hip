// teal_gemv_w16_bf16.hip — sparse_gemv_kernel instantiations: 16-bit weights, bf16 activations.
#include "teal_gemv_kernel.h"

namespace teal {
hipError_t launch_gemv_w16_bf16(const Params& p, size_t lds, int lpr, int krt, hipStream_t st) {
    return launch_gemv_q<true, false>(p, lds, lpr, krt, st);
}
}  // namespace teal
