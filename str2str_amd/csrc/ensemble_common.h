// The pieces the ensemble_*.hip units share: the wave reduction, the recognition of a row chunk of a self matrix, and the launch of a
// kernel whose dynamic LDS may exceed the default limit.
#pragma once

#include <hip/hip_runtime.h>

namespace ensemble {

// Sum over the 64 lanes of a wave (xor tree o = 32 .. 1: every lane ends with the same value, summed in the same order).
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// a [n_a, n_res, 3] inside b's [n_b, n_res, 3] storage on a structure boundary = a row chunk of the self matrix: the row of b at which a
// starts, otherwise -1.  A kernel given row0 >= 0 evaluates a pair below the diagonal as its mirror pair, which is what makes a chunked
// self matrix exactly symmetric.
inline long long self_row0(const float* a, const float* b, int n_a, int n_b, int n_res) {
    const long long stride = 3ll * n_res;
    if (a >= b && a - b < stride * n_b && (a - b) % stride == 0 && (a - b) / stride + n_a <= n_b) return (a - b) / stride;
    return -1;
}

// Launch with `lds` bytes of dynamic LDS, raising the kernel's limit first where that is above the default 64 KiB.
template <typename... Params, typename... Args>
inline int launch_dynamic_lds(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    if (lds > 64 * 1024) {
        const hipError_t rc = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (rc != hipSuccess) return (int)rc;
    }
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
    return (int)hipGetLastError();
}

}  // namespace ensemble
