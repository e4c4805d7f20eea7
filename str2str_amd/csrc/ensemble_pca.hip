// Essential dynamics of an ensemble on the device: the mean structure and the 3L x 3L covariance of the superposed CA coordinates, and the
// projection of structures onto given components (what `gmx covar` / `gmx anaeig` compute).  The reference repository has no such function;
// the yardstick is the float64 numpy restatement in tests/ref_pca.py.
//
//   s2s_ca_aligned_mean   m = sum_s p_s y_s,  y_s = R_s x_s + t_s in float64 (the float32 coordinates widened; never rounded back).
//   s2s_ca_covariance     C = sum_s p_s (y_s - m)(y_s - m)^T, two-pass.  A prepass writes sqrt(p_s) (y_s - m) in blocks of 48 coordinates x
//                         structures; every 48 x 48 block of C on or above the diagonal is one wave on the tile set and operands
//                         of sym48_f64.h, the k loop running over the structures in ascending order: C is exactly
//                         symmetric.  The structures pass through the workspace in chunks of a multiple of 4 (one MFMA's k); the
//                         accumulators of a later chunk start from the running C, so the chain of MFMAs of an entry -- and with it every
//                         bit of C -- is the same for any chunk size.
//   s2s_ca_project        proj[s, k] = sum_c (y_sc - m_c) v_kc, one wave per structure.
//
// Everything is float64; contraction stays on (an fma only removes a rounding).
#include <hip/hip_runtime.h>
#include <math.h>

#include "str2str_hip.h"
#include "sym48_f64.h"

namespace {

using sym48::MEAN_GROUPS;

// Coordinate c = 3 i + a of structure s after its transform (xform NULL: the identity, the widened float32 value itself).
__device__ __forceinline__ double aligned_coord(const float* __restrict__ x, const double* __restrict__ xform, long long s, int n3, int c) {
    const float* p = x + s * n3;
    if (!xform) return (double)p[c];
    const int i3 = c - c % 3, a = c % 3;
    const double* t = xform + s * 12;
    return t[3 * a] * (double)p[i3] + t[3 * a + 1] * (double)p[i3 + 1] + t[3 * a + 2] * (double)p[i3 + 2] + t[9 + a];
}

// sym48::grouped_column_sum over the structures, the term of structure s being p_s y_s: the order is a function of their number alone.
__global__ void __launch_bounds__(64 * MEAN_GROUPS) aligned_mean_kernel(const float* __restrict__ x, int n, int n3,
                                                                        const double* __restrict__ xform, const double* __restrict__ p,
                                                                        double* __restrict__ mean) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const double uniform = 1.0 / (double)n;
    double m;
    if (sym48::grouped_column_sum(n, c < n3, [=](long long s) { return (p ? p[s] : uniform) * aligned_coord(x, xform, s, n3, c); }, m)) mean[c] = m;
}

// Prepass of one chunk (structures s0 .. s0 + n_chunk - 1 of n; Sp = n_chunk rounded up to 4): out[(blk * Sp + k) * 48 + r] =
// sqrt(p_s) (y_s[48 blk + r] - mean[48 blk + r]), zero for a coordinate >= n3 and for a padding structure k >= n_chunk (sym48_f64.h's layout).
__global__ void __launch_bounds__(256) cov_prep_kernel(const float* __restrict__ x, int n, int n3, int nblk, const double* __restrict__ xform,
                                                       const double* __restrict__ p, const double* __restrict__ mean, int s0, int n_chunk, int Sp,
                                                       double* __restrict__ out) {
    const int k = blockIdx.x, cp = blockIdx.y * 256 + threadIdx.x;   // cp: the padded coordinate, 0 .. 48 nblk - 1
    if (cp >= nblk * 48 || k >= Sp) return;
    double v = 0.0;
    if (k < n_chunk && cp < n3) {
        const long long s = (long long)s0 + k;
        const double ps = p ? p[s] : 1.0 / (double)n;
        v = sqrt(ps) * (aligned_coord(x, xform, s, n3, cp) - mean[cp]);
    }
    out[((size_t)(cp / 48) * Sp + k) * 48 + cp % 48] = v;
}

// One wave per 48 x 48 block (bi = blockIdx.y, bj = blockIdx.x) of C with bi <= bj, on the tiles and operands of sym48_f64.h, one operand
// set per k-step: three waves per SIMD, so the 2080 blocks of the cap are resident at once.  The running-value load and the mirrored store
// are its own loops (measured faster than the header's helpers: DESIGN.md).  first: start from zero, otherwise from the running C.
__global__ void __launch_bounds__(64) cov_product_kernel(const double* __restrict__ buf, int Sp, int n3, int first, double* __restrict__ cov) {
    const int bi = blockIdx.y, bj = blockIdx.x, lane = threadIdx.x;
    if (bi > bj) return;
    const int q = lane >> 4, col = lane & 15;
    const double* pa = buf + (size_t)bi * Sp * 48 + q * 48 + col;
    const double* pb = buf + (size_t)bj * Sp * 48 + q * 48 + col;
    sym48::Block acc;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            acc[i][j] = sym48::d4{0.0, 0.0, 0.0, 0.0};
            if (!first) {
                const int gc = bj * 48 + 16 * j + col;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int gr = bi * 48 + 16 * i + q + 4 * r;
                    if (gr < n3 && gc < n3) acc[i][j][r] = cov[(size_t)gr * n3 + gc];
                }
            }
        }
    for (int k0 = 0; k0 < Sp; k0 += 4) {
        sym48::Operands<1> x;
        x.load(pa, pb);
        pa += 192; pb += 192;
        x.accumulate(acc);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int gc = bj * 48 + 16 * j + col;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gr = bi * 48 + 16 * i + q + 4 * r;
                if (gr >= n3 || gc >= n3 || gr > gc) continue;   // (gr > gc only inside a diagonal block: that entry comes from its mirror)
                cov[(size_t)gr * n3 + gc] = acc[i][j][r];
                if (gr < gc) cov[(size_t)gc * n3 + gr] = acc[i][j][r];
            }
        }
}

// One wave per structure: z = y - mean goes to LDS once, then sym48::project_row: the order is a function of the chain length alone.
__global__ void __launch_bounds__(64) project_kernel(const float* __restrict__ x, int n3, const double* __restrict__ xform,
                                                     const double* __restrict__ mean, const double* __restrict__ comp, int K,
                                                     double* __restrict__ proj) {
    extern __shared__ double z[];
    const int lane = threadIdx.x;
    const long long s = blockIdx.x;
    for (int c = lane; c < n3; c += 64) z[c] = aligned_coord(x, xform, s, n3, c) - mean[c];
    __syncthreads();
    sym48::project_row(n3, [&](int c) { return z[c]; }, comp, K, proj + s * K);
}

}  // namespace

extern "C" int s2s_ca_aligned_mean(const float* x, int n, int n_res, const double* xform, const double* p, double* mean, void* stream) {
    if (!x || !mean || n < 1 || n_res < 1 || n_res > S2S_PCA_MAX_RES) return (int)hipErrorInvalidValue;
    const int n3 = 3 * n_res;
    hipLaunchKernelGGL(aligned_mean_kernel, dim3((unsigned)((n3 + 63) / 64)), dim3(64 * MEAN_GROUPS), 0, (hipStream_t)stream, x, n, n3, xform, p,
                       mean);
    return (int)hipGetLastError();
}

extern "C" int s2s_ca_covariance(const float* x, int n, int n_res, const double* xform, const double* p, const double* mean, double* cov,
                                 double* workspace, long long workspace_doubles, void* stream) {
    if (!x || !mean || !cov || !workspace || n < 1 || n_res < 1 || n_res > S2S_PCA_MAX_RES) return (int)hipErrorInvalidValue;
    const int n3 = 3 * n_res, nblk = (n3 + 47) / 48;
    const long long n4 = ((long long)n + 3) / 4 * 4;
    long long chunk = workspace_doubles / (48ll * nblk) / 4 * 4;   // structures per chunk: a multiple of 4 that the workspace holds
    if (chunk < 4) return (int)hipErrorInvalidValue;
    if (chunk > n4) chunk = n4;
    hipStream_t st = (hipStream_t)stream;
    for (long long s0 = 0; s0 < n; s0 += chunk) {
        const int n_chunk = (int)(n - s0 < chunk ? n - s0 : chunk), Sp = (n_chunk + 3) / 4 * 4;
        hipLaunchKernelGGL(cov_prep_kernel, dim3((unsigned)Sp, (unsigned)((nblk * 48 + 255) / 256)), dim3(256), 0, st, x, n, n3, nblk, xform, p, mean,
                           (int)s0, n_chunk, Sp, workspace);
        hipLaunchKernelGGL(cov_product_kernel, dim3((unsigned)nblk, (unsigned)nblk), dim3(64), 0, st, workspace, Sp, n3, s0 == 0 ? 1 : 0, cov);
    }
    return (int)hipGetLastError();
}

extern "C" int s2s_ca_project(const float* x, int n, int n_res, const double* xform, const double* mean, const double* components,
                              int n_components, double* proj, void* stream) {
    if (!x || !mean || !components || !proj || n < 1 || n_res < 1 || n_res > S2S_PCA_MAX_RES || n_components < 1)
        return (int)hipErrorInvalidValue;
    const int n3 = 3 * n_res;
    hipLaunchKernelGGL(project_kernel, dim3((unsigned)n), dim3(64), (size_t)n3 * sizeof(double), (hipStream_t)stream, x, n3, xform, mean, components,
                       n_components, proj);
    return (int)hipGetLastError();
}
