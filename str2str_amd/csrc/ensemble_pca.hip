// Essential dynamics of an ensemble on the device: the mean structure and the 3L x 3L covariance of the superposed CA coordinates, and the
// projection of structures onto given components (what `gmx covar` / `gmx anaeig` compute).  The reference repository has no such function;
// the yardstick is the float64 numpy restatement in tests/ref_pca.py.
//
//   s2s_ca_aligned_mean   m = sum_s p_s y_s,  y_s = R_s x_s + t_s in float64 (the float32 coordinates widened; never rounded back).
//   s2s_ca_covariance     C = sum_s p_s (y_s - m)(y_s - m)^T, two-pass.  A prepass writes sqrt(p_s) (y_s - m) in blocks of 48 coordinates x
//                         structures; every 48 x 48 block of C on or above the diagonal is one [48, R] x [R, 48] float64 matrix product
//                         on v_mfma_f64_16x16x4_f64 (nine accumulator tiles per wave, the idiom of ensemble_rmsd.hip), the k loop running
//                         over the structures in ascending order.  The SAME scaled coordinates serve as either operand, products commute
//                         and the sums run in one order; the lower triangle is written from its mirror, so C is exactly symmetric.
//                         The structures pass through the workspace in chunks of a multiple of 4 (one MFMA's k); the accumulators of a
//                         later chunk start from the running C, so the chain of MFMAs of an entry -- and with it every bit of C -- is the
//                         same for any chunk size.
//   s2s_ca_project        proj[s, k] = sum_c (y_sc - m_c) v_kc, one wave per structure.
//
// Everything is float64; contraction stays on (an fma only removes a rounding).
#include <hip/hip_runtime.h>
#include <math.h>

#include "ensemble_common.h"
#include "str2str_hip.h"

namespace {

using ensemble::wave_sum;

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int MEAN_GROUPS = 16;   // structure groups of a workgroup of the mean kernel (64 coordinates x 16 groups = 1024 threads)

// Coordinate c = 3 i + a of structure s after its transform (xform NULL: the identity, the widened float32 value itself).
__device__ __forceinline__ double aligned_coord(const float* __restrict__ x, const double* __restrict__ xform, long long s, int n3, int c) {
    const float* p = x + s * n3;
    if (!xform) return (double)p[c];
    const int i3 = c - c % 3, a = c % 3;
    const double* t = xform + s * 12;
    return t[3 * a] * (double)p[i3] + t[3 * a + 1] * (double)p[i3 + 1] + t[3 * a + 2] * (double)p[i3 + 2] + t[9 + a];
}

// Thread (group g, coordinate c) adds the structures g, g + 16, ... in ascending order; the 16 partial sums of a coordinate are then added in
// ascending g: the order is a function of the number of structures alone.
__global__ void __launch_bounds__(64 * MEAN_GROUPS) aligned_mean_kernel(const float* __restrict__ x, int n, int n3,
                                                                        const double* __restrict__ xform, const double* __restrict__ p,
                                                                        double* __restrict__ mean) {
    __shared__ double part[MEAN_GROUPS][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const double uniform = 1.0 / (double)n;
    double acc = 0.0;
    if (c < n3)
        for (int s = g; s < n; s += MEAN_GROUPS) acc += (p ? p[s] : uniform) * aligned_coord(x, xform, s, n3, c);
    part[g][lane] = acc;
    __syncthreads();
    if (g == 0 && c < n3) {
        double m = part[0][lane];
        for (int k = 1; k < MEAN_GROUPS; ++k) m += part[k][lane];
        mean[c] = m;
    }
}

// Prepass of one chunk (structures s0 .. s0 + n_chunk - 1 of n; Sp = n_chunk rounded up to 4): out[(blk * Sp + k) * 48 + r] =
// sqrt(p_s) (y_s[48 blk + r] - mean[48 blk + r]), zero for a coordinate >= n3 and for a padding structure k >= n_chunk.
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

// One wave per 48 x 48 block (bi = blockIdx.y, bj = blockIdx.x) of C with bi <= bj.  MFMA operands (lane maps of the f64 16x16x4 form): lane l
// feeds A[row = l & 15][k = l >> 4] and B[k = l >> 4][col = l & 15], and receives D[row = (l >> 4) + 4 r][col = l & 15] in register r.
// first: the accumulators start from zero, otherwise from the running C.  Entries with row <= col are stored and copied to their mirror.
__global__ void __launch_bounds__(64) cov_product_kernel(const double* __restrict__ buf, int Sp, int n3, int first, double* __restrict__ cov) {
    const int bi = blockIdx.y, bj = blockIdx.x, lane = threadIdx.x;
    if (bi > bj) return;
    const int q = lane >> 4, col = lane & 15;
    const double* pa = buf + (size_t)bi * Sp * 48 + q * 48 + col;
    const double* pb = buf + (size_t)bj * Sp * 48 + q * 48 + col;
    d4 acc[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
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
        double av[3], bv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { av[c] = pa[16 * c]; bv[c] = pb[16 * c]; }
        pa += 192; pb += 192;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bv[j], acc[i][j], 0, 0, 0);
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

// One wave per structure: z = y - mean goes to LDS once, then lane l adds the coordinates l, l + 64, ... of every component in ascending
// order and the lanes meet in the xor tree: the order is a function of the chain length alone.
__global__ void __launch_bounds__(64) project_kernel(const float* __restrict__ x, int n3, const double* __restrict__ xform,
                                                     const double* __restrict__ mean, const double* __restrict__ comp, int K,
                                                     double* __restrict__ proj) {
    extern __shared__ double z[];
    const int lane = threadIdx.x;
    const long long s = blockIdx.x;
    for (int c = lane; c < n3; c += 64) z[c] = aligned_coord(x, xform, s, n3, c) - mean[c];
    __syncthreads();
    for (int k = 0; k < K; ++k) {
        const double* v = comp + (size_t)k * n3;
        double acc = 0.0;
        for (int c = lane; c < n3; c += 64) acc += z[c] * v[c];
        acc = wave_sum(acc);
        if (lane == 0) proj[s * K + k] = acc;
    }
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
