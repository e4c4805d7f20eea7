// Time-lagged covariances of a feature trajectory on the device: the reversible mean, the instantaneous and the time-lagged covariance
// over the T - lag frame pairs (t, t + lag), and the projection of feature rows onto given components -- the heavy half of TICA
// (deeptime's Covariance(lagtime, reversible=True, remove_data_mean=True, bessels_correction=False); oracle/tica.py restates it).
// include/str2str_hip.h has the definition; the yardstick is the float64 restatement in tests/ref_tica.py.
//
//   s2s_lagged_mean         m = (1 / 2n) sum_{t<n} (f_t + f_{t+lag}), n = T - lag, in float64 on the widened float32 features.
//   s2s_lagged_covariances  with z_t = (f_t - m) / sqrt(2n):  C00 = sum_t (z_t z_t^T + z_{t+lag} z_{t+lag}^T),
//                           C0t = sum_t (z_t z_{t+lag}^T + z_{t+lag} z_t^T).  A prepass writes the two operand streams z_t and z_{t+lag},
//                           indexed by PAIR (no halo), in blocks of 48 features x 4-padded pairs; one wave owns a 48 x 48 block on or above
//                           the diagonal and forms BOTH matrices from the same four operand loads per k-step: 18 accumulator tiles, 36
//                           v_mfma_f64_16x16x4_f64 per 12 loaded doubles per lane.  Entries with row <= column are stored and copied to
//                           their mirror: both matrices are exactly symmetric.  When the triangle has fewer blocks than the device has
//                           wave slots the pairs are divided into G contiguous groups (G a function of (n, D) alone), each with partial
//                           matrices of its own in the workspace; a last kernel adds them in ascending group order.  The pairs pass
//                           through the workspace in chunks of a multiple of 4 per group; a later chunk's accumulators start from the
//                           running values, so the chain of MFMAs of an entry -- every bit -- is the same for any workspace size.
//   s2s_feature_project     proj[s, k] = sum_c (f_sc - m_c) v_kc, one wave per row, f read directly (no staging: D is not bounded by LDS).
//
// Everything is float64, no float atomics; contraction stays on (an fma only removes a rounding).
#include <hip/hip_runtime.h>
#include <math.h>

#include "ensemble_common.h"
#include "str2str_hip.h"

namespace {

using ensemble::wave_sum;

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int MEAN_GROUPS = 16;    // pair groups of a workgroup of the mean kernel (64 features x 16 groups = 1024 threads)
constexpr int TILE_DOUBLES = 256;  // one 16 x 16 accumulator tile in the lane layout: register r of lane l at r * 64 + l
constexpr int BLOCK_DOUBLES = 9 * TILE_DOUBLES;   // S2S_TICA_PARTIAL_BLOCK_DOUBLES

// How the pairs are divided (the rule of include/str2str_hip.h, S2S_TICA_GROUPS): a function of (n, D) alone.
struct Split {
    int nblk;            // blocks of 48 features
    long long ntri;      // blocks on or above the diagonal
    long long n4;        // the pairs rounded up to 4
    long long group;     // pairs per group, a multiple of 4
    int groups;          // G
};

inline Split split_of(int T, int D, int lag) {
    Split s;
    s.nblk = (int)S2S_TICA_BLOCKS(D);
    s.ntri = S2S_TICA_TRIANGLE(D);
    s.n4 = S2S_TICA_PAIRS4(T, lag);
    s.group = S2S_TICA_GROUP_PAIRS(D, T, lag);
    s.groups = (int)S2S_TICA_GROUPS(D, T, lag);
    return s;
}

// Thread (group g, feature c) adds the pairs g, g + 16, ... in ascending order, each as f_t + f_{t+lag}; the 16 partial sums of a feature
// are then added in ascending g and divided by 2n: the order is a function of (T, lag) alone.
__global__ void __launch_bounds__(64 * MEAN_GROUPS) lagged_mean_kernel(const float* __restrict__ f, int n, int D, int lag,
                                                                       double* __restrict__ mean) {
    __shared__ double part[MEAN_GROUPS][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    double acc = 0.0;
    if (c < D)
        for (long long t = g; t < n; t += MEAN_GROUPS) acc += (double)f[t * D + c] + (double)f[(t + lag) * D + c];
    part[g][lane] = acc;
    __syncthreads();
    if (g == 0 && c < D) {
        double m = part[0][lane];
        for (int k = 1; k < MEAN_GROUPS; ++k) m += part[k][lane];
        mean[c] = m / (2.0 * (double)n);
    }
}

// Prepass of one pass (every group advanced to the pair offset `off` of its own, `step` pairs each).  Slot (g, k) holds the pair
// t = g * group + off + k; stream 0 is z_t, stream 1 is z_{t+lag}:  out[(((s * nblk + blk) * G + g) * step + k) * 48 + r] =
// (f[t + s lag][48 blk + r] - mean[48 blk + r]) / sqrt(2n), zero for a feature >= D and for a padding pair t >= n.  Slots past the end of
// their group are neither written nor read.
__global__ void __launch_bounds__(256) lagged_prep_kernel(const float* __restrict__ f, int n, int D, int lag, int nblk, int G, long long group,
                                                          long long n4, long long off, int step, const double* __restrict__ mean,
                                                          double* __restrict__ out) {
    const long long slot = blockIdx.x;                       // g * step + k
    const int cp = blockIdx.y * 256 + threadIdx.x;           // the padded feature, 0 .. 48 nblk - 1
    const int g = (int)(slot / step), k = (int)(slot % step);
    if (cp >= nblk * 48 || g >= G) return;
    const long long len4 = (n4 - g * group < group) ? n4 - g * group : group;   // the group's pairs, 4-padded
    if (off + k >= len4) return;
    const long long t = g * group + off + k;
    double z0 = 0.0, z1 = 0.0;
    if (t < n && cp < D) {
        const double m = mean[cp], s = sqrt(2.0 * (double)n);
        z0 = ((double)f[t * D + cp] - m) / s;
        z1 = ((double)f[(t + lag) * D + cp] - m) / s;
    }
    const size_t at = (((size_t)(cp / 48) * G + g) * step + k) * 48 + cp % 48, stream = (size_t)nblk * G * step * 48;
    out[at] = z0;
    out[stream + at] = z1;
}

// Block (bi, bj), bi <= bj, number `tri` of the upper triangle in row-major order.
__device__ __forceinline__ void block_of(long long tri, int nblk, int& bi, int& bj) {
    int i = 0;
    while (tri >= nblk - i) { tri -= nblk - i; ++i; }
    bi = i; bj = i + (int)tri;
}

// Entries with row <= col of an accumulated block go to C and to their mirror.  (gr > gc occurs only inside a diagonal block: that entry
// comes from its mirror.)
__device__ __forceinline__ void store_block(const d4 (&acc)[3][3], int bi, int bj, int q, int col, int D, double* __restrict__ c) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int gc = bj * 48 + 16 * j + col;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gr = bi * 48 + 16 * i + q + 4 * r;
                if (gr >= D || gc >= D || gr > gc) continue;
                c[(size_t)gr * D + gc] = acc[i][j][r];
                if (gr < gc) c[(size_t)gc * D + gr] = acc[i][j][r];
            }
        }
}

// The operands of one k-step (4 pairs) of a lane: z_t (a0) and z_{t+lag} (a1) of the row block, z_t (b0) and z_{t+lag} (b1) of the column
// block, three doubles each (the three 16-row tiles of a 48-block).
struct Operands {
    double a0[3], a1[3], b0[3], b1[3];

    __device__ __forceinline__ void load(const double* __restrict__ pa, const double* __restrict__ pb, size_t stream) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { a0[c] = pa[16 * c]; a1[c] = pa[stream + 16 * c]; b0[c] = pb[16 * c]; b1[c] = pb[stream + 16 * c]; }
    }

    __device__ __forceinline__ void accumulate(d4 (&s00)[3][3], d4 (&s0t)[3][3]) const {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                s00[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[i], b0[j], s00[i][j], 0, 0, 0);
                s00[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[i], b1[j], s00[i][j], 0, 0, 0);
                s0t[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[i], b1[j], s0t[i][j], 0, 0, 0);
                s0t[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[i], b0[j], s0t[i][j], 0, 0, 0);
            }
    }
};

// One wave per (block of the upper triangle = blockIdx.x, group = blockIdx.y).  MFMA operands (lane maps of the f64 16x16x4 form): lane l
// feeds A[row = l & 15][k = l >> 4] and B[k = l >> 4][col = l & 15], and receives D[row = (l >> 4) + 4 r][col = l & 15] in register r.
// Per k-step (4 pairs) the lane loads z_t and z_{t+lag} of block bi (a0, a1) and of block bj (b0, b1), three doubles each, and every tile
// (i, j) takes   C00 += a0_i b0_j, C00 += a1_i b1_j, C0t += a0_i b1_j, C0t += a1_i b0_j   in that order.
// first: the accumulators start from zero, otherwise from the running values -- of C itself (part == NULL: one group), or of the group's
// partial block in the lane layout, part[(((g * 2 + m) * ntri + tri) * 9 + 3 i + j) * 256 + r * 64 + lane].
__global__ void __launch_bounds__(64) lagged_product_kernel(const double* __restrict__ buf, int nblk, long long ntri, int G, long long group,
                                                            long long n4, long long off, int step, int D, int first,
                                                            double* __restrict__ c00, double* __restrict__ c0t, double* __restrict__ part) {
    const long long tri = blockIdx.x;
    const int g = blockIdx.y, lane = threadIdx.x;
    const long long len4 = (n4 - g * group < group) ? n4 - g * group : group;
    long long kn = len4 - off;
    if (kn <= 0) return;                                     // this group is already through
    if (kn > step) kn = step;
    int bi, bj;
    block_of(tri, nblk, bi, bj);
    const int q = lane >> 4, col = lane & 15;
    const size_t stream = (size_t)nblk * G * step * 48;
    const double* pa = buf + (((size_t)bi * G + g) * step + q) * 48 + col;
    const double* pb = buf + (((size_t)bj * G + g) * step + q) * 48 + col;
    double* p00 = part ? part + ((((size_t)g * 2 + 0) * ntri + tri) * BLOCK_DOUBLES) + lane : nullptr;
    double* p0t = part ? part + ((((size_t)g * 2 + 1) * ntri + tri) * BLOCK_DOUBLES) + lane : nullptr;
    d4 s00[3][3], s0t[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            s00[i][j] = d4{0.0, 0.0, 0.0, 0.0};
            s0t[i][j] = d4{0.0, 0.0, 0.0, 0.0};
            if (first) continue;
            const int gc = bj * 48 + 16 * j + col;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (part) {
                    s00[i][j][r] = p00[(3 * i + j) * TILE_DOUBLES + r * 64];
                    s0t[i][j][r] = p0t[(3 * i + j) * TILE_DOUBLES + r * 64];
                } else {
                    const int gr = bi * 48 + 16 * i + q + 4 * r;
                    if (gr < D && gc < D) {
                        s00[i][j][r] = c00[(size_t)gr * D + gc];
                        s0t[i][j][r] = c0t[(size_t)gr * D + gc];
                    }
                }
            }
        }
    // Two operand sets in turn (no register copies between steps): while one set's 36 MFMAs run, the other set's loads are in flight.  The
    // step after the last one reloads the last step's operands (an address that is valid anyway) and never uses them.
    Operands x, y;
    const long long steps = kn / 4;
    x.load(pa, pb, stream);
    for (long long s = 0; s < steps; s += 2) {
        const int hop1 = s + 1 < steps ? 192 : 0;
        y.load(pa + hop1, pb + hop1, stream);
        __builtin_amdgcn_sched_barrier(0);                     // (the loads stay ahead of the other set's MFMAs)
        x.accumulate(s00, s0t);
        if (s + 1 >= steps) break;
        const int hop2 = hop1 + (s + 2 < steps ? 192 : 0);
        x.load(pa + hop2, pb + hop2, stream);
        __builtin_amdgcn_sched_barrier(0);
        y.accumulate(s00, s0t);
        pa += hop2; pb += hop2;
    }
    if (part) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    p00[(3 * i + j) * TILE_DOUBLES + r * 64] = s00[i][j][r];
                    p0t[(3 * i + j) * TILE_DOUBLES + r * 64] = s0t[i][j][r];
                }
    } else {
        store_block(s00, bi, bj, q, col, D, c00);
        store_block(s0t, bi, bj, q, col, D, c0t);
    }
}

// One wave per (block of the upper triangle = blockIdx.x, matrix = blockIdx.y): the G partial blocks are added in ascending g, in the lane
// layout the product kernel left them in, and the sums go to C and to the mirrors.
__global__ void __launch_bounds__(64) lagged_reduce_kernel(const double* __restrict__ part, int nblk, long long ntri, int G, int D,
                                                           double* __restrict__ c00, double* __restrict__ c0t) {
    const long long tri = blockIdx.x;
    const int m = blockIdx.y, lane = threadIdx.x;
    int bi, bj;
    block_of(tri, nblk, bi, bj);
    const size_t per_group = (size_t)2 * ntri * BLOCK_DOUBLES;
    const double* p = part + ((size_t)m * ntri + tri) * BLOCK_DOUBLES + lane;
    d4 acc[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = p[(3 * i + j) * TILE_DOUBLES + r * 64];
    for (int g = 1; g < G; ++g) {
        p += per_group;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] += p[(3 * i + j) * TILE_DOUBLES + r * 64];
    }
    store_block(acc, bi, bj, lane >> 4, lane & 15, D, m ? c0t : c00);
}

// One wave per row: lane l adds the features l, l + 64, ... of every component in ascending order, read from f itself, and the lanes meet
// in the xor tree: the order is a function of D alone.
__global__ void __launch_bounds__(64) feature_project_kernel(const float* __restrict__ f, int D, const double* __restrict__ mean,
                                                             const double* __restrict__ comp, int K, double* __restrict__ proj) {
    const int lane = threadIdx.x;
    const long long s = blockIdx.x;
    const float* row = f + s * D;
    for (int k = 0; k < K; ++k) {
        const double* v = comp + (size_t)k * D;
        double acc = 0.0;
        for (int c = lane; c < D; c += 64) acc += ((double)row[c] - mean[c]) * v[c];
        acc = wave_sum(acc);
        if (lane == 0) proj[s * K + k] = acc;
    }
}

inline bool bad_shape(int T, int D, int lag) { return D < 1 || D > S2S_TICA_MAX_FEATURES || lag < 1 || T <= lag; }

}  // namespace

extern "C" int s2s_lagged_mean(const float* f, int T, int D, int lag, double* mean, void* stream) {
    if (!f || !mean || bad_shape(T, D, lag)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(lagged_mean_kernel, dim3((unsigned)((D + 63) / 64)), dim3(64 * MEAN_GROUPS), 0, (hipStream_t)stream, f, T - lag, D, lag,
                       mean);
    return (int)hipGetLastError();
}

extern "C" int s2s_lagged_covariances(const float* f, int T, int D, int lag, const double* mean, double* c00, double* c0t, double* workspace,
                                      long long workspace_doubles, void* stream) {
    if (!f || !mean || !c00 || !c0t || !workspace || bad_shape(T, D, lag)) return (int)hipErrorInvalidValue;
    const Split sp = split_of(T, D, lag);
    const int n = T - lag, G = sp.groups;
    const long long partials = G > 1 ? (long long)G * 2 * sp.ntri * BLOCK_DOUBLES : 0;
    const long long per_pair = 2ll * sp.nblk * 48 * G;                       // operand doubles of one pair slot of every group
    long long step = (workspace_doubles - partials) / per_pair / 4 * 4;      // pairs per group and pass: a multiple of 4 that the workspace holds
    if (workspace_doubles < partials || step < 4) return (int)hipErrorInvalidValue;
    if (step > sp.group) step = sp.group;
    if (step * G > 2147483644ll) step = 2147483644ll / G / 4 * 4;            // (the prepass grid's x extent)
    double* part = G > 1 ? workspace + per_pair * step : nullptr;
    hipStream_t st = (hipStream_t)stream;
    for (long long off = 0; off < sp.group; off += step) {
        hipLaunchKernelGGL(lagged_prep_kernel, dim3((unsigned)(step * G), (unsigned)((sp.nblk * 48 + 255) / 256)), dim3(256), 0, st, f, n, D, lag,
                           sp.nblk, G, sp.group, sp.n4, off, (int)step, mean, workspace);
        hipLaunchKernelGGL(lagged_product_kernel, dim3((unsigned)sp.ntri, (unsigned)G), dim3(64), 0, st, workspace, sp.nblk, sp.ntri, G, sp.group,
                           sp.n4, off, (int)step, D, off == 0 ? 1 : 0, c00, c0t, part);
    }
    if (G > 1)
        hipLaunchKernelGGL(lagged_reduce_kernel, dim3((unsigned)sp.ntri, 2u), dim3(64), 0, st, part, sp.nblk, sp.ntri, G, D, c00, c0t);
    return (int)hipGetLastError();
}

extern "C" int s2s_feature_project(const float* f, int T, int D, const double* mean, const double* components, int n_components, double* proj,
                                   void* stream) {
    if (!f || !mean || !components || !proj || T < 1 || D < 1 || D > S2S_TICA_MAX_FEATURES || n_components < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(feature_project_kernel, dim3((unsigned)T), dim3(64), 0, (hipStream_t)stream, f, D, mean, components, n_components, proj);
    return (int)hipGetLastError();
}
