// Time-lagged covariances of a feature trajectory on the device: the reversible mean, the instantaneous and the time-lagged covariance
// over the T - lag frame pairs (t, t + lag), and the projection of feature rows onto given components -- the heavy half of TICA
// (deeptime's Covariance(lagtime, reversible=True, remove_data_mean=True, bessels_correction=False); oracle/tica.py restates it).
// include/str2str_hip.h has the definition; the yardstick is the float64 restatement in tests/ref_tica.py.
//
//   s2s_lagged_mean         m = (1 / 2n) sum_{t<n} (f_t + f_{t+lag}), n = T - lag, in float64 on the widened float32 features.
//   s2s_lagged_covariances  with z_t = (f_t - m) / sqrt(2n):  C00 = sum_t (z_t z_t^T + z_{t+lag} z_{t+lag}^T),
//                           C0t = sum_t (z_t z_{t+lag}^T + z_{t+lag} z_t^T).  A prepass writes the two operand streams z_t and z_{t+lag},
//                           indexed by PAIR (no halo), in blocks of 48 features x 4-padded pairs; the symmetric block product of
//                           sym48_f64.h with two streams forms BOTH matrices, exactly symmetric, from the same four operand loads per
//                           k-step.  When the triangle has fewer blocks than the device has wave slots the pairs are divided into G
//                           contiguous groups (G a function of (n, D) alone), each with partial matrices of its own in the workspace; a
//                           last kernel adds them in ascending group order.  The pairs pass through the workspace in passes of a multiple
//                           of 4 per group: every bit is the same for any workspace size.
//   s2s_feature_project     proj[s, k] = sum_c (f_sc - m_c) v_kc, one wave per row, f read directly (no staging: D is not bounded by LDS).
//
// Everything is float64, no float atomics; contraction stays on (an fma only removes a rounding).
#include <hip/hip_runtime.h>
#include <math.h>

#include "str2str_hip.h"
#include "sym48_f64.h"

namespace {

using sym48::BLOCK_DOUBLES;   // S2S_TICA_PARTIAL_BLOCK_DOUBLES
using sym48::MEAN_GROUPS;

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

// sym48::grouped_column_sum over the pairs, the term of pair t being f_t + f_{t+lag}, divided by 2n: the order is a function of (T, lag) alone.
__global__ void __launch_bounds__(64 * MEAN_GROUPS) lagged_mean_kernel(const float* __restrict__ f, int n, int D, int lag,
                                                                       double* __restrict__ mean) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    double m;
    if (sym48::grouped_column_sum(n, c < D, [=](long long t) { return (double)f[t * D + c] + (double)f[(t + lag) * D + c]; }, m))
        mean[c] = m / (2.0 * (double)n);
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

// One wave per (block of the upper triangle = blockIdx.x, group = blockIdx.y) of one pass, on the pieces of sym48_f64.h; buf is the
// prepass's output.
// first: the accumulators start from zero, otherwise from the running values -- of c00 and c0t themselves (part == NULL: one group), or of
// the group's partial blocks in the lane layout, part[((g * 2 + m) * ntri + tri) * BLOCK_DOUBLES ...], m = 0 for c00, 1 for c0t.
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
    sym48::block_of(tri, nblk, bi, bj);
    const int q = lane >> 4, col = lane & 15;
    const size_t stream = (size_t)nblk * G * step * 48;
    const double* pa = buf + (((size_t)bi * G + g) * step + q) * 48 + col;
    const double* pb = buf + (((size_t)bj * G + g) * step + q) * 48 + col;
    double* p00 = part ? part + ((((size_t)g * 2 + 0) * ntri + tri) * BLOCK_DOUBLES) + lane : nullptr;
    double* p0t = part ? part + ((((size_t)g * 2 + 1) * ntri + tri) * BLOCK_DOUBLES) + lane : nullptr;
    sym48::Block s00, s0t;
    sym48::zero(s00);
    sym48::zero(s0t);
    if (!first && part) {
        sym48::load_partial(s00, p00);
        sym48::load_partial(s0t, p0t);
    } else if (!first) {
        sym48::load_running(s00, bi, bj, q, col, D, c00);
        sym48::load_running(s0t, bi, bj, q, col, D, c0t);
    }
    // Two operand sets in turn (no register copies between steps): while one set's MFMAs run, the other set's loads are in flight.  The
    // step after the last one reloads the last step's operands (an address that is valid anyway) and never uses them.
    sym48::Operands<2> x, y;
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
        sym48::store_partial(s00, p00);
        sym48::store_partial(s0t, p0t);
    } else {
        sym48::store_mirrored(s00, bi, bj, q, col, D, c00);
        sym48::store_mirrored(s0t, bi, bj, q, col, D, c0t);
    }
}

// One wave per (block of the upper triangle = blockIdx.x, matrix = blockIdx.y): the G partial blocks are added in ascending g, in the lane
// layout the product kernel left them in, and the sums go to the matrix and to the mirrors.
__global__ void __launch_bounds__(64) lagged_reduce_kernel(const double* __restrict__ part, int nblk, long long ntri, int G, int D,
                                                           double* __restrict__ c00, double* __restrict__ c0t) {
    const long long tri = blockIdx.x;
    const int m = blockIdx.y, lane = threadIdx.x;
    int bi, bj;
    sym48::block_of(tri, nblk, bi, bj);
    const size_t per_group = (size_t)2 * ntri * BLOCK_DOUBLES;
    const double* p = part + ((size_t)m * ntri + tri) * BLOCK_DOUBLES + lane;
    sym48::Block acc;
    sym48::load_partial(acc, p);
    for (int g = 1; g < G; ++g) {
        p += per_group;
        sym48::add_partial(acc, p);
    }
    sym48::store_mirrored(acc, bi, bj, lane >> 4, lane & 15, D, m ? c0t : c00);
}

// One wave per row, sym48::project_row on f_s - mean read from f itself: the order is a function of D alone.
__global__ void __launch_bounds__(64) feature_project_kernel(const float* __restrict__ f, int D, const double* __restrict__ mean,
                                                             const double* __restrict__ comp, int K, double* __restrict__ proj) {
    const long long s = blockIdx.x;
    const float* row = f + s * D;
    sym48::project_row(D, [=](int c) { return ((double)row[c] - mean[c]); }, comp, K, proj + s * K);
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
    if (G > 1) hipLaunchKernelGGL(lagged_reduce_kernel, dim3((unsigned)sp.ntri, 2u), dim3(64), 0, st, part, sp.nblk, sp.ntri, G, D, c00, c0t);
    return (int)hipGetLastError();
}

extern "C" int s2s_feature_project(const float* f, int T, int D, const double* mean, const double* components, int n_components, double* proj,
                                   void* stream) {
    if (!f || !mean || !components || !proj || T < 1 || D < 1 || D > S2S_TICA_MAX_FEATURES || n_components < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(feature_project_kernel, dim3((unsigned)T), dim3(64), 0, (hipStream_t)stream, f, D, mean, components, n_components, proj);
    return (int)hipGetLastError();
}
