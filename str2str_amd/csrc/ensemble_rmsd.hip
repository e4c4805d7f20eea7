// Minimum RMSD under optimal rigid superposition, on the device: what users do first with the ensembles the sampler writes
// (superpose, distance from the start, diversity, coverage of an MD reference, RMSF).  The reference repository has no such
// function; the yardstick is a float64 SVD Kabsch (tests/test_ensemble_rmsd.py).
//
//   s2s_ca_rmsd_matrix   all pairs of two ensembles.  With weighted centroids a-bar, b-bar and centred coordinates,
//                          MSD = (G_a + G_b - 2 lambda) / W,   G = sum_i w_i |x_i - x-bar|^2,   W = sum_i w_i,
//                        lambda = the largest eigenvalue of Horn's symmetric 4 x 4 matrix built from the nine entries of
//                        H_ab = sum_i w_i (a_i - a-bar)(b_i - b-bar)^T: the maximum of tr(R H) over PROPER rotations (det R = +1; a
//                        mirror image is not superposable).  All H of a 16 x 16 block of pairs are one [48, L] x [L, 48] float64
//                        matrix product on v_mfma_f64_16x16x4_f64: nine accumulator tiles, tile (c_a, c_b) = H[c_a][c_b] of the 256 pairs,
//                        so every lane ends the loop over residues holding the complete H of its four pairs.
//   s2s_ca_superpose     many mobile structures onto one target: RMSD and the transform (rotation from the eigen-quaternion).
//   s2s_apply_xform      one transform per sample applied to float32 points.
//
// Everything is float64 (the float32 inputs are widened first): the MSD is the small difference of numbers of size L Rg^2, and a
// float32 evaluation of the same formula errs by 1e-3 .. 1e-2 A in RMSD between near-identical conformations.
// Eigenvalues by cyclic Jacobi on the 4 x 4 (kabsch_f64.h, shared with ensemble_tm.hip).
#include <hip/hip_runtime.h>
#include <math.h>

#include "ensemble_common.h"
#include "kabsch_f64.h"
#include "str2str_hip.h"
#include "sym48_f64.h"

namespace {

using namespace kabsch;
using ensemble::wave_sum;

// Prepass, one wave per structure slot (slots n .. 16 ceil(n/16) - 1 and residues L .. Lp - 1 are zero padding): weighted centroid, G, and
// sqrt(w_i) (x_i - x-bar) as float64 in blocks of 16 structures, out[(blk * Lp + i) * 48 + 16 c + s].  The SAME scaled coordinates serve
// as either operand of the product, so H_ba is the transpose of H_ab bit for bit (products commute, the sums run in one order).
__global__ void __launch_bounds__(64) rmsd_prep_kernel(const float* __restrict__ x, int n, int L, int Lp, const float* __restrict__ w,
                                                       double* __restrict__ g_out, double* __restrict__ out, double* __restrict__ w_sum) {
    const int s = blockIdx.x, lane = threadIdx.x;
    double* o = out + ((size_t)(s >> 4) * Lp) * 48 + (s & 15);
    if (s >= n) {
        for (int i = lane; i < Lp; i += 64) { o[(size_t)i * 48] = 0.0; o[(size_t)i * 48 + 16] = 0.0; o[(size_t)i * 48 + 32] = 0.0; }
        if (lane == 0) g_out[s] = 0.0;
        return;
    }
    const float* p = x + (size_t)s * L * 3;
    double sw = 0, sx = 0, sy = 0, sz = 0;
    for (int i = lane; i < L; i += 64) {
        const double wi = w ? (double)w[i] : 1.0;
        sw += wi; sx += wi * p[3 * i]; sy += wi * p[3 * i + 1]; sz += wi * p[3 * i + 2];
    }
    sw = wave_sum(sw); sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz);
    const double cx = sx / sw, cy = sy / sw, cz = sz / sw;
    double g = 0;
    for (int i = lane; i < Lp; i += 64) {
        double dx = 0, dy = 0, dz = 0;
        if (i < L) {
            const double wi = w ? (double)w[i] : 1.0, r = w ? sqrt(wi) : 1.0;
            dx = p[3 * i] - cx; dy = p[3 * i + 1] - cy; dz = p[3 * i + 2] - cz;
            g += wi * (dx * dx + dy * dy + dz * dz);
            dx *= r; dy *= r; dz *= r;
        }
        o[(size_t)i * 48] = dx; o[(size_t)i * 48 + 16] = dy; o[(size_t)i * 48 + 32] = dz;
    }
    g = wave_sum(g);
    if (lane == 0) {
        g_out[s] = g;
        if (s == 0 && w_sum) *w_sum = sw;
    }
}

// One wave per 16 x 16 block of pairs (A block = blockIdx.y, B block = 4 blockIdx.x + wave), on the tiles, operands and lane maps of
// sym48_f64.h: register r of lane l holds the pair (row (l >> 4) + 4 r, column l & 15) of the block in every tile.  row0 >= 0: the A
// ensemble is rows row0 .. of the B ensemble (a row chunk of a self matrix); a pair below the diagonal is then evaluated as its mirror
// pair (H transposed in registers), so the matrix is exactly symmetric and independent of the chunking.
// mirror: the whole self matrix in one launch -- blocks below the diagonal are skipped and written by their mirror block.
__global__ void __launch_bounds__(256) rmsd_pairs_kernel(const double* __restrict__ a_buf, const double* __restrict__ g_a, int n_a,
                                                         const double* __restrict__ b_buf, const double* __restrict__ g_b, int n_b, int L,
                                                         int Lp, const double* __restrict__ w_sum, long long row0, int mirror,
                                                         double* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bi = blockIdx.y, bj = blockIdx.x * 4 + wave;
    if (bj >= (n_b + 15) / 16) return;   // wave-uniform; no block-level synchronisation in this kernel
    if (mirror && bi > bj) return;
    const int q = lane >> 4, col = lane & 15;
    const double* pa = a_buf + (size_t)bi * Lp * 48 + q * 48 + col;
    const double* pb = b_buf + (size_t)bj * Lp * 48 + q * 48 + col;
    sym48::Block acc;
    sym48::zero(acc);
    for (int k0 = 0; k0 < Lp; k0 += 4) {
        sym48::Operands<1> x;
        x.load(pa, pb);
        pa += 192; pb += 192;
        x.accumulate(acc);
    }
    const double W = *w_sum;
    const int gj = bj * 16 + col;
    const double gb = g_b[gj];   // (the G arrays are padded to whole blocks)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int gi = bi * 16 + q + 4 * r;
        if (gi >= n_a || gj >= n_b) continue;
        const bool swap = row0 >= 0 && row0 + gi > gj;
        double h[3][3], k[4][4], v[4][4];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) h[i][j] = swap ? acc[j][i][r] : acc[i][j][r];
        horn_matrix(h, k);
        jacobi4<false>(k, v);
        const double msd = L == 1 ? 0.0 : (g_a[gi] + gb - 2.0 * max_diag(k)) / W;   // (one point superposes exactly)
        const double rmsd = sqrt(fmax(msd, 0.0));
        out[(size_t)gi * n_b + gj] = rmsd;
        if (mirror && bi < bj) out[(size_t)gj * n_b + gi] = rmsd;
    }
}

// One wave per mobile structure; every lane repeats the 4 x 4 eigenproblem (no divergence), lane 0 writes.
__global__ void __launch_bounds__(64) superpose_kernel(const float* __restrict__ mobile, int L, const float* __restrict__ target,
                                                       const float* __restrict__ w, double* __restrict__ rmsd, double* __restrict__ xform) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const float* m = mobile + (size_t)s * L * 3;
    double sw = 0, cm[3] = {0, 0, 0}, ct[3] = {0, 0, 0};
    for (int i = lane; i < L; i += 64) {
        const double wi = w ? (double)w[i] : 1.0;
        sw += wi;
#pragma unroll
        for (int c = 0; c < 3; ++c) { cm[c] += wi * m[3 * i + c]; ct[c] += wi * target[3 * i + c]; }
    }
    sw = wave_sum(sw);
#pragma unroll
    for (int c = 0; c < 3; ++c) { cm[c] = wave_sum(cm[c]) / sw; ct[c] = wave_sum(ct[c]) / sw; }
    double h[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, g = 0;
    for (int i = lane; i < L; i += 64) {
        const double wi = w ? (double)w[i] : 1.0;
        double a[3], b[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { a[c] = m[3 * i + c] - cm[c]; b[c] = target[3 * i + c] - ct[c]; }
        g += wi * (a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double wa = wi * a[c];
#pragma unroll
            for (int e = 0; e < 3; ++e) h[c][e] += wa * b[e];
        }
    }
    g = wave_sum(g);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int e = 0; e < 3; ++e) h[c][e] = wave_sum(h[c][e]);
    double R[3][3];
    const double lam = horn_rotation(h, R);
    if (lane == 0) {
        const double msd = L == 1 ? 0.0 : (g - 2.0 * lam) / sw;
        rmsd[s] = sqrt(fmax(msd, 0.0));
        double* o = xform + (size_t)s * 12;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            o[3 * c] = R[c][0]; o[3 * c + 1] = R[c][1]; o[3 * c + 2] = R[c][2];
            o[9 + c] = ct[c] - (R[c][0] * cm[0] + R[c][1] * cm[1] + R[c][2] * cm[2]);
        }
    }
}

__global__ void __launch_bounds__(256) apply_xform_kernel(const float* __restrict__ pts, const double* __restrict__ xform, long long n_total,
                                                          long long M, float* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_total) return;
    const double* t = xform + (idx / M) * 12;
    const double x = pts[3 * idx], y = pts[3 * idx + 1], z = pts[3 * idx + 2];
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * idx + c] = (float)(t[3 * c] * x + t[3 * c + 1] * y + t[3 * c + 2] * z + t[9 + c]);
}

inline long long region_doubles(long long n, long long Lp) { return ((n + 15) / 16) * 16 * (3 * Lp + 1); }

}  // namespace

extern "C" int s2s_ca_rmsd_matrix(const float* a, int n_a, const float* b, int n_b, int n_res, const float* weights, double* rmsd,
                                  double* workspace, long long workspace_doubles, void* stream) {
    if (!a || !b || !rmsd || !workspace || n_a < 1 || n_b < 1 || n_res < 1) return (int)hipErrorInvalidValue;
    const long long Lp = ((long long)n_res + 3) / 4 * 4, nba = ((long long)n_a + 15) / 16, nbb = ((long long)n_b + 15) / 16;
    if ((long long)n_a * n_b >= (1ll << 31) || nba > 65535) return (int)hipErrorInvalidValue;
    const bool whole = a == b && n_a == n_b;
    const long long need = 2 + region_doubles(n_b, Lp) + (whole ? 0 : region_doubles(n_a, Lp));
    if (workspace_doubles < need) return (int)hipErrorInvalidValue;
    const long long row0 = ensemble::self_row0(a, b, n_a, n_b, n_res);
    hipStream_t st = (hipStream_t)stream;
    double* gb = workspace + 2;
    double* cb = gb + nbb * 16;
    double* ga = whole ? gb : cb + nbb * Lp * 48;
    double* ca = whole ? cb : ga + nba * 16;
    hipLaunchKernelGGL(rmsd_prep_kernel, dim3((unsigned)(nbb * 16)), dim3(64), 0, st, b, n_b, n_res, (int)Lp, weights, gb, cb, workspace);
    if (!whole)
        hipLaunchKernelGGL(rmsd_prep_kernel, dim3((unsigned)(nba * 16)), dim3(64), 0, st, a, n_a, n_res, (int)Lp, weights, ga, ca,
                           (double*)nullptr);
    hipLaunchKernelGGL(rmsd_pairs_kernel, dim3((unsigned)((nbb + 3) / 4), (unsigned)nba), dim3(256), 0, st, ca, ga, n_a, cb, gb, n_b, n_res,
                       (int)Lp, workspace, row0, whole ? 1 : 0, rmsd);
    return (int)hipGetLastError();
}

extern "C" int s2s_ca_superpose(const float* mobile, int n_mobile, const float* target, int n_res, const float* weights, double* rmsd,
                                double* xform, void* stream) {
    if (!mobile || !target || !rmsd || !xform || n_mobile < 1 || n_res < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(superpose_kernel, dim3((unsigned)n_mobile), dim3(64), 0, (hipStream_t)stream, mobile, n_res, target, weights, rmsd,
                       xform);
    return (int)hipGetLastError();
}

extern "C" int s2s_apply_xform(const float* points, const double* xform, int n_samples, long long n_points, float* out, void* stream) {
    if (!points || !xform || !out || n_samples < 1 || n_points < 1) return (int)hipErrorInvalidValue;
    const long long total = (long long)n_samples * n_points, blocks = (total + 255) / 256;
    if (blocks >= (1ll << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(apply_xform_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, points, xform, total, n_points, out);
    return (int)hipGetLastError();
}
