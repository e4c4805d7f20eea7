// Float64 Kabsch pieces shared by the superposition kernels (ensemble_rmsd.hip, ensemble_tm.hip): Horn's symmetric 4 x 4 quaternion
// matrix of a cross-covariance H, its eigen-decomposition by cyclic Jacobi, and the proper rotation of the top eigen-quaternion.
// Jacobi rather than Newton on the characteristic quartic: it converges on identical structures, mirror images, collinear / planar
// chains and L = 1, 2, 3, where Newton from (G_a + G_b) / 2 stalls on the (near-)multiple root.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace kabsch {

// One Jacobi rotation in the (P, Q) plane of the symmetric a (both triangles kept) and, with VEC, of the eigenvector columns v.
template <int P, int Q, bool VEC>
__device__ __forceinline__ bool jacobi_rotate(double (&a)[4][4], double (&v)[4][4], double thr) {
    const double apq = a[P][Q];
    if (!(fabs(apq) > thr)) return false;
    const double d = a[Q][Q] - a[P][P], b = 2.0 * apq;
    const double t = (d >= 0.0 ? b : -b) / (fabs(d) + sqrt(d * d + b * b));   // the smaller root of t^2 + 2 t theta - 1, theta = d / b
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    a[P][P] -= t * apq;
    a[Q][Q] += t * apq;
    a[P][Q] = a[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r != P && r != Q) {
            const double g = a[r][P], h = a[r][Q];
            a[r][P] = a[P][r] = c * g - s * h;
            a[r][Q] = a[Q][r] = s * g + c * h;
        }
        if (VEC) {
            const double g = v[r][P], h = v[r][Q];
            v[r][P] = c * g - s * h;
            v[r][Q] = s * g + c * h;
        }
    }
    return true;
}

// Cyclic Jacobi on a symmetric 4 x 4: sweeps until no off-diagonal entry exceeds 2^-58 ||a||_F (what is left moves an eigenvalue by
// far less than one rounding of ||a||), at most 16 sweeps (convergence is quadratic; 5-7 in practice).  a's diagonal = eigenvalues.
template <bool VEC>
__device__ __forceinline__ void jacobi4(double (&a)[4][4], double (&v)[4][4]) {
    double n2 = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            n2 += a[i][j] * a[i][j];
            if (VEC) v[i][j] = i == j ? 1.0 : 0.0;
        }
    if (!(n2 > 1e-260)) return;   // (a zero matrix; also keeps d*d + b*b above the underflow range)
    const double thr = sqrt(n2) * 0x1p-58;
    for (int sweep = 0; sweep < 16; ++sweep) {
        bool any = false;
        any |= jacobi_rotate<0, 1, VEC>(a, v, thr);
        any |= jacobi_rotate<0, 2, VEC>(a, v, thr);
        any |= jacobi_rotate<0, 3, VEC>(a, v, thr);
        any |= jacobi_rotate<1, 2, VEC>(a, v, thr);
        any |= jacobi_rotate<1, 3, VEC>(a, v, thr);
        any |= jacobi_rotate<2, 3, VEC>(a, v, thr);
        if (!any) break;
    }
}

// Horn's matrix of H[i][j] = sum w a_i b_j (the rotation takes a onto b); quaternion order (w, x, y, z).
__device__ __forceinline__ void horn_matrix(const double (&h)[3][3], double (&k)[4][4]) {
    k[0][0] = h[0][0] + h[1][1] + h[2][2];
    k[1][1] = h[0][0] - h[1][1] - h[2][2];
    k[2][2] = -h[0][0] + h[1][1] - h[2][2];
    k[3][3] = -h[0][0] - h[1][1] + h[2][2];
    k[0][1] = k[1][0] = h[1][2] - h[2][1];
    k[0][2] = k[2][0] = h[2][0] - h[0][2];
    k[0][3] = k[3][0] = h[0][1] - h[1][0];
    k[1][2] = k[2][1] = h[0][1] + h[1][0];
    k[1][3] = k[3][1] = h[2][0] + h[0][2];
    k[2][3] = k[3][2] = h[1][2] + h[2][1];
}

__device__ __forceinline__ double max_diag(const double (&k)[4][4]) {
    return fmax(fmax(k[0][0], k[1][1]), fmax(k[2][2], k[3][3]));
}

// The proper rotation (det = +1) that maximises tr(R H): R of the normalised eigen-quaternion of Horn's matrix of H for its largest
// eigenvalue, which is returned (any optimal rotation where the eigenspace is degenerate; the identity for H = 0).
__device__ __forceinline__ double horn_rotation(const double (&h)[3][3], double (&R)[3][3]) {
    double k[4][4], v[4][4];
    horn_matrix(h, k);
    jacobi4<true>(k, v);
    const double lam = max_diag(k);
    double qv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) qv[r] = k[0][0] == lam ? v[r][0] : k[1][1] == lam ? v[r][1] : k[2][2] == lam ? v[r][2] : v[r][3];
    const double qn = 1.0 / sqrt(qv[0] * qv[0] + qv[1] * qv[1] + qv[2] * qv[2] + qv[3] * qv[3]);
    const double qw = qv[0] * qn, qx = qv[1] * qn, qy = qv[2] * qn, qz = qv[3] * qn;
    R[0][0] = 1.0 - 2.0 * (qy * qy + qz * qz); R[0][1] = 2.0 * (qx * qy - qw * qz); R[0][2] = 2.0 * (qx * qz + qw * qy);
    R[1][0] = 2.0 * (qx * qy + qw * qz); R[1][1] = 1.0 - 2.0 * (qx * qx + qz * qz); R[1][2] = 2.0 * (qy * qz - qw * qx);
    R[2][0] = 2.0 * (qx * qz - qw * qy); R[2][1] = 2.0 * (qy * qz + qw * qx); R[2][2] = 1.0 - 2.0 * (qx * qx + qy * qy);
    return lam;
}

}  // namespace kabsch
