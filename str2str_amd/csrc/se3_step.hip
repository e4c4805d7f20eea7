// Fused SE(3) score + reverse step (gfx950).  One workgroup per sample, one thread per residue
// (strided when N > 256); the only cross-residue term is the per-sample centre of mass.
//
// Mirrors, op for op and dtype for dtype (float32 with the reference's float64 islands):
//   FrameDiffuser.score     src/models/score/frame.py:109-143
//   SO3Diffuser.score       src/models/score/so3.py:274-309  (+ igso3_expansion :21-62, score :85-130)
//   R3Diffuser.score        src/models/score/r3.py:133-137
//   FrameDiffuser.reverse   frame.py:153-210
//   SO3Diffuser.reverse     so3.py:333-370  (compose_rotvec in float64, so3.py:13-19)
//   R3Diffuser.reverse      r3.py:79-125    (float64 after the float64 mask promotion)
//   assemble_rigid + Rigid.to_tensor_7   frame.py:9-15, rigid_utils.py:1203-1215
//
// The per-sample schedule scalars (sigma bin, g(t)^2, exp(-beta/2), 1-exp(-beta), b(t)) are
// computed on the host once per trajectory with the reference's own float32 formulae and passed
// in `params` (8 floats per sample): no np.digitize round trip inside the loop.
//
// IGSO(3) series: omega (float32, from the reference's float32 conversion chain) and the float32 weights are promoted
// and the 1000-term sums of so3.py:21-62 / :85-130 are evaluated entirely in float64 -- the exact value of the formula the
// reference evaluates in float32.  Where that formula is well conditioned the two agree to float32 rounding; where it is
// not (f << sum|terms|, or the O(omega^3) difference lo*dhi - hi*dlo at small omega) the reference's own float32 value is
// rounding noise around this one.  Parity is judged against float64 anchors generated from the reference's own functions
// (tests/golden/make_golden_score64.py): |ours - ref64| <= |ref32 - ref64| + 4e-5 |s| per residue.  Terms whose float32
// weight exp(-l(l+1)sigma^2/2) underflowed to 0 contribute exactly 0 and are skipped.  Two departures from the chain: the
// product quaternion q0^-1 qt is taken with w >= 0 before it becomes a rotation vector, and q0 = +-qt gives v = 0 (see there);
// against float64 the score then sits within 3 x the chain's own principal-branch distance on every orientation and is exactly
// 0 for one rotation on both sides (tests/score_cases.py).
#include <hip/hip_runtime.h>

#include "geom.h"
#include "str2str_hip.h"

using namespace s2s;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxPerThread = 8;  // N <= 2048
constexpr int kL = 1000;

__global__ void __launch_bounds__(kThreads) se3_step_kernel(
    const float* __restrict__ x0_7, const float* __restrict__ xt_7, const float* __restrict__ mask,
    const float* __restrict__ diffuse_mask, const float* __restrict__ params, const double* __restrict__ z_rot,
    const double* __restrict__ z_trans, const double* __restrict__ rot_score_in,
    const double* __restrict__ trans_score_in, float* __restrict__ next7, double* __restrict__ rot_score_out,
    double* __restrict__ trans_score_out, int N, double dt_all, const double* __restrict__ dt_per_sample, double coord_scale_d,
    int probability_flow, int center, double noise_scale) {
    __shared__ double s_cw[kL];      // (2l+1) * exp(-l(l+1) sigma^2 / 2) in float64 (sigma = the float32 bin value)
    __shared__ int s_leff;
    __shared__ double s_red[4][kThreads / 64];
    __shared__ double s_com[3];

    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    // the step size is a property of a trajectory (1 / int(num_timesteps T), diffusion_module.py:267 of the reference): one value
    // for the batch, or one per sample when trajectories of different length share a batch
    const double dt = dt_per_sample ? dt_per_sample[b] : dt_all;
    // x * 0.1 on a float32 tensor uses float32(0.1); x / 0.1 on the float64 tensor uses the double 0.1
    const float coord_scale = (float)coord_scale_d;
    const float* P = params + (long long)b * 8;
    const float sigma = P[0], g2_rot = P[1], e_half = P[2], cond_var = P[3], b_t = P[4], g2_trans = P[5];
    const float g_rot = P[6], g_trans = P[7];

    if (tid == 0) s_leff = 0;
    __syncthreads();
    {
        const double s2 = (double)sigma * (double)sigma;
        int last = 0;
        for (int l = tid; l < kL; l += kThreads) {
            const double a = -(double)(l * (l + 1));
            const double w = exp(a * s2 / 2.0);
            s_cw[l] = (double)(2 * l + 1) * w;
            if ((float)w != 0.0f) last = l + 1;  // below the float32 underflow the reference's term is exactly 0
        }
        atomicMax(&s_leff, last);
    }
    __syncthreads();
    const int leff = s_leff;

    double x1[kMaxPerThread][3];
    double part[4] = {0.0, 0.0, 0.0, 0.0};  // x, y, z sums and the residue count of the centre of mass
    const double half_or_one = probability_flow ? 0.5 : 1.0;

#pragma unroll
    for (int it = 0; it < kMaxPerThread; ++it) {
        const int n = tid + it * kThreads;
        x1[it][0] = x1[it][1] = x1[it][2] = 0.0;
        if (n >= N) continue;
        const long long r = (long long)b * N + n;
        const float* a0 = (rot_score_in ? xt_7 : x0_7) + r * 7;
        const float* at = xt_7 + r * 7;
        const Quat<float> q0{a0[0], a0[1], a0[2], a0[3]};
        const Vec3<float> t0{a0[4], a0[5], a0[6]};
        const Quat<float> qt{at[0], at[1], at[2], at[3]};
        const Vec3<float> tt{at[4], at[5], at[6]};
        const double m = (double)mask[r];
        const double dm = (double)diffuse_mask[r];

        const Mat3<float> Rt = quat_to_rot<float>(qt);
        const Quat<float> qtm = matrix_to_quaternion<float>(Rt);
        const float xts[3] = {tt.x * coord_scale, tt.y * coord_scale, tt.z * coord_scale};
        double rs[3], tsc[3];
        if (rot_score_in) {  // reverse-only call (FrameDiffuser.reverse with caller-provided scores)
#pragma unroll
            for (int c = 0; c < 3; ++c) { rs[c] = rot_score_in[r * 3 + c]; tsc[c] = trans_score_in[r * 3 + c]; }
        } else {
        // ---- rotation score: v = log(R0^T R_t) through the reference's conversion chain
        const float n2 = q0.w * q0.w + q0.x * q0.x + q0.y * q0.y + q0.z * q0.z;
        const Quat<float> q0inv{q0.w / n2, (q0.x * -1.0f) / n2, (q0.y * -1.0f) / n2, (q0.z * -1.0f) / n2};
        const Quat<float> q0i = matrix_to_quaternion<float>(quat_to_rot<float>(q0inv));
        // Both factors leave matrix_to_quaternion with their largest component positive, so whenever that component is not w
        // the inverse and the frame take opposite signs and the product has w = -cos(theta / 2): the same rotation as angle
        // 2 pi - theta, rebuilt as |xyz| * angle / sin(angle / 2) one rounding of atan2f from sin's zero (3e-6 / theta rad of
        // noise in omega).  The representative with w >= 0 gives the same score vector (f is symmetric about pi, df
        // antisymmetric, v flips) from the principal angle, where the conversion is well conditioned.
        Quat<float> p = quat_multiply<float>(q0i, qtm);
        if (p.w < 0.0f) { p.w = -p.w; p.x = -p.x; p.y = -p.y; p.z = -p.z; }
        Vec3<float> v = quaternion_to_axis_angle<float>(p);
        // One rotation on both sides (q0 = qt or q0 = -qt, component for component): R0^T Rt is the identity and the score is
        // exactly 0.  The chain does not return that: invert_quat divides by |q|^2, which is 1 to float32 rounding only, so
        // R(q0^-1) is not the exact transpose of R(qt) and v comes out as a few 1e-8 (a score of up to 1e-5 at sigma = 0.1).
        const bool same = (q0.w == qt.w && q0.x == qt.x && q0.y == qt.y && q0.z == qt.z) ||
                          (q0.w == -qt.w && q0.x == -qt.x && q0.y == -qt.y && q0.z == -qt.z);
        if (same) v.x = v.y = v.z = 0.0f;
        const float omega = sqrtf(v.x * v.x + v.y * v.y + v.z * v.z) + 1e-6f;

        const double omd = (double)omega;
        const double lo = sin(omd / 2.0);
        const double dlo = 0.5 * cos(omd / 2.0);
        double f = 0.0, df = 0.0;
        for (int l = 0; l < leff; ++l) {
            const double lh = (double)l + 0.5;
            double hi, ch;
            sincos(omd * lh, &hi, &ch);
            const double cw = s_cw[l];
            f += cw * hi / lo;
            df += cw * (lo * (lh * ch) - hi * dlo) / (lo * lo);
        }
        const float ff = (float)f;
        const float sc = (float)df / (ff + 1e-4f);
        const float den = omega + 1e-6f;
        rs[0] = (double)((sc * v.x) / den) * m; rs[1] = (double)((sc * v.y) / den) * m; rs[2] = (double)((sc * v.z) / den) * m;

        // ---- translation score (scaled coordinates)
        const float x0s[3] = {t0.x * coord_scale, t0.y * coord_scale, t0.z * coord_scale};
#pragma unroll
        for (int c = 0; c < 3; ++c) tsc[c] = (double)(-(xts[c] - e_half * x0s[c]) / cond_var) * m;
        }

        if (rot_score_out) {
            rot_score_out[r * 3 + 0] = rs[0]; rot_score_out[r * 3 + 1] = rs[1]; rot_score_out[r * 3 + 2] = rs[2];
        }
        if (trans_score_out) {
            trans_score_out[r * 3 + 0] = tsc[0]; trans_score_out[r * 3 + 1] = tsc[1]; trans_score_out[r * 3 + 2] = tsc[2];
        }
        if (!next7) continue;

        // ---- reverse, rotation: geodesic step R(rot_t) * R(-perturb) in float64
        const Vec3<float> rot_t = quaternion_to_axis_angle<float>(qtm);
        double pr[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double drift = ((double)(-1.0f * g2_rot) * rs[c]) * dt * half_or_one;
            double diff = 0.0;
            if (!probability_flow) diff = (double)(g_rot * (float)sqrt(dt)) * (noise_scale * z_rot[r * 3 + c]);
            pr[c] = -1.0 * (drift + diff);
        }
        const Mat3<float> R1f = quaternion_to_matrix<float>(axis_angle_to_quaternion<float>(rot_t));
        const Mat3<double> R1 = mat_cast<double, float>(R1f);
        const Mat3<double> R2 = quaternion_to_matrix<double>(axis_angle_to_quaternion<double>(Vec3<double>{pr[0], pr[1], pr[2]}));
        const Mat3<double> cR = rot_matmul<double>(R1, R2);
        const Vec3<double> rv1d = quaternion_to_axis_angle<double>(matrix_to_quaternion<double>(cR));
        const float rot_1[3] = {(float)rv1d.x, (float)rv1d.y, (float)rv1d.z};
        const float rt[3] = {rot_t.x, rot_t.y, rot_t.z};
        Vec3<double> rvn;
        rvn.x = dm * (double)rot_1[0] + (1.0 - dm) * (double)rt[0];
        rvn.y = dm * (double)rot_1[1] + (1.0 - dm) * (double)rt[1];
        rvn.z = dm * (double)rot_1[2] + (1.0 - dm) * (double)rt[2];
        const Mat3<double> Rn = quaternion_to_matrix<double>(axis_angle_to_quaternion<double>(rvn));
        const Quat<float> qn = matrix_to_quaternion<float>(mat_cast<float, double>(Rn));
        float* o = next7 + r * 7;
        o[0] = qn.w; o[1] = qn.x; o[2] = qn.y; o[3] = qn.z;

        // ---- reverse, translation (float64 from the score promotion onwards)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float fc = (-0.5f * b_t) * xts[c];
            double drift = ((double)fc - (double)g2_trans * tsc[c]) * dt * half_or_one;
            double diff = 0.0;
            if (!probability_flow) diff = (double)(g_trans * (float)sqrt(dt)) * (noise_scale * z_trans[r * 3 + c]);
            x1[it][c] = (double)xts[c] - (drift + diff);
            part[c] += (center == 2) ? m * x1[it][c] : x1[it][c];
        }
        part[3] += (center == 2) ? m : 1.0;
    }
    if (!next7) return;

    // ---- centre of mass: center == 1 over ALL residues of the sample, as the reference does (r3.py:117-122
    //      is called with mask=None); center == 2 over the residues with mask > 0 only, which is what makes
    //      a padded (mixed-length) batch reproduce each chain's un-padded run
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        double v = part[c];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((tid & 63) == 0) s_red[c][tid >> 6] = v;
    }
    __syncthreads();
    if (tid < 3) {
        double v = 0.0, cnt = 0.0;
        for (int w = 0; w < kThreads / 64; ++w) { v += s_red[tid][w]; cnt += s_red[3][w]; }
        // a sample without residues (center == 2, mask all zero) has no centre: 0, not 0 / 0, which would turn the
        // translations of its frozen residues into NaN through 0 * NaN in the blend below
        s_com[tid] = (center && cnt > 0.0) ? v / (double)(float)cnt : 0.0;
    }
    __syncthreads();

#pragma unroll
    for (int it = 0; it < kMaxPerThread; ++it) {
        const int n = tid + it * kThreads;
        if (n >= N) continue;
        const long long r = (long long)b * N + n;
        const double dm = (double)diffuse_mask[r];
        float* o = next7 + r * 7;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double xc = (x1[it][c] - s_com[c]) / coord_scale_d;
            const double blended = dm * xc + (1.0 - dm) * (double)xt_7[r * 7 + 4 + c];
            o[4 + c] = (float)blended;
        }
    }
}

}  // namespace

extern "C" int s2s_se3_step(const float* x0_7, const float* xt_7, const float* mask, const float* diffuse_mask,
                            const float* params8, const double* z_rot, const double* z_trans,
                            const double* rot_score_in, const double* trans_score_in, float* next7,
                            double* rot_score_out, double* trans_score_out, int n_samples, int n_res, double dt,
                            const double* dt_per_sample, double coordinate_scaling, int probability_flow, int center_trans,
                            double noise_scale, void* stream) {
    if (n_samples <= 0 || n_res <= 0) return 0;
    if (n_res > kThreads * kMaxPerThread) return (int)hipErrorInvalidValue;
    if (!probability_flow && (!z_rot || !z_trans)) return (int)hipErrorInvalidValue;
    if ((rot_score_in == nullptr) != (trans_score_in == nullptr)) return (int)hipErrorInvalidValue;
    if (!rot_score_in && !x0_7) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(se3_step_kernel, dim3(n_samples), dim3(kThreads), 0, (hipStream_t)stream, x0_7, xt_7, mask,
                       diffuse_mask, params8, z_rot, z_trans, rot_score_in, trans_score_in, next7, rot_score_out, trans_score_out, n_res, dt,
                       dt_per_sample, coordinate_scaling, probability_flow, center_trans, noise_scale);
    return (int)hipGetLastError();
}
