// The cross-covariance product of csrc/ensemble_rmsd.hip (H of 16 x 16 pairs per wave, float64) in two formulations on the same
// prepass buffers: v_mfma_f64_16x16x4_f64 (nine accumulator tiles) against plain float64 FMAs with the same lane -> pair map (36 FMAs and
// 15 loads per residue and lane).  1000 x 10000 structures, L = 256; each pair stores one asymmetric combination of its nine sums.
// Prints both times (interleaved rounds, median) and the largest difference of the outputs (summation order differs: rounding size).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cmath>
#include <vector>
typedef double d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void store(const double (&h)[3][3], double* out, size_t idx) {
    double s = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) s += (double)(3 * i + j + 1) * h[i][j];
    out[idx] = s;
}

template <bool MFMA>
__global__ void __launch_bounds__(256) product(const double* __restrict__ a_buf, const double* __restrict__ b_buf, int n_a, int n_b, int Lp,
                                               double* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, bi = blockIdx.y, bj = blockIdx.x * 4 + wave;
    if (bj >= (n_b + 15) / 16) return;
    const int q = lane >> 4, col = lane & 15;
    const double* pb = b_buf + (size_t)bj * Lp * 48;
    const double* pa = a_buf + (size_t)bi * Lp * 48;
    d4 acc[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
    if (MFMA) {
        pa += q * 48 + col; pb += q * 48 + col;
        for (int k0 = 0; k0 < Lp; k0 += 4, pa += 192, pb += 192) {
            double av[3], bv[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { av[c] = pa[16 * c]; bv[c] = pb[16 * c]; }
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
    } else {
        pa += q; pb += col;    // rows q + 4 r of the A block, column col of the B block
        for (int k = 0; k < Lp; ++k, pa += 48, pb += 48) {
            double bv[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) bv[c] = pb[16 * c];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double av = pa[16 * i + 4 * r];
#pragma unroll
                    for (int j = 0; j < 3; ++j) acc[i][j][r] = fma(av, bv[j], acc[i][j][r]);
                }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int gi = bi * 16 + q + 4 * r, gj = bj * 16 + col;
        if (gi >= n_a || gj >= n_b) continue;
        double h[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) h[i][j] = acc[i][j][r];
        store(h, out, (size_t)gi * n_b + gj);
    }
}

int main() {
    const int n_a = 1000, n_b = 10000, L = 256, nba = (n_a + 15) / 16, nbb = (n_b + 15) / 16;
    std::vector<double> ha((size_t)nba * L * 48), hb((size_t)nbb * L * 48);
    unsigned long long st = 88172645463325252ull;
    auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (double)(st >> 11) / 9007199254740992.0 * 40.0 - 20.0; };
    for (auto& v : ha) v = rnd();
    for (auto& v : hb) v = rnd();
    double *da, *db, *o0, *o1;
    const size_t ob = (size_t)n_a * n_b * sizeof(double);
    if (hipMalloc(&da, ha.size() * 8) || hipMalloc(&db, hb.size() * 8) || hipMalloc(&o0, ob) || hipMalloc(&o1, ob)) return 1;
    hipMemcpy(da, ha.data(), ha.size() * 8, hipMemcpyHostToDevice);
    hipMemcpy(db, hb.data(), hb.size() * 8, hipMemcpyHostToDevice);
    const dim3 grid((nbb + 3) / 4, nba), block(256);
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    std::vector<float> t[2];
    for (int round = 0; round < 43; ++round)      // 3 warm-up rounds, then 40 interleaved
        for (int v = 0; v < 2; ++v) {
            hipEventRecord(e0, 0);
            if (v == 0) hipLaunchKernelGGL((product<true>), grid, block, 0, 0, da, db, n_a, n_b, L, o0);
            else hipLaunchKernelGGL((product<false>), grid, block, 0, 0, da, db, n_a, n_b, L, o1);
            hipEventRecord(e1, 0);
            if (hipEventSynchronize(e1) != hipSuccess) return 2;
            float ms; hipEventElapsedTime(&ms, e0, e1);
            if (round >= 3) t[v].push_back(ms);
        }
    std::vector<double> r0((size_t)n_a * n_b), r1(r0.size());
    hipMemcpy(r0.data(), o0, ob, hipMemcpyDeviceToHost); hipMemcpy(r1.data(), o1, ob, hipMemcpyDeviceToHost);
    double dmax = 0, vmax = 0;
    for (size_t i = 0; i < r0.size(); ++i) { dmax = std::max(dmax, std::fabs(r0[i] - r1[i])); vmax = std::max(vmax, std::fabs(r0[i])); }
    const double flop = 18.0 * L * n_a * n_b;
    for (int v = 0; v < 2; ++v) {
        std::sort(t[v].begin(), t[v].end());
        const double med = t[v][t[v].size() / 2];
        printf("%s  median %.3f ms  min %.3f ms  %.1f TFLOP/s (median)\n", v ? "f64 FMA " : "f64 MFMA", med, t[v][0], flop / med * 1e-9);
    }
    printf("max |MFMA - FMA| = %.3e (largest value %.3e)\n", dmax, vmax);
    return 0;
}
