// The per-pair CLASS of the edge embedding's first layer: which distogram row and which relative-position row a pair (i, j) gathers.
// One definition for the kernels that need it -- edge_embed_f16_kernel (csrc/edge_embed_f16.h, setup_b) and the class expansion
// (csrc/pair_embed_expand.hip) -- because the bin rule's strict comparisons and the unfused distance are pinned by the parity tests.
#pragma once
#include <hip/hip_runtime.h>

namespace s2s {

constexpr int kEeBinSlots = 64 + 4;   // floats of the LDS edge table: n_bins <= 32 lower edges | 1e8 | 3e38 ...
constexpr int kEeRecProj = 168;       // floats of a class-table record with the fused projection: z[128] | attn_bias[8] | pair_z[32]
constexpr int kEeRecPlain = 128;      // ... without: z only

// s_bins (LDS, kEeBinSlots floats) <- the ascending lower edges, 1e8 (the last bin's upper edge), 3e38 beyond.  The caller synchronises.
__device__ __forceinline__ void ee_fill_bins(float* s_bins, const float* __restrict__ bin_lower, int n_bins) {
    if (threadIdx.x < kEeBinSlots)
        s_bins[threadIdx.x] = (int)threadIdx.x < n_bins ? bin_lower[threadIdx.x] : ((int)threadIdx.x == n_bins ? 1e8f : 3.0e38f);
}

// distogram bin of the pair with CA positions a, b: 0 .. n_bins - 1, or -1 for "none" (geo_utils.py:44-56)
// The squared distance is  fma(dz, dz, fma(dx, dx, dy dy)),  WRITTEN OUT: that is what the edge embedding has always evaluated -- its
// source said (dx dx + dy dy) + dz dz with the _rn intrinsics, which hipcc contracts all the same under the default -ffp-contract=fast
// -- and a pair whose distance lies within an ulp of a bin edge takes another bin with another rounding.  Explicit fmas leave the
// compiler no choice, so every kernel that includes this header picks the same bin, whatever its unit's flags.
__device__ __forceinline__ int ee_pair_bin(const float* s_bins, int n_bins, float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    const float dist = sqrtf(__fmaf_rn(dz, dz, __fmaf_rn(dx, dx, __fmul_rn(dy, dy))));
    // the reference's one-hot (dist > lower[k]) * (dist < upper[k]), upper = lower[k+1] (1e8 for the last): with ascending
    // edges (torch.linspace) that is k = #{edges < dist} - 1 unless dist sits exactly on the next edge (then no bin at all)
    int cnt = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {  // s_bins: n_bins <= 32 edges | 1e8 (the last bin's upper edge) | 3e38 ...
        const float4 e = *reinterpret_cast<const float4*>(&s_bins[4 * u]);
        cnt += (e.x < dist) + (e.y < dist) + (e.z < dist) + (e.w < dist);
    }
    cnt = cnt > n_bins ? n_bins : cnt;                  // dist beyond 1e8 when n_bins < 32: no bin, as below
    const float up = s_bins[cnt];                       // upper edge of bin cnt - 1
    return (cnt >= 1 && dist < up) ? cnt - 1 : -1;
}

// row of the relative-position table: idx_i - idx_j + rel_off, clamped to the table
__device__ __forceinline__ long long ee_rel_row(long long idx_i, long long idx_j, int rel_off, int n_rel) {
    long long d = idx_i - idx_j + rel_off;
    return d < 0 ? 0 : (d >= n_rel ? n_rel - 1 : d);
}

// row of the class table (s2s_edge_embed_classes_f16x3): fa, fb = class of fixed_mask at i, j (0 / 1); d = ee_rel_row; bin = ee_pair_bin
__device__ __forceinline__ unsigned ee_class_row(unsigned fa, unsigned fb, unsigned d, int bin, int n_rel, int n_bins) {
    return ((fa * 2u + fb) * (unsigned)n_rel + d) * (unsigned)(n_bins + 1) + (unsigned)(bin + 1);
}

}  // namespace s2s
