// Device helpers shared by the MFMA translation units: the vector types, the 32 x 32 accumulator layout, a compile-time loop and
// the split-f16 ("f16x3") primitive.
//
// Split.  An fp32 value x becomes two f16 numbers  x = x_h + x_l (+ <= 2^-24 |x|),  x_h = rn16(x),  x_l = rn16(x - x_h), and a
// product keeps  W_h x_h + W_h x_l + W_l x_h  on v_mfma_f32_32x32x16_f16 (csrc/pair_f16.h, header).  The split is written as
// ONE opaque inline-asm block per 2 or 4 values:
//   x_h = rn16(x):            v_cvt_pk_f16_f32, two values per instruction
//   x_l = rn16(x - x_h):      the difference is exact in fp32, so ONE fused multiply-add that reads x_h as f16 and rounds to f16
//                             (v_fma_mixlo / mixhi_f16:  (-x_h) * 1.0 + x) gives the bits of convert-back + subtract + convert
//   range maximum:            v_max3_f32 with |.| (range_flag.h)
// = 1.5 VALU instructions per value, 2 with the maximum (hipcc's expansion of the C expressions: 6).  Why one opaque block:
//   - both planes come from the same materialised fp32 value.  With fp contraction the compiler otherwise derives x_h and x_l from
//     DIFFERENT fused forms of the producing expression, and near an f16 rounding tie the pair then misses x by a whole f16 ulp;
//   - the block stays where it is written (the edge kernels pin VALU pieces under specific MFMAs);
//   - the maximum does not enter the compiler's reasoning (as an fmaxf chain it cost 300 spilled registers).
// Kernels group these blocks as their schedules need (split8_f16 in node_gemm.hip, enc_split8 in enc_attention.hip, ...).
#pragma once
#include <hip/hip_runtime.h>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));   // a 16 B fragment
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// weights are packed as the split of 2^5 w (W_l stays in f16's normal range): accumulators carry 32 x the layer output
constexpr float kWS = 32.0f, kInvWS = 1.0f / 32.0f;

__device__ __forceinline__ f32x16 mfma_f16(f16x8 a, f16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
// row of a 32 x 32 tile held by accumulator register r of a lane in half h (lanes 32 h .. 32 h + 31)
__device__ __forceinline__ int rowmap(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
// v + the same register of lane ^ 32: a sum over the wave's two halves
__device__ __forceinline__ float xhalf_sum(float v) { return v + __shfl_xor(v, 32, 64); }
// this lane's 4 consecutive elements of group g of a B-layout vector
__device__ __forceinline__ float4 ldg4(const float* __restrict__ base, int g, int h) {
    return *reinterpret_cast<const float4*>(base + 8 * g + 4 * h);
}

// compile-time loop: f(IC<B>{}), f(IC<B + 1>{}), ..., f(IC<E - 1>{})
template <int I> struct IC { static constexpr int value = I; };
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B < E) {
        f(IC<B>{});
        static_for<B + 1, E>(f);
    }
}

// Four values -> x_h as two packed f16 pairs (h0 = x0, x1; h1 = x2, x3), x_l the same (l0, l1); |x| into the range maximum.
__device__ __forceinline__ void split4_f16(float x0, float x1, float x2, float x3, unsigned& h0, unsigned& h1, unsigned& l0, unsigned& l1,
                                           float& amax) {
    asm volatile(
        "v_max3_f32 %4, %4, |%5|, |%6|\n\t"
        "v_cvt_pk_f16_f32 %0, %5, %6\n\t"
        "v_max3_f32 %4, %4, |%7|, |%8|\n\t"
        "v_cvt_pk_f16_f32 %1, %7, %8\n\t"
        "v_fma_mixlo_f16 %2, -%0, 1.0, %5 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixlo_f16 %3, -%1, 1.0, %7 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %2, -%0, 1.0, %6 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %3, -%1, 1.0, %8 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
        : "=&v"(h0), "=&v"(h1), "=&v"(l0), "=&v"(l1), "+v"(amax)
        : "v"(x0), "v"(x1), "v"(x2), "v"(x3));
}
// the same into elements at .. at + 3 (at a multiple of 4) of the plane fragments (ph, pl)
__device__ __forceinline__ void split4_f16(const float (&x)[4], f16x8& ph, f16x8& pl, int at, float& amax) {
    unsigned h0, h1, l0, l1;
    split4_f16(x[0], x[1], x[2], x[3], h0, h1, l0, l1, amax);
    u32x4 hv = __builtin_bit_cast(u32x4, ph), lv = __builtin_bit_cast(u32x4, pl);
    hv[at / 2] = h0; hv[at / 2 + 1] = h1;
    lv[at / 2] = l0; lv[at / 2 + 1] = l1;
    ph = __builtin_bit_cast(f16x8, hv);
    pl = __builtin_bit_cast(f16x8, lv);
}

// Two values -> elements at, at + 1 (at even) of the plane fragments (ph, pl), |x| into the range maximum.
__device__ __forceinline__ void split2_f16(float x0, float x1, f16x8& ph, f16x8& pl, int at, float& amax) {
    unsigned hh, ll;
    asm volatile(
        "v_max3_f32 %2, %2, |%3|, |%4|\n\t"
        "v_cvt_pk_f16_f32 %0, %3, %4\n\t"
        "v_fma_mixlo_f16 %1, -%0, 1.0, %3 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %1, -%0, 1.0, %4 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
        : "=&v"(hh), "=&v"(ll), "+v"(amax)
        : "v"(x0), "v"(x1));
    u32x4 hv = __builtin_bit_cast(u32x4, ph), lv = __builtin_bit_cast(u32x4, pl);
    hv[at / 2] = hh;
    lv[at / 2] = ll;
    ph = __builtin_bit_cast(f16x8, hv);
    pl = __builtin_bit_cast(f16x8, lv);
}
// the same without the range maximum (bounded values such as probabilities, or a caller that takes the maximum itself)
__device__ __forceinline__ void split2_f16(float x0, float x1, f16x8& ph, f16x8& pl, int at) {
    unsigned hh, ll;
    asm volatile(
        "v_cvt_pk_f16_f32 %0, %2, %3\n\t"
        "v_fma_mixlo_f16 %1, -%0, 1.0, %2 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %1, -%0, 1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
        : "=&v"(hh), "=&v"(ll)
        : "v"(x0), "v"(x1));
    u32x4 hv = __builtin_bit_cast(u32x4, ph), lv = __builtin_bit_cast(u32x4, pl);
    hv[at / 2] = hh;
    lv[at / 2] = ll;
    ph = __builtin_bit_cast(f16x8, hv);
    pl = __builtin_bit_cast(f16x8, lv);
}

}  // namespace
