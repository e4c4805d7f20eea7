// EdgeTransition / edge embedding on split-f16 MFMA ("f16x3"): fp32-equivalent accuracy on the 16-bit matrix cores, the DEFAULT
// arithmetic of the pair stream.  Same operators and contracts as s2s_edge_transition / s2s_edge_embed (csrc/pair_mlp.hip, the
// exact fp32-MFMA kernels; reference EdgeTransition.forward, src/models/net/layers.py:170-185 + mask ipa.py:372, and
// EmbeddingModule.forward, denoising_ipa.py:137-158).
//
// Arithmetic.  Every fp32 operand is split into two f16 numbers  x = x_h + x_l (+ <= 2^-24 |x|),  x_h = rn16(x), x_l = rn16(x - x_h)
// -- 11 + 11 significant bits plus the sign of the residue, i.e. fp32's 24 -- and a product keeps  w_h x_h + w_h x_l + w_l x_h  (the
// dropped w_l x_l is below one fp32 rounding of the product) on v_mfma_f32_32x32x16_f16 with fp32 accumulation: 3 MFMAs per
// (k-step, tile).  f16's narrow exponent is handled by one exact power-of-two scaling: the weight side stores the split of 2^5 w,
// W_h = rn16(32 w), W_l = rn16(32 w - W_h)  (so that the small part stays in f16's normal range; 2 A fragments per (k-step, tile),
// 4 KiB per slot, 32 KiB stages, 0.94 MB stream), the activation side two plane registers x_h, x_l, and the accumulators carry
// 32 x the layer output: the factor 2^-5 rides in the multiply-add that adds the bias / seeds in every epilogue (LayerNorm, scale
// invariant, runs on the scaled values with 1024 eps).  A value of x_l below f16's normal range (|x| < 0.25) is rounded to 2^-25
// absolute -- 1.7e-8 rms on an O(1) output, under fp32's own rounding.
// RANGE: activations must stay below f16's 65504.  Every activation that is split here feeds a running maximum; a tile whose
// maximum reaches 2^15 (or is not finite) raises the caller's range flag (range_flag.h), and the sampler re-runs that chunk on the
// exact fp32 kernels (str2str_amd/sampler.py) -- an overflow is neither silent nor an error.  Weights with |32 w| >= 65504 are
// refused at pack time (ops.pack_f16x2_layer).
// This header: what both kernel templates (edge_transition_f16.h, edge_embed_f16.h) use; a .hip unit holds two instantiations.
#pragma once
#include <hip/hip_runtime.h>

#include "edge_embed_class.h"
#include "f16x3.h"
#include "range_flag.h"
#include "str2str_hip.h"

namespace {

constexpr int kStageBytes = 32 * 1024;  // 8 slots x 4 fragments x 1 KiB

// max(x, 0) as ONE instruction.  fmaxf() of a value the compiler cannot see through (a pinned register, an MFMA result) is preceded by
// a canonicalising v_max_f32 x, x (IEEE quieting of a signalling NaN): 128 of the edge embedding's ~1500 VALU instructions per tile.
// v_max_f32 itself returns the other operand for any NaN input, which is what the two-instruction form computes as well.
__device__ __forceinline__ float relu1(float x) {
    float r;
    asm("v_max_f32 %0, 0, %1" : "=v"(r) : "v"(x));
    return r;
}

}  // namespace

#define S2S_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
