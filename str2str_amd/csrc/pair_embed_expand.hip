// Edge embedding, second half of the CLASS path: expand the class table of s2s_edge_embed_classes_f16x3 to the pair tensors.
//
// With one timestep per chunk and a 0/1 fixed mask, a pair's whole MLP input -- and with it z, attn_bias and pair_z before the edge
// mask -- depends only on its class (fixed_i, fixed_j, d, bin): csrc/edge_embed_f16.h ("TABLE") runs the MLP once per class row, and
// this kernel computes every pair's class exactly as the edge embedding does (edge_embed_class.h: the same device functions) and
// copies the row.  No matrix work, no weights: a wave owns a 32-pair block (16 KiB of z), reads its rows out of the cache -- the
// table is a few MB to a few tens of MB -- and writes 672 B per pair.
//   z         = row's z x (m_i m_j)   (the table holds z x 1.0, so the product is the edge embedding's own last multiply)
//   attn_bias, pair_z = the row's, or the projection bias where m_i m_j = 0 (what the projection of a zero vector gives);
//               the node mask must be 0/1 for the two projections (the caller's eligibility rule).
// Layouts as s2s_edge_embed_f16x3: z row-major [B,N,N,128] or tiled (a 32-pair block is [32 chunks of 4 channels][32 pairs][4]),
// attn_bias head-major [B,8,N,N], pair_z [B,N,N,32].  Every access is a whole-line 16 B-per-lane access except attn_bias (4 B per
// lane, 128 B runs, as in the edge embedding).  32-bit pair indices inside a launch; the entry point splits like s2s_edge_embed_f16x3.
// INDEX MODE (out_tiled = 2): z is not written at all.  `out` receives one int32 per pair in flat pair order, the pair's class row, or
// -1 where m_i m_j = 0, so that a consumer that reads record index + 1 of [a record of zeros | table] gets z x (m_i m_j) for a 0/1
// mask (s2s_edge_transition_f16x3, io_layout bit 3; the caller provides the zero record).  attn_bias and pair_z are written as in
// the other modes.
// RECORD SIZE: 168 floats whenever proj_bias_cat64 is given, also where the two projection outputs are not asked for (z alone out of a
// table that was built with the fused projection), else 128.
#include <hip/hip_runtime.h>

#include "edge_embed_class.h"
#include "pair_launch.h"
#include "str2str_hip.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <bool PROJ, bool REC168 = PROJ>
__global__ void __launch_bounds__(256) edge_embed_expand_kernel(
    const float* __restrict__ table, const int* __restrict__ fixed_cls, const float* __restrict__ bin_lower,
    const long long* __restrict__ residue_idx, const float* __restrict__ ca, const float* __restrict__ mask,
    const float* __restrict__ proj_b, float* __restrict__ out, float* __restrict__ attn_bias, float* __restrict__ pair_z,
    long long M, int N, int rel_off, int n_rel, int n_bins, int out_tiled) {
    constexpr unsigned kRec = REC168 ? s2s::kEeRecProj : s2s::kEeRecPlain;
    __shared__ __attribute__((aligned(16))) float s_bins[s2s::kEeBinSlots];
    const unsigned lane = threadIdx.x & 63, h = lane >> 5, wave = threadIdx.x >> 6;
    s2s::ee_fill_bins(s_bins, bin_lower, n_bins);
    __syncthreads();
    const long long p0 = ((long long)blockIdx.x * 4 + wave) * 32;   // this wave's 32-pair block
    if (p0 >= M) return;
    long long pl = p0 + (lane & 31);
    const bool valid = pl < M;
    pl = valid ? pl : M - 1;   // lanes past the end run on the last pair (the tiled buffer holds whole blocks)
    const unsigned p = (unsigned)pl;
    // p = (bb N + i) N + j:  global row bi = p / N,  j = p - bi N,  bb = bi / N
    const unsigned bi = p / (unsigned)N, j = p - bi * (unsigned)N, bb = bi / (unsigned)N, bj = bb * (unsigned)N + j;
    const int bin = s2s::ee_pair_bin(s_bins, n_bins, ca[bi * 3 + 0], ca[bi * 3 + 1], ca[bi * 3 + 2], ca[bj * 3 + 0], ca[bj * 3 + 1], ca[bj * 3 + 2]);
    const unsigned d = (unsigned)s2s::ee_rel_row(residue_idx[bi], residue_idx[bj], rel_off, n_rel);
    const unsigned row = s2s::ee_class_row((unsigned)fixed_cls[bi], (unsigned)fixed_cls[bj], d, bin, n_rel, n_bins);
    const float em = mask ? __fmul_rn(mask[bi], mask[bj]) : 1.0f;
    const float* rec = table + (unsigned long long)row * kRec;

    if (out_tiled == 2) {   // index mode: 4 B per pair, 128 B per wave
        if (valid && h == 0) reinterpret_cast<int*>(out)[p] = em == 0.f ? -1 : (int)row;
    } else if (out_tiled) {   // lane (pair n, half h) owns chunks 2g + h of its pair: the store of group g covers 1 KiB of the block
        float* o = out + (unsigned long long)(p0 >> 5) * 4096u + lane * 4u;
        f32x4 v[16];
#pragma unroll
        for (int g = 0; g < 16; ++g) v[g] = *reinterpret_cast<const f32x4*>(rec + 8 * g + 4 * h);
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const f32x4 w = {__fmul_rn(v[g].x, em), __fmul_rn(v[g].y, em), __fmul_rn(v[g].z, em), __fmul_rn(v[g].w, em)};
            __builtin_nontemporal_store(w, reinterpret_cast<f32x4*>(o + g * 256));
        }
    } else {           // half-wave h copies the 512 B row of pair 2 it + h: lane c of it moves channels 4c .. 4c+3
        const unsigned c = lane & 31;
        f32x4 v[16];
        float e[16];
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int n = 2 * it + (int)h;
            const unsigned rn = (unsigned)__shfl((int)row, n, 64);
            e[it] = __shfl(em, n, 64);
            v[it] = *reinterpret_cast<const f32x4*>(table + (unsigned long long)rn * kRec + 4 * c);
        }
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const long long pn = p0 + 2 * it + h;
            const f32x4 w = {__fmul_rn(v[it].x, e[it]), __fmul_rn(v[it].y, e[it]), __fmul_rn(v[it].z, e[it]), __fmul_rn(v[it].w, e[it])};
            if (pn < M) __builtin_nontemporal_store(w, reinterpret_cast<f32x4*>(out + (unsigned long long)pn * 128u + 4 * c));
        }
    }
    if constexpr (PROJ) {
        // attention bias, heads 4h .. 4h+3 of this lane's pair, head-major
        {
            f32x4 a = *reinterpret_cast<const f32x4*>(rec + 128 + 4 * h);
            const f32x4 b = *reinterpret_cast<const f32x4*>(proj_b + 4 * h);
            a = em == 0.f ? b : a;
            const long long NN = (long long)N * N;
            float* o = attn_bias + ((unsigned long long)p + 7ull * bb * (unsigned long long)NN + 4ull * h * (unsigned long long)NN);
            if (valid) { o[0] = a.x; o[NN] = a.y; o[2 * NN] = a.z; o[3 * NN] = a.w; }
        }
        // pair_z: 8 lanes per pair (128 B), 8 pairs per instruction
        const unsigned c = lane & 7;
        const f32x4 b = *reinterpret_cast<const f32x4*>(proj_b + 8 + 4 * c);
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int n = 8 * it + (int)(lane >> 3);
            const unsigned rn = (unsigned)__shfl((int)row, n, 64);
            const float en = __shfl(em, n, 64);
            f32x4 a = *reinterpret_cast<const f32x4*>(table + (unsigned long long)rn * kRec + 136 + 4 * c);
            a = en == 0.f ? b : a;
            const long long pn = p0 + n;
            if (pn < M) *reinterpret_cast<f32x4*>(pair_z + (unsigned long long)pn * 32u + 4 * c) = a;
        }
    }
}

}  // namespace

extern "C" int s2s_edge_embed_expand(const float* table, const int* fixed_cls, const float* bin_lower, const long long* residue_idx,
                                     const float* ca_xyz, const float* mask, const float* proj_bias_cat64, float* out, int out_tiled,
                                     float* proj_attn_bias, float* proj_pair_z, int n_samples, int n_res, int rel_offset, int n_rel,
                                     int n_bins, void* stream) {
    if (n_samples <= 0 || n_res <= 0) return 0;
    if (n_bins < 1 || n_bins > 32 || out_tiled < 0 || out_tiled > 2 || n_rel < 1) return (int)hipErrorInvalidValue;
    if ((proj_attn_bias != nullptr) != (proj_pair_z != nullptr) || (proj_attn_bias && !proj_bias_cat64)) return (int)hipErrorInvalidValue;
    // 32-bit pair indices inside a launch: the split of s2s_edge_embed_f16x3 (and its test hook)
    const long long NN = (long long)n_res * n_res;
    if (NN >= (1ll << 31)) return (int)hipErrorInvalidValue;
    const long long chunk = s2s::samples_per_launch("S2S_EE_MAX_PAIRS", (1ll << 31) - 1, NN, n_samples, out_tiled == 1);   // (mode 2 is the index tensor)
    if (chunk < 1) return (int)hipErrorInvalidValue;
    for (long long b0 = 0; b0 < n_samples; b0 += chunk) {
        const long long nb = n_samples - b0 < chunk ? n_samples - b0 : chunk;
        const long long M = nb * NN, rows0 = b0 * n_res;
        const unsigned grid = (unsigned)((M + 127) / 128);
        const float* mk = mask ? mask + rows0 : nullptr;
        float* o = out + (out_tiled == 2 ? b0 * NN : b0 * NN * 128);   // (index mode: one 4-byte word per pair)
        if (proj_attn_bias)
            hipLaunchKernelGGL(edge_embed_expand_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, table, fixed_cls + rows0,
                               bin_lower, residue_idx + rows0, ca_xyz + rows0 * 3, mk, proj_bias_cat64, o, proj_attn_bias + b0 * 8 * NN,
                               proj_pair_z + b0 * NN * 32, M, n_res, rel_offset, n_rel, n_bins, out_tiled);
        else if (proj_bias_cat64)   // z alone out of 168-float records
            hipLaunchKernelGGL((edge_embed_expand_kernel<false, true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, table, fixed_cls + rows0,
                               bin_lower, residue_idx + rows0, ca_xyz + rows0 * 3, mk, (const float*)nullptr, o, (float*)nullptr,
                               (float*)nullptr, M, n_res, rel_offset, n_rel, n_bins, out_tiled);
        else
            hipLaunchKernelGGL(edge_embed_expand_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, table, fixed_cls + rows0,
                               bin_lower, residue_idx + rows0, ca_xyz + rows0 * 3, mk, (const float*)nullptr, o, (float*)nullptr,
                               (float*)nullptr, M, n_res, rel_offset, n_rel, n_bins, out_tiled);
    }
    return (int)hipGetLastError();
}
