// EdgeTransition on split-f16 MFMA: the kernel template and its launcher (arithmetic and range guard: pair_f16.h).
//
// Schedule.  One wave owns 32 pairs; the 4 waves of a workgroup share the weight stream (30 stages of 32 KiB through a ring of
// LDS buffers, see s_w).  A stage is 8 SLOTS of 6 MFMAs / 4 A fragments.  Per pair tile (240 slots):
//   A_t  (4 slots)  layer-1 output tile t (32 of the 384 hidden channels) over the 8 k-steps of the 128 edge channels;
//                   the edge row is split once into 8 x 2 f16 plane registers.
//   B_t  (12 slots) layer-2 k-steps 2t, 2t+1 (= the 32 channels of a1 tile t) into all 12 output tiles; the 192
//                   layer-2 accumulators stay resident, a1 is never materialised beyond two tiles.  B_11 runs tile-pair major
//                   (its first output tiles are complete early), every other B_t k-step major.
//   order: A_0 A_1 | B_0 A_2 | B_1 A_3 | ... | B_9 A_11 | B_10 B_11 | final layer (48 slots, k-step major) [| projection, 8 slots].
//   A slot = six MFMAs, each followed by at most one 1 KiB piece of the weight pipe and one small VALU piece, pinned there by
//   sched_barrier (the slot body in the kernel has the table).  Found with an in-kernel timeline probe (profiles/
//   r04a_et_phase_probe.txt): a slot of bare MFMAs runs at the matrix pipe's 192 cycles; the four loads / four LDS stores of the
//   weight pipe issued as a block cost 60 / 120 cycles, a 20-instruction VALU block behind one MFMA ~100.  So:
//     - the ReLU + per-node seeds + split of a1 tile t-1 runs in 2-value halves behind MFMAs 2 and 4 of the A_t slots;
//     - the layer-2 epilogue (ReLU + residual + split = the final layer's input) runs in 4-value pieces: block 0 under the second
//       half of B_11, block 1 under the final layer's k-steps 0..7 into a second plane buffer, block 2 under k-steps 8..15;
//     - the next tile's edge row is requested two loads per slot over two stages (a 16-load burst held its slot for 2.4 k cycles) and
//       split in halves under the last final-layer block; its per-node seeds a quarter behind each of four MFMAs;
//     - what stays exposed: tile 11 of layer 1 -> planes (0.4 k cycles) and LayerNorm + store (5.2 k of a tile's 78 k).
//   Every activation is split exactly once.  C->B chaining as in pair_mlp.hip: element j of lane (pair, g) in k-step 2t'+u is
//   accumulator register 8u+j of tile t' (row 32t' + (r&3) + 8(r>>2) + 4g); the host packs A fragments in that k order and in the
//   slot order above (ops.pack_f16x3_stream; part of the ABI version).
//   Weight pipe: this wave's quarter of the next stage travels global -> VGPR -> LDS in two halves, each loaded (buffer
//   loads: SGPR base + constant lane offset) five slots before it is stored; the workgroup barrier sits at the top
//   of the last slot of a stage, after which the next stage's first fragments are fetched one slot ahead.
//   Workgroups are persistent (one per CU).  With the fused projection (PROJ) the stream has a 31st stage and the two LDS buffers
//   swap roles after every tile (odd stage count).
// Pair-tensor layouts: row-major [B,N,N,128] (the reference's) or TILED on either side (include/str2str_hip.h): a lane owns one pair,
//   so on row-major rows every load / store instruction touches 32 B in each of 32 cache lines; tiled, 8 whole lines.  The last
//   EdgeTransition of a trunk writes no pair tensor at all (io_layout bit 2).
#pragma once
#include "pair_f16.h"
#include "pair_launch.h"

namespace s2s {

// the arguments of s2s_edge_transition_f16x3 (include/str2str_hip.h) in its order, filled once by the public entry point
struct EtArgs {
    const float *edge, *node_ab, *node_p;  const void* weight_stream;
    const float *b2, *ln_gamma, *ln_beta, *mask;  float* out;
    int n_samples, n_res;  float ln_eps;  int io_layout;
    const float* proj_bias_cat64;  float *proj_attn_bias, *proj_pair_z;
    int prescale_exp;  int* range_words;  void* stream;
};
// Inside the library only, each in its own translation unit (two instantiations of the kernel per unit):
// chains below 32 residues: a 32-pair tile spans more than two rows, the row seeds stay per-lane loads
__attribute__((visibility("hidden"))) int et_f16x3_short_chains(const EtArgs& a);
// the first EdgeTransition behind the class path of the edge embedding: edge rows read by class (io_layout bit 3)
__attribute__((visibility("hidden"))) int et_f16x3_by_class(const EtArgs& a);

}  // namespace s2s

namespace {

constexpr int kStagesBase = 30;         // + 1 stage (8 slots) for the fused pair projection of the next IPA block
constexpr int kClsSlot = 200;           // BYCLS: the schedule slot that requests the next tile's class indices (one HBM round trip ahead of slot kXv0 + 1)

// slot s of the schedule: phase 0 = A (layer 1), 1 = B (layer 2), 2 = F (final layer)
struct SlotDesc { int phase, t, a, b; };  // A: tile t, a = k-step pair 0..3;  B: tile t, a = u (k-step 2t+u), b = tile pair 0..5 (B_11: pair-major);
                                          // F: a = k-step 0..23, b = tile pair 0..1
constexpr SlotDesc slot_desc(int s) {
    if (s < 8) return {0, s / 4, s % 4, 0};
    if (s < 168) {
        const int tau = s - 8, blk = tau / 16, o = tau % 16;
        if (o < 12) return {1, blk, o / 6, o % 6};
        return {0, blk + 2, o - 12, 0};
    }
    if (s < 180) return {1, 10, (s - 168) / 6, (s - 168) % 6};
    if (s < 192) return {1, 11, (s - 180) % 2, (s - 180) / 2};   // B_11 tile-pair major: output tiles 2b, 2b+1 are complete after slot 181 + 2b

    if (s < 240) return {2, 0, (s - 192) / 2, (s - 192) % 2};
    return {3, 0, s - 240, 0};  // P: fused projection k-step s - 240 (both output tiles)
}
// ROTATED TILE LOOP (round 4).  LayerNorm + store and the fused projection of tile n run under / after the first two layer-1 tiles
// of tile n + 1:  A_0 A_1 (+ LayerNorm of the previous tile in pieces behind their MFMAs) | P (projection of the previous tile) |
// B_0 A_2 | ... | F.  The kernel's slot position ns (weight-pipe stage ns / 8) maps to the schedule slot s above; the weight
// stream keeps the host's order (projection stage last): logical stage 1 of a PROJ stream is blob stage 30.
constexpr int sched_slot(bool proj, int ns) { return !proj ? ns : (ns < 8 ? ns : (ns < 16 ? 240 + (ns - 8) : ns - 8)); }
constexpr int blob_stage(bool proj, int st) { return !proj ? st : (st == 0 ? 0 : (st == 1 ? 30 : st - 1)); }

__device__ float s2s_one[1] = {1.0f};   // stands in for an absent node mask (read with stride 0)

// PROJ: also emit the NEXT IPA block's linear_b / down_z (ipa.py:177,253) of the pair vector just produced -- one more
// weight stage (64 x 128 Wcat, chain-packed), 8 more slots on the LayerNorm output while it is still in registers,
// attention bias written head-major [B,8,N,N], pair_z [B,N,N,32].  Saves the 512 B/pair re-read of z by s2s_pair_project.
// BYCLS (io_layout bit 3; the first EdgeTransition behind the edge embedding's class path): `edge` is not a pair tensor but the records of
// the class table, record 0 all zero and class r at record r + 1, and `cls_idx` holds one int32 per pair, its class or -1 where the edge
// mask is zero (s2s_edge_embed_expand, index mode).  A lane reads its pair's z[128] straight out of its record: the same 16 B groups at
// a stride of 8 floats as a row-major edge row, from a table that stays in the L2 instead of a pair tensor from HBM.
template <bool PROJ, bool STAGE, bool BYCLS = false>
__global__ void __launch_bounds__(256) edge_transition_f16_kernel(
    const float* __restrict__ edge, const float* __restrict__ node_ab, const float* __restrict__ node_p,
    const char* __restrict__ wblob, const float* __restrict__ b2,
    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mask,
    float* __restrict__ out, long long M, int N, float ln_eps, int io_layout, unsigned mask_stride, const float* __restrict__ proj_b,
    float* __restrict__ proj_bias_out, float* __restrict__ proj_pz_out, int* __restrict__ range_flag, float sk,
    const int* __restrict__ cls_idx) {
    constexpr int kStages = kStagesBase + (PROJ ? 1 : 0);
    constexpr int kSlots = 8 * kStages;
    // Weight stages in LDS.  PROJ (31 stages, every launch of the sampler): a RING of four 32 KiB buffers, stage x in buffer x & 3, the
    // weight pipe TWO stages ahead (stage x is stored during stage x - 2), and a workgroup barrier only in front of the even stages
    // (+ stage 29, where the odd stage count breaks the period: stages 29 30 | 0 1 of the next tile sit in buffers 1 2 | 0 1) --
    // 17 barriers per tile instead of 31.  A buffer is rewritten two stages after its last read and read two stages after its last
    // write, and with no two consecutive stage boundaries without a barrier there is one in between both times.  (Same-call A/Bs,
    // profiles/r05_et_barrier_ab.txt: every second barrier skipped, results aside, -1.45 % per launch; this ring -0.4 .. -0.8 %.)  Without the projection (30 stages;
    // stand-alone callers): two buffers, one stage ahead, a barrier per stage, as before.
    constexpr int kRing = PROJ ? 4 : 2, kAhead = PROJ ? 2 : 1;
    __shared__ __attribute__((aligned(16))) char s_w[kRing][kStageBytes];
    __shared__ __attribute__((aligned(16))) float s_vec[768 + 64];  // b2 | bf | gamma | beta | projection bias
    // STAGE (chains of 32+ residues): the two rows A_i (+ b1) of node_ab a wave's tile can touch, staged per tile (see stage_rows below)
    __shared__ __attribute__((aligned(16))) float s_rows[STAGE ? 4 * 2 * 384 : 4];
    const int lane = threadIdx.x & 63, h = lane >> 5, wave = threadIdx.x >> 6;

    // ---- weight pipe (see header).  Each wave moves one contiguous 12 KiB of every stage.
    const unsigned voff = wave * 8192 + lane * 16;
    typedef __attribute__((address_space(3))) char lds_char;
    // two base registers (a DS instruction's immediate offset has 16 bits): buffers (0, 1) and (2, 3) of the ring, or the two buffers
    lds_char* lds_image[2] = {(lds_char*)&s_w[0][lane * 16], (lds_char*)&s_w[kRing / 2][lane * 16]};
    asm volatile("" : "+v"(lds_image[0]), "+v"(lds_image[1]));  // opaque: every LDS access = base register + immediate
    auto ring_buf = [&](int r) -> lds_char* { return PROJ ? lds_image[r >> 1] + (r & 1) * kStageBytes : lds_image[r]; };   // r: compile-time at every call site
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)wblob, 0, kStages * kStageBytes, 0x00020000);
    auto ldw = [&](unsigned vo, int so) -> f32x4 {
        const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, vo, so, 0);
        return f32x4{__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w)};
    };
    // scalars on purpose: an array captured by the lambdas is demoted to memory by hipcc
    f32x4 c0, c1, c2, c3;  // staging group A (first half of the quarter)
    f32x4 e0, e1, e2, e3;  // staging group B (second half)
    typedef __attribute__((address_space(3))) f32x4 lds_f4;
    auto cp_load_a = [&](int stage) {
        const int so = blob_stage(PROJ, stage) * kStageBytes;  // compile-time at every call site
        c0 = ldw(voff, so); c1 = ldw(voff + 1024, so); c2 = ldw(voff + 2048, so); c3 = ldw(voff + 3072, so);
    };
    auto cp_load_b = [&](int stage) {
        const int so = blob_stage(PROJ, stage) * kStageBytes + 4096;
        e0 = ldw(voff, so); e1 = ldw(voff + 1024, so); e2 = ldw(voff + 2048, so); e3 = ldw(voff + 3072, so);
    };
    auto cp_store_a = [&](int par) {
        lds_char* d = ring_buf(par) + wave * 8192;
        *(lds_f4*)(d) = c0; *(lds_f4*)(d + 1024) = c1; *(lds_f4*)(d + 2048) = c2; *(lds_f4*)(d + 3072) = c3;
    };
    auto cp_store_b = [&](int par) {
        lds_char* d = ring_buf(par) + (wave * 8192 + 4096);
        *(lds_f4*)(d) = e0; *(lds_f4*)(d + 1024) = e1; *(lds_f4*)(d + 2048) = e2; *(lds_f4*)(d + 3072) = e3;
    };
    // the same, one 1 KiB piece at a time (k = 0..3): inside the tile loop a piece rides behind a single MFMA
    auto cp_load_piece = [&](auto grp, auto kc, int stage) {
        constexpr int k = decltype(kc)::value;
        const int so = blob_stage(PROJ, stage) * kStageBytes + (decltype(grp)::value ? 4096 : 0);
        const f32x4 v = ldw(voff + 1024 * k, so);
        if constexpr (decltype(grp)::value == 0) {
            if constexpr (k == 0) c0 = v; else if constexpr (k == 1) c1 = v; else if constexpr (k == 2) c2 = v; else c3 = v;
        } else {
            if constexpr (k == 0) e0 = v; else if constexpr (k == 1) e1 = v; else if constexpr (k == 2) e2 = v; else e3 = v;
        }
    };
    auto cp_store_piece = [&](auto grp, auto kc, int par) {
        constexpr int k = decltype(kc)::value;
        lds_char* d = ring_buf(par) + (wave * 8192 + (decltype(grp)::value ? 4096 : 0) + 1024 * k);
        if constexpr (decltype(grp)::value == 0)
            *(lds_f4*)(d) = k == 0 ? c0 : (k == 1 ? c1 : (k == 2 ? c2 : c3));
        else
            *(lds_f4*)(d) = k == 0 ? e0 : (k == 1 ? e1 : (k == 2 ? e2 : e3));
    };
    cp_load_a(0);
    cp_load_b(0);

    // ---- persistent workgroup: tiles of 128 pairs (32 per wave) blockIdx.x, blockIdx.x + gridDim.x, ...
    // Per-pair context as four 32-bit indices (the launcher keeps 8 M below 2^32): the row pointers are re-formed where they are
    // used (one v_mad_u64_u32 each) instead of living in twelve address registers through the whole tile -- this kernel sits at the
    // 512-register limit, and one more long-lived VGPR costs hundreds of spills.
    struct PairCtx {
        unsigned p, bi, bj, boff;  // flat pair index; flat node rows of i and j; offset of head 0 of this pair in a head-major [B,8,N,N] tensor
        unsigned r0, aoff;         // STAGE: the tile's first node row (wave-uniform), this lane's byte offset of its row's 16 B groups in s_rows
        float em_i, em_j;          // the two node masks, multiplied where the edge mask is used: a product formed here would wait
        bool valid;                // for the loads (vmcnt(0): the whole weight pipe) in the middle of the final layer
    };
    const unsigned NNu = (unsigned)N * (unsigned)N;
    const long long NN = (long long)N * N;
    // division by N through floor(2^32 / N) (quotient short by at most one for x < 2^31; a 64-bit division is ~100 VALU instructions)
    const unsigned n_magic = N >= 2 ? (unsigned)((1ull << 32) / (unsigned)N) : 0u;
    auto div_n = [&](unsigned x, unsigned& q, unsigned& r) {
        q = N >= 2 ? __umulhi(x, n_magic) : x;
        r = x - q * (unsigned)N;
        const bool fix = r >= (unsigned)N;
        q = fix ? q + 1 : q;
        r = fix ? r - (unsigned)N : r;
    };
    auto setup = [&](long long wg_tile) -> PairCtx {
        long long pl = (wg_tile * 4 + wave) * 32 + (lane & 31);
        PairCtx c;
        c.valid = pl < M;
        if (!c.valid) pl = M - 1;  // waves / lanes past the end run on the last pair and store nothing
        const unsigned p = (unsigned)pl;
        // p = (bb N + i) N + j:  flat row bi = p / N,  j = p - bi N,  bb = bi / N
        unsigned bi, j, bb, i;
        div_n(p, bi, j);
        div_n(bi, bb, i);
        c.p = p;
        c.bi = bi;
        c.bj = bb * (unsigned)N + j;
        c.r0 = (unsigned)__builtin_amdgcn_readfirstlane((int)bi);   // consecutive pairs of a chain of 32+ residues: rows r0 and r0 + 1 at most
        c.aoff = (unsigned)wave * 3072u + (bi != c.r0 ? 1536u : 0u) + 16u * (unsigned)h;
        c.boff = p + 7u * bb * NNu;
        // (no branch on the mask's presence: a value merged from two paths is materialised -- and waited for -- at the join;
        //  the launcher passes a one-element "1.0" and stride 0 for an absent mask)
        c.em_i = mask[bi * mask_stride];
        c.em_j = mask[c.bj * mask_stride];
        return c;
    };
    // The 32 pair rows of a wave are one 16 KiB block of z in either layout (header, "Pair-tensor layouts"): row-major, a lane's
    // 16 B group g sits at  n 512 + g 32 + h 16  of the block; tiled, at  g 1024 + lane 16  -- a load / store instruction of the wave
    // then covers 8 whole cache lines instead of 32 B of 32 lines.  (p & 31, not lane & 31: a clamped lane re-reads the last pair.)
    const bool in_tiled = io_layout & 1, out_tiled = io_layout & 2, no_out = io_layout & 4;
    const int in_step = in_tiled ? 256 : 8, out_step = out_tiled ? 256 : 8;   // floats between a lane's consecutive 16 B groups
    auto row_of = [&](const float* base, unsigned p, bool tiled) -> const float* {
        const unsigned blk = tiled ? p >> 5 : p, mul = tiled ? 4096u : 128u;
        const unsigned in_blk = tiled ? ((lane & 32) + (p & 31)) * 4 : 4 * h;
        return base + ((unsigned long long)blk * mul + in_blk);
    };
    auto erow_of = [&](const PairCtx& c) -> const float* { return row_of(edge, c.p, in_tiled); };
    // The pair stream is NON-TEMPORAL (round 6): every edge row is read once and every output row written once per launch (4.3 GB each way at
    // cfg2), and as ordinary accesses they push the 0.97 MB weight stream -- which all 32 workgroups of an XCD re-read every tile -- out of the
    // 4 MiB L2 between two uses (the re-fetches from the Infinity Cache showed in FETCH_SIZE: 378 instead of 301 B per pair).  With the nt bit
    // on the row loads and the output stores: -0.5 .. -1.2 % per launch at every shape measured (same-call A/B, profiles/r06_et_nt_ab.txt;
    // loads alone -0.4 %; nt on the fused projection's stores as well: no further gain, not kept).
    auto ldrow = [&](const float* r, int g) -> float4 {
        const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(r + g * in_step));
        return make_float4(v.x, v.y, v.z, v.w);
    };
    // BYCLS: a pair's row as ONE 32-bit byte offset into the records (below 4 GB by the CALLER's rule, see the header: the row count is
    // not known here): record cls + 1, this lane's
    // half.  The loads are base (scalar) + offset (one register) + immediate; the class index itself lives from its load to the offset.
    // Table rows are plain loads: they are re-read from the L2 by every tile that meets the class (nt measured, profiles/r08_et_by_class_stop_rule.md).
    const unsigned cls_rec = (io_layout & 16) ? s2s::kEeRecProj : s2s::kEeRecPlain;
    auto cls_pair = [&](long long wg_tile) -> unsigned {   // flat pair of this lane in tile wg_tile, clamped like setup()
        const unsigned p = ((unsigned)wg_tile * 4u + (unsigned)wave) * 32u + ((unsigned)lane & 31u);
        return p < (unsigned)M ? p : (unsigned)M - 1u;
    };
    auto cls_off = [&](int cls) -> unsigned { return ((unsigned)(cls + 1) * cls_rec + 4u * (unsigned)h) * 4u; };
    auto ldrow_cls = [&](unsigned off, int g) -> float4 {
        const f32x4* q = reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(edge) + off + 32 * g);
        const f32x4 v = *q;
        return make_float4(v.x, v.y, v.z, v.w);
    };
    const long long n_wt = (M + 127) / 128;
    long long wt = blockIdx.x;
    // (No phase stagger between workgroups: each requests its next edge row 16+ slots ahead of its use (kXv0 below), so running in
    //  lockstep costs no time, while a start delay would add to every launch: profiles/r04t_et_phase_stagger_ab.txt.)
    PairCtx cur = setup(wt);

    // ---- the pair's 128 edge channels, split once: xpl[ks][plane] = B operand of layer-1 k-step ks.  Element j of k-step
    //      2t+u is channel 32t + 8(2u + (j>>2)) + 4h + (j&3): the accumulator layout of a 128-channel block (register 8u+j of
    //      tile t), so the exact sum of the three planes later serves as the residual row of block 0 without a second read.
    f16x8 xpl[8][2];
    float amax = 0.f;   // range guard (range_flag.h): running maximum of every value that is split into f16 planes
    // Block exponent of the hidden activations (sk = 2^-prescale_exp, 1 by default): the planes of h1 = relu(layer 1) and of
    // relu(layer 2) + x hold sk x the value -- relu is positively homogeneous, so the factor rides in constants that exist anyway
    // (layer 1: (acc + 32 B_j) * (sk / 32) + sk A_i, the caller hands node_ab in as [sk A_i | 32 B_j | 32 sk G_j]; layer 2: relu(acc / 32 + sk b2) + sk x; final
    // layer: the per-node start value 32 sk G_j, which carries the bias b_f) and LayerNorm removes it (eps scaled alike).  Exact for powers of two; sk = 1 gives today's bits.
    const float inv1 = kInvWS * sk;
    // planes (x_h, x_l), see the header
    auto split4 = [&](const float (&x)[4], f16x8& ph, f16x8& pm, int at) {
        split4_f16(x, ph, pm, at, amax);
    };
    {
        float4 xv[16];
        if constexpr (BYCLS) {
            const unsigned off = cls_off(cls_idx[cur.p]);
#pragma unroll
            for (int i = 0; i < 16; ++i) xv[i] = ldrow_cls(off, i);
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) xv[i] = ldrow(erow_of(cur), i);  // accumulator ("chain") channel order, see xpl
        }
        for (int i = threadIdx.x; i < 768; i += 256)
            s_vec[i] = i < 384 ? sk * b2[i] : (i < 512 ? 0.f : (i < 640 ? gamma[i - 512] : beta[i - 640]));   // (384..511 unused: bf rides in the per-node start values G_j)
        if (PROJ && threadIdx.x < 64) s_vec[768 + threadIdx.x] = proj_b[threadIdx.x];
        cp_store_a(0);
        cp_load_a(1);
        cp_store_b(0);
        if constexpr (kAhead == 2) {   // the ring starts with stages 0 and 1 in LDS and the first half of stage 2 on its way
            cp_load_b(1);
            cp_store_a(1);
            cp_load_a(2);
            cp_store_b(1);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float x[4] = {xv[i].x, xv[i].y, xv[i].z, xv[i].w};
            split4(x, xpl[i >> 1][0], xpl[i >> 1][1], 4 * (i & 1));
        }
    }

    f32x16 a1t[2];     // layer-1 tiles t (even / odd)
    f32x16 a2[12];     // layer-2 accumulators, then relu(.)+residual = the final layer's input
    f32x16 a3[4];
    f32x16 pq[2];      // fused projection accumulators (64 padded output rows)
    float sa[16];  // per-node seeds A_i(+b1) of the a1 tile that is split next (the j-side seeds B_j start the tile's accumulators: seedc_piece)
    // quarter rq of the seeds of tile t (C layout: register 4rq + e = channel 32t + 8rq + 4h + e): A_i + b1 (384 channels) and B_j of
    // the per-node first-layer halves [B,N,768].  (The j-side rows differ from lane to lane -- 16 B in each of 32 rows per load
    // instruction.  Reading them from a column-blocked copy [B][96][N][4], 8 cache lines per instruction as in the edge embedding,
    // was measured: 2 % fewer cycles in the layer-2 blocks, no change in launch time; not worth a second copy of the node vectors.)
    // The row seeds A_i are the same for every pair of a row: 32 consecutive pairs of a chain of 32+ residues touch two rows at most, and
    // a wave used to fetch them with 48 load instructions per tile whose 64 lanes ask for one or two addresses -- the kernel without those
    // loads ran 2.2 % faster (tile 0's seeds for all tiles; timing only).  STAGE: the tile's rows r0, r0 + 1 (2 x 1536 B) go through LDS,
    // three contiguous 1 KiB loads + three LDS stores per wave and tile (stage_load / stage_store: requested right after the next tile's
    // setup, stored five slots later, first read 20+ slots after that; this tile's last read is ~40 slots before the store -- one
    // private region per wave, LDS operations of a wave are in order: no barrier), and a quarter of seeds is one ds_read_b128.
    f32x4 g_st0, g_st1, g_st2;   // staging registers of the row copy
    const unsigned n_node_rows = (unsigned)(M / N);
    auto stage_load = [&](const PairCtx& c) {
        if constexpr (STAGE) {
            const unsigned r1 = c.r0 + 1 < n_node_rows ? c.r0 + 1 : c.r0;
            auto piece = [&](int k) -> f32x4 {
                const unsigned o = (unsigned)k * 1024u + 16u * (unsigned)lane;   // byte o of [row r0 | row r1]
                const bool second = o >= 1536u;
                const float* src = node_ab + (unsigned long long)(second ? r1 : c.r0) * 896u + ((second ? o - 1536u : o) >> 2);
                const float4 v = *reinterpret_cast<const float4*>(src);
                return f32x4{v.x, v.y, v.z, v.w};
            };
            g_st0 = piece(0); g_st1 = piece(1); g_st2 = piece(2);
        }
    };
    auto stage_store = [&]() {
        if constexpr (STAGE) {
            typedef __attribute__((address_space(3))) f32x4 lds_v4;
            lds_v4* d = (lds_v4*)((__attribute__((address_space(3))) char*)s_rows + wave * 3072 + lane * 16);
            d[0] = g_st0; d[64] = g_st1; d[128] = g_st2;
        }
    };
    auto seeds_piece = [&](const PairCtx& c, int t, int rq) {
        if constexpr (STAGE) {
            const f32x4 x = *(const lds_f4*)((__attribute__((address_space(3))) const char*)s_rows + c.aoff + (32 * t + 8 * rq) * 4);
            sa[4 * rq + 0] = x[0]; sa[4 * rq + 1] = x[1]; sa[4 * rq + 2] = x[2]; sa[4 * rq + 3] = x[3];
        } else {
            const float4 x = ldg4(node_ab + (unsigned long long)c.bi * 896u + 32 * t, rq, h);
            sa[4 * rq + 0] = x.x; sa[4 * rq + 1] = x.y; sa[4 * rq + 2] = x.z; sa[4 * rq + 3] = x.w;
        }
    };
    // The j-side seeds are the START VALUE of the layer-1 accumulators (round 5): the caller hands the second half of node_ab in as
    // 32 B_j -- the accumulators' scale -- and quarter rq of tile t is loaded straight into the accumulator registers of a1t[t & 1]
    // (dead from the split of tile t - 2 on; hipcc loads into the accumulator file directly), so that the tile's first product lands
    // on it and the epilogue is relu(acc (sk / 32) + sk A_i): one add per hidden value less (-208 VALU instructions per tile on the
    // ISA, -0.5 % per launch in a same-call A/B).
    auto seedc_piece = [&](const PairCtx& c, int t, int rq) {
        const float4 y = ldg4(node_ab + (unsigned long long)c.bj * 896u + 384 + 32 * t, rq, h);
        a1t[t & 1][4 * rq + 0] = y.x; a1t[t & 1][4 * rq + 1] = y.y; a1t[t & 1][4 * rq + 2] = y.z; a1t[t & 1][4 * rq + 3] = y.w;
    };
    auto seeds_load = [&](const PairCtx& c, int t) {
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) seeds_piece(c, t, rq);
    };
    stage_load(cur);
    stage_store();
    seeds_load(cur, 0);
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) { seedc_piece(cur, 0, rq); seedc_piece(cur, 1, rq); }

    f16x8 fr[2][4];  // A fragments of the current / next slot: (W_h, W_l) of two (k-step, tile) units
    f16x8 xp[2][2];  // layer 2: planes of k-steps 2t, 2t+1 of the current a1 tile; final layer: current / next k-step
    auto fetch = [&](int par, int slot_in_stage, f16x8 (&f)[4]) {
        typedef __attribute__((address_space(3))) f16x8 lds_frag;
        const lds_frag* s = (const lds_frag*)ring_buf(par) + slot_in_stage * 4 * 64;
        // fragment 1 (W_l of the first unit) is what a slot's FIRST MFMA reads: requested last, the wait in front of that MFMA covers all
        // four reads (LDS returns in order) and the slot's other MFMAs need none -- one s_waitcnt per slot instead of two or three
        // (profiles/r05l_et_waitcnt_ab.txt)
        f[0] = s[0]; f[2] = s[128]; f[3] = s[192]; f[1] = s[64];
    };
    // quarter qd (registers 4qd..4qd+3) of  relu(a1 tile + seeds)  -> planes of k-step qd>>1, elements 4(qd&1)..
    auto s_quarter = [&](const f32x16& tile_acc, auto qc) {
        constexpr int qd = decltype(qc)::value;
        float x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = fmaxf(__builtin_fmaf(tile_acc[4 * qd + j], inv1, sa[4 * qd + j]), 0.f);
        split4(x, xp[qd >> 1][0], xp[qd >> 1][1], 4 * (qd & 1));
    };
    // the same in two halves (values 2hh, 2hh+1 of the quarter): 10 VALU instructions, small enough to sit behind one MFMA
    auto s_half = [&](const f32x16& tile_acc, auto qc, auto hc) {
        constexpr int qd = decltype(qc)::value, j0 = 4 * qd + 2 * decltype(hc)::value;
        const float x0 = fmaxf(__builtin_fmaf(tile_acc[j0], inv1, sa[j0]), 0.f);
        const float x1 = fmaxf(__builtin_fmaf(tile_acc[j0 + 1], inv1, sa[j0 + 1]), 0.f);
        split2_f16(x0, x1, xp[qd >> 1][0], xp[qd >> 1][1], 4 * (qd & 1) + 2 * decltype(hc)::value, amax);
    };
    // residual rows n'_i (block 1) and n'_j (block 2) of  x = [e | n'_i | n'_j]  in accumulator layout, two 16 B groups per call
    float rs[64];
    auto row_load2 = [&](const float* r, float (&dst)[64], int g0) {
#pragma unroll
        for (int g = g0; g < g0 + 2; ++g) {
            const float4 v = ldg4(r, g, h);
            dst[4 * g + 0] = v.x; dst[4 * g + 1] = v.y; dst[4 * g + 2] = v.z; dst[4 * g + 3] = v.w;
        }
    };
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    S2S_LDS_BARRIER();  // stage 0 and s_vec are in LDS
    fetch(0, 0, fr[0]);

    // ---- LayerNorm(128) over the pair's channels (half here, half in lane ^ 32), + bf, edge mask, store -- of the PREVIOUS tile,
    //      cut into pieces that ride behind the MFMAs of this tile's first eight slots (rotated tile loop: sched_slot above).  The
    //      arithmetic and its order are those of a plain epilogue: bias, running sum and running sum of squared deviations over the
    //      lane's 64 channels in accumulator order, ((a - mean) rstd) gamma + beta, mask.  (LayerNorm is scale invariant: the
    //      statistics run on the 32 x scaled accumulator, with 1024 eps.)
    PairCtx prv = cur;   // the tile whose final-layer accumulators a3 holds; none before the first tile (nothing is stored, and
    prv.valid = false;   // a zero mask keeps the idle pass out of the range maximum)
    prv.em_i = 0.f;
    float ln_sum = 0.f, ln_var = 0.f, ln_mean = 0.f, ln_rstd = 0.f, ln_em = 0.f;
    float* ln_orow = out;
    f16x8 xln[8][2];     // PROJ: planes of the LayerNorm output = B operands of the projection k-steps (chain order)
    auto ln_add = [&](auto qc) {   // piece q = (tile t, quarter rq): running sum (bf is the accumulators' start value, slots 192 / 193)
        constexpr int q = decltype(qc)::value, t = q / 4, rq = q % 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) ln_sum += a3[t][4 * rq + j];
    };
    auto ln_dev = [&](auto qc) {
        constexpr int q = decltype(qc)::value, t = q / 4, rq = q % 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float dd = a3[t][4 * rq + j] - ln_mean;
            ln_var += dd * dd;
        }
    };
    // normalise + mask + store [+ PROJ: planes of projection k-step q / 2]; a3 is only read (a value written back into an
    // accumulator tuple drags the whole 16-register tuple into the VALU's half of the register file)
    auto ln_out = [&](auto qc, const float4& ga, const float4& be) {
        constexpr int q = decltype(qc)::value, t = q / 4, rq = q % 4;
        float4 o;
        o.x = ((a3[t][4 * rq + 0] - ln_mean) * ln_rstd * ga.x + be.x) * ln_em;
        o.y = ((a3[t][4 * rq + 1] - ln_mean) * ln_rstd * ga.y + be.y) * ln_em;
        o.z = ((a3[t][4 * rq + 2] - ln_mean) * ln_rstd * ga.z + be.z) * ln_em;
        o.w = ((a3[t][4 * rq + 3] - ln_mean) * ln_rstd * ga.w + be.w) * ln_em;
        if (prv.valid && !no_out) {
            __builtin_nontemporal_store(f32x4{o.x, o.y, o.z, o.w}, reinterpret_cast<f32x4*>(ln_orow + q * out_step));
        }
        if constexpr (PROJ) {
            const float x[4] = {o.x, o.y, o.z, o.w};
            split4(x, xln[2 * t + (rq >> 1)][0], xln[2 * t + (rq >> 1)][1], 4 * (rq & 1));
        }
    };
    // PROJ: rows 0..7 (+ bias) -> attention bias, head-major; rows 8..39 -> pair_z channel row - 8 (same map as pair_mlp.hip); group g of 5
    auto proj_store = [&](auto gc) {
        constexpr int g = decltype(gc)::value;
        if (prv.valid) {
            const float4 bq = ldg4(s_vec + 768, g, h);
            if constexpr (g == 0) {
                float* o = proj_bias_out + ((unsigned long long)prv.boff + 4 * h * NN);
                o[0] = __builtin_fmaf(pq[0][0], kInvWS, bq.x);
                o[NN] = __builtin_fmaf(pq[0][1], kInvWS, bq.y);
                o[2 * NN] = __builtin_fmaf(pq[0][2], kInvWS, bq.z);
                o[3 * NN] = __builtin_fmaf(pq[0][3], kInvWS, bq.w);
            } else {
                constexpr int t = g >> 2, rq = g & 3;
                *reinterpret_cast<float4*>(proj_pz_out + (unsigned long long)prv.p * 32u + 8 * (g - 1) + 4 * h) =
                    make_float4(__builtin_fmaf(pq[t][4 * rq + 0], kInvWS, bq.x), __builtin_fmaf(pq[t][4 * rq + 1], kInvWS, bq.y),
                                __builtin_fmaf(pq[t][4 * rq + 2], kInvWS, bq.z), __builtin_fmaf(pq[t][4 * rq + 3], kInvWS, bq.w));
            }
        }
    };
#pragma unroll
    for (int t = 0; t < 4; ++t) a3[t] = zero16;

    constexpr int kHead = PROJ ? 16 : 15;  // slots that still work for the previous tile: A_0 A_1 + its projection (PROJ) or the first seven slots of B_0
    long long wt_next = wt;
    bool has_next = false;
    PairCtx nxt = cur;  // next tile's context, edge row and planes: produced under the last 16 slots of this tile
    float4 xv[16];
    unsigned ncls = 0;   // BYCLS: the next tile's class index (from slot kClsSlot), then its row offset (from slot kXv0 + 1)
    f16x8 xpn[8][2];
    f16x8 xq[8][2];   // final-layer input planes of k-steps 8..15 (block 1 of the layer-2 epilogue)
    auto slot = [&](auto sc) {
        constexpr int ns = decltype(sc)::value;      // position in the tile loop: weight-pipe stage ns / 8
        constexpr int s = sched_slot(PROJ, ns);      // slot of the schedule (slot_desc)
        constexpr SlotDesc d = slot_desc(s);
        constexpr int stage = ns / 8, ss = ns % 8, par = stage & (kRing - 1);
        constexpr int st_next = (stage + 1) % kStages, st_fill = (stage + kAhead) % kStages;   // the stage read next; the stage whose weights are stored during this one
#ifdef S2S_ET_ALL_BARRIERS   // (debug builds: a barrier in front of every stage -- the reference the ring's barrier placement is stress-tested against, tools/et_ring_stress.py)
        constexpr bool barrier_here = true;
#else
        constexpr bool barrier_here = !PROJ || (st_next & 1) == 0 || st_next == kStages - 2;    // in front of st_next (ring comment at s_w)
#endif

        // ---------------- top of the slot: next slot's fragments, loads that land under later slots
        if constexpr (ss < 7) {
            fetch(par, ss + 1, fr[(ns + 1) & 1]);
        } else {
            if constexpr (barrier_here) S2S_LDS_BARRIER();
            fetch(st_next & (kRing - 1), 0, fr[(ns + 1) & 1]);
        }
        // next tile: context + edge row under the middle final-layer block, seeds of its tile 0 near the end
        // (the edge row in pieces: a burst of 16 loads per wave holds the slot for ~2 k cycles -- the workgroup's 64 KiB through one
        //  address unit -- and whatever waits next on the in-order counter waits for all of it.  Two loads per slot, in slots whose
        //  next counter wait (the weight store 4+ slots later) is at least 6 slots away: HBM latency fits in between.)
        constexpr int kXv0 = 208;
        if constexpr (BYCLS && s == kClsSlot) ncls = (unsigned)cls_idx[cls_pair(has_next ? wt_next : wt)];
        if constexpr (BYCLS && s == kXv0 + 1) ncls = cls_off((int)ncls);
        if constexpr (s == kXv0) nxt = setup(has_next ? wt_next : wt);
        if constexpr (s == kXv0 + 3) stage_load(nxt);     // (slots ss = 3, 0 of the next stage: none of the edge row's loads)
        if constexpr (s == kXv0 + 8) stage_store();
        if constexpr (s > kXv0 && s <= kXv0 + 16 && ((s & 3) == 1 || (s & 3) == 2)) {
            constexpr int i = 4 * ((s - kXv0) / 4) + 2 * ((s & 3) - 1);   // 2 loads in each of the slots ss = 1, 2, 5, 6 of two stages
            if constexpr (BYCLS) {
                xv[i] = ldrow_cls(ncls, i);
                xv[i + 1] = ldrow_cls(ncls, i + 1);
            } else {
                const float* er = erow_of(nxt);
                xv[i] = ldrow(er, i);
                xv[i + 1] = ldrow(er, i + 1);
            }
        }
        if constexpr (s == 236) seeds_load(nxt, 0);
        // ... and the start values of its first two layer-1 tiles (both accumulator tiles are dead from slot 179 on)
        if constexpr (s == 237) { seedc_piece(nxt, 0, 0); seedc_piece(nxt, 0, 1); seedc_piece(nxt, 0, 2); seedc_piece(nxt, 0, 3); }
        if constexpr (s == 238) { seedc_piece(nxt, 1, 0); seedc_piece(nxt, 1, 1); seedc_piece(nxt, 1, 2); seedc_piece(nxt, 1, 3); }
        // seeds of a1 tile t+1 are fetched in the middle of B_t, in a slot without weight-pipe work (consumed under A_{t+2}, 6+ slots
        // later; a fetch 3 slots ahead of its use cost ~300 cycles at the fetch and ~300 at the use in the timeline probe)
        constexpr bool seeds_slot = d.phase == 1 && d.a == 1 && d.b == 0 && d.t + 1 < 12;   // a quarter behind each of its first 4 MFMAs
        // residual rows of the layer-2 epilogue blocks 1 (n'_i, under B_11) and 2 (n'_j, under the first final-layer block)
        if constexpr (s >= 184 && s < 192) row_load2(node_p + (unsigned long long)cur.bi * 128u, rs, 2 * (s - 184));
        // bias of this slot's layer-2 epilogue pieces (below): block 0 two pieces per slot under the second half of B_11, blocks 1 and 2 one
        constexpr int ep_blk = (s >= 184 && s < 192) ? 0 : ((s >= 192 && s < 224) ? 1 + (s - 192) / 16 : -1);
        constexpr int ep_q = ep_blk == 0 ? 2 * (s - 184) : (s - 192) % 16;
        float4 ep_b = {0.f, 0.f, 0.f, 0.f}, ep_b1 = {0.f, 0.f, 0.f, 0.f};
        if constexpr (ep_blk >= 0) ep_b = ldg4(s_vec + 128 * ep_blk, ep_q, h);
        if constexpr (ep_blk == 0) ep_b1 = ldg4(s_vec, ep_q + 1, h);
        // previous tile's LayerNorm (table below): gamma / beta of the two pieces normalised in this slot
        constexpr int ln_k = ns == 7 ? 0 : ((PROJ && d.phase == 3 && d.a < 7) ? d.a + 1 : ((!PROJ && ns >= 8 && ns < 15) ? ns - 7 : -1));   // their projection k-step
        float4 lnv[4] = {};
        if constexpr (ln_k >= 0) {
#pragma unroll
            for (int k = 0; k < 2; ++k) { lnv[2 * k] = ldg4(s_vec + 512, 2 * ln_k + k, h); lnv[2 * k + 1] = ldg4(s_vec + 640, 2 * ln_k + k, h); }
        }
        // final layer: its accumulators start at G_j = 32 sk (Wf[:, 256:] n'_j + bf), the third column group of node_ab -- the j-side residual
        // of the layer's input x = h2 + [e | n'_i | n'_j] (layers.py:181) taken through the layer per NODE instead of being added to 64
        // hidden values per lane and tile: -64 multiply-adds, -64 registers (the rows n'_j), the bias out of LDS.  Loaded straight into
        // the accumulator registers (dead since the previous tile's LayerNorm), two 16 B pieces per slot in slots 182 .. 189: tile t is
        // complete 4+ slots before its first product (slot 192 / 193) and not live while the layer-2 blocks need every register --
        // same-call A/B against the kernel before (profiles/r05p_et_gseed_ab.txt): four pieces per slot from 184 -0.35 %, from 176 +1.7 %
        // (spills), two per slot from 180 / 182 / 184: -0.67 / -0.70 / -0.45 %.  (Bound: the kernel with that residual simply left out, -1.3 %.)
        constexpr int kGSlot = 182, kGPer = 2;   // two pieces per slot from slot 182
        if constexpr (s >= kGSlot && s < kGSlot + 16 / kGPer) {
#pragma unroll
            for (int u = 0; u < kGPer; ++u) {
                constexpr int p0 = (s - kGSlot) * kGPer;
                const int t3 = (p0 + u) / 4, rq = (p0 + u) % 4;
                const float4 v = ldg4(node_ab + (unsigned long long)cur.bj * 896u + 768 + 32 * t3, rq, h);
                a3[t3][4 * rq + 0] = v.x; a3[t3][4 * rq + 1] = v.y; a3[t3][4 * rq + 2] = v.z; a3[t3][4 * rq + 3] = v.w;
            }
        }
        __builtin_amdgcn_sched_barrier(0);

        // ---------------- the 6 MFMAs, each followed by at most one piece of the weight pipe and one small VALU piece, pinned there
        // (slot-by-slot probe: a slot of bare MFMAs runs at the matrix pipe's 192 cycles; weight-pipe instructions issued as a block
        //  in front of / behind the MFMAs cost 60-120 cycles per slot, a 20-instruction VALU block behind the first MFMA ~100):
        //   weight pipe  group B of stage+1 loaded in slot 0 and stored in slot 5, group A of stage+2 loaded in slot 4 and stored in
        //                slot 1 of the next stage, one 1 KiB piece behind each of MFMAs 0..3; both land in the buffer this stage's
        //                predecessor used, free from that stage's barrier (top of its slot 7) on;
        //   A_t          relu + seeds + split of a1 tile t-1, half a quarter (2 values) behind MFMAs 2 and 4;
        //   layer-2 epilogue  relu(a2 + b2) + x,  x = [e | n'_i | n'_j]  (layers.py:181), in accumulator layout, in 4-value pieces of two
        //                halves: block 0 (its tiles are complete after slot 183: B_11 runs tile-pair major) two pieces per slot under
        //                slots 184..191, in place into the planes the edge row used during layers 1-2 -- whose exact sum x_h + x_l is the
        //                residual row e; block 1 one piece per slot under the final layer's k-steps 0..7 (slots 192..207) into the
        //                planes xq, block 2 under k-steps 8..15 (which read xq) back into xpl;
        //   slots 228..235  split of the next tile's edge row, four halves per slot;
        //   previous tile (positions ns 0..7 = A_0 A_1 of this one, 8..15 = its projection; MFMA i of the slot):
        //                ns 0..3   running sum of piece 4 ns + i behind MFMAs 0..3
        //                ns 4, 5   mean behind MFMA 0 of ns 4; squared deviations of pieces 6 (ns-4) + {0 1 | 2 3 | 4 5} behind MFMAs 1, 3, 5
        //                ns 6      pieces 12 13 | 14 15 behind MFMAs 0, 1; rstd / mask / row pointer behind MFMA 3
        //                normalise + mask + store + (PROJ) split of the two pieces of projection k-step k, behind MFMAs 1 and 3:
        //                k = 0 in ns 7, k = a + 1 in projection slot a (whose MFMAs read k-step a): two k-steps of planes alive at a time
        //                (!PROJ: k = ns - 7 in ns 8..14, the first slots of B_0);
        //                PROJ: the projection's five store groups behind the MFMAs of the first slot after it (ns 16).
        const f16x8 (&f)[4] = fr[ns & 1];
        auto mfma_i = [&](auto ic) {
            constexpr int i = decltype(ic)::value;
            if constexpr (d.phase == 0) {
                f32x16& acc = a1t[d.t & 1];
                const f16x8 (&x)[2] = xpl[2 * d.a + (i >= 3)];
                constexpr int fa = (i == 0 ? 1 : (i < 3 ? 0 : (i == 3 ? 3 : 2))), xa = (i == 1 || i == 4) ? 1 : 0;   // W_l x_h, W_h x_l, W_h x_h
                acc = mfma_f16(f[fa], x[xa], acc);   // (a tile's first product lands on its start value 32 B_j: seedc_piece)
            } else {
                constexpr bool fin = d.phase == 2, prj = d.phase == 3;
                constexpr bool first = i < 2 && (prj ? d.a == 0 : (fin ? false : (d.t == 0 && d.a == 0)));   // (final layer: onto 32 bf)
                f32x16& t = prj ? pq[i & 1] : (fin ? a3[2 * d.b + (i & 1)] : a2[2 * d.b + (i & 1)]);
                const f16x8 (&x)[2] = prj ? xln[d.a] : (fin ? ((d.a >> 3) == 1 ? xq[d.a & 7] : xpl[d.a & 7]) : xp[d.a]);
                constexpr int fa = 2 * (i & 1) + (i < 2 ? 1 : 0), xa = (i == 2 || i == 3) ? 1 : 0;                   // W_l x_h, W_h x_l, W_h x_h
                if constexpr (first) t = mfma_f16(f[fa], x[xa], zero16); else t = mfma_f16(f[fa], x[xa], t);
            }
        };
        // (cutting a half once more -- arithmetic behind one MFMA, split behind the next -- measured 0.7 % slower: a VALU instruction costs
        //  its ~5 cycles wherever it sits; what remains to gain is fewer of them)
        auto ep_half = [&](auto qc, auto hc, const float4& bq) {   // values 2hh, 2hh+1 of piece q = (tile t, quarter rq) of block ep_blk
            constexpr int q = decltype(qc)::value, hh = decltype(hc)::value, t = q / 4, rq = q % 4, j0 = 4 * rq + 2 * hh, e0 = 4 * (rq & 1) + 2 * hh;
            const f32x16& a = a2[4 * (ep_blk < 0 ? 0 : ep_blk) + t];
            f16x8 (&P)[2] = ep_blk == 1 ? xq[2 * t + (rq >> 1)] : xpl[2 * t + (rq >> 1)];
            float r0 = 0.f, r1 = 0.f;
            if constexpr (ep_blk == 0) {   // the residual of block 0 is the edge row = x_h + x_l of the planes this piece replaces (to 2^-24 |x|)
                // (float) x_h + (float) x_l as ONE v_fma_mix_f32 per value (x_h * 1.0 + x_l with both read as f16: the same single rounding
                //  as convert, convert, add)
                const unsigned hw = __builtin_bit_cast(u32x4, P[0])[e0 / 2], lw = __builtin_bit_cast(u32x4, P[1])[e0 / 2];
                asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel_hi:[1,0,1]" : "=v"(r0) : "v"(hw), "v"(lw));
                asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[1,0,1] op_sel_hi:[1,0,1]" : "=v"(r1) : "v"(hw), "v"(lw));
            } else if constexpr (ep_blk == 1) {
                r0 = rs[16 * t + j0];
                r1 = rs[16 * t + j0 + 1];
            }
            float x0 = fmaxf(__builtin_fmaf(a[j0], kInvWS, hh ? bq.z : bq.x), 0.f), x1 = fmaxf(__builtin_fmaf(a[j0 + 1], kInvWS, hh ? bq.w : bq.y), 0.f);
            if constexpr (ep_blk != 2) {   // block 2's residual n'_j went through the final layer on the node side: G_j, the accumulators' start value
                x0 = __builtin_fmaf(r0, sk, x0);   // (sk = 1: r0 + relu(.), exactly)
                x1 = __builtin_fmaf(r1, sk, x1);
            }
            split2_f16(x0, x1, P[0], P[1], e0, amax);
        };
        static_for<0, 6>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            mfma_i(ic);
            if constexpr (i < 4) {
                if constexpr (ss == 0) cp_load_piece(IC<1>{}, ic, st_fill);   // the pipe wraps into the next tile's first stages
                if constexpr (ss == 4) cp_load_piece(IC<0>{}, ic, (stage + kAhead + 1) % kStages);
                // (the piece loaded LAST is stored first: its wait on the in-order counter covers the group, three waits fewer per slot)
                if constexpr (ss == 1) cp_store_piece(IC<0>{}, IC<3 - i>{}, st_fill & (kRing - 1));
                if constexpr (ss == 5) cp_store_piece(IC<1>{}, IC<3 - i>{}, st_fill & (kRing - 1));
            }
            if constexpr (seeds_slot && i < 4) seeds_piece(cur, d.t + 1, i);
            if constexpr (seeds_slot && i < 4 && d.t + 2 < 12) seedc_piece(cur, d.t + 2, i);   // start value of a1 tile t + 2 (A_{t+2} follows this block)
            if constexpr (d.phase == 0 && d.t >= 1 && (i == 2 || i == 4)) s_half(a1t[(d.t - 1) & 1], IC<d.a>{}, IC<(i - 2) / 2>{});
            if constexpr (ep_blk > 0 && (i == 2 || i == 4)) ep_half(IC<ep_q>{}, IC<(i - 2) / 2>{}, ep_b);
            if constexpr (ep_blk == 0 && i >= 1 && i <= 4) {   // pieces ep_q (halves behind MFMAs 1, 2) and ep_q + 1 (3, 4)
                if constexpr (i <= 2) ep_half(IC<ep_q>{}, IC<i - 1>{}, ep_b); else ep_half(IC<ep_q + 1>{}, IC<i - 3>{}, ep_b1);
            }
            if constexpr (s >= 228 && s < 236 && i >= 1 && i <= 4) {   // next tile's edge row: k-step s - 228, elements 2(i-1), 2(i-1)+1
                constexpr int k = s - 228, e = 2 * (i - 1);
                const float4 v = xv[2 * k + (e >> 2)];
                if constexpr ((e & 2) == 0) split2_f16(v.x, v.y, xpn[k][0], xpn[k][1], e, amax);
                else split2_f16(v.z, v.w, xpn[k][0], xpn[k][1], e, amax);
            }
            // ---- previous tile: LayerNorm pieces (table above)
            if constexpr (ns < 4 && i < 4) ln_add(IC<4 * ns + i>{});
            if constexpr (ns == 4 && i == 0) ln_mean = xhalf_sum(ln_sum) * (1.0f / 128);
            if constexpr ((ns == 4 || ns == 5) && (i == 1 || i == 3 || i == 5)) { ln_dev(IC<6 * (ns - 4) + i - 1>{}); ln_dev(IC<6 * (ns - 4) + i>{}); }
            if constexpr (ns == 6 && (i == 0 || i == 1)) { ln_dev(IC<12 + 2 * i>{}); ln_dev(IC<12 + 2 * i + 1>{}); }
            if constexpr (ns == 6 && i == 3) {
                ln_rstd = 1.0f / sqrtf(xhalf_sum(ln_var) * (1.0f / 128) + ln_eps * ((kWS * sk) * (kWS * sk)));
                ln_em = prv.em_i * prv.em_j;
                ln_orow = const_cast<float*>(row_of(out, prv.p, out_tiled));
                ln_sum = 0.f;
                ln_var = 0.f;
            }
            if constexpr (ln_k >= 0 && (i == 1 || i == 3)) ln_out(IC<2 * ln_k + (i - 1) / 2>{}, lnv[i - 1], lnv[i]);
            if constexpr (PROJ && ns == kHead && i < 5) proj_store(ic);
            __builtin_amdgcn_sched_barrier(0);
        });

        // ---------------- exposed steps
        if constexpr (s == 179) {  // B_10 done: tile 11 -> planes (nothing left to hide it under)
            s_quarter(a1t[1], IC<0>{}); s_quarter(a1t[1], IC<1>{}); s_quarter(a1t[1], IC<2>{}); s_quarter(a1t[1], IC<3>{});
        }
    };
    for (;;) {
    wt_next = wt + gridDim.x;
    has_next = wt_next < n_wt;
    static_for<0, kSlots>(slot);

    prv = cur;   // a3 holds this tile's final-layer accumulators: LayerNorm, store and projection in the next pass
#pragma unroll
    for (int i = 0; i < 8; ++i) { xpl[i][0] = xpn[i][0]; xpl[i][1] = xpn[i][1]; }
    // (the next tile's stage 0 sits in buffer 0 again: the ring index is the tile-local stage number)
    if (!has_next) break;
    cur = nxt;
    wt = wt_next;
    }  // persistent tile loop
    // after the last tile: its LayerNorm, store and projection, i.e. the head of one more pass (a second copy of those slots: a branch
    // out of the middle of the loop body costs ~250 spilled registers).  Its layer-1 MFMAs run on the last tile's planes once more
    // (xpn is that tile's row again when there is no next tile) and their results are dropped.
    static_for<0, kHead>(slot);
    if constexpr (PROJ) { proj_store(IC<0>{}); proj_store(IC<1>{}); proj_store(IC<2>{}); proj_store(IC<3>{}); proj_store(IC<4>{}); }
    s2s::range_report(range_flag, amax, s2s::kRangeEdgeTransition);
}

template <bool STAGE, bool BYCLS = false>
int et_launch(const s2s::EtArgs& a) {
    if (a.n_samples <= 0 || a.n_res <= 0) return 0;
    const int io_layout = a.io_layout;
    if ((io_layout & ~31) || ((io_layout & 4) && !a.proj_attn_bias) || (!(io_layout & 4) && !a.out)) return (int)hipErrorInvalidValue;
    // by class (bit 3): not with a tiled input, only with the fused projection; bit 4 (the record size) only with bit 3
    if (BYCLS != ((io_layout & 8) != 0) || (BYCLS ? ((io_layout & 1) || !a.proj_attn_bias) : (io_layout & 16) != 0)) return (int)hipErrorInvalidValue;
    if (a.prescale_exp < 0 || a.prescale_exp > 15) return (int)hipErrorInvalidValue;
    const float sk = ldexpf(1.0f, -a.prescale_exp);
    const long long NN = (long long)a.n_res * a.n_res;
    // 32-bit pair / head-major indices inside a launch (8 M < 2^32): split the samples over several launches when needed
    const long long chunk = s2s::samples_per_launch("S2S_ET_MAX_PAIRS", (1ll << 29) - 1, NN, a.n_samples, (io_layout & 3) != 0);
    if (chunk < 1) return (int)hipErrorInvalidValue;
    const float* one = nullptr;   // s2s_one of the current device
    if (hipGetSymbolAddress((void**)&one, HIP_SYMBOL(s2s_one)) != hipSuccess) return (int)hipErrorInvalidValue;
    const int n_cu = s2s::cu_count();
    for (long long b0 = 0; b0 < a.n_samples; b0 += chunk) {
        const long long nb = a.n_samples - b0 < chunk ? a.n_samples - b0 : chunk;
        const long long M = nb * NN, rows0 = b0 * a.n_res;
        const dim3 grid(s2s::persistent_grid(M, n_cu));
        // BYCLS: words [0, M32) of `edge` are the pairs' class indices, the records follow and do not move with the launch
        const long long m32 = ((long long)a.n_samples * NN + 31) / 32 * 32;
        const float* e = BYCLS ? a.edge + m32 : a.edge + b0 * NN * 128;
        const int* ci = BYCLS ? reinterpret_cast<const int*>(a.edge) + b0 * NN : nullptr;
        const float* nab = a.node_ab + rows0 * 896;
        const float* np = a.node_p + rows0 * 128;
        const float* mk = a.mask ? a.mask + rows0 : one;
        const unsigned mks = a.mask ? 1u : 0u;
        float* o = a.out ? a.out + b0 * NN * 128 : nullptr;
        auto k_proj = &edge_transition_f16_kernel<true, STAGE, BYCLS>;
        if (a.proj_attn_bias) {
            hipLaunchKernelGGL(k_proj, grid, dim3(256), 0, (hipStream_t)a.stream, e, nab, np,
                               (const char*)a.weight_stream, a.b2, a.ln_gamma, a.ln_beta, mk, o, M, a.n_res, a.ln_eps, io_layout, mks,
                               a.proj_bias_cat64, a.proj_attn_bias + b0 * 8 * NN, a.proj_pair_z + b0 * NN * 32, a.range_words, sk, ci);
        } else if constexpr (!BYCLS) {
            auto k_plain = &edge_transition_f16_kernel<false, STAGE>;
            hipLaunchKernelGGL(k_plain, grid, dim3(256), 0, (hipStream_t)a.stream, e, nab, np,
                               (const char*)a.weight_stream, a.b2, a.ln_gamma, a.ln_beta, mk, o, M, a.n_res, a.ln_eps, io_layout, mks,
                               (const float*)nullptr, (float*)nullptr, (float*)nullptr, a.range_words, sk, (const int*)nullptr);
        }
    }
    return (int)hipGetLastError();
}

}  // namespace
