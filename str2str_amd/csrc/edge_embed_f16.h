#pragma once
#include "pair_f16.h"

namespace {

// Edge embedding on split-f16 MFMA (arithmetic and range guard: pair_f16.h): same operator and contract as s2s_edge_embed (csrc/pair_mlp.hip; reference
// EmbeddingModule.forward edge branch, denoising_ipa.py:137-158).  The first Linear(120 -> 128) is a sum of four gathered
// rows (+ ReLU); the two 128 x 128 layers, LayerNorm and (PROJ) the first IPA block's linear_b / down_z run as f16x3 slots
// exactly like the edge transition (edge_transition_f16.h): 5 weight stages of 32 KiB (W2 | W3 | [linear_b; down_z]), 40 slots of 6 MFMAs per
// 32-pair tile, persistent workgroups; the NEXT tile's rows are gathered and split under the current tile's MFMAs.
// TABLE (s2s_edge_embed_classes_f16x3): the same body on the rows of the CLASS TABLE instead of on pairs.  "Pair" r is the class
//   r = ((fa 2 + fb) n_rel + d) (n_bins + 1) + (bin + 1)   (s2s::ee_class_row)
// and gathers node_a[fa], node_b[fb] (N = the number of rows of these two operands), rel_tab[d], bin_tab[bin] (kb = 0 for bin = -1):
// no CA, residue index or mask is read, the edge mask is 1, and a row's outputs go to one contiguous record of `out`
// (z[128] | attn_bias[8] | pair_z[32] with PROJ, z alone without).  Only the per-pair setup and the output addresses differ: the
// weight pipe, the slots, the split, LayerNorm, the projection and the range tracking are the statements below, shared.
template <bool PROJ, bool TABLE = false>
__global__ void __launch_bounds__(256) edge_embed_f16_kernel(
    const float* __restrict__ node_a, const float* __restrict__ node_b, const float* __restrict__ rel_tab,
    const float* __restrict__ bin_tab, const float* __restrict__ bin_lower, const long long* __restrict__ residue_idx,
    const float* __restrict__ ca, const char* __restrict__ wblob, const float* __restrict__ b2, const float* __restrict__ b3,
    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mask, float* __restrict__ out,
    long long M, int N, int rel_off, int n_rel, int n_bins, float ln_eps, int out_tiled, const float* __restrict__ proj_b,
    float* __restrict__ proj_bias_out, float* __restrict__ proj_pz_out, int* __restrict__ range_flag) {
    constexpr int kStages = PROJ ? 5 : 4;
    constexpr int kSlots = 8 * kStages;
    __shared__ __attribute__((aligned(16))) char s_w[2][kStageBytes];
    __shared__ __attribute__((aligned(16))) float s_vec[512 + 64];  // b2 | b3 | gamma | beta | projection bias
    __shared__ __attribute__((aligned(16))) float s_bins[s2s::kEeBinSlots];    // distogram bin lower edges (ascending), padded with 3e38
    const int lane = threadIdx.x & 63, h = lane >> 5, wave = threadIdx.x >> 6;

    // ---- weight pipe (identical to the edge transition's)
    const unsigned voff = wave * 8192 + lane * 16;
    typedef __attribute__((address_space(3))) char lds_char;
    lds_char* lds_image[2] = {(lds_char*)&s_w[0][lane * 16], (lds_char*)&s_w[1][lane * 16]};
    asm volatile("" : "+v"(lds_image[0]), "+v"(lds_image[1]));
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)wblob, 0, kStages * kStageBytes, 0x00020000);
    auto ldw = [&](unsigned vo, int so) -> f32x4 {
        const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, vo, so, 0);
        return f32x4{__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w)};
    };
    f32x4 c0, c1, c2, c3, e0, e1, e2, e3;
    typedef __attribute__((address_space(3))) f32x4 lds_f4;
    auto cp_load_a = [&](int stage) {
        const int so = stage * kStageBytes;
        c0 = ldw(voff, so); c1 = ldw(voff + 1024, so); c2 = ldw(voff + 2048, so); c3 = ldw(voff + 3072, so);
    };
    auto cp_load_b = [&](int stage) {
        const int so = stage * kStageBytes + 4096;
        e0 = ldw(voff, so); e1 = ldw(voff + 1024, so); e2 = ldw(voff + 2048, so); e3 = ldw(voff + 3072, so);
    };
    auto cp_store_a = [&](int par) {
        lds_char* d = lds_image[par] + wave * 8192;   // (last-loaded piece first: its counter wait covers the group)
        *(lds_f4*)(d + 3072) = c3; *(lds_f4*)(d + 2048) = c2; *(lds_f4*)(d + 1024) = c1; *(lds_f4*)(d) = c0;
    };
    auto cp_store_b = [&](int par) {
        lds_char* d = lds_image[par] + (wave * 8192 + 4096);
        *(lds_f4*)(d + 3072) = e3; *(lds_f4*)(d + 2048) = e2; *(lds_f4*)(d + 1024) = e1; *(lds_f4*)(d) = e0;
    };
    cp_load_a(0);
    cp_load_b(0);

    // ---- per-tile context: the four first-layer rows of this lane's pair
    // node_b / rel_tab / bin_tab come COLUMN-BLOCKED: [32 chunks of 4 channels][rows][4], so that the 16 B a lane wants of
    // its pair's row sit next to the neighbouring pairs' (consecutive j -> consecutive rows): one load instruction touches
    // 8 cache lines instead of 32.  Lane part of the address in voffset, chunk pair (2G, 2G+1) in the scalar offset.
    struct Ctx {
        const float* ra;
        unsigned vb, vr, vk;   // byte offsets of (row, chunk h) in node_b / rel_tab / bin_tab
        float kb;
        long long p, boff;
        float em;
        bool valid;
    };
    const long long NN = (long long)N * N;
    const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc((void*)node_b, 0, (unsigned)((TABLE ? (long long)N : M / N) * 512), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_r = __builtin_amdgcn_make_buffer_rsrc((void*)rel_tab, 0, n_rel * 512, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_k = __builtin_amdgcn_make_buffer_rsrc((void*)bin_tab, 0, n_bins * 512, 0x00020000);
    // setup in two halves so that the per-pair loads (CA coordinates, residue indices, masks) are in flight for a few slots
    // before they are consumed; the distogram edges sit in LDS (s_bins)
    struct Raw {
        long long p, bi, bj, bb;
        float ax, ay, az, bx, by, bz;
        long long ii, ij;
        float mi, mj;
        bool valid;
    };
    // The launcher keeps the pair count of one launch below 2^31: 32-bit index arithmetic, division by N through
    // floor(2^32 / N) (quotient short by at most one for x < 2^31; a 64-bit division is ~100 VALU instructions).
    const unsigned n_magic = N >= 2 ? (unsigned)((1ull << 32) / (unsigned)N) : 0u;
    auto div_n = [&](unsigned x, unsigned& q, unsigned& r) {
        q = N >= 2 ? __umulhi(x, n_magic) : x;
        r = x - q * (unsigned)N;
        const bool fix = r >= (unsigned)N;
        q = fix ? q + 1 : q;
        r = fix ? r - (unsigned)N : r;
    };
    const float* mask_or_any = mask ? mask : ca;  // always a readable [B N] float array: no branch around the mask loads
    auto setup_a = [&](long long wg_tile) -> Raw {
        long long p = (wg_tile * 4 + wave) * 32 + (lane & 31);
        Raw r;
        r.valid = p < M;
        p = r.valid ? p : M - 1;
        r.p = p;
        if constexpr (TABLE) {   // class row p -> (fa, fb, d, bin + 1), carried in the fields of the row / column node, the two indices
            const unsigned nb1 = (unsigned)n_bins + 1u, q = (unsigned)p / nb1, cls = q / (unsigned)n_rel;
            r.bi = cls >> 1; r.bj = cls & 1u; r.bb = 0;
            r.ii = q - cls * (unsigned)n_rel; r.ij = (unsigned)p - q * nb1;
            r.ax = r.ay = r.az = r.bx = r.by = r.bz = 0.f;
            r.mi = r.mj = 1.f;
            return r;
        }
        // p = (bb N + i) N + j:  global row bi = p / N,  j = p - bi N,  bb = bi / N
        unsigned bi, j, bb, i;
        div_n((unsigned)p, bi, j);
        div_n(bi, bb, i);
        r.bi = bi; r.bb = bb; r.bj = bb * (unsigned)N + j;
        r.ax = ca[r.bi * 3 + 0]; r.ay = ca[r.bi * 3 + 1]; r.az = ca[r.bi * 3 + 2];
        r.bx = ca[r.bj * 3 + 0]; r.by = ca[r.bj * 3 + 1]; r.bz = ca[r.bj * 3 + 2];
        r.ii = residue_idx[r.bi];
        r.ij = residue_idx[r.bj];
        r.mi = mask_or_any[r.bi];
        r.mj = mask_or_any[r.bj];
        return r;
    };
    auto setup_b = [&](const Raw& r) -> Ctx {
        Ctx c;
        c.valid = r.valid;
        // distogram bin and relative-position row of this pair (edge_embed_class.h); TABLE: the class row names them
        const int bin = TABLE ? (int)r.ij - 1 : s2s::ee_pair_bin(s_bins, n_bins, r.ax, r.ay, r.az, r.bx, r.by, r.bz);
        const long long d = TABLE ? r.ii : s2s::ee_rel_row(r.ii, r.ij, rel_off, n_rel);
        c.ra = node_a + r.bi * 128;
        const unsigned jj = (unsigned)(r.bj - r.bb * N);
        c.vb = ((unsigned)r.bb * 32u * (unsigned)N + (unsigned)h * (unsigned)N + jj) * 16u;
        c.vr = ((unsigned)h * (unsigned)n_rel + (unsigned)d) * 16u;
        c.vk = ((unsigned)h * (unsigned)n_bins + (unsigned)(bin < 0 ? 0 : bin)) * 16u;
        c.kb = bin < 0 ? 0.f : 1.f;
        c.p = r.p;
        c.boff = r.p + 7 * r.bb * NN;
        c.em = (!TABLE && mask) ? r.mi * r.mj : 1.0f;
        return c;
    };
    float amax = 0.f;   // range guard (range_flag.h)
    auto split4 = [&](const float (&x)[4], f16x8& ph, f16x8& pm, int at) {  // planes (x_h, x_l)
        split4_f16(x, ph, pm, at, amax);
    };
    // first-layer sum in accumulator layout: g1[4G + q] = channel 8G + 4h + q, built row by row (same association as the
    // fp32 kernel: ((a + b) + r) + kb*k)
    float g1[64];
    auto row_set = [&](const float* r) {
#pragma unroll
        for (int G = 0; G < 16; ++G) {
            const float4 v = ldg4(r, G, h);
            g1[4 * G + 0] = v.x; g1[4 * G + 1] = v.y; g1[4 * G + 2] = v.z; g1[4 * G + 3] = v.w;
        }
    };
    float tmp[64];
    auto row_cb = [&](const __amdgpu_buffer_rsrc_t& rs, unsigned vo, int rows, float (&dst)[64], int G0, int G1) {
#pragma unroll
        for (int G = G0; G < G1; ++G) {  // chunk 2G + h of the row: scalar offset 2G rows-blocks of 16 B
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, vo, G * 32 * rows, 0);
            dst[4 * G + 0] = __uint_as_float(v.x); dst[4 * G + 1] = __uint_as_float(v.y);
            dst[4 * G + 2] = __uint_as_float(v.z); dst[4 * G + 3] = __uint_as_float(v.w);
        }
    };
    auto row_add = [&](float scale) {  // pinned: left alone, the compiler sinks these adds to the splits 20 slots later and keeps
#pragma unroll                         // (spills) all four loaded rows until then
        for (int i = 63; i >= 0; --i) {   // (last-loaded values first: one counter wait for the whole row instead of one per load)
            g1[i] = __fmaf_rn(scale, tmp[i], g1[i]);  // (explicit: both template variants must round alike)
            asm volatile("" : "+v"(g1[i]));
        }
    };
    // ReLU + split of first-layer k-step ks (registers 8ks .. 8ks+7 of g1: chain order) into planes
    auto g1_split = [&](f16x8 (&dst)[2], int ks) {
        const float x0[4] = {relu1(g1[8 * ks + 0]), relu1(g1[8 * ks + 1]), relu1(g1[8 * ks + 2]), relu1(g1[8 * ks + 3])};
        const float x1[4] = {relu1(g1[8 * ks + 4]), relu1(g1[8 * ks + 5]), relu1(g1[8 * ks + 6]), relu1(g1[8 * ks + 7])};
        split4(x0, dst[0], dst[1], 0);
        split4(x1, dst[0], dst[1], 4);
    };

    const long long n_wt = (M + 127) / 128;
    long long wt = blockIdx.x;
    if constexpr (!TABLE) s2s::ee_fill_bins(s_bins, bin_lower, n_bins);
    __syncthreads();
    Ctx cur = setup_b(setup_a(wt));
    f16x8 xp[8][2];  // planes of the current layer's input (8 k-steps of 16)
    {
        row_set(cur.ra);
        for (int i = threadIdx.x; i < 512; i += 256)
            s_vec[i] = i < 128 ? kWS * b2[i] : (i < 256 ? kWS * b3[i - 128] : (i < 384 ? gamma[i - 256] : beta[i - 384]));   // biases x 32 (accumulator scale)
        if (PROJ && threadIdx.x < 64) s_vec[512 + threadIdx.x] = proj_b[threadIdx.x];
        cp_store_a(0);
        cp_load_a(1);
        cp_store_b(0);
        row_cb(rs_b, cur.vb, N, tmp, 0, 16); row_add(1.0f);
        row_cb(rs_r, cur.vr, n_rel, tmp, 0, 16); row_add(1.0f);
        row_cb(rs_k, cur.vk, n_bins, tmp, 0, 16); row_add(cur.kb);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) g1_split(xp[ks], ks);
    }
    f32x16 a2[4], a3[4], pq[2];
    f16x8 fr[2][4];
    auto fetch = [&](int par, int slot_in_stage, f16x8 (&f)[4]) {
        typedef __attribute__((address_space(3))) f16x8 lds_frag;
        const lds_frag* s = (const lds_frag*)lds_image[par] + slot_in_stage * 4 * 64;
        f[0] = s[0]; f[2] = s[128]; f[3] = s[192]; f[1] = s[64];   // (the slot's first MFMA reads f[1]: one counter wait per slot, as in the edge transition)
    };
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // The VALU work of a tile is cut into per-k-step pieces, each pinned (empty asm on its inputs / outputs: otherwise the
    // compiler sinks a piece to its first use, i.e. in FRONT of the MFMAs that wait for it) into a slot whose MFMAs do not depend
    // on it, and interleaved with them by sched_group_barrier.
    auto pin_frag = [&](f16x8 (&x)[2]) { asm volatile("" : "+v"(x[0]), "+v"(x[1])); };
    // accumulator start = bias (registers 4 rq + q of tile t <-> channel 32 t + 8 rq + 4 h + q)
    auto bias16 = [&](const float* vec, int t) -> f32x16 {   // (s_vec holds 32 x bias: the accumulators carry 32 x the layer output)
        const float4 b0 = ldg4(vec, 4 * t, h), b1 = ldg4(vec, 4 * t + 1, h), b2v = ldg4(vec, 4 * t + 2, h), b3v = ldg4(vec, 4 * t + 3, h);
        return f32x16{b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w, b2v.x, b2v.y, b2v.z, b2v.w, b3v.x, b3v.y, b3v.z, b3v.w};
    };
    // layer-2 output (bias already in the accumulator): ReLU + split of k-step k -> layer-3 input planes xp[k]
    auto l2_piece = [&](auto kc) {
        constexpr int k = decltype(kc)::value, t = k / 2;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int rq = 2 * (k & 1) + u;
            const float xx[4] = {relu1(a2[t][4 * rq + 0]) * kInvWS, relu1(a2[t][4 * rq + 1]) * kInvWS,
                                 relu1(a2[t][4 * rq + 2]) * kInvWS, relu1(a2[t][4 * rq + 3]) * kInvWS};
            split4(xx, xp[k][0], xp[k][1], 4 * u);
        }
        pin_frag(xp[k]);
    };
    float ln_mean = 0.f, ln_rstd = 0.f;
    // output block of the wave (16 KiB): row-major  n 512 + g 32 + h 16,  tiled  g 1024 + lane 16  (edge transition, "Pair-tensor layouts")
    // (TABLE: row-major records of kRec floats)
    constexpr unsigned kRec = TABLE ? (PROJ ? s2s::kEeRecProj : s2s::kEeRecPlain) : 128u;
    const unsigned out_lane = out_tiled ? lane * 16u : (unsigned)((lane & 31) * (kRec * 4) + h * 16), out_step = out_tiled ? 1024u : 32u;
    f16x8 xq[2][2];  // LayerNorm output planes of the projection's current / next k-step
    // LayerNorm output of k-step k (16 channels): scale, shift, edge mask, store (+ planes for the projection)
    __amdgpu_buffer_rsrc_t rs_out;  // this tile's 32 output rows; rows past M are outside num_records: their stores are dropped
    auto out_rsrc = [&](long long wg_tile) {
        const long long p0 = (wg_tile * 4 + __builtin_amdgcn_readfirstlane(wave)) * 32;
        const long long left = M - p0;
        // (tiled layout: the pairs of a partial last tile are interleaved with its padding, which the buffer holds: whole block)
        rs_out = __builtin_amdgcn_make_buffer_rsrc((void*)(out + (p0 < M ? p0 : 0) * kRec), 0,
                                                   (unsigned)(left <= 0 ? 0 : (left < 32 && !out_tiled ? left : 32)) * (kRec * 4u), 0x00020000);
    };
    float4 lga[2], lbe[2];  // gamma / beta of the next LayerNorm piece, read at the top of its slot
    auto ln_load = [&](auto kc) {
        constexpr int k = decltype(kc)::value;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int g = 4 * (k / 2) + 2 * (k & 1) + u;
            lga[u] = ldg4(s_vec + 256, g, h);
            lbe[u] = ldg4(s_vec + 384, g, h);
        }
    };
    auto ln_piece = [&](auto kc, const Ctx& c) {
        constexpr int k = decltype(kc)::value, t = k / 2;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int rq = 2 * (k & 1) + u, g = 4 * t + rq;
            const float4 ga = lga[u], be = lbe[u];
            float4 o;
            // (the channel offset goes into the store's immediate field, not into an SGPR soffset: a 128-bit buffer store with an
            // SGPR offset followed by VALU writes of its data registers lost the last lanes' data in the plain variant)
            // explicit roundings: the fused-projection and the plain variant of this kernel must agree bit for bit
            o.x = __fmul_rn(__fmaf_rn(__fmul_rn(a3[t][4 * rq + 0] - ln_mean, ln_rstd), ga.x, be.x), c.em);
            o.y = __fmul_rn(__fmaf_rn(__fmul_rn(a3[t][4 * rq + 1] - ln_mean, ln_rstd), ga.y, be.y), c.em);
            o.z = __fmul_rn(__fmaf_rn(__fmul_rn(a3[t][4 * rq + 2] - ln_mean, ln_rstd), ga.z, be.z), c.em);
            o.w = __fmul_rn(__fmaf_rn(__fmul_rn(a3[t][4 * rq + 3] - ln_mean, ln_rstd), ga.w, be.w), c.em);
            // (plain stores: with the nt bit, no change beyond the noise; profiles/r06_et_nt_ab.txt)
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{__float_as_uint(o.x), __float_as_uint(o.y), __float_as_uint(o.z), __float_as_uint(o.w)},
                                                   rs_out, out_lane + (unsigned)g * out_step, 0, 0);
            if constexpr (PROJ) {
                const float xx[4] = {o.x, o.y, o.z, o.w};
                split4(xx, xq[k & 1][0], xq[k & 1][1], 4 * u);
            }
        }
        if constexpr (PROJ) pin_frag(xq[k & 1]);
    };
    // rows of the next tile's first layer, eight 16 B loads per slot (a burst of 32 per wave backs up the vector memory
    // pipe and with it the wave's MFMA issue)
    auto row_load8 = [&](const float* r, float (&dst)[64], int half) {
#pragma unroll
        for (int G = 8 * half; G < 8 * half + 8; ++G) {
            const float4 v = ldg4(r, G, h);
            dst[4 * G + 0] = v.x; dst[4 * G + 1] = v.y; dst[4 * G + 2] = v.z; dst[4 * G + 3] = v.w;
        }
    };
    S2S_LDS_BARRIER();
    fetch(0, 0, fr[0]);
    f32x16 initA0 = bias16(s_vec, 0), initA1 = bias16(s_vec, 1), initB0, initB1;
    // per-pair scalars (CA coordinates, residue indices, masks) of the tile after this one: requested a whole tile ahead -- used four
    // slots after the request they cost the tile ~1.2 k cycles of waiting (profiles/r03f_ee_phase_probe.txt)
    Raw nraw = setup_a(wt + gridDim.x < n_wt ? wt + gridDim.x : wt);

    for (;;) {
    const long long wt_next = wt + gridDim.x;
    const bool has_next = wt_next < n_wt;
    Ctx nxt = cur;
    f16x8 xl[2];  // the next tile's last k-step (xp[7] is read by the final layer's last slot)
    static_for<0, kSlots>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        constexpr int stage = s / 8, ss = s % 8, par = stage & 1;
        constexpr int layer = s / 16;             // 0: layer 2, 1: layer 3, 2: projection
        constexpr int ks = layer < 2 ? (s % 16) / 2 : s - 32;
        constexpr int pr = layer < 2 ? s % 2 : 0;
        // ---------------- top of the slot: LDS / global loads whose results are used under later MFMAs
        // the accumulators of a layer's first two slots start from the bias, read one slot ahead (A: slots 0 / 16, B: 1 / 17)
        if constexpr (s == kSlots - 1) { initA0 = bias16(s_vec, 0); initA1 = bias16(s_vec, 1); }
        if constexpr (s == 0) { initB0 = bias16(s_vec, 2); initB1 = bias16(s_vec, 3); }
        if constexpr (s == 15) { initA0 = bias16(s_vec + 128, 0); initA1 = bias16(s_vec + 128, 1); }
        if constexpr (s == 16) { initB0 = bias16(s_vec + 128, 2); initB1 = bias16(s_vec + 128, 3); }
        if constexpr (PROJ && s >= 31 && s < 39) ln_load(IC<s - 31>{});
        if constexpr (ss < 7) {
            fetch(par, ss + 1, fr[(s + 1) & 1]);
        } else {
            S2S_LDS_BARRIER();
            fetch(par ^ 1, 0, fr[(s + 1) & 1]);
        }
        // next tile: per-pair loads under slot 0, context under slot 4, then its four first-layer rows
        if constexpr (s == 30) out_rsrc(wt);
        if constexpr (s == 5) row_load8(nxt.ra, g1, 0);
        if constexpr (s == 6) row_load8(nxt.ra, g1, 1);
        if constexpr (s == 7) row_cb(rs_b, nxt.vb, N, tmp, 0, 8);
        if constexpr (s == 8) row_cb(rs_b, nxt.vb, N, tmp, 8, 16);
        if constexpr (s == 13) row_cb(rs_r, nxt.vr, n_rel, tmp, 0, 8);
        if constexpr (s == 14) row_cb(rs_r, nxt.vr, n_rel, tmp, 8, 16);
        if constexpr (s == 18) row_cb(rs_k, nxt.vk, n_bins, tmp, 0, 8);
        if constexpr (s == 19) row_cb(rs_k, nxt.vk, n_bins, tmp, 8, 16);
        __builtin_amdgcn_sched_barrier(0);

        // ---------------- the 12 MFMAs and the VALU pieces that run under them
        const f16x8 (&f)[4] = fr[s & 1];
        const f16x8 (&x)[2] = layer < 2 ? xp[ks] : xq[ks & 1];
        f32x16& t0 = layer == 0 ? a2[2 * pr] : (layer == 1 ? a3[2 * pr] : pq[0]);
        f32x16& t1 = layer == 0 ? a2[2 * pr + 1] : (layer == 1 ? a3[2 * pr + 1] : pq[1]);
        if constexpr (ks == 0) {
            if constexpr (layer < 2) {
                t0 = mfma_f16(f[1], x[0], pr == 0 ? initA0 : initB0); t1 = mfma_f16(f[3], x[0], pr == 0 ? initA1 : initB1);
            } else {
                t0 = mfma_f16(f[1], x[0], zero16); t1 = mfma_f16(f[3], x[0], zero16);
            }
        } else {
            t0 = mfma_f16(f[1], x[0], t0); t1 = mfma_f16(f[3], x[0], t1);  // W_l x_h
        }
        t0 = mfma_f16(f[0], x[1], t0); t1 = mfma_f16(f[2], x[1], t1);      // W_h x_l
        t0 = mfma_f16(f[0], x[0], t0); t1 = mfma_f16(f[2], x[0], t1);      // W_h x_h
        if constexpr (s == 1) nxt = setup_b(nraw);                                                        // the next tile's context
        if constexpr (s == 26) nraw = setup_a(wt_next + gridDim.x < n_wt ? wt_next + gridDim.x : wt_next);   // requests for the tile after it
        if constexpr (s == 12) row_add(1.0f);     // a + b   (same association as the fp32 kernel: ((a + b) + r) + kb k)
        if constexpr (s == 17) row_add(1.0f);     // + relative-position row
        if constexpr (s == 22) row_add(nxt.kb);   // + distogram row
        // layer-2 output, k-step k (read by slots 16 + 2k, 17 + 2k) under slot 14 + 2k, k-step 0 under slot 15
        if constexpr (s >= 16 && s <= 28 && s % 2 == 0) l2_piece(IC<(s - 14) / 2>{});
        if constexpr (s == 15) l2_piece(IC<0>{});   // tiles 0, 1 of the layer-2 output are complete after slot 14
        // next tile's first layer: k-step k of xp is last read by slot 17 + 2k, so k = 0..6 go under slots 24..30 and the
        // last one (under slot 23) into xl
        if constexpr (s >= 24 && s < 31) { g1_split(xp[s - 24], s - 24); pin_frag(xp[s - 24]); }
        if constexpr (s == 23) { g1_split(xl, 7); pin_frag(xl); }
        // LayerNorm output k-step k + 1 under projection slot 32 + k
        if constexpr (PROJ && s >= 32 && s < 39) ln_piece(IC<s - 31>{}, cur);
        // weight pipe: one load / LDS store behind each of the first four MFMAs (edge transition, same slots)
        if constexpr (ss == 0) cp_load_b((stage + 1) % kStages);
        if constexpr (ss == 4) cp_load_a((stage + 2) % kStages);
        if constexpr (ss == 1) cp_store_a(par ^ 1);
        if constexpr (ss == 5) cp_store_b(par ^ 1);
        constexpr int copy_kind = (ss == 0 || ss == 4) ? 0x020 : ((ss == 1 || ss == 5) ? 0x200 : 0);   // VMEM read | DS write | none
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // one MFMA,
            if (copy_kind != 0 && i < 4) __builtin_amdgcn_sched_group_barrier(copy_kind, 1, 0);   // one piece of the weight pipe,
            __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);  // up to eight VALU instructions behind it
        }
        __builtin_amdgcn_sched_barrier(0);

        // ---------------- exposed steps
        if constexpr (s == 31) {  // layer-3 output (bias included): LayerNorm statistics
            float sum = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) sum += a3[t][r];
            ln_mean = __fmul_rn(xhalf_sum(sum), 1.0f / 128);
            float var = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float dd = a3[t][r] - ln_mean;
                    var = __fmaf_rn(dd, dd, var);
                }
            ln_rstd = 1.0f / sqrtf(__fmaf_rn(xhalf_sum(var), 1.0f / 128, ln_eps * (kWS * kWS)));   // (scaled accumulator: 1024 eps)
            if constexpr (PROJ) {
                ln_piece(IC<0>{}, cur);
            } else {
                static_for<0, 8>([&](auto kc) { ln_load(kc); ln_piece(kc, cur); });
            }
        }
    });
    if constexpr (PROJ) {
        if (cur.valid) {
            const float4 b0 = ldg4(s_vec + 512, 0, h);
            // (TABLE: both projections follow z in the class row's record)
            float* o = TABLE ? out + cur.p * kRec + 128 + 4 * h : proj_bias_out + cur.boff + 4 * h * NN;
            const long long hs = TABLE ? 1 : NN;
            float* pz = TABLE ? out + cur.p * kRec + 136 : proj_pz_out + cur.p * 32;
            o[0] = __builtin_fmaf(pq[0][0], kInvWS, b0.x);
            o[hs] = __builtin_fmaf(pq[0][1], kInvWS, b0.y);
            o[2 * hs] = __builtin_fmaf(pq[0][2], kInvWS, b0.z);
            o[3 * hs] = __builtin_fmaf(pq[0][3], kInvWS, b0.w);
#pragma unroll
            for (int g = 1; g <= 4; ++g) {
                const int t = g >> 2, rq = g & 3;
                const float4 bq = ldg4(s_vec + 512, g, h);
                *reinterpret_cast<float4*>(pz + 8 * (g - 1) + 4 * h) =
                    make_float4(__builtin_fmaf(pq[t][4 * rq + 0], kInvWS, bq.x), __builtin_fmaf(pq[t][4 * rq + 1], kInvWS, bq.y),
                                __builtin_fmaf(pq[t][4 * rq + 2], kInvWS, bq.z), __builtin_fmaf(pq[t][4 * rq + 3], kInvWS, bq.w));
            }
        }
    }
    if (!has_next) break;
    cur = nxt;
    wt = wt_next;
    xp[7][0] = xl[0]; xp[7][1] = xl[1];
    if constexpr (kStages % 2 == 1) {  // odd stage count: the next tile's stage 0 sits in the other buffer
        lds_char* sw = lds_image[0];
        lds_image[0] = lds_image[1];
        lds_image[1] = sw;
    }
    }  // persistent tile loop
    s2s::range_report(range_flag, amax, s2s::kRangeEdgeEmbed);
}

}  // namespace
