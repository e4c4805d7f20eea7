// A 48 x 48 float64 block as 3 x 3 accumulator tiles of one wave on v_mfma_f64_16x16x4_f64, and the kernels built on it that the
// ensemble_*.hip units share: the tile set, its loads and stores (running values, partial blocks of a k-split, the mirrored store) and the
// operands of a k-step for one operand stream (ensemble_pca.hip, ensemble_rmsd.hip) and for two (ensemble_tica.hip), for symmetric block
// products  C (+)= sum_k z_k z_k^T;  and the two order-fixed skeletons around such a product (grouped column sum, row projection).
//
// Lane maps of the f64 16x16x4 form: lane l feeds A[row = l & 15][k = l >> 4] and B[k = l >> 4][col = l & 15], and receives
// D[row = (l >> 4) + 4 r][col = l & 15] in register r.  With q = l >> 4 and col = l & 15, tile (i, j) of block (bi, bj) therefore holds, in
// register r of lane l, the entry (row 48 bi + 16 i + q + 4 r, column 48 bj + 16 j + col).
//
// Operand layout: a stream is blocks of 48 columns x k (k a multiple of 4), element (k, r) of a block at k * 48 + r, so the lane reads its
// three doubles of a k-step (4 values of k) at q * 48 + col + 16 c and advances by 192.
//
// Everything is float64.  An entry's chain of MFMAs runs in ascending k from zero or from the running value, the SAME operand values serve as
// A and as B, and only entries with row <= column are stored, each also to its mirror: C is exactly symmetric, however k is cut into passes.
#pragma once

#include <hip/hip_runtime.h>

#include "ensemble_common.h"

namespace sym48 {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef d4 Block[3][3];                            // the nine accumulator tiles of a 48 x 48 block

constexpr int TILE_DOUBLES = 256;                  // one 16 x 16 tile in the lane layout: register r of lane l at r * 64 + l
constexpr int BLOCK_DOUBLES = 9 * TILE_DOUBLES;    // a partial block in the lane layout, tile (i, j) at (3 i + j) * 256
constexpr int MEAN_GROUPS = 16;                    // item groups of a workgroup of grouped_column_sum (64 columns x 16 groups = 1024 threads)

// f(i, j, r) for the 36 registers of a lane's block: register r of tile (i, j).
template <typename F>
__device__ __forceinline__ void each_register(F f) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) f(i, j, r);
}

__device__ __forceinline__ void zero(Block& acc) {
    each_register([&](int i, int j, int r) { acc[i][j][r] = 0.0; });
}

// The running values of block (bi, bj) of the row-major n x n matrix c; an entry outside the matrix keeps what acc holds.
__device__ __forceinline__ void load_running(Block& acc, int bi, int bj, int q, int col, int n, const double* __restrict__ c) {
    each_register([&](int i, int j, int r) {
        const int gr = bi * 48 + 16 * i + q + 4 * r, gc = bj * 48 + 16 * j + col;
        if (gr < n && gc < n) acc[i][j][r] = c[(size_t)gr * n + gc];
    });
}

// A partial block in the lane layout; p points at the lane's first double (block + lane).
__device__ __forceinline__ void load_partial(Block& acc, const double* __restrict__ p) {
    each_register([&](int i, int j, int r) { acc[i][j][r] = p[(3 * i + j) * TILE_DOUBLES + r * 64]; });
}

__device__ __forceinline__ void add_partial(Block& acc, const double* __restrict__ p) {
    each_register([&](int i, int j, int r) { acc[i][j][r] += p[(3 * i + j) * TILE_DOUBLES + r * 64]; });
}

__device__ __forceinline__ void store_partial(const Block& acc, double* __restrict__ p) {
    each_register([&](int i, int j, int r) { p[(3 * i + j) * TILE_DOUBLES + r * 64] = acc[i][j][r]; });
}

// Entries with row <= col of an accumulated block go to the n x n matrix c and to their mirror.  (gr > gc occurs only inside a diagonal
// block: that entry comes from its mirror.)
__device__ __forceinline__ void store_mirrored(const Block& acc, int bi, int bj, int q, int col, int n, double* __restrict__ c) {
    each_register([&](int i, int j, int r) {
        const int gr = bi * 48 + 16 * i + q + 4 * r, gc = bj * 48 + 16 * j + col;
        if (gr >= n || gc >= n || gr > gc) return;
        c[(size_t)gr * n + gc] = acc[i][j][r];
        if (gr < gc) c[(size_t)gc * n + gr] = acc[i][j][r];
    });
}

// Block (bi, bj), bi <= bj, number `tri` of the upper triangle in row-major order.
__device__ __forceinline__ void block_of(long long tri, int nblk, int& bi, int& bj) {
    int i = 0;
    while (tri >= nblk - i) { tri -= nblk - i; ++i; }
    bi = i; bj = i + (int)tri;
}

// The operands of one k-step of a lane, for STREAMS operand streams, and their MFMAs into as many blocks.
template <int STREAMS>
struct Operands;

// One stream: the row block's three doubles (a) and the column block's (b); nine MFMAs, acc[i][j] += a_i b_j.
template <>
struct Operands<1> {
    double a[3], b[3];

    __device__ __forceinline__ void load(const double* __restrict__ pa, const double* __restrict__ pb) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { a[c] = pa[16 * c]; b[c] = pb[16 * c]; }
    }

    __device__ __forceinline__ void accumulate(Block& acc) const {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
};

// Two streams `stream` doubles apart, z (a0, b0) and z' (a1, b1): both  s00 += z z^T + z' z'^T  and  s0t += z z'^T + z' z^T  from the
// same four loads, every tile (i, j) taking  s00 += a0_i b0_j, s00 += a1_i b1_j, s0t += a0_i b1_j, s0t += a1_i b0_j  in that order.
template <>
struct Operands<2> {
    double a0[3], a1[3], b0[3], b1[3];

    __device__ __forceinline__ void load(const double* __restrict__ pa, const double* __restrict__ pb, size_t stream) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { a0[c] = pa[16 * c]; a1[c] = pa[stream + 16 * c]; b0[c] = pb[16 * c]; b1[c] = pb[stream + 16 * c]; }
    }

    __device__ __forceinline__ void accumulate(Block& s00, Block& s0t) const {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                s00[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[i], b0[j], s00[i][j], 0, 0, 0);
                s00[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[i], b1[j], s00[i][j], 0, 0, 0);
                s0t[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[i], b1[j], s0t[i][j], 0, 0, 0);
                s0t[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[i], b0[j], s0t[i][j], 0, 0, 0);
            }
    }
};

// Column sums over n_items items in an order that is a function of n_items alone, for a workgroup of 64 x MEAN_GROUPS threads: thread
// (group g = threadIdx.x >> 6, column lane = threadIdx.x & 63; live: the column exists) adds term(item) of the items g, g + 16, ... in
// ascending order, and the 16 partial sums of a column are then added in ascending g.  -> true in the one thread that then holds the sum.
template <typename Term>
__device__ __forceinline__ bool grouped_column_sum(long long n_items, bool live, Term term, double& sum) {
    __shared__ double part[MEAN_GROUPS][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    double acc = 0.0;
    if (live)
        for (long long t = g; t < n_items; t += MEAN_GROUPS) acc += term(t);
    part[g][lane] = acc;
    __syncthreads();
    if (g != 0 || !live) return false;
    sum = part[0][lane];
    for (int k = 1; k < MEAN_GROUPS; ++k) sum += part[k][lane];
    return true;
}

// One wave per row: proj_row[k] = sum_c centred(c) comp[k][c].  Lane l adds the columns l, l + 64, ... of every component in ascending
// order and the lanes meet in the xor tree: the order is a function of `width` alone.
template <typename Centred>
__device__ __forceinline__ void project_row(int width, Centred centred, const double* __restrict__ comp, int K, double* __restrict__ proj_row) {
    const int lane = threadIdx.x;
    for (int k = 0; k < K; ++k) {
        const double* v = comp + (size_t)k * width;
        double acc = 0.0;
        for (int c = lane; c < width; c += 64) acc += centred(c) * v[c];
        acc = ensemble::wave_sum(acc);
        if (lane == 0) proj_row[k] = acc;
    }
}

}  // namespace sym48
