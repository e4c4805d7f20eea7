// TM-score under the identity correspondence (residue i <-> residue i, as the TMscore program, not TM-align) on the device: the
// length-normalised companion of ensemble_rmsd.hip for ensemble diversity and coverage.
//
//   TM(a, b) = max over the evaluated superpositions (R proper, t) of (1/L) sum_i f_i,   f_i = 1 / (1 + |R a_i + t - b_i|^2 / d0^2).
//
// The search is fixed and has no data-dependent termination (DESIGN.md "TM-score"): every seed window (s, n) starts from weights 1 on
// residues s .. s+n-1, then 33 times: weighted Kabsch of a onto b (kabsch_f64.h), evaluate f and the score, w <- f^2.  f is convex in
// d^2, so the weighted least-squares problem is the exact maximiser of a minorant of the score and a reweighting never lowers it; the
// result is the maximum over all seeds and evaluations, a continuous function of the coordinates.  A heuristic like the original's
// shrinking cut-off search: a certified lower bound of the optimum, not the optimum.
//
// Mapping: one lane per (pair, seed).  A workgroup owns a 4 x 4 tile of pairs; the eight structures are widened to float64, moved to
// their own centroid (the search is translation invariant; this keeps sum w a b^T - (sum w a)(sum w b)^T / W free of cancellation for
// chains far from the origin) and staged once in LDS as [residue][coordinate][structure].  Wave = one b structure, 16-lane group = one
// a structure, lane in the group = seed: the four groups read neighbouring words, the lanes of a group get a broadcast.  One pass over
// the residues per iteration: d^2, f and the score under the current (R, t), and the 16 sums W, sum w a, sum w b, sum w a b^T of the
// next Kabsch with w = f^2.  The per-pair weights rule out the matrix instruction of the RMSD kernel: the loop is vector float64.  The
// 4 x 4 eigen-solve runs once per lane and iteration, never replicated.  No atomics, no host round trip; the order of every sum is
// fixed by the lane, so a value does not depend on the launch it is computed in.
#include <hip/hip_runtime.h>
#include <math.h>

#include "ensemble_common.h"
#include "kabsch_f64.h"
#include "str2str_hip.h"

namespace {

using namespace kabsch;

constexpr int TILE = 4;          // structures of each ensemble per workgroup
constexpr int SLOTS = 2 * TILE;  // LDS structure slots: a tile, then b tile
constexpr int ITERS = 33;
constexpr int MAX_SEEDS = 16;    // lanes per pair
constexpr int MAX_RES = S2S_TM_MAX_RES;

struct Seeds {
    int n;
    int start[MAX_SEEDS], len[MAX_SEEDS];
};

// The whole chain, then windows of L/2 and L/4 (at least 4) residues at half-window strides plus one flush with the end.
inline Seeds make_seeds(int L) {
    Seeds sd{};
    auto add = [&](int s, int n) {
        for (int k = 0; k < sd.n; ++k)
            if (sd.start[k] == s && sd.len[k] == n) return;   // (a duplicate window at small L: the maximum is unchanged)
        if (sd.n < MAX_SEEDS) { sd.start[sd.n] = s; sd.len[sd.n] = n; }
        ++sd.n;
    };
    add(0, L);
    for (int div = 2; div <= 4; div += 2) {
        const int n = L / div > 4 ? L / div : 4;
        if (n >= L) continue;
        const int stride = n / 2 > 1 ? n / 2 : 1;
        int s = 0, last = 0;
        for (; s + n <= L; s += stride) { add(s, n); last = s; }
        if (last + n < L) add(L - n, n);
    }
    return sd;
}

struct Sums {
    double w, a[3], b[3], ab[3][3];
    __device__ __forceinline__ void clear() {
        w = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a[c] = b[c] = 0.0;
#pragma unroll
            for (int e = 0; e < 3; ++e) ab[c][e] = 0.0;
        }
    }
    __device__ __forceinline__ void add(double wi, const double (&x)[3], const double (&y)[3]) {
        w += wi;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double wx = wi * x[c];
            a[c] += wx;
            b[c] += wi * y[c];
#pragma unroll
            for (int e = 0; e < 3; ++e) ab[c][e] += wx * y[e];
        }
    }
};

// grid (a tiles, b tiles), 256 threads.  row0 >= 0: the a ensemble is rows row0 .. of the b ensemble (a row chunk of a self matrix); a
// pair below the diagonal is then evaluated as its mirror pair (the two LDS slots exchanged), so the matrix is exactly symmetric and
// independent of the chunking.  mirror: the whole self matrix in one launch -- tiles below the diagonal are skipped and written by their
// mirror tile.  XFORM (n_b = 1): also the transform of the winning evaluation, xform[n_a, 12].
template <bool XFORM>
__global__ void __launch_bounds__(256) tm_pairs_kernel(const float* __restrict__ a, int n_a, const float* __restrict__ b, int n_b, int L,
                                                       Seeds seeds, double inv_d02, long long row0, int mirror, double* __restrict__ tm,
                                                       double* __restrict__ xform) {
    extern __shared__ double xs[];        // [L][3][SLOTS] centred coordinates, then [SLOTS][3] centroids
    double* cen = xs + (size_t)L * 3 * SLOTS;
    const int tid = threadIdx.x, bi = blockIdx.x, bj = blockIdx.y;
    if (mirror && bi > bj) return;        // (the whole workgroup, before the barrier)
    {
        const int slot = tid >> 5, sub = tid & 31;   // 32 threads stage one structure
        const bool of_a = slot < TILE;
        const long long g = of_a ? (long long)bi * TILE + slot : (long long)bj * TILE + slot - TILE;
        const bool valid = g < (of_a ? n_a : n_b);
        const float* p = (of_a ? a : b) + (valid ? (size_t)g * L * 3 : 0);
        double s[3] = {0.0, 0.0, 0.0};
        if (valid)
            for (int i = sub; i < L; i += 32) { s[0] += p[3 * i]; s[1] += p[3 * i + 1]; s[2] += p[3 * i + 2]; }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            for (int o = 16; o > 0; o >>= 1) s[c] += __shfl_xor(s[c], o, 64);
            s[c] /= (double)L;
        }
        for (int i = sub; i < L; i += 32)
#pragma unroll
            for (int c = 0; c < 3; ++c) xs[((size_t)i * 3 + c) * SLOTS + slot] = valid ? (double)p[3 * i + c] - s[c] : 0.0;
        if (sub < 3) cen[slot * 3 + sub] = sub == 0 ? s[0] : sub == 1 ? s[1] : s[2];
    }
    __syncthreads();

    const int lane = tid & 63, ia = lane >> 4, jb = tid >> 6, seed = lane & 15;
    const long long gi = (long long)bi * TILE + ia, gj = (long long)bj * TILE + jb;
    if (gj >= n_b) return;                // wave-uniform; no barrier below
    const bool swap = row0 >= 0 && row0 + gi > gj;
    const int sa = swap ? TILE + jb : ia, sb = swap ? ia : TILE + jb;
    const int sd = seed < seeds.n ? seed : 0;   // (spare lanes repeat the whole-chain seed)
    const int s0 = seeds.start[sd], s1 = s0 + seeds.len[sd];
    const double* pa = xs + sa;
    const double* pb = xs + sb;

    Sums S;
    S.clear();
    for (int i = 0; i < L; ++i) {
        double x[3], y[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { x[c] = pa[(i * 3 + c) * SLOTS]; y[c] = pb[(i * 3 + c) * SLOTS]; }
        S.add(i >= s0 && i < s1 ? 1.0 : 0.0, x, y);
    }

    double best = -1.0, bR[3][3], bt[3];
    for (int it = 0; it < ITERS; ++it) {
        const double iw = 1.0 / S.w;
        double abar[3], bbar[3], h[3][3], R[3][3], t[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { abar[c] = S.a[c] * iw; bbar[c] = S.b[c] * iw; }
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int e = 0; e < 3; ++e) h[c][e] = S.ab[c][e] - S.a[c] * bbar[e];
        horn_rotation(h, R);
#pragma unroll
        for (int c = 0; c < 3; ++c) t[c] = bbar[c] - (R[c][0] * abar[0] + R[c][1] * abar[1] + R[c][2] * abar[2]);
        S.clear();
        double score = 0.0;
        for (int i = 0; i < L; ++i) {
            double x[3], y[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { x[c] = pa[(i * 3 + c) * SLOTS]; y[c] = pb[(i * 3 + c) * SLOTS]; }
            double d2 = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double d = R[c][0] * x[0] + R[c][1] * x[1] + R[c][2] * x[2] + t[c] - y[c];
                d2 += d * d;
            }
            const double f = 1.0 / (1.0 + d2 * inv_d02);
            score += f;
            S.add(f * f, x, y);
        }
        score /= (double)L;
        if (score > best) {
            best = score;
            if (XFORM) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    bt[c] = t[c];
#pragma unroll
                    for (int e = 0; e < 3; ++e) bR[c][e] = R[c][e];
                }
            }
        }
    }

    double m = best;
    for (int o = 8; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));   // over the 16 seeds of the pair
    const bool valid = gi < n_a;
    if (seed == 0 && valid) {
        tm[(size_t)gi * n_b + gj] = m;
        if (mirror && bi < bj) tm[(size_t)gj * n_b + gi] = m;
    }
    if (XFORM) {
        const unsigned winners = (unsigned)(__ballot(best == m) >> (lane & 48)) & 0xffffu;
        if (valid && seed == __ffs(winners) - 1) {   // the first seed that reached the maximum
            double* o = xform + (size_t)gi * 12;
            const double* ca = cen + sa * 3;
            const double* cb = cen + sb * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                o[3 * c] = bR[c][0]; o[3 * c + 1] = bR[c][1]; o[3 * c + 2] = bR[c][2];
                o[9 + c] = bt[c] + cb[c] - (bR[c][0] * ca[0] + bR[c][1] * ca[1] + bR[c][2] * ca[2]);
            }
        }
    }
}

template <bool XFORM>
int launch(const float* a, int n_a, const float* b, int n_b, int L, double d0, long long row0, int mirror, double* tm, double* xform,
           hipStream_t st) {
    const long long ta = ((long long)n_a + TILE - 1) / TILE, tb = ((long long)n_b + TILE - 1) / TILE;
    if (L > MAX_RES || tb > 65535 || (long long)n_a * n_b >= (1ll << 31)) return (int)hipErrorInvalidValue;
    const Seeds seeds = make_seeds(L);
    if (seeds.n > MAX_SEEDS) return (int)hipErrorInvalidValue;
    if (!(d0 > 0.0)) d0 = L > 15 ? fmax(0.5, 1.24 * cbrt((double)L - 15.0) - 1.8) : 0.5;
    const size_t lds = ((size_t)L * 3 * SLOTS + SLOTS * 3) * sizeof(double);
    return ensemble::launch_dynamic_lds(tm_pairs_kernel<XFORM>, dim3((unsigned)ta, (unsigned)tb), dim3(256), lds, st, a, n_a, b, n_b, L, seeds,
                                        1.0 / (d0 * d0), row0, mirror, tm, xform);
}

}  // namespace

extern "C" int s2s_ca_tm_matrix(const float* a, int n_a, const float* b, int n_b, int n_res, double d0, double* tm, void* stream) {
    if (!a || !b || !tm || n_a < 1 || n_b < 1 || n_res < 1) return (int)hipErrorInvalidValue;
    const bool whole = a == b && n_a == n_b;
    return launch<false>(a, n_a, b, n_b, n_res, d0, ensemble::self_row0(a, b, n_a, n_b, n_res), whole ? 1 : 0, tm, nullptr, (hipStream_t)stream);
}

extern "C" int s2s_ca_tm_superpose(const float* mobile, int n_mobile, const float* target, int n_res, double d0, double* tm,
                                   double* xform12, void* stream) {
    if (!mobile || !target || !tm || !xform12 || n_mobile < 1 || n_res < 1) return (int)hipErrorInvalidValue;
    return launch<true>(mobile, n_mobile, target, 1, n_res, d0, -1, 0, tm, xform12, (hipStream_t)stream);
}
