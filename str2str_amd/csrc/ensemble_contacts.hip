// Contacts on CA atoms on the device: the contact map of an ensemble, per-structure contact statistics (number of contacts, contact order),
// the native contact list of one structure and the fraction of native contacts Q (hard, and the soft form of Best, Hummer and Eaton 2013)
// of every structure against it.  include/str2str_hip.h has the definitions.
//
//   v(i, j) = (dx dx + dy dy) + dz dz in float64 on the widened float32 coordinates;  contact(i, j)  <=>  j - i >= min_seq_sep and v < cutoff^2.
//
// Four kernels:
//   map     pair-major.  A workgroup owns a SIDE x SIDE tile of pairs (i, j) of the upper triangle (SIDE = 16 M, a thread owns M x M of
//           them) and walks the structures in batches of MAP_BATCH, whose i-rows and j-rows it stages in LDS as float64 planes: a thread
//           reads 3 M + 3 M words per structure for its M M pairs (lanes 0 .. 15 of a j read are consecutive words, an i read is a
//           broadcast).  Counts stay in registers as int32.  Without weights the structures are split over workgroups, which meet in
//           int32 global atomics.  With weights one workgroup (M = 1: the most tiles) walks ALL structures of the launch in ascending
//           order, every pair's float64 sum stays in one thread's register and starts from what the caller's buffer holds: a sequence of
//           launches over consecutive runs of structures is the one ascending sum.  A second small kernel mirrors the upper triangle into the lower.
//   stats   structure-major.  A workgroup stages a tile of S structures (S > 1 at short chains) as float64 planes x / y / z; the waves
//           share the rows i of a structure and their lanes sweep j.  Contacts are counted by a 64-wide ballot, separations summed as
//           integers; the waves meet in LDS integer atomics.
//   list    one workgroup: row counts (ballot), an exclusive scan over the rows, then the fill -- the list is in ascending (i, j) order
//           whatever the interleaving of the waves, because the soft sum below depends on the order of its terms.
//   q       a tile of Q_TILE structures in LDS as float32; threads stride over the list, so one entry (and its bound (lam d0)^2, formed
//           once) serves the whole tile.  Per (entry, structure) one sqrt and one exp in float64.  The soft sum is formed as
//           thread-strided partial sums in ascending entry order, the wave's xor tree, then the waves in turn: its order depends on the
//           list's length and this file's block shape alone, never on the launch.
// No floating-point atomics.  Built without contraction: every float64 operation rounds on its own, as in the numpy yardstick.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ensemble_common.h"
#include "str2str_hip.h"

namespace {

constexpr int MAX_RES = S2S_CONTACT_MAX_RES;
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int MAP_BATCH = 16;                     // structures staged per round of the map kernel
constexpr int MAP_TARGET_WORKGROUPS = 2048;       // what the unweighted map splits the structures for
constexpr int STATS_MAX_TILE = 16;                // structures per workgroup of the statistics kernel at short chains
constexpr int Q_TILE = 8;                         // structures per workgroup of the Q kernel
static_assert(MAX_RES <= 1024, "the scan of the list kernel gives every lane of one wave at most 16 rows");
static_assert((size_t)MAP_BATCH * 2 * 3 * 64 * 8 <= 64 * 1024, "the widest map tile fits static LDS");
static_assert((size_t)MAX_RES * 24 + STATS_MAX_TILE * 12 <= 64 * 1024, "a structure of the statistics kernel fits the default dynamic LDS");
static_assert((size_t)MAX_RES * 24 + ((size_t)MAX_RES + 1) * 4 <= 64 * 1024, "the native structure and its row offsets fit the default dynamic LDS");
static_assert((size_t)MAX_RES * 12 * Q_TILE + WAVES * Q_TILE * 12 <= 160 * 1024, "the tile of the Q kernel fits a CU");

__device__ __forceinline__ double sq_dist(double xi, double yi, double zi, double xj, double yj, double zj) {
    const double dx = xi - xj, dy = yi - yj, dz = zi - zj;
    return (dx * dx + dy * dy) + dz * dz;
}

// ------------------------------------------------------------------------------------------------------------------------ contact map
// grid: upper-triangular tiles x splits of the structures (tile fastest).  WEIGHTED: one split; counts and wsum are added into without
// atomics (a pair has one owner), and wsum continues the caller's ascending sum.
template <int M, bool WEIGHTED>
__global__ void __launch_bounds__(THREADS) contact_map_kernel(const float* __restrict__ ca, int R, int L, double c2, int sep,
                                                              const double* __restrict__ w, int per_split, int* __restrict__ counts,
                                                              double* __restrict__ wsum) {
    constexpr int SIDE = 16 * M;
    __shared__ double xs[MAP_BATCH][2][3][SIDE];   // [structure][i-rows | j-rows][x | y | z][residue of the tile]
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int nt = (L + SIDE - 1) / SIDE, tiles = nt * (nt + 1) / 2;
    const int tile = (int)(blockIdx.x % (unsigned)tiles), split = (int)(blockIdx.x / (unsigned)tiles);
    int bi = 0, bj = tile;
    while (bj >= nt - bi) {                       // row bi of the triangle holds nt - bi tiles
        bj -= nt - bi;
        ++bi;
    }
    bj += bi;
    const int i0 = bi * SIDE, j0 = bj * SIDE;
    if (j0 + SIDE - 1 - i0 < sep) return;          // the whole tile lies inside the band (uniform: before any barrier)
    const int s0 = split * per_split, s1 = s0 + per_split < R ? s0 + per_split : R;

    int cnt[M][M];
    double sum[M][M];
#pragma unroll
    for (int a = 0; a < M; ++a)
#pragma unroll
        for (int b = 0; b < M; ++b) {
            cnt[a][b] = 0;
            sum[a][b] = 0.0;
            if (WEIGHTED) {
                const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
                if (i < L && j < L && j - i >= sep) sum[a][b] = wsum[(size_t)i * L + j];
            }
        }

    for (int b0 = s0; b0 < s1; b0 += MAP_BATCH) {
        const int nb = s1 - b0 < MAP_BATCH ? s1 - b0 : MAP_BATCH;
        __syncthreads();                           // the previous batch has been read
        for (int k = tid; k < nb * 6 * SIDE; k += THREADS) {
            const int r = k % SIDE, c = (k / SIDE) % 3, side = (k / (3 * SIDE)) % 2, s = k / (6 * SIDE);
            const int res = (side ? j0 : i0) + r;
            xs[s][side][c][r] = res < L ? (double)ca[((size_t)(b0 + s) * L + res) * 3 + c] : 0.0;   // (pairs past L are never written out)
        }
        __syncthreads();
        for (int s = 0; s < nb; ++s) {
            double xi[M], yi[M], zi[M], xj[M], yj[M], zj[M];
#pragma unroll
            for (int a = 0; a < M; ++a) {
                xi[a] = xs[s][0][0][ty + 16 * a]; yi[a] = xs[s][0][1][ty + 16 * a]; zi[a] = xs[s][0][2][ty + 16 * a];
                xj[a] = xs[s][1][0][tx + 16 * a]; yj[a] = xs[s][1][1][tx + 16 * a]; zj[a] = xs[s][1][2][tx + 16 * a];
            }
            const double ws = WEIGHTED ? w[b0 + s] : 0.0;
#pragma unroll
            for (int a = 0; a < M; ++a)
#pragma unroll
                for (int b = 0; b < M; ++b) {
                    const bool in = sq_dist(xi[a], yi[a], zi[a], xj[b], yj[b], zj[b]) < c2;   // (false for NaN)
                    cnt[a][b] += (int)in;
                    if (WEIGHTED) sum[a][b] += in ? ws : 0.0;
                }
        }
    }

#pragma unroll
    for (int a = 0; a < M; ++a)
#pragma unroll
        for (int b = 0; b < M; ++b) {
            const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
            if (i < L && j < L && j - i >= sep) {
                const size_t o = (size_t)i * L + j;
                if (WEIGHTED) {
                    counts[o] += cnt[a][b];
                    wsum[o] = sum[a][b];
                } else if (cnt[a][b]) {
                    atomicAdd(&counts[o], cnt[a][b]);
                }
            }
        }
}

// lower triangle <- upper triangle (the band and the diagonal are never written by the map kernel and stay as the caller set them)
__global__ void __launch_bounds__(THREADS) contact_mirror_kernel(int L, int* __restrict__ counts, double* __restrict__ wsum) {
    const long long n = (long long)L * L;
    for (long long k = (long long)blockIdx.x * THREADS + threadIdx.x; k < n; k += (long long)gridDim.x * THREADS) {
        const int i = (int)(k / L), j = (int)(k % L);
        if (i > j) {
            counts[k] = counts[(size_t)j * L + i];
            if (wsum) wsum[k] = wsum[(size_t)j * L + i];
        }
    }
}

template <int M, bool WEIGHTED>
int launch_map(const float* ca, int R, int L, double c2, int sep, const double* w, int* counts, double* wsum, hipStream_t st) {
    constexpr int SIDE = 16 * M;
    const long long nt = (L + SIDE - 1) / SIDE, tiles = nt * (nt + 1) / 2, batches = ((long long)R + MAP_BATCH - 1) / MAP_BATCH;
    long long splits = WEIGHTED ? 1 : (MAP_TARGET_WORKGROUPS + tiles - 1) / tiles;
    splits = splits > batches ? batches : splits;
    const long long per_split = (batches + splits - 1) / splits * MAP_BATCH;   // whole batches
    splits = ((long long)R + per_split - 1) / per_split;
    hipLaunchKernelGGL((contact_map_kernel<M, WEIGHTED>), dim3((unsigned)(tiles * splits)), dim3(THREADS), 0, st, ca, R, L, c2, sep, w,
                       (int)per_split, counts, wsum);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------- per-structure contact statistics
// grid: tiles of S structures.  LDS: float64 planes [S][x | y | z][L], then the 64-bit separation sums [S], then the int counts [S].
__global__ void __launch_bounds__(THREADS) contact_stats_kernel(const float* __restrict__ ca, int R, int L, int S, double c2, int sep,
                                                                int* __restrict__ n_contacts, long long* __restrict__ sep_sum) {
    extern __shared__ double xs[];
    unsigned long long* sums = (unsigned long long*)(xs + (size_t)S * 3 * L);
    int* ns = (int*)(sums + S);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s0 = blockIdx.x * S, have = R - s0 < S ? R - s0 : S;
    for (int k = tid; k < have * 3 * L; k += THREADS) {
        const int r = k % L, c = (k / L) % 3, s = k / (3 * L);
        xs[k] = (double)ca[((size_t)(s0 + s) * L + r) * 3 + c];
    }
    if (tid < S) {
        sums[tid] = 0ull;
        ns[tid] = 0;
    }
    __syncthreads();
    for (int s = 0; s < have; ++s) {
        const double *x = xs + (size_t)s * 3 * L, *y = x + L, *z = y + L;
        int n = 0, sp = 0;                         // n: the wave's count (uniform); sp: this lane's separations (< L^2 / 64 * L: fits)
        for (int i = wave; i + sep < L; i += WAVES) {
            const double xi = x[i], yi = y[i], zi = z[i];
            for (int j0 = i + sep; j0 < L; j0 += 64) {
                const int j = j0 + lane;
                const bool in = j < L && sq_dist(xi, yi, zi, x[j], y[j], z[j]) < c2;   // (false for NaN)
                n += __popcll(__ballot(in));
                if (in) sp += j - i;
            }
        }
        const long long total = ensemble::wave_sum((long long)sp);
        if (lane == 0 && n) {
            atomicAdd(&ns[s], n);
            atomicAdd(&sums[s], (unsigned long long)total);
        }
    }
    __syncthreads();
    if (tid < have) {
        n_contacts[s0 + tid] = ns[tid];
        sep_sum[s0 + tid] = (long long)sums[tid];
    }
}

// ------------------------------------------------------------------------------------------------------------ native contact list
// One workgroup.  LDS: float64 planes [x | y | z][L], then int start [L + 1].
__global__ void __launch_bounds__(THREADS) native_list_kernel(const float* __restrict__ native, int L, double c2, int sep,
                                                              int* __restrict__ pairs, double* __restrict__ d0, int* __restrict__ n_out) {
    extern __shared__ double xs[];
    const double *x = xs, *y = xs + L, *z = xs + 2 * (size_t)L;
    int* start = (int*)(xs + 3 * (size_t)L);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < 3 * L; k += THREADS) xs[k] = (double)native[(size_t)(k % L) * 3 + k / L];
    __syncthreads();
    for (int i = wave; i < L; i += WAVES) {        // the number of contacts (i, j > i) of every row
        const double xi = x[i], yi = y[i], zi = z[i];
        int n = 0;
        for (int j0 = i + sep; j0 < L; j0 += 64) {
            const int j = j0 + lane;
            n += __popcll(__ballot(j < L && sq_dist(xi, yi, zi, x[j], y[j], z[j]) < c2));
        }
        if (lane == 0) start[i] = n;
    }
    __syncthreads();
    if (wave == 0) {                               // exclusive scan: a lane sums its run of rows, the wave scans the 64 sums
        const int per = (L + 63) / 64, r0 = lane * per, r1 = r0 + per < L ? r0 + per : L;
        int mine = 0;
        for (int r = r0; r < r1; ++r) mine += start[r];
        int incl = mine;
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        int run = incl - mine;
        for (int r = r0; r < r1; ++r) {
            const int n = start[r];
            start[r] = run;
            run += n;
        }
        if (lane == 63) {
            start[L] = incl;
            *n_out = incl;
        }
    }
    __syncthreads();
    for (int i = wave; i < L; i += WAVES) {        // the fill: rows ascending by construction, j ascending inside a row
        const double xi = x[i], yi = y[i], zi = z[i];
        int base = start[i];
        for (int j0 = i + sep; j0 < L; j0 += 64) {
            const int j = j0 + lane;
            double v = 0.0;
            bool in = false;
            if (j < L) {
                v = sq_dist(xi, yi, zi, x[j], y[j], z[j]);
                in = v < c2;
            }
            const unsigned long long m = __ballot(in);
            if (in) {
                const int pos = base + __popcll(m & ((1ull << lane) - 1ull));   // < start[i + 1] <= slots: the same decisions as the count
                pairs[2 * (size_t)pos] = i;
                pairs[2 * (size_t)pos + 1] = j;
                d0[pos] = sqrt(v);
            }
            base += __popcll(m);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- fraction of native contacts
// grid: tiles of Q_TILE structures.  LDS: float32 [Q_TILE][L][3], then double part [WAVES][Q_TILE], then int hit [WAVES][Q_TILE].
__global__ void __launch_bounds__(THREADS) native_q_kernel(const float* __restrict__ ca, int R, int L, const int* __restrict__ pairs,
                                                           const double* __restrict__ d0, int n, double beta, double lam,
                                                           double* __restrict__ q_soft, double* __restrict__ q_hard, int* __restrict__ hits) {
    extern __shared__ float xb[];
    double* part = (double*)(xb + (size_t)Q_TILE * L * 3);
    int* hit = (int*)(part + WAVES * Q_TILE);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * Q_TILE, nm = R - m0 < Q_TILE ? R - m0 : Q_TILE;
    {
        const float* src = ca + (size_t)m0 * L * 3;
        const int have = nm * L * 3;
        for (int k = tid; k < Q_TILE * L * 3; k += THREADS) xb[k] = k < have ? src[k] : 0.0f;   // (the slots past R are never written out)
    }
    __syncthreads();
    double acc[Q_TILE];
    int cnt[Q_TILE];
#pragma unroll
    for (int m = 0; m < Q_TILE; ++m) {
        acc[m] = 0.0;
        cnt[m] = 0;
    }
    for (int e = tid; e < n; e += THREADS) {       // ascending entries per thread
        const int i = pairs[2 * (size_t)e], j = pairs[2 * (size_t)e + 1];
        if ((unsigned)i >= (unsigned)L || (unsigned)j >= (unsigned)L) continue;   // not an entry of a list of this chain: nothing is read
        const double b = lam * d0[e], b2 = b * b;
        const float* pi = xb + 3 * i;
        const float* pj = xb + 3 * j;
#pragma unroll
        for (int m = 0; m < Q_TILE; ++m) {
            const double v = sq_dist((double)pi[m * L * 3], (double)pi[m * L * 3 + 1], (double)pi[m * L * 3 + 2], (double)pj[m * L * 3],
                                     (double)pj[m * L * 3 + 1], (double)pj[m * L * 3 + 2]);
            cnt[m] += (int)(v < b2);               // (false for NaN)
            acc[m] += 1.0 / (1.0 + exp(beta * (sqrt(v) - b)));
        }
    }
#pragma unroll
    for (int m = 0; m < Q_TILE; ++m) {
        const double a = ensemble::wave_sum(acc[m]);
        const int c = ensemble::wave_sum(cnt[m]);
        if (lane == 0) {
            part[wave * Q_TILE + m] = a;
            hit[wave * Q_TILE + m] = c;
        }
    }
    __syncthreads();
    if (tid < nm) {
        double a = part[tid];
        int c = hit[tid];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {          // the waves in turn
            a += part[w * Q_TILE + tid];
            c += hit[w * Q_TILE + tid];
        }
        q_soft[m0 + tid] = n > 0 ? a / (double)n : 1.0;
        q_hard[m0 + tid] = n > 0 ? (double)c / (double)n : 1.0;
        hits[m0 + tid] = c;
    }
}

inline bool positive_finite(double v) { return v > 0.0 && isfinite(v); }

// No pair is n_res apart: a larger separation means the same empty set, and i + sep stays far from overflow in the kernels.
inline int clamp_sep(int sep, int n_res) { return sep < n_res ? sep : n_res; }

}  // namespace

extern "C" int s2s_ca_contact_map(const float* ca, int n, int n_res, double cutoff, int min_seq_sep, const double* weights, int* counts,
                                  double* weighted, void* stream) {
    if (!ca || !counts || (weights != nullptr) != (weighted != nullptr) || n < 1 || n > S2S_CONTACT_MAX_STRUCTURES || n_res < 1 || n_res > MAX_RES)
        return (int)hipErrorInvalidValue;
    if (!positive_finite(cutoff) || min_seq_sep < 1) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const double c2 = cutoff * cutoff;
    min_seq_sep = clamp_sep(min_seq_sep, n_res);
    int rc;
    if (weights) {                                 // one workgroup per tile and no split: the smallest tile gives the most workgroups
        rc = launch_map<1, true>(ca, n, n_res, c2, min_seq_sep, weights, counts, weighted, st);
    } else {                                       // the largest tile that the chain fills at least half of
        rc = n_res > 32   ? launch_map<4, false>(ca, n, n_res, c2, min_seq_sep, nullptr, counts, nullptr, st)
             : n_res > 16 ? launch_map<2, false>(ca, n, n_res, c2, min_seq_sep, nullptr, counts, nullptr, st)
                          : launch_map<1, false>(ca, n, n_res, c2, min_seq_sep, nullptr, counts, nullptr, st);
    }
    if (rc != 0) return rc;
    const long long cells = (long long)n_res * n_res;
    hipLaunchKernelGGL(contact_mirror_kernel, dim3((unsigned)((cells + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, n_res, counts, weighted);
    return (int)hipGetLastError();
}

extern "C" int s2s_ca_contact_stats(const float* ca, int n, int n_res, double cutoff, int min_seq_sep, int* n_contacts, long long* sep_sum,
                                    void* stream) {
    if (!ca || !n_contacts || !sep_sum || n < 1 || n_res < 1 || n_res > MAX_RES) return (int)hipErrorInvalidValue;
    if (!positive_finite(cutoff) || min_seq_sep < 1) return (int)hipErrorInvalidValue;
    min_seq_sep = clamp_sep(min_seq_sep, n_res);
    int S = THREADS / n_res;                       // enough rows for the four waves at short chains
    S = S < 1 ? 1 : S > STATS_MAX_TILE ? STATS_MAX_TILE : S;
    const size_t lds = (size_t)S * 3 * n_res * 8 + (size_t)S * 12;
    hipLaunchKernelGGL(contact_stats_kernel, dim3((unsigned)(((long long)n + S - 1) / S)), dim3(THREADS), lds, (hipStream_t)stream, ca, n, n_res, S,
                       cutoff * cutoff, min_seq_sep, n_contacts, sep_sum);
    return (int)hipGetLastError();
}

extern "C" int s2s_ca_native_contacts(const float* native, int n_res, double cutoff, int min_seq_sep, int* pairs, double* d0, int* n_pairs,
                                      void* stream) {
    if (!native || !pairs || !d0 || !n_pairs || n_res < 1 || n_res > MAX_RES) return (int)hipErrorInvalidValue;
    if (!positive_finite(cutoff) || min_seq_sep < 1) return (int)hipErrorInvalidValue;
    min_seq_sep = clamp_sep(min_seq_sep, n_res);
    const size_t lds = (size_t)n_res * 24 + ((size_t)n_res + 1) * 4;
    hipLaunchKernelGGL(native_list_kernel, dim3(1), dim3(THREADS), lds, (hipStream_t)stream, native, n_res, cutoff * cutoff, min_seq_sep, pairs,
                       d0, n_pairs);
    return (int)hipGetLastError();
}

extern "C" int s2s_ca_native_q(const float* ca, int n, int n_res, const int* pairs, const double* d0, int n_pairs, double beta, double lam,
                               double* q_soft, double* q_hard, int* hits, void* stream) {
    if (!ca || !q_soft || !q_hard || !hits || n < 1 || n_res < 1 || n_res > MAX_RES || n_pairs < 0) return (int)hipErrorInvalidValue;
    if ((n_pairs > 0 && (!pairs || !d0)) || n_pairs > S2S_CONTACT_LIST_SLOTS(n_res) || !positive_finite(beta) || !positive_finite(lam))
        return (int)hipErrorInvalidValue;
    const size_t lds = (size_t)Q_TILE * n_res * 12 + WAVES * Q_TILE * 12;
    return ensemble::launch_dynamic_lds(native_q_kernel, dim3((unsigned)(((long long)n + Q_TILE - 1) / Q_TILE)), dim3(THREADS), lds,
                                        (hipStream_t)stream, ca, n, n_res, pairs, d0, n_pairs, beta, lam, q_soft, q_hard, hits);
}
