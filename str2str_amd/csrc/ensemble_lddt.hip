// lDDT on CA atoms (Mariani et al. 2013; the reference's src/models/loss.py:384-460) on the device: the superposition-free companion of
// ensemble_rmsd.hip and ensemble_tm.hip for chains with a hinge, a floppy terminus or a disordered loop.
//
//   P(a) = {(i, j) : |i - j| >= min_seq_sep, d_a(i, j) < cutoff},   hits = sum over P(a) of #{t in {0.5, 1, 2, 4} : |d_a - d_b| < t},
//   lDDT(a -> b) = hits / (4 |P(a)|), 1.0 for an empty P(a); per residue the same with i fixed.  (include/str2str_hip.h has the definition.)
//
// One entry of the matrix costs O(L^2), and most of it would be spent on pairs farther apart than the cutoff.  Two passes:
//   list   one workgroup per reference structure, its widened coordinates in LDS.  The waves sweep the rows i > j; a __ballot and a prefix
//          popcount append (i, j, d_a) of every included pair to the structure's list in the caller's workspace, and count every residue's
//          partners.  An unordered pair is stored once and stands for both orders.  The order of the list depends on the interleaving of
//          the waves, nothing downstream does: everything after it is an integer sum.
//   score  one workgroup per (tile of TB models, run of reference structures).  The tile is staged once in LDS as float32 [model][residue][3].
//          Lanes stride over a list (coalesced; one read of an entry serves all TB models) and form the eight float64 bounds
//          (d_a + t)^2 and (d_a - t)^2 once per entry; per model two LDS points, v = |b_i - b_j|^2 in float64 and eight comparisons,
//          |d_a - d_b| < t  <=>  v < (d_a + t)^2 and (d_a - t < 0 or v > (d_a - t)^2): no square root in the inner loop.  One int32
//          counter per model in registers; the wave sums them by shuffles, the waves meet in LDS, one thread per model divides.
// No floating-point atomics, and no loop whose trip count depends on data other than the length of a list.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ensemble_common.h"
#include "str2str_hip.h"

namespace {

constexpr int MAX_RES = S2S_LDDT_MAX_RES;
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int TB_WIDE = 16, TB_NARROW = 8;        // models per tile
constexpr size_t HALF_CU_LDS = 80 * 1024;         // two workgroups per CU fit below it
constexpr int MAX_REFS_PER_WG = 8;
static_assert(MAX_RES <= 32768, "a list entry packs (i << 16) | j");
static_assert((size_t)MAX_RES * 12 * TB_NARROW + WAVES * TB_NARROW * 4 + (size_t)MAX_RES * 4 * TB_NARROW <= 160 * 1024, "the per-residue tile fits a CU");

// The workspace: d_a [n_a][slots] float64, then (i << 16 | j) [n_a][slots], list lengths [n_a][2] (the second word is padding), partner
// counts [n_a][L], all int32.
struct Lists {
    double* d;
    int* ij;
    int* n;
    int* partners;
    long long slots;
};

inline Lists carve(void* ws, long long n_a, long long L) {
    Lists l;
    l.slots = S2S_LDDT_LIST_SLOTS(L);
    l.d = (double*)ws;
    l.ij = (int*)(l.d + n_a * l.slots);
    l.n = l.ij + n_a * l.slots;
    l.partners = l.n + 2 * n_a;
    return l;
}

__global__ void __launch_bounds__(THREADS) lddt_list_kernel(const float* __restrict__ a, int L, double cutoff, int sep, Lists out) {
    extern __shared__ double xa[];                 // [L][3] widened coordinates, then int partners [L], then the fill count
    int* partners = (int*)(xa + (size_t)3 * L);
    int* fill = partners + L;
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* p = a + (size_t)s * L * 3;
    for (int k = tid; k < 3 * L; k += THREADS) xa[k] = (double)p[k];
    for (int k = tid; k < L; k += THREADS) partners[k] = 0;
    if (tid == 0) *fill = 0;
    __syncthreads();
    double* od = out.d + (size_t)s * out.slots;
    int* oij = out.ij + (size_t)s * out.slots;
    for (int i = sep + wave; i < L; i += WAVES) {  // (sep >= 1: row i pairs with j = 0 .. i - sep)
        const double x = xa[3 * i], y = xa[3 * i + 1], z = xa[3 * i + 2];
        const int jn = i - sep + 1;
        for (int j0 = 0; j0 < jn; j0 += 64) {
            const int j = j0 + lane;
            double d = 0.0;
            bool in = false;
            if (j < jn) {
                const double dx = x - xa[3 * j], dy = y - xa[3 * j + 1], dz = z - xa[3 * j + 2];
                d = sqrt((dx * dx + dy * dy) + dz * dz);
                in = d < cutoff;                   // (false for NaN)
            }
            const unsigned long long m = __ballot(in);
            if (m == 0) continue;                  // wave-uniform
            const int found = __popcll(m);
            int base = 0;
            if (lane == 0) {
                base = atomicAdd(fill, found);
                atomicAdd(&partners[i], found);
            }
            base = __shfl(base, 0, 64);
            if (in) {
                const int pos = base + __popcll(m & ((1ull << lane) - 1ull));   // at most L (L - 1) / 2 pairs exist: pos < slots
                od[pos] = d;
                oij[pos] = (i << 16) | j;
                atomicAdd(&partners[j], 1);
            }
        }
    }
    __syncthreads();
    if (tid == 0) out.n[2 * s] = *fill;
    for (int k = tid; k < L; k += THREADS) out.partners[(size_t)s * L + k] = partners[k];
}

// grid: tiles of b x runs of refs_per_wg reference structures, flattened (tile fastest).  PER_RES: also per_res [n_a, n_b, L].
template <int TB, bool PER_RES>
__global__ void __launch_bounds__(THREADS) lddt_score_kernel(const float* __restrict__ b, int n_b, int L, int n_a, int refs_per_wg, Lists in,
                                                             double* __restrict__ lddt, double* __restrict__ per_res) {
    extern __shared__ float xb[];                  // [TB][L][3] the tile, then int sums [WAVES][TB], then (PER_RES) int hit [TB][L]
    int* sums = (int*)(xb + (size_t)TB * L * 3);
    int* hit = sums + WAVES * TB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles = (n_b + TB - 1) / TB;
    const int tile = (int)(blockIdx.x % (unsigned)tiles), run = (int)(blockIdx.x / (unsigned)tiles);
    const int m0 = tile * TB, nm = n_b - m0 < TB ? n_b - m0 : TB;
    {
        const float* src = b + (size_t)m0 * L * 3;
        const int have = nm * L * 3;
        for (int k = tid; k < TB * L * 3; k += THREADS) xb[k] = k < have ? src[k] : 0.0f;   // (the slots past n_b are never written out)
    }
    const int r1 = (run + 1) * refs_per_wg < n_a ? (run + 1) * refs_per_wg : n_a;
    for (int r = run * refs_per_wg; r < r1; ++r) {
        if (PER_RES)
            for (int k = tid; k < TB * L; k += THREADS) hit[k] = 0;
        __syncthreads();                           // the tile (first round), hit cleared, sums free again
        const int n = in.n[2 * r];
        const double* ld = in.d + (size_t)r * in.slots;
        const int* lij = in.ij + (size_t)r * in.slots;
        int cnt[TB];
#pragma unroll
        for (int m = 0; m < TB; ++m) cnt[m] = 0;
        for (int e = tid; e < n; e += THREADS) {
            const double d = ld[e];
            const int ij = lij[e], i = ij >> 16, j = ij & 0xffff;
            const double l0 = d - 0.5, l1 = d - 1.0, l2 = d - 2.0, l3 = d - 4.0;
            const double lo0 = l0 < 0.0 ? -1.0 : l0 * l0, lo1 = l1 < 0.0 ? -1.0 : l1 * l1;   // (v >= 0 > -1: no lower bound)
            const double lo2 = l2 < 0.0 ? -1.0 : l2 * l2, lo3 = l3 < 0.0 ? -1.0 : l3 * l3;
            const double hi0 = (d + 0.5) * (d + 0.5), hi1 = (d + 1.0) * (d + 1.0), hi2 = (d + 2.0) * (d + 2.0), hi3 = (d + 4.0) * (d + 4.0);
            const float* pi = xb + 3 * i;
            const float* pj = xb + 3 * j;
#pragma unroll
            for (int m = 0; m < TB; ++m) {
                const double dx = (double)pi[m * L * 3] - (double)pj[m * L * 3];
                const double dy = (double)pi[m * L * 3 + 1] - (double)pj[m * L * 3 + 1];
                const double dz = (double)pi[m * L * 3 + 2] - (double)pj[m * L * 3 + 2];
                const double v = (dx * dx + dy * dy) + dz * dz;
                const int h = (int)(v < hi0 && v > lo0) + (int)(v < hi1 && v > lo1) + (int)(v < hi2 && v > lo2) + (int)(v < hi3 && v > lo3);
                cnt[m] += h;
                if (PER_RES && h) {
                    atomicAdd(&hit[m * L + i], h);
                    atomicAdd(&hit[m * L + j], h);
                }
            }
        }
#pragma unroll
        for (int m = 0; m < TB; ++m) {
            int c = cnt[m];
            for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
            if (lane == 0) sums[wave * TB + m] = c;
        }
        __syncthreads();
        if (tid < nm) {
            int h = 0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) h += sums[w * TB + tid];
            // (an unordered pair stands for both orders: 2 h / (4 * 2 n) is this same quotient)
            lddt[(size_t)r * n_b + m0 + tid] = n > 0 ? (double)h / (double)(4ll * n) : 1.0;
        }
        if (PER_RES) {
            const int* partners = in.partners + (size_t)r * L;
            for (int k = tid; k < nm * L; k += THREADS) {
                const int c = partners[k % L];
                per_res[((size_t)r * n_b + m0) * L + k] = c > 0 ? (double)hit[k] / (double)(4ll * c) : 1.0;
            }
        }
    }
}

template <int TB, bool PER_RES>
int launch_score(const float* b, int n_b, int L, int n_a, const Lists& lists, double* lddt, double* per_res, hipStream_t st) {
    const long long tiles = ((long long)n_b + TB - 1) / TB;
    long long refs = tiles * n_a / 4096;           // keep a few thousand workgroups before a tile starts serving several references
    refs = refs < 1 ? 1 : refs > MAX_REFS_PER_WG ? MAX_REFS_PER_WG : refs;
    const long long blocks = tiles * (((long long)n_a + refs - 1) / refs);
    const size_t lds = (size_t)TB * L * 12 + WAVES * TB * 4 + (PER_RES ? (size_t)TB * L * 4 : 0);
    return ensemble::launch_dynamic_lds(lddt_score_kernel<TB, PER_RES>, dim3((unsigned)blocks), dim3(THREADS), lds, st, b, n_b, L, n_a, (int)refs,
                                        lists, lddt, per_res);
}

template <bool PER_RES>
int run(const float* a, int n_a, const float* b, int n_b, int L, double cutoff, int sep, double* lddt, double* per_res, void* ws,
        long long ws_bytes, hipStream_t st) {
    if (!a || !b || !lddt || !ws || (PER_RES && !per_res) || n_a < 1 || n_b < 1 || L < 1 || L > MAX_RES) return (int)hipErrorInvalidValue;
    if (!(cutoff > 0.0) || !isfinite(cutoff) || sep < 1 || (long long)n_a * n_b >= (1ll << 31)) return (int)hipErrorInvalidValue;
    if (ws_bytes < S2S_LDDT_WORKSPACE_BYTES(n_a, L) || ((uintptr_t)ws & 7)) return (int)hipErrorInvalidValue;
    const Lists lists = carve(ws, n_a, L);
    hipLaunchKernelGGL(lddt_list_kernel, dim3((unsigned)n_a), dim3(THREADS), (size_t)L * 28 + 8, st, a, L, cutoff, sep, lists);
    const hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return (int)rc;
    // the wide tile while two workgroups of it share a CU, the narrow one above
    if ((size_t)L * 12 * TB_WIDE + WAVES * TB_WIDE * 4 <= HALF_CU_LDS) return launch_score<TB_WIDE, PER_RES>(b, n_b, L, n_a, lists, lddt, per_res, st);
    return launch_score<TB_NARROW, PER_RES>(b, n_b, L, n_a, lists, lddt, per_res, st);
}

}  // namespace

extern "C" int s2s_ca_lddt_matrix(const float* a, int n_a, const float* b, int n_b, int n_res, double cutoff, int min_seq_sep, double* lddt,
                                  void* workspace, long long workspace_bytes, void* stream) {
    return run<false>(a, n_a, b, n_b, n_res, cutoff, min_seq_sep, lddt, nullptr, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int s2s_ca_lddt_per_residue(const float* model, int n_model, const float* target, int n_res, double cutoff, int min_seq_sep,
                                       double* per_res, double* total, void* workspace, long long workspace_bytes, void* stream) {
    return run<true>(target, 1, model, n_model, n_res, cutoff, min_seq_sep, total, per_res, workspace, workspace_bytes, (hipStream_t)stream);
}
