// Solution scattering of CA-bead structures on the device: the Debye (1915) intensity I(q) and the Kirkwood mean inverse distance behind
// the hydrodynamic radius.  No counterpart in the reference.  include/str2str_hip.h has the definition; float64 arithmetic on the float32
// coordinates, contraction off (build.py), so the argument a = q r of every sine is the float64 numpy value.
//
// A workgroup of 256 threads owns one (structure, tile of 16 q-values).  The structure is staged once in LDS, widened, as three float64
// planes (8-byte stride between lanes: no bank conflict), next to the residues' types, the tile's q-values and the tile's slice of the
// form-factor table.  Thread t walks the pairs i < j of the flattened upper triangle, t, t + 256, ... in ascending order (so a short row
// idles no lane), forms r once per pair and keeps one accumulator per q-value of the tile in registers.  The workgroups of tile 0 also
// add 1 / r when the caller asks for it; that branch is the same for the whole workgroup.
// Sums: the xor tree of a wave, then the four waves in turn; thread k of the workgroup adds the diagonal of q-value k in ascending i.  The
// order depends on n_res and the block shape only, and a q-value's sum on nothing but that q-value: no floating-point atomics.
// What this is NOT: no hydration shell, no excluded-volume term, no built-in residue form-factor table, no side chains, no Nygaard or
// other correction of the Kirkwood value.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ensemble_common.h"
#include "str2str_hip.h"

namespace {

using ensemble::wave_sum;

constexpr int MAX_RES = S2S_SAXS_MAX_RES, MAX_Q = S2S_SAXS_MAX_Q, MAX_TYPES = S2S_SAXS_MAX_TYPES;
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int TILE = 16;             // q-values of a workgroup: one float64 accumulator each per thread

constexpr size_t lds_bytes(int L, int n_types) {
    return (size_t)L * (3 * 8 + 4) + (size_t)n_types * TILE * 8 + TILE * 8 + (size_t)WAVES * (TILE + 1) * 8 + 8;
}
static_assert(lds_bytes(MAX_RES, MAX_TYPES) <= 64 * 1024, "the longest chain and the largest table fit the default LDS limit");

struct Params {
    const float* ca;
    const double* q;
    int n_q;
    const int* types;
    const double* table;
    int n_types;
    double* intensity;
    double* inv_r_mean;
};

__global__ void __launch_bounds__(THREADS) saxs_kernel(int L, Params p) {
    extern __shared__ double lds[];
    double* xs = lds;                          // [L] per plane
    double* ys = xs + L;
    double* zs = ys + L;
    double* tab = zs + L;                      // [n_types][TILE] the tile's slice of the table, 0.0 past n_q
    double* qs = tab + p.n_types * TILE;       // [TILE]
    double* red = qs + TILE;                   // [WAVES][TILE + 1]
    int* ty = (int*)(red + WAVES * (TILE + 1)); // [L]
    const int s = blockIdx.x, q0 = blockIdx.y * TILE, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nk = min(TILE, p.n_q - q0);      // the q-values of this tile (the same for the whole workgroup)
    const bool with_inv = p.inv_r_mean != nullptr && blockIdx.y == 0;

    const float* src = p.ca + (size_t)s * L * 3;
    for (int k = tid; k < 3 * L; k += THREADS) {
        const int i = k / 3, c = k - 3 * i;
        (c == 0 ? xs : c == 1 ? ys : zs)[i] = (double)src[k];
    }
    for (int i = tid; i < L; i += THREADS) ty[i] = min(max(p.types[i], 0), p.n_types - 1);   // (the binding rejects a type outside the table)
    for (int k = tid; k < p.n_types * TILE; k += THREADS) {
        const int t = k / TILE, c = k - TILE * t;
        tab[k] = c < nk ? p.table[(size_t)t * p.n_q + q0 + c] : 0.0;
    }
    if (tid < TILE) qs[tid] = tid < nk ? p.q[q0 + tid] : 0.0;
    __syncthreads();

    double acc[TILE], inv = 0.0;
#pragma unroll
    for (int k = 0; k < TILE; ++k) acc[k] = 0.0;
    const long long n_pairs = (long long)L * (L - 1) / 2;
    int i = 0, off = tid;                      // the pair (i, i + 1 + off): row i of the upper triangle has L - 1 - i entries
    for (long long pair = tid; pair < n_pairs; pair += THREADS) {
        while (off >= L - 1 - i) {             // (ends: pair < n_pairs puts it in a row before the last)
            off -= L - 1 - i;
            ++i;
        }
        const int j = i + 1 + off;
        const double dx = xs[i] - xs[j], dy = ys[i] - ys[j], dz = zs[i] - zs[j];
        const double r = sqrt((dx * dx + dy * dy) + dz * dz);
        const double* fi = tab + ty[i] * TILE;
        const double* fj = tab + ty[j] * TILE;
#pragma unroll
        for (int k = 0; k < TILE; ++k) {
            if (k < nk) {
                const double a = qs[k] * r;
                const double sinc = a == 0.0 ? 1.0 : sin(a) / a;
                acc[k] += (fi[k] * fj[k]) * sinc;
            }
        }
        if (with_inv) inv += 1.0 / r;
        off += THREADS;
    }

#pragma unroll
    for (int k = 0; k < TILE; ++k) {
        const double v = wave_sum(acc[k]);
        if (lane == 0) red[wave * (TILE + 1) + k] = v;
    }
    inv = wave_sum(inv);
    if (lane == 0) red[wave * (TILE + 1) + TILE] = inv;
    __syncthreads();

    if (tid <= TILE && (tid < nk || (tid == TILE && with_inv))) {
        double sum = 0.0;
        for (int w = 0; w < WAVES; ++w) sum += red[w * (TILE + 1) + tid];
        // |x_i - x_i|^2 is 0.0 for a finite bead and NaN otherwise: added to the diagonal it leaves f^2 as it is or makes the structure NaN
        // even where it has no pair (n_res = 1)
        double diag = 0.0;
        for (int b = 0; b < L; ++b) {
            const double dx = xs[b] - xs[b], dy = ys[b] - ys[b], dz = zs[b] - zs[b];
            const double self = (dx * dx + dy * dy) + dz * dz;
            const double f = tid < TILE ? tab[ty[b] * TILE + tid] : 0.0;
            diag += f * f + self;
        }
        if (tid < TILE) p.intensity[(size_t)s * p.n_q + q0 + tid] = diag + 2.0 * sum;
        else p.inv_r_mean[s] = (2.0 * sum) / ((double)L * (double)L) + diag;
    }
}

}  // namespace

extern "C" int s2s_ca_scattering(const float* ca, int n, int n_res, const double* q, int n_q, const int* types, const double* table, int n_types,
                                 double* intensity, double* inv_r_mean, void* stream) {
    if (!ca || !q || !types || !table || !intensity || n < 1 || n_res < 1 || n_res > MAX_RES || n_q < 1 || n_q > MAX_Q || n_types < 1 ||
        n_types > MAX_TYPES)
        return (int)hipErrorInvalidValue;
    const Params p = {ca, q, n_q, types, table, n_types, intensity, inv_r_mean};
    return ensemble::launch_dynamic_lds(saxs_kernel, dim3((unsigned)n, (unsigned)((n_q + TILE - 1) / TILE)), dim3(THREADS),
                                        lds_bytes(n_res, n_types), (hipStream_t)stream, n_res, p);
}
