// Backbone violations (the reference's between_residue_bond_loss, between_residue_clash_loss and extreme_ca_ca_distance_violations,
// src/models/loss.py:714-1017, 1237-1314, restricted to the atoms the sampler writes: N, CA, C, O, CB) on the device.  Where the ensemble
// scores of ensemble_rmsd / _tm / _lddt.hip compare structures with each other, this one looks inside each structure.
// include/str2str_hip.h has the definition; float64 arithmetic on the float32 coordinates, contraction off (build.py), so every term is the
// float64 numpy value and masks and counts are exact integers.
//
// One workgroup per structure.  Its 5 L atoms are staged once in LDS, widened, as three planes x / y / z (8-byte stride between lanes: no
// bank conflict, where 24-byte records would need care), then
//   connections  one thread per consecutive pair: the C-N length, the two cosines, the CA-CA step.  O(L).
//   sweep        a wave owns the rows i = wave, wave + WAVES, ...; its lanes test the residue pairs (i, j > i) against the exact prefilter
//                d(CA_i, CA_j) < rho_i + rho_j + (3.4 - clash_tolerance), rho = the largest distance of a residue's existing atoms from
//                its CA.  A __ballot and a prefix popcount append the survivors, in order, to the wave's ring in LDS; whenever 64 are
//                waiting every lane takes one and expands its 25 atom pairs.
// Sums: a loss term is non-zero exactly where the pair clashes, so a surviving pair's 25 terms are summed by its lane in (a, b) order, the
// pairs of a row are folded in ascending j into the row's own LDS slot by one lane (the ring keeps the order; pairs the prefilter dropped
// would have added exact zeros), and the rows meet in a fixed tree.  The order depends on L only; no floating-point atomics.  Masks and
// counts use integer LDS atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ensemble_common.h"
#include "str2str_hip.h"

namespace {

using ensemble::wave_sum;

constexpr int MAX_RES = S2S_VIOL_MAX_RES;
constexpr int THREADS_SHORT = 512, THREADS_LONG = 1024, SHORT_RES = 256;   // chains up to SHORT_RES: three workgroups share a CU
constexpr int RING = 128;                                                  // survivors a wave holds: fewer than 64 waiting + 64 new
constexpr int N_ATOMS = 5;                                                 // N, CA, C, O, CB (atom14 slots 0 .. 4)
constexpr int PRO = 14;                                                    // (aatype of proline in the reference's residue order)
constexpr int EXIST_BITS = 0x1f, CLASH_SHIFT = 5, VIOL_BIT = 1 << 10, PRO_BIT = 1 << 11;
enum { C_PAIRS, C_CLASHES, C_CN, C_CACN, C_CNCA, C_CA_MASK, C_CA_VIOL, C_BOND_RES, C_CLASH_RES, C_UNION_RES, N_COUNTERS };

constexpr size_t lds_bytes(int L, int threads) {
    return (size_t)L * (3 * N_ATOMS * 8 + 8 + 8 + 4 + 4) + 16 * 8 + (size_t)(threads / 64) * RING * 4 + N_COUNTERS * 4;
}
static_assert(lds_bytes(MAX_RES, THREADS_LONG) <= 160 * 1024, "a structure of S2S_VIOL_MAX_RES residues fits the LDS of a CU");
static_assert(MAX_RES < 65536, "a ring entry packs (i << 16) | j");

struct Params {
    const float* atoms;
    const unsigned char* exists;
    const int* aatype;
    const int* residue_index;
    double tol_factor, clash_tol;
    double* losses;
    double* fractions;
    double* per_res_loss;
    unsigned char* bond_mask;
    unsigned char* clash_mask;
    int* n_clash_pairs;
};

// The sum over the workgroup in a fixed order: the xor tree of a wave, then the waves in turn.  Every thread returns the same value.
template <int WAVES>
__device__ double block_sum(double v, double* red, int lane, int wave) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < WAVES; ++w) t += red[w];
    __syncthreads();
    return t;
}

// The C-N peptide bond of two residues numbered n and n + 1 is no clash: its slots (`a` of residue i, `b` of residue j), -1 if there is none.
__device__ inline void bonded_slots(int ri_i, int ri_j, int& a, int& b) {
    a = b = -1;
    if ((long long)ri_j == (long long)ri_i + 1) { a = 2; b = 0; }
    else if ((long long)ri_i == (long long)ri_j + 1) { a = 0; b = 2; }
}

template <int THREADS>
__global__ void __launch_bounds__(THREADS) violations_kernel(int L, Params p) {
    constexpr int WAVES = THREADS / 64;
    extern __shared__ double lds[];
    const int A = N_ATOMS * L;
    double* xs = lds;                  // [5 L] per plane
    double* ys = xs + A;
    double* zs = ys + A;
    double* rho = zs + A;              // [L]
    double* slot = rho + L;            // [L] the connections' loss sums, later the rows' clash sums
    double* red = slot + L;            // [16]
    int* flags = (int*)(red + 16);     // [L] bits 0-4 atom exists, 5-9 atom clashes, 10 the connection to the next residue is violated, 11 PRO
    int* ri = flags + L;               // [L]
    int* ring = ri + L;                // [WAVES][RING]
    int* counters = ring + WAVES * RING;
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    {
        const float* src = p.atoms + (size_t)s * A * 3;
        for (int k = tid; k < 3 * A; k += THREADS) {
            const int atom = k / 3, c = k - 3 * atom;
            (c == 0 ? xs : c == 1 ? ys : zs)[atom] = (double)src[k];
        }
    }
    for (int r = tid; r < L; r += THREADS) {
        int f = p.aatype[r] == PRO ? PRO_BIT : 0;
        for (int a = 0; a < N_ATOMS; ++a) f |= (p.exists[r * N_ATOMS + a] != 0) << a;
        flags[r] = f;
        ri[r] = p.residue_index[r];
        slot[r] = 0.0;
    }
    if (tid < N_COUNTERS) counters[tid] = 0;
    __syncthreads();

    // ---- the prefilter's radii, and the connections k -> k + 1
    for (int r = tid; r < L; r += THREADS) {
        const int f = flags[r];
        double m = 0.0;
        for (int a = 0; a < N_ATOMS; ++a) {
            if (a == 1 || !((f >> a) & 1)) continue;
            const double dx = xs[5 * r + a] - xs[5 * r + 1], dy = ys[5 * r + a] - ys[5 * r + 1], dz = zs[5 * r + a] - zs[5 * r + 1];
            m = fmax(m, sqrt((dx * dx + dy * dy) + dz * dz));
        }
        rho[r] = m;
    }
    double sum_cn = 0.0, sum_cacn = 0.0, sum_cnca = 0.0;
    int n_cn = 0, n_cacn = 0, n_cnca = 0, n_ca = 0, n_ca_viol = 0;
    for (int k = tid; k < L - 1; k += THREADS) {
        constexpr double EPS = 1e-6;
        const int f0 = flags[k], f1 = flags[k + 1];
        const bool no_gap = (long long)ri[k + 1] - (long long)ri[k] == 1;
        const int ca0 = 5 * k + 1, c0 = 5 * k + 2, n1 = 5 * k + 5, ca1 = 5 * k + 6;
        const double cnx = xs[n1] - xs[c0], cny = ys[n1] - ys[c0], cnz = zs[n1] - zs[c0];            // next N - this C
        const double cax = xs[ca0] - xs[c0], cay = ys[ca0] - ys[c0], caz = zs[ca0] - zs[c0];         // this CA - this C
        const double nax = xs[ca1] - xs[n1], nay = ys[ca1] - ys[n1], naz = zs[ca1] - zs[n1];         // next CA - next N
        const double c_n = sqrt(EPS + ((cnx * cnx + cny * cny) + cnz * cnz));
        const double ca_c = sqrt(EPS + ((cax * cax + cay * cay) + caz * caz));
        const double n_ca_len = sqrt(EPS + ((nax * nax + nay * nay) + naz * naz));
        const bool pro = f1 & PRO_BIT;
        const double gt = pro ? 1.341 : 1.329, sd = pro ? 0.016 : 0.014;
        const double e_cn = sqrt(EPS + (c_n - gt) * (c_n - gt));
        const double ux = cnx / c_n, uy = cny / c_n, uz = cnz / c_n;
        const double cos_cacn = ((cax / ca_c) * ux + (cay / ca_c) * uy) + (caz / ca_c) * uz;
        const double cos_cnca = ((-ux) * (nax / n_ca_len) + (-uy) * (nay / n_ca_len)) + (-uz) * (naz / n_ca_len);
        const double e_cacn = sqrt(EPS + (cos_cacn - -0.4473) * (cos_cacn - -0.4473));
        const double e_cnca = sqrt(EPS + (cos_cnca - -0.5203) * (cos_cnca - -0.5203));
        // The widths are the reference's own: its CA-C-N term takes the C-N bond-length stddev 0.014 (loss.py:809, not the 0.0311 of its
        // cosine table), its C-N-CA term the cosine's 0.0353 (:826).  This restates that definition; it is not a slip to be repaired here.
        const double w_cn = p.tol_factor * sd, w_cacn = p.tol_factor * 0.014, w_cnca = p.tol_factor * 0.0353;
        const double l_cn = fmax(e_cn - w_cn, 0.0), l_cacn = fmax(e_cacn - w_cacn, 0.0), l_cnca = fmax(e_cnca - w_cnca, 0.0);
        const bool m_cn = no_gap && (f0 & 4) && (f1 & 1), m_cacn = m_cn && (f0 & 2), m_cnca = m_cn && (f1 & 2);
        if (m_cn) { sum_cn += l_cn; ++n_cn; }
        if (m_cacn) { sum_cacn += l_cacn; ++n_cacn; }
        if (m_cnca) { sum_cnca += l_cnca; ++n_cnca; }
        if ((m_cn && e_cn > w_cn) || (m_cacn && e_cacn > w_cacn) || (m_cnca && e_cnca > w_cnca)) atomicOr(&flags[k], VIOL_BIT);
        slot[k] = (l_cn + l_cacn) + l_cnca;       // (unmasked, as the reference's per_residue_loss_sum is)
        if (no_gap && (f0 & 2) && (f1 & 2)) {
            const double dx = xs[ca0] - xs[ca1], dy = ys[ca0] - ys[ca1], dz = zs[ca0] - zs[ca1];
            ++n_ca;
            n_ca_viol += (sqrt(EPS + ((dx * dx + dy * dy) + dz * dz)) - 3.80209737096) > 1.5;
        }
    }
    {
        const int c[5] = {wave_sum(n_cn), wave_sum(n_cacn), wave_sum(n_cnca), wave_sum(n_ca), wave_sum(n_ca_viol)};
        if (lane == 0)
            for (int q = 0; q < 5; ++q)
                if (c[q]) atomicAdd(&counters[C_CN + q], c[q]);
    }
    sum_cn = block_sum<WAVES>(sum_cn, red, lane, wave);        // (its barriers also publish slot, flags and the counters)
    sum_cacn = block_sum<WAVES>(sum_cacn, red, lane, wave);
    sum_cnca = block_sum<WAVES>(sum_cnca, red, lane, wave);
    if (tid == 0) {
        p.losses[4 * (size_t)s + 0] = sum_cn / ((double)counters[C_CN] + 1e-6);
        p.losses[4 * (size_t)s + 1] = sum_cacn / ((double)counters[C_CACN] + 1e-6);
        p.losses[4 * (size_t)s + 2] = sum_cnca / ((double)counters[C_CNCA] + 1e-6);
    }
    for (int r = tid; r < L; r += THREADS)        // half of each connection's loss to either residue
        p.per_res_loss[(size_t)s * L + r] = 0.5 * ((r < L - 1 ? slot[r] : 0.0) + (r > 0 ? slot[r - 1] : 0.0));
    __syncthreads();
    for (int r = tid; r < L; r += THREADS) slot[r] = 0.0;
    __syncthreads();

    // ---- clashes: the prefilter sweep and the expansion of its survivors
    const double reach = (3.4 - p.clash_tol) + 1e-9;            // twice the largest radius; the slack covers the rounding of the test itself
    constexpr double RAD[N_ATOMS] = {1.55, 1.7, 1.7, 1.52, 1.7};
    int* my_ring = ring + wave * RING;
    int head = 0, waiting = 0, n_pairs = 0, n_clashes = 0;

    auto expand = [&](int n) {                                  // the first n <= 64 entries of the ring, one per lane
        double sum = 0.0;
        int i = 0;
        if (lane < n) {
            const int e = my_ring[(head + lane) & (RING - 1)], j = e & 0xffff;
            i = e >> 16;
            const int fi = flags[i], fj = flags[j];
            int skip_a, skip_b;
            bonded_slots(ri[i], ri[j], skip_a, skip_b);
            double jx[N_ATOMS], jy[N_ATOMS], jz[N_ATOMS];
#pragma unroll
            for (int b = 0; b < N_ATOMS; ++b) { jx[b] = xs[5 * j + b]; jy[b] = ys[5 * j + b]; jz[b] = zs[5 * j + b]; }
            int hit_i = 0, hit_j = 0, c = 0;
#pragma unroll
            for (int a = 0; a < N_ATOMS; ++a) {
                if (!((fi >> a) & 1)) continue;
                const double ax = xs[5 * i + a], ay = ys[5 * i + a], az = zs[5 * i + a];
#pragma unroll
                for (int b = 0; b < N_ATOMS; ++b) {
                    if (!((fj >> b) & 1) || (a == skip_a && b == skip_b)) continue;
                    const double dx = ax - jx[b], dy = ay - jy[b], dz = az - jz[b];
                    const double d = sqrt(1e-10 + ((dx * dx + dy * dy) + dz * dz));
                    const double bound = (RAD[a] + RAD[b]) - p.clash_tol;
                    if (d < bound) {                            // (false for NaN)
                        sum += bound - d;
                        ++c;
                        hit_i |= 1 << a;
                        hit_j |= 1 << b;
                    }
                }
            }
            if (c) {
                n_clashes += c;
                atomicOr(&flags[i], hit_i << CLASH_SHIFT);
                atomicOr(&flags[j], hit_j << CLASH_SHIFT);
            }
        }
        // the clashing pairs' sums into their rows, in the ring's order: ascending j within a row, and a row belongs to this wave alone
        unsigned long long nz = __ballot(sum != 0.0);
        while (nz) {
            const int l = __ffsll((long long)nz) - 1;
            const double v = __shfl(sum, l, 64);
            const int row = __shfl(i, l, 64);
            if (lane == 0) slot[row] += v;
            nz &= nz - 1;
        }
        head = (head + n) & (RING - 1);
        waiting -= n;
    };

    for (int i = wave; i < L - 1; i += WAVES) {
        const double cx = xs[5 * i + 1], cy = ys[5 * i + 1], cz = zs[5 * i + 1], rho_i = rho[i];
        const int fi = flags[i] & EXIST_BITS, ri_i = ri[i], n_i = __popc(fi);
        for (int j0 = i + 1; j0 < L; j0 += 64) {
            const int j = j0 + lane;
            bool in = false;
            if (j < L && ri[j] != ri_i) {                       // (equal residue numbers: neither is below the other, no pair)
                const int fj = flags[j] & EXIST_BITS;
                int a, b;
                bonded_slots(ri_i, ri[j], a, b);
                n_pairs += n_i * __popc(fj) - (a >= 0 ? ((fi >> a) & 1) & ((fj >> b) & 1) : 0);
                const double dx = cx - xs[5 * j + 1], dy = cy - ys[5 * j + 1], dz = cz - zs[5 * j + 1];
                in = !(sqrt((dx * dx + dy * dy) + dz * dz) >= (rho_i + rho[j]) + reach);      // (a NaN survives and clashes with nothing)
            }
            const unsigned long long m = __ballot(in);
            if (m == 0) continue;                               // wave-uniform
            if (in) my_ring[(head + waiting + __popcll(m & ((1ull << lane) - 1ull))) & (RING - 1)] = (i << 16) | j;
            waiting += __popcll(m);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the ring is read by other lanes of this wave
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (waiting >= 64) expand(64);
        }
    }
    if (waiting > 0) expand(waiting);
    n_pairs = wave_sum(n_pairs);
    n_clashes = wave_sum(n_clashes);
    if (lane == 0) {
        atomicAdd(&counters[C_PAIRS], n_pairs);
        atomicAdd(&counters[C_CLASHES], n_clashes);
    }
    __syncthreads();

    // ---- the rows in a fixed tree, the masks and the fractions
    double clash_sum = 0.0;
    for (int r = tid; r < L; r += THREADS) clash_sum += slot[r];
    clash_sum = block_sum<WAVES>(clash_sum, red, lane, wave);
    int n_bond = 0, n_clash = 0, n_union = 0;
    for (int r = tid; r < L; r += THREADS) {
        const int f = flags[r];
        const int bond = ((f & VIOL_BIT) || (r > 0 && (flags[r - 1] & VIOL_BIT))) ? 1 : 0;     // a violated connection marks both residues
        const int hits = (f >> CLASH_SHIFT) & EXIST_BITS;
        p.bond_mask[(size_t)s * L + r] = (unsigned char)bond;
        for (int a = 0; a < N_ATOMS; ++a) p.clash_mask[((size_t)s * L + r) * N_ATOMS + a] = (unsigned char)((hits >> a) & 1);
        n_bond += bond;
        n_clash += hits != 0;
        n_union += bond | (hits != 0);
    }
    n_bond = wave_sum(n_bond); n_clash = wave_sum(n_clash); n_union = wave_sum(n_union);
    if (lane == 0) {
        atomicAdd(&counters[C_BOND_RES], n_bond);
        atomicAdd(&counters[C_CLASH_RES], n_clash);
        atomicAdd(&counters[C_UNION_RES], n_union);
    }
    __syncthreads();
    if (tid == 0) {
        const double residues = 1e-4 + (double)L;               // (masked_mean's eps, a sequence mask of ones)
        p.losses[4 * (size_t)s + 3] = clash_sum / (1e-6 + (double)counters[C_PAIRS]);
        p.n_clash_pairs[s] = counters[C_CLASHES];
        p.fractions[4 * (size_t)s + 0] = (double)counters[C_BOND_RES] / residues;
        p.fractions[4 * (size_t)s + 1] = (double)counters[C_CLASH_RES] / residues;
        p.fractions[4 * (size_t)s + 2] = (double)counters[C_UNION_RES] / residues;
        p.fractions[4 * (size_t)s + 3] = (double)counters[C_CA_VIOL] / (1e-4 + (double)counters[C_CA_MASK]);
    }
}

template <int THREADS>
int launch(int n, int L, const Params& p, hipStream_t st) {
    return ensemble::launch_dynamic_lds(violations_kernel<THREADS>, dim3((unsigned)n), dim3(THREADS), lds_bytes(L, THREADS), st, L, p);
}

}  // namespace

extern "C" int s2s_backbone_violations(const float* atoms, int n, int n_res, const unsigned char* atom_exists, const int* aatype,
                                       const int* residue_index, double tolerance_factor, double clash_tolerance, double* losses,
                                       double* fractions, double* per_residue_loss, unsigned char* bond_mask,
                                       unsigned char* clash_atom_mask, int* n_clash_pairs, void* stream) {
    if (!atoms || !atom_exists || !aatype || !residue_index || !losses || !fractions || !per_residue_loss || !bond_mask || !clash_atom_mask ||
        !n_clash_pairs || n < 1 || n_res < 1 || n_res > MAX_RES || !isfinite(tolerance_factor) || !isfinite(clash_tolerance))
        return (int)hipErrorInvalidValue;
    const Params p = {atoms, atom_exists, aatype, residue_index, tolerance_factor, clash_tolerance, losses, fractions, per_residue_loss,
                      bond_mask, clash_atom_mask, n_clash_pairs};
    if (n_res <= SHORT_RES) return launch<THREADS_SHORT>(n, n_res, p, (hipStream_t)stream);
    return launch<THREADS_LONG>(n, n_res, p, (hipStream_t)stream);
}
