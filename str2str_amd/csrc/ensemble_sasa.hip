// Solvent-accessible surface area of the backbone atoms the sampler writes (N, CA, C, O, CB) by Shrake and Rupley's point test (J. Mol.
// Biol. 79 (1973) 351), on the device.  No counterpart in the reference.  include/str2str_hip.h has the definition; float64 arithmetic on
// the float32 coordinates, contraction off (build.py), so every point test is the float64 numpy value and the counts are exact integers.
//
// One workgroup per structure.  Its 5 L atoms are staged once in LDS, widened, as planes x / y / z / R (8-byte stride between lanes: no
// bank conflict), the unit sphere as planes too.  A wave owns the atoms a = wave, wave + WAVES, ...; lane l owns the points l, l + 64, ...
// of the atom: their positions in registers, one alive bit each (8 at a time: a sphere above 512 points takes two passes).  The wave sweeps the structure's atoms 64 at a time through the prefilter
//   |c_a - c_b|^2 < ((R_a + R_b)(1 + 2^-30) + 2^-30 (1 + M))^2,   M = the largest |coordinate| of the structure's existing atoms,
// and walks the survivors straight off the __ballot mask, lowest index first: the neighbour's index is wave-uniform, so one broadcast LDS
// read of it serves every lane's points, and no list of neighbours is kept that a dense structure could overflow.  The sweep of an atom
// ends as soon as no lane has a live point.  The prefilter is exact in effect: a point lies within R_a (1 + 4 u) + 2 u (M + 2 R_a) of c_a
// and is buried only within R_b (1 + 4 u) of c_b (u = 2^-53, the roundings of the point and of the test), and 2^-30 exceeds those terms by
// a factor of 2^20; an atom it drops cannot bury a point, so no output depends on it.  An atom with a NaN coordinate survives it and
// buries nothing.
// Sums: a count is the popcount of the alive bits over the wave (integer adds).  The areas go to LDS; one thread per residue adds its five
// in slot order, and the residues meet in a fixed tree (thread t adds the residues t, t + THREADS, ... in ascending order, the xor tree of
// a wave, then the waves in turn): the order depends on L and the block shape only.  No floating-point atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ensemble_common.h"
#include "str2str_hip.h"

namespace {

using ensemble::wave_sum;

constexpr int MAX_RES = S2S_SASA_MAX_RES, MAX_POINTS = S2S_SASA_MAX_POINTS;
constexpr int THREADS_SHORT = 512, THREADS_LONG = 1024, SHORT_RES = 256;   // chains up to SHORT_RES: two workgroups share a CU
constexpr int SLOTS_FEW = 2, SLOTS_MANY = 8;                               // points of an atom a lane holds at a time: spheres up to 128 points, finer ones
constexpr int N_ATOMS = 5;                                                 // N, CA, C, O, CB (atom14 slots 0 .. 4)
constexpr double FOUR_PI = 4.0 * 3.141592653589793;                        // (exact: a power of two times the float64 pi)
constexpr double SLACK = 1.0 / (double)(1 << 30);

constexpr size_t lds_bytes(int L, int P) {
    return (size_t)L * N_ATOMS * (5 * 8 + 4) + (size_t)P * 3 * 8 + 16 * 8;
}
static_assert(lds_bytes(MAX_RES, MAX_POINTS) <= 160 * 1024, "a structure of S2S_SASA_MAX_RES residues and the finest sphere fit the LDS of a CU");
static_assert(2 * lds_bytes(SHORT_RES, MAX_POINTS) <= 160 * 1024, "two short workgroups share a CU, whatever the sphere");
static_assert(MAX_POINTS % (64 * SLOTS_MANY) == 0 && SLOTS_MANY <= 32, "whole passes; a lane's alive bits fit one 32-bit mask");

struct Params {
    const float* atoms;
    const unsigned char* exists;
    const double* radii;
    double probe;
    const double* sphere;
    int n_points;
    int* counts;
    double* per_residue;
    double* total;
};

template <int THREADS, int SLOTS>
__global__ void __launch_bounds__(THREADS) sasa_kernel(int L, Params p) {
    constexpr int WAVES = THREADS / 64;
    extern __shared__ double lds[];
    const int A = N_ATOMS * L, P = p.n_points;
    double* xs = lds;                  // [5 L] per plane
    double* ys = xs + A;
    double* zs = ys + A;
    double* Rs = zs + A;               // [5 L] the expanded radius radii + probe
    double* area = Rs + A;             // [5 L] the atoms' areas, 0.0 for an atom that does not exist
    double* ux = area + A;             // [P] per plane
    double* uy = ux + P;
    double* uz = uy + P;
    double* red = uz + P;              // [16]
    int* ex = (int*)(red + 16);        // [5 L] the atom exists
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    double m = 0.0;                    // the largest |coordinate| of the existing atoms (fmax drops a NaN; with an infinity every atom survives)
    {
        const float* src = p.atoms + (size_t)s * A * 3;
        for (int k = tid; k < 3 * A; k += THREADS) {
            const int atom = k / 3, c = k - 3 * atom;
            const double v = (double)src[k];
            (c == 0 ? xs : c == 1 ? ys : zs)[atom] = v;
            if (p.exists[atom]) m = fmax(m, fabs(v));
        }
    }
    for (int a = tid; a < A; a += THREADS) {
        Rs[a] = p.radii[a] + p.probe;
        ex[a] = p.exists[a] != 0;
        area[a] = 0.0;
    }
    for (int k = tid; k < 3 * P; k += THREADS) {
        const int point = k / 3, c = k - 3 * point;
        (c == 0 ? ux : c == 1 ? uy : uz)[point] = p.sphere[k];
    }
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    for (int w = 0; w < WAVES; ++w) m = fmax(m, red[w]);
    const double slack = SLACK * (1.0 + m);
    const int n_slots = (P + 63) >> 6;                          // wave-uniform: the slots of a lane that can hold a point

    for (int a = wave; a < A; a += WAVES) {                     // (wave-uniform throughout: a, its neighbours, the exits)
        int count = 0;
        if (ex[a]) {
            const double cx = xs[a], cy = ys[a], cz = zs[a], ra = Rs[a];
            for (int q0 = 0; q0 < n_slots; q0 += SLOTS) {       // a pass over the atoms per SLOTS x 64 points: one for the usual spheres
                double px[SLOTS], py[SLOTS], pz[SLOTS];
                unsigned alive = 0;
#pragma unroll
                for (int q = 0; q < SLOTS; ++q) {
                    const int k = lane + 64 * (q0 + q);
                    px[q] = py[q] = pz[q] = 0.0;
                    if (k < P) {
                        px[q] = cx + ra * ux[k];
                        py[q] = cy + ra * uy[k];
                        pz[q] = cz + ra * uz[k];
                        alive |= 1u << q;
                    }
                }
                for (int j0 = 0; j0 < A && __ballot(alive != 0); j0 += 64) {
                    const int j = j0 + lane;
                    bool in = false;
                    if (j < A && j != a && ex[j]) {
                        const double dx = cx - xs[j], dy = cy - ys[j], dz = cz - zs[j];
                        const double reach = (ra + Rs[j]) * (1.0 + SLACK) + slack;
                        in = !(((dx * dx + dy * dy) + dz * dz) >= reach * reach);      // (a NaN survives and buries nothing)
                    }
                    unsigned long long near = __ballot(in);
                    while (near) {
                        const int b = j0 + __ffsll((long long)near) - 1;
                        near &= near - 1;
                        const double bx = xs[b], by = ys[b], bz = zs[b], rb = Rs[b];
                        const double rb2 = rb * rb;
#pragma unroll
                        for (int q = 0; q < SLOTS; ++q) {
                            if (q0 + q >= n_slots) break;
                            const double dx = px[q] - bx, dy = py[q] - by, dz = pz[q] - bz;
                            if (((dx * dx + dy * dy) + dz * dz) < rb2) alive &= ~(1u << q);   // (false for NaN)
                        }
                        if (!__ballot(alive != 0)) break;
                    }
                }
                count += wave_sum((int)__popc(alive));
            }
            if (lane == 0) area[a] = (double)count * (FOUR_PI * ra * ra / (double)P);
        }
        if (lane == 0) p.counts[(size_t)s * A + a] = count;
    }
    __syncthreads();

    double sum = 0.0;
    for (int r = tid; r < L; r += THREADS) {
        const double v = (((area[5 * r] + area[5 * r + 1]) + area[5 * r + 2]) + area[5 * r + 3]) + area[5 * r + 4];
        p.per_residue[(size_t)s * L + r] = v;
        sum += v;
    }
    sum = wave_sum(sum);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < WAVES; ++w) t += red[w];
        p.total[s] = t;
    }
}

template <int THREADS, int SLOTS>
int launch(int n, int L, const Params& p, hipStream_t st) {
    return ensemble::launch_dynamic_lds(sasa_kernel<THREADS, SLOTS>, dim3((unsigned)n), dim3(THREADS), lds_bytes(L, p.n_points), st, L, p);
}

}  // namespace

extern "C" int s2s_backbone_sasa(const float* atoms, int n, int n_res, const unsigned char* atom_exists, const double* radii, double probe,
                                 const double* sphere, int n_points, int* counts, double* per_residue, double* total, void* stream) {
    if (!atoms || !atom_exists || !radii || !sphere || !counts || !per_residue || !total || n < 1 || n_res < 1 || n_res > MAX_RES ||
        n_points < 1 || n_points > MAX_POINTS || !isfinite(probe) || probe < 0.0)
        return (int)hipErrorInvalidValue;
    const Params p = {atoms, atom_exists, radii, probe, sphere, n_points, counts, per_residue, total};
    const bool few = n_points <= 64 * SLOTS_FEW;
    if (n_res <= SHORT_RES)
        return few ? launch<THREADS_SHORT, SLOTS_FEW>(n, n_res, p, (hipStream_t)stream) : launch<THREADS_SHORT, SLOTS_MANY>(n, n_res, p, (hipStream_t)stream);
    return few ? launch<THREADS_LONG, SLOTS_FEW>(n, n_res, p, (hipStream_t)stream) : launch<THREADS_LONG, SLOTS_MANY>(n, n_res, p, (hipStream_t)stream);
}
