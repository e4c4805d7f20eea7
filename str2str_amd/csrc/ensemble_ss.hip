// Secondary structure (Kabsch & Sander 1983: hydrogen-bond energy, n-turns, bridges, ladders, bends and the eight state letters) and the
// backbone torsions phi, psi, omega of every structure of an ensemble, on the device.  The violations of ensemble_violations.hip say
// whether a backbone is possible; this says what it is.  include/str2str_hip.h has the definition, with its two departures from the DSSP
// program (the energy threshold alone makes a bond, no beta-bulge merging); float64 arithmetic on the float32 coordinates, contraction off
// (build.py), so every energy, cosine and comparison is the float64 numpy value and the letters are exact.
//
// One workgroup per structure.  N, CA, C, O are staged once in LDS, widened, one float64 plane per atom and coordinate (consecutive lanes
// read consecutive 8-byte words), and the amide hydrogens are built next to them.  Then
//   sweep     a wave owns the donors j = wave, wave + WAVES, ...: N_j, H_j and CA_j are wave-uniform, its lanes hold the acceptors
//             i = 64 w + lane, test them against the CA prefilter and evaluate the energy of the survivors; a __ballot packs the bonds into
//             word w of row j of the relation, L x ceil(L / 64) words of LDS: bit i of row j <=> hb(i -> j).  The row is the donor's
//             because the N-H -> O column (the lowest energy over the acceptors of a donor, the lowest i among equals) is then a running
//             minimum per lane and one shuffle tree per row, with no floating-point atomic and no pass over the pairs of its own.
//   patterns  one thread per residue: turns and bends are a few bit tests; bridge partners are enumerated from the set bits of rows i and
//             i + 1 (every bridge of i has a bond donated to i or to i + 1), so the pass is O(bonds), not O(L^2).
//   states    the six steps of the definition, each a gather against the state after the previous one, a barrier between them.
// A structure's outputs depend on nothing but its own coordinates: any chunking gives the same bytes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ensemble_common.h"
#include "str2str_hip.h"

namespace {

constexpr int MAX_RES = S2S_SS_MAX_RES;
constexpr int THREADS_SHORT = 512, THREADS_LONG = 1024, SHORT_RES = 256;   // chains up to SHORT_RES: three workgroups share a CU
constexpr int PRO = 14;                                                    // (aatype of proline in the reference's residue order)
constexpr int N_PLANES = 15;                                               // N, CA, C, O, H times x, y, z
enum { AT_N, AT_CA, AT_C, AT_O, AT_H };
enum { CONN = 1, HAS_H = 2 };                                              // flags[]
enum { T3 = 1, T4 = 2, T5 = 4, BRIDGE = 8, LADDER = 16, BEND = 32 };       // pat[]; turn_n is T3 << (n - 3)
constexpr double Q = 27.888, E_BOND = -0.5, CA_REACH = 9.0, R_MIN = 0.5, E_MIN = -9.9, COS_BEND = 0.3420201433256687;

constexpr int words(int L) { return (L + 63) / 64; }
constexpr int pad8(int n) { return (n + 7) & ~7; }
constexpr size_t lds_bytes(int L) {
    return (size_t)L * N_PLANES * 8 + (size_t)L * words(L) * 8 + (size_t)pad8(L) * (4 + 4 + 1 + 1) + 8;
}
static_assert(lds_bytes(MAX_RES) <= 160 * 1024, "the planes and the bond relation of S2S_SS_MAX_RES residues fit the LDS of a CU");
static_assert(MAX_RES >= 512, "cfg4's chains are 512 residues long");

struct Params {
    const float* atoms;
    const int* aatype;
    const int* residue_index;
    unsigned char* ss;
    int* n_hbonds;
    double* hb_energy;
    int* hb_partner;
    double* torsions;
};

struct V3 { double x, y, z; };
__device__ inline V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline double dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ inline double len(V3 a) { return sqrt(dot(a, a)); }

// The IUPAC torsion of four points in (-pi, pi]: atan2(|b2| b1 . (b2 x b3), (b1 x b2) . (b2 x b3)).
__device__ inline double dihedral(V3 p0, V3 p1, V3 p2, V3 p3) {
    const V3 b1 = sub(p1, p0), b2 = sub(p2, p1), b3 = sub(p3, p2);
    const V3 n1 = cross(b1, b2), n2 = cross(b2, b3);
    return atan2(len(b2) * dot(b1, n2) + 0.0, dot(n1, n2));
}

template <int THREADS>
__global__ void __launch_bounds__(THREADS) ss_kernel(int L, Params p) {
    constexpr int WAVES = THREADS / 64;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int W = words(L), LP = pad8(L);
    double* planes = lds;                                                  // [15][L]
    unsigned long long* bits = (unsigned long long*)(planes + (size_t)N_PLANES * L);   // [L][W]: bit i of row j <=> hb(i -> j)
    int* flags = (int*)(bits + (size_t)L * W);                             // [LP]
    int* pat = flags + LP;                                                 // [LP]
    unsigned char* st_a = (unsigned char*)(pat + LP);                      // [LP] the state after steps 1-2, then after step 4
    unsigned char* st_b = st_a + LP;                                       // [LP] the state after step 3
    int* counter = (int*)(st_b + LP);
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    auto at = [&](int a, int r) -> V3 { return {planes[(3 * a) * L + r], planes[(3 * a + 1) * L + r], planes[(3 * a + 2) * L + r]}; };

    {
        const float* src = p.atoms + (size_t)s * L * 15;                   // [L][5][3]; CB is not used
        for (int k = tid; k < 15 * L; k += THREADS) {
            const int r = k / 15, ac = k - 15 * r;
            if (ac < 12) planes[ac * L + r] = (double)src[k];
        }
    }
    for (int r = tid; r < L; r += THREADS) {
        const bool conn = r > 0 && (long long)p.residue_index[r] == (long long)p.residue_index[r - 1] + 1;
        flags[r] = conn ? (p.aatype[r] == PRO ? CONN : CONN | HAS_H) : 0;
    }
    for (int k = tid; k < L * W; k += THREADS) bits[k] = 0ull;
    if (tid == 0) *counter = 0;
    __syncthreads();

    // ---- the amide hydrogens and the torsions
    for (int r = tid; r < L; r += THREADS) {
        const int f = flags[r];
        V3 h = {0.0, 0.0, 0.0};
        if (f & HAS_H) {
            const V3 co = sub(at(AT_C, r - 1), at(AT_O, r - 1)), n = at(AT_N, r);
            const double l = len(co);
            h = {n.x + co.x / l, n.y + co.y / l, n.z + co.z / l};
        }
        planes[(3 * AT_H) * L + r] = h.x;
        planes[(3 * AT_H + 1) * L + r] = h.y;
        planes[(3 * AT_H + 2) * L + r] = h.z;
        double phi = 0.0, psi = 0.0, omega = 0.0;
        if (f & CONN) {
            phi = dihedral(at(AT_C, r - 1), at(AT_N, r), at(AT_CA, r), at(AT_C, r));
            omega = dihedral(at(AT_CA, r - 1), at(AT_C, r - 1), at(AT_N, r), at(AT_CA, r));
        }
        if (r + 1 < L && (flags[r + 1] & CONN)) psi = dihedral(at(AT_N, r), at(AT_CA, r), at(AT_C, r), at(AT_N, r + 1));
        double* t = p.torsions + ((size_t)s * L + r) * 3;
        t[0] = phi; t[1] = psi; t[2] = omega;
    }
    __syncthreads();

    // ---- the sweep: donors by wave, acceptors by lane
    int n_bonds = 0;
    for (int j = wave; j < L; j += WAVES) {
        if (!(flags[j] & HAS_H)) {                                         // wave-uniform
            if (lane == 0) {
                p.hb_energy[(size_t)s * L + j] = 0.0;
                p.hb_partner[(size_t)s * L + j] = -1;
            }
            continue;
        }
        const V3 nj = at(AT_N, j), hj = at(AT_H, j), caj = at(AT_CA, j);
        double best_e = INFINITY;
        int best_i = INT32_MAX;
        for (int w = 0; w < W; ++w) {
            const int i = 64 * w + lane;
            bool bond = false;
            if (i < L && i != j && i + 1 != j && len(sub(at(AT_CA, i), caj)) < CA_REACH) {
                const V3 o = at(AT_O, i), c = at(AT_C, i);
                const double r_on = len(sub(o, nj)), r_ch = len(sub(c, hj)), r_oh = len(sub(o, hj)), r_cn = len(sub(c, nj));
                double e = Q * (((1.0 / r_on + 1.0 / r_ch) - 1.0 / r_oh) - 1.0 / r_cn);
                if (r_on < R_MIN || r_ch < R_MIN || r_oh < R_MIN || r_cn < R_MIN) e = E_MIN;
                bond = e < E_BOND;
                if (e < best_e) { best_e = e; best_i = i; }                // ascending i per lane: the lowest i among equals stays
            }
            const unsigned long long m = __ballot(bond);
            if (lane == 0) {
                bits[(size_t)j * W + w] = m;
                n_bonds += __popcll(m);
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double oe = __shfl_xor(best_e, o, 64);
            const int oi = __shfl_xor(best_i, o, 64);
            if (oe < best_e || (oe == best_e && oi < best_i)) { best_e = oe; best_i = oi; }
        }
        if (lane == 0) {
            const bool any = best_i != INT32_MAX;
            p.hb_energy[(size_t)s * L + j] = any ? best_e : 0.0;
            p.hb_partner[(size_t)s * L + j] = any ? best_i : -1;
        }
    }
    if (lane == 0 && n_bonds) atomicAdd(counter, n_bonds);
    __syncthreads();
    if (tid == 0) p.n_hbonds[s] = *counter;

    // ---- turns, bends, bridges and ladders: bit tests on the relation
    auto hb = [&](int a, int d) -> bool { return (bits[(size_t)d * W + (a >> 6)] >> (a & 63)) & 1ull; };    // 0 <= a, d < L
    auto ok3 = [&](int i) -> bool { return i >= 1 && i <= L - 2 && (flags[i] & CONN) && (flags[i + 1] & CONN); };   // i - 1 .. i + 1 unbroken
    auto valid = [&](int i, int j) -> bool { return ok3(i) && ok3(j) && (i - j >= 3 || j - i >= 3); };
    auto par = [&](int i, int j) -> bool {
        return valid(i, j) && ((hb(i - 1, j) && hb(j, i + 1)) || (hb(j - 1, i) && hb(i, j + 1)));
    };
    auto anti = [&](int i, int j) -> bool {
        return valid(i, j) && ((hb(i, j) && hb(j, i)) || (hb(i - 1, j + 1) && hb(j - 1, i + 1)));
    };
    for (int i = tid; i < L; i += THREADS) {
        int f = 0;
        for (int n = 3; n <= 5; ++n) {
            if (i + n >= L) break;
            bool unbroken = true;
            for (int k = i + 1; k <= i + n; ++k) unbroken = unbroken && (flags[k] & CONN);
            if (unbroken && hb(i, i + n)) f |= T3 << (n - 3);
        }
        if (i >= 2 && i <= L - 3 && (flags[i - 1] & CONN) && (flags[i] & CONN) && (flags[i + 1] & CONN) && (flags[i + 2] & CONN)) {
            const V3 ca = at(AT_CA, i), u = sub(ca, at(AT_CA, i - 2)), v = sub(at(AT_CA, i + 2), ca);
            if (dot(u, v) / (len(u) * len(v)) < COS_BEND) f |= BEND;
        }
        if (ok3(i)) {
            // Every bridge partner j of i has hb(j -> i), hb(j - 1 -> i), hb(j -> i + 1) or hb(j - 1 -> i + 1): the set bits a of rows i
            // and i + 1 give the candidates j = a and j = a + 1, each then held to the whole definition.
            for (int d = i; d <= i + 1; ++d)
                for (int w = 0; w < W; ++w) {
                    unsigned long long m = bits[(size_t)d * W + w];
                    while (m) {
                        const int a = 64 * w + __ffsll((long long)m) - 1;
                        m &= m - 1;
                        for (int j = a; j <= a + 1 && j < L; ++j) {
                            const bool pr = par(i, j), an = anti(i, j);
                            if (pr || an) f |= BRIDGE;
                            if ((pr && (par(i + 1, j + 1) || par(i - 1, j - 1))) || (an && (anti(i + 1, j - 1) || anti(i - 1, j + 1)))) f |= LADDER;
                        }
                    }
                }
        }
        pat[i] = f;
    }
    __syncthreads();

    // ---- the states.  i starts an n-helix iff turn_n(i - 1) and turn_n(i); residue r lies in the helices that start at r - n + 1 .. r.
    auto starts = [&](int i, int t) -> bool { return i >= 1 && (pat[i - 1] & t) && (pat[i] & t); };
    for (int r = tid; r < L; r += THREADS) {                               // steps 1 and 2: B, E over it, H over everything
        const int f = pat[r];
        unsigned char c = (f & LADDER) ? 'E' : (f & BRIDGE) ? 'B' : '-';
        for (int i = r - 3; i <= r; ++i)
            if (starts(i, T4)) c = 'H';
        st_a[r] = c;
    }
    __syncthreads();
    auto minor_helix = [&](const unsigned char* before, unsigned char* after, int n, int t, unsigned char letter) {
        for (int r = tid; r < L; r += THREADS) {
            unsigned char c = before[r];
            for (int i = r - n + 1; i <= r; ++i) {
                if (!starts(i, t)) continue;                               // (turn_n(i) holds, so i + n < L)
                bool room = true;
                for (int k = i; k < i + n; ++k) room = room && (before[k] == '-' || before[k] == letter);
                if (room) c = letter;
            }
            after[r] = c;
        }
    };
    minor_helix(st_a, st_b, 3, T3, 'G');                                   // step 3
    __syncthreads();
    minor_helix(st_b, st_a, 5, T5, 'I');                                   // step 4
    __syncthreads();
    for (int r = tid; r < L; r += THREADS) {                               // steps 5 and 6
        unsigned char c = st_a[r];
        if (c == '-') {
            bool turn = false;
            for (int n = 3; n <= 5; ++n)
                for (int i = r - n + 1; i <= r - 1; ++i)
                    if (i >= 0 && (pat[i] & (T3 << (n - 3)))) turn = true;
            if (turn) c = 'T';
            else if (pat[r] & BEND) c = 'S';
        }
        p.ss[(size_t)s * L + r] = c;
    }
}

template <int THREADS>
int launch(int n, int L, const Params& p, hipStream_t st) {
    return ensemble::launch_dynamic_lds(ss_kernel<THREADS>, dim3((unsigned)n), dim3(THREADS), lds_bytes(L), st, L, p);
}

}  // namespace

extern "C" int s2s_secondary_structure(const float* atoms, int n, int n_res, const int* aatype, const int* residue_index, unsigned char* ss,
                                       int* n_hbonds, double* hb_energy, int* hb_partner, double* torsions, void* stream) {
    if (!atoms || !aatype || !residue_index || !ss || !n_hbonds || !hb_energy || !hb_partner || !torsions || n < 1 || n_res < 1 ||
        n_res > MAX_RES)
        return (int)hipErrorInvalidValue;
    const Params p = {atoms, aatype, residue_index, ss, n_hbonds, hb_energy, hb_partner, torsions};
    if (n_res <= SHORT_RES) return launch<THREADS_SHORT>(n, n_res, p, (hipStream_t)stream);
    return launch<THREADS_LONG>(n, n_res, p, (hipStream_t)stream);
}
