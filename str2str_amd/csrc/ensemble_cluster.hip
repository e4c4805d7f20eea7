// Threshold clustering of an ensemble on the device: packed neighbour bits from row chunks of a pairwise matrix, then the GROMOS
// algorithm (Daura et al. 1999; `gmx cluster -method gromos`) as two small stream-ordered kernels per extracted cluster.
//
// Bit layout: adj[i][w] bit b (little-endian) is the relation i ~ (64 w + b); W = ceil(n / 64) words per row; one __ballot of a wave over
// 64 consecutive columns is one word.  The diagonal is always set, bits of columns >= n are always clear, NaN never compares true.
//
// Loop state (int[3], device): [0] live structures, [1] clusters extracted so far, [2] size of the cluster the last pick extracted
// (0: that round had nothing to do, the update after it returns at once).  A round with nothing live changes nothing, so
// the host may enqueue any number of rounds between two readbacks of the state.
#include <hip/hip_runtime.h>

#include "ensemble_common.h"
#include "str2str_hip.h"

namespace {

using ensemble::wave_sum;
using u64 = unsigned long long;
constexpr int PICK_THREADS = 1024;                  // one workgroup; one thread per word of a row in the prefix sum
constexpr int MAX_N = S2S_CLUSTER_MAX_N;            // 64 * PICK_THREADS
static_assert(MAX_N == 64 * PICK_THREADS, "the pick kernel scans one live word per thread");

// ---- adjacency ------------------------------------------------------------------------------------------------------------------
// One wave per (row, word): lane l holds column 64 w + l.
__global__ void __launch_bounds__(256) adjacency_kernel(const double* __restrict__ values, int n_rows, int row0, int n, int W, double cutoff,
                                                        int at_least, u64* __restrict__ adj) {
    const long long task = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);       // wave-uniform
    if (task >= (long long)n_rows * W) return;
    const int r = (int)(task / W), w = (int)(task % W);
    const int col = w * 64 + (int)(threadIdx.x & 63);
    bool near = false;
    if (col < n) {
        const double v = values[(long long)r * n + col];
        near = (at_least ? v >= cutoff : v <= cutoff) || col == row0 + r;
    }
    const u64 word = __ballot(near);
    if ((threadIdx.x & 63) == 0) adj[(long long)(row0 + r) * W + w] = word;
}

// One wave per row of the chunk: deg[row] = number of set bits of the row.
__global__ void __launch_bounds__(256) degree_kernel(const u64* __restrict__ adj, int n_rows, int row0, int W, int* __restrict__ deg) {
    const int r = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (r >= n_rows) return;
    const u64* row = adj + (long long)(row0 + r) * W;
    int c = 0;
    for (int w = threadIdx.x & 63; w < W; w += 64) c += __popcll(row[w]);
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) deg[row0 + r] = c;
}

// ---- the greedy loop ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) init_kernel(int n, int W, u64* __restrict__ live, int* __restrict__ state) {
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w < W) live[w] = (w + 1) * 64 <= n ? ~0ull : (~0ull >> (64 * (w + 1) - n));
    if (w == 0) { state[0] = n; state[1] = 0; state[2] = 0; }
}

// Exclusive prefix sum of one int per thread over the workgroup (PICK_THREADS = 16 waves); *total = the sum.
__device__ inline int block_exclusive_scan(int v, int* wave_tot, int* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wave_tot[wv] = inc;
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < PICK_THREADS / 64; ++k) {
        const int t = wave_tot[k];
        before += k < wv ? t : 0;
        all += t;
    }
    __syncthreads();
    *total = all;
    return before + inc - v;
}

// A single workgroup: the centre is the live row of the largest live-neighbour count, the lowest index among equals (one 64-bit
// maximum of (deg << 32) | (0xFFFFFFFF - index)); its live neighbours become cluster state[1] and leave `live`.  Once that count is 1
// every live structure is alone: they are all labelled here, in index order, by a prefix sum over the live bits.
__global__ void __launch_bounds__(PICK_THREADS) pick_kernel(const u64* __restrict__ adj, const int* __restrict__ deg, int n, int W,
                                                            int* __restrict__ labels, int* __restrict__ centres, int* __restrict__ sizes,
                                                            int* __restrict__ state, u64* __restrict__ live, u64* __restrict__ members) {
    __shared__ u64 wave_key[PICK_THREADS / 64];
    __shared__ int wave_tot[PICK_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n_live = state[0], k = state[1];
    if (n_live <= 0) {                               // (uniform over the workgroup)
        if (tid == 0) state[2] = 0;
        return;
    }
    u64 key = 0;                                     // a live row has deg >= 1, so 0 is below every candidate
    for (int i = tid; i < n; i += PICK_THREADS)
        if ((live[i >> 6] >> (i & 63)) & 1) {
            const u64 cand = ((u64)(unsigned)deg[i] << 32) | (u64)(0xFFFFFFFFu - (unsigned)i);
            key = cand > key ? cand : key;
        }
    for (int o = 32; o > 0; o >>= 1) {
        const u64 other = __shfl_xor(key, o);
        key = other > key ? other : key;
    }
    if (lane == 0) wave_key[wv] = key;
    __syncthreads();
    key = 0;
    for (int q = 0; q < PICK_THREADS / 64; ++q) key = wave_key[q] > key ? wave_key[q] : key;
    const int top = (int)(key >> 32);
    const int centre = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFu));

    u64 mine = 0;                                    // this thread's word (W <= PICK_THREADS) of the structures that leave
    if (tid < W) {
        mine = live[tid];
        if (top > 1) {
            mine &= adj[(long long)centre * W + tid];
            if (tid == (centre >> 6)) mine |= 1ull << (centre & 63);             // the centre is live and its own neighbour
        }
    }
    int total;
    const int first = block_exclusive_scan(__popcll(mine), wave_tot, &total);
    if (tid < W) {
        live[tid] &= ~mine;
        members[tid] = mine;
        int rank = first;
        for (u64 bits = mine; bits; bits &= bits - 1) {
            const int i = tid * 64 + __ffsll((long long)bits) - 1;
            if (top > 1) {
                labels[i] = k;
            } else {                                 // singletons: one cluster each, in index order
                labels[i] = k + rank;
                centres[k + rank] = i;
                sizes[k + rank] = 1;
                ++rank;
            }
        }
    }
    if (tid == 0) {
        if (top > 1) { centres[k] = centre; sizes[k] = total; }
        state[0] = n_live - total;
        state[1] = k + (top > 1 ? 1 : total);
        state[2] = top > 1 ? total : 0;              // after the singleton step nothing is live: no count is read again
    }
}

// One wave per row: a live row loses the neighbours that just left.
__global__ void __launch_bounds__(256) update_kernel(const u64* __restrict__ adj, int n, int W, const int* __restrict__ state,
                                                     const u64* __restrict__ live, const u64* __restrict__ members, int* __restrict__ deg) {
    if (state[2] == 0) return;
    const int i = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (i >= n || !((live[i >> 6] >> (i & 63)) & 1)) return;
    const u64* row = adj + (long long)i * W;
    int c = 0;
    for (int w = threadIdx.x & 63; w < W; w += 64) c += __popcll(row[w] & members[w]);
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) deg[i] -= c;
}

}  // namespace

extern "C" int s2s_cluster_adjacency(const double* values, int n_rows, int row0, int n, double cutoff, int at_least,
                                     unsigned long long* adj, int* deg, void* stream) {
    if (!values || !adj || !deg || n < 1 || n > MAX_N || n_rows < 1 || row0 < 0 || row0 > n - n_rows) return (int)hipErrorInvalidValue;
    const int W = (n + 63) / 64;
    hipStream_t st = (hipStream_t)stream;
    const long long tasks = (long long)n_rows * W;
    hipLaunchKernelGGL(adjacency_kernel, dim3((unsigned)((tasks + 3) / 4)), dim3(256), 0, st, values, n_rows, row0, n, W, cutoff, at_least, adj);
    hipLaunchKernelGGL(degree_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, st, adj, n_rows, row0, W, deg);
    return (int)hipGetLastError();
}

extern "C" int s2s_cluster_gromos(const unsigned long long* adj, int* deg, int n, int init, int n_rounds, int* labels, int* centres,
                                  int* sizes, int* state, unsigned long long* live_ws, unsigned long long* members_ws, void* stream) {
    if (!adj || !deg || !labels || !centres || !sizes || !state || !live_ws || !members_ws || n < 1 || n > MAX_N || n_rounds < 0)
        return (int)hipErrorInvalidValue;
    const int W = (n + 63) / 64;
    hipStream_t st = (hipStream_t)stream;
    if (init) hipLaunchKernelGGL(init_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, st, n, W, live_ws, state);
    for (int r = 0; r < n_rounds; ++r) {
        hipLaunchKernelGGL(pick_kernel, dim3(1), dim3(PICK_THREADS), 0, st, adj, deg, n, W, labels, centres, sizes, state, live_ws, members_ws);
        hipLaunchKernelGGL(update_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, adj, n, W, state, live_ws, members_ws, deg);
    }
    return (int)hipGetLastError();
}
