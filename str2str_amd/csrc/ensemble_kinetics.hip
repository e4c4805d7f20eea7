// Markov-state-model kinetics on the device: k-means in a low-dimensional feature space (nearest centre, Lloyd update, farthest-point
// seeding) and sliding-window transition counts of labelled trajectories.  include/str2str_kinetics.h has the contract -- the squared
// float64 distance summed over the dimensions in ascending order, the lowest index on every tie --; the yardstick is the float64
// restatement in tests/ref_kinetics.py.
//
//   s2k_assign             a workgroup owns 256 frames, a thread one of them with its coordinates in registers (d <= 16, padded with zeros
//                          to 2, 4, 8 or 16: a padded term adds +0.0, which changes no bit) or in LDS (d > 16, coordinate-major: a wave
//                          reads consecutive doubles); the centres pass through LDS in tiles, every lane reading the same centre value.
//   s2k_centre_update      count (per segment of the frames, LDS counters) -> scan (segments, then labels) -> fill (a stable counting sort:
//                          a frame's slot is its label's offset + the label's frames in earlier segments, earlier tiles and earlier in
//                          the tile) -> one wave per (cluster, block of dimensions) sums the members in list order.
//   s2k_farthest_point     per centre: one launch updates the minimal distances and leaves a (value, index) maximum per workgroup, one
//                          single-workgroup launch takes the maximum of those and copies the frame to the centres.
//   s2k_transition_counts  a row of workgroups per trajectory; k <= 64: the counts of a workgroup in LDS first, then one int64 atomic per
//                          non-zero entry; larger k: int64 atomics straight to the matrix.
//
// Everything is float64 with contraction off (build.py): every distance is bit for bit the numpy restatement's.  No float atomics.
#include <hip/hip_runtime.h>

#include "ensemble_common.h"
#include "str2str_kinetics.h"

namespace {

constexpr int BLOCK = 256;

// ---------------------------------------------------------------------------------------------------------------- nearest centre
// After the tiles: the label, the optional distance and the changed-label count of the frame t of this thread (valid: t < T).
__device__ __forceinline__ void assign_store(long long t, bool valid, int label, double best, int* labels, double* dist2, const int* prev,
                                             int* changed) {
    bool differs = false;
    if (valid) {
        if (prev) differs = prev[t] != label;             // (read before the store: labels may be prev itself)
        labels[t] = label;
        if (dist2) dist2[t] = best;
    }
    if (changed) {
        const unsigned long long m = __ballot(differs);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(changed, (int)__popcll(m));
    }
}

// The coordinates in DR registers.  tile[c * DR + i]: the centres of the current tile, padded with zeros like the frame.
template <int DR>
__global__ void __launch_bounds__(BLOCK) assign_reg_kernel(const double* __restrict__ x, int T, int d, const double* __restrict__ centres, int k,
                                                           int tile_centres, int* labels, double* __restrict__ dist2, const int* prev,
                                                           int* __restrict__ changed) {
    extern __shared__ double tile[];
    const long long t = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool valid = t < T;
    double p[DR];
#pragma unroll
    for (int i = 0; i < DR; ++i) p[i] = (valid && i < d) ? x[t * d + i] : 0.0;
    double best = 0.0;
    int label = 0;
    for (int c0 = 0; c0 < k; c0 += tile_centres) {
        const int nc = k - c0 < tile_centres ? k - c0 : tile_centres;
        __syncthreads();                                   // (the previous tile has been read)
        for (int e = threadIdx.x; e < nc * DR; e += BLOCK) {
            const int c = e / DR, i = e % DR;
            tile[e] = i < d ? centres[(size_t)(c0 + c) * d + i] : 0.0;
        }
        __syncthreads();
        for (int c = 0; c < nc; ++c) {
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < DR; ++i) {
                const double diff = p[i] - tile[c * DR + i];
                acc += diff * diff;
            }
            if (c0 + c == 0 || acc < best) { best = acc; label = c0 + c; }
        }
    }
    assign_store(t, valid, label, best, labels, dist2, prev, changed);
}

// d > 16: the coordinates of the 256 frames in LDS, coordinate-major (pts[i * 256 + thread]), then the tile of centres (tile[c * d + i]).
__global__ void __launch_bounds__(BLOCK) assign_lds_kernel(const double* __restrict__ x, int T, int d, const double* __restrict__ centres, int k,
                                                           int tile_centres, int* labels, double* __restrict__ dist2, const int* prev,
                                                           int* __restrict__ changed) {
    extern __shared__ double lds[];
    double* pts = lds;
    double* tile = lds + (size_t)d * BLOCK;
    const long long t0 = (long long)blockIdx.x * BLOCK;
    const long long t = t0 + threadIdx.x;
    const bool valid = t < T;
    const int rows = T - t0 < BLOCK ? (int)(T - t0) : BLOCK;
    for (int e = threadIdx.x; e < BLOCK * d; e += BLOCK) {   // (coalesced over the rows' storage)
        const int r = e / d, i = e % d;
        pts[i * BLOCK + r] = r < rows ? x[t0 * d + e] : 0.0;
    }
    double best = 0.0;
    int label = 0;
    for (int c0 = 0; c0 < k; c0 += tile_centres) {
        const int nc = k - c0 < tile_centres ? k - c0 : tile_centres;
        __syncthreads();                                   // (the frames are in place; the previous tile has been read)
        for (int e = threadIdx.x; e < nc * d; e += BLOCK) tile[e] = centres[(size_t)c0 * d + e];
        __syncthreads();
        for (int c = 0; c < nc; ++c) {
            double acc = 0.0;
            for (int i = 0; i < d; ++i) {
                const double diff = pts[i * BLOCK + threadIdx.x] - tile[c * d + i];
                acc += diff * diff;
            }
            if (c0 + c == 0 || acc < best) { best = acc; label = c0 + c; }
        }
    }
    assign_store(t, valid, label, best, labels, dist2, prev, changed);
}

// ---------------------------------------------------------------------------------------------------------------- Lloyd update
// The segmentation of the frames: `len` frames per segment (a multiple of 256), `segments` of them.
struct Segments {
    long long len;
    int segments;
};

inline Segments segments_of(int T, int k, long long workspace_ints) {
    const long long tiles = ((long long)T + BLOCK - 1) / BLOCK;
    long long want = (workspace_ints - (long long)T - k - 1) / k;
    if (want > S2K_MAX_SEGMENTS) want = S2K_MAX_SEGMENTS;
    if (want > tiles) want = tiles;
    Segments s;
    s.len = (tiles + want - 1) / want * BLOCK;
    s.segments = (int)(((long long)T + s.len - 1) / s.len);
    return s;
}

// hist[s * k + j] = the frames of segment s = blockIdx.x with label j.
__global__ void __launch_bounds__(BLOCK) update_count_kernel(const int* __restrict__ labels, int T, int k, long long seg_len,
                                                             int* __restrict__ hist) {
    extern __shared__ int cnt[];
    for (int j = threadIdx.x; j < k; j += BLOCK) cnt[j] = 0;
    __syncthreads();
    const long long t0 = blockIdx.x * seg_len, t1 = t0 + seg_len < T ? t0 + seg_len : (long long)T;
    for (long long t = t0 + threadIdx.x; t < t1; t += BLOCK) {
        const int l = labels[t];
        if (l >= 0 && l < k) atomicAdd(&cnt[l], 1);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < k; j += BLOCK) hist[(size_t)blockIdx.x * k + j] = cnt[j];
}

// One workgroup: hist becomes, per label, the exclusive prefix over the segments; counts the totals; offsets [k + 1] their exclusive scan.
__global__ void __launch_bounds__(BLOCK) update_scan_kernel(int* __restrict__ hist, int segments, int k, int* __restrict__ counts,
                                                            int* __restrict__ offsets) {
    __shared__ int total[S2K_MAX_CENTRES];
    __shared__ int part[BLOCK];
    for (int j = threadIdx.x; j < k; j += BLOCK) {
        int run = 0;
        for (int s = 0; s < segments; ++s) {
            const int v = hist[(size_t)s * k + j];
            hist[(size_t)s * k + j] = run;
            run += v;
        }
        total[j] = run;
        counts[j] = run;
    }
    __syncthreads();
    const int per = (k + BLOCK - 1) / BLOCK;                  // consecutive labels per thread
    const int j0 = threadIdx.x * per, j1 = j0 + per < k ? j0 + per : k;
    int sum = 0;
    for (int j = j0; j < j1; ++j) sum += total[j];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 1; o < BLOCK; o <<= 1) {                     // inclusive scan of the 256 partial sums
        const int v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - sum;
    for (int j = j0; j < j1; ++j) {
        offsets[j] = run;
        run += total[j];
    }
    if (threadIdx.x == BLOCK - 1) offsets[k] = part[BLOCK - 1];
}

// members[offsets[j] + r] = the r-th frame of label j in ascending frame order.  The segment's frames pass in tiles of 256 in order; next[j]
// is the slot of the label's next frame.
__global__ void __launch_bounds__(BLOCK) update_fill_kernel(const int* __restrict__ labels, int T, int k, long long seg_len,
                                                            const int* __restrict__ offsets, const int* __restrict__ hist,
                                                            int* __restrict__ members) {
    extern __shared__ int next[];
    __shared__ int lab[BLOCK];
    for (int j = threadIdx.x; j < k; j += BLOCK) next[j] = offsets[j] + hist[(size_t)blockIdx.x * k + j];
    const long long t0 = blockIdx.x * seg_len, t1 = t0 + seg_len < T ? t0 + seg_len : (long long)T;
    for (long long base = t0; base < t1; base += BLOCK) {
        const long long t = base + threadIdx.x;
        int l = t < t1 ? labels[t] : -1;
        if (l < 0 || l >= k) l = -1;
        __syncthreads();                                   // (next is set; the previous tile is through)
        lab[threadIdx.x] = l;
        __syncthreads();
        if (l >= 0) {
            int r = 0;
            for (int i = 0; i < (int)threadIdx.x; ++i) r += lab[i] == l;
            const long long at = (long long)next[l] + r;
            if (at >= 0 && at < T) members[at] = (int)t;     // (always true while labels are what the count saw)
        }
        __syncthreads();
        if (l >= 0) atomicAdd(&next[l], 1);
    }
}

// One wave per (cluster = blockIdx.x, block of W dimensions = blockIdx.y): the rule of the header.
__global__ void __launch_bounds__(64) update_sum_kernel(const double* __restrict__ x, int T, int d, int W, const int* __restrict__ counts,
                                                        const int* __restrict__ offsets, const int* __restrict__ members,
                                                        double* __restrict__ centres) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const int n = counts[j];
    if (n <= 0) return;                                    // an empty cluster keeps its centre
    const int start = offsets[j], slots = 64 / W;
    const int s = lane / W, dim = blockIdx.y * W + lane % W;
    double acc = 0.0;
    if (dim < d) {
#pragma unroll 4
        for (int m = s; m < n; m += slots) {
            const int t = members[start + m];
            acc += (t >= 0 && t < T) ? x[(size_t)t * d + dim] : 0.0;
        }
    }
    for (int o = 32; o >= W; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (s == 0 && dim < d) centres[(size_t)j * d + dim] = acc / (double)n;
}

// ---------------------------------------------------------------------------------------------------------------- farthest point
// (value, index) maxima: the larger value, the lower index among equals.
__device__ __forceinline__ void take_max(double& v, int& i, double ov, int oi) {
    if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) { v = ov; i = oi; }
}

// The maximum over the workgroup, valid in thread 0.
__device__ __forceinline__ void block_max(double& v, int& i) {
    __shared__ double wv[BLOCK / 64];
    __shared__ int wi[BLOCK / 64];
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        take_max(v, i, ov, oi);
    }
    if ((threadIdx.x & 63) == 0) { wv[threadIdx.x >> 6] = v; wi[threadIdx.x >> 6] = i; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < BLOCK / 64; ++w) take_max(v, i, wv[w], wi[w]);
}

// m_t = D2(x_t, centre c) (c == 0) or min(m_t, that), over the `per` frames of this workgroup; bval / bidx [gridDim.x]: their maximum.
__global__ void __launch_bounds__(BLOCK) seed_update_kernel(const double* __restrict__ x, int T, int d, long long per,
                                                            const double* __restrict__ centres, int c, double* __restrict__ mind,
                                                            double* __restrict__ bval, int* __restrict__ bidx) {
    __shared__ double ctr[S2K_MAX_DIM];
    if (threadIdx.x < d) ctr[threadIdx.x] = centres[(size_t)c * d + threadIdx.x];
    __syncthreads();
    const long long t0 = blockIdx.x * per, t1 = t0 + per < T ? t0 + per : (long long)T;
    double v = 0.0;
    int at = -1;
    for (long long t = t0 + threadIdx.x; t < t1; t += BLOCK) {
        double acc = 0.0;
        for (int i = 0; i < d; ++i) {
            const double diff = x[t * d + i] - ctr[i];
            acc += diff * diff;
        }
        if (c > 0) {
            const double old = mind[t];
            if (old < acc) acc = old;
        }
        mind[t] = acc;
        take_max(v, at, acc, (int)t);
    }
    block_max(v, at);
    if (threadIdx.x == 0) { bval[blockIdx.x] = v; bidx[blockIdx.x] = at; }
}

// One workgroup: the maximum of the nb block maxima is frame number c of the seeding.
__global__ void __launch_bounds__(BLOCK) seed_pick_kernel(const double* __restrict__ x, int T, int d, const double* __restrict__ bval,
                                                          const int* __restrict__ bidx, int nb, int c, int* __restrict__ indices,
                                                          double* __restrict__ centres) {
    __shared__ int chosen;
    double v = 0.0;
    int at = -1;
    for (int b = threadIdx.x; b < nb; b += BLOCK) take_max(v, at, bval[b], bidx[b]);
    block_max(v, at);
    if (threadIdx.x == 0) chosen = (at >= 0 && at < T) ? at : 0;
    __syncthreads();
    const int t = chosen;
    if (threadIdx.x == 0) indices[c] = t;
    if (threadIdx.x < d) centres[(size_t)c * d + threadIdx.x] = x[(size_t)t * d + threadIdx.x];
}

// Frame `first` is centre 0.
__global__ void __launch_bounds__(64) seed_first_kernel(const double* __restrict__ x, int d, int first, int* __restrict__ indices,
                                                        double* __restrict__ centres) {
    if (threadIdx.x == 0) indices[0] = first;
    if (threadIdx.x < d) centres[threadIdx.x] = x[(size_t)first * d + threadIdx.x];
}

// ---------------------------------------------------------------------------------------------------------------- transition counts
// Workgroup (trajectory = blockIdx.x, part = blockIdx.y of gridDim.y): the trajectory's start is the sum of the lengths in front of it.
// local: the counts of this workgroup in LDS (k * k unsigned words), for k <= 64.
template <bool LOCAL>
__global__ void __launch_bounds__(BLOCK) transition_kernel(const int* __restrict__ labels, int T, const int* __restrict__ lengths, int k, int lag,
                                                           unsigned long long* __restrict__ counts) {
    extern __shared__ unsigned int local[];
    __shared__ long long wsum[BLOCK / 64];
    const int traj = blockIdx.x;
    long long s = 0;
    for (int i = threadIdx.x; i < traj; i += BLOCK) s += lengths[i];
    s = ensemble::wave_sum(s);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    if (LOCAL)
        for (int e = threadIdx.x; e < k * k; e += BLOCK) local[e] = 0u;
    __syncthreads();
    long long start = 0;
    for (int w = 0; w < BLOCK / 64; ++w) start += wsum[w];
    const long long len = lengths[traj];
    const bool inside = start >= 0 && len > lag && start + len <= T;          // (wave-uniform)
    if (inside) {
        const long long n = len - lag;
        for (long long i = (long long)blockIdx.y * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.y * BLOCK) {
            const int a = labels[start + i], b = labels[start + i + lag];
            if (a >= 0 && a < k && b >= 0 && b < k) {
                if (LOCAL) atomicAdd(&local[a * k + b], 1u);
                else atomicAdd(&counts[(size_t)a * k + b], 1ull);
            }
        }
    }
    if (LOCAL) {
        __syncthreads();
        for (int e = threadIdx.x; e < k * k; e += BLOCK)
            if (local[e]) atomicAdd(&counts[e], (unsigned long long)local[e]);
    }
}

inline bool bad_shape(int T, int d, int k) { return T < 1 || d < 1 || d > S2K_MAX_DIM || k < 1 || k > S2K_MAX_CENTRES; }

}  // namespace

extern "C" int s2k_abi_version(void) { return S2K_ABI_VERSION; }

extern "C" int s2k_assign(const double* x, int T, int d, const double* centres, int k, int max_centres, int* labels, double* dist2,
                          const int* prev_labels, int* changed, void* stream) {
    if (!x || !centres || !labels || bad_shape(T, d, k) || max_centres < 0 || (prev_labels == nullptr) != (changed == nullptr))
        return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    if (changed) {
        const hipError_t rc = hipMemsetAsync(changed, 0, sizeof(int), st);
        if (rc != hipSuccess) return (int)rc;
    }
    const int dr = d <= 2 ? 2 : d <= 4 ? 4 : d <= 8 ? 8 : d <= 16 ? 16 : d;        // d' of the header
    int tile = S2K_ASSIGN_TILE_BYTES / (8 * dr);
    if (tile > k) tile = k;
    if (max_centres > 0 && tile > max_centres) tile = max_centres;
    const dim3 grid((unsigned)(((long long)T + BLOCK - 1) / BLOCK)), block(BLOCK);
    const size_t tile_bytes = (size_t)tile * dr * sizeof(double);
    switch (dr) {
        case 2:
            return ensemble::launch_dynamic_lds(assign_reg_kernel<2>, grid, block, tile_bytes, st, x, T, d, centres, k, tile, labels, dist2,
                                                prev_labels, changed);
        case 4:
            return ensemble::launch_dynamic_lds(assign_reg_kernel<4>, grid, block, tile_bytes, st, x, T, d, centres, k, tile, labels, dist2,
                                                prev_labels, changed);
        case 8:
            return ensemble::launch_dynamic_lds(assign_reg_kernel<8>, grid, block, tile_bytes, st, x, T, d, centres, k, tile, labels, dist2,
                                                prev_labels, changed);
        case 16:
            return ensemble::launch_dynamic_lds(assign_reg_kernel<16>, grid, block, tile_bytes, st, x, T, d, centres, k, tile, labels, dist2,
                                                prev_labels, changed);
        default:
            return ensemble::launch_dynamic_lds(assign_lds_kernel, grid, block, (size_t)d * BLOCK * sizeof(double) + tile_bytes, st, x, T, d,
                                                centres, k, tile, labels, dist2, prev_labels, changed);
    }
}

extern "C" int s2k_centre_update(const double* x, int T, int d, const int* labels, int k, int* counts, double* centres, int* workspace,
                                 long long workspace_ints, void* stream) {
    if (!x || !labels || !counts || !centres || !workspace || bad_shape(T, d, k) || workspace_ints < S2K_UPDATE_WORKSPACE_INTS(T, k, 1))
        return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const Segments sg = segments_of(T, k, workspace_ints);
    int* members = workspace;
    int* offsets = workspace + T;
    int* hist = offsets + k + 1;
    const size_t lds = (size_t)k * sizeof(int);
    hipLaunchKernelGGL(update_count_kernel, dim3((unsigned)sg.segments), dim3(BLOCK), lds, st, labels, T, k, sg.len, hist);
    hipLaunchKernelGGL(update_scan_kernel, dim3(1), dim3(BLOCK), 0, st, hist, sg.segments, k, counts, offsets);
    hipLaunchKernelGGL(update_fill_kernel, dim3((unsigned)sg.segments), dim3(BLOCK), lds, st, labels, T, k, sg.len, offsets, hist, members);
    int W = 1;
    while (W < d && W < 8) W <<= 1;
    hipLaunchKernelGGL(update_sum_kernel, dim3((unsigned)k, (unsigned)((d + W - 1) / W)), dim3(64), 0, st, x, T, d, W, counts, offsets, members,
                       centres);
    return (int)hipGetLastError();
}

extern "C" int s2k_farthest_point(const double* x, int T, int d, int k, int first, int* indices, double* centres, double* workspace,
                                  long long workspace_doubles, void* stream) {
    if (!x || !indices || !centres || !workspace || bad_shape(T, d, k) || k > T || first < 0 || first >= T ||
        workspace_doubles < S2K_SEED_WORKSPACE_DOUBLES(T))
        return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const long long tiles = ((long long)T + BLOCK - 1) / BLOCK;
    const long long want = tiles < S2K_SEED_BLOCKS ? tiles : S2K_SEED_BLOCKS;
    const long long per = (tiles + want - 1) / want * BLOCK;
    const int nb = (int)(((long long)T + per - 1) / per);
    double* mind = workspace;
    double* bval = workspace + T;
    int* bidx = reinterpret_cast<int*>(bval + S2K_SEED_BLOCKS);
    hipLaunchKernelGGL(seed_first_kernel, dim3(1), dim3(64), 0, st, x, d, first, indices, centres);
    for (int c = 0; c < k; ++c) {
        hipLaunchKernelGGL(seed_update_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, st, x, T, d, per, centres, c, mind, bval, bidx);
        if (c + 1 < k) hipLaunchKernelGGL(seed_pick_kernel, dim3(1), dim3(BLOCK), 0, st, x, T, d, bval, bidx, nb, c + 1, indices, centres);
    }
    return (int)hipGetLastError();
}

extern "C" int s2k_transition_counts(const int* labels, int T, const int* lengths, int n_traj, int k, int lag, long long* counts,
                                     void* stream) {
    if (!labels || !lengths || !counts || T < 1 || n_traj < 1 || k < 1 || k > S2K_MAX_CENTRES || lag < 1) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t rc = hipMemsetAsync(counts, 0, (size_t)k * k * sizeof(long long), st);
    if (rc != hipSuccess) return (int)rc;
    long long parts = ((long long)T / n_traj + 4 * BLOCK - 1) / (4 * BLOCK);      // about 4 pairs per thread of a mean trajectory
    if (parts < 1) parts = 1;
    if (parts > 1024) parts = 1024;
    const dim3 grid((unsigned)n_traj, (unsigned)parts), block(BLOCK);
    unsigned long long* out = reinterpret_cast<unsigned long long*>(counts);
    if (k <= 64)
        hipLaunchKernelGGL(transition_kernel<true>, grid, block, (size_t)k * k * sizeof(unsigned int), st, labels, T, lengths, k, lag, out);
    else
        hipLaunchKernelGGL(transition_kernel<false>, grid, block, 0, st, labels, T, lengths, k, lag, out);
    return (int)hipGetLastError();
}
