/* Markov-state-model kinetics on the device: k-means in a low-dimensional feature space (nearest centre, the Lloyd update, farthest-point
 * seeding) and the transition counts of the labelled trajectories.  A family of its own next to include/str2str_hip.h, in the same
 * libstr2str_hip.so (csrc/ensemble_kinetics.hip), with its own prefix s2k_ and its own version: s2k_abi_version() == S2K_ABI_VERSION.
 *
 * Conventions, for every entry point:
 *   - x [T, d] float64, row-major: a feature row per frame (the output of s2s_feature_project or s2s_ca_project, typically).
 *     1 <= d <= S2K_MAX_DIM, 1 <= k <= S2K_MAX_CENTRES, 1 <= T <= 2^31 - 1.  centres [k, d] float64, row-major.
 *   - every pointer is device memory; the last argument is the hipStream_t; the return value is a hipError_t as int.  A NULL where a
 *     buffer is required, a size outside the limits or a workspace below its minimum returns hipErrorInvalidValue before any launch.
 *   - THE DISTANCE: the squared float64 distance  D2(x_t, c_j) = sum_{i = 0 .. d-1} (x_ti - c_ji)^2,  accumulated over the dimensions in
 *     ascending order, every difference, square and sum rounded on its own (no fused multiply-add).  No square root is taken anywhere.
 *   - THE TIE RULE: the lowest index wins.  The nearest centre of a frame is the lowest j of minimal D2 (a later centre replaces an
 *     earlier one only if it is strictly nearer); the farthest frame is the lowest t of maximal value.
 *   - no floating-point atomics: every floating-point result is bit for bit the same from call to call, for any tile bound and for any
 *     workspace size.  The integer atomics (the changed-label counter, the transition counts) are exact and order-free.
 *   - NaN features are outside the contract.
 */
#ifndef STR2STR_KINETICS_H
#define STR2STR_KINETICS_H

#ifdef __cplusplus
extern "C" {
#endif

#define S2K_ABI_VERSION 1
#define S2K_MAX_DIM 64          /* a frame's coordinates stay in registers (d <= 16) or in LDS (256 frames x 64 x 8 B = 128 KiB) */
#define S2K_MAX_CENTRES 4096    /* the per-label counters of a workgroup of s2k_centre_update stay in LDS: 16 KiB */
#define S2K_ASSIGN_TILE_BYTES 16384   /* the centres pass through LDS in tiles of at most this many bytes */
#define S2K_MAX_SEGMENTS 1024   /* s2k_centre_update divides the frames into at most this many contiguous segments */
#define S2K_SEED_BLOCKS 1024    /* s2k_farthest_point divides the frames among at most this many workgroups */

int s2k_abi_version(void);

/* Nearest centre.  labels [T] int32: the lowest j of minimal D2(x_t, c_j).  dist2 [T] float64 or NULL: that minimal D2.
 * prev_labels [T] int32 and changed (one int32) are given together or are both NULL: changed is zeroed by the entry and receives the
 * number of t with labels[t] != prev_labels[t] (integer atomic).  labels may be prev_labels itself.
 * A workgroup owns 256 frames, a thread one of them; the centres pass through LDS in tiles of
 *     min(k, max_centres if > 0, S2K_ASSIGN_TILE_BYTES / (8 d'))  centres  (d' = d rounded up to 2, 4, 8 or 16 where d <= 16, else d),
 * visited in ascending order.  max_centres (>= 0; 0: no bound of its own) is a test hook: it changes no byte of any output. */
int s2k_assign(const double* x, int T, int d, const double* centres, int k, int max_centres, int* labels, double* dist2,
               const int* prev_labels, int* changed, void* stream);

/* The Lloyd update in a fixed summation order.  counts [k] int32: the frames of every label.  centres [k, d], in place: the mean of the
 * members of every cluster that has any; an empty cluster keeps its centre byte for byte.  A label outside 0 .. k-1 is "unassigned":
 * its frame belongs to no cluster.
 * The frames are counted per label, the counts scanned, and the frame indices filled into one list ordered by (label, frame index).  Then
 * one wave per (cluster, block of W dimensions), W = the power of two >= min(d, 8): lane (s, i), s < 64 / W, adds the coordinate i of the
 * members s, s + 64 / W, s + 2 (64 / W), ... of the list in that order, and the 64 / W partial sums are added by an xor tree over
 * s (offsets 32 .. W); the mean is that sum divided by the count.  The order is a function of (count, d) alone.
 * workspace: caller-owned int32, workspace_ints >= S2K_UPDATE_WORKSPACE_INTS(T, k, 1).  More workspace only lets the count and the fill
 * run on more segments of the frames, S2K_UPDATE_WORKSPACE_INTS(T, k, segments), up to S2K_MAX_SEGMENTS: every output is the same. */
#define S2K_UPDATE_WORKSPACE_INTS(T, k, segments) ((long long)(T) + (long long)(k) + 1 + (long long)(segments) * (long long)(k))
int s2k_centre_update(const double* x, int T, int d, const int* labels, int k, int* counts, double* centres, int* workspace,
                      long long workspace_ints, void* stream);

/* Deterministic seeding, k <= T, 0 <= first < T.  indices [k] int32, centres [k, d]: centre 0 is frame `first`; centre c is the frame of
 * largest  m_t = min_{c' < c} D2(x_t, x_indices[c'])  (the lowest t on ties; a chosen frame has m_t = 0).  The whole greedy loop is
 * enqueued by the one call, two launches per centre: the update of m with the block maxima, and the final maximum over the blocks.
 * workspace: caller-owned float64, S2K_SEED_WORKSPACE_DOUBLES(T) values (m and the block maxima with their indices). */
#define S2K_SEED_WORKSPACE_DOUBLES(T) ((long long)(T) + 2 * S2K_SEED_BLOCKS)
int s2k_farthest_point(const double* x, int T, int d, int k, int first, int* indices, double* centres, double* workspace,
                       long long workspace_doubles, void* stream);

/* Sliding-window transition counts.  labels [T] int32 of n_traj >= 1 trajectories laid end to end, lengths [n_traj] int32 (device memory,
 * every length >= 0, their sum T).  counts [k, k] int64, zeroed by the entry:  counts[a, b] = the number of pairs (t, t + lag), lag >= 1,
 * with both frames in one trajectory, labels[t] = a and labels[t + lag] = b, both in 0 .. k-1 (any other label is "unassigned" and
 * counts nowhere).  A trajectory of at most lag frames contributes nothing; one that would reach past T is ignored.  Integer atomics. */
int s2k_transition_counts(const int* labels, int T, const int* lengths, int n_traj, int k, int lag, long long* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STR2STR_KINETICS_H */
