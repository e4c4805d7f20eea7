"""The cases of tests/test_kinetics.py and tests/test_kinetics_bounds.py and their preconditions.  A helper, not a test module.

Labels, seeding indices and iteration counts are integers decided by comparisons of float64 distances.  The device sums the same terms in
the same order as tests/ref_kinetics.py, but the equality of the integers must not rest on that: a case is usable only if, in every
assignment of every Lloyd iteration, the best and the second-best squared distance differ by at least MIN_GAP relative, and in every
farthest-point step the largest and the second-largest minimal distance do.  ``reference`` asserts both (on the CPU, once per case) and
also that the case converges with no empty cluster.

Inputs: Gaussian blobs of unit width around k // 2 (at least one) centres of spread 6, plus the degenerate (1, 1, 1).  The shapes are the
smallest with a tail: T one past a multiple of the 256-frame workgroup (65: one partial wave past the first; 257; 1031; 4099: more than
one segment of the update and more than one block of the seeding), d on both sides of the register / LDS switch at 16 (2, 3, 4, 10; 33),
k below, at and above a 64-lane wave and beyond one LDS tile of centres at d = 2 (130 < 1024, so max_centres forces the tiling)."""
import functools

import numpy as np

import ref_kinetics as RK

MIN_GAP = 1e-9
CASES = ((1, 1, 1), (65, 2, 2), (257, 3, 7), (1031, 10, 65), (130, 33, 5), (1031, 2, 130), (4099, 4, 40))   # (T, d, k)
COUNT_CASES = ((1, 1, 1), (65, 7, 1), (257, 65, 20), (1031, 130, 3))                                        # (T, k, lag)
BOUNDS_T, BOUNDS_D, BOUNDS_K = (1, 65, 257), (1, 3, 33), (1, 7, 65)


def blobs(T, d, k, seed=0):
    rng = np.random.default_rng([seed, T, d, k])
    centres = 6.0 * rng.standard_normal((max(1, k // 2), d))
    return centres[rng.integers(0, len(centres), size=T)] + rng.standard_normal((T, d))


@functools.lru_cache(maxsize=None)
def reference(T, d, k):
    """-> dict(x, seed_indices, seed_centres, and ref_kinetics.lloyd's result from those centres), its preconditions asserted."""
    x = blobs(T, d, k)
    indices, centres, seed_gap = RK.farthest_points(x, k)
    res = RK.lloyd(x, centres)
    assert seed_gap >= MIN_GAP and res["gap"] >= MIN_GAP, (T, d, k, seed_gap, res["gap"])
    assert res["converged"] and not res["empty"] and len(set(indices.tolist())) == k, (T, d, k, res["n_iter"])
    for v in (x, indices, centres, res["centres"], res["labels"]):
        v.setflags(write=False)
    return dict(res, x=x, seed_indices=indices, seed_centres=centres, seed_gap=seed_gap)


def label_string(T, k, seed=0):
    """T labels out of -1 .. k-1 (about one in sixteen unassigned) with some persistence, so that the counts are not uniform."""
    rng = np.random.default_rng([seed, T, k])
    labels = rng.integers(0, k, size=T)
    stay = rng.random(T) < 0.5
    for t in range(1, T):
        if stay[t]:
            labels[t] = labels[t - 1]
    labels[rng.random(T) < 1.0 / 16] = -1
    return labels.astype(np.int32)


def split_lengths(T, n_traj):
    """n_traj lengths summing to T, unequal where T allows."""
    if n_traj == 1 or T < n_traj:
        return [T] + [0] * (n_traj - 1)
    cuts = [T // 2, T // 2 + T // 5]
    return [cuts[0], cuts[1] - cuts[0], T - cuts[1]]


def three_basins(T=1500, seed=3):
    """A planted three-basin trajectory in two features: a three-state Markov chain (stay with probability 0.97) hopping between
    wells at (0, 0), (8, 0) and (0, 8) of width 0.5.  TICA of it is well-posed: two slow coordinates, both above the cut-off.
    -> (features float32 [T, 2], the planted state of every frame)."""
    rng = np.random.default_rng(seed)
    wells = np.array([[0.0, 0.0], [8.0, 0.0], [0.0, 8.0]])
    state = np.zeros(T, dtype=np.int64)
    for t in range(1, T):
        state[t] = state[t - 1] if rng.random() < 0.97 else rng.integers(0, 3)
    return (wells[state] + 0.5 * rng.standard_normal((T, 2))).astype(np.float32), state
