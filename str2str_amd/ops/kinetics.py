"""Markov-state-model kinetics on the device (include/str2str_kinetics.h, csrc/ensemble_kinetics.hip): the nearest centre of every feature
row, the Lloyd update in a fixed summation order, deterministic farthest-point seeding and the sliding-window transition counts of
labelled trajectories.  Features are float64 [T, d] device tensors, d <= KINETICS_MAX_DIM: the output of ``feature_project`` or
``ca_project``, typically.  Squared float64 distances summed over the dimensions in ascending order; the lowest index wins every tie."""
from typing import Optional

import torch

from .binding import HipLibraryError, _check, _p, _req, _stream, load_library
from .ensemble import _integer

KINETICS_MAX_DIM = 64          # S2K_MAX_DIM: a frame's coordinates stay in registers or in LDS
KINETICS_MAX_CENTRES = 4096    # S2K_MAX_CENTRES: the per-label counters of a workgroup stay in LDS
KINETICS_MAX_SEGMENTS = 1024   # S2K_MAX_SEGMENTS: the segments s2k_centre_update counts and fills the frames in
KINETICS_SEED_BLOCKS = 1024    # S2K_SEED_BLOCKS: the block maxima in the workspace of s2k_farthest_point


def _rows(fn: str, x, what: str = "features"):
    """``x`` [T, d], the feature rows of ``fn``, checked but for the device -> (T, d)."""
    if not isinstance(x, torch.Tensor):
        raise HipLibraryError(f"{fn}: expected tensors, got {type(x).__name__} for {what}")
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise HipLibraryError(f"{fn}: {what} {tuple(x.shape)}, expected [T, d]")
    T, d = x.shape
    if d > KINETICS_MAX_DIM or T > 2 ** 31 - 1:
        raise HipLibraryError(f"{fn}: at most {KINETICS_MAX_DIM} dimensions and {2 ** 31 - 1} frames, got {d} and {T} (reduce the dimension first)")
    return T, d


def _centres(fn: str, centres, d: int) -> int:
    """``centres`` [k, d] of ``fn``, checked but for the device -> k."""
    if not isinstance(centres, torch.Tensor) or centres.ndim != 2 or centres.shape[0] < 1 or centres.shape[1] != d:
        raise HipLibraryError(f"{fn}: centres {tuple(getattr(centres, 'shape', ()))}, expected [k, {d}]")
    if centres.shape[0] > KINETICS_MAX_CENTRES:
        raise HipLibraryError(f"{fn}: at most {KINETICS_MAX_CENTRES} centres, got {centres.shape[0]}")
    return centres.shape[0]


def _labels(fn: str, labels, T: int, what: str = "labels"):
    if not isinstance(labels, torch.Tensor) or labels.shape != (T,):
        raise HipLibraryError(f"{fn}: {what} {tuple(getattr(labels, 'shape', ()))}, expected [{T}]")


def kmeans_assign(features: torch.Tensor, centres: torch.Tensor, prev_labels: Optional[torch.Tensor] = None, max_centres: Optional[int] = None):
    """The nearest of ``centres`` [k, d] fp64 for every row of ``features`` [T, d] fp64 -> (labels [T] int32: the lowest index of minimal
    squared distance, dist2 [T] fp64: that distance, changed: a one-element int32 tensor counting the rows whose label differs from
    ``prev_labels`` [T] int32, or None without them).  ``max_centres`` bounds the centres of a tile in LDS; it changes no byte."""
    fn = "kmeans_assign"
    T, d = _rows(fn, features)
    k = _centres(fn, centres, d)
    if prev_labels is not None:
        _labels(fn, prev_labels, T, "prev_labels")
    tile = 0 if max_centres is None else _integer(fn, "max_centres", max_centres)
    _req(features, torch.float64, "features"); _req(centres, torch.float64, "centres")
    if prev_labels is not None:
        _req(prev_labels, torch.int32, "prev_labels")
    labels = torch.empty(T, dtype=torch.int32, device=features.device)
    dist2 = torch.empty(T, dtype=torch.float64, device=features.device)
    changed = None if prev_labels is None else torch.empty(1, dtype=torch.int32, device=features.device)
    _check(load_library().s2k_assign(_p(features), T, d, _p(centres), k, tile, _p(labels), _p(dist2), _p(prev_labels), _p(changed), _stream()),
           "s2k_assign")
    return labels, dist2, changed


def kmeans_update(features: torch.Tensor, labels: torch.Tensor, centres: torch.Tensor, max_segments: Optional[int] = None) -> torch.Tensor:
    """The Lloyd update: ``centres`` [k, d] fp64 becomes, IN PLACE, the mean of the rows of ``features`` [T, d] fp64 with each label
    (``labels`` [T] int32; a label outside 0 .. k-1 belongs to no cluster); a cluster without rows keeps its centre byte for byte
    -> counts [k] int32.  The sums run in an order that depends on (count, d) alone: no float atomics, the same bytes on every call.
    ``max_segments`` bounds the segments the rows are counted and filled in (the size of the workspace); it changes no byte."""
    fn = "kmeans_update"
    T, d = _rows(fn, features)
    k = _centres(fn, centres, d)
    _labels(fn, labels, T)
    segments = min(KINETICS_MAX_SEGMENTS, -(-T // 256)) if max_segments is None else _integer(fn, "max_segments", max_segments)
    _req(features, torch.float64, "features"); _req(centres, torch.float64, "centres"); _req(labels, torch.int32, "labels")
    counts = torch.empty(k, dtype=torch.int32, device=features.device)
    ws = torch.empty(T + k + 1 + segments * k, dtype=torch.int32, device=features.device)   # S2K_UPDATE_WORKSPACE_INTS
    _check(load_library().s2k_centre_update(_p(features), T, d, _p(labels), k, _p(counts), _p(centres), _p(ws), ws.numel(), _stream()),
           "s2k_centre_update")
    return counts


def farthest_points(features: torch.Tensor, k: int, first: int = 0):
    """Deterministic seeding: row ``first`` of ``features`` [T, d] fp64, then k - 1 times the row of largest minimal squared distance to the
    rows chosen so far, the lowest index on ties -> (indices [k] int32, centres [k, d] fp64).  k <= T.  One call enqueues the whole loop."""
    fn = "farthest_points"
    T, d = _rows(fn, features)
    k = _integer(fn, "k", k, 1, KINETICS_MAX_CENTRES)
    if k > T:
        raise HipLibraryError(f"{fn}: {k} centres out of {T} frames")
    first = _integer(fn, "first", first, 0, T - 1)
    _req(features, torch.float64, "features")
    indices = torch.empty(k, dtype=torch.int32, device=features.device)
    centres = torch.empty(k, d, dtype=torch.float64, device=features.device)
    ws = torch.empty(T + 2 * KINETICS_SEED_BLOCKS, dtype=torch.float64, device=features.device)   # S2K_SEED_WORKSPACE_DOUBLES
    _check(load_library().s2k_farthest_point(_p(features), T, d, k, first, _p(indices), _p(centres), _p(ws), ws.numel(), _stream()),
           "s2k_farthest_point")
    return indices, centres


def transition_counts(labels: torch.Tensor, n_states: int, lag: int, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """counts [k, k] int64 of the pairs (labels[t], labels[t + lag]) inside one trajectory with both labels in 0 .. k-1 (a negative label
    is "unassigned").  ``labels`` [T] int32: the trajectories laid end to end; ``lengths`` [n_traj] int32 device tensor summing to T
    (None: one trajectory).  A trajectory of at most ``lag`` frames contributes nothing.  Integer atomics: exact."""
    fn = "transition_counts"
    if not isinstance(labels, torch.Tensor) or labels.ndim != 1 or labels.shape[0] < 1 or labels.shape[0] > 2 ** 31 - 1:
        raise HipLibraryError(f"{fn}: labels {tuple(getattr(labels, 'shape', ()))}, expected [T]")
    T = labels.shape[0]
    k = _integer(fn, "n_states", n_states, 1, KINETICS_MAX_CENTRES)
    lag = _integer(fn, "lag", lag)
    if lengths is not None and (not isinstance(lengths, torch.Tensor) or lengths.ndim != 1 or lengths.shape[0] < 1):
        raise HipLibraryError(f"{fn}: lengths {tuple(getattr(lengths, 'shape', ()))}, expected [n_traj]")
    _req(labels, torch.int32, "labels")
    if lengths is None:
        lengths = torch.full((1,), T, dtype=torch.int32, device=labels.device)
    _req(lengths, torch.int32, "lengths")
    counts = torch.empty(k, k, dtype=torch.int64, device=labels.device)
    _check(load_library().s2k_transition_counts(_p(labels), T, _p(lengths), lengths.shape[0], k, lag, _p(counts), _stream()),
           "s2k_transition_counts")
    return counts
