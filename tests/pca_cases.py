"""The inputs of the essential-dynamics tests (tests/test_ensemble_pca*.py) and their float64 yardstick values (tests/ref_pca.py), built
once and shared read-only.

Conditions on the inputs, checked here on the CPU and met by redrawing the seed:
  * fitted cases: every coordinate of every intermediate float64 target of the fit rounds is at least 2^-40 relative away from a float32
    rounding boundary, so that the device and the yardstick (whose means differ by ~1e-15 relative) round the same float32 targets;
  * summary cases: every projected value is at least 1e-9 of the reference's range away from a bin edge of the histograms (the
    reference's own extremes, which define the range, excepted), so that both sides count the same histograms."""
import functools
from typing import NamedTuple

import numpy as np

import ref_pca as ref

PLAIN_SHAPES = ((5, 3), (33, 16), (40, 17), (130, 40), (6, 33))      # (R, L): see tests/test_ensemble_pca.py for why these
FITTED_SHAPES = ((40, 20), (33, 48), (100, 7))
MODE_SD = (3.0, 1.5, 0.7)                                   # x sqrt(L) / 3 Angstrom: the planted amplitudes' standard deviations
NOISE = 0.05


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def chain(rng, L):
    """A random-walk chain of 3.8 A steps [L, 3]."""
    steps = rng.normal(size=(L, 3))
    return np.cumsum(3.8 * steps / np.linalg.norm(steps, axis=1, keepdims=True), axis=0)


def rotation(rng):
    """A random proper rotation."""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else q[:, ::-1]


def rigid_moves(rng, x, reach=30.0):
    """Every structure of x [R, L, 3] under its own random proper rotation and a translation of up to ``reach`` A."""
    out = np.empty_like(x)
    for s in range(len(x)):
        d = rng.normal(size=3)
        out[s] = x[s] @ rotation(rng).T + d / np.linalg.norm(d) * rng.uniform(0.0, reach)
    return out


# ---------------------------------------------------------------------------------------------------------------- without fit
@functools.lru_cache(maxsize=None)
def plain(R, L, weighted=False, offset=False):
    """-> (x [R, L, 3] float32: a chain with 1 A of independent noise per coordinate, centred at the origin or ``offset`` by 100 A in
    every coordinate; p [R] or None: random sample weights that include zeros)."""
    rng = np.random.default_rng(1000 * R + L)
    x = chain(rng, L)[None] + rng.normal(size=(R, L, 3))
    x -= x.mean(axis=(0, 1))
    if offset:
        x += 100.0
    p = None
    if weighted:
        p = rng.uniform(0.2, 2.0, size=R)
        p[rng.choice(R, size=max(1, R // 5), replace=False)] = 0.0
    return _frozen(x.astype(np.float32), p)


@functools.lru_cache(maxsize=None)
def plain_reference(R, L, weighted=False, offset=False):
    """-> (mean [L, 3], covariance, centred coordinates z [R, 3L], normalised weights) of ``plain`` by the yardstick."""
    x, p = plain(R, L, weighted, offset)
    return _frozen(*ref.moments(x, None, p))


# ------------------------------------------------------------------------------------------------------------------- with fit
class Planted(NamedTuple):
    x: np.ndarray          # [R, L, 3] float32
    chain: np.ndarray      # [L, 3]
    modes: np.ndarray      # [3, 3L] orthonormal rows
    seed: int


def draw_planted(rng, M, modes, R, sd=MODE_SD, moved=True):
    L = len(M)
    amp = rng.normal(size=(R, 3)) * (np.asarray(sd) * np.sqrt(L) / 3.0)
    x = (M.reshape(-1)[None] + amp @ modes + NOISE * rng.normal(size=(R, 3 * L))).reshape(R, L, 3)
    return (rigid_moves(rng, x) if moved else x).astype(np.float32)


def away_from_float32_boundaries(m, rel=2.0 ** -40):
    """Is every entry of the float64 array at least ``rel`` (relative) away from the midpoints of its float32 neighbours?"""
    m = np.asarray(m, dtype=np.float64).reshape(-1)
    f = m.astype(np.float32)
    mids = [(f.astype(np.float64) + np.nextafter(f, np.float32(side)).astype(np.float64)) / 2.0 for side in (np.inf, -np.inf)]
    return bool((np.minimum(np.abs(m - mids[0]), np.abs(m - mids[1])) >= rel * np.abs(m)).all())


def fit_is_reproducible(x, **fit_args):
    targets = []
    ref.fit_transforms(x, targets=targets, **fit_args)
    return all(away_from_float32_boundaries(t) for t in targets)


@functools.lru_cache(maxsize=None)
def planted(R, L):
    for seed in range(7000 * R + L, 7000 * R + L + 64):
        rng = np.random.default_rng(seed)
        M = chain(rng, L)
        modes = np.linalg.qr(rng.normal(size=(3 * L, 3)))[0].T
        x = draw_planted(rng, M, modes, R)
        if fit_is_reproducible(x) and fit_is_reproducible(x, target=x[0], n_fit_rounds=1):
            return Planted(*_frozen(x, M, modes), seed)
    raise AssertionError("no seed met the rounding-boundary condition")


@functools.lru_cache(maxsize=None)
def planted_reference(R, L):
    """-> (mean, covariance by the SVD route, the Frobenius distance to Horn's route, z [R, 3L]) of ``planted`` by the yardstick."""
    x = planted(R, L).x
    xform = ref.fit_transforms(x)
    mean, cov, z, _ = ref.moments(x, xform)
    other = ref.ensemble_covariance(x, route="horn")[1]
    return _frozen(mean, cov) + (float(np.linalg.norm(cov - other)),) + _frozen(z)


# ------------------------------------------------------------------------------------------------------------------ summaries
def clear_of_bin_edges(pc, ref_key="target", n_bins=50, rel=1e-9):
    """Is every projected value at least ``rel`` of the reference's range away from every bin edge (the reference's own extremes excepted)?"""
    lo, hi = pc[ref_key].min(0), pc[ref_key].max(0)
    for k, v in pc.items():
        for c in range(v.shape[1]):
            col = v[:, c]
            if k == ref_key:
                col = np.delete(col, [col.argmin(), col.argmax()])
            edges = np.histogram_bin_edges(col, bins=n_bins, range=(lo[c], hi[c]))
            if np.abs(col[:, None] - edges[None, :]).min() < rel * (hi[c] - lo[c]):
                return False
    return True


@functools.lru_cache(maxsize=None)
def summary_ensembles(L=20, R_ref=60, R=50):
    """-> {"target": the reference ensemble; "resample": new draws of the same distribution; "no_mode2": draws with the second planted
    mode switched off}, float32, every one rigidly moved."""
    for seed in range(4242, 4242 + 64):
        rng = np.random.default_rng(seed)
        M = chain(rng, L)
        modes = np.linalg.qr(rng.normal(size=(3 * L, 3)))[0].T
        both = {"target": draw_planted(rng, M, modes, R_ref), "resample": draw_planted(rng, M, modes, R),
                "no_mode2": draw_planted(rng, M, modes, R, sd=(MODE_SD[0], 0.0, MODE_SD[2]))}
        w = summary_weights(both)
        if (fit_is_reproducible(both["target"]) and fit_is_reproducible(both["target"], p=w["target"])
                and clear_of_bin_edges(ref.js_pca(both)[1]) and clear_of_bin_edges(ref.js_pca(both, hist_weights=w)[1])):
            _frozen(*both.values())
            return both
    raise AssertionError("no seed met the conditions")


def summary_weights(both):
    """Per-structure weights by key for the ``weights=`` case: a ramp over every ensemble."""
    return {k: np.linspace(0.25, 2.0, len(v)) for k, v in both.items()}
