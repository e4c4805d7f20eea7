"""The numpy yardstick of the solvent-accessible surface (include/str2str_hip.h, csrc/ensemble_sasa.hip): Shrake and Rupley's point test in
float64, brute force -- every point of every atom against every other atom, no prefilter and no neighbour list -- with every term formed
in the operation order of the definition, one rounding per operation.  It also returns a case's margin: the smallest |v - R_b^2| / R_b^2
over all its point-atom comparisons, the distance of its nearest comparison from flipping."""
import math

import numpy as np

RADII = (1.55, 1.7, 1.7, 1.52, 1.7)       # Bondi: N, CA, C, O, CB
GLY = 7
CHUNK_TERMS = 1 << 22                     # point-atom comparisons formed at a time (a few arrays of 32 MiB)


def sphere(n_points):
    """The golden spiral of the definition -> float64 [P, 3]."""
    P = int(n_points)
    k = np.arange(P, dtype=np.float64)
    y = (k * (2.0 / P) - 1.0) + 1.0 / P
    r = np.sqrt(1.0 - y * y)
    phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
    return np.stack([np.cos(phi) * r, y, np.sin(phi) * r], axis=1)


def exists_from_aatype(aatype):
    exists = np.ones((len(aatype), 5), dtype=bool)
    exists[np.asarray(aatype) == GLY, 4] = False
    return exists


def default_radii(L):
    return np.tile(np.asarray(RADII, dtype=np.float64), (L, 1))


def sasa(atoms, exists, radii, probe=1.4, n_points=96, only=None):
    """One structure: atoms [L, 5, 3] (float32 values), exists [L, 5], radii [L, 5] -> dict(counts int32 [L, 5], per_residue float64 [L],
    total float64, margin float64).  ``only``: flat atom indices 5 r + a; the other atoms keep the count 0 (a spot check of a long chain:
    the areas are then those of the chosen atoms alone)."""
    L = atoms.shape[0]
    P = int(n_points)
    c = np.asarray(atoms, dtype=np.float64).reshape(5 * L, 3)
    ex = np.asarray(exists).reshape(-1) != 0
    R = np.asarray(radii, dtype=np.float64).reshape(-1) + float(probe)
    u = sphere(P)
    A = 5 * L
    R2 = R * R
    counts = np.zeros(A, dtype=np.int32)
    margin = np.inf
    step = max(1, CHUNK_TERMS // (P * A))
    others = np.arange(A)
    todo = others if only is None else np.asarray(only, dtype=np.int64)
    for t0 in range(0, len(todo), step):
        rows = todo[t0:t0 + step]
        p = c[rows, None, :] + R[rows, None, None] * u[None, :, :]                   # [a, P, 3]: the product rounded, then the sum
        dx = p[:, :, 0, None] - c[None, None, :, 0]
        dy = p[:, :, 1, None] - c[None, None, :, 1]
        dz = p[:, :, 2, None] - c[None, None, :, 2]
        v = (dx * dx + dy * dy) + dz * dz                                            # [a, P, A]
        counted = ex[rows, None, None] & ex[None, None, :] & (others[None, None, :] != rows[:, None, None])
        with np.errstate(invalid="ignore"):
            buried = ((v < R2[None, None, :]) & counted).any(axis=2)                 # [a, P]
            rel = np.abs(v - R2[None, None, :]) / R2[None, None, :]
        counts[rows] = np.where(ex[rows], (~buried).sum(axis=1), 0)
        rel = rel[np.broadcast_to(counted, rel.shape)]
        if rel.size:
            margin = min(margin, float(np.nanmin(rel)) if not np.isnan(rel).all() else np.inf)
    w = 4.0 * math.pi * R * R / P                                                    # left to right
    with np.errstate(invalid="ignore"):
        area = np.where(ex, counts.astype(np.float64) * w, 0.0).reshape(L, 5)
    per_residue = (((area[:, 0] + area[:, 1]) + area[:, 2]) + area[:, 3]) + area[:, 4]
    return dict(counts=counts.reshape(L, 5), per_residue=per_residue, total=np.float64(np.cumsum(per_residue)[-1]), margin=margin)


def ensemble(atoms, exists, radii, probe=1.4, n_points=96):
    """atoms [R, L, 5, 3] -> dict(counts [R, L, 5], per_residue [R, L], total [R], margin: the smallest of the structures')."""
    out = [sasa(x, exists, radii, probe, n_points) for x in atoms]
    return dict(counts=np.stack([o["counts"] for o in out]), per_residue=np.stack([o["per_residue"] for o in out]),
                total=np.array([o["total"] for o in out]), margin=min(o["margin"] for o in out))


def relative(atoms, exists, radii, probe=1.4, n_points=96, in_chain=None):
    """atoms [R, L, 5, 3] -> float64 [R, L]: every residue's area in the chain over the area of its own atoms alone."""
    exists, radii = np.asarray(exists), np.asarray(radii, dtype=np.float64)
    in_chain = ensemble(atoms, exists, radii, probe, n_points)["per_residue"] if in_chain is None else in_chain
    alone = np.stack([[sasa(x[r:r + 1], exists[r:r + 1], radii[r:r + 1], probe, n_points)["per_residue"][0] for r in range(x.shape[0])] for x in atoms])
    with np.errstate(invalid="ignore", divide="ignore"):
        return in_chain / alone
