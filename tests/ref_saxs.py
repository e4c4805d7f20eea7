"""The float64 numpy statement of the solution-scattering definitions of include/str2str_hip.h (csrc/ensemble_saxs.hip): the Debye
intensity and the Kirkwood mean inverse distance of CA-bead structures.  It evaluates the same IEEE expressions in the same order as the
kernel up to the argument a = q r of the sine: three exact differences of the widened float32 coordinates, three squares, two additions
(dx dx + dy dy) + dz dz, ``np.sqrt``, one product.  Then ``np.sin(a) / a`` (1.0 where a == 0.0), a term (f_i f_j) s, and the pair terms
summed in float64 by numpy (pairwise summation, not the kernel's order: the device test's bound covers the difference).  The diagonal term
is f_i^2 + |x_i - x_i|^2, which is f_i^2 for a finite bead and NaN otherwise."""
import numpy as np

MAX_ELEMENTS = 1 << 23             # (pairs x q-values) evaluated at a time


def _inputs(ca, q, types, table):
    x = np.asarray(ca)
    assert x.dtype == np.float32 and x.ndim == 3 and x.shape[2] == 3, (x.dtype, x.shape)
    q = np.asarray(q, dtype=np.float64)
    assert q.ndim == 1 and q.size >= 1
    table = np.ones((1, q.size)) if table is None else np.asarray(table, dtype=np.float64)
    types = np.zeros(x.shape[1], dtype=np.int64) if types is None else np.asarray(types)
    assert table.ndim == 2 and table.shape[1] == q.size and types.shape == (x.shape[1],)
    assert types.min() >= 0 and types.max() < table.shape[0]
    return x.astype(np.float64), q, types, table


def pair_distances(x):
    """x [R, L, 3] float64 -> (r [R, N] in the order of np.triu_indices(L, 1), i [N], j [N])."""
    i, j = np.triu_indices(x.shape[1], k=1)
    d = x[:, i] - x[:, j]
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    with np.errstate(invalid="ignore"):
        return np.sqrt((dx * dx + dy * dy) + dz * dz), i, j


def sinc(a):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(a == 0.0, 1.0, np.sin(a) / a)


def scattering(ca, q, types=None, table=None):
    """ca [R, L, 3] float32 -> (intensity [R, Q], inv_r_mean [R]) float64."""
    x, q, types, table = _inputs(ca, q, types, table)
    R, L = x.shape[:2]
    r, i, j = pair_distances(x)
    f = table[types]                                            # [L, Q]
    dd = x - x
    with np.errstate(invalid="ignore"):
        self_v = (dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]) + dd[..., 2] * dd[..., 2]    # [R, L]: 0.0, or NaN for a non-finite bead
    intensity = np.empty((R, q.size))
    step = max(1, MAX_ELEMENTS // max(1, R * r.shape[1]))
    for k0 in range(0, q.size, step):
        qk = q[k0:k0 + step]
        with np.errstate(invalid="ignore"):
            a = r[:, :, None] * qk[None, None, :]
            terms = (f[i, k0:k0 + step] * f[j, k0:k0 + step])[None] * sinc(a)
            off = terms.sum(axis=1)
            diag = ((f[:, k0:k0 + step] * f[:, k0:k0 + step])[None] + self_v[:, :, None]).sum(axis=1)
            intensity[:, k0:k0 + step] = diag + 2.0 * off
    with np.errstate(invalid="ignore", divide="ignore"):
        inv_r_mean = (2.0 * (1.0 / r).sum(axis=1)) / (float(L) * float(L)) + self_v.sum(axis=1)
    return intensity, inv_r_mean


def hydrodynamic_radius(ca):
    with np.errstate(divide="ignore"):
        return 1.0 / scattering(ca, [0.0])[1]


def radius_of_gyration_sq(ca):
    """The float64 mean squared distance of the beads from their centroid, per structure."""
    x = np.asarray(ca, dtype=np.float64)
    return ((x - x.mean(axis=1, keepdims=True)) ** 2).sum(-1).mean(-1)
