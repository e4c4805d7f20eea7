"""The float64 numpy restatement of the essential-dynamics metrics (include/str2str_hip.h, csrc/ensemble_pca.hip and the tails of
str2str_amd.metrics): superposition rounds, mean, covariance, cross-correlation, PCA, projections and the ensemble summaries.

The superposition runs by two independent float64 routes, ``route="svd"`` (Kabsch's SVD with the determinant correction) and
``route="horn"`` (the top eigenvector of Horn's symmetric 4 x 4 quaternion matrix by numpy.linalg.eigh); ``two_routes`` returns the
Frobenius distance between the covariances they lead to, which is the measure of what the choice of a float64 superposition algorithm
alone does to a covariance (the device's Jacobi solve is a third such route)."""
import numpy as np

PSEUDO_C = 1e-6


# ------------------------------------------------------------------------------------------------------------------ superposition
def _centred(x, target, w):
    w = np.ones(len(x)) if w is None else np.asarray(w, dtype=np.float64)
    cm, ct = (w[:, None] * x).sum(0) / w.sum(), (w[:, None] * target).sum(0) / w.sum()
    return w, cm, ct, x - cm, target - ct


def _rotation_svd(h):
    """The proper rotation that maximises tr(R H), H = sum_i w_i a_i b_i^T (a mobile, b target, both centred)."""
    u, _, vt = np.linalg.svd(h)
    d = np.sign(np.linalg.det(vt.T @ u.T))
    return vt.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ u.T


def _rotation_horn(h):
    """The same rotation from the top eigenvector (w, x, y, z) of Horn's matrix (Horn 1987)."""
    (sxx, sxy, sxz), (syx, syy, syz), (szx, szy, szz) = h
    n = np.array([[sxx + syy + szz, syz - szy, szx - sxz, sxy - syx],
                  [syz - szy, sxx - syy - szz, sxy + syx, szx + sxz],
                  [szx - sxz, sxy + syx, -sxx + syy - szz, syz + szy],
                  [sxy - syx, szx + sxz, syz + szy, -sxx - syy + szz]])
    q0, q1, q2, q3 = np.linalg.eigh(n)[1][:, -1]
    return np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                     [2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                     [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]])


ROUTES = {"svd": _rotation_svd, "horn": _rotation_horn}


def superpose(X, target, w=None, route="svd"):
    """X [R, L, 3] onto target [L, 3] -> xform [R, 12] float64: row-major proper rotation, then translation (s2s_ca_superpose's layout)."""
    X, target = np.asarray(X, dtype=np.float64), np.asarray(target, dtype=np.float64)
    out = np.empty((len(X), 12))
    for s, x in enumerate(X):
        w_, cm, ct, a, b = _centred(x, target, w)
        rot = ROUTES[route]((w_[:, None] * a).T @ b) if X.shape[1] > 1 else np.eye(3)
        out[s, :9], out[s, 9:] = rot.reshape(-1), ct - rot @ cm
    return out


def aligned(X, xform=None):
    """-> y [R, 3L] float64: R_s x_s + t_s (xform None: the widened coordinates themselves)."""
    X = np.asarray(X, dtype=np.float64)
    if xform is None:
        return X.reshape(len(X), -1).copy()
    rot, t = xform[:, :9].reshape(-1, 3, 3), xform[:, 9:]
    y = ((rot[:, None, :, 0] * X[:, :, None, 0] + rot[:, None, :, 1] * X[:, :, None, 1]) + rot[:, None, :, 2] * X[:, :, None, 2]) + t[:, None, :]
    return y.reshape(len(X), -1)


def weights(R, p=None):
    """Sample weights normalised to sum 1 (None: 1 / R)."""
    if p is None:
        return np.full(R, 1.0 / R)
    p = np.asarray(p, dtype=np.float64)
    return p / p.sum()


def fit_transforms(X, target=None, p=None, residue_weights=None, n_fit_rounds=5, fit=True, route="svd", targets=None):
    """The round loop -> xform [R, 12] (None without ``fit``).  ``targets``: a list that receives the float64 mean of every round but the
    last, before its rounding to float32."""
    if not fit:
        return None
    X = np.asarray(X, dtype=np.float32)
    t = X[0] if target is None else np.asarray(target, dtype=np.float32)
    for k in range(n_fit_rounds):
        xform = superpose(X, t, residue_weights, route)
        if k + 1 < n_fit_rounds:
            m = (weights(len(X), p)[:, None] * aligned(X, xform)).sum(0)
            if targets is not None:
                targets.append(m)
            t = m.astype(np.float32).reshape(-1, 3)
    return xform


# ---------------------------------------------------------------------------------------------------------- mean, covariance, DCCM
def moments(X, xform=None, p=None):
    """-> (mean [L, 3], covariance [3L, 3L], the centred coordinates z [R, 3L], the normalised weights): two-pass, population form."""
    y = aligned(X, xform)
    p = weights(len(y), p)
    m = (p[:, None] * y).sum(0)
    z = y - m
    return m.reshape(-1, 3), (p[:, None] * z).T @ z, z, p


def ensemble_covariance(X, target=None, p=None, residue_weights=None, n_fit_rounds=5, fit=True, route="svd"):
    return moments(X, fit_transforms(X, target, p, residue_weights, n_fit_rounds, fit, route), p)[:2]


def two_routes(X, **kwargs):
    """-> (covariance by the SVD route, by Horn's route, the Frobenius distance between them)."""
    a, b = (ensemble_covariance(X, route=r, **kwargs)[1] for r in ("svd", "horn"))
    return a, b, float(np.linalg.norm(a - b))


def dccm(cov):
    L = len(cov) // 3
    tr = np.einsum("iaja->ij", cov.reshape(L, 3, L, 3))
    d = np.diag(tr)
    den = np.sqrt(d[:, None] * d[None, :])
    c = np.clip(np.where(den > 0, tr / np.where(den > 0, den, 1.0), 0.0), -1.0, 1.0)
    np.fill_diagonal(c, 1.0)
    return c


# ------------------------------------------------------------------------------------------------------------------------- PCA
def top_components(cov, k):
    """-> (variances [k] descending, clamped at 0; components [k, n], the largest-magnitude entry of each positive)."""
    vals, vecs = np.linalg.eigh(cov)
    vals, vecs = vals[::-1][:k], vecs[:, ::-1][:, :k].T
    sign = np.sign(vecs[np.arange(k), np.argmax(np.abs(vecs), axis=1)])
    return np.maximum(vals, 0.0), vecs * sign[:, None]


def project(X, mean, components, xform=None):
    return (aligned(X, xform) - np.asarray(mean).reshape(-1)) @ np.asarray(components).T


def pca(X, n_components=10, target=None, p=None, residue_weights=None, n_fit_rounds=5, fit=True, route="svd"):
    """-> (mean, components, variances, total variance, projections) as str2str_amd.metrics.pca defines them."""
    xform = fit_transforms(X, target, p, residue_weights, n_fit_rounds, fit, route)
    mean, cov, _, _ = moments(X, xform, p)
    variances, components = top_components(cov, n_components)
    return mean, components, variances, float(np.trace(cov)), project(X, mean, components, xform)


def pca_project(X, mean, components, route="svd"):
    X = np.asarray(X, dtype=np.float32)
    return project(X, mean, components, superpose(X, np.asarray(mean).astype(np.float32), None, route))


def _js(p, q):
    p, q = p / p.sum(), q / q.sum()
    m = (p + q) / 2.0
    rel = lambda x, y: np.where(x > 0, x * np.log(np.where(x > 0, x, 1.0) / y), 0.0)  # noqa: E731
    return float(np.sqrt((rel(p, m).sum() + rel(q, m).sum()) / 2.0))


def js_pca(both, ref_key="target", n_bins=50, n_components=2, hist_weights=None):
    """-> ({k: the unrounded mean JS distance}, {k: projections}); ``hist_weights`` {k: [R_k]}: histogram weights, the reference's also
    weight its PCA."""
    hw = hist_weights or {}
    mean, comps = pca(both[ref_key], n_components, p=hw.get(ref_key))[:2]
    pc = {k: pca_project(v, mean, comps) for k, v in both.items()}
    lo, hi = pc[ref_key].min(0), pc[ref_key].max(0)
    hist = {k: [np.histogram(v[:, c], bins=n_bins, weights=hw.get(k), range=(lo[c], hi[c]))[0] + PSEUDO_C for c in range(n_components)]
            for k, v in pc.items()}
    return {k: float(np.mean([_js(a, b) for a, b in zip(h, hist[ref_key])])) for k, h in hist.items()}, pc


def dynamics_frame(both, ref_key="target", route="svd"):
    """{k: covariance about the ensemble's own mean after ONE superposition onto the reference's fitted mean structure (float32)}."""
    ref = np.asarray(both[ref_key], dtype=np.float32)
    target = moments(ref, fit_transforms(ref, route=route))[0].astype(np.float32)
    return {k: moments(v, superpose(np.asarray(v, dtype=np.float32), target, None, route))[1] for k, v in both.items()}


def rmsip(covs, sizes, ref_key="target", n_components=10):
    out = {}
    for k, c in covs.items():
        K = min(n_components, len(c) - 6, sizes[ref_key] - 1, sizes[k] - 1)
        u, v = top_components(covs[ref_key], K)[1], top_components(c, K)[1]
        out[k] = float(np.sqrt(np.square(u @ v.T).sum() / K))
    return out


def dccm_mae(covs, ref_key="target"):
    c = {k: dccm(v) for k, v in covs.items()}
    iu = np.triu_indices(len(c[ref_key]), k=1)
    return {k: float(np.abs(v[iu] - c[ref_key][iu]).mean()) for k, v in c.items()}


def total_variance(covs):
    return {k: float(np.trace(v)) for k, v in covs.items()}
