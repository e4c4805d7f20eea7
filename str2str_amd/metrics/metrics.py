"""Ensemble metrics of the evaluation step on the device (reference: src/metrics/metrics.py; driver src/eval.py:47-99).

Same function names, arguments and return values (dicts keyed like the input, rounded to 4 decimals) as the reference for
``validity`` (:108-121), ``bonding_validity`` (:124-137), ``js_pwd`` (:140-166) and ``js_rg`` (:203-224).  The N^2 x R work --
pairwise CA distances, per-channel histograms and Jensen-Shannon distances, clash counts, radii of gyration -- runs in two HIP
kernels (csrc/ensemble_metrics.hip) straight on the coordinates the sampler just produced (or on arrays read back from PDB
files); numpy only finishes the O(R) / O(bins) tails.  ``js_tica`` (:169-200): pairwise distances on the device, then the TICA
projection -- deeptime's estimator when it is installed (the reference's), otherwise the same estimator in numpy (``tica_fit``:
deeptime 0.4.4's conventions -- reversible covariances, absolute 1e-6 cut-off, eigenpairs by descending magnitude, canonical signs,
kinetic-map scaling -- so that the projections themselves, not only the score, are the reference's).  Per-sample ``weights=``
(:139-150,178-179,206-208) are histogram weights on both paths.

Not in the reference (its paper's diversity figures came from external tools): minimum RMSD under optimal rigid superposition --
``pairwise_rmsd``, ``diversity_rmsd``, ``coverage_rmsd``, ``superpose``, ``rmsf`` -- on csrc/ensemble_rmsd.hip.  Proper rotations only
(a mirror image is not superposable), float64 arithmetic on the float32 coordinates, optional per-RESIDUE weights.  Its length-normalised
companion, the TM-score under the identity correspondence -- ``tm_d0``, ``pairwise_tm``, ``diversity_tm``, ``coverage_tm``,
``tm_superpose`` -- runs on csrc/ensemble_tm.hip.  Where one global superposition is the wrong tool (a hinge, a floppy terminus, a
disordered loop) the CA-lDDT needs none: ``pairwise_lddt``, ``lddt`` (per model or per residue), ``diversity_lddt``, ``coverage_lddt``,
``cluster_lddt`` on csrc/ensemble_lddt.hip -- the definition of the reference's own ``lddt`` (src/models/loss.py:384-460), float64
distances, integer counts; the first argument is the reference whose environment is scored, so the matrix is not symmetric.  Which states an ensemble visits: ``cluster_rmsd``, ``cluster_tm``, ``cluster_lddt``,
``cluster_from_matrix`` (GROMOS clustering at a cutoff, csrc/ensemble_cluster.hip) threshold those matrices chunk by chunk into packed
neighbour bits and cluster them on the device; only labels, centres and sizes come back.  All of these compare structures with each
other; ``backbone_violations`` (csrc/ensemble_violations.hip) looks inside each one: the reference's between-residue bond, angle and clash
terms (src/models/loss.py:714-1017, 1237-1314) on the full backbone the sampler writes, with ``backbone_validity`` and ``violation_rate``
as its dict-in / dict-out companions.  What a conformation is: ``secondary_structure`` (csrc/ensemble_ss.hip) assigns Kabsch & Sander's
eight states from the backbone hydrogen bonds and ``backbone_torsions`` gives phi, psi, omega; ``ss_propensity``, ``ss_content``,
``ss_mae`` and ``js_rama`` are the ensemble summaries built on them.  Which residues touch: ``contact_map``, ``contact_order``,
``native_contacts`` and ``fraction_native_contacts`` (csrc/ensemble_contacts.hip: CA contacts by squared float64 distances; the hard Q and
the soft Q of Best, Hummer and Eaton 2013), with ``contact_mae``, ``js_q`` and ``mean_q`` as the ensemble-against-reference summaries.
How buried each residue is: ``solvent_accessibility`` and ``relative_accessibility`` (csrc/ensemble_sasa.hip: Shrake and Rupley's point
test on N, CA, C, O, CB -- no side chains, so absolute areas overstate the exposure of large residues), with ``mean_sasa``, ``sasa_mae``
and ``js_sasa`` as the summaries.  What a solution measurement would see: ``saxs_profile``, ``ensemble_saxs`` and ``hydrodynamic_radius``
(csrc/ensemble_saxs.hip: the Debye intensity and the Kirkwood radius of the CA beads -- no hydration shell, no excluded volume, no
built-in form factors, no side chains), ``saxs_mae``, ``mean_rh`` and ``js_rh`` as the summaries, ``saxs_chi2`` and ``read_saxs_dat`` for
the comparison with a measured curve.  How the ensemble moves: ``ensemble_covariance``, ``cross_correlation``, ``pca`` and ``pca_project``
(csrc/ensemble_pca.hip: mean structure, 3L x 3L covariance and projections of the superposed CA coordinates in float64; the symmetric
eigenproblem stays on the host), with ``js_pca``, ``rmsip``, ``dccm_mae`` and ``total_variance`` as the summaries -- Cartesian PCA of one
global superposition, CA only, no quasi-harmonic entropy.  Which coordinates are slow: ``tica`` and ``tica_project``
(csrc/ensemble_tica.hip: the reversible mean and the time-lagged covariances of any feature trajectory and the projections in float64 on
the device; the two eigenproblems stay on the host) give the components, eigenvalues and implied timescales behind ``js_tica``, whose
``backend="device"`` runs on them -- no weights in the fit, no VAMP score.  Which states, and how fast between them: ``kmeans``,
``assign_states``, ``msm``, ``state_populations`` and ``js_msm`` (csrc/ensemble_kinetics.hip: nearest centre, Lloyd update, farthest-point
seeding and transition counts on the device; the k x k estimators stay on the host) -- no PCCA+, no Bayesian errors, no k-means++ or
mini-batches, no relocation of empty clusters, no weights in the fit, at most 64 dimensions.
"""
from __future__ import annotations

import math
from functools import partial
from typing import Callable, NamedTuple

import numpy as np
import torch

from .. import ops

EPS = 1e-12
PSEUDO_C = 1e-6


def _dev(x) -> torch.Tensor:
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    if t.ndim == 2:
        t = t[None]
    assert t.ndim == 3 and t.shape[-1] == 3, f"CA coords should be 2D or 3D, got {tuple(t.shape)}"
    return t.to("cuda", torch.float32).contiguous()


def _js(p: np.ndarray, q: np.ndarray) -> float:
    """scipy.spatial.distance.jensenshannon on two 1-D vectors (natural log)."""
    p = p / p.sum(); q = q / q.sum()
    m = (p + q) / 2.0
    rel = lambda x, y: np.where(x > 0, x * np.log(np.where(x > 0, x, 1.0) / y), 0.0)  # noqa: E731
    return float(np.sqrt((rel(p, m).sum() + rel(q, m).sum()) / 2.0))


def validity(ca_coords_dict, ca_vdw_radius=1.7, allowable_overlap=0.4, k_exclusion=0):
    bar = 2 * ca_vdw_radius - allowable_overlap
    return {k: np.around(1.0 - float((ops.ca_sample_stats(_dev(v), bar, k_exclusion)[0] > 0).double().mean()), decimals=4) for k, v in ca_coords_dict.items()}


def bonding_validity(ca_coords_dict, ref_key="target", eps=1e-6):
    adj = {k: ops.ca_sample_stats(_dev(v))[1] for k, v in ca_coords_dict.items()}
    thres = adj[ref_key].max() + 1e-6          # float32 arithmetic, as the reference forms it (metrics.py:133)
    return {k: np.around(float((a < thres).sum()) / len(a), decimals=4) for k, a in adj.items()}


def _weights(weights, ca_coords_dict):
    """The reference's default (metrics.py:148-150): ones for every ensemble without an entry.  -> {k: float64 [len(v)]}"""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in (weights or {}).items()}
    for k, v in ca_coords_dict.items():
        w.setdefault(k, np.ones(len(v)))
        if w[k].shape != (len(v),):
            raise ValueError(f"weights[{k!r}] has shape {w[k].shape} for {len(v)} samples")
    return w


def _host(v, dtype=None) -> np.ndarray:
    """A tensor on any device, an array or a list as a host array."""
    return np.asarray(v.cpu() if torch.is_tensor(v) else v, dtype=dtype)


# ---- summaries of per-structure values: a dict-in / dict-out metric below is "values per structure, per ensemble", then one of these ----
def against_reference(summaries, ref_key="target", distance=lambda p, ref: np.abs(p - ref).mean()):
    """{k: an ensemble's histogram or profile} -> {k: ``distance`` from the reference's (default: mean absolute difference; 0.0 if empty)}."""
    return {**{k: np.around(float(distance(v, summaries[ref_key])) if v.size else 0.0, decimals=4) for k, v in summaries.items() if k != ref_key}, ref_key: 0.0}


def js_of_values(values, ref_key="target", n_bins=50, weights=None, value_range=None):
    """{k: float64 [R_k], a number per structure} -> {k: JS distance from the reference's}: histograms of ``n_bins`` bins over
    ``value_range`` (None: the reference's smallest to largest value) with per-structure ``weights`` by key and PSEUDO_C."""
    w = _weights(weights, values)
    lo, hi = (values[ref_key].min(), values[ref_key].max()) if value_range is None else value_range
    return js_of_histograms({k: np.histogram(v, bins=n_bins, weights=w[k], range=(lo, hi))[0] + PSEUDO_C for k, v in values.items()}, ref_key)


def mean_of_values(values, weights=None):
    """{k: float64 [R_k], a number per structure} -> {k: their (weighted) mean, rounded to 4 decimals}."""
    w = _weights(weights, values)
    return {k: np.around(float(np.average(v, weights=w[k])), decimals=4) for k, v in values.items()}


# what js_rama, js_q, ss_mae and saxs_mae are of the histograms, fractions of native contacts, propensities and curves one already has
js_of_histograms = partial(against_reference, distance=_js)
js_q_of = partial(js_of_values, value_range=(0.0, 1.0))
ss_mae_of = partial(against_reference, distance=lambda p, ref: (0.5 * np.abs(p - ref).sum(1)).mean())
saxs_mae_of = partial(against_reference, distance=lambda c, ref: (np.abs(c - ref) / ref).mean())


def js_pwd(ca_coords_dict, ref_key="target", n_bins=50, pwd_offset=3, weights=None):
    ref = _dev(ca_coords_dict[ref_key])
    wd = None
    if weights:   # float64 per-sample weights into the device histograms
        wd = {k: torch.as_tensor(v, device="cuda") for k, v in _weights(weights, ca_coords_dict).items()}
    out = {k: np.around(float(ops.ca_pwd_js(ref, _dev(v), pwd_offset, n_bins, PSEUDO_C, ref_weights=wd[ref_key] if wd else None,
                                            pred_weights=wd[k] if wd else None).mean()), decimals=4)
           for k, v in ca_coords_dict.items() if k != ref_key}
    out[ref_key] = 0.0
    return out


def radius_of_gyration(coords):
    return ops.ca_sample_stats(_dev(coords))[2].cpu().numpy()


def js_rg(ca_coords_dict, ref_key="target", n_bins=50, weights=None):
    w = _weights(weights, ca_coords_dict)
    # the reference's Rg is float64 (float32 squared distances x float64 weights, metrics.py:62-78) and so are its histogram edges
    return js_of_values({k: np.asarray(radius_of_gyration(v), dtype=np.float64) for k, v in ca_coords_dict.items()}, ref_key, n_bins, w)


def pairwise_distance_ca(coords, k=1) -> np.ndarray:
    """reference :38-50: upper-triangular CA distances [B, (L - k)(L - k + 1)/2], float32, computed on the device in numpy's own
    float32 arithmetic (s2s_ca_pairwise_distances): bit for bit the reference's features."""
    return ops.ca_pairwise_distances(_dev(coords), k).cpu().numpy()


def tica_fit(x: np.ndarray, lagtime: int, dim: int = 2, epsilon: float = 1e-6):
    """TICA (time-lagged independent component analysis) of a trajectory x [T, D] as deeptime 0.4.4's ``TICA(dim, lagtime)`` -- the
    estimator the reference calls (metrics.py:175; environment.yml:184) -- computes it: reversible estimate (mean and covariances
    symmetrised over the (x_t, x_{t+lag}) pairs, no Bessel correction), C00 whitened on the eigenvectors whose eigenvalue magnitude
    reaches the ABSOLUTE cut-off ``epsilon`` (raised above the magnitude of the most negative eigenvalue when rounding produced one -- a
    relative cut-off would keep a different subspace for rank-deficient pairwise-distance features, whose largest eigenvalue is
    1e2 .. 1e4 A^2), symmetric eigenproblem of the whitened time-lagged covariance, eigenpairs by DESCENDING MAGNITUDE (a negative
    eigenvalue can rank second), canonical signs (every vector's largest-magnitude entry positive), kinetic-map scaling (vector x
    eigenvalue).  -> (mean [D], projection [D, dim]); transform = (x - mean) @ proj.
    Pinned by an analytic two-state process and against the restatement in oracle/tica.py (tests/test_host_cpu.py)."""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[0] <= lagtime:
        raise ValueError(f"js_tica: {x.shape[0]} frames are not enough for lagtime {lagtime}")
    x0, xt = x[:-lagtime], x[lagtime:]
    mean = 0.5 * (x0.mean(0) + xt.mean(0))
    a, b = x0 - mean, xt - mean
    n = 2.0 * a.shape[0]
    c00 = (a.T @ a + b.T @ b) / n
    c0t = (a.T @ b + b.T @ a) / n
    return mean, _tica_from_covariances(c00, c0t, dim, epsilon)[0]


def _tica_from_covariances(c00: np.ndarray, c0t: np.ndarray, dim: int, epsilon: float):
    """The tail of ``tica_fit`` on the reversible covariances [D, D], wherever they were formed: eigh of C00, the absolute cut-off,
    whitening, the symmetric eigenproblem of the whitened C0t, magnitude order, canonical signs, kinetic map.
    -> (projection [D, <= dim], eigenvalues [<= dim], the rank kept above the cut-off)."""
    import scipy.linalg

    def by_magnitude(vals, vecs):
        order = np.argsort(np.abs(vals))[::-1]
        return vals[order], vecs[:, order]

    def canonical(vecs):
        top = np.argmax(np.abs(vecs), axis=0)
        return vecs * np.sign(vecs[top, np.arange(vecs.shape[1])])[None, :]

    w, v = by_magnitude(*scipy.linalg.eigh(c00))
    cut = max(epsilon, -w.min() + 1e-16) if w.min() < 0 else epsilon
    m = len(w) - int(np.searchsorted(np.abs(w)[::-1], cut))
    if m == 0:
        raise ValueError("js_tica: the reference ensemble has no variance above the cut-off")
    white = canonical(v[:, :m]) / np.sqrt(w[:m])[None, :]     # [D, m]: white.T C00 white = I
    lam, u = by_magnitude(*scipy.linalg.eigh(white.T @ c0t @ white))
    proj = canonical(white @ u) * lam[None, :]
    return proj[:, :dim], lam[:dim], m


class EnsembleTICA(NamedTuple):
    """The slow components of a feature trajectory [T, D], float64: ``mean`` [D] (the reversible mean the covariances are taken about),
    ``components`` [D, dim] (``tica_fit``'s projection: whitened, canonical signs, kinetic-map scale; fewer columns when the rank is
    below ``dim``), ``eigenvalues`` [dim] (the autocorrelations at the lag, by descending magnitude), ``timescales`` [dim]
    (-lagtime / ln |eigenvalue| in frames, inf for |eigenvalue| >= 1), ``lagtime`` and ``rank`` (the eigenvalues of C00 kept above
    the cut-off)."""
    mean: np.ndarray
    components: np.ndarray
    eigenvalues: np.ndarray
    timescales: np.ndarray
    lagtime: int
    rank: int


def _features(x, pwd_offset=1) -> torch.Tensor:
    """[T, L, 3] coordinates -> their CA distances (``pairwise_distance_ca``'s, left on the device); [T, D] -> taken as features.
    -> float32 device tensor [T, D]."""
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    if t.ndim == 3:
        return ops.ca_pairwise_distances(_dev(t), pwd_offset)
    if t.ndim != 2:
        raise ValueError(f"tica: expected coordinates [T, L, 3] or features [T, D], got {tuple(t.shape)}")
    return t.to("cuda", torch.float32).contiguous()


def tica(coords_or_features, lagtime=20, dim=2, epsilon=1e-6, pwd_offset=1, max_pairs=None) -> EnsembleTICA:
    """Which collective coordinates are slow?  TICA of a trajectory in time order, ``tica_fit``'s estimator with its heavy half on the
    device: coordinates [T, L, 3] are featurised with their CA distances (``pwd_offset`` as in ``pairwise_distance_ca``), an input
    [T, D] is taken as features (any: distances, sines and cosines of torsions, ...; rounded to float32).  The reversible mean and the
    two D x D covariances over the T - ``lagtime`` frame pairs run on the device in float64 (csrc/ensemble_tica.hip; ``max_pairs`` bounds
    the pairs its workspace holds at a time and changes no bit); the two symmetric eigenproblems run on the host, as for ``pca``
    (``_tica_from_covariances``: the tail ``tica_fit`` runs).  No weights in the fit, no VAMP score, at most ops.TICA_MAX_FEATURES
    features."""
    if isinstance(lagtime, bool) or int(lagtime) != lagtime or lagtime < 1:
        raise ValueError(f"tica: lagtime must be an integer >= 1, got {lagtime}")
    if isinstance(dim, bool) or int(dim) != dim or dim < 1:
        raise ValueError(f"tica: dim must be an integer >= 1, got {dim}")
    f = _features(coords_or_features, pwd_offset)
    if f.shape[0] <= lagtime:
        raise ValueError(f"js_tica: {f.shape[0]} frames are not enough for lagtime {lagtime}")
    mean = ops.lagged_mean(f, int(lagtime))
    c00, c0t = ops.lagged_covariances(f, mean, int(lagtime), max_pairs)
    proj, lam, rank = _tica_from_covariances(c00.cpu().numpy(), c0t.cpu().numpy(), int(dim), epsilon)
    with np.errstate(divide="ignore"):
        timescales = np.where(np.abs(lam) >= 1.0, np.inf, -float(lagtime) / np.log(np.minimum(np.abs(lam), 1.0)))
    return EnsembleTICA(mean.cpu().numpy(), np.ascontiguousarray(proj), lam, np.abs(timescales), int(lagtime), int(rank))


def tica_project(coords_or_features, model: EnsembleTICA, pwd_offset=1) -> np.ndarray:
    """``coords_or_features`` ([R, L, 3] or [R, D], as in ``tica``) on the components of ``model`` -> float64 [R, dim]:
    proj[s, k] = sum_c (f_sc - mean_c) v_ck in float64, on the device."""
    f = _features(coords_or_features, pwd_offset)
    mean = torch.as_tensor(np.asarray(model.mean, dtype=np.float64), device=f.device).contiguous()
    comps = torch.as_tensor(np.ascontiguousarray(np.asarray(model.components, dtype=np.float64).T), device=f.device)
    return ops.feature_project(f, mean, comps).cpu().numpy()


def js_tica(ca_coords_dict, ref_key="target", n_bins=50, lagtime=20, return_tic=True, weights=None, backend="host"):
    """reference :169-200: TICA (2 components, fitted on the reference ensemble's pairwise distances) -> 50-bin histograms over the
    reference's range per component -> mean Jensen-Shannon distance.  -> results (, projections) like the reference.
    ``backend="host"`` (the default) is the reference's path: the features go to the host and deeptime's estimator, or ``tica_fit``
    without it, fits and projects them there.  ``backend="device"`` fits with ``tica`` and projects every ensemble with
    ``tica_project`` -- mean, covariances and projections on the device, the same histogram tail; it never consults deeptime."""
    if backend not in ("host", "device"):
        raise ValueError(f"js_tica: backend must be 'host' or 'device', got {backend!r}")
    w = _weights(weights, ca_coords_dict)
    if backend == "device":
        model = tica(ca_coords_dict[ref_key], lagtime, dim=2)
        return _js_tica_tail({k: tica_project(v, model) for k, v in ca_coords_dict.items()}, ref_key, n_bins, w, return_tic)
    ca_pwd = {k: pairwise_distance_ca(v) for k, v in ca_coords_dict.items()}
    try:
        from deeptime.decomposition import TICA

        tica_model = TICA(dim=2, lagtime=lagtime).fit(ca_pwd[ref_key]).fetch_model()
        ca_dr2d = {k: tica_model.transform(v) for k, v in ca_pwd.items()}
    except ImportError:
        mean, proj = tica_fit(ca_pwd[ref_key], lagtime, dim=2)
        ca_dr2d = {k: (v.astype(np.float64) - mean) @ proj for k, v in ca_pwd.items()}
    return _js_tica_tail(ca_dr2d, ref_key, n_bins, w, return_tic)


def _js_tica_tail(ca_dr2d, ref_key, n_bins, w, return_tic):
    """The histogram tail of ``js_tica`` on the projections of either backend."""
    d_min, d_max = ca_dr2d[ref_key].min(axis=0), ca_dr2d[ref_key].max(axis=0)
    binned = {k: np.stack([np.histogram(v[:, c], bins=n_bins, weights=w[k], range=(d_min[c], d_max[c]))[0] + PSEUDO_C for c in range(v.shape[1])], 1)
              for k, v in ca_dr2d.items()}      # [n_bins, 2]
    results = against_reference(binned, ref_key, lambda v, ref: np.mean([_js(v[:, c], ref[:, c]) for c in range(v.shape[1])]))
    if return_tic:
        return results, ca_dr2d
    return results


# ---- Markov state models: k-means microstates of the slow coordinates, transition counts, populations and timescales ------------------
class EnsembleKMeans(NamedTuple):
    """Microstates of a feature space [T, d]: ``centres`` [k, d] float64, ``labels`` [T] int32 (the nearest centre of every row, the
    lowest index on ties), ``counts`` [k] (the rows of every state), ``inertia`` (the sum of the squared distances to the nearest
    centre), ``n_iter`` (the assignments that were run) and ``converged`` (the last assignment changed no label).  The labels are those
    of the last assignment and the centres the ones they were assigned against."""
    centres: np.ndarray
    labels: np.ndarray
    counts: np.ndarray
    inertia: float
    n_iter: int
    converged: bool


class EnsembleMSM(NamedTuple):
    """A Markov state model at ``lagtime``: ``counts`` [k, k] int64 (all states), ``active`` (the states of the largest strongly
    connected set, ascending), and on the active set ``transition_matrix`` [n, n], ``stationary`` [n], ``eigenvalues`` [n] (real, by
    descending magnitude; the first is 1) and ``timescales`` [n - 1] (-lagtime / ln |eigenvalue| of the second eigenvalue on, in frames;
    inf for |eigenvalue| >= 1).  ``converged``: the reversible estimate met its tolerance (always True for the row-normalised one)."""
    counts: np.ndarray
    active: np.ndarray
    transition_matrix: np.ndarray
    stationary: np.ndarray
    eigenvalues: np.ndarray
    timescales: np.ndarray
    lagtime: int
    converged: bool


def _count(fn, name, v, lo=1) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
        raise ValueError(f"{fn}: {name} must be an integer >= {lo}, got {v!r}")
    return int(v)


def _feature_rows(fn, x) -> torch.Tensor:
    """Feature rows [T, d] (array or tensor, any device) -> float64 device tensor."""
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{fn}: expected features [T, d], got {tuple(t.shape)}")
    if t.shape[1] > ops.KINETICS_MAX_DIM:
        raise ValueError(f"{fn}: at most {ops.KINETICS_MAX_DIM} dimensions, got {t.shape[1]}: reduce first (tica_project, pca_project)")
    return t.to("cuda", torch.float64).contiguous()


def kmeans(features, n_states, init="farthest", first=0, max_iter=100, max_centres=None) -> EnsembleKMeans:
    """Which microstates does an ensemble visit?  Lloyd's k-means of feature rows [T, d <= 64] (``tica_project`` or ``pca_project`` output,
    typically) on the device (csrc/ensemble_kinetics.hip).  ``init``: "farthest" (row ``first``, then repeatedly the row farthest from the
    chosen ones: deterministic, no random numbers) or an array [n_states, d] of centres.  The loop is assign, then update, until an
    assignment changes no label (an integer criterion: the device's counter of changed labels, no float tolerance) or ``max_iter``
    assignments have run.  Squared float64 distances, the lowest index on ties; the update sums in a fixed order, so a run is
    reproducible bit for bit; a state that loses all its rows keeps its centre (no relocation).  ``max_centres`` bounds the centres
    per LDS tile and changes no bit.  No k-means++, no mini-batches, no weights."""
    fn = "kmeans"
    k, max_iter = _count(fn, "n_states", n_states), _count(fn, "max_iter", max_iter)
    if k > ops.KINETICS_MAX_CENTRES:
        raise ValueError(f"{fn}: at most {ops.KINETICS_MAX_CENTRES} states, got {k}")
    if isinstance(init, str) and init != "farthest":
        raise ValueError(f"{fn}: init must be 'farthest' or an array of centres, got {init!r}")
    x = _feature_rows(fn, features)
    T, d = x.shape
    if isinstance(init, str):
        if k > T:
            raise ValueError(f"{fn}: {k} states out of {T} frames")
        centres = ops.farthest_points(x, k, _count(fn, "first", first, 0))[1]
    else:
        centres = (init if torch.is_tensor(init) else torch.as_tensor(np.asarray(init))).to("cuda", torch.float64).contiguous().clone()
        if centres.shape != (k, d):
            raise ValueError(f"{fn}: init {tuple(centres.shape)}, expected [{k}, {d}]")
    prev, converged = None, False
    for n_iter in range(1, max_iter + 1):
        labels, dist2, changed = ops.kmeans_assign(x, centres, prev, max_centres)
        if changed is not None and int(changed.item()) == 0:
            converged = True
            break
        if n_iter < max_iter:
            ops.kmeans_update(x, labels, centres)
            prev = labels
    lab = labels.cpu().numpy()
    return EnsembleKMeans(centres.cpu().numpy(), lab, np.bincount(lab, minlength=k), float(dist2.cpu().numpy().sum()), n_iter, converged)


def assign_states(features, model_or_centres) -> np.ndarray:
    """The state of every feature row [R, d] of any ensemble: the nearest centre of an ``EnsembleKMeans`` (or of an array [k, d]), the
    rule of ``kmeans`` -> int32 [R]."""
    x = _feature_rows("assign_states", features)
    c = model_or_centres.centres if isinstance(model_or_centres, EnsembleKMeans) else model_or_centres
    c = (c if torch.is_tensor(c) else torch.as_tensor(np.asarray(c))).to("cuda", torch.float64).contiguous()
    if c.ndim != 2 or c.shape[1] != x.shape[1]:
        raise ValueError(f"assign_states: centres {tuple(c.shape)} for features {tuple(x.shape)}")
    return ops.kmeans_assign(x, c)[0].cpu().numpy()


def state_populations(labels, n_states, weights=None) -> np.ndarray:
    """The (weighted) fraction of an ensemble in every state -> float64 [n_states]; a negative label is unassigned."""
    lab = np.asarray(labels)
    w = np.ones(len(lab)) if weights is None else np.asarray(weights, dtype=np.float64)
    if w.shape != lab.shape:
        raise ValueError(f"state_populations: weights {w.shape} for {lab.shape} labels")
    keep = (lab >= 0) & (lab < n_states)
    hist = np.bincount(lab[keep], weights=w[keep], minlength=int(n_states))
    return hist / hist.sum()


def _active_set(counts: np.ndarray) -> np.ndarray:
    """The largest strongly connected set of the graph counts > 0; on a size tie the set that holds the lowest state."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components

    _, comp = connected_components(csr_matrix(counts > 0), directed=True, connection="strong")
    sizes = np.bincount(comp)
    lowest = np.array([np.flatnonzero(comp == c)[0] for c in range(len(sizes))])
    best = min(range(len(sizes)), key=lambda c: (-sizes[c], lowest[c]))
    return np.flatnonzero(comp == best)


def _reversible_mle(c: np.ndarray, tol: float, max_iter: int):
    """The reversible maximum-likelihood estimate of a count matrix on a strongly connected set: the fixed point of
    x_ij <- (c_ij + c_ji) / (c_i / x_i + c_j / x_j) (c_i, x_i: row sums) from x = C + C^T, until the relative residual
    |x_ij (c_i / x_i + c_j / x_j) - (c_ij + c_ji)| / (c_ij + c_ji) is at most ``tol`` wherever c_ij + c_ji > 0.
    -> (transition matrix x_ij / x_i, stationary x_i / sum x, converged)."""
    c = np.asarray(c, dtype=np.float64)
    s, ci = c + c.T, c.sum(1)
    x, pair = s.copy(), s > 0
    converged = False
    for _ in range(int(max_iter)):
        q = ci / x.sum(1)
        denom = q[:, None] + q[None, :]
        if (np.abs(x * denom - s)[pair] <= tol * s[pair]).all():
            converged = True
            break
        x = np.where(pair, s / np.where(pair, denom, 1.0), 0.0)
    xi = x.sum(1)
    return x / xi[:, None], xi / xi.sum(), converged


def _msm_tail(counts: np.ndarray, lagtime: int, reversible: bool, tol: float, max_iter: int) -> EnsembleMSM:
    """The k x k host tail of ``msm`` on the count matrix."""
    active = _active_set(counts)
    c = counts[np.ix_(active, active)].astype(np.float64)
    if len(active) == 1 and c[0, 0] == 0:      # no transition was counted at all
        t, pi, converged = np.ones((1, 1)), np.ones(1), True
    elif reversible:
        t, pi, converged = _reversible_mle(c, tol, max_iter)
    else:
        t, converged = c / c.sum(1)[:, None], True
        w, v = np.linalg.eig(t.T)
        pi = np.abs(np.real(v[:, np.argmin(np.abs(w - 1.0))]))
        pi = pi / pi.sum()
    root = np.sqrt(pi)
    sym = root[:, None] * t / root[None, :]
    lam = np.linalg.eigvalsh(0.5 * (sym + sym.T))
    lam = lam[np.argsort(-np.abs(lam), kind="stable")]
    mag = np.abs(lam[1:])
    timescales = np.full(mag.shape, np.inf)
    with np.errstate(divide="ignore"):
        timescales[mag < 1.0] = np.abs(-float(lagtime) / np.log(mag[mag < 1.0]))     # (an eigenvalue 0: timescale 0)
    return EnsembleMSM(counts, active, t, pi, lam, timescales, int(lagtime), bool(converged))


def msm(labels, n_states, lagtime, lengths=None, reversible=True, tol=1e-12, max_iter=100000) -> EnsembleMSM:
    """A Markov state model of labelled trajectories: ``labels`` [T] (states 0 .. n_states - 1 in time order, a negative label is
    unassigned; several trajectories laid end to end with their ``lengths``).  The sliding-window counts of the pairs (t, t + lagtime)
    run on the device; the n_states x n_states tail runs on the host: the largest strongly connected set (the set with the lowest state
    on a size tie), then the row-normalised counts or (``reversible``) the reversible maximum-likelihood estimate (``_reversible_mle``:
    its fixed-point iteration to the relative residual ``tol``, at most ``max_iter`` rounds), the stationary distribution, the real
    spectrum of the symmetrised matrix and the implied timescales.  No coarse-graining (PCCA+), no Bayesian errors."""
    fn = "msm"
    k, lag = _count(fn, "n_states", n_states), _count(fn, "lagtime", lagtime)
    lab = torch.as_tensor(np.asarray(labels.cpu() if torch.is_tensor(labels) else labels))
    if lab.ndim != 1 or lab.shape[0] < 1:
        raise ValueError(f"{fn}: expected labels [T], got {tuple(lab.shape)}")
    lens = None
    if lengths is not None:
        lens = np.asarray(lengths, dtype=np.int64)
        if lens.ndim != 1 or len(lens) < 1 or (lens < 0).any() or lens.sum() != lab.shape[0]:
            raise ValueError(f"{fn}: lengths {lens.tolist()} do not sum to the {lab.shape[0]} labels")
        lens = torch.as_tensor(lens).to("cuda", torch.int32)
    counts = ops.transition_counts(lab.to("cuda", torch.int32).contiguous(), k, lag, lens).cpu().numpy()
    return _msm_tail(counts, lag, bool(reversible), float(tol), int(max_iter))


def js_msm(ca_coords_dict, ref_key="target", lagtime=20, n_states=100, dim=4, weights=None, return_model=False):
    """Does a sampled ensemble populate the metastable states of the reference?  ``tica(reference, lagtime, dim)`` on the time-ordered
    reference, ``kmeans`` with ``n_states`` microstates on its projection; every ensemble, the reference included, then goes through
    ``tica_project`` and ``assign_states``, and its state histogram (per-sample ``weights`` by key, PSEUDO_C added) is compared with the
    reference's by the Jensen-Shannon distance -> {key: distance rounded to 4 decimals, the reference 0.0}; with ``return_model`` also the
    ``EnsembleMSM`` of the reference's labels at ``lagtime``.  Only the reference needs time order.  Where the marginals of ``js_tica``
    cannot tell two basins that overlap in every coordinate from one, the states can."""
    labels = msm_states(ca_coords_dict, ref_key, lagtime, n_states, dim)
    results = js_of_states(labels, n_states, ref_key, weights)
    if return_model:
        return results, msm(labels[ref_key], n_states, lagtime)
    return results


def msm_states(ca_coords_dict, ref_key="target", lagtime=20, n_states=100, dim=4):
    """The first half of ``js_msm``: {key: coordinates or features} -> {key: int32 [R_k], the microstate of every structure}, the states
    being the k-means states of the reference's TICA projection."""
    k = _count("js_msm", "n_states", n_states)
    model = tica(ca_coords_dict[ref_key], lagtime, dim=dim)
    proj = {key: tica_project(v, model) for key, v in ca_coords_dict.items()}
    if k > len(proj[ref_key]):
        raise ValueError(f"js_msm: {k} states out of {len(proj[ref_key])} reference frames")
    states = kmeans(proj[ref_key], k)
    return {key: assign_states(p, states) for key, p in proj.items()}


def js_of_states(labels, n_states, ref_key="target", weights=None):
    """The second half of ``js_msm``: {key: state labels} -> {key: JS distance of the (weighted) state histogram from the reference's}."""
    w = _weights(weights, labels)
    return js_of_histograms({key: np.bincount(lab, weights=w[key], minlength=int(n_states)) + PSEUDO_C for key, lab in labels.items()}, ref_key)


# ---- pair scores: RMSD, TM-score and lDDT as one family ------------------------------------------------------------------------------
COVERAGE_CHUNK_PAIRS = 1 << 24   # pairs per launch of a coverage or cluster walk: 128 MiB of float64 scores at a time, whatever the ensembles' sizes


class PairScore(NamedTuple):
    """A score of one structure against another, described for the ensemble summaries every such score gets (``_diversity``,
    ``_coverage``, ``_cluster``)."""
    matrix: Callable          # (a, b=None, **kwargs) -> device float64 [Ra, Rb]: ops.ca_rmsd_matrix, ops.ca_tm_matrix, ops.ca_lddt_matrix
    higher_is_better: bool
    self_value: float         # of a structure against itself
    symmetric: bool           # matrix(a)[i, j] is matrix(a)[j, i] bit for bit; otherwise the structure of the row is the reference of a pair
    reference_rows: bool      # a coverage walk takes its rows from the reference ensemble (the lDDT references), not from the samples


RMSD = PairScore(ops.ca_rmsd_matrix, higher_is_better=False, self_value=0.0, symmetric=True, reference_rows=False)
TM = PairScore(ops.ca_tm_matrix, higher_is_better=True, self_value=1.0, symmetric=True, reference_rows=False)
LDDT = PairScore(ops.ca_lddt_matrix, higher_is_better=True, self_value=1.0, symmetric=False, reference_rows=True)


def _chunk_rows(n: int, chunk_pairs) -> int:
    return ops.rmsd_row_chunk(n, COVERAGE_CHUNK_PAIRS if chunk_pairs is None else chunk_pairs)


def _diversity(score: PairScore, ca_coords_dict, **kwargs):
    """Per ensemble the mean score over its pairs i != j (``self_value`` for a single structure)."""
    out = {}
    for k, v in ca_coords_dict.items():
        x = _dev(v)
        n = x.shape[0]
        if n <= 1:
            out[k] = score.self_value
        elif score.symmetric:   # (the diagonal is ``self_value`` up to rounding, which the upper-triangle sum leaves out)
            out[k] = np.around(float(torch.triu(score.matrix(x, None, **kwargs), diagonal=1).sum()) / (n * (n - 1) / 2), decimals=4)
        else:                   # (the diagonal is exactly ``self_value``)
            out[k] = np.around((float(score.matrix(x, None, **kwargs).sum()) - n * score.self_value) / (n * (n - 1)), decimals=4)
    return out


def _coverage_extrema(score: PairScore, samples: torch.Tensor, ref: torch.Tensor, chunk_pairs=None, **kwargs):
    """(per reference frame: its best score with any sample, per sample: its best score with any reference frame), device float64, over
    row chunks of the matrix with running extrema: the matrix itself is never held, and an extremum is exact whatever the chunking."""
    row_set, col_set = (ref, samples) if score.reference_rows else (samples, ref)
    best, running, start = ("max", torch.maximum, -float("inf")) if score.higher_is_better else ("min", torch.minimum, float("inf"))
    rows = _chunk_rows(col_set.shape[0], chunk_pairs)
    per_col = torch.full((col_set.shape[0],), start, dtype=torch.float64, device=ref.device)
    per_row = torch.empty(row_set.shape[0], dtype=torch.float64, device=ref.device)
    for r0 in range(0, row_set.shape[0], rows):
        m = score.matrix(row_set[r0:r0 + rows], col_set, **kwargs)
        per_row[r0:r0 + rows] = getattr(m, best)(dim=1).values
        per_col = running(per_col, getattr(m, best)(dim=0).values)
    return (per_row, per_col) if score.reference_rows else (per_col, per_row)


def _coverage(score: PairScore, ca_coords_dict, ref_key, chunk_pairs=None, **kwargs):
    """-> (recall, precision): per ensemble the mean over the reference frames of the best score with any of its samples, and the mean
    over its samples of the best score with any reference frame; the reference's own entries are ``self_value``."""
    ref = _dev(ca_coords_dict[ref_key])
    recall, precision = {}, {}
    for k, v in ca_coords_dict.items():
        if k == ref_key:
            continue
        per_ref, per_sample = _coverage_extrema(score, _dev(v), ref, chunk_pairs, **kwargs)
        recall[k] = np.around(float(per_ref.mean()), decimals=4)
        precision[k] = np.around(float(per_sample.mean()), decimals=4)
    recall[ref_key] = precision[ref_key] = score.self_value
    return recall, precision


# ---- minimum RMSD under optimal superposition (csrc/ensemble_rmsd.hip) -----------------------------------------------------------


def pairwise_rmsd(a, b=None, weights=None) -> np.ndarray:
    """Minimum RMSD of every structure of ``a`` [Ra, L, 3] against every structure of ``b`` [Rb, L, 3] (default: ``a`` itself; the self
    matrix is exactly symmetric) -> float64 [Ra, Rb]."""
    return ops.ca_rmsd_matrix(_dev(a), None if b is None else _dev(b), weights).cpu().numpy()


def diversity_rmsd(ca_coords_dict, weights=None):
    """Ensemble diversity: the mean RMSD over the pairs i < j of each ensemble (0.0 for a single structure)."""
    return _diversity(RMSD, ca_coords_dict, weights=weights)


def coverage_rmsd(ca_coords_dict, ref_key="target", weights=None, chunk_pairs=None):
    """How well each ensemble covers the reference ensemble -> (recall, precision): recall[k] = mean over reference frames of the
    minimum RMSD to any sample of k, precision[k] = mean over samples of k of the minimum RMSD to any reference frame."""
    return _coverage(RMSD, ca_coords_dict, ref_key, chunk_pairs, weights=weights)


def superpose(coords, target, weights=None):
    """Every structure of ``coords`` [R, L, 3] moved onto ``target`` [L, 3] by its optimal proper rotation + translation
    -> (aligned float32 [R, L, 3], rmsd float64 [R])."""
    x = _dev(coords)
    rmsd, xform = ops.ca_superpose(x, _dev(target)[0], weights)
    return ops.apply_xform(x, xform).cpu().numpy(), rmsd.cpu().numpy()


def rmsf(coords, target=None, weights=None) -> np.ndarray:
    """Per-residue root-mean-square fluctuation of an ensemble [R, L, 3] after superposition on ``target`` (default: its first
    structure): sqrt(mean over samples |x - mean x|^2) -> float64 [L]."""
    x = _dev(coords)
    rmsd, xform = ops.ca_superpose(x, x[0] if target is None else _dev(target)[0], weights)
    y = ops.apply_xform(x, xform).double()
    return (y - y.mean(0, keepdim=True)).square().sum(-1).mean(0).sqrt().cpu().numpy()


# ---- TM-score under the identity correspondence (csrc/ensemble_tm.hip) ------------------------------------------------------------
def tm_d0(L: int) -> float:
    """The TM-score's distance scale for chains of L residues: max(0.5, 1.24 cbrt(L - 15) - 1.8) for L > 15, else 0.5 (A)."""
    return max(0.5, 1.24 * float(np.cbrt(L - 15.0)) - 1.8) if L > 15 else 0.5


def pairwise_tm(a, b=None, d0=None) -> np.ndarray:
    """TM-score of every structure of ``a`` [Ra, L, 3] against every structure of ``b`` [Rb, L, 3] (default: ``a`` itself; the self
    matrix is exactly symmetric) -> float64 [Ra, Rb].  Residue i is matched with residue i and the score is normalised by the common
    length L (the TMscore program's convention, not TM-align's); ``d0`` overrides ``tm_d0(L)``.  The superposition search is a fixed
    monotone one (33 reweighted Kabsch steps from each of at most 16 seed windows): every value is the score of a real
    superposition, hence a lower bound of the optimum -- a heuristic, like the original program's search."""
    return ops.ca_tm_matrix(_dev(a), None if b is None else _dev(b), d0).cpu().numpy()


def diversity_tm(ca_coords_dict):
    """Ensemble diversity: the mean TM-score over the pairs i < j of each ensemble (1.0 for a single structure).  LOWER means more
    diverse, the opposite sense of ``diversity_rmsd``."""
    return _diversity(TM, ca_coords_dict)


def coverage_tm(ca_coords_dict, ref_key="target", chunk_pairs=None):
    """How well each ensemble covers the reference ensemble -> (recall, precision): recall[k] = mean over reference frames of the
    maximum TM-score to any sample of k, precision[k] = mean over samples of k of the maximum TM-score to any reference frame
    (higher is better; the reference's own entries are 1.0)."""
    return _coverage(TM, ca_coords_dict, ref_key, chunk_pairs)


def tm_superpose(coords, target):
    """Every structure of ``coords`` [R, L, 3] moved onto ``target`` [L, 3] by the superposition that scored its TM-score (it favours
    the well-matching part of the chain where ``superpose`` minimises the RMSD of all of it) -> (aligned float32 [R, L, 3], tm float64 [R])."""
    x = _dev(coords)
    tm, xform = ops.ca_tm_superpose(x, _dev(target)[0])
    return ops.apply_xform(x, xform).cpu().numpy(), tm.cpu().numpy()


# ---- lDDT: no superposition (csrc/ensemble_lddt.hip; the definition of src/models/loss.py:384-460) -------------------------------------
def pairwise_lddt(a, b=None, cutoff=15.0, min_seq_sep=1) -> np.ndarray:
    """CA-lDDT of every structure of ``b`` [Rb, L, 3] (default: ``a`` itself) in the environment of every structure of ``a`` [Ra, L, 3]
    -> float64 [Ra, Rb] in [0, 1].  Entry (i, j): of the pairs of residues of ``a[i]`` closer than ``cutoff`` A and at least ``min_seq_sep``
    apart in sequence, the mean fraction of the thresholds 0.5 / 1 / 2 / 4 A within which ``b[j]`` keeps the distance.  Not symmetric."""
    return ops.ca_lddt_matrix(_dev(a), None if b is None else _dev(b), cutoff, min_seq_sep).cpu().numpy()


def lddt(coords, target, per_residue=False) -> np.ndarray:
    """CA-lDDT of every structure of ``coords`` [R, L, 3] against the reference ``target`` [L, 3] -> float64 [R], or with ``per_residue``
    [R, L] (1.0 for a residue the target gives no partner), the reference's ``lddt(..., per_residue=)`` at cutoff 15 A."""
    per_res, total = ops.ca_lddt_per_residue(_dev(coords), _dev(target)[0])
    return (per_res if per_residue else total).cpu().numpy()


def diversity_lddt(ca_coords_dict):
    """Ensemble diversity: the mean lDDT over the ordered pairs i != j of each ensemble (1.0 for a single structure).  LOWER means more
    diverse, the sense of ``diversity_tm``."""
    return _diversity(LDDT, ca_coords_dict)


def coverage_lddt(ca_coords_dict, ref_key="target", chunk_pairs=None):
    """How well each ensemble covers the reference ensemble -> (recall, precision), the reference ensemble's frames being the lDDT
    references: recall[k] = mean over reference frames of the best lDDT any sample of k reaches in that frame's environment, precision[k]
    = mean over samples of k of its best lDDT in any reference frame's environment (higher is better; the reference's own entries are 1.0)."""
    return _coverage(LDDT, ca_coords_dict, ref_key, chunk_pairs)


# ---- contacts: which residues touch (csrc/ensemble_contacts.hip; CA atoms, the identity correspondence) -----------------------------------
def contact_map(coords, cutoff=8.0, min_seq_sep=3, weights=None) -> np.ndarray:
    """The contact-probability map of the ensemble ``coords`` [R, L, 3] -> float64 [L, L], symmetric: the fraction of structures (with
    per-structure ``weights`` [R]: of their weight) in which residues i and j, at least ``min_seq_sep`` apart in sequence, have CA atoms
    closer than ``cutoff`` A.  0 inside the band |i - j| < min_seq_sep."""
    n = len(coords) if np.ndim(coords) == 3 else 1
    if weights is None:
        return ops.ca_contact_map(_dev(coords), cutoff, min_seq_sep)[0].cpu().numpy() / float(n)
    w = np.asarray(weights, dtype=np.float64)
    if w.shape != (n,):
        raise ValueError(f"weights has shape {w.shape} for {n} structures")
    return ops.ca_contact_map(_dev(coords), cutoff, min_seq_sep, torch.as_tensor(w, device="cuda"))[1].cpu().numpy() / w.sum()


def contact_order(coords, cutoff=8.0, min_seq_sep=3) -> np.ndarray:
    """The relative contact order (Plaxco, Simons and Baker 1998) of every structure of ``coords`` [R, L, 3] -> float64 [R]: the mean
    sequence separation of its contacts over the chain length, 0.0 for a structure without contacts."""
    x = _dev(coords)
    n, sep_sum = (t.cpu().numpy() for t in ops.ca_contact_stats(x, cutoff, min_seq_sep))
    return np.where(n > 0, sep_sum.astype(np.float64) / (float(x.shape[1]) * np.maximum(n, 1)), 0.0)


def native_contacts(native, cutoff=8.0, min_seq_sep=4):
    """The native contact list of ``native`` [L, 3] -> (pairs [n, 2] int32 in ascending (i, j) order, d0 [n] float64: their distances).
    The defaults are those of Best, Hummer and Eaton (2013) on CA atoms: closer than 8 A, |i - j| > 3."""
    if np.ndim(native) != 2:
        raise ValueError(f"native has shape {np.shape(native)}, expected [L, 3]")
    pairs, d0 = ops.ca_native_contacts(_dev(native)[0], cutoff, min_seq_sep)
    return pairs.cpu().numpy(), d0.cpu().numpy()


def fraction_native_contacts(coords, native, soft=True, beta=5.0, lam=1.2, cutoff=8.0, min_seq_sep=4) -> np.ndarray:
    """Q of every structure of ``coords`` [R, L, 3] against the native contacts of ``native`` [L, 3] -> float64 [R].  ``soft``: the mean
    over the native contacts of 1 / (1 + exp(beta (d - lam d0))) (Best, Hummer and Eaton 2013; beta = 5 / A and lam = 1.2 are their
    values for CA models -- the native itself then scores slightly below 1); otherwise the fraction with d < lam d0.  1.0 when the native
    has no contact."""
    if np.ndim(native) != 2:
        raise ValueError(f"native has shape {np.shape(native)}, expected [L, 3]")
    x, nat = _dev(coords), _dev(native)[0]
    if nat.shape[0] != x.shape[1]:
        raise ValueError(f"native has {nat.shape[0]} residues for the ensemble's {x.shape[1]}")
    return q_of_contacts(x, *ops.ca_native_contacts(nat, cutoff, min_seq_sep), soft, beta, lam)


def q_of_contacts(coords, pairs, d0, soft=True, beta=5.0, lam=1.2) -> np.ndarray:
    """``fraction_native_contacts`` against a native contact list one already has (``native_contacts``'s arrays, or device tensors)."""
    q_soft, q_hard, _ = ops.ca_native_q(_dev(coords), *(torch.as_tensor(t, device="cuda") for t in (pairs, d0)), beta, lam)
    return (q_soft if soft else q_hard).cpu().numpy()


def contact_mae(ca_coords_dict, ref_key="target", cutoff=8.0, min_seq_sep=3, weights=None):
    """The mean absolute difference of each ensemble's contact-probability map from the reference ensemble's, over the pairs at least
    ``min_seq_sep`` apart (0.0 when there is none).  ``weights``: per-structure weights by key, as in ``js_pwd``."""
    w = _weights(weights, ca_coords_dict) if weights else {}
    return contact_mae_of({k: contact_map(v, cutoff, min_seq_sep, w.get(k)) for k, v in ca_coords_dict.items()}, ref_key, min_seq_sep)


def contact_mae_of(maps, ref_key="target", min_seq_sep=3):
    """``contact_mae`` of contact-probability maps {k: [L, L]} one already has."""
    return against_reference({k: m[np.triu_indices(len(m), k=min_seq_sep)] for k, m in maps.items()}, ref_key)


def _q_by_key(ca_coords_dict, ref_key, native, **q_args):
    """Q of every ensemble against ``native`` (None: the first structure of the reference ensemble) -> {k: float64 [len(v)]}."""
    return {k: fraction_native_contacts(v, ca_coords_dict[ref_key][0] if native is None else native, **q_args) for k, v in ca_coords_dict.items()}


def js_q(ca_coords_dict, ref_key="target", native=None, n_bins=50, weights=None, **q_args):
    """The Jensen-Shannon distance between each ensemble's distribution of the fraction of native contacts and the reference ensemble's:
    histograms of ``n_bins`` bins over the fixed range [0, 1].  ``native`` [L, 3]: None takes the first structure of the reference
    ensemble; ``q_args``: the arguments of ``fraction_native_contacts``."""
    w = _weights(weights, ca_coords_dict)
    return js_q_of(_q_by_key(ca_coords_dict, ref_key, native, **q_args), ref_key, n_bins, w)


def mean_q(ca_coords_dict, ref_key="target", native=None, weights=None, **q_args):
    """The (weighted) mean fraction of native contacts of each ensemble; the arguments of ``js_q``."""
    w = _weights(weights, ca_coords_dict)
    return mean_of_values(_q_by_key(ca_coords_dict, ref_key, native, **q_args), w)


# ---- backbone violations: inside each structure (csrc/ensemble_violations.hip; the definition of src/models/loss.py:714-1017, 1237-1314) ----
GLY = 7                                       # aatype of glycine in the reference's residue order: no CB
ATOM37_BACKBONE = (0, 1, 2, 4, 3)             # atom37 slots of N, CA, C, O, CB (atom14 slots 0 .. 4)


def _atom_exists(aatype: np.ndarray) -> np.ndarray:
    """aatype [L] -> uint8 [L, 5]: which of N, CA, C, O, CB a residue has (a GLY has no CB)."""
    return ((np.arange(5) < 4) | (aatype != GLY)[:, None]).astype(np.uint8)


class BackboneViolations(NamedTuple):
    """Per structure of an ensemble [R, L, 5, 3]: the four flat-bottom loss means and the four fractions of the reference's
    ``find_structural_violations`` / ``compute_violation_metrics`` (float64 [R]), the per-residue connection loss (float64 [R, L]),
    ``bond_mask`` [R, L] (a residue at a violated connection), ``clash_atom_mask`` [R, L, 5] (N, CA, C, O, CB in a clashing pair), both
    bool, and ``n_clash_pairs`` [R] int32."""
    c_n_loss_mean: np.ndarray
    ca_c_n_loss_mean: np.ndarray
    c_n_ca_loss_mean: np.ndarray
    clashes_mean_loss: np.ndarray
    violations_between_residue_bond: np.ndarray
    violations_between_residue_clash: np.ndarray
    violations_per_residue: np.ndarray
    violations_extreme_ca_ca_distance: np.ndarray
    per_residue_loss_sum: np.ndarray
    bond_mask: np.ndarray
    clash_atom_mask: np.ndarray
    n_clash_pairs: np.ndarray


def _backbone_dev(atoms) -> torch.Tensor:
    """[R, L, 5, 3] atom14 order, or [R, L, 37, 3] atom37 as the sampler returns it (one structure without the leading axis) -> device
    float32 [R, L, 5, 3]."""
    t = atoms if torch.is_tensor(atoms) else torch.as_tensor(np.asarray(atoms))
    if t.ndim == 3:
        t = t[None]
    if t.ndim != 4 or t.shape[-1] != 3 or t.shape[-2] not in (5, 37):
        raise ValueError(f"backbone atoms should be [R, L, 5, 3] (N, CA, C, O, CB) or [R, L, 37, 3] (atom37), got {tuple(t.shape)}")
    if t.shape[-2] == 37:
        t = t[:, :, list(ATOM37_BACKBONE)]
    return t.to("cuda", torch.float32).contiguous()


def backbone_violations(atoms, aatype=None, residue_index=None, tolerance_factor=12.0, clash_tolerance=1.5, max_structures=None) -> BackboneViolations:
    """Is every backbone of the ensemble chemically possible?  The reference's structural-violation terms between residues (bond length and
    the two angles at every peptide bond, clashes of the van der Waals spheres, extreme CA-CA steps; include/str2str_hip.h has the
    formulas) of ``atoms`` [R, L, 5, 3] or atom37 [R, L, 37, 3], for the one sequence ``aatype`` [L] (default: all ALA; a GLY has no CB)
    numbered ``residue_index`` [L] (default: 0 .. L - 1; a jump in the numbers is a chain break).  The tolerances are the reference's
    defaults."""
    x = _backbone_dev(atoms)
    aatype, residue_index = _sequence_arrays("backbone_violations", x.shape[1], aatype, residue_index)
    losses, fractions, per_res, bond_mask, clash_mask, n_pairs = ops.backbone_violations(x, _atom_exists(aatype), aatype, residue_index,
                                                                                         tolerance_factor, clash_tolerance, max_structures)
    return BackboneViolations(*losses.cpu().numpy().T, *fractions.cpu().numpy().T, per_res.cpu().numpy(), bond_mask.cpu().numpy().astype(bool),
                              clash_mask.cpu().numpy().astype(bool), n_pairs.cpu().numpy())


def validity_of_violations(res: BackboneViolations):
    """-> (the share of structures without a violated connection, the share without a clash) of one ensemble's violations."""
    return (np.around(1.0 - float(res.bond_mask.any(axis=1).mean()), decimals=4),
            np.around(1.0 - float((res.n_clash_pairs > 0).mean()), decimals=4))


def rate_of_violations(res: BackboneViolations):
    """-> the mean over the structures of ``violations_per_residue`` of one ensemble's violations."""
    return np.around(float(res.violations_per_residue.mean()), decimals=4)


def backbone_validity(atoms_dict, aatype=None, residue_index=None):
    """The full-backbone companions of ``validity`` / ``bonding_validity`` -> (val_bb_bond, val_bb_clash): per ensemble the share of
    structures without a violated connection, and without a clash."""
    shares = {k: validity_of_violations(backbone_violations(v, aatype, residue_index)) for k, v in atoms_dict.items()}
    return {k: v[0] for k, v in shares.items()}, {k: v[1] for k, v in shares.items()}


def violation_rate(atoms_dict, aatype=None, residue_index=None):
    """Per ensemble the mean over its structures of ``violations_per_residue``: the fraction of residues at a violated connection or with
    a clashing atom."""
    return {k: rate_of_violations(backbone_violations(v, aatype, residue_index)) for k, v in atoms_dict.items()}


# ---- secondary structure and backbone torsions (csrc/ensemble_ss.hip; Kabsch & Sander 1983, include/str2str_hip.h has the definition) ----
HELIX_STATES, STRAND_STATES = (b"H", b"G", b"I"), (b"E", b"B")


class SecondaryStructure(NamedTuple):
    """Per structure of an ensemble [R, L, 5, 3]: ``ss`` [R, L] numpy 'S1' (- B E H G I T S), ``n_hbonds`` [R] int32 (backbone hydrogen
    bonds), and DSSP's N-H -> O column: ``hbond_energy`` [R, L] float64 (kcal/mol) and ``hbond_partner`` [R, L] int32, the best acceptor
    of every amide hydrogen (0.0 and -1 where there is none)."""
    ss: np.ndarray
    n_hbonds: np.ndarray
    hbond_energy: np.ndarray
    hbond_partner: np.ndarray


def _sequence_arrays(fn, L, aatype, residue_index):
    """The defaults of the per-sequence arguments: all ALA, numbered 0 .. L - 1."""
    aatype = np.zeros(L, dtype=np.int64) if aatype is None else _host(aatype).reshape(-1)
    residue_index = np.arange(L) if residue_index is None else _host(residue_index).reshape(-1)
    if aatype.shape != (L,) or residue_index.shape != (L,):
        raise ValueError(f"{fn}: aatype {aatype.shape} and residue_index {residue_index.shape} for {L} residues")
    return aatype, residue_index


def secondary_structure(atoms, aatype=None, residue_index=None, max_structures=None) -> SecondaryStructure:
    """What is every conformation of the ensemble?  Kabsch & Sander's assignment (hydrogen-bond energy below -0.5 kcal/mol, n-turns,
    bridges, ladders, bends; the energy threshold alone makes a bond and beta-bulges are not merged: include/str2str_hip.h) of ``atoms``
    [R, L, 5, 3] or atom37 [R, L, 37, 3], for the one sequence ``aatype`` [L] (default: all ALA; a PRO has no amide hydrogen) numbered
    ``residue_index`` [L] (default: 0 .. L - 1; a jump in the numbers is a chain break)."""
    return secondary_structure_and_torsions(atoms, aatype, residue_index, max_structures)[0]


def secondary_structure_and_torsions(atoms, aatype=None, residue_index=None, max_structures=None, fn="secondary_structure"):
    """One launch -> (what ``secondary_structure`` returns, the two results of ``backbone_torsions``: they do not depend on ``aatype``)."""
    x = _backbone_dev(atoms)
    aatype, residue_index = _sequence_arrays(fn, x.shape[1], aatype, residue_index)
    ss, n_hbonds, energy, partner, angles = ops.secondary_structure(x, aatype, residue_index, max_structures)
    conn = np.append(False, np.diff(residue_index.astype(np.int64)) == 1)   # residue i follows i - 1 in the numbering
    return (SecondaryStructure(ss.cpu().numpy().view("S1"), n_hbonds.cpu().numpy(), energy.cpu().numpy(), partner.cpu().numpy()),
            angles.cpu().numpy(), np.stack([conn, np.append(conn[1:], False), conn], axis=1))


def ss_strings(result) -> list:
    """One string of state letters per structure of a ``SecondaryStructure`` (or of its ``ss`` array)."""
    ss = np.atleast_2d(result.ss if isinstance(result, SecondaryStructure) else result)
    return [row.tobytes().decode("ascii") for row in ss]


def backbone_torsions(atoms, residue_index=None):
    """-> (angles float64 [R, L, 3]: phi, psi, omega in radians in (-pi, pi], IUPAC sign, omega_i being the bond before residue i;
    mask bool [L, 3]: phi and omega are defined where residue i follows i - 1 in the numbering, psi where i + 1 follows i; an undefined
    angle is 0.0)."""
    return secondary_structure_and_torsions(atoms, None, residue_index, fn="backbone_torsions")[1:]


def _propensity(ss: np.ndarray) -> np.ndarray:
    """ss 'S1' [R, L] -> float64 [L, 3]: the fractions of the structures in which a residue is helix, strand, other."""
    helix, strand = np.isin(ss, HELIX_STATES), np.isin(ss, STRAND_STATES)
    return np.stack([helix.mean(0), strand.mean(0), (~helix & ~strand).mean(0)], axis=1)


def ss_propensity(atoms_dict, aatype=None, residue_index=None):
    """Per ensemble the per-residue fractions of helix (H, G, I), strand (E, B) and other -> {k: float64 [L, 3]}."""
    return {k: _propensity(secondary_structure(v, aatype, residue_index).ss) for k, v in atoms_dict.items()}


def ss_content(atoms_dict, aatype=None, residue_index=None):
    """-> (helix, strand): per ensemble the mean fraction of residues in helix (H, G, I) and in strand (E, B)."""
    return ss_content_of(ss_propensity(atoms_dict, aatype, residue_index))


def ss_content_of(prop):
    """``ss_content`` of propensities {k: [L, 3]} one already has."""
    return tuple({k: np.around(float(p[:, c].mean()), decimals=4) for k, p in prop.items()} for c in (0, 1))


def ss_mae(atoms_dict, ref_key="target", aatype=None, residue_index=None):
    """Per ensemble the mean over the residues of half the L1 distance of its (helix, strand, other) propensities from the reference
    ensemble's: 0 for equal propensities, 1 where every residue is in another class."""
    return ss_mae_of(ss_propensity(atoms_dict, aatype, residue_index), ref_key)


def _rama_histogram(angles: np.ndarray, mask: np.ndarray, n_bins: int = 36) -> np.ndarray:
    """The phi / psi histogram over [-pi, pi)^2 of every structure's residues with both angles defined, flattened, with PSEUDO_C."""
    both = mask[:, 0] & mask[:, 1]
    phi, psi = angles[:, both, 0].reshape(-1), angles[:, both, 1].reshape(-1)
    wrap = lambda a: np.where(a >= math.pi, a - 2.0 * math.pi, a)   # noqa: E731  (pi itself belongs to the first bin)
    h = np.histogram2d(wrap(phi), wrap(psi), bins=n_bins, range=((-math.pi, math.pi), (-math.pi, math.pi)))[0]
    return h.reshape(-1) + PSEUDO_C


def js_rama(atoms_dict, ref_key="target", n_bins=36, residue_index=None):
    """Jensen-Shannon distance of the Ramachandran (phi, psi) histograms, n_bins x n_bins over [-pi, pi)^2, pooled over all structures
    and all residues with both angles defined.  The angles come from the device; the histogram tail is numpy, as for ``js_rg``."""
    return js_of_histograms({k: _rama_histogram(*backbone_torsions(v, residue_index), n_bins) for k, v in atoms_dict.items()}, ref_key)


# ---- solvent accessibility (csrc/ensemble_sasa.hip; Shrake & Rupley 1973, include/str2str_hip.h has the definition) ----
SASA_RADII = (1.55, 1.7, 1.7, 1.52, 1.7)      # Bondi radii of N, CA, C, O, CB in Angstrom: the clash radii of the violations, MDTraj's, Biopython's


class SolventAccessibility(NamedTuple):
    """Per structure of an ensemble [R, L, 5, 3]: ``counts`` [R, L, 5] int32 (the accessible sphere points of N, CA, C, O, CB),
    ``per_residue`` [R, L] and ``total`` [R] float64 in square Angstrom."""
    counts: np.ndarray
    per_residue: np.ndarray
    total: np.ndarray


def solvent_accessibility(atoms, aatype=None, residue_index=None, radii=None, probe=1.4, n_points=96, max_structures=None) -> SolventAccessibility:
    """How much of each residue, and of the chain, does the solvent reach?  Shrake and Rupley's surface (``n_points`` test points on every
    atom's sphere of radius ``radii + probe``; include/str2str_hip.h) of ``atoms`` [R, L, 5, 3] or atom37 [R, L, 37, 3], for the one
    sequence ``aatype`` [L] (default: all ALA; a GLY has no CB).  ``radii`` [L, 5]: SASA_RADII for every residue by default.
    ``residue_index`` is accepted like its siblings' and not used: a surface knows no chain breaks.  NOT an all-atom surface: there are no
    side chains beyond CB, so absolute values overstate the exposure of large residues."""
    return accessibility(atoms, aatype, residue_index, radii, probe, n_points, max_structures, False, "solvent_accessibility")[0]


def relative_accessibility(atoms, aatype=None, residue_index=None, radii=None, probe=1.4, n_points=96, max_structures=None) -> np.ndarray:
    """-> float64 [R, L] in [0, 1]: each residue's surface in the chain over the surface of the same residue's own atoms alone (the same
    conformation of its five atoms, the rest of the chain taken away), the share of its own surface that the rest of the chain leaves
    exposed (NaN for a residue none of whose atoms exists).  The denominator comes from the same kernel on the residues as one-residue
    structures.  NOT the relative accessibility against tabulated Gly-X-Gly maxima: no such table is in the tree."""
    return accessibility(atoms, aatype, residue_index, radii, probe, n_points, max_structures, True, "relative_accessibility")[1]


def accessibility(atoms, aatype=None, residue_index=None, radii=None, probe=1.4, n_points=96, max_structures=None, relative=True, fn="accessibility"):
    """One launch on the chains -> (what ``solvent_accessibility`` returns, what ``relative_accessibility`` returns or None without ``relative``)."""
    x = _backbone_dev(atoms)
    R, L = x.shape[:2]
    aatype, _ = _sequence_arrays(fn, L, aatype, residue_index)
    exists = _atom_exists(aatype)
    radii = np.tile(np.asarray(SASA_RADII, dtype=np.float64), (L, 1)) if radii is None else _host(radii, np.float64)
    if radii.shape != (L, 5):
        raise ValueError(f"{fn}: radii {radii.shape} for {L} residues, expected [{L}, 5]")
    counts, in_chain, total = ops.backbone_sasa(x, exists, radii, probe, n_points, max_structures)
    res = SolventAccessibility(counts.cpu().numpy(), in_chain.cpu().numpy(), total.cpu().numpy())
    if not relative:
        return res, None
    alone = torch.empty_like(in_chain)
    kinds, kind_of = np.unique(np.concatenate([radii, exists.astype(np.float64)], axis=1), axis=0, return_inverse=True)
    for q in range(len(kinds)):                                 # the residues that share radii and existing atoms share a launch sequence
        idx = torch.as_tensor(np.nonzero(kind_of.reshape(-1) == q)[0], device=x.device)
        own = x[:, idx].reshape(-1, 1, 5, 3).contiguous()
        r0 = int(idx[0])
        alone[:, idx] = ops.backbone_sasa(own, exists[r0:r0 + 1], radii[r0:r0 + 1], probe, n_points, max_structures)[1].reshape(R, len(idx))
    return res, (in_chain / alone).cpu().numpy()


def mean_sasa(atoms_dict, aatype=None, residue_index=None, **sasa_args):
    """Per ensemble the mean total solvent-accessible surface of its structures in square Angstrom; ``sasa_args``: those of ``solvent_accessibility``."""
    return mean_of_values({k: solvent_accessibility(v, aatype, residue_index, **sasa_args).total for k, v in atoms_dict.items()})


def sasa_mae(atoms_dict, ref_key="target", aatype=None, residue_index=None, **sasa_args):
    """Per ensemble the mean over the residues of the absolute difference of its mean relative accessibility from the reference ensemble's."""
    return against_reference({k: relative_accessibility(v, aatype, residue_index, **sasa_args).mean(0) for k, v in atoms_dict.items()}, ref_key)


def js_sasa(atoms_dict, ref_key="target", n_bins=50, weights=None, aatype=None, residue_index=None, **sasa_args):
    """``js_of_values`` of the structures' total surface: histograms of ``n_bins`` bins over the range of the reference ensemble, as in ``js_rg``."""
    w = _weights(weights, atoms_dict)
    return js_of_values({k: solvent_accessibility(v, aatype, residue_index, **sasa_args).total for k, v in atoms_dict.items()}, ref_key, n_bins, w)


# ---- solution scattering (csrc/ensemble_saxs.hip; Debye 1915, Kirkwood 1954; include/str2str_hip.h has the definition) ----
SAXS_Q_GRID = np.arange(51) / 100.0           # 0.00, 0.01, ..., 0.50 per Angstrom: the grid of eval.py, inside the range of the CA-bead approximation


def saxs_profile_and_rh(coords, q, aatype=None, form_factors=None, max_structures=None):
    """-> (what ``saxs_profile`` returns, what ``hydrodynamic_radius`` returns: it depends neither on ``q`` nor on the form factors):
    ``ops.ca_scattering`` walked over the q-list in runs of ops.SAXS_MAX_Q (whole tiles, so every column has the bytes of a single call)."""
    x = _dev(coords)
    q = _host(q, np.float64)
    if q.ndim != 1 or q.size < 1:
        raise ValueError(f"q has shape {q.shape}, expected [Q] with Q >= 1")
    table = types = None
    if form_factors is not None:
        table = _host(form_factors, np.float64)
        if table.ndim != 2 or table.shape[1] != q.size:
            raise ValueError(f"form_factors has shape {table.shape} for {q.size} q-values, expected [n_types, {q.size}]")
        types = None if aatype is None else _host(aatype)
        if types is not None and types.shape != (x.shape[1],):
            raise ValueError(f"aatype has shape {types.shape} for {x.shape[1]} residues")
    runs = [ops.ca_scattering(x, q[k:k + ops.SAXS_MAX_Q], types, None if table is None else table[:, k:k + ops.SAXS_MAX_Q], max_structures)
            for k in range(0, q.size, ops.SAXS_MAX_Q)]
    with np.errstate(divide="ignore"):
        return np.concatenate([r[0].cpu().numpy() for r in runs], axis=1), 1.0 / runs[0][1].cpu().numpy()


def saxs_profile(coords, q, aatype=None, form_factors=None, max_structures=None) -> np.ndarray:
    """What would a SAXS measurement see of each structure?  The Debye intensity I(q) = sum_i f_i^2 + 2 sum_{i<j} f_i f_j sin(q r_ij) /
    (q r_ij) of the CA beads of ``coords`` [R, L, 3] at the ``q`` [Q] (1/Angstrom) -> float64 [R, Q].  By default every residue is the same
    point scatterer (f = 1, I(0) = L^2), the usual CA-bead approximation, good for q <~ 0.3 / Angstrom.  A caller with residue form factors
    passes ``form_factors`` [n_types, Q] (any sign: contrast can be negative) and ``aatype`` [L] (the row of every residue; without
    ``form_factors`` it is not used).  NOT here: a hydration shell, an excluded-volume term, a built-in form-factor table, side chains."""
    return saxs_profile_and_rh(coords, q, aatype, form_factors, max_structures)[0]


def ensemble_saxs(coords, q, weights=None, aatype=None, form_factors=None, max_structures=None) -> np.ndarray:
    """The curve of the ensemble -> float64 [Q]: the (``weights`` [R]: weighted) mean of the structures' *intensities*, which is what a
    solution of them scatters."""
    return mean_curve(saxs_profile(coords, q, aatype, form_factors, max_structures), weights)


def mean_curve(rows, weights=None) -> np.ndarray:
    """``ensemble_saxs`` of the structures' intensities [R, Q] one already has."""
    w = None if weights is None else np.asarray(weights, dtype=np.float64)
    if w is not None and w.shape != (len(rows),):
        raise ValueError(f"weights has shape {w.shape} for {len(rows)} structures")
    return np.average(rows, axis=0, weights=w)   # (None: the plain mean)


def hydrodynamic_radius(coords, max_structures=None) -> np.ndarray:
    """Kirkwood's hydrodynamic radius of the CA beads of every structure of ``coords`` [R, L, 3] -> float64 [R] in Angstrom:
    1 / Rh = (1 / L^2) sum_{i != j} 1 / r_ij.  inf for a single bead, 0 where two beads coincide.  No Nygaard or other correction."""
    return saxs_profile_and_rh(coords, [0.0], None, None, max_structures)[1]


def saxs_mae(ca_coords_dict, ref_key="target", q=None, weights=None, **saxs_args):
    """Per ensemble the mean over ``q`` (SAXS_Q_GRID by default) of |I - I_ref| / I_ref, I the ensemble's curve (``ensemble_saxs``) and I_ref
    the reference ensemble's.  ``weights``: per-structure weights by key, as in ``js_pwd``; ``saxs_args``: ``aatype``, ``form_factors``."""
    q = SAXS_Q_GRID if q is None else q
    w = _weights(weights, ca_coords_dict) if weights else {}
    return saxs_mae_of({k: ensemble_saxs(v, q, w.get(k), **saxs_args) for k, v in ca_coords_dict.items()}, ref_key)


def mean_rh(ca_coords_dict, weights=None):
    """The (weighted) mean hydrodynamic radius of each ensemble in Angstrom."""
    w = _weights(weights, ca_coords_dict)
    return mean_of_values({k: hydrodynamic_radius(v) for k, v in ca_coords_dict.items()}, w)


def js_rh(ca_coords_dict, ref_key="target", n_bins=50, weights=None):
    """``js_of_values`` of the structures' hydrodynamic radius: histograms of ``n_bins`` bins over the range of the reference ensemble, as in ``js_rg``."""
    w = _weights(weights, ca_coords_dict)
    return js_of_values({k: hydrodynamic_radius(v) for k, v in ca_coords_dict.items()}, ref_key, n_bins, w)


def saxs_chi2(intensity, i_exp, sigma, background=False):
    """A computed curve against a measured one on the same q grid -> (chi2, scale, background): the weighted least-squares fit
    i_exp ~ scale * intensity (+ a constant with ``background``) in closed form, and its reduced chi^2 = sum(((scale * intensity +
    background - i_exp) / sigma)^2) / (Q - 1) (Q - 2 with the constant).  ``background`` is returned as 0.0 when it is not fitted."""
    i_calc, i_exp, sigma = (np.asarray(v, dtype=np.float64) for v in (intensity, i_exp, sigma))
    dof = 2 if background else 1
    if i_calc.ndim != 1 or i_exp.shape != i_calc.shape or sigma.shape != i_calc.shape or i_calc.size <= dof:
        raise ValueError(f"saxs_chi2: curves of shapes {i_calc.shape}, {i_exp.shape}, {sigma.shape}: expected three [Q] with Q > {dof}")
    if not (np.isfinite(sigma) & (sigma > 0.0)).all():
        raise ValueError("saxs_chi2: sigma must be finite and positive")
    w = 1.0 / (sigma * sigma)
    s_cc, s_ce = float((w * i_calc * i_calc).sum()), float((w * i_calc * i_exp).sum())
    if background:
        s_w, s_c, s_e = float(w.sum()), float((w * i_calc).sum()), float((w * i_exp).sum())
        det = s_cc * s_w - s_c * s_c
        scale, const = (s_ce * s_w - s_c * s_e) / det, (s_cc * s_e - s_c * s_ce) / det
    else:
        scale, const = s_ce / s_cc, 0.0
    resid = (scale * i_calc + const - i_exp) / sigma
    return float((resid * resid).sum()) / (i_calc.size - dof), float(scale), float(const)


def read_saxs_dat(path, q_unit="1/A"):
    """A measured curve from a three-column text file (q, I, sigma; whitespace-separated, ``#`` starts a comment) -> (q in 1/Angstrom, I,
    sigma) float64 [Q].  Lines that are not three numbers (headers, footers) are skipped, rows with sigma <= 0 or a non-finite value dropped.  ``q_unit``:
    "1/A", or "1/nm" (q is divided by 10)."""
    if q_unit not in ("1/A", "1/nm"):
        raise ValueError(f"read_saxs_dat: q_unit {q_unit!r}: expected '1/A' or '1/nm'")
    rows = []
    with open(path) as f:
        for line in f:
            fields = line.split("#", 1)[0].split()
            if len(fields) != 3:
                continue
            try:
                row = [float(v) for v in fields]
            except ValueError:
                continue
            if all(math.isfinite(v) for v in row) and row[2] > 0.0:
                rows.append(row)
    data = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    return (data[:, 0] / 10.0 if q_unit == "1/nm" else data[:, 0].copy()), data[:, 1].copy(), data[:, 2].copy()


# ---- essential dynamics: covariance, PCA, cross-correlation (csrc/ensemble_pca.hip; include/str2str_hip.h has the definition) ----
class EnsemblePCA(NamedTuple):
    """The principal components of the superposed CA coordinates of an ensemble [R, L, 3], float64: ``mean`` [L, 3] (the mean structure
    the covariance is taken about), ``components`` [K, 3L] (orthonormal rows, coordinate 3 i + a, descending variance, every row's
    largest-magnitude entry positive), ``variances`` [K] (A^2, clamped at 0), ``total_variance`` (tr C, the sum of the squared RMSF) and
    ``projections`` [R, K] (the fitted structures themselves, under the transforms that made the covariance, on the components)."""
    mean: np.ndarray
    components: np.ndarray
    variances: np.ndarray
    total_variance: float
    projections: np.ndarray


def _aligned_moments(x, xform, sample_weights=None, max_structures=None):
    """-> device float64 (mean [L, 3], covariance [3L, 3L]) of the ensemble x under ``xform`` (None: the identity): two-pass."""
    mean = ops.ca_aligned_mean(x, xform, sample_weights)
    return mean, ops.ca_covariance(x, mean, xform, sample_weights, max_structures)


def _fit_and_moments(coords, target, sample_weights, residue_weights, n_fit_rounds, fit):
    x = _dev(coords)
    xform = ops.ca_fit_transforms(x, None if target is None else _dev(target)[0], sample_weights, residue_weights, n_fit_rounds, fit)
    return (x, xform, *_aligned_moments(x, xform, sample_weights))


def ensemble_covariance(coords, target=None, sample_weights=None, residue_weights=None, n_fit_rounds=5, fit=True):
    """How does the ensemble move?  -> (mean [L, 3], covariance [3L, 3L]) float64 of the CA coordinates ``coords`` [R, L, 3] after
    superposition: every structure is superposed (``superpose``'s optimal proper rotation + translation, per-residue ``residue_weights``
    [L] if given) onto ``target`` [L, 3] (default: the first structure), ``n_fit_rounds`` times, the target of every further round being the
    mean of the superposed structures rounded to float32 -- a fixed count, no data-dependent stop.  ``fit=False``: the input is already
    aligned.  With y_s the transformed structure in float64 (never rounded to float32) and p = ``sample_weights`` [R] (>= 0, normalised
    to sum 1; default 1 / R): mean = sum_s p_s y_s and C[3i+a, 3j+b] = sum_s p_s (y_sia - m_ia)(y_sjb - m_jb), the population covariance (no
    Bessel factor), two-pass, exactly symmetric.  One structure gives all zeros.  CA atoms only, at most ops.PCA_MAX_RES residues."""
    _, _, mean, cov = _fit_and_moments(coords, target, sample_weights, residue_weights, n_fit_rounds, fit)
    return mean.cpu().numpy(), cov.cpu().numpy()


def _dccm(cov: torch.Tensor) -> torch.Tensor:
    """Covariance [3L, 3L] -> [L, L]: c_ij = tr C_ij / sqrt(tr C_ii tr C_jj) over the 3 x 3 blocks; the diagonal is exactly 1, c_ij = 0
    wherever either trace is 0 (a residue that does not move)."""
    L = cov.shape[0] // 3
    blocks = cov.reshape(L, 3, L, 3)
    tr = (blocks[:, 0, :, 0] + blocks[:, 1, :, 1]) + blocks[:, 2, :, 2]
    d = tr.diagonal()
    den = (d[:, None] * d[None, :]).sqrt()
    c = torch.where(den > 0.0, tr / torch.where(den > 0.0, den, torch.ones_like(den)), torch.zeros_like(tr)).clamp(-1.0, 1.0)
    c.fill_diagonal_(1.0)
    return c


def cross_correlation(coords, target=None, sample_weights=None, residue_weights=None, n_fit_rounds=5, fit=True) -> np.ndarray:
    """Which residues move together?  The dynamical cross-correlation map of ``ensemble_covariance``'s C (same arguments) -> float64 [L, L]
    in [-1, 1]: c_ij = <dr_i . dr_j> / sqrt(<|dr_i|^2> <|dr_j|^2>) = tr C_ij / sqrt(tr C_ii tr C_jj).  The diagonal is exactly 1; c_ij = 0
    where residue i or j does not move at all."""
    return _dccm(_fit_and_moments(coords, target, sample_weights, residue_weights, n_fit_rounds, fit)[3]).cpu().numpy()


def _top_components(cov: np.ndarray, k: int):
    """The ``k`` largest eigenpairs of the symmetric ``cov`` -> (variances [k] descending, clamped at 0; components [k, n], every row's
    largest-magnitude entry positive: the rule of ``tica_fit``'s ``canonical``)."""
    import scipy.linalg

    n = cov.shape[0]
    vals, vecs = scipy.linalg.eigh(cov, subset_by_index=[n - k, n - 1])
    vals, vecs = vals[::-1], vecs[:, ::-1].T
    top = np.argmax(np.abs(vecs), axis=1)
    sign = np.sign(vecs[np.arange(k), top])
    return np.maximum(vals, 0.0), np.ascontiguousarray(vecs * np.where(sign == 0.0, 1.0, sign)[:, None])


def _at_least_two(fn, x):
    if x.shape[0] < 2:
        raise ValueError(f"{fn}: needs at least 2 structures, got {x.shape[0]}")
    return x


def pca(coords, n_components=10, target=None, sample_weights=None, residue_weights=None, n_fit_rounds=5, fit=True) -> EnsemblePCA:
    """Which collective coordinates carry the variance?  Principal components of ``ensemble_covariance``'s C (same arguments; R >= 2):
    the top ``n_components`` (1 .. 3L) eigenpairs in descending eigenvalue order with canonical signs, variances clamped at 0.  The mean,
    the covariance and the projections run on the device; the symmetric 3L x 3L eigenproblem runs on the host (scipy.linalg.eigh, as
    ``tica_fit``'s does), for the top components only: 0.23 s at 3L = 768 and 0.46 s at 3L = 3072 for ten of them (profiles/pca_timing.md;
    a full decomposition at 3072 is on the order of 10 s, an unmeasured estimate), against milliseconds on the device.  It is well-posed for
    the top components even with fewer structures than coordinates (at most R - 1 variances are non-zero).  Cartesian PCA of ONE global
    superposition: a hinge smears across components (``lddt`` and ``contact_map`` are the superposition-free tools)."""
    x = _at_least_two("pca", _dev(coords))
    n3 = 3 * x.shape[1]
    if isinstance(n_components, bool) or int(n_components) != n_components or not 1 <= n_components <= n3:
        raise ValueError(f"pca: n_components must be an integer in 1 .. {n3}, got {n_components}")
    x, xform, mean, cov = _fit_and_moments(x, target, sample_weights, residue_weights, n_fit_rounds, fit)
    cov_h = cov.cpu().numpy()
    variances, components = _top_components(cov_h, int(n_components))
    proj = ops.ca_project(x, mean, torch.as_tensor(components, device=x.device), xform)
    return EnsemblePCA(mean.cpu().numpy(), components, variances, float(np.trace(cov_h)), proj.cpu().numpy())


def pca_project(coords, model: EnsemblePCA, residue_weights=None) -> np.ndarray:
    """``coords`` [R, L, 3] on the components of ``model`` -> float64 [R, K]: every structure is superposed ONCE onto the model's mean
    structure (rounded to float32), then proj[s, k] = sum_c (y_sc - mean_c) v_kc with y in float64."""
    x = _dev(coords)
    mean = torch.as_tensor(np.asarray(model.mean, dtype=np.float64), device=x.device).contiguous()
    comps = torch.as_tensor(np.asarray(model.components, dtype=np.float64), device=x.device).contiguous()
    xform = ops.ca_superpose(x, mean.to(torch.float32), residue_weights)[1]
    return ops.ca_project(x, mean, comps, xform).cpu().numpy()


def js_of_columns(values, ref_key="target", n_bins=50, weights=None):
    """{k: float64 [R_k, K], K numbers per structure} -> {k: the mean over the K columns of the JS distance from the reference's}:
    per column histograms of ``n_bins`` bins over the reference's range with per-structure ``weights`` by key and PSEUDO_C."""
    w = _weights(weights, values)
    lo, hi = values[ref_key].min(axis=0), values[ref_key].max(axis=0)
    hist = {k: np.stack([np.histogram(v[:, c], bins=n_bins, weights=w[k], range=(lo[c], hi[c]))[0] + PSEUDO_C for c in range(v.shape[1])])
            for k, v in values.items()}                      # [K, n_bins]
    return against_reference(hist, ref_key, lambda h, ref: np.mean([_js(a, b) for a, b in zip(h, ref)]))


def js_pca(ca_coords_dict, ref_key="target", n_bins=50, n_components=2, weights=None, return_pc=True):
    """Does each ensemble populate the reference's essential subspace the way the reference does?  PCA (``n_components``, fitted on the
    reference ensemble -- no time order needed, unlike ``js_tica``) -> every ensemble, the reference included, through ``pca_project`` ->
    ``n_bins``-bin histograms over the reference's range per component -> mean Jensen-Shannon distance.  ``weights``: per-structure
    weights by key, as in ``js_pwd``; the reference's also weight its PCA.  -> results (, projections {k: [R_k, n_components]})."""
    w = _weights(weights, ca_coords_dict)
    model = pca(ca_coords_dict[ref_key], n_components, sample_weights=w[ref_key] if weights else None)
    pc = {k: pca_project(v, model) for k, v in ca_coords_dict.items()}
    results = js_of_columns(pc, ref_key, n_bins, w)
    return (results, pc) if return_pc else results


def dynamics_frame(ca_coords_dict, ref_key="target"):
    """The common frame of ``rmsip``, ``dccm_mae`` and ``total_variance``: every ensemble (R >= 2), the reference included, is superposed
    once on the reference ensemble's mean structure (``ensemble_covariance``'s mean, rounded to float32) and its covariance is taken about
    its own mean under those transforms -> {k: device float64 [3L, 3L]}."""
    ref = _at_least_two("dynamics_frame", _dev(ca_coords_dict[ref_key]))
    target = ops.ca_aligned_mean(ref, ops.ca_fit_transforms(ref)).to(torch.float32)
    covs = {}
    for k, v in ca_coords_dict.items():
        x = _at_least_two("dynamics_frame", _dev(v))
        if x.shape[1] != ref.shape[1]:
            raise ValueError(f"dynamics_frame: {k!r} has {x.shape[1]} residues for the reference's {ref.shape[1]}")
        covs[k] = _aligned_moments(x, ops.ca_superpose(x, target)[1])[1]
    return covs


def rmsip_of(covs, n_structures, ref_key="target", n_components=10):
    """``rmsip`` of the covariances {k: [3L, 3L]} of ``dynamics_frame`` and the ensembles' sizes {k: R_k}."""
    n3 = covs[ref_key].shape[0]
    out = {}
    for k, c in covs.items():
        K = min(int(n_components), n3 - 6, n_structures[ref_key] - 1, n_structures[k] - 1)
        if K < 1:
            raise ValueError(f"rmsip: no component to compare for {k!r}: min(n_components, 3L - 6, R_ref - 1, R - 1) = {K}")
        if k == ref_key:
            out[k] = 1.0
            continue
        u, v = (_top_components(_host(m, np.float64), K)[1] for m in (covs[ref_key], c))
        out[k] = np.around(float(np.sqrt(np.square(u @ v.T).sum() / K)), decimals=4)
    return out


def rmsip(ca_coords_dict, ref_key="target", n_components=10):
    """Does each ensemble span the reference's essential subspace?  The root mean square inner product (Amadei et al. 1999) of the top K
    components u_i of the reference ensemble and v_j of each ensemble in ``dynamics_frame``'s common frame: sqrt((1 / K) sum_{i,j <= K}
    (u_i . v_j)^2), 1 for equal subspaces, K = min(n_components, 3L - 6, R_ref - 1, R_k - 1) (ValueError if K < 1).  The reference's is 1.0."""
    return rmsip_of(dynamics_frame(ca_coords_dict, ref_key), {k: len(_dev(v)) for k, v in ca_coords_dict.items()}, ref_key, n_components)


def dccm_mae_of(dccms, ref_key="target"):
    """``dccm_mae`` of cross-correlation maps {k: [L, L]} one already has."""
    return against_reference({k: m[np.triu_indices(len(m), k=1)] for k, m in dccms.items()}, ref_key)


def dccm_mae(ca_coords_dict, ref_key="target"):
    """Do the same residues move together?  The mean |c - c_ref| over the pairs i < j of each ensemble's cross-correlation map from the
    reference ensemble's, both in ``dynamics_frame``'s common frame (0.0 for a single residue)."""
    return dccm_mae_of({k: _dccm(c).cpu().numpy() for k, c in dynamics_frame(ca_coords_dict, ref_key).items()}, ref_key)


def total_variance_of(covs):
    """``total_variance`` of the covariances of ``dynamics_frame``."""
    return {k: np.around(float(c.diagonal().sum()), decimals=4) for k, c in covs.items()}


def total_variance(ca_coords_dict, ref_key="target"):
    """How much does each ensemble move?  tr C in A^2 (the sum over the residues of the squared RMSF) in ``dynamics_frame``'s common frame."""
    return total_variance_of(dynamics_frame(ca_coords_dict, ref_key))


# ---- clustering at a cutoff (csrc/ensemble_cluster.hip) ----------------------------------------------------------------------------
class ClusterResult(NamedTuple):
    """GROMOS clusters of R structures, most populated first: ``labels`` [R] (the cluster of every structure), ``centres`` [K] (the index
    of every cluster's centre), ``sizes`` [K] (non-increasing), numpy int32."""
    labels: np.ndarray
    centres: np.ndarray
    sizes: np.ndarray


def _cluster_chunks(n: int, rows: int, chunk, cutoff: float, at_least: bool) -> ClusterResult:
    """``chunk(r0, r1)`` -> rows r0 .. r1 - 1 of the n x n matrix (device float64), thresholded into the neighbour bits as they come:
    one chunk of the matrix is alive at a time."""
    adj = deg = None
    for r0 in range(0, n, rows):
        adj, deg = ops.cluster_adjacency(chunk(r0, min(r0 + rows, n)), cutoff, at_least, r0, adj, deg)
    return ClusterResult(*(t.cpu().numpy() for t in ops.cluster_gromos(adj, deg)))


def _cluster(score: PairScore, coords, cutoff: float, chunk_pairs=None, **kwargs) -> ClusterResult:
    """GROMOS clusters of an ensemble under ``score`` at an already checked ``cutoff``; a directed score counts as the worse of its two
    directions (rows r0 .. r1 of the matrix and of its transpose come from two launches)."""
    x = _dev(coords)
    n = x.shape[0]
    if score.symmetric:
        chunk = lambda r0, r1: score.matrix(x[r0:r1], x, **kwargs)   # noqa: E731
    else:
        worse = torch.minimum if score.higher_is_better else torch.maximum
        chunk = lambda r0, r1: worse(score.matrix(x[r0:r1], x, **kwargs), score.matrix(x, x[r0:r1], **kwargs).T)   # noqa: E731
    return _cluster_chunks(n, _chunk_rows(n, chunk_pairs), chunk, cutoff, score.higher_is_better)


def cluster_rmsd(coords, cutoff: float, weights=None, chunk_pairs=None) -> ClusterResult:
    """GROMOS clustering (Daura et al. 1999; ``gmx cluster -method gromos``) of an ensemble [R, L, 3] under the minimum RMSD of
    ``pairwise_rmsd``: i and j are neighbours iff rmsd(i, j) <= ``cutoff`` (A).  The structure with the most live neighbours (the lowest
    index among equals) is the next centre, it and its live neighbours form the cluster and leave, until none is left.  The float64 matrix
    is walked in row chunks of ``chunk_pairs`` pairs and never held (R x R / 8 bytes of bits are); the result does not depend on it."""
    cutoff = float(cutoff)
    if not 0.0 < cutoff < math.inf:
        raise ValueError(f"cluster_rmsd: cutoff must be a positive finite RMSD in Angstrom, got {cutoff}")
    return _cluster(RMSD, coords, cutoff, chunk_pairs, weights=weights)


def cluster_tm(coords, cutoff: float, d0=None) -> ClusterResult:
    """``cluster_rmsd`` under the TM-score of ``pairwise_tm``: i and j are neighbours iff tm(i, j) >= ``cutoff``, 0 < cutoff <= 1."""
    cutoff = float(cutoff)
    if not 0.0 < cutoff <= 1.0:
        raise ValueError(f"cluster_tm: cutoff must be a TM-score in (0, 1], got {cutoff}")
    return _cluster(TM, coords, cutoff, d0=d0)


def cluster_lddt(coords, cutoff: float) -> ClusterResult:
    """``cluster_rmsd`` under the symmetrised lDDT min(lddt(i -> j), lddt(j -> i)): i and j are neighbours iff each keeps the other's local
    distances to ``cutoff``, 0 < cutoff <= 1.  Rows r0 .. r1 of the matrix and of its transpose come from two launches; an entry is the
    same integer division wherever it is computed, so the relation is exactly symmetric."""
    cutoff = float(cutoff)
    if not 0.0 < cutoff <= 1.0:
        raise ValueError(f"cluster_lddt: cutoff must be an lDDT in (0, 1], got {cutoff}")
    return _cluster(LDDT, coords, cutoff)


def cluster_from_matrix(values, cutoff: float, at_least: bool = False) -> ClusterResult:
    """GROMOS clustering of a symmetric [R, R] matrix of one's own (device tensor or numpy array): neighbours are the pairs with
    ``values <= cutoff`` (distances), or ``values >= cutoff`` with ``at_least`` (similarities).  NaN is never a neighbour."""
    cutoff = float(cutoff)
    if math.isnan(cutoff):
        raise ValueError("cluster_from_matrix: cutoff is NaN")
    v = values if torch.is_tensor(values) else np.asarray(values, dtype=np.float64)
    if v.ndim != 2 or v.shape[0] != v.shape[1] or v.shape[0] < 1:
        raise ValueError(f"cluster_from_matrix: expected a square matrix, got {tuple(v.shape)}")
    same = (v == v.T) | ((v != v) & (v.T != v.T))           # (NaN in both places counts as equal)
    if not bool(same.all()):
        raise ValueError("cluster_from_matrix: the matrix is not symmetric")
    v = torch.as_tensor(v).to("cuda", torch.float64).contiguous()
    n = v.shape[0]
    return _cluster_chunks(n, n, lambda r0, r1: v[r0:r1], cutoff, bool(at_least))
