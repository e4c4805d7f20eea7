"""Ensemble metrics on the device: CA statistics, distance histograms, Kabsch RMSD, TM-score and superposition, lDDT, clustering,
backbone violations, secondary structure and torsions, contact maps and the fraction of native contacts, solvent accessibility, solution
scattering (Debye intensity, Kirkwood hydrodynamic radius), essential dynamics (mean structure, covariance and projections of the superposed
CA coordinates), time-lagged covariances of a feature trajectory (the heavy half of TICA) and projections of feature rows."""
import math
from typing import Optional

import numpy as np
import torch

from .binding import HipLibraryError, _check, _p, _req, _stream, load_library

RMSD_LAUNCH_PAIRS = 2 ** 31 - 1   # s2s_ca_rmsd_matrix and s2s_ca_tm_matrix take fewer than 2^31 pairs per call
TM_MAX_RES = 800                  # S2S_TM_MAX_RES: the chain length whose tiles fit the LDS of s2s_ca_tm_matrix
TM_MAX_COLS = 4 * 65535           # structures of b per s2s_ca_tm_matrix call
LDDT_MAX_RES = 1024               # S2S_LDDT_MAX_RES: the chain length whose tile of models fits the LDS of s2s_ca_lddt_matrix
LDDT_WORKSPACE_BYTES = 256 << 20  # budget of the pair lists of one s2s_ca_lddt_matrix launch: rows of a are chunked to stay under it
VIOL_MAX_RES = 1024               # S2S_VIOL_MAX_RES: the chain length whose atoms fit the LDS of s2s_backbone_violations as float64
VIOL_MAX_STRUCTURES = 1 << 20     # structures per s2s_backbone_violations launch, unless max_structures says less
SS_MAX_RES = 704                  # S2S_SS_MAX_RES: the chain length whose atoms and bond relation fit the LDS of s2s_secondary_structure
SS_MAX_STRUCTURES = 1 << 20       # structures per s2s_secondary_structure launch, unless max_structures says less
SASA_MAX_RES = 512                # S2S_SASA_MAX_RES: the chain length whose atoms, radii and areas fit the LDS of s2s_backbone_sasa as float64
SASA_MAX_POINTS = 1024            # S2S_SASA_MAX_POINTS: the sphere of s2s_backbone_sasa stays in LDS, a lane owns at most 16 of its points
SASA_MAX_STRUCTURES = 1 << 20     # structures per s2s_backbone_sasa launch, unless max_structures says less
SAXS_MAX_RES = 1024               # S2S_SAXS_MAX_RES: the chain length whose beads and types fit the LDS of s2s_ca_scattering as float64 planes
SAXS_MAX_Q = 1024                 # S2S_SAXS_MAX_Q: q-values per s2s_ca_scattering call, in tiles of 16
SAXS_MAX_TYPES = 64               # S2S_SAXS_MAX_TYPES: rows of the form-factor table, whose slice of a tile stays in LDS
SAXS_MAX_STRUCTURES = 1 << 20     # structures per s2s_ca_scattering launch, unless max_structures says less
CONTACT_MAX_RES = 1024            # S2S_CONTACT_MAX_RES: the chain length whose tile of structures fits the LDS of s2s_ca_native_q
CONTACT_LAUNCH_STRUCTURES = 65535  # S2S_CONTACT_MAX_STRUCTURES: structures per launch of the contact kernels
PCA_MAX_RES = 1024                # S2S_PCA_MAX_RES: the chain length whose centred coordinates fit the LDS of s2s_ca_project as float64
PCA_WORKSPACE_BYTES = 256 << 20   # budget of the centred coordinates of one chunk of s2s_ca_covariance, unless max_structures says less
TICA_MAX_FEATURES = 16384         # S2S_TICA_MAX_FEATURES: two D x D float64 matrices of 2 GiB each
TICA_WAVE_SLOTS = 1024            # S2S_TICA_WAVE_SLOTS: the waves of s2s_lagged_covariances' product kernel that run at once
TICA_MIN_GROUP_PAIRS = 512        # S2S_TICA_MIN_GROUP_PAIRS: the frame pairs from which a group of its k-split is worth a wave
CLUSTER_MAX_N = 65536             # S2S_CLUSTER_MAX_N: structures per clustering (512 MB of neighbour bits)
CLUSTER_ROUNDS_PER_SYNC = 32      # rounds of the greedy loop enqueued between two readbacks of its state


def ca_sample_stats(ca: torch.Tensor, clash_bar: float = 3.0, k_exclusion: int = 0):
    """CA [R, L, 3] fp32 device tensor -> (n_clash [R] int32, adjacent_max [R] fp32, radius_of_gyration [R] fp64)."""
    lib = load_library()
    _req(ca, name="ca")
    R, L = ca.shape[:2]
    nc = torch.empty(R, dtype=torch.int32, device=ca.device)
    am = torch.empty(R, dtype=torch.float32, device=ca.device)
    rg = torch.empty(R, dtype=torch.float64, device=ca.device)
    _check(lib.s2s_ca_sample_stats(_p(ca), R, L, float(clash_bar), int(k_exclusion), _p(nc), _p(am), _p(rg), _stream()), "s2s_ca_sample_stats")
    return nc, am, rg


def ca_pairwise_distances(ca: torch.Tensor, offset: int = 1) -> torch.Tensor:
    """Upper-triangular CA distances [R, D] float32 of every sample (np.triu_indices(L, k=offset) order) in numpy's float32 arithmetic."""
    lib = load_library()
    _req(ca, name="ca")
    R, L = ca.shape[0], ca.shape[1]
    if ca.ndim != 3 or ca.shape[2] != 3 or L <= offset:
        raise HipLibraryError(f"ca_pairwise_distances: coordinates {tuple(ca.shape)}, offset {offset}")
    D = (L - offset) * (L - offset + 1) // 2
    out = torch.empty(R, D, dtype=torch.float32, device=ca.device)
    for r0 in range(0, R, 65535):
        n = min(65535, R - r0)
        _check(lib.s2s_ca_pairwise_distances(_p(ca[r0:r0 + n]), n, L, int(offset), _p(out[r0:r0 + n]), _stream()), "s2s_ca_pairwise_distances")
    return out


def ca_pwd_js(ref_ca: torch.Tensor, pred_ca: torch.Tensor, offset: int = 3, n_bins: int = 50, pseudo: float = 1e-6,
              ref_weights: Optional[torch.Tensor] = None, pred_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per pair channel Jensen-Shannon distance between the distance histograms of two CA ensembles -> [D] fp64.
    ``ref_weights`` / ``pred_weights``: per-sample float64 histogram weights (device tensors), None = ones."""
    lib = load_library()
    _req(ref_ca, name="ref_ca"); _req(pred_ca, name="pred_ca")
    L = ref_ca.shape[1]
    if pred_ca.shape[1] != L:
        raise HipLibraryError("ca_pwd_js: the ensembles have different lengths")
    for nme, w, n in (("ref_weights", ref_weights, ref_ca.shape[0]), ("pred_weights", pred_weights, pred_ca.shape[0])):
        if w is not None:
            _req(w, torch.float64, nme)
            if w.numel() != n:
                raise HipLibraryError(f"ca_pwd_js: {nme} has {w.numel()} entries for {n} samples")
    out = torch.empty((L - offset) * (L - offset + 1) // 2, dtype=torch.float64, device=ref_ca.device)
    _check(lib.s2s_ca_pwd_js(_p(ref_ca), ref_ca.shape[0], _p(pred_ca), pred_ca.shape[0], L, int(offset), int(n_bins), float(pseudo),
                             _p(out), _p(ref_weights), _p(pred_weights), _stream()), "s2s_ca_pwd_js")
    return out


def _ensemble_pair(fn: str, a, b, on_device: bool = True):
    """The two ensembles of a pair matrix of ``fn``, a [Ra, L, 3] and b [Rb, L, 3] (None: ``a`` itself), checked -> (a, b, Ra, L, Rb).
    ``on_device=False`` leaves the device / dtype / contiguity check to the caller, who has something to check before it."""
    b = a if b is None else b
    if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)):
        raise HipLibraryError(f"{fn}: expected tensors, got {type(a).__name__} and {type(b).__name__}")
    if a.ndim != 3 or b.ndim != 3 or a.shape[2] != 3 or b.shape[1:] != a.shape[1:] or a.shape[0] < 1 or b.shape[0] < 1 or a.shape[1] < 1:
        raise HipLibraryError(f"{fn}: coordinates {tuple(a.shape)} and {tuple(b.shape)}")
    if on_device:
        _req(a, name="a"); _req(b, name="b")
    return a, b, a.shape[0], a.shape[1], b.shape[0]


def _mobile_target(fn: str, mobile, target, what: str = "mobile", on_device: bool = True):
    """``mobile`` [R, L, 3] (named ``what`` in the messages of ``fn``) onto ``target`` [L, 3], checked -> (R, L)."""
    if not (isinstance(mobile, torch.Tensor) and isinstance(target, torch.Tensor)):
        raise HipLibraryError(f"{fn}: expected tensors, got {type(mobile).__name__} and {type(target).__name__}")
    if mobile.ndim != 3 or mobile.shape[2] != 3 or target.shape != mobile.shape[1:] or mobile.shape[0] < 1 or mobile.shape[1] < 1:
        raise HipLibraryError(f"{fn}: {what} {tuple(mobile.shape)}, target {tuple(target.shape)}")
    if on_device:
        _req(mobile, name=what); _req(target, name="target")
    return mobile.shape[0], mobile.shape[1]


def _integer(fn: str, name: str, v, lo: int = 1, hi: Optional[int] = None) -> int:
    """The parameter ``name`` of ``fn`` as an int: an integer (not a bool) >= ``lo``, and <= ``hi`` where there is one."""
    if isinstance(v, bool) or int(v) != v or v < lo or (hi is not None and v > hi):
        raise HipLibraryError(f"{fn}: {name} must be an integer {f'>= {lo}' if hi is None else f'in {lo} .. {hi}'}, got {v}")
    return int(v)


def _positive(v, message: str) -> float:
    """``v`` as a float when it is positive and finite; otherwise the error ``message`` with the float in its ``{}``."""
    v = float(v)
    if not 0.0 < v < float("inf"):
        raise HipLibraryError(message.format(v))
    return v


def _structures(fn: str, x, what: str, tail: tuple, max_res: int):
    """One ensemble ``x`` [R, L, *tail] of ``fn`` (named ``what`` in its messages) of at most ``max_res`` residues, checked but for the
    device -> (R, L)."""
    if not isinstance(x, torch.Tensor):
        raise HipLibraryError(f"{fn}: expected tensors, got {type(x).__name__} for {what}")
    if x.ndim != 2 + len(tail) or x.shape[2:] != tail or x.shape[0] < 1 or x.shape[1] < 1:
        raise HipLibraryError(f"{fn}: {what} {tuple(x.shape)}, expected [R, L, {', '.join(map(str, tail))}]")
    if x.shape[1] > max_res:
        raise HipLibraryError(f"{fn}: at most {max_res} residues, got {x.shape[1]}")
    return x.shape[0], x.shape[1]


def _ca_ensemble(fn: str, ca, max_res: int):
    """``ca`` [R, L, 3], the CA coordinates of one ensemble -> (R, L)."""
    return _structures(fn, ca, "coordinates ca", (3,), max_res)


def _launch_structures(fn: str, max_structures, launch_structures: int) -> int:
    """``max_structures`` (None or an integer >= 1) of ``fn`` -> the structures per launch."""
    return launch_structures if max_structures is None else min(_integer(fn, "max_structures", max_structures), launch_structures)


def _backbone_ensemble(fn: str, atoms, max_res: int, max_structures, launch_structures: int) -> int:
    """``atoms`` [R, L, 5, 3] of at most ``max_res`` residues and ``max_structures`` of ``fn``, checked but for the device -> the
    structures per launch."""
    _structures(fn, atoms, "atoms", (5, 3), max_res)
    return _launch_structures(fn, max_structures, launch_structures)


def _pair_out(fn: str, out, n_a: int, n_b: int, device) -> torch.Tensor:
    """The [n_a, n_b] float64 result of a pair matrix of ``fn``: the caller's ``out``, checked, or a new tensor."""
    if out is None:
        return torch.empty(n_a, n_b, dtype=torch.float64, device=device)
    if _req(out, torch.float64, "out").shape != (n_a, n_b):
        raise HipLibraryError(f"{fn}: out {tuple(out.shape)} for {n_a} x {n_b} pairs")
    return out


def _row_chunks(n: int, rows: int, *tensors):
    """Chunks of at most ``rows`` of the ``n`` leading rows of every tensor -> (rows of the chunk, a pointer to the chunk of each)."""
    for r0 in range(0, n, rows):
        m = min(rows, n - r0)
        yield (m, *(_p(t[r0:r0 + m]) for t in tensors))


def _rmsd_weights(weights, L: int, device):
    if weights is None:
        return None
    w = torch.as_tensor(weights).to(device, torch.float32).contiguous()
    if w.shape != (L,):
        raise HipLibraryError(f"weights: expected [{L}] (one per residue), got {tuple(w.shape)}")
    return w


def rmsd_row_chunk(n_b: int, max_pairs: Optional[int] = None) -> int:
    """Rows of A per s2s_ca_rmsd_matrix call so that one call stays within ``max_pairs`` pairs (at least one row)."""
    cap = RMSD_LAUNCH_PAIRS if max_pairs is None else min(int(max_pairs), RMSD_LAUNCH_PAIRS)
    return max(1, min(cap // n_b, 16 * 65535))


def ca_rmsd_matrix(a: torch.Tensor, b: Optional[torch.Tensor] = None, weights=None, max_pairs: Optional[int] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Minimum RMSD (optimal proper rotation + translation, float64) of every pair of a [Ra, L, 3] and b [Rb, L, 3] fp32 device tensors
    -> [Ra, Rb] fp64.  ``b=None``: the self matrix of ``a`` (exactly symmetric).  ``weights``: per-residue [L], >= 0.  ``max_pairs``
    bounds the pairs (and with them the scratch) of one launch: rows are chunked, the result is bit for bit the same for any value.
    The caller bounds Ra x Rb (the output); metrics.coverage_rmsd shows the chunked use that never holds the whole matrix."""
    a, b, n_a, L, n_b = _ensemble_pair("ca_rmsd_matrix", a, b)
    w = _rmsd_weights(weights, L, a.device)
    out = _pair_out("ca_rmsd_matrix", out, n_a, n_b, a.device)
    rows = rmsd_row_chunk(n_b, max_pairs)
    lib = load_library()
    region = lambda n: -(-n // 16) * 16 * (3 * (-(-L // 4) * 4) + 1)  # noqa: E731
    ws = torch.empty(2 + region(n_b) + region(min(rows, n_a)), dtype=torch.float64, device=a.device)
    for n, pa, po in _row_chunks(n_a, rows, a, out):
        _check(lib.s2s_ca_rmsd_matrix(pa, n, _p(b), n_b, L, _p(w), po, _p(ws), ws.numel(), _stream()), "s2s_ca_rmsd_matrix")
    return out


def ca_superpose(mobile: torch.Tensor, target: torch.Tensor, weights=None):
    """mobile [R, L, 3] onto target [L, 3] (fp32 device tensors) -> (rmsd [R] fp64, xform [R, 12] fp64: row-major proper rotation, then
    translation; rotation @ x + translation maps mobile onto target)."""
    R, L = _mobile_target("ca_superpose", mobile, target)
    w = _rmsd_weights(weights, L, mobile.device)
    lib = load_library()
    rmsd = torch.empty(R, dtype=torch.float64, device=mobile.device)
    xform = torch.empty(R, 12, dtype=torch.float64, device=mobile.device)
    _check(lib.s2s_ca_superpose(_p(mobile), R, _p(target), L, _p(w), _p(rmsd), _p(xform), _stream()), "s2s_ca_superpose")
    return rmsd, xform


def apply_xform(points: torch.Tensor, xform: torch.Tensor) -> torch.Tensor:
    """points [R, M, 3] fp32, xform [R, 12] fp64 (ca_superpose) -> rotation @ point + translation, float64 arithmetic, fp32 result."""
    lib = load_library()
    _req(points, name="points"); _req(xform, torch.float64, "xform")
    if points.ndim != 3 or points.shape[2] != 3 or xform.shape != (points.shape[0], 12) or points.shape[0] < 1 or points.shape[1] < 1:
        raise HipLibraryError(f"apply_xform: points {tuple(points.shape)}, xform {tuple(xform.shape)}")
    out = torch.empty_like(points)
    _check(lib.s2s_apply_xform(_p(points), _p(xform), points.shape[0], points.shape[1], _p(out), _stream()), "s2s_apply_xform")
    return out


def _pca_inputs(fn: str, ca, xform, sample_weights):
    """``ca`` [R, L, 3] with the optional ``xform`` [R, 12] and ``sample_weights`` [R] (a tensor on any device, array or list; >= 0 with a
    positive finite sum) of ``fn``, checked but for the device -> (R, L, the weights as a host float64 tensor normalised to sum 1, or None)."""
    R, L = _ca_ensemble(fn, ca, PCA_MAX_RES)
    if xform is not None and (not isinstance(xform, torch.Tensor) or xform.shape != (R, 12)):
        raise HipLibraryError(f"{fn}: xform {tuple(getattr(xform, 'shape', ()))} for {R} structures, expected [{R}, 12]")
    if sample_weights is None:
        return R, L, None
    p = torch.as_tensor(sample_weights).detach().to("cpu", torch.float64).contiguous()
    if p.shape != (R,):
        raise HipLibraryError(f"{fn}: sample_weights {tuple(p.shape)} for {R} structures")
    total = float(p.sum())
    if not (bool((p >= 0.0).all()) and 0.0 < total < float("inf")):
        raise HipLibraryError(f"{fn}: sample_weights must be >= 0 with a positive finite sum")
    return R, L, p / total


def _pca_on_device(ca, xform, p):
    _req(ca, name="ca")
    if xform is not None:
        _req(xform, torch.float64, "xform")
    return None if p is None else p.to(ca.device)


def _mean_of(fn: str, mean, shape: tuple, of: str = ""):
    """The ``mean`` argument of ``fn`` is a tensor of ``shape`` (checked but for the device); ``of``: what the message says the shape is for."""
    if not isinstance(mean, torch.Tensor) or mean.shape != shape:
        raise HipLibraryError(f"{fn}: mean {tuple(getattr(mean, 'shape', ()))}{of}, expected {list(shape)}")


def _projection(x, x_name: str, mean, components):
    """What ``ca_project`` and ``feature_project`` share once their shapes are checked: the rows ``x`` fp32, ``mean`` and ``components``
    [K, width] fp64, all on the device -> (K, proj [rows, K] fp64 on that device, uninitialised)."""
    _req(x, name=x_name); _req(mean, torch.float64, "mean"); _req(components, torch.float64, "components")
    K = components.shape[0]
    return K, torch.empty(x.shape[0], K, dtype=torch.float64, device=x.device)


def ca_aligned_mean(ca: torch.Tensor, xform: Optional[torch.Tensor] = None, sample_weights=None) -> torch.Tensor:
    """The mean structure of ca [R, L, 3] (fp32 device tensor) after the transforms ``xform`` [R, 12] fp64 (``ca_superpose``'s; None: the
    identity) -> [L, 3] fp64: sum_s p_s (R_s x_s + t_s) in float64, p = ``sample_weights`` [R] normalised to sum 1 (None: 1 / R).  The order
    of the sum depends on R alone."""
    R, L, p = _pca_inputs("ca_aligned_mean", ca, xform, sample_weights)
    p = _pca_on_device(ca, xform, p)
    mean = torch.empty(L, 3, dtype=torch.float64, device=ca.device)
    _check(load_library().s2s_ca_aligned_mean(_p(ca), R, L, _p(xform), _p(p), _p(mean), _stream()), "s2s_ca_aligned_mean")
    return mean


def ca_covariance(ca: torch.Tensor, mean: torch.Tensor, xform: Optional[torch.Tensor] = None, sample_weights=None,
                  max_structures: Optional[int] = None) -> torch.Tensor:
    """The covariance of the transformed coordinates of ca [R, L, 3] about ``mean`` [L, 3] fp64 -> [3L, 3L] fp64, coordinate 3 i + a:
    sum_s p_s (y_s - mean)(y_s - mean)^T (population form), exactly symmetric.  ``max_structures`` bounds the structures (rounded up to a
    multiple of 4) whose centred coordinates the workspace holds at a time; the result is bit for bit the same for any value."""
    fn = "ca_covariance"
    R, L, p = _pca_inputs(fn, ca, xform, sample_weights)
    chunk = -(-_launch_structures(fn, max_structures, max(4, PCA_WORKSPACE_BYTES // (8 * 48 * -(-3 * L // 48)))) // 4) * 4
    _mean_of(fn, mean, (L, 3), f" for {L} residues")
    p = _pca_on_device(ca, xform, p)
    _req(mean, torch.float64, "mean")
    cov = torch.empty(3 * L, 3 * L, dtype=torch.float64, device=ca.device)
    ws = torch.empty(-(-3 * L // 48) * 48 * min(chunk, -(-R // 4) * 4), dtype=torch.float64, device=ca.device)   # S2S_PCA_WORKSPACE_DOUBLES
    _check(load_library().s2s_ca_covariance(_p(ca), R, L, _p(xform), _p(p), _p(mean), _p(cov), _p(ws), ws.numel(), _stream()), "s2s_ca_covariance")
    return cov


def ca_project(ca: torch.Tensor, mean: torch.Tensor, components: torch.Tensor, xform: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ca [R, L, 3] after ``xform`` onto ``components`` [K, 3L] fp64 about ``mean`` [L, 3] fp64 -> [R, K] fp64: sum_c (y_sc - mean_c) v_kc.
    The order of a sum depends on L alone."""
    fn = "ca_project"
    R, L, _ = _pca_inputs(fn, ca, xform, None)
    if not (isinstance(mean, torch.Tensor) and isinstance(components, torch.Tensor)) or mean.shape != (L, 3) or components.ndim != 2 \
            or components.shape[0] < 1 or components.shape[1] != 3 * L:
        raise HipLibraryError(f"{fn}: mean {tuple(getattr(mean, 'shape', ()))} and components {tuple(getattr(components, 'shape', ()))}, "
                              f"expected [{L}, 3] and [K, {3 * L}]")
    _pca_on_device(ca, xform, None)
    K, proj = _projection(ca, "ca", mean, components)
    _check(load_library().s2s_ca_project(_p(ca), R, L, _p(xform), _p(mean), _p(components), K, _p(proj), _stream()), "s2s_ca_project")
    return proj


def ca_fit_transforms(ca: torch.Tensor, target: Optional[torch.Tensor] = None, sample_weights=None, residue_weights=None,
                      n_fit_rounds: int = 5, fit: bool = True) -> Optional[torch.Tensor]:
    """The transforms of an essential-dynamics fit of ca [R, L, 3] -> xform [R, 12] fp64 (None with ``fit=False``: the identity).
    ``ca_superpose`` onto ``target`` [L, 3] fp32 (None: ``ca[0]``), ``n_fit_rounds`` times; after each round but the last the target becomes
    the ``sample_weights``-weighted mean of the transformed structures, formed in float64 and rounded to float32 (the superposition takes a
    float32 target).  A fixed count: no data-dependent stop.  ``residue_weights`` [L] go to the superposition only."""
    fn = "ca_fit_transforms"
    _pca_inputs(fn, ca, None, sample_weights)
    if not fit:
        return None
    rounds = _integer(fn, "n_fit_rounds", n_fit_rounds)
    if target is not None:
        _mobile_target(fn, ca, target, "coordinates ca", on_device=False)
    _req(ca, name="ca")
    target = ca[0] if target is None else _req(target, name="target")
    for k in range(rounds):
        xform = ca_superpose(ca, target, residue_weights)[1]
        if k + 1 < rounds:
            target = ca_aligned_mean(ca, xform, sample_weights).to(torch.float32)
    return xform


def tica_groups(n_pairs: int, D: int):
    """S2S_TICA_GROUPS / S2S_TICA_GROUP_PAIRS of include/str2str_hip.h: how s2s_lagged_covariances divides ``n_pairs`` frame pairs of ``D``
    features -> (the number of groups G, the pairs of a group: a multiple of 4).  A function of (n_pairs, D) alone."""
    blocks = -(-D // 48)
    n4 = -(-n_pairs // 4) * 4
    wanted = max(1, min(TICA_WAVE_SLOTS // (blocks * (blocks + 1) // 2), -(-n4 // TICA_MIN_GROUP_PAIRS)))
    group = -(-(n4 // 4) // wanted) * 4
    return -(-n4 // group), group


def _features(fn: str, f, lag=None):
    """``f`` [T, D], the feature rows of ``fn`` in time order, and its ``lag`` (None: ``fn`` has none), checked but for the device
    -> (T, D, lag)."""
    if not isinstance(f, torch.Tensor):
        raise HipLibraryError(f"{fn}: expected tensors, got {type(f).__name__} for features")
    if f.ndim != 2 or f.shape[0] < 1 or f.shape[1] < 1:
        raise HipLibraryError(f"{fn}: features {tuple(f.shape)}, expected [T, D]")
    T, D = f.shape
    if D > TICA_MAX_FEATURES or T > 2 ** 31 - 1:
        raise HipLibraryError(f"{fn}: at most {TICA_MAX_FEATURES} features and {2 ** 31 - 1} frames, got {D} and {T}")
    if lag is not None:
        lag = _integer(fn, "lag", lag)
        if T <= lag:
            raise HipLibraryError(f"{fn}: {T} frames are not enough for lagtime {lag}")
    return T, D, lag


def lagged_mean(features: torch.Tensor, lag: int) -> torch.Tensor:
    """The reversible mean of the feature trajectory features [T, D] (fp32 device tensor, a row per frame in time order) over its
    n = T - ``lag`` frame pairs (t, t + lag) -> [D] fp64: (1 / 2n) sum_t (f_t + f_{t+lag}) in float64.  The order of the sum depends on
    (T, lag) alone."""
    T, D, lag = _features("lagged_mean", features, lag)
    _req(features, name="features")
    mean = torch.empty(D, dtype=torch.float64, device=features.device)
    _check(load_library().s2s_lagged_mean(_p(features), T, D, lag, _p(mean), _stream()), "s2s_lagged_mean")
    return mean


def lagged_covariances(features: torch.Tensor, mean: torch.Tensor, lag: int, max_pairs: Optional[int] = None):
    """The instantaneous and the time-lagged covariance of features [T, D] about ``mean`` [D] fp64 over the n = T - ``lag`` frame pairs
    -> (c00, c0t), each [D, D] fp64: with a = f_t - mean and b = f_{t+lag} - mean, sum_t (a a^T + b b^T) / 2n and sum_t (a b^T + b a^T) / 2n
    (the reversible estimate, population form), both exactly symmetric.  ``max_pairs`` bounds the frame pairs (each group of
    ``tica_groups`` takes a multiple of 4, at least 4) whose centred features the workspace holds at a time; the default is what
    PCA_WORKSPACE_BYTES holds.  The result is bit for bit the same for any value."""
    fn = "lagged_covariances"
    T, D, lag = _features(fn, features, lag)
    _mean_of(fn, mean, (D,))
    blocks = -(-D // 48)
    G, group = tica_groups(T - lag, D)
    pairs = PCA_WORKSPACE_BYTES // (8 * 2 * 48 * blocks) if max_pairs is None else _integer(fn, "max_pairs", max_pairs)
    step = min(group, max(4, -(-(pairs // G) // 4) * 4))
    _req(features, name="features"); _req(mean, torch.float64, "mean")
    c00, c0t = (torch.empty(D, D, dtype=torch.float64, device=features.device) for _ in range(2))
    partials = G * 2 * (blocks * (blocks + 1) // 2) * 2304 if G > 1 else 0
    ws = torch.empty(2 * blocks * 48 * G * step + partials, dtype=torch.float64, device=features.device)   # S2S_TICA_WORKSPACE_DOUBLES
    _check(load_library().s2s_lagged_covariances(_p(features), T, D, lag, _p(mean), _p(c00), _p(c0t), _p(ws), ws.numel(), _stream()),
           "s2s_lagged_covariances")
    return c00, c0t


def feature_project(features: torch.Tensor, mean: torch.Tensor, components: torch.Tensor) -> torch.Tensor:
    """features [T, D] (fp32 device tensor) onto ``components`` [K, D] fp64 about ``mean`` [D] fp64 -> [T, K] fp64:
    sum_c (f_sc - mean_c) v_kc.  The order of a sum depends on D alone."""
    fn = "feature_project"
    T, D, _ = _features(fn, features)
    _mean_of(fn, mean, (D,))
    if not isinstance(components, torch.Tensor) or components.ndim != 2 or components.shape[0] < 1 or components.shape[1] != D:
        raise HipLibraryError(f"{fn}: components {tuple(getattr(components, 'shape', ()))}, expected [K, {D}]")
    K, proj = _projection(features, "features", mean, components)
    _check(load_library().s2s_feature_project(_p(features), T, D, _p(mean), _p(components), K, _p(proj), _stream()), "s2s_feature_project")
    return proj


def _tm_d0(d0) -> float:
    """The C ABI's encoding: 0 selects the length formula.  An explicit d0 must be a positive finite number."""
    if d0 is None:
        return 0.0
    return _positive(d0, "d0: expected a positive finite length in Angstrom (None = the formula of the chain length), got {}")


def ca_tm_matrix(a: torch.Tensor, b: Optional[torch.Tensor] = None, d0: Optional[float] = None, max_pairs: Optional[int] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """TM-score (residue i against residue i, normalised by the common length L, float64) of every pair of a [Ra, L, 3] and
    b [Rb, L, 3] fp32 device tensors -> [Ra, Rb] fp64 in (0, 1].  ``b=None``: the self matrix of ``a`` (exactly symmetric).  ``d0``: the
    distance scale in Angstrom, None = max(0.5, 1.24 cbrt(L - 15) - 1.8).  The superposition search is the fixed monotone reweighted
    Kabsch iteration of include/str2str_hip.h: a certified lower bound of the optimum, a heuristic like the TMscore program's.
    ``max_pairs`` bounds the pairs of one launch: rows are chunked, the result is bit for bit the same for any value."""
    a, b, n_a, L, n_b = _ensemble_pair("ca_tm_matrix", a, b)
    if L > TM_MAX_RES or n_b > TM_MAX_COLS:
        raise HipLibraryError(f"ca_tm_matrix: at most {TM_MAX_RES} residues and {TM_MAX_COLS} structures of b, got {L} and {n_b}")
    d0 = _tm_d0(d0)
    out = _pair_out("ca_tm_matrix", out, n_a, n_b, a.device)
    lib = load_library()
    for n, pa, po in _row_chunks(n_a, rmsd_row_chunk(n_b, max_pairs), a, out):
        _check(lib.s2s_ca_tm_matrix(pa, n, _p(b), n_b, L, d0, po, _stream()), "s2s_ca_tm_matrix")
    return out


def ca_tm_superpose(mobile: torch.Tensor, target: torch.Tensor, d0: Optional[float] = None):
    """mobile [R, L, 3] onto target [L, 3] (fp32 device tensors) -> (tm [R] fp64: the ca_tm_matrix entries of the pairs, xform [R, 12]
    fp64 in ca_superpose's layout: the superposition that scored each TM; apply_xform consumes it)."""
    R, L = _mobile_target("ca_tm_superpose", mobile, target)
    if L > TM_MAX_RES:
        raise HipLibraryError(f"ca_tm_superpose: at most {TM_MAX_RES} residues, got {L}")
    d0 = _tm_d0(d0)
    lib = load_library()
    tm = torch.empty(R, dtype=torch.float64, device=mobile.device)
    xform = torch.empty(R, 12, dtype=torch.float64, device=mobile.device)
    _check(lib.s2s_ca_tm_superpose(_p(mobile), R, _p(target), L, d0, _p(tm), _p(xform), _stream()), "s2s_ca_tm_superpose")
    return tm, xform


def lddt_workspace_bytes(n_a: int, n_res: int) -> int:
    """S2S_LDDT_WORKSPACE_BYTES: the scratch of one s2s_ca_lddt_matrix call with ``n_a`` reference structures of ``n_res`` residues."""
    slots = (n_res * (n_res - 1) // 2 + 1) // 2 * 2
    return n_a * (12 * slots + 8 + 4 * n_res)


def _lddt_args(what: str, L: int, cutoff, min_seq_sep):
    cutoff = _positive(cutoff, what + ": cutoff must be a positive finite distance in Angstrom, got {}")
    min_seq_sep = _integer(what, "min_seq_sep", min_seq_sep)
    if L > LDDT_MAX_RES:
        raise HipLibraryError(f"{what}: at most {LDDT_MAX_RES} residues, got {L}")
    return cutoff, min_seq_sep


def ca_lddt_matrix(a: torch.Tensor, b: Optional[torch.Tensor] = None, cutoff: float = 15.0, min_seq_sep: int = 1,
                   max_pairs: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """CA-lDDT (include/str2str_hip.h: no superposition, residue i against residue i, float64) of every structure of b [Rb, L, 3] scored
    in the environment of every structure of a [Ra, L, 3], fp32 device tensors -> [Ra, Rb] fp64 in [0, 1].  NOT symmetric: ``a[i]`` is the
    reference, its pairs closer than ``cutoff`` and at least ``min_seq_sep`` apart in sequence are the ones scored.  ``b=None``: ``a``
    against itself (the diagonal is exactly 1).  Rows of ``a`` are chunked so that the pair lists of one launch stay within
    LDDT_WORKSPACE_BYTES and the pairs within ``max_pairs``; every entry is one division of two integers, bit for bit the same for any
    chunking."""
    a, b, n_a, L, n_b = _ensemble_pair("ca_lddt_matrix", a, b, on_device=False)
    cutoff, min_seq_sep = _lddt_args("ca_lddt_matrix", L, cutoff, min_seq_sep)
    _req(a, name="a"); _req(b, name="b")
    out = _pair_out("ca_lddt_matrix", out, n_a, n_b, a.device)
    rows = min(rmsd_row_chunk(n_b, max_pairs), max(1, LDDT_WORKSPACE_BYTES // lddt_workspace_bytes(1, L)), n_a)
    lib = load_library()
    ws = torch.empty(lddt_workspace_bytes(rows, L) // 8 + 1, dtype=torch.int64, device=a.device)
    for n, pa, po in _row_chunks(n_a, rows, a, out):
        _check(lib.s2s_ca_lddt_matrix(pa, n, _p(b), n_b, L, cutoff, min_seq_sep, po, _p(ws), ws.numel() * 8, _stream()), "s2s_ca_lddt_matrix")
    return out


def ca_lddt_per_residue(model: torch.Tensor, target: torch.Tensor, cutoff: float = 15.0, min_seq_sep: int = 1):
    """model [R, L, 3] scored in the environment of the reference target [L, 3] (fp32 device tensors) -> (per_res [R, L] fp64: the lDDT of
    every residue, 1.0 where the target gives it no partner; total [R] fp64: bit for bit ``ca_lddt_matrix(target[None], model)[0]``)."""
    R, L = _mobile_target("ca_lddt_per_residue", model, target, "model", on_device=False)
    cutoff, min_seq_sep = _lddt_args("ca_lddt_per_residue", L, cutoff, min_seq_sep)
    _req(model, name="model"); _req(target, name="target")
    lib = load_library()
    per_res = torch.empty(R, L, dtype=torch.float64, device=model.device)
    total = torch.empty(R, dtype=torch.float64, device=model.device)
    ws = torch.empty(lddt_workspace_bytes(1, L) // 8 + 1, dtype=torch.int64, device=model.device)
    _check(lib.s2s_ca_lddt_per_residue(_p(model), R, _p(target), L, cutoff, min_seq_sep, _p(per_res), _p(total), _p(ws), ws.numel() * 8,
                                       _stream()), "s2s_ca_lddt_per_residue")
    return per_res, total


def _contact_args(what: str, min_seq_sep=None, **positive):
    """The parameters of a contact function ``what``, checked -> the ``positive`` ones as floats, in order, then ``min_seq_sep`` (unless
    None) as an int."""
    out = [_positive(v, f"{what}: {name} must be positive and finite, got {{}}") for name, v in positive.items()]
    return out if min_seq_sep is None else out + [_integer(what, "min_seq_sep", min_seq_sep)]


def ca_contact_map(ca: torch.Tensor, cutoff: float = 8.0, min_seq_sep: int = 3, weights: Optional[torch.Tensor] = None):
    """The contact map of the ensemble ca [R, L, 3] (fp32 device tensor; include/str2str_hip.h: residues at least ``min_seq_sep`` apart in
    sequence whose squared CA distance, in float64, is below ``cutoff``^2) -> (counts [L, L] int32: the structures in which each pair is a
    contact, symmetric, zero inside the band; weighted [L, L] fp64, or None without ``weights``: the sum of ``weights`` [R] (fp64 device
    tensor) over those structures, in ascending structure order).  The contact probability is ``counts / R`` or ``weighted /
    weights.sum()``.  R is walked in launches of CONTACT_LAUNCH_STRUCTURES; both results are bit for bit the same for any such size."""
    R, L = _ca_ensemble("ca_contact_map", ca, CONTACT_MAX_RES)
    cutoff, min_seq_sep = _contact_args("ca_contact_map", min_seq_sep, cutoff=cutoff)
    if weights is not None and (not isinstance(weights, torch.Tensor) or weights.shape != (R,)):
        raise HipLibraryError(f"ca_contact_map: weights {tuple(getattr(weights, 'shape', ()))} for {R} structures")
    _req(ca, name="ca")
    if weights is not None:
        _req(weights, torch.float64, "weights")
    counts = torch.zeros(L, L, dtype=torch.int32, device=ca.device)
    weighted = None if weights is None else torch.zeros(L, L, dtype=torch.float64, device=ca.device)
    lib = load_library()
    for n, p_ca, *p_w in _row_chunks(R, CONTACT_LAUNCH_STRUCTURES, ca, *(() if weights is None else (weights,))):
        _check(lib.s2s_ca_contact_map(p_ca, n, L, cutoff, min_seq_sep, p_w[0] if p_w else None, _p(counts), _p(weighted), _stream()),
               "s2s_ca_contact_map")
    return counts, weighted


def ca_contact_stats(ca: torch.Tensor, cutoff: float = 8.0, min_seq_sep: int = 3):
    """Per structure of ca [R, L, 3] (fp32 device tensor) -> (n_contacts [R] int32; sep_sum [R] int64: the sum of j - i over its contacts).
    The relative contact order is ``sep_sum / (L * n_contacts)``, 0.0 for a structure without contacts."""
    R, L = _ca_ensemble("ca_contact_stats", ca, CONTACT_MAX_RES)
    cutoff, min_seq_sep = _contact_args("ca_contact_stats", min_seq_sep, cutoff=cutoff)
    _req(ca, name="ca")
    n_contacts = torch.empty(R, dtype=torch.int32, device=ca.device)
    sep_sum = torch.empty(R, dtype=torch.int64, device=ca.device)
    lib = load_library()
    for n, p_ca, *p_out in _row_chunks(R, CONTACT_LAUNCH_STRUCTURES, ca, n_contacts, sep_sum):
        _check(lib.s2s_ca_contact_stats(p_ca, n, L, cutoff, min_seq_sep, *p_out, _stream()), "s2s_ca_contact_stats")
    return n_contacts, sep_sum


def ca_native_contacts(native: torch.Tensor, cutoff: float = 8.0, min_seq_sep: int = 4):
    """The native contact list of native [L, 3] (fp32 device tensor) -> (pairs [n, 2] int32: (i, j) with j - i >= ``min_seq_sep`` closer
    than ``cutoff``, in ascending (i, j) order; d0 [n] fp64: their distances).  Reads the length of the list back from the device."""
    if not isinstance(native, torch.Tensor):
        raise HipLibraryError(f"ca_native_contacts: expected a tensor, got {type(native).__name__}")
    if native.ndim != 2 or native.shape[1] != 3 or native.shape[0] < 1:
        raise HipLibraryError(f"ca_native_contacts: native {tuple(native.shape)}, expected [L, 3]")
    L = native.shape[0]
    cutoff, min_seq_sep = _contact_args("ca_native_contacts", min_seq_sep, cutoff=cutoff)
    if L > CONTACT_MAX_RES:
        raise HipLibraryError(f"ca_native_contacts: at most {CONTACT_MAX_RES} residues, got {L}")
    _req(native, name="native")
    slots = max(1, L * (L - 1) // 2)                           # S2S_CONTACT_LIST_SLOTS
    pairs = torch.empty(slots, 2, dtype=torch.int32, device=native.device)
    d0 = torch.empty(slots, dtype=torch.float64, device=native.device)
    n = torch.zeros(1, dtype=torch.int32, device=native.device)
    _check(load_library().s2s_ca_native_contacts(_p(native), L, cutoff, min_seq_sep, _p(pairs), _p(d0), _p(n), _stream()), "s2s_ca_native_contacts")
    n = int(n.item())
    return pairs[:n].clone(), d0[:n].clone()


def ca_native_q(ca: torch.Tensor, pairs: torch.Tensor, d0: torch.Tensor, beta: float = 5.0, lam: float = 1.2):
    """The fraction of native contacts of every structure of ca [R, L, 3] (fp32 device tensor) against the list (pairs [n, 2] int32, d0 [n]
    fp64) of ``ca_native_contacts`` -> (q_soft [R] fp64: the mean of 1 / (1 + exp(beta (d - lam d0))), Best, Hummer and Eaton 2013; q_hard
    [R] fp64: hits / n; hits [R] int32: the entries with d < lam d0).  An empty list gives 1.0.  A structure's values are bit for bit the
    same in any launch."""
    R, L = _ca_ensemble("ca_native_q", ca, CONTACT_MAX_RES)
    beta, lam = _contact_args("ca_native_q", beta=beta, lam=lam)
    if not (isinstance(pairs, torch.Tensor) and isinstance(d0, torch.Tensor)) or pairs.ndim != 2 or pairs.shape[1] != 2 or d0.shape != pairs.shape[:1]:
        raise HipLibraryError(f"ca_native_q: pairs {tuple(getattr(pairs, 'shape', ()))} and d0 {tuple(getattr(d0, 'shape', ()))}, expected [n, 2] and [n]")
    n_pairs = pairs.shape[0]
    if n_pairs > max(1, L * (L - 1) // 2):
        raise HipLibraryError(f"ca_native_q: {n_pairs} entries for a chain of {L} residues")
    _req(ca, name="ca"); _req(pairs, torch.int32, "pairs"); _req(d0, torch.float64, "d0")
    q_soft, q_hard = (torch.empty(R, dtype=torch.float64, device=ca.device) for _ in range(2))
    hits = torch.empty(R, dtype=torch.int32, device=ca.device)
    lib = load_library()
    for n, p_ca, *p_out in _row_chunks(R, CONTACT_LAUNCH_STRUCTURES, ca, q_soft, q_hard, hits):
        _check(lib.s2s_ca_native_q(p_ca, n, L, _p(pairs) if n_pairs else None, _p(d0) if n_pairs else None, n_pairs, beta, lam, *p_out, _stream()),
               "s2s_ca_native_q")
    return q_soft, q_hard, hits


def _sequence_input(what: str, v, shape, dtype, fn: str = "backbone_violations") -> torch.Tensor:
    """A per-sequence input of ``fn`` (a few KB; tensor, array or list), checked, as a contiguous tensor of the C ABI's type."""
    t = torch.as_tensor(v)
    if t.shape != shape or t.is_floating_point() or t.is_complex():
        raise HipLibraryError(f"{fn}: {what}: expected integers of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    if dtype == torch.uint8:
        return (t != 0).to(torch.uint8).contiguous()
    if t.numel() and (int(t.min()) < -2 ** 31 or int(t.max()) > 2 ** 31 - 1):
        raise HipLibraryError(f"{fn}: {what} does not fit 32 bits")
    return t.to(dtype).contiguous()


def backbone_violations(atoms: torch.Tensor, atom_exists, aatype, residue_index, tolerance_factor: float = 12.0, clash_tolerance: float = 1.5,
                        max_structures: Optional[int] = None):
    """The structural violations of include/str2str_hip.h (the reference's between-residue bond, angle and clash terms and its extreme
    CA-CA steps) of every structure of atoms [R, L, 5, 3] fp32 device tensor, atom14 slots N, CA, C, O, CB.  ``atom_exists`` [L, 5]
    (non-zero: the atom exists), ``aatype`` [L] (the reference's residue order) and ``residue_index`` [L] belong to the one sequence of the
    ensemble.  -> device tensors (losses [R, 4] fp64: C-N, CA-C-N, C-N-CA, clash means; fractions [R, 4] fp64: residues with a violated
    connection, with a clashing atom, with either, extreme CA-CA steps; per_residue_loss [R, L] fp64; bond_mask [R, L] uint8;
    clash_atom_mask [R, L, 5] uint8; n_clash_pairs [R] int32).  ``max_structures`` bounds the structures of one launch; a structure's
    results are bit for bit the same for any value."""
    rows = _backbone_ensemble("backbone_violations", atoms, VIOL_MAX_RES, max_structures, VIOL_MAX_STRUCTURES)
    R, L = atoms.shape[:2]
    tolerance_factor, clash_tolerance = float(tolerance_factor), float(clash_tolerance)
    if not (abs(tolerance_factor) < float("inf") and abs(clash_tolerance) < float("inf")):
        raise HipLibraryError(f"backbone_violations: tolerances must be finite, got {tolerance_factor} and {clash_tolerance}")
    exists = _sequence_input("atom_exists", atom_exists, (L, 5), torch.uint8)
    aatype = _sequence_input("aatype", aatype, (L,), torch.int32)
    residue_index = _sequence_input("residue_index", residue_index, (L,), torch.int32)
    _req(atoms, name="atoms")
    dev = atoms.device
    exists, aatype, residue_index = exists.to(dev), aatype.to(dev), residue_index.to(dev)
    lib = load_library()
    losses, fractions = (torch.empty(R, 4, dtype=torch.float64, device=dev) for _ in range(2))
    per_res = torch.empty(R, L, dtype=torch.float64, device=dev)
    bond_mask = torch.empty(R, L, dtype=torch.uint8, device=dev)
    clash_mask = torch.empty(R, L, 5, dtype=torch.uint8, device=dev)
    n_pairs = torch.empty(R, dtype=torch.int32, device=dev)
    for n, p_atoms, *p_out in _row_chunks(R, rows, atoms, losses, fractions, per_res, bond_mask, clash_mask, n_pairs):
        _check(lib.s2s_backbone_violations(p_atoms, n, L, _p(exists), _p(aatype), _p(residue_index), tolerance_factor, clash_tolerance, *p_out,
                                           _stream()), "s2s_backbone_violations")
    return losses, fractions, per_res, bond_mask, clash_mask, n_pairs


def secondary_structure(atoms: torch.Tensor, aatype, residue_index, max_structures: Optional[int] = None):
    """The secondary structure and the backbone torsions of include/str2str_hip.h (Kabsch & Sander's hydrogen bonds, turns, bridges,
    ladders and bends; phi, psi, omega) of every structure of atoms [R, L, 5, 3] fp32 device tensor, atom14 slots N, CA, C, O, CB.
    ``aatype`` [L] (the reference's residue order; a PRO has no amide hydrogen) and ``residue_index`` [L] (a jump in the numbers is a chain
    break) belong to the one sequence of the ensemble.  -> device tensors (ss [R, L] uint8: the ASCII letters - B E H G I T S; n_hbonds [R]
    int32; hb_energy [R, L] fp64 and hb_partner [R, L] int32: the best acceptor of every N-H, 0.0 and -1 where there is none; torsions
    [R, L, 3] fp64: phi, psi, omega in radians, 0.0 where undefined).  ``max_structures`` bounds the structures of one launch; a
    structure's results are bit for bit the same for any value."""
    rows = _backbone_ensemble("secondary_structure", atoms, SS_MAX_RES, max_structures, SS_MAX_STRUCTURES)
    R, L = atoms.shape[:2]
    aatype = _sequence_input("aatype", aatype, (L,), torch.int32, "secondary_structure")
    residue_index = _sequence_input("residue_index", residue_index, (L,), torch.int32, "secondary_structure")
    _req(atoms, name="atoms")
    dev = atoms.device
    aatype, residue_index = aatype.to(dev), residue_index.to(dev)
    lib = load_library()
    ss = torch.empty(R, L, dtype=torch.uint8, device=dev)
    n_hbonds = torch.empty(R, dtype=torch.int32, device=dev)
    hb_energy = torch.empty(R, L, dtype=torch.float64, device=dev)
    hb_partner = torch.empty(R, L, dtype=torch.int32, device=dev)
    torsions = torch.empty(R, L, 3, dtype=torch.float64, device=dev)
    for n, p_atoms, *p_out in _row_chunks(R, rows, atoms, ss, n_hbonds, hb_energy, hb_partner, torsions):
        _check(lib.s2s_secondary_structure(p_atoms, n, L, _p(aatype), _p(residue_index), *p_out, _stream()), "s2s_secondary_structure")
    return ss, n_hbonds, hb_energy, hb_partner, torsions


def sphere_points(n_points: int) -> np.ndarray:
    """The unit sphere of the Shrake-Rupley test: the golden spiral of include/str2str_hip.h -> float64 [n_points, 3].  Built on the host
    in numpy so that the kernel and a numpy statement of the definition read the same bits."""
    P = _integer("sphere_points", "n_points", n_points, 1, SASA_MAX_POINTS)
    k = np.arange(P, dtype=np.float64)
    y = (k * (2.0 / P) - 1.0) + 1.0 / P
    r = np.sqrt(1.0 - y * y)
    phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
    return np.stack([np.cos(phi) * r, y, np.sin(phi) * r], axis=1)


def backbone_sasa(atoms: torch.Tensor, atom_exists, radii, probe: float = 1.4, n_points: int = 96, max_structures: Optional[int] = None):
    """The solvent-accessible surface of include/str2str_hip.h (Shrake and Rupley's point test on the spheres of radius ``radii + probe``)
    of every structure of atoms [R, L, 5, 3] fp32 device tensor, atom14 slots N, CA, C, O, CB.  ``atom_exists`` [L, 5] (non-zero: the atom
    exists) and ``radii`` [L, 5] (Angstrom, finite and positive where the atom exists) belong to the one sequence of the ensemble.
    -> device tensors (counts [R, L, 5] int32: the accessible points of ``sphere_points(n_points)`` per atom; per_residue [R, L] fp64 in
    A^2; total [R] fp64).  Backbone and CB only: no side chains.  ``max_structures`` bounds the structures of one launch; a structure's
    results are bit for bit the same for any value."""
    rows = _backbone_ensemble("backbone_sasa", atoms, SASA_MAX_RES, max_structures, SASA_MAX_STRUCTURES)
    R, L = atoms.shape[:2]
    exists = _sequence_input("atom_exists", atom_exists, (L, 5), torch.uint8, "backbone_sasa")
    radii = torch.as_tensor(radii)
    if radii.shape != (L, 5) or radii.is_complex():
        raise HipLibraryError(f"backbone_sasa: radii: expected numbers of shape {(L, 5)}, got {radii.dtype} {tuple(radii.shape)}")
    radii = radii.to("cpu", torch.float64).contiguous()
    there = radii[exists.cpu() != 0]
    if not bool((torch.isfinite(there) & (there > 0.0)).all()):
        raise HipLibraryError("backbone_sasa: radii must be finite and positive where the atom exists")
    probe = float(probe)
    if not 0.0 <= probe < float("inf"):
        raise HipLibraryError(f"backbone_sasa: probe must be finite and >= 0, got {probe}")
    sphere = torch.from_numpy(sphere_points(n_points))
    _req(atoms, name="atoms")
    dev = atoms.device
    exists, radii, sphere = exists.to(dev), radii.to(dev), sphere.to(dev)
    lib = load_library()
    counts = torch.empty(R, L, 5, dtype=torch.int32, device=dev)
    per_res = torch.empty(R, L, dtype=torch.float64, device=dev)
    total = torch.empty(R, dtype=torch.float64, device=dev)
    for n, p_atoms, *p_out in _row_chunks(R, rows, atoms, counts, per_res, total):
        _check(lib.s2s_backbone_sasa(p_atoms, n, L, _p(exists), _p(radii), probe, _p(sphere), int(n_points), *p_out, _stream()), "s2s_backbone_sasa")
    return counts, per_res, total


def _host_array(fn: str, what: str, v, dtype) -> np.ndarray:
    """A small per-ensemble input of ``fn`` (tensor on any device, array or list) as a contiguous host array of ``dtype``; integers stay
    integers (a float array is no list of types)."""
    try:
        a = np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v)
    except (TypeError, ValueError) as e:
        raise HipLibraryError(f"{fn}: {what}: {e}") from None
    if a.dtype == object or a.dtype.kind not in ("iu" if dtype == np.int32 else "iuf"):
        raise HipLibraryError(f"{fn}: {what}: expected {'integers' if dtype == np.int32 else 'real numbers'}, got {a.dtype}")
    return a


def ca_scattering(ca: torch.Tensor, q, types=None, table=None, max_structures: Optional[int] = None):
    """The solution scattering of include/str2str_hip.h of every structure of ca [R, L, 3] fp32 device tensor, CA beads: the Debye intensity
    I(q_k) = sum_i f_i^2 + 2 sum_{i<j} f_i f_j sin(q_k r_ij) / (q_k r_ij) at the ``q`` [Q] (1/Angstrom, finite and >= 0) and the Kirkwood
    mean inverse distance.  ``table`` [n_types, Q]: the form factor of every type at every q, finite, of any sign (None: one type, all
    ones, so I(0) = L^2); ``types`` [L]: the type of every residue, integers in 0 .. n_types - 1 (None: all 0).  -> device tensors
    (intensity [R, Q] fp64; inv_r_mean [R] fp64 = (2 / L^2) sum_{i<j} 1 / r_ij: the hydrodynamic radius is its reciprocal, inf for one
    bead, 0 for coincident beads).  No hydration shell, no excluded volume, no built-in form factors, no side chains.  ``max_structures``
    bounds the structures of one launch; a structure's results are bit for bit the same for any value."""
    fn = "ca_scattering"
    R, L = _ca_ensemble(fn, ca, SAXS_MAX_RES)
    rows = _launch_structures(fn, max_structures, SAXS_MAX_STRUCTURES)
    q = _host_array(fn, "q", q, np.float64).astype(np.float64)
    if q.ndim != 1 or not 1 <= q.size <= SAXS_MAX_Q:
        raise HipLibraryError(f"{fn}: q {q.shape}, expected [Q] with 1 <= Q <= {SAXS_MAX_Q}")
    if not (np.isfinite(q) & (q >= 0.0)).all():
        raise HipLibraryError(f"{fn}: q must be finite and >= 0")
    Q = q.size
    table = np.ones((1, Q)) if table is None else _host_array(fn, "table", table, np.float64).astype(np.float64)
    if table.ndim != 2 or table.shape[1] != Q or not 1 <= table.shape[0] <= SAXS_MAX_TYPES:
        raise HipLibraryError(f"{fn}: table {table.shape}, expected [n_types, {Q}] with 1 <= n_types <= {SAXS_MAX_TYPES}")
    if not np.isfinite(table).all():
        raise HipLibraryError(f"{fn}: table must be finite")
    types = np.zeros(L, dtype=np.int32) if types is None else _host_array(fn, "types", types, np.int32)
    if types.shape != (L,):
        raise HipLibraryError(f"{fn}: types {types.shape} for {L} residues")
    if types.size and (int(types.min()) < 0 or int(types.max()) >= table.shape[0]):
        raise HipLibraryError(f"{fn}: types must lie in 0 .. {table.shape[0] - 1}, got {int(types.min())} .. {int(types.max())}")
    _req(ca, name="ca")
    dev = ca.device
    q_d, table_d = torch.from_numpy(np.ascontiguousarray(q)).to(dev), torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    types_d = torch.from_numpy(np.ascontiguousarray(types.astype(np.int32))).to(dev)
    lib = load_library()
    intensity = torch.empty(R, Q, dtype=torch.float64, device=dev)
    inv_r_mean = torch.empty(R, dtype=torch.float64, device=dev)
    for n, p_ca, *p_out in _row_chunks(R, rows, ca, intensity, inv_r_mean):
        _check(lib.s2s_ca_scattering(p_ca, n, L, _p(q_d), Q, _p(types_d), _p(table_d), table.shape[0], *p_out, _stream()), "s2s_ca_scattering")
    return intensity, inv_r_mean


def cluster_adjacency(values: torch.Tensor, cutoff: float, at_least: bool = False, row0: int = 0, adj: Optional[torch.Tensor] = None,
                      deg: Optional[torch.Tensor] = None):
    """Rows ``row0 ..`` of an n x n matrix, values [n_rows, n] fp64 device tensor -> (adj [n, ceil(n / 64)] int64: the packed neighbour
    bits, bit j % 64 of word j // 64 of row i is ``values[i, j] <= cutoff`` (``>=`` with ``at_least``: similarities), deg [n] int32: the
    popcount of every row).  The diagonal is always set, bits past n are clear, NaN is never a neighbour.  ``adj`` / ``deg``: the buffers
    an earlier row chunk filled (the other rows are left alone); None allocates them."""
    lib = load_library()
    _req(values, torch.float64, "values")
    if values.ndim != 2 or values.shape[0] < 1 or values.shape[1] < 1:
        raise HipLibraryError(f"cluster_adjacency: values {tuple(values.shape)}")
    n_rows, n = values.shape
    if n > CLUSTER_MAX_N:
        raise HipLibraryError(f"cluster_adjacency: at most {CLUSTER_MAX_N} structures, got {n}")
    if not 0 <= row0 <= n - n_rows:
        raise HipLibraryError(f"cluster_adjacency: rows {row0} .. {row0 + n_rows - 1} of a {n} x {n} matrix")
    W = -(-n // 64)
    adj = torch.zeros(n, W, dtype=torch.int64, device=values.device) if adj is None else _req(adj, torch.int64, "adj")
    deg = torch.zeros(n, dtype=torch.int32, device=values.device) if deg is None else _req(deg, torch.int32, "deg")
    if adj.shape != (n, W) or deg.shape != (n,):
        raise HipLibraryError(f"cluster_adjacency: adj {tuple(adj.shape)}, deg {tuple(deg.shape)} for {n} structures")
    _check(lib.s2s_cluster_adjacency(_p(values), n_rows, int(row0), n, float(cutoff), int(bool(at_least)), _p(adj), _p(deg), _stream()),
           "s2s_cluster_adjacency")
    return adj, deg


def cluster_gromos(adj: torch.Tensor, deg: torch.Tensor, rounds_per_sync: int = CLUSTER_ROUNDS_PER_SYNC):
    """GROMOS clustering of the neighbour bits of ``cluster_adjacency`` (symmetric, diagonal set) -> device int32 (labels [n]: the cluster
    of every structure, ids in order of extraction; centres [K]; sizes [K], non-increasing).  The centre of a cluster is the live
    structure with the most live neighbours, the lowest index among equals.  ``rounds_per_sync`` rounds are enqueued between two
    readbacks of the live count; the result does not depend on it.  ``adj`` and ``deg`` are left as they are."""
    lib = load_library()
    _req(adj, torch.int64, "adj"); _req(deg, torch.int32, "deg")
    n = deg.numel()
    if adj.ndim != 2 or deg.ndim != 1 or n < 1 or adj.shape != (n, -(-n // 64)):
        raise HipLibraryError(f"cluster_gromos: adj {tuple(adj.shape)}, deg {tuple(deg.shape)}")
    if n > CLUSTER_MAX_N:
        raise HipLibraryError(f"cluster_gromos: at most {CLUSTER_MAX_N} structures, got {n}")
    if int(rounds_per_sync) < 1:
        raise HipLibraryError(f"cluster_gromos: rounds_per_sync {rounds_per_sync}")
    dev = adj.device
    live_deg = torch.empty_like(deg).copy_(deg)              # the loop counts its live neighbours down in place
    labels, centres, sizes = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    state = torch.empty(3, dtype=torch.int32, device=dev)
    live, members = (torch.empty(adj.shape[1], dtype=torch.int64, device=dev) for _ in range(2))
    init, enqueued = 1, 0
    while True:
        _check(lib.s2s_cluster_gromos(_p(adj), _p(live_deg), n, init, int(rounds_per_sync), _p(labels), _p(centres), _p(sizes), _p(state),
                                      _p(live), _p(members), _stream()), "s2s_cluster_gromos")
        init, enqueued = 0, enqueued + int(rounds_per_sync)
        n_live, n_clusters = state[:2].tolist()
        if n_live == 0:
            return labels, centres[:n_clusters], sizes[:n_clusters]
        if enqueued >= n:                                    # every round with something live removes at least one structure
            raise HipLibraryError(f"cluster_gromos: {n_live} of {n} structures still live after {enqueued} rounds")
