"""Essential dynamics without a device: the float64 restatement (tests/ref_pca.py) held to facts that need no device, the numpy tails of
str2str_amd.metrics on top of it, and the host side of the wrappers, the C ABI and eval.py's ``dynamics`` report."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import pca_cases as cases
import ref_pca as ref
from conftest import ROOT, record_margin
from ensemble_cases import close_4, load_eval_entry

U24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------- the restatement against known answers
@pytest.mark.parametrize("R,L", ((7, 5), (40, 17)))
def test_single_mode_is_rank_one(R, L):
    """X_s = M + a_s u with sum a_s = 0 and no fit: C = var(a) u u^T, one variance var(a) |u|^2, the component +-u / |u| under the sign
    rule, c_ij = u_i . u_j / (|u_i| |u_j|).  M, u and a are small dyadic numbers, so the float32 inputs carry them exactly."""
    rng = np.random.default_rng(R + L)
    M = rng.integers(-64, 64, size=(L, 3)) / 4.0
    u = rng.integers(-8, 9, size=(L, 3)) / 8.0
    u[0] = (-1.5, -0.5, 0.25)                                  # (no residue of the first two at rest; one largest entry, for the sign rule)
    u[1] = (0.5, 1.0, -0.125)
    a = rng.integers(-16, 17, size=R).astype(np.float64)
    a[-1] -= a.sum()
    a /= 4.0
    X = (M[None] + a[:, None, None] * u[None]).astype(np.float32)
    assert (X.astype(np.float64) == M[None] + a[:, None, None] * u[None]).all() and a.sum() == 0.0
    mean, cov = ref.ensemble_covariance(X, fit=False)
    var_a, uf = float((a * a).mean()), u.reshape(-1)
    want = var_a * np.outer(uf, uf)
    tol = 8 * 2.0 ** -52 * R                                   # (the mean is a sum of R terms with p = 1 / R, which is no dyadic number)
    assert np.abs(mean - M).max() <= tol * np.abs(X).max() and np.abs(cov - want).max() <= tol * np.abs(want).max()
    m, comps, variances, total, proj = ref.pca(X, 3, fit=False)
    lam = var_a * float(uf @ uf)
    assert abs(variances[0] - lam) <= 1e-13 * lam and (variances[1:] <= 1e-13 * lam).all() and abs(total - lam) <= 1e-13 * lam
    unit = uf / np.linalg.norm(uf)
    unit = unit * np.sign(unit[np.argmax(np.abs(unit))])
    assert np.abs(comps[0] - unit).max() <= 1e-13 and comps[0][np.argmax(np.abs(comps[0]))] > 0
    assert np.abs(proj[:, 0] - a * np.linalg.norm(uf) * np.sign(unit @ uf)).max() <= 1e-12 * np.abs(a).max()
    norms = np.linalg.norm(u, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        want_c = np.where((norms[:, None] * norms[None, :]) > 0, (u @ u.T) / (norms[:, None] * norms[None, :]), 0.0)
    np.fill_diagonal(want_c, 1.0)
    c = ref.dccm(cov)
    assert np.abs(c - want_c).max() <= 1e-13 and (np.diag(c) == 1.0).all() and (c[norms == 0] == np.eye(L)[norms == 0]).all()


def test_rigid_copies_have_no_variance():
    """Rigidly moved float32 copies of one structure, fitted: what is left is the float32 rounding of the moved copies, at most
    4 x 2^-24 x max |x| per coordinate, so tr C <= 3L (4 x 2^-24 x max |x|)^2."""
    rng = np.random.default_rng(5)
    L = 24
    M = cases.chain(rng, L)
    X = cases.rigid_moves(rng, np.repeat(M[None], 12, axis=0)).astype(np.float32)
    for route in ref.ROUTES:
        _, cov = ref.ensemble_covariance(X, route=route)
        bound = 3 * L * (4 * U24 * float(np.abs(X).max())) ** 2
        record_margin("ensemble_pca_ref_rigid_copies_trace", float(np.trace(cov)), bound)
        assert 0.0 <= np.trace(cov) <= bound, (route, np.trace(cov), bound)


@pytest.mark.parametrize("R,L", cases.FITTED_SHAPES)
def test_two_float64_routes_agree(R, L):
    """SVD Kabsch and Horn's quaternion matrix lead to the same covariance up to float64 rounding, and the fifth round no longer moves
    the top eigenvalue."""
    mean, cov, dist, _ = cases.planted_reference(R, L)
    rel = dist / float(np.linalg.norm(cov))
    print(f"R={R} L={L}: two-route distance {dist:.3e} ({rel:.3e} relative)")
    record_margin("ensemble_pca_ref_two_routes_rel", rel, 1e-12)
    assert 0.0 < rel <= 1e-12
    top4 = np.linalg.eigvalsh(ref.ensemble_covariance(cases.planted(R, L).x, n_fit_rounds=4)[1])[-1]
    top5 = np.linalg.eigvalsh(cov)[-1]
    assert abs(top5 - top4) <= 1e-4 * top5
    spectrum = np.linalg.eigvalsh(cov)[::-1]
    assert (-np.diff(spectrum[:4]) > 0.1).all()                # the planted modes stand clear of each other and of the noise
    # the three planted modes carry the variance: the top three components lie in their span once the rigid-body part is fitted away
    assert spectrum[:3].sum() >= 0.97 * spectrum.sum()


def test_case_builder_conditions():
    assert cases.away_from_float32_boundaries(np.array([1.0, 1.0 + 2.0 ** -25 + 2.0 ** -30]))
    assert not cases.away_from_float32_boundaries(np.array([1.0 + 2.0 ** -24 + 2.0 ** -50]))     # next to the midpoint of 1 and 1 + 2^-23
    pc = {"target": np.array([[0.0], [0.31], [1.0]]), "pred": np.array([[0.55]])}
    assert cases.clear_of_bin_edges(pc, n_bins=10) and not cases.clear_of_bin_edges({**pc, "pred": np.array([[0.5 + 1e-12]])}, n_bins=10)
    for R, L in cases.FITTED_SHAPES:
        assert cases.fit_is_reproducible(cases.planted(R, L).x)
    both = cases.summary_ensembles()
    assert cases.clear_of_bin_edges(ref.js_pca(both)[1]) and not cases.plain(5, 3)[0].flags.writeable


# ----------------------------------------------------------------------------------- the metrics layer on the yardstick as its device
@pytest.fixture
def yardstick_as_device(monkeypatch):
    """str2str_amd.metrics with the five device functions replaced by the restatement on host tensors."""
    from str2str_amd import ops
    from str2str_amd.metrics import metrics

    T = torch.from_numpy
    arr = lambda t: None if t is None else np.asarray(t)       # noqa: E731
    monkeypatch.setattr(ops, "ca_superpose", lambda x, target, w=None: (None, T(ref.superpose(x.numpy(), target.numpy(), arr(w)))))
    monkeypatch.setattr(ops, "ca_aligned_mean", lambda x, xform=None, p=None: T(ref.moments(x.numpy(), arr(xform), arr(p))[0]))
    monkeypatch.setattr(ops, "ca_covariance", lambda x, mean, xform=None, p=None, max_structures=None: T(ref.moments(x.numpy(), arr(xform), arr(p))[1]))
    monkeypatch.setattr(ops, "ca_project", lambda x, mean, comps, xform=None: T(ref.project(x.numpy(), mean.numpy(), comps.numpy(), arr(xform))))

    def fit(x, target=None, p=None, w=None, n_fit_rounds=5, fit=True):
        xf = ref.fit_transforms(x.numpy(), arr(target), arr(p), arr(w), n_fit_rounds, fit)
        return None if xf is None else T(xf)

    monkeypatch.setattr(ops, "ca_fit_transforms", fit)
    monkeypatch.setattr(metrics, "_dev", lambda a: (torch.as_tensor(np.array(a))[None] if np.ndim(a) == 2 else torch.as_tensor(np.array(a))).float().contiguous())
    return metrics


def test_metrics_are_the_restatements_tails(yardstick_as_device):
    metrics = yardstick_as_device
    both = cases.summary_ensembles()
    sizes = {k: len(v) for k, v in both.items()}
    x = both["target"]
    mean, cov = metrics.ensemble_covariance(x)
    want_mean, want_cov = ref.ensemble_covariance(x)
    assert mean.dtype == cov.dtype == np.float64 and (mean == want_mean).all() and (cov == want_cov).all()
    c = metrics.cross_correlation(x)
    assert np.abs(c - ref.dccm(want_cov)).max() <= 2.0 ** -50 and (np.diag(c) == 1.0).all() and np.abs(c).max() == 1.0
    model = metrics.pca(x, 4)
    want = ref.pca(x, 4)
    assert isinstance(model, metrics.EnsemblePCA) and model._fields == ("mean", "components", "variances", "total_variance", "projections")
    assert model.components.shape == (4, 60) and model.projections.shape == (60, 4) and model.variances.shape == (4,)
    assert np.abs(model.variances - want[2]).max() <= 1e-12 * want[2][0] and abs(model.total_variance - want[3]) <= 1e-12 * want[3]
    assert (np.diff(model.variances) <= 0).all() and (model.variances >= 0).all()
    assert np.abs(model.components - want[1]).max() <= 1e-10       # (same signs: the canonical rule)
    assert all(row[np.argmax(np.abs(row))] > 0 for row in model.components)
    assert np.abs(model.components @ model.components.T - np.eye(4)).max() <= 1e-13
    # the projections of the fitted ensemble itself: weighted mean 0, variances the eigenvalues
    assert np.abs(model.projections.mean(0)).max() <= 1e-12 and np.abs(model.projections.var(0) - model.variances).max() <= 1e-11
    assert np.abs(metrics.pca_project(both["resample"], model) - ref.pca_project(both["resample"], want[0], want[1])).max() <= 1e-9

    js, pc = metrics.js_pca(both)
    want_js, want_pc = ref.js_pca(both)
    assert list(js) == ["resample", "no_mode2", "target"] and js["target"] == 0.0 and want_js["target"] == 0.0
    assert all(close_4(js[k], want_js[k]) for k in both) and all(np.abs(pc[k] - want_pc[k]).max() <= 1e-9 for k in both)
    assert metrics.js_pca(both, return_pc=False) == js
    w = cases.summary_weights(both)
    js_w, want_w = metrics.js_pca(both, weights=w, return_pc=False), ref.js_pca(both, hist_weights=w)[0]
    assert all(close_4(js_w[k], want_w[k]) for k in both) and js_w["resample"] != js["resample"]
    with pytest.raises(ValueError, match="weights"):
        metrics.js_pca(both, weights={"resample": np.ones(3)})

    covs = ref.dynamics_frame(both)
    got, want_r = metrics.rmsip(both), ref.rmsip(covs, sizes)
    assert got["target"] == 1.0 and abs(want_r["target"] - 1.0) <= 1e-12 and all(close_4(got[k], want_r[k]) for k in both)
    assert metrics.rmsip({"target": x, "pred": x.copy()})["pred"] == 1.0           # an ensemble with itself
    got3 = metrics.rmsip(both, n_components=3)
    assert all(close_4(got3[k], ref.rmsip(covs, sizes, n_components=3)[k]) for k in both)
    # K = min(n_components, 3L - 6, R_ref - 1, R_k - 1): three structures leave two components
    few = {"target": x, "pred": both["resample"][:3]}
    assert close_4(metrics.rmsip(few)["pred"], ref.rmsip(ref.dynamics_frame(few), {"target": 60, "pred": 3})["pred"])
    got, want_d = metrics.dccm_mae(both), ref.dccm_mae(covs)
    assert got["target"] == 0.0 and all(close_4(got[k], want_d[k]) for k in both) and got["no_mode2"] > got["resample"] > 0.0
    got, want_v = metrics.total_variance(both), ref.total_variance(covs)
    assert all(close_4(got[k], want_v[k]) for k in both)
    # the planted truth: without the second mode the essential subspace is another one and the distribution along it collapses
    assert js["no_mode2"] > js["resample"] and metrics.rmsip(both, n_components=3)["no_mode2"] < metrics.rmsip(both, n_components=3)["resample"]


def test_too_few_structures_raise(yardstick_as_device):
    metrics = yardstick_as_device
    x = cases.plain(5, 3)[0]
    mean, cov = metrics.ensemble_covariance(x[:1], fit=False)
    assert (cov == 0.0).all() and cov.shape == (9, 9) and (mean == x[0].astype(np.float64)).all()      # one structure: all zeros
    for call in (lambda: metrics.pca(x[:1]), lambda: metrics.js_pca({"target": x[:1], "pred": x}), lambda: metrics.rmsip({"target": x, "pred": x[:1]}),
                 lambda: metrics.dccm_mae({"target": x[:1], "pred": x}), lambda: metrics.total_variance({"target": x, "pred": x[:1]})):
        with pytest.raises(ValueError, match="at least 2 structures"):
            call()
    with pytest.raises(ValueError, match="rmsip"):              # 3L - 6 = 3 > 0 but n_components = 0 leaves K < 1
        metrics.rmsip({"target": x, "pred": x}, n_components=0)
    with pytest.raises(ValueError, match="rmsip"):              # two residues: 3L - 6 = 0
        metrics.rmsip({"target": x[:, :2], "pred": x[:, :2]})
    for bad in (0, 10, 2.5, True):
        with pytest.raises(ValueError, match="n_components"):
            metrics.pca(x, bad)


# ------------------------------------------------------------------------------------------------------------- the host side
def _wrapper_cases():
    ca, mean = torch.zeros(6, 8, 3), torch.zeros(8, 3, dtype=torch.float64)
    return {"ca_aligned_mean": dict(ca=ca), "ca_covariance": dict(ca=ca, mean=mean),
            "ca_project": dict(ca=ca, mean=mean, components=torch.zeros(2, 24, dtype=torch.float64)), "ca_fit_transforms": dict(ca=ca)}


@pytest.mark.parametrize("fn", list(_wrapper_cases()))
def test_wrappers_reject_bad_arguments_before_the_device(fn, monkeypatch):
    from str2str_amd import ops
    from str2str_amd.ops import ensemble

    def touched(*a, **k):
        raise AssertionError("touched the device")

    monkeypatch.setattr(ensemble, "load_library", touched)
    kwargs = _wrapper_cases()[fn]
    call = getattr(ops, fn)
    with pytest.raises(ops.HipLibraryError, match="no CPU fallback"):
        call(**kwargs)
    with pytest.raises(ops.HipLibraryError, match=f"^{fn}: coordinates ca"):
        call(**{**kwargs, "ca": torch.zeros(6, 8, 2)})
    with pytest.raises(ops.HipLibraryError, match=f"^{fn}: at most {ops.PCA_MAX_RES} residues"):
        call(**{**kwargs, "ca": torch.zeros(1, ops.PCA_MAX_RES + 1, 3)})
    if fn != "ca_fit_transforms":
        with pytest.raises(ops.HipLibraryError, match=f"^{fn}: xform"):
            call(**kwargs, xform=torch.zeros(5, 12, dtype=torch.float64))
    if fn != "ca_project":
        for bad in (np.ones(5), -np.ones(6), np.zeros(6), np.full(6, np.inf)):
            with pytest.raises(ops.HipLibraryError, match=f"^{fn}: sample_weights"):
                call(**kwargs, sample_weights=bad)
    if fn == "ca_covariance":
        for bad in (0, -1, True, 1.5):
            with pytest.raises(ops.HipLibraryError, match="^" + re.escape(f"{fn}: max_structures must be an integer >= 1, got {bad}") + "$"):
                call(**kwargs, max_structures=bad)
        with pytest.raises(ops.HipLibraryError, match=f"^{fn}: mean"):
            call(**{**kwargs, "mean": torch.zeros(7, 3, dtype=torch.float64)})
    if fn == "ca_project":
        with pytest.raises(ops.HipLibraryError, match=f"^{fn}: mean"):
            call(**{**kwargs, "components": torch.zeros(2, 23, dtype=torch.float64)})
    if fn == "ca_fit_transforms":
        for bad in (0, -1, True, 1.5):
            with pytest.raises(ops.HipLibraryError, match="^" + re.escape(f"{fn}: n_fit_rounds must be an integer >= 1, got {bad}") + "$"):
                call(**kwargs, n_fit_rounds=bad)
        assert call(**kwargs, n_fit_rounds=0, fit=False) is None       # the count is checked when fitting only
        with pytest.raises(ops.HipLibraryError, match=f"^{fn}: coordinates ca"):
            call(**kwargs, target=torch.zeros(7, 3))


def test_header_binding_and_build_agree():
    from str2str_amd import build, ops
    from str2str_amd.ops import binding

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "str2str_hip.h")).read(), flags=re.S)
    for name, arity in (("s2s_ca_aligned_mean", 7), ("s2s_ca_covariance", 10), ("s2s_ca_project", 9)):
        proto = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr, flags=re.M)
        assert proto, name
        args = [a.strip() for a in proto.group(1).split(",")]
        assert len(args) == len(binding._SIGNATURES[name]) == arity and args[-1] == "void* stream" and name in ops.EXPORTS
    assert "S2S_PCA_MAX_RES 1024" in hdr and ops.PCA_MAX_RES == 1024
    assert build.UNITS["ensemble_pca.hip"] == [] and os.path.isfile(os.path.join(build.CSRC, "ensemble_pca.hip"))
    assert all(callable(getattr(ops, f)) for f in ("ca_aligned_mean", "ca_covariance", "ca_project", "ca_fit_transforms"))


def test_dynamics_report_columns_and_switch(monkeypatch):
    from str2str_amd.utils import config as C

    entry = load_eval_entry("s2s_eval_entry_dynamics_cpu")
    assert entry.DYNAMICS_COLUMNS == ("js_pca", "rmsip", "dccm_mae", "var_total", "var_total_target")
    report = entry.REPORTS[4]
    assert len(entry.REPORTS) == 5 and report == entry.Report("dynamics", "dynamics", entry.DYNAMICS_COLUMNS, entry.dynamics_row, True)
    assert len(entry.EXTRA_METRICS) == 12
    others = set(entry.EXTRA_METRICS) | set(entry.CLUSTER_COLUMNS) | set(entry.metric_columns(None)) | {"saxs_chi2"}
    for attr in ("SS_COLUMNS", "CONTACT_COLUMNS", "SASA_COLUMNS", "SAXS_COLUMNS"):
        others |= set(getattr(entry, attr))
    assert not set(entry.DYNAMICS_COLUMNS) & others
    monkeypatch.setenv("TEST_DATA", "/nonexistent")
    compose = lambda *args: C.compose(os.path.join(ROOT, "configs"), "eval.yaml", list(args))   # noqa: E731
    switch = entry.dynamics_switch
    assert switch(compose("+dynamics=true").get("dynamics")) is True and switch(compose("+dynamics=false").get("dynamics")) is False
    assert compose().get("dynamics") is None
    for value, want in ((None, False), (True, True), (False, False), ("true", True), ("false", False), ("False", False), (" True ", True),
                        ("0", False), ("yes", True)):
        assert switch(value) is want
    for bad in ("maybe", 2, 1.0, 2.5, [True]):
        with pytest.raises(ValueError, match="dynamics"):
            switch(bad)
    with pytest.raises(ValueError, match="dynamics"):           # rejected before anything is read or written
        entry.evaluate_prediction("/nonexistent/pred", "/nonexistent/target", dynamics="maybe")
    assert inspect.signature(entry.evaluate_prediction).parameters["dynamics"].default is None
