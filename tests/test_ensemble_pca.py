"""Essential dynamics on the device (csrc/ensemble_pca.hip) against the float64 numpy restatement in tests/ref_pca.py.

Without fit the two sides hold the same float64 y (the widened float32 coordinates) and differ in the order of their sums alone; the
bounds are the project's reordered-sum rule with u = 2^-52 (each side is within (n - 1) u / 2 of the exact sum relative to the sum of the
terms' magnitudes; the 16 covers the roundings of a term: the square roots of the weights, the products, the subtraction of the mean):

    |mean - ref|        <= (R + 16) u sum_s p_s |y_sc|
    |C[r, c] - ref|     <= (R + 16) u sum_s p_s |z_sr| |z_sc|,   z = y - m      (the CENTRED magnitudes: what the offset cases are for --
                                                                                 a one-pass E[xy] - E[x] E[y] fails them by 100^2)
    |proj[s, k] - ref|  <= (3L + 16) u sum_c |z_sc| |v_kc|

The device centres about its own mean, which differs from the yardstick's by some delta <= the first bound; C changes by
-delta_r sum_s p_s z_sc - delta_c sum_s p_s z_sr + delta_r delta_c, and sum_s p_s z_s is itself a rounding residue: second order.

With fit the superposition enters: the device's Jacobi solve is a third float64 route next to the yardstick's two (SVD, Horn + eigh), so
||C_gpu - C_ref||_F is held to the a-priori term above in Frobenius norm plus 16 x the distance between the yardstick's two routes (one
sample of rounding noise is no ceiling).  Weyl and Davis-Kahan then bound the variances and the top components by the measured
||C_gpu - C_ref||_F."""
import glob
import os

import numpy as np
import pytest
import torch

import pca_cases as cases
import ref_pca as ref
from conftest import GOLDEN, record_margin
from ensemble_cases import close_4, load_eval_entry, to_device as _dev, write_models

pytestmark = pytest.mark.gpu

U52, U24 = 2.0 ** -52, 2.0 ** -24


def _apriori_cov_bound(z, p):
    """[3L, 3L]: (R + 16) u sum_s p_s |z_sr| |z_sc|."""
    return (len(z) + 16) * U52 * ((p[:, None] * np.abs(z)).T @ np.abs(z))


@pytest.mark.parametrize("offset", (False, True), ids=("origin", "offset100"))
@pytest.mark.parametrize("weighted", (False, True), ids=("uniform", "weighted"))
@pytest.mark.parametrize("R,L", cases.PLAIN_SHAPES)
def test_moments_and_projection_without_fit(R, L, weighted, offset):
    """(5, 3): 9 coordinates, a partial tile, R no multiple of 4; (33, 16): exactly one 48-block; (40, 17): a second block with 3 live
    rows; (130, 40): 2.5 blocks, so off-diagonal and mirrored blocks;
    (6, 33): 99 coordinates, three blocks with a 3-wide last one at odd row and column blocks, and only two k-steps."""
    from str2str_amd import ops

    x, p = cases.plain(R, L, weighted, offset)
    want_mean, want_cov, z, pn = cases.plain_reference(R, L, weighted, offset)
    xd = _dev(x)
    mean = ops.ca_aligned_mean(xd, None, p)
    cov = ops.ca_covariance(xd, mean, None, p)
    assert mean.is_cuda and cov.is_cuda and mean.dtype == cov.dtype == torch.float64 and mean.shape == (L, 3) and cov.shape == (3 * L, 3 * L)
    mean_h, cov_h = mean.cpu().numpy(), cov.cpu().numpy()
    y = x.astype(np.float64).reshape(R, -1)
    share_m = float((np.abs(mean_h - want_mean).reshape(-1) / ((R + 16) * U52 * (pn[:, None] * np.abs(y)).sum(0))).max())
    share_c = float((np.abs(cov_h - want_cov) / _apriori_cov_bound(z, pn)).max())
    print(f"R={R} L={L} weighted={weighted} offset={offset}: mean at {share_m:.3e} of its bound, covariance at {share_c:.3e}")
    record_margin("ensemble_pca_mean_of_apriori_bound", share_m, 1.0)
    record_margin("ensemble_pca_covariance_of_apriori_bound", share_c, 1.0)
    assert share_m <= 1.0 and share_c <= 1.0
    assert cov_h.tobytes() == np.ascontiguousarray(cov_h.T).tobytes()                       # exactly symmetric
    for max_structures in (4, 8, R):                                                        # any chunking: identical bytes
        assert torch.equal(ops.ca_covariance(xd, mean, None, p, max_structures=max_structures), cov), max_structures
    # projection onto random unit vectors about the yardstick's mean: the same z on both sides
    K = min(5, 3 * L)
    v = np.linalg.qr(np.random.default_rng(R).normal(size=(3 * L, K)))[0].T.copy()
    proj = ops.ca_project(xd, _dev(want_mean.copy()), _dev(v)).cpu().numpy()
    share_p = float((np.abs(proj - z @ v.T) / ((3 * L + 16) * U52 * (np.abs(z) @ np.abs(v).T))).max())
    record_margin("ensemble_pca_projection_of_apriori_bound", share_p, 1.0)
    assert proj.shape == (R, K) and share_p <= 1.0, share_p
    # a row slice of the ensemble as its own call: the sub-ensemble's result, whatever lies around it in memory
    a, b = 1, R - 1
    ps = None if p is None else p[a:b]
    sub_mean, sub_cov, sub_z, sub_p = ref.moments(x[a:b], None, ps)
    got_mean = ops.ca_aligned_mean(xd[a:b], None, ps)
    got_cov = ops.ca_covariance(xd[a:b], got_mean, None, ps)
    assert (np.abs(got_cov.cpu().numpy() - sub_cov) <= _apriori_cov_bound(sub_z, sub_p)).all()
    alone = xd[a:b].clone()
    assert torch.equal(ops.ca_aligned_mean(alone, None, ps), got_mean) and torch.equal(ops.ca_covariance(alone, got_mean, None, ps), got_cov)
    assert torch.equal(ops.ca_project(xd[a:b], mean, _dev(v)), ops.ca_project(xd, mean, _dev(v))[a:b])


def test_one_structure_and_identity_transforms():
    from str2str_amd import ops
    from str2str_amd.metrics import metrics

    x, _ = cases.plain(33, 16)
    mean, cov = metrics.ensemble_covariance(x[:1], fit=False)
    assert (cov == 0.0).all() and (mean == x[0].astype(np.float64)).all()
    xd = _dev(x)
    eye = torch.tensor([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=torch.float64, device="cuda").repeat(33, 1)
    m0, m1 = ops.ca_aligned_mean(xd), ops.ca_aligned_mean(xd, eye)
    assert torch.equal(m0, m1) and torch.equal(ops.ca_covariance(xd, m0), ops.ca_covariance(xd, m0, eye))
    assert ops.ca_fit_transforms(xd, fit=False) is None
    assert torch.equal(ops.ca_fit_transforms(xd, n_fit_rounds=1), ops.ca_superpose(xd, xd[0])[1])
    with pytest.raises(ValueError, match="at least 2 structures"):
        metrics.pca(x[:1])


@pytest.mark.parametrize("R,L", cases.FITTED_SHAPES)
def test_fitted_covariance_pca_and_cross_correlation(R, L):
    from str2str_amd.metrics import metrics

    c = cases.planted(R, L)
    want_mean, want_cov, two_routes, z = cases.planted_reference(R, L)
    mean, cov = metrics.ensemble_covariance(c.x)
    assert cov.tobytes() == np.ascontiguousarray(cov.T).tobytes()
    delta = float(np.linalg.norm(cov - want_cov))
    bound = float(np.linalg.norm(_apriori_cov_bound(z, np.full(R, 1.0 / R)))) + 16.0 * two_routes
    print(f"R={R} L={L}: ||C_gpu - C_ref||_F = {delta:.3e}, bound {bound:.3e} (two routes {two_routes:.3e}), share {delta / bound:.3f}")
    record_margin(f"ensemble_pca_fitted_covariance_frobenius R={R} L={L}", delta, bound)
    record_margin("ensemble_pca_fitted_covariance_frobenius_of_bound", delta / bound, 1.0)
    assert delta <= bound
    assert np.abs(mean - want_mean).max() <= 1e-11 * np.abs(want_mean).max()
    # Weyl: every eigenvalue moves by at most ||dC||_2 <= ||dC||_F
    model = metrics.pca(c.x, 3)
    spectrum, vectors = np.linalg.eigh(want_cov)
    spectrum, vectors = spectrum[::-1], vectors[:, ::-1].T
    d_var = float(np.abs(model.variances - spectrum[:3]).max())
    print(f"  variances off by {d_var:.3e} (Weyl: {delta:.3e})")
    assert d_var <= delta
    assert abs(model.total_variance - np.trace(want_cov)) <= np.sqrt(3 * L) * delta
    # Davis-Kahan: sin(theta) <= 2 ||dC||_F / gap, gap = the distance of the eigenvalue to its nearest neighbour in the reference spectrum
    for k in range(3):
        gap = min(spectrum[k - 1] - spectrum[k] if k else np.inf, spectrum[k] - spectrum[k + 1])
        v = model.components[k]
        sin = float(np.linalg.norm(v - vectors[k] * (vectors[k] @ v)))
        print(f"  component {k}: sin(theta) = {sin:.3e}, Davis-Kahan {2 * delta / gap:.3e} (gap {gap:.3f})")
        assert gap > 0.1 and sin <= 2.0 * delta / gap, (k, sin, gap)
        assert v[np.argmax(np.abs(v))] > 0.0
    assert np.abs(model.projections.var(0) - model.variances).max() <= 1e-9 * model.variances[0]
    cc = metrics.cross_correlation(c.x)
    assert (np.diag(cc) == 1.0).all() and cc.min() >= -1.0 and cc.max() <= 1.0 and cc.tobytes() == np.ascontiguousarray(cc.T).tobytes()
    assert np.abs(cc - ref.dccm(want_cov)).max() <= 1e-9
    # consistency with what exists: one round onto X[0] is rmsf's superposition; rmsf rounds the aligned coordinates to float32 and
    # this path does not
    _, cov1 = metrics.ensemble_covariance(c.x, target=c.x[0], n_fit_rounds=1)
    fluct = np.sqrt(np.einsum("iaia->i", cov1.reshape(L, 3, L, 3)))
    d_rmsf = float(np.abs(fluct - metrics.rmsf(c.x)).max())
    record_margin("ensemble_pca_rmsf_consistency", d_rmsf, 4 * U24 * float(np.abs(c.x).max()))
    assert d_rmsf <= 4 * U24 * float(np.abs(c.x).max())


def test_summaries_equal_the_restatements_tails():
    from str2str_amd.metrics import metrics

    both = cases.summary_ensembles()
    sizes = {k: len(v) for k, v in both.items()}
    js, pc = metrics.js_pca(both)
    want_js, want_pc = ref.js_pca(both)
    assert js["target"] == 0.0 and all(close_4(js[k], want_js[k]) for k in both), (js, want_js)
    assert all(np.abs(pc[k] - want_pc[k]).max() <= 1e-9 for k in both)
    covs = ref.dynamics_frame(both)
    rm, dm, tv = metrics.rmsip(both), metrics.dccm_mae(both), metrics.total_variance(both)
    assert rm["target"] == 1.0 and dm["target"] == 0.0
    for got, want in ((rm, ref.rmsip(covs, sizes)), (dm, ref.dccm_mae(covs)), (tv, ref.total_variance(covs))):
        assert all(close_4(got[k], want[k]) for k in both), (got, want)
    rm3, want3 = metrics.rmsip(both, n_components=3), ref.rmsip(covs, sizes, n_components=3)
    assert all(close_4(rm3[k], want3[k]) for k in both)
    # the second planted mode switched off: further from the reference along its components, and another essential subspace
    assert js["no_mode2"] > js["resample"] and rm["no_mode2"] < rm["resample"] and rm3["no_mode2"] < rm3["resample"]
    w = cases.summary_weights(both)
    js_w, want_w = metrics.js_pca(both, weights=w, return_pc=False), ref.js_pca(both, hist_weights=w)[0]
    assert all(close_4(js_w[k], want_w[k]) for k in both) and js_w["resample"] != js["resample"]
    with pytest.raises(ValueError, match="weights"):
        metrics.js_pca(both, weights={"resample": np.ones(3)})
    model = metrics.pca(both["target"], 2)
    assert metrics.pca_project(both["target"], model).tobytes() == pc["target"].tobytes()


def test_eval_dynamics_switch(tmp_path):
    """The CLN025 fixture as an ensemble of noisy copies.  With the switch: the dynamics csv (DYNAMICS_COLUMNS, a mean row) and the
    cross-correlation table of L (L - 1) / 2 rows; the metrics csv is byte for byte the one of a run without the switch, which writes no
    dynamics file at all.  The target ensemble scored against itself has js_pca 0.0 and rmsip 1.0."""
    from str2str_amd.common.pdb_utils import extract_backbone_coords

    entry = load_eval_entry("s2s_eval_entry_dynamics")
    fixture = os.path.join(GOLDEN, "pdb", "CLN025.pdb")
    tgt = extract_backbone_coords(fixture)
    L = tgt.shape[1]
    rng = np.random.default_rng(21)
    target_dir = tmp_path / "targets"
    target_dir.mkdir()
    write_models(str(target_dir / "CLN025.pdb"), fixture, tgt[0][None] + rng.normal(size=(12, L, 3)) * 0.8)
    samples = tgt[0][None] + rng.normal(size=(9, L, 3)) * 0.6
    listing = {}
    for sub, switch, own in (("plain", None, False), ("dynamics", True, False), ("itself", "true", True)):
        pred_dir = tmp_path / sub / "samples" / "all"
        pred_dir.mkdir(parents=True)
        if own:
            write_models(str(pred_dir / "CLN025.pdb"), fixture, extract_backbone_coords(str(target_dir / "CLN025.pdb")))
        else:
            write_models(str(pred_dir / "CLN025.pdb"), fixture, samples)
        entry.evaluate_prediction(str(pred_dir), str(target_dir), tag="t", dynamics=switch)
        files = glob.glob(str(tmp_path / sub / "metrics_t_*.csv"))
        assert len(files) == 1
        listing[sub] = (sorted(os.listdir(tmp_path / sub)), open(files[0], "rb").read())
    assert [f.split("_")[0] for f in listing["plain"][0]] == ["metrics", "samples"]
    assert [f.split("_")[0] for f in listing["dynamics"][0]] == ["dynamics", "dynamics", "metrics", "samples"]
    assert listing["dynamics"][1] == listing["plain"][1]

    def rows_of(sub):
        path = glob.glob(str(tmp_path / sub / "dynamics_t_*.csv"))[0]
        return {r[0]: r[1:] for r in (ln.rstrip("\n").split("\t") for ln in open(path))}

    rows = rows_of("dynamics")
    assert rows[""] == list(entry.DYNAMICS_COLUMNS) and set(rows) == {"", "CLN025", "mean"} and rows["mean"] == rows["CLN025"]
    ca = {"target": extract_backbone_coords(str(target_dir / "CLN025.pdb")),
          "pred": extract_backbone_coords(str(tmp_path / "dynamics" / "samples" / "all" / "CLN025.pdb"))}
    covs = ref.dynamics_frame(ca)
    want = (ref.js_pca(ca)[0]["pred"], ref.rmsip(covs, {k: len(v) for k, v in ca.items()})["pred"], ref.dccm_mae(covs)["pred"],
            ref.total_variance(covs)["pred"], ref.total_variance(covs)["target"])
    got = [float(v) for v in rows["CLN025"]]
    assert all(close_4(g, w) for g, w in zip(got, want)), (got, want)
    assert 0.0 < got[0] < 1.0 and 0.0 < got[1] < 1.0 and got[3] > 0.0 and got[4] > got[3]
    table = [ln.rstrip("\n").split("\t") for ln in open(tmp_path / "dynamics" / "dynamics" / "CLN025.csv")]
    assert table[0] == ["i", "j", "c_pred", "c_target"] and len(table) == 1 + L * (L - 1) // 2
    body = np.array([[float(v) for v in row] for row in table[1:]])
    i, j = np.triu_indices(L, k=1)
    assert (body[:, 0] == i).all() and (body[:, 1] == j).all() and np.abs(body[:, 2:]).max() <= 1.0
    assert np.abs(body[:, 2] - ref.dccm(covs["pred"])[i, j]).max() <= 1e-4 and np.abs(body[:, 3] - ref.dccm(covs["target"])[i, j]).max() <= 1e-4
    own = [float(v) for v in rows_of("itself")["CLN025"]]
    assert own[0] == 0.0 and own[1] == 1.0 and own[2] == 0.0 and own[3] == own[4]
    # a target of a single structure does not move: a warning, NaN columns and an empty table, the metrics csv as ever
    pred_dir = tmp_path / "single" / "samples" / "all"
    pred_dir.mkdir(parents=True)
    write_models(str(pred_dir / "CLN025.pdb"), fixture, samples)
    entry.evaluate_prediction(str(pred_dir), os.path.join(GOLDEN, "pdb"), tag="t", dynamics=True)
    assert rows_of("single")["CLN025"] == [""] * 5
    assert open(tmp_path / "single" / "dynamics" / "CLN025.csv").read().split() == ["i", "j", "c_pred", "c_target"]
