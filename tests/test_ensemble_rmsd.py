"""Minimum RMSD under optimal superposition on the device (csrc/ensemble_rmsd.hip) against a float64 SVD Kabsch written here.

The reference repository has no such function, so the yardstick is this file's own: weighted centring, ``np.linalg.svd`` of the
cross-covariance H, lambda = s0 + s1 + sign(det(U V^T)) s2 (proper rotations only), MSD = (G_a + G_b - 2 lambda) / W.
tests/test_ensemble_rmsd_cpu.py guards it against an independent evaluation (``eigvalsh`` of Horn's 4 x 4).

Bounds (a-priori rounding bounds, not fitted):
  MSD   |MSD_gpu - MSD_ref| <= 8 * 2^-53 * (S_a + S_b), S = sum_i w_i |x_i|^2 of the RAW coordinates: G_a, G_b and the nine entries of H
        are L-term float64 sums (error <= L u x the sum of magnitudes), lambda_max is 2-Lipschitz in ||H||_F, which gives 3 u (G_a + G_b)
        for the minimum; the rest of the 8 covers the centring and the eigen-solve.  L = 1: exactly 0.
  RMSD  <= 1e-4 A everywhere (the project's standard), <= 1e-9 A wherever RMSD_ref >= 0.01 A (the square root amplifies near 0).
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, record_margin
from ensemble_cases import load_eval_entry, to_device as _dev, write_models

pytestmark = pytest.mark.gpu

U64 = 2.0 ** -53
LENGTHS = (1, 2, 3, 7, 35, 80, 255, 256, 512)
CROSS = ((1, 5), (17, 24), (100, 17), (5, 100))
SELF = (1, 5, 17, 24, 100)
SIGMAS = (1e-3, 0.05, 0.5, 2.0, 8.0)


# ------------------------------------------------------------------------------------------------------------------ input recipe
def random_walk(rng, L):
    step = rng.normal(size=(L, 3))
    step *= 3.8 / np.linalg.norm(step, axis=1, keepdims=True)
    return np.cumsum(step, axis=0)


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def make_ensemble(rng, n, L, base, first_kind=0):
    """n structures [n, L, 3] float32 around ``base``: exact copies, copies with Gaussian noise of the SIGMAS, unrelated chains, mirror
    images and an exactly collinear chain, in turn; each under a random rotation and a translation of up to 50 A per axis."""
    out, kinds = [], []
    for s in range(n):
        kind = (s + first_kind) % 9
        if kind == 0:
            x = base.copy()
        elif kind <= 5:
            x = base + rng.normal(size=base.shape) * SIGMAS[kind - 1]
        elif kind == 6:
            x = random_walk(rng, L)
        elif kind == 7:
            x = base * np.array([-1.0, 1.0, 1.0])
        else:
            x = np.arange(L)[:, None] * 3.8 * np.array([[0.6, 0.0, 0.8]])
        out.append(x @ random_rotation(rng).T + rng.uniform(-50.0, 50.0, size=3))
        kinds.append(kind)
    return np.asarray(out, dtype=np.float32), kinds


def make_weights(rng, L, mode):
    if mode == "none":
        return None
    if mode == "two" and L >= 3:       # all but two residues zeroed
        w = np.zeros(L, dtype=np.float32)
        w[rng.choice(L, size=2, replace=False)] = rng.uniform(0.5, 2.0, size=2)
        return w
    w = rng.uniform(0.5, 2.0, size=L).astype(np.float32)
    w[2::3] = 0.0                      # every third weight is zero
    return w


# ------------------------------------------------------------------------------------------------------- float64 SVD reference
def _centre(x, w):
    x = np.asarray(x, dtype=np.float64)
    w = np.ones(x.shape[-2]) if w is None else np.asarray(w, dtype=np.float64)
    c = (w[:, None] * x).sum(-2, keepdims=True) / w.sum()
    d = x - c
    return d, w, (w * (d * d).sum(-1)).sum(-1), c[..., 0, :]


def ref_msd_matrix(a, b, w=None):
    """-> (MSD [n_a, n_b], bound scale S_a + S_b [n_a, n_b], G_a + G_b [n_a, n_b]) in float64."""
    da, ww, ga, _ = _centre(a, w)
    db, _, gb, _ = _centre(b, w)
    h = np.einsum("ail,bim->ablm", da * ww[:, None], db)
    u, s, vt = np.linalg.svd(h)
    sign = np.sign(np.linalg.det(u @ vt))
    lam = s[..., 0] + s[..., 1] + sign * s[..., 2]
    msd = (ga[:, None] + gb[None, :] - 2.0 * lam) / ww.sum()
    raw = lambda x: (ww * (np.asarray(x, dtype=np.float64) ** 2).sum(-1)).sum(-1)  # noqa: E731
    if a.shape[1] == 1:
        msd = np.zeros_like(msd)
    return msd, raw(a)[:, None] + raw(b)[None, :], ga[:, None] + gb[None, :]


def ref_rmsd_matrix(a, b, w=None):
    return np.sqrt(np.maximum(ref_msd_matrix(a, b, w)[0], 0.0))


def ref_superpose(mobile, target, w=None):
    """float64 Kabsch -> (rotation [R, 3, 3], translation [R, 3]) with det = +1."""
    dm, ww, _, cm = _centre(mobile, w)
    dt, _, _, ct = _centre(target[None], w)
    h = np.einsum("ail,im->alm", dm * ww[:, None], dt[0])      # sum w m t^T
    u, s, vt = np.linalg.svd(h)
    d = np.sign(np.linalg.det(u @ vt))
    u[..., :, 2] *= d[:, None]
    rot = np.swapaxes(u @ vt, -1, -2)                           # R = V D U^T
    return rot, ct - np.einsum("rij,rj->ri", rot, cm)


def f32_formula_rmsd(a, b, w=None):
    """The same formula evaluated in float32 (centring, G, H, eigenvalue of the 4 x 4): recorded, not asserted."""
    f = np.float32
    ww = np.ones(a.shape[1], dtype=f) if w is None else np.asarray(w, dtype=f)
    cen = lambda x: x - ((ww[:, None] * x).sum(-2, keepdims=True, dtype=f) / ww.sum(dtype=f)).astype(f)  # noqa: E731
    da, db = cen(np.asarray(a, dtype=f)), cen(np.asarray(b, dtype=f))
    ga, gb = (ww * (da * da).sum(-1, dtype=f)).sum(-1, dtype=f), (ww * (db * db).sum(-1, dtype=f)).sum(-1, dtype=f)
    h = np.einsum("ail,bim->ablm", da * ww[:, None], db).astype(f)
    lam = np.linalg.eigvalsh(horn(h).astype(f))[..., -1]
    msd = ((ga[:, None] + gb[None, :] - f(2) * lam) / ww.sum(dtype=f)).astype(f)
    return np.sqrt(np.maximum(msd, f(0))).astype(np.float64)


def horn(h):
    """Horn's symmetric 4 x 4 of H [..., 3, 3] = sum w a b^T (largest eigenvalue = max of tr(R H) over proper rotations)."""
    k = np.zeros(h.shape[:-2] + (4, 4), dtype=h.dtype)
    k[..., 0, 0] = h[..., 0, 0] + h[..., 1, 1] + h[..., 2, 2]
    k[..., 1, 1] = h[..., 0, 0] - h[..., 1, 1] - h[..., 2, 2]
    k[..., 2, 2] = -h[..., 0, 0] + h[..., 1, 1] - h[..., 2, 2]
    k[..., 3, 3] = -h[..., 0, 0] - h[..., 1, 1] + h[..., 2, 2]
    k[..., 0, 1] = k[..., 1, 0] = h[..., 1, 2] - h[..., 2, 1]
    k[..., 0, 2] = k[..., 2, 0] = h[..., 2, 0] - h[..., 0, 2]
    k[..., 0, 3] = k[..., 3, 0] = h[..., 0, 1] - h[..., 1, 0]
    k[..., 1, 2] = k[..., 2, 1] = h[..., 0, 1] + h[..., 1, 0]
    k[..., 1, 3] = k[..., 3, 1] = h[..., 2, 0] + h[..., 0, 2]
    k[..., 2, 3] = k[..., 3, 2] = h[..., 1, 2] + h[..., 2, 1]
    return k


# ------------------------------------------------------------------------------------------------------------------------ checks
def check_matrix(tag, got, a, b, w):
    msd_ref, s_raw, g_sum = ref_msd_matrix(a, b, w)
    rmsd_ref = np.sqrt(np.maximum(msd_ref, 0.0))
    L = a.shape[1]
    assert got.shape == rmsd_ref.shape and got.dtype == np.float64 and np.isfinite(got).all()
    d_msd, bound = np.abs(got * got - np.maximum(msd_ref, 0.0)), 8.0 * U64 * s_raw
    d_rmsd = np.abs(got - rmsd_ref)
    big = rmsd_ref >= 0.01
    f32_err = np.abs(f32_formula_rmsd(a, b, w) - rmsd_ref)
    print(f"{tag}: msd err / bound = {float((d_msd / bound).max()):.3f}  rmsd err = {float(d_rmsd.max()):.3e}"
          f"  (>= 0.01 A: {float(d_rmsd[big].max()) if big.any() else 0.0:.3e})  float32 formula rmsd err = {float(f32_err.max()):.3e}"
          f"  = {float((np.abs(f32_formula_rmsd(a, b, w) ** 2 - np.maximum(msd_ref, 0)) / (2.0 ** -24 * g_sum)).max()) if L > 1 else 0.0:.3f}"
          " x 2^-24 (G_a + G_b) in MSD")
    record_margin("ensemble_rmsd_msd_over_bound", float((d_msd / bound).max()), 1.0)
    record_margin("ensemble_rmsd_rmsd_abs", float(d_rmsd.max()), 1e-4)
    if big.any():
        record_margin("ensemble_rmsd_rmsd_abs_above_0.01A", float(d_rmsd[big].max()), 1e-9)
    record_margin("ensemble_rmsd_float32_formula_rmsd_abs(recorded, not asserted)", float(f32_err.max()), 1e-4)
    if L == 1:
        assert (got == 0.0).all()
    assert (d_msd <= bound).all(), (tag, float((d_msd / bound).max()))
    assert d_rmsd.max() <= 1e-4, (tag, float(d_rmsd.max()))
    assert not big.any() or d_rmsd[big].max() <= 1e-9, (tag, float(d_rmsd[big].max()))


@pytest.mark.parametrize("wmode", ["none", "third", "two"])
@pytest.mark.parametrize("L", LENGTHS)
def test_rmsd_matrix_against_float64_svd(L, wmode):
    from str2str_amd import ops

    rng = np.random.default_rng(1000 + L)
    base = random_walk(rng, L)
    w = make_weights(rng, L, wmode)
    for n_a, n_b in CROSS:
        a, _ = make_ensemble(rng, n_a, L, base)
        b, _ = make_ensemble(rng, n_b, L, base, first_kind=3)
        got = ops.ca_rmsd_matrix(_dev(a), _dev(b), _dev(w)).cpu().numpy()
        check_matrix(f"cross L={L} {n_a}x{n_b} w={wmode}", got, a, b, w)
    for n in SELF:
        a, _ = make_ensemble(rng, n, L, base)
        got = ops.ca_rmsd_matrix(_dev(a), None, _dev(w)).cpu().numpy()
        check_matrix(f"self L={L} n={n} w={wmode}", got, a, a, w)
        assert (got == got.T).all()                      # exactly symmetric
        assert np.abs(np.diag(got)).max() <= 1e-4


def test_mirror_image_is_not_superposable():
    from str2str_amd import ops

    rng = np.random.default_rng(7)
    base = random_walk(rng, 35)
    mirror = base * np.array([1.0, 1.0, -1.0])
    a = np.asarray([base @ random_rotation(rng).T + 10.0], dtype=np.float32)
    b = np.asarray([mirror @ random_rotation(rng).T - 20.0], dtype=np.float32)
    got = ops.ca_rmsd_matrix(_dev(a), _dev(b)).cpu().numpy()
    check_matrix("mirror L=35", got, a, b, None)
    # with improper rotations allowed the two would superpose exactly; the proper-rotation minimum of a non-planar chain is far from 0
    assert got[0, 0] > 0.1 and abs(got[0, 0] - ref_rmsd_matrix(a, b)[0, 0]) <= 1e-9


@pytest.mark.parametrize("wmode", ["none", "third"])
def test_chunking_is_bit_identical(wmode):
    from str2str_amd import ops

    rng = np.random.default_rng(11)
    L = 80
    base = random_walk(rng, L)
    w = _dev(make_weights(rng, L, wmode))
    a = _dev(make_ensemble(rng, 100, L, base)[0])
    b = _dev(make_ensemble(rng, 24, L, base, first_kind=2)[0])
    for x, y, n_b in ((a, None, 100), (a, b, 24)):
        whole = ops.ca_rmsd_matrix(x, y, w)
        for max_pairs in (n_b, 1000):
            assert torch.equal(ops.ca_rmsd_matrix(x, y, w, max_pairs=max_pairs), whole), (n_b, max_pairs)


@pytest.mark.parametrize("wmode", ["none", "third", "two"])
@pytest.mark.parametrize("L", LENGTHS)
def test_superpose_transform(L, wmode):
    from str2str_amd import ops

    rng = np.random.default_rng(2000 + L)
    base = random_walk(rng, L)
    w = make_weights(rng, L, wmode)
    mobile, _ = make_ensemble(rng, 24, L, base)            # includes the mirror image and the collinear chain
    target = np.asarray(base @ random_rotation(rng).T + rng.uniform(-50, 50, size=3), dtype=np.float32)
    rmsd, xform = ops.ca_superpose(_dev(mobile), _dev(target), _dev(w))
    rmsd, xform = rmsd.cpu().numpy(), xform.cpu().numpy()
    rot, trans = xform[:, :9].reshape(-1, 3, 3), xform[:, 9:]
    ortho = float(np.abs(np.swapaxes(rot, 1, 2) @ rot - np.eye(3)).max())
    det = float(np.abs(np.linalg.det(rot) - 1.0).max())
    msd_ref, s_raw, _ = ref_msd_matrix(mobile, target[None], w)
    msd_ref, bound = np.maximum(msd_ref[:, 0], 0.0), 8.0 * U64 * s_raw[:, 0]
    ww = np.ones(L) if w is None else w.astype(np.float64)
    moved = np.einsum("rij,rlj->rli", rot, mobile.astype(np.float64)) + trans[:, None, :]
    msd_x = (ww * ((moved - target.astype(np.float64)[None]) ** 2).sum(-1)).sum(-1) / ww.sum()
    if L == 1:
        msd_ref = np.zeros_like(msd_ref)
    print(f"superpose L={L} w={wmode}: |R^T R - I| = {ortho:.3e}  |det - 1| = {det:.3e}  msd(xform) err / bound = "
          f"{float((np.abs(msd_x - msd_ref) / bound).max()):.3f}  rmsd err = {float(np.abs(rmsd - np.sqrt(msd_ref)).max()):.3e}")
    record_margin("ensemble_rmsd_superpose_orthogonality", max(ortho, det), 2.0 ** -44)
    record_margin("ensemble_rmsd_superpose_msd_of_xform_over_bound", float((np.abs(msd_x - msd_ref) / bound).max()), 1.0)
    assert ortho <= 2.0 ** -44 and det <= 2.0 ** -44
    assert (np.abs(msd_x - msd_ref) <= bound).all()
    assert (np.abs(rmsd * rmsd - msd_ref) <= bound).all() and np.abs(rmsd - np.sqrt(msd_ref)).max() <= 1e-4


@pytest.mark.parametrize("M", [35, 37 * 12])
def test_apply_xform_is_the_rounded_float64_application(M):
    from str2str_amd import ops

    rng = np.random.default_rng(5)
    R = 17
    pts = (rng.normal(size=(R, M, 3)) * 30.0).astype(np.float32)
    xform = np.concatenate([np.stack([random_rotation(rng) for _ in range(R)]).reshape(R, 9), rng.uniform(-50, 50, size=(R, 3))], axis=1)
    got = ops.apply_xform(_dev(pts), _dev(xform)).cpu().numpy()
    want = np.einsum("rij,rmj->rmi", xform[:, :9].reshape(R, 3, 3), pts.astype(np.float64)) + xform[:, None, 9:]
    want32 = want.astype(np.float32)
    assert got.dtype == np.float32 and got.shape == pts.shape
    ulps = np.abs(got.astype(np.float64) - want32.astype(np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)
    record_margin("ensemble_rmsd_apply_xform_ulp", float(ulps.max()), 1.0)
    assert ulps.max() <= 1.0


def test_diversity_and_coverage_metrics():
    from str2str_amd.metrics import metrics

    rng = np.random.default_rng(21)
    L = 35
    base = random_walk(rng, L)
    ref, _ = make_ensemble(rng, 1000, L, base)
    pred, _ = make_ensemble(rng, 100, L, base, first_kind=1)
    one = pred[:1]
    full = ref_rmsd_matrix(pred, pred)
    div = metrics.diversity_rmsd({"target": ref[:17], "pred": pred, "one": one})
    assert div["pred"] == np.around(full[np.triu_indices(100, 1)].mean(), decimals=4) and div["one"] == 0.0
    assert div["target"] == np.around(ref_rmsd_matrix(ref[:17], ref[:17])[np.triu_indices(17, 1)].mean(), decimals=4)
    got = metrics.pairwise_rmsd(pred, ref[:24])
    check_matrix("pairwise_rmsd 100x24", got, pred, ref[:24], None)

    cross = ref_rmsd_matrix(pred, ref)                     # [100, 1000]
    for chunk in (None, 5000):
        per_ref, per_sample = metrics._coverage_extrema(metrics.RMSD, _dev(pred), _dev(ref), chunk_pairs=chunk)
        assert np.abs(per_ref.cpu().numpy() - cross.min(0)).max() <= 1e-4 and np.abs(per_sample.cpu().numpy() - cross.min(1)).max() <= 1e-4
        recall, precision = metrics.coverage_rmsd({"target": ref, "pred": pred}, chunk_pairs=chunk)
        assert recall == {"pred": np.around(cross.min(0).mean(), decimals=4), "target": 0.0}
        assert precision == {"pred": np.around(cross.min(1).mean(), decimals=4), "target": 0.0}


def test_rmsf():
    from str2str_amd.metrics import metrics

    rng = np.random.default_rng(31)
    L, R = 50, 2000
    base = random_walk(rng, L)
    # rigid motions of one structure: no fluctuation
    rigid = np.asarray([base @ random_rotation(rng).T + rng.uniform(-50, 50, size=3) for _ in range(64)], dtype=np.float32)
    f = metrics.rmsf(rigid)
    record_margin("ensemble_rmsd_rmsf_of_rigid_motions", float(f.max()), 1e-4)
    assert f.shape == (L,) and f.dtype == np.float64 and f.max() <= 1e-4
    # per-residue Gaussian noise, rigidly moved: against the float64 CPU pipeline (SVD Kabsch, same target)
    sigma = rng.uniform(0.1, 2.0, size=L)
    noisy = np.asarray([(base + rng.normal(size=(L, 3)) * sigma[:, None]) @ random_rotation(rng).T + rng.uniform(-50, 50, size=3)
                        for _ in range(R)], dtype=np.float32)
    target = base.astype(np.float32)
    w = make_weights(rng, L, "third")
    for ww in (None, w):
        rot, trans = ref_superpose(noisy, target, ww)
        y = np.einsum("rij,rlj->rli", rot, noisy.astype(np.float64)) + trans[:, None, :]
        want = np.sqrt(((y - y.mean(0)) ** 2).sum(-1).mean(0))
        got = metrics.rmsf(noisy, target=target, weights=ww)
        record_margin("ensemble_rmsd_rmsf_vs_float64_pipeline", float(np.abs(got - want).max()), 1e-6)
        assert np.abs(got - want).max() <= 1e-6, float(np.abs(got - want).max())
    aligned, rmsd = metrics.superpose(noisy[:24], target)
    assert aligned.dtype == np.float32 and aligned.shape == (24, L, 3)
    assert np.abs(rmsd - ref_rmsd_matrix(noisy[:24], target[None])[:, 0]).max() <= 1e-9
    assert np.abs(np.sqrt(((aligned.astype(np.float64) - target) ** 2).sum(-1).mean(-1)) - rmsd).max() <= 1e-4


@pytest.mark.parametrize("family", ["rmsd", "tm", "lddt"])
def test_eval_extra_metric_columns(tmp_path, family):
    import glob

    from str2str_amd.common.pdb_utils import extract_backbone_coords
    from str2str_amd.metrics import metrics

    entry = load_eval_entry(f"s2s_eval_entry_{family}")
    target_dir = os.path.join(GOLDEN, "pdb")
    template = os.path.join(target_dir, "CLN025.pdb")
    tgt = extract_backbone_coords(template)
    rng = np.random.default_rng(3)
    coords = tgt[0][None] + rng.normal(size=(6,) + tgt.shape[1:]) * 0.7
    five = ["val_clash", "val_bond", "js_pwd", "js_rg", "js_tica"]
    extra = [f"div_{family}", f"{family}_recall", f"{family}_precision"]
    for sub, names in (("plain", None), ("extra", extra)):
        pred_dir = tmp_path / sub / "samples" / "all"
        pred_dir.mkdir(parents=True)
        write_models(str(pred_dir / "CLN025.pdb"), template, coords)
        entry.evaluate_prediction(str(pred_dir), target_dir, tag="t", extra_metrics=names)
        files = glob.glob(str(tmp_path / sub / "metrics_t_*.csv"))
        assert len(files) == 1
        rows = [ln.rstrip("\n").split("\t") for ln in open(files[0])]
        assert rows[0] == [""] + five + (names or []) and [r[0] for r in rows[1:]] == ["CLN025", "mean"]
        if names:
            ca = {"target": tgt, "pred": extract_backbone_coords(str(pred_dir / "CLN025.pdb"))}
            assert ca["pred"].shape == (6,) + tgt.shape[1:]
            recall, precision = getattr(metrics, f"coverage_{family}")(ca)
            want = [getattr(metrics, f"diversity_{family}")(ca)["pred"], recall["pred"], precision["pred"]]
            # (an RMSD diversity is positive; a TM-score or lDDT diversity lies strictly inside (0, 1))
            assert [float(v) for v in rows[1][6:]] == [float(v) for v in want] and (want[0] > 0.0 if family == "rmsd" else 0.0 < want[0] < 1.0)


def test_wrong_out_is_rejected_and_eval_computes_every_family_once(tmp_path, monkeypatch):
    """``ca_rmsd_matrix`` checks a caller's ``out`` like the TM and lDDT wrappers; one ``evaluate_prediction`` with every extra column
    computes each coverage pair and the backbone violations once per target, and writes the row the public functions give."""
    import glob

    from str2str_amd import ops
    from str2str_amd.common.pdb_utils import extract_backbone_atoms, extract_backbone_coords
    from str2str_amd.metrics import metrics

    entry = load_eval_entry("s2s_eval_entry_once")
    target_dir = os.path.join(GOLDEN, "pdb")
    template = os.path.join(target_dir, "CLN025.pdb")
    tgt = extract_backbone_coords(template)
    rng = np.random.default_rng(3)
    coords = tgt[0][None] + rng.normal(size=(6,) + tgt.shape[1:]) * 0.7
    a = _dev(coords.astype(np.float32))
    for out in (torch.empty(7, 6, dtype=torch.float64, device="cuda"), torch.empty(6, 6, dtype=torch.float32, device="cuda")):
        with pytest.raises(ops.HipLibraryError, match="out"):
            ops.ca_rmsd_matrix(a, out=out)
    out = torch.empty(6, 6, dtype=torch.float64, device="cuda")
    assert ops.ca_rmsd_matrix(a, out=out) is out and torch.equal(out, ops.ca_rmsd_matrix(a))

    calls = {}

    def counted(module, name):
        fn = getattr(module, name)

        def passes_through(*args, **kwargs):
            calls[name] = calls.get(name, 0) + 1
            return fn(*args, **kwargs)

        monkeypatch.setattr(module, name, passes_through)

    for name in ("coverage_rmsd", "coverage_tm", "coverage_lddt"):
        counted(metrics, name)
    counted(ops, "backbone_violations")
    pred_dir = tmp_path / "samples" / "all"
    pred_dir.mkdir(parents=True)
    pred_file = str(pred_dir / "CLN025.pdb")
    write_models(pred_file, template, coords)
    entry.evaluate_prediction(str(pred_dir), target_dir, tag="t", extra_metrics=list(entry.EXTRA_METRICS))
    assert calls == {"coverage_rmsd": 1, "coverage_tm": 1, "coverage_lddt": 1, "backbone_violations": 1}
    monkeypatch.undo()

    files = glob.glob(str(tmp_path / "metrics_t_*.csv"))
    assert len(files) == 1
    rows = [ln.rstrip("\n").split("\t") for ln in open(files[0])]
    assert rows[0][6:] == list(entry.EXTRA_METRICS) and [r[0] for r in rows[1:]] == ["CLN025", "mean"]
    atoms, aatype, residue_index = extract_backbone_atoms(pred_file)
    bond, clash = metrics.backbone_validity({"pred": atoms}, aatype, residue_index)
    want = [bond["pred"], clash["pred"], metrics.violation_rate({"pred": atoms}, aatype, residue_index)["pred"]]
    ca = {"target": tgt, "pred": extract_backbone_coords(pred_file)}
    for family in ("rmsd", "tm", "lddt"):
        recall, precision = getattr(metrics, f"coverage_{family}")(ca)
        want += [getattr(metrics, f"diversity_{family}")(ca)["pred"], recall["pred"], precision["pred"]]
    assert [float(v) for v in rows[1][6:]] == [float(v) for v in want]
