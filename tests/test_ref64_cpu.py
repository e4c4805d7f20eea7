"""The float64 references of tests/ref64.py pinned to the reference-generated fixtures, and the distance of the float32 chain
(oracle/) from them on the very inputs tests/test_geometry_parity.py feeds the HIP kernels.  CPU only.

Bounds here are float32 rounding budgets of the fixtures (which are float32 results of a float32 chain): eps32 = 1.19e-7 per
operation on the output's scale, times the handful of operations the value passes through."""
import numpy as np
import pytest
import torch

import ref64
import score_cases as sc
from conftest import T, golden, record_margin

EPS32 = 2.0 ** -23


def check(name, achieved, bound):
    record_margin(name, achieved, bound)
    assert achieved < bound, (name, achieved, bound)


@pytest.fixture(scope="module")
def diffuser(tmp_path_factory):
    from str2str_amd.factory import build_diffuser

    return build_diffuser(str(tmp_path_factory.mktemp("so3cache")))


@pytest.mark.parametrize("branch", ["ode", "sde"])
def test_reverse_step64_matches_the_reference_fixture(diffuser, branch):
    """score_reverse.npz: the reference's own reverse step from its own scores (4 x 12 residues, diffuse_mask = mask, centre
    over all residues, noise scale 1).  Its SDE frames were drawn after torch.manual_seed(99): float64 normals, rotation noise
    first.  Rotations as matrices of the normalised quaternions: 25 float32 operations of the chain on entries <= 1;
    translations: 3 roundings at the fixture's 17 to 20 A."""
    g = golden("score_reverse.npz")
    z_rot = z_trans = None
    if branch == "sde":
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(99)
            z_rot = torch.randn(g["rot_score"].shape, dtype=torch.float64)
            z_trans = torch.randn(g["trans_score"].shape, dtype=torch.float64)
    R, x = ref64.reverse_step64(T(g["xt"]), T(g["rot_score"]), T(g["trans_score"]), T(g["t"]), float(g["dt"]), T(g["mask"]), T(g["mask"]),
                                1, 1.0, branch == "ode", z_rot, z_trans, diffuser)
    nxt = T(g["next7" if branch == "ode" else "next7_sde"])
    scale = float(nxt[..., 4:].abs().max())
    check(f"reverse_step64 vs fixture [{branch}]: rotation matrix entries", float((ref64.quat_rot64(nxt[..., :4]) - R).abs().max()), 25 * EPS32)
    check(f"reverse_step64 vs fixture [{branch}]: translations (A, scale {scale:.0f})", float((nxt[..., 4:].double() - x).abs().max()),
          3 * EPS32 * scale)


def test_compose_update64_matches_the_reference_fixture():
    g = golden("prims.npz")
    ref = ref64.compose_update64(np.concatenate([g["q"], g["t"]], -1), g["upd"], g["msk"][:, 0])
    scale = max(1.0, float(np.abs(g["comp7"]).max()))
    check("compose_update64 vs fixture / output scale", float((T(g["comp7"]).double() - ref).abs().max()) / scale, 2 * EPS32)


def test_backbone64_matches_the_reference_fixture():
    g = golden("backbone.npz")
    a37, m37, bb5 = ref64.backbone64(g["rigids7"].reshape(-1, 7), g["psi"].reshape(-1, 2), g["aatype"].reshape(-1))
    scale = max(1.0, float(np.abs(g["atom37"]).max()))
    check("backbone64 atom37 vs fixture / coordinate scale", float((T(g["atom37"]).reshape(-1, 37, 3).double() - a37).abs().max()) / scale, 2 * EPS32)
    check("backbone64 atom14 vs fixture / coordinate scale",
          float((T(g["atom14"]).reshape(-1, 14, 3)[:, :5].double() - bb5).abs().max()) / scale, 2 * EPS32)
    assert np.array_equal(m37.numpy(), g["mask37"].reshape(-1, 37))
    # no residue types given: alanine everywhere
    a37_none, _, _ = ref64.backbone64(g["rigids7"].reshape(-1, 7), g["psi"].reshape(-1, 2), None)
    ala = g["aatype"].reshape(-1) == 0
    assert ala.any() and torch.equal(a37_none[ala], a37[ala])


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_js_channels_np_equals_the_reference_fixture(tag):
    """Exactly: histogram counts are integers and the Jensen-Shannon distance is the same scipy call.  A numpy that bins
    differently fails here and is not blamed on the kernel."""
    g = golden("metrics.npz")
    ch = ref64.js_channels_np(g[f"{tag}_target"], g[f"{tag}_pred"])
    assert np.array_equal(ch, g[f"{tag}_js_pwd_channels"]), float(np.abs(ch - g[f"{tag}_js_pwd_channels"]).max())


def test_sample_stats_np_on_the_planted_walk():
    """The planted pairs are what they claim in numpy's float32 distance: exactly 3.0 A (no clash under the strict <) and one
    ulp less (a clash); Rg of the float64 formula against the reference fixture's float32-mean value."""
    ca = ref64.walk_ensemble(5, 63)
    d = ref64.pairwise_np(ca, 1)
    r_, c_ = np.triu_indices(63, k=1)
    exact, below = d[:, (r_ == 0) & (c_ == 62)][:, 0], d[:, (r_ == 1) & (c_ == 61)][:, 0]
    assert (exact == np.float32(3.0)).all() and (below == np.nextafter(np.float32(3.0), np.float32(0))).all()
    n0, adj, _ = ref64.sample_stats_np(ca, 3.0, 0)
    assert (n0 == (d < np.float32(3.0)).sum(-1)).all() and (n0 >= 1).all() and adj.dtype == np.float32
    assert (ref64.sample_stats_np(ca, np.nextafter(np.float32(3.0), np.float32(4)), 0)[0] >= n0 + 1).all()
    two = ref64.walk_ensemble(5, 2)
    assert list(ref64.sample_stats_np(two, 3.0, 0)[0]) == [0, 1, 0, 1, 0] and list(ref64.sample_stats_np(two, 3.0, 3)[0]) == [0] * 5
    g = golden("metrics.npz")
    rg = ref64.sample_stats_np(g["b_pred"])[2]
    check("sample_stats_np Rg vs fixture (float32 mean in the fixture), relative", float(np.abs(rg / g["b_rg_pred"] - 1).max()), EPS32)


def test_prior_rotation64_is_the_oracle_sample(diffuser):
    """oracle SO3.sample (np.interp on the sigma bin's cdf row, float32 axis times angle) as a matrix."""
    from oracle import diffuser as OD
    from oracle import geometry as OG

    so3 = OD.SO3()
    t = torch.tensor([0.05, 1.0, 0.05])
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(3)
        rv = so3.sample(t, (3, 40, 3))
        torch.manual_seed(3)
        z, u = torch.randn(3, 40, 3), torch.rand(3, 40)
    idx = [int(so3.t_to_idx(x)) for x in t]
    rows = np.stack([so3.cdf_row(i) for i in sorted(set(idx))])
    R = ref64.prior_rotation64(z, u, rows, [sorted(set(idx)).index(i) for i in idx], so3.discrete_omega)
    check("prior_rotation64 vs the oracle's draw: rotation matrix entries", float((OG.axis_angle_to_matrix(rv).double() - R).abs().max()), 10 * EPS32)


def test_all_masked_sample_keeps_its_frame_in_float64(diffuser):
    case = ref64.se3_case("ode-c2", 65, diffuser)
    case["mask"][1] = 0.0
    case["diffuse_mask"][1] = 0.0
    R, x = ref64.se3_ref64(case, diffuser)
    assert torch.isfinite(R).all() and torch.isfinite(x).all()
    assert torch.equal(x[1], case["xt7"][1, :, 4:].double()) and torch.equal(R[1], ref64.quat_rot64(case["xt7"][1, :, :4]))


@pytest.mark.parametrize("family", sorted(ref64.SE3_FAMILIES))
def test_float32_chain_distance_from_float64(diffuser, family):
    """How far the reference's float32 chain (oracle.diffuser.FrameDiffuser.reverse) sits from reverse_step64 on every input
    of the GPU test, per case family, over all N: the figures that test's tolerances are three times.  Centre mode 2 and a
    per-sample dt have no equivalent in one call of the chain, so it runs one sample at a time on the sample's unpadded
    prefix with its own dt.  No case and no planted frame is left out: a frame at exactly pi is not among the planted ones
    (pi - 1e-4 is), so nothing had to be dropped.  The assertions only keep the band meaningful: a rotation error of a few
    tens of eps32 (the chain's matrix -> quaternion -> axis-angle -> quaternion -> matrix round trips, twice per step) and a
    translation error of a few eps32 of the sample's scale."""
    e_rot, e_trans = ref64.se3_family_distance(family, diffuser)
    record_margin(f"se3 float32 chain vs float64 [{family}]: e_rot (matrix entries)", e_rot, 50 * EPS32)
    record_margin(f"se3 float32 chain vs float64 [{family}]: e_trans / sample scale", e_trans, 4 * EPS32)
    assert 0 < e_rot < 50 * EPS32 and 0 < e_trans < 4 * EPS32, (e_rot, e_trans)
    # the planted inputs are what they claim
    case = ref64.se3_case(family, 257, diffuser)
    q = case["xt7"][..., :4]
    assert torch.equal(q[:, 0], torch.tensor([1.0, 0, 0, 0]).expand(3, 4)) and (q[:, 1, 0] < 0).all() and (q[:, 256 - 1, 0] < 0).all()
    ang = 2 * torch.atan2(q[:, 2:4, 1:].double().norm(dim=-1), q[:, 2:4, 0].double())
    assert (ang[:, 0] - (np.pi - 1e-4)).abs().max() < 1e-6 and (ang[:, 1] - 1e-7).abs().max() < 1e-9
    assert (q.double().norm(dim=-1) - 1).abs().max() < 2 * EPS32


# ----------------------------------------------------------------------------------------------- SE(3) score
def _fixture_sigma(diffuser, t):
    return diffuser.step_params(T(t).float())[:, 0].double().numpy()


def test_igso3_series64_matches_the_float64_anchors(diffuser):
    """score64.npz holds the reference's own series functions evaluated in float64 on its float32 rotation vectors
    (so3_score.npz: 5 x 48 vectors up to pi at five t, given directly; score_reverse.npz: the vectors its chain produced).
    rot_score_of_rotvec64 is the same formula on the same vectors, on every residue of either branch: a few float64 roundings
    of the 1000-term sums, relative to the largest score of the sample."""
    g, a = golden("so3_score.npz"), golden("score64.npz")
    sig = _fixture_sigma(diffuser, g["t"])
    assert np.array_equal(sig.astype(np.float32), g["discrete_sigma"][g["sigma_idx"]])
    s = ref64.rot_score_of_rotvec64(T(g["vec"]), sig).numpy()
    scale = np.abs(a["grid_score64"]).max(axis=(1, 2), keepdims=True)
    check("rot_score_of_rotvec64 vs float64 anchors [omega grid] / sample scale", float(np.abs((s - a["grid_score64"]) / scale).max()), 1e-10)
    sr = golden("score_reverse.npz")
    s = ref64.rot_score_of_rotvec64(T(a["sr_rotvec"]), _fixture_sigma(diffuser, sr["t"])).numpy() * sr["mask"][..., None]
    scale = np.abs(a["sr_score64"]).max(axis=(1, 2), keepdims=True)
    check("rot_score_of_rotvec64 vs float64 anchors [score_reverse] / sample scale", float(np.abs((s - a["sr_score64"]) / scale).max()), 1e-10)


def test_score64_matches_the_reference_fixture_on_the_principal_branch(diffuser):
    """score_reverse.npz: the reference's own scores of 4 x 12 frames.  Where its float32 chain takes the principal branch,
    score64 (exact relative rotation of the float32 quaternions) sits within 2e-6 rad of rotation vector, through the score's
    Jacobian, of the float64 anchor on the chain's float32 vector; and the oracle's float32 value within what the anchors
    grant any float32 evaluation (2 spread32 + alg32 + 4e-5 |s|) on top of that.  Translations: the float32 formula's
    roundings, 4 eps32 of (|0.1 x_t| + |0.1 x_0|) / cond_var."""
    from oracle import diffuser as OD
    from oracle.geometry import Frames

    g, a = golden("score_reverse.npz"), golden("score64.npz")
    t = T(g["t"]).float()
    p8 = diffuser.step_params(t)
    rot, trans = ref64.score64(T(g["x0"]), T(g["xt"]), t, T(g["mask"]), diffuser)
    w = ref64.score_chain32(T(g["x0"]), T(g["xt"]), p8, T(g["mask"]))[2]
    sel = ((w >= 0) & (T(g["mask"]) > 0)).numpy()
    assert 8 <= sel.sum() < sel.size, "the fixture holds both branches"
    theta = ref64.relative_rotvec64(T(g["x0"])[..., :4], T(g["xt"])[..., :4]).norm(dim=-1).numpy()
    budget = 2e-6 * sc.score_jacobian(theta, p8[:, 0].double().numpy()[:, None])
    d_anchor = np.abs(rot.numpy() - a["sr_score64"]).max(-1)
    check("score64 vs float64 anchors [score_reverse, principal]: max error / (2e-6 rad x Jacobian)", float((d_anchor / budget)[sel].max()), 1.0)
    rs, ts = OD.FrameDiffuser().score(Frames.from_tensor_7(T(g["x0"])), Frames.from_tensor_7(T(g["xt"])), t, T(g["mask"]))
    grant = budget + 2 * a["sr_spread32"] + a["sr_alg32"] + 4e-5 * np.abs(a["sr_score64"]).max(-1)
    check("score64 vs the oracle's float32 score [score_reverse, principal]: max error / granted", float((np.abs(rs.numpy() - rot.numpy()).max(-1) / grant)[sel].max()), 1.0)
    cs = 0.1
    scale = float(((cs * T(g["xt"])[..., 4:].abs() + cs * T(g["x0"])[..., 4:].abs()).double() / p8[:, 3].double().reshape(-1, 1, 1)).max())
    check(f"score64 vs the oracle's translation score (scale {scale:.0f})", float((ts.double() - trans).abs().max()), 4 * EPS32 * scale)
    check(f"score64 vs the fixture's translation score (scale {scale:.0f})", float((T(g["trans_score"]) - trans).abs().max()), 4 * EPS32 * scale)


def test_score_table_properties(diffuser):
    """What tests/score_cases.py claims about its score table: planted angles and orientation classes are what they say, every
    band from theta = 1e-6 up holds at least a quarter of its residues on either branch of the float32 chain, masks of three
    kinds with finite garbage underneath, translations within +-300 A, and every principal D32 is explained by 2e-6 rad of
    rotation vector through the score's Jacobian plus the float64 rounding of the series (score_cases.score_conditioning)."""
    for N in sc.SCORE_N:
        c = sc.score_case(N, diffuser)
        x0, xt, m = c["x0"], c["xt"], c["mask"] > 0
        assert torch.isfinite(x0).all() and torch.isfinite(xt).all()
        assert float((xt[..., :4].double().norm(dim=-1) - 1).abs()[m].max()) < 2 * EPS32
        assert float((x0[..., :4].double().norm(dim=-1) - 1).abs()[m].max()) < 2 * EPS32
        assert float(xt[..., 4:][m].abs().max()) <= 300 and float(x0[..., 4:][m].abs().max()) <= 300
        theta = ref64.relative_rotvec64(x0[..., :4], xt[..., :4]).norm(dim=-1)
        want = torch.as_tensor(sc.SCORE_THETA, dtype=torch.float64)[c["band"]]
        assert float((theta - want).abs()[m].max()) < 4 * EPS32
        zero = m & (c["band"] == 0)
        assert torch.equal(x0[..., :4][zero], xt[..., :4][zero]) and (theta[zero] == 0).all()
        assert (sc.score_ref64(N, diffuser)[0][zero] == 0).all()
        q = xt[..., :4]
        for k, name in enumerate(sc.SCORE_CLASSES):
            s = m & (c["cls"] == k)
            if not s.any():
                continue
            if "~" in name:
                i, j = sc._COMP[name[0]], sc._COMP[name[-1]]
                top = q[s].abs().topk(2, dim=-1).indices.sort(dim=-1).values
                assert (top == torch.tensor(sorted((i, j)))).all()
                assert (q[s][:, i] * q[s][:, j] < 0).all() and float((q[s][:, i].abs() - q[s][:, j].abs()).abs().max()) < 1.1e-3
            else:
                assert (q[s].abs().argmax(dim=-1) == sc._COMP[name[0]]).all() and ((q[s][:, 0] > 0) == (name[1] == "+")).all()
        if N >= 65:
            assert m[0].all() and not m[1].all() and m[1, -1] + m[1, 0] >= 0 and m[2, :N - N // 4].all() and not m[2, N - N // 4:].any()
            garbage = xt[..., :4][~m].double().norm(dim=-1)
            assert float(garbage.min()) >= 0.49 and float(garbage.max()) <= 2.01 and float((garbage - 1).abs().min()) > 1e-4 or N < 257
        if N >= 257:
            for k in range(1, len(sc.SCORE_THETA)):
                in_band = m & (c["band"] == k)
                share = float((in_band & c["wrapped"]).sum()) / float(in_band.sum())
                assert 0.25 <= share <= 0.75, (N, sc.SCORE_BAND[k], share)
    D, Dt = sc.score_d32(diffuser)
    J, E = sc.score_conditioning(diffuser)
    ratio = D / (2e-6 * J + 2 * E)
    print("D32 per (band, sample):\n", D.numpy(), "\nD32 / (2e-6 J + 2 E64):\n", ratio.numpy(), "\ntranslation D32 per sample:", Dt.numpy())
    for k in range(len(sc.SCORE_THETA)):
        for b in range(sc.SCORE_B):
            record_margin(f"score float32 chain vs float64 [{sc.family_label(k, b)}]: D32 / (2e-6 rad x Jacobian + float64 series rounding)",
                          float(ratio[k, b]), 1.0)
            record_margin(f"score float32 chain vs float64 [{sc.family_label(k, b)}]: D32", float(D[k, b]), float(2e-6 * J[k, b] + 2 * E[k, b]))
    assert (D > 0).all() and (ratio < 1).all(), ratio
    assert (Dt > 0).all()


def test_emulated_score_contract_meets_the_bound(diffuser):
    """The kernel's contract on the CPU (the float32 chain with the product quaternion's sign standardised, the series in
    float64, v = 0 where q_0 = +-q_t) stays inside 3 x D32 on the residues of either branch at every N; masked residues and
    theta = 0 are exactly 0, also with x_0's quaternion negated.  The chain itself is not 0 at theta = 0 (its |q|^2 division)."""
    D, Dt = sc.score_d32(diffuser)
    for N in sc.SCORE_N:
        c = sc.score_case(N, diffuser)
        rot, trans, _ = ref64.score_chain32(c["x0"], c["xt"], c["p8"], c["mask"], standardise=True)
        assert torch.isfinite(rot).all() and torch.isfinite(trans).all()
        for which in ("principal", "wrapped"):
            e = sc.score_family_errors(rot, N, diffuser, which)
            ok = ~torch.isnan(e)
            check(f"emulated score contract vs float64, {which} residues: max error / (3 x D32)", float((e / (3 * D))[ok].max()) if ok.any() else 0.0, 1.0)
        assert (sc.trans_sample_errors(trans, N, diffuser) <= 3 * Dt).all()
        assert (rot[c["mask"] == 0] == 0).all() and (trans[c["mask"] == 0] == 0).all()
        zero = (c["band"] == 0) & (c["mask"] > 0)
        flipped = c["x0"] * torch.tensor([-1.0, -1, -1, -1, 1, 1, 1])
        assert (rot[zero] == 0).all() and (ref64.score_chain32(flipped, c["xt"], c["p8"], c["mask"], standardise=True)[0][zero] == 0).all()
        if N >= 257:
            assert (ref64.score_chain32(c["x0"], c["xt"], c["p8"], c["mask"])[0][zero] != 0).any()


def _mistaken_score(kind, c, diffuser):
    """(rot, trans) [B, N, 3] float64 of a score with one planted mistake."""
    x0, xt, m = ref64._f64(c["x0"]), ref64._f64(c["xt"]), ref64._f64(c["mask"])[..., None]
    p8 = c["p8"].double()
    sig = p8[:, 0]
    conj = torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=torch.float64)
    v = ref64.relative_rotvec64(x0[..., :4], xt[..., :4])
    trans = ref64.trans_score64(x0[..., 4:], xt[..., 4:], p8, 0.1)
    if kind == "x0 and xt swapped":
        return ref64.score64(c["xt"], c["x0"], c["t"], c["mask"], diffuser)
    if kind == "Rt R0^T for R0^T Rt":
        v = ref64.relative_rotvec64(xt[..., :4] * conj, x0[..., :4] * conj)
    elif kind == "sigma of the next sample":
        sig = sig.roll(-1)
    elif kind == "sigma bin k + 1":
        sd = diffuser.rot_diffuser
        idx = (sd.t_to_idx(c["t"]) + 1).clamp(max=len(sd.discrete_sigma) - 1)
        sig = torch.as_tensor(np.asarray(sd.discrete_sigma)[idx.numpy()]).double()
    elif kind == "mask not applied":
        m = torch.ones_like(m)
    elif kind == "e_half dropped":
        q8 = p8.clone()
        q8[:, 2] = 1.0
        trans = ref64.trans_score64(x0[..., 4:], xt[..., 4:], q8, 0.1)
    elif kind == "product sign not standardised":
        rot, trans, _ = ref64.score_chain32(c["x0"], c["xt"], c["p8"], c["mask"], standardise=False)
        return rot, trans
    return ref64.rot_score_of_rotvec64(v, sig) * m, trans * m


@pytest.mark.parametrize("kind", ["x0 and xt swapped", "Rt R0^T for R0^T Rt", "sigma of the next sample", "sigma bin k + 1", "mask not applied",
                                  "e_half dropped", "product sign not standardised"])
def test_planted_score_mistakes_leave_the_bound(diffuser, kind):
    """Each mistake, made in float64 on the N = 257 case (the un-standardised sign: in the float32 chain), fails the check the
    GPU test makes: some family beyond 3 x D32 (rotation), some sample beyond 3 x the translation D32, or a masked residue that
    is not exactly 0.  The un-standardised sign fails on wrapped residues only, in every band up to theta = 0.1."""
    N = 257
    D, Dt = sc.score_d32(diffuser)
    c = sc.score_case(N, diffuser)
    rot, trans = _mistaken_score(kind, c, diffuser)
    e_p, e_w = (sc.score_family_errors(rot, N, diffuser, which) / (3 * D) for which in ("principal", "wrapped"))
    e_t = sc.trans_sample_errors(trans, N, diffuser) / (3 * Dt)
    masked = c["mask"] == 0
    worst_rot = float(torch.nan_to_num(torch.maximum(e_p, e_w), nan=0.0).max())
    print(f"{kind}: rotation {worst_rot:.3g} x bound, translation {float(e_t.max()):.3g} x bound")
    if kind == "mask not applied":
        assert not (rot[masked] == 0).all() and not (trans[masked] == 0).all()
    elif kind == "e_half dropped":
        assert float(e_t.max()) > 10 and worst_rot <= 1
    elif kind == "product sign not standardised":
        assert float(torch.nan_to_num(e_p, nan=0.0).max()) <= 1 and float(e_t.max()) <= 1
        assert (e_w[:6] > 10).all(), e_w
    elif kind == "sigma bin k + 1":
        assert worst_rot > 10 and float(e_t.max()) <= 1
    else:
        assert worst_rot > 10
    if kind == "sigma of the next sample":
        assert (torch.nan_to_num(torch.maximum(e_p, e_w), nan=0.0).amax(0) > 10).all()     # every sample notices


# ----------------------------------------------------------------------------------------------- forward marginal, noising branch
def _oracle_forward_marginal(diffuser, seed, gt4, t, mask):
    """(frames of oracle.FrameDiffuser.forward_marginal after torch.manual_seed(seed), its draws, the arguments that describe
    them to forward_marginal64)."""
    from oracle import diffuser as OD
    from oracle.geometry import Frames

    od = OD.FrameDiffuser()
    B, N = gt4.shape[:2]
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        fm = od.forward_marginal(Frames.from_tensor_4x4(gt4), t, mask)
        torch.manual_seed(seed)
        z, u, zt = torch.randn(B, N, 3), torch.rand(B, N), torch.randn(B, N, 3)
    idx = [int(od.so3.t_to_idx(x)) for x in t]
    rows = sorted(set(idx))
    mb = od.r3.marginal_b_t(t)
    args = dict(rig0_4x4=gt4, z_axis=z, u=u, z_trans=zt, cdf_rows=np.stack([od.so3.cdf_row(i) for i in rows]),
                row_of_sample=[rows.index(i) for i in idx], omega_grid=od.so3.discrete_omega,
                params2=torch.stack([torch.exp(-0.5 * mb), torch.sqrt(1 - torch.exp(-mb))], -1), diffuse_mask=mask)
    return fm, args


def test_forward_marginal64_is_the_oracle_draw(diffuser):
    """oracle.FrameDiffuser.forward_marginal under the generator seeding of test_prior_rotation64_is_the_oracle_sample (axis
    normals, uniforms, then translation normals) on 3 x 40 random frames at t = (0.05, 1, 0.05) with a fifth frozen: the
    restatement on given noise (forward_marginal_chain32) returns its bits, and forward_marginal64 its frames within the
    reverse-step fixture's budget (25 float32 operations on the rotation, 3 roundings of the translation's scale).  Then
    forward_marginal.npz, the reference's own draw."""
    rng = np.random.default_rng(5)
    gt4 = torch.zeros(3, 40, 4, 4)
    gt4[..., :3, :3] = ref64.quat_rot64(ref64.unit_quats(rng, (3, 40))).float()
    gt4[..., :3, 3] = torch.as_tensor(rng.uniform(-50, 50, size=(3, 40, 3))).float()
    mask = torch.as_tensor((rng.uniform(size=(3, 40)) >= 0.2).astype(np.float64))
    g = golden("forward_marginal.npz")
    for name, seed, frames, t, m, want in (("seeded", 3, gt4, torch.tensor([0.05, 1.0, 0.05]), mask, None),
                                           ("fixture", int(g["seed_fm"]), T(g["gt4"]), float(g["t_delta"]) * torch.ones(3), T(g["mask"]), T(g["rigids_t"]))):
        fm, args = _oracle_forward_marginal(diffuser, seed, frames, t, m)
        assert torch.equal(ref64.forward_marginal_chain32(**args), fm)
        R, x = ref64.forward_marginal64(**args)
        for what, out in (("oracle", fm), ("fixture", want)):
            if out is None:
                continue
            scale = float(x.abs().max())
            check(f"forward_marginal64 vs the {what}'s draw [{name}]: rotation matrix entries", float((ref64.quat_rot64(out[..., :4]) - R).abs().max()), 25 * EPS32)
            check(f"forward_marginal64 vs the {what}'s draw [{name}]: translations (A, scale {scale:.0f})", float((out[..., 4:].double() - x).abs().max()),
                  3 * EPS32 * scale)
        frozen = m == 0
        assert frozen.any() and torch.equal(x[frozen], frames[..., :3, 3][frozen].double())


def test_forward_marginal_table_properties(diffuser):
    """The noising table: every branch of np.interp, every planted frame and every pi crossing occurs from N = 255 up, the
    crossings cross (the composed angle about the drawn axis lies on either side of pi), the 4 x 4 inputs are orthonormal to
    float32 rounding only, a fifth of the residues is frozen, and b = r / N does not line up with a workgroup of 256.  The
    float32 chain's distances (what the GPU bounds are three times) are recorded."""
    for N in sc.FM_N:
        c = sc.fm_case(N, diffuser)
        kinds = {k for _, _, k, _ in c["plants"]}
        R0 = c["rig0"][..., :3, :3].double()
        off = (R0 @ R0.transpose(-1, -2) - torch.eye(3, dtype=torch.float64)).abs().amax(dim=(-1, -2))
        assert 0 < float(off.max()) < 8 * EPS32
        if N >= 255:
            assert kinds == {"u", "pi"} | set(ref64.FRAME_PLANTS) and N % 256 != 0
            assert 0.1 < float((c["diffuse_mask"] == 0).float().mean()) < 0.3
            R64, _ = ref64.forward_marginal64(**sc.fm_args(c, diffuse_mask=None))
            ang = torch.acos(((R64.diagonal(dim1=-2, dim2=-1).sum(-1) - 1) / 2).clamp(-1, 1))
            pi_res = [(b, n, d) for b, n, k, d in c["plants"] if k == "pi"]
            got = torch.stack([ang[b, n] for b, n, _ in pi_res])
            want = torch.as_tensor([abs(d) for _, _, d in pi_res])
            assert {d for _, _, d in pi_res} == set(sc.PI_CROSS)
            assert float(((np.pi - got) - want).abs().max()) < 2e-6
        e_rot, e_trans = sc.fm_d32(N, diffuser)
        record_margin(f"forward marginal float32 chain vs float64 [N={N}]: e_rot (matrix entries)", e_rot, sc.FM_CAP / 3)
        record_margin(f"forward marginal float32 chain vs float64 [N={N}]: e_trans / sample scale", e_trans, sc.FM_CAP / 3)
        print(f"N={N}: chain e_rot {e_rot:.3e}, e_trans {e_trans:.3e}; bounds {sc.fm_bounds(N, diffuser)}")
        assert 0 < e_rot < 50 * EPS32 and 0 < e_trans < 4 * EPS32, (e_rot, e_trans)


def _mistaken_forward_marginal(kind, c):
    """Frames (R [B,N,3,3], x [B,N,3]) float64 of the noising branch with one planted mistake."""
    a = sc.fm_args(c)
    g = ref64._f64(c["rig0"])
    R0, x0 = ref64.matrix_rot64(g[..., :3, :3]), g[..., :3, 3]
    dm = ref64._f64(c["diffuse_mask"])[..., None]
    if kind == "the neighbour's CDF row":
        a["row_of_sample"] = tuple(1 - r for r in c["rows"])
    elif kind == "the blend reversed":
        a["diffuse_mask"] = 1 - c["diffuse_mask"]
    elif kind == "std and e_half swapped":
        a["params2"] = c["params2"].flip(-1)
    if kind == "R_draw R0 for R0 R_draw":
        Rd = ref64.prior_rotation64(c["z_axis"], c["u"], c["cdf"], c["rows"], c["omega"])
        R, x = ref64.forward_marginal64(**a)
        return torch.where(dm[..., None] > 0, Rd @ R0, R0), x
    if kind == "the lower knot off by one":
        cdf, om, u = c["cdf"].numpy(), c["omega"].double().numpy(), c["u"].double().numpy()
        ang = np.empty_like(u)
        for b, r in enumerate(c["rows"]):
            xp = cdf[r]
            j = np.clip(np.searchsorted(xp, u[b], side="right") - 1, 0, len(xp) - 2)
            lo = np.clip(j - 1, 0, len(xp) - 2)
            with np.errstate(divide="ignore", invalid="ignore"):   # (flat stretches of the row; np.where drops them)
                ang[b] = np.where(u[b] < xp[0], om[0], np.where(u[b] >= xp[-1], om[-1], (om[lo + 1] - om[lo]) / (xp[lo + 1] - xp[lo]) * (u[b] - xp[lo]) + om[lo]))
        z = ref64._f64(c["z_axis"])
        Rd = ref64.rotvec_exp64(z / z.norm(dim=-1, keepdim=True) * torch.as_tensor(ang)[..., None])
        _, x = ref64.forward_marginal64(**a)
        return torch.where(dm[..., None] > 0, R0 @ Rd, R0), x
    return ref64.forward_marginal64(**a)


@pytest.mark.parametrize("kind", ["R_draw R0 for R0 R_draw", "the neighbour's CDF row", "the lower knot off by one", "the blend reversed",
                                  "std and e_half swapped"])
def test_planted_forward_marginal_mistakes_leave_the_bound(diffuser, kind):
    """Each mistake, made in float64 on the N = 257 case, is at least ten times the bound of the GPU test away."""
    N = 257
    c = sc.fm_case(N, diffuser)
    R, x = _mistaken_forward_marginal(kind, c)
    R64, x64 = sc.fm_ref64(N, diffuser)
    b_rot, b_trans = sc.fm_bounds(N, diffuser)
    e = [ref64.rot_trans_error(R[b], x[b], R64[b], x64[b]) for b in range(sc.FM_B)]
    e_rot, e_trans = max(a for a, _ in e), max(b for _, b in e)
    print(f"{kind}: rotation {e_rot / b_rot:.3g} x bound, translation {e_trans / b_trans:.3g} x bound")
    if kind == "std and e_half swapped":
        assert e_trans > 10 * b_trans and e_rot == 0
    elif kind == "the blend reversed":
        assert e_trans > 10 * b_trans and e_rot > 10 * b_rot
    else:
        assert e_rot > 10 * b_rot and e_trans == 0
