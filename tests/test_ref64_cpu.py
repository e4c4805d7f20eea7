"""The float64 references of tests/ref64.py pinned to the reference-generated fixtures, and the distance of the float32 chain
(oracle/) from them on the very inputs tests/test_geometry_parity.py feeds the HIP kernels.  CPU only.

Bounds here are float32 rounding budgets of the fixtures (which are float32 results of a float32 chain): eps32 = 1.19e-7 per
operation on the output's scale, times the handful of operations the value passes through."""
import numpy as np
import pytest
import torch

import ref64
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
