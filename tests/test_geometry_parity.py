"""The HIP kernels that carry no matrix product -- the SE(3) step, the per-residue frame kernels, the forward-marginal prior and
the ensemble statistics -- against the float64 references of tests/ref64.py, through ``str2str_amd.ops``, at the shapes where
each kernel changes path (more than one workgroup, the strided residue loop, partial last workgroups, grid-stride loops).

Tolerances.  SE(3) step: three times the distance of the reference's own float32 chain (oracle/) from float64 on the same case
family, recomputed here (tests/test_ref64_cpu.py records it); the kernel is that chain with another libm.  Pure geometry
kernels: this project's 1e-6 of the output scale, tightened after the first MI355X run to a few float32 roundings
(EPS32 = 2^-23) so that every bound sits within about 5x of the achieved margin (profiles/parity_margins.json).  Integer and
float32-exact quantities (clash counts, distances, zero fills): equality.  The float64 statistics keep a worst-case
summation-order budget, which a deterministic kernel does not use up.
"""
import numpy as np
import pytest
import torch

import ref64
from conftest import record_margin

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS32 = 2.0 ** -23


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module")
def diffuser(tmp_path_factory):
    from str2str_amd.factory import build_diffuser

    return build_diffuser(str(tmp_path_factory.mktemp("so3cache")))


def check(name, achieved, bound):
    record_margin(name, achieved, bound)
    assert achieved < bound, (name, achieved, bound)


def _dev(x):
    return x.to(DEV).contiguous()


def _dt(case):
    return _dev(case["dt"]) if case["dt_kind"] == "vec" else float(case["dt"][0])


def _noise(case):
    return (None, None) if case["probability_flow"] else (_dev(case["z_rot"]), _dev(case["z_trans"]))


def _reverse(case, rot_score=None, trans_score=None):
    """The reverse-only call: next frames [B, N, 7] from given scores."""
    from str2str_amd import ops

    z_rot, z_trans = _noise(case)
    rs = _dev(case["rot_score"]) if rot_score is None else rot_score
    ts = _dev(case["trans_score"]) if trans_score is None else trans_score
    nxt, _, _ = ops.se3_step(None, _dev(case["xt7"]), _dev(case["mask"]), _dev(case["diffuse_mask"]), _dev(case["p8"]), _dt(case),
                             probability_flow=case["probability_flow"], center=case["center"], noise_scale=case["noise_scale"],
                             z_rot=z_rot, z_trans=z_trans, rot_score_in=rs, trans_score_in=ts)
    return nxt


def _errors(nxt, R64, x64):
    nxt = nxt.cpu()
    assert torch.isfinite(nxt).all()
    e = [ref64.rot_trans_error(ref64.quat_rot64(nxt[b, :, :4]), nxt[b, :, 4:], R64[b], x64[b]) for b in range(nxt.shape[0])]
    return max(a for a, _ in e), max(b for _, b in e)


# ----------------------------------------------------------------------------------------------- SE(3) step
@pytest.mark.parametrize("N", ref64.SE3_N)
@pytest.mark.parametrize("family", sorted(ref64.SE3_FAMILIES))
def test_se3_reverse_vs_float64(diffuser, family, N):
    """One reverse step against reverse_step64: B = 3 at t = (min_t, 0.37, 1), ODE and SDE (noise scale 1 and 0.3, float64
    noise fed in), centre modes 0 / 1 / 2 (mode 2 with prefix masks of lengths N, ceil(N/2), 1), a diffuse_mask that freezes
    a fifth of the residues under a full mask, scalar and per-sample dt; planted frames and scores as ref64.se3_case lists
    them.  Rotations as matrices of the normalised output quaternion, over every residue: a frozen or padded residue must
    return its input frame within the same tolerance.  Bound: 3 x the float32 chain's own distance from float64 over the
    case family (all N)."""
    case = ref64.se3_case(family, N, diffuser)
    e_rot, e_trans = ref64.se3_family_distance(family, diffuser)
    R64, x64 = ref64.se3_ref64(case, diffuser)
    a_rot, a_trans = _errors(_reverse(case), R64, x64)
    print(f"{family} N={N}: rot {a_rot:.3e} (chain {e_rot:.3e}), trans {a_trans:.3e} (chain {e_trans:.3e})")
    check(f"se3 reverse vs float64 [{family}]: rotation matrix entries (bound 3 x float32 chain)", a_rot, 3 * e_rot)
    check(f"se3 reverse vs float64 [{family}]: translations / sample scale (bound 3 x float32 chain)", a_trans, 3 * e_trans)
    frozen = case["diffuse_mask"] == 0
    if frozen.any():   # 0 * x + 1 * x_t in float64: the translation of a frozen residue comes back bit for bit
        assert torch.equal(_reverse(case).cpu()[..., 4:][frozen], case["xt7"][..., 4:][frozen])


@pytest.mark.parametrize("N", [65, 513])
@pytest.mark.parametrize("family", ["ode-c1", "ode-c2", "sde-c1", "sde03-c2"])
def test_se3_fused_call_equals_split_calls(diffuser, family, N):
    """The call the sampler makes (scores from x0 and the reverse step in one launch) returns the frames of a reverse-only call
    fed the scores it returned, bit for bit."""
    from str2str_amd import ops

    case = ref64.se3_case(family, N, diffuser)
    rng = np.random.default_rng(N)
    x0 = np.concatenate([ref64.unit_quats(rng, (ref64.SE3_B, N)),
                         case["xt7"][..., 4:].numpy() + rng.normal(scale=3.0, size=(ref64.SE3_B, N, 3)).astype(np.float32)], -1)
    z_rot, z_trans = _noise(case)
    nxt, rs, ts = ops.se3_step(_dev(torch.as_tensor(x0)), _dev(case["xt7"]), _dev(case["mask"]), _dev(case["diffuse_mask"]), _dev(case["p8"]),
                               _dt(case), probability_flow=case["probability_flow"], center=case["center"],
                               noise_scale=case["noise_scale"], z_rot=z_rot, z_trans=z_trans, want_next=True, want_scores=True)
    assert torch.isfinite(nxt).all() and torch.isfinite(rs).all() and torch.isfinite(ts).all() and rs.abs().max() > 0
    assert (rs.cpu()[case["mask"] == 0] == 0).all() and (ts.cpu()[case["mask"] == 0] == 0).all()
    assert torch.equal(nxt, _reverse(case, rs, ts))
    assert not torch.equal(nxt[..., :4].cpu(), case["xt7"][..., :4])


@pytest.mark.parametrize("family,N", [("ode-c2", 65), ("sde03-c2", 513)])
def test_se3_all_masked_sample_under_masked_centre(diffuser, family, N):
    """A sample without residues (mask = diffuse_mask = 0) under the masked centre of mass has no centre: its frames come back
    (translations bit for bit, rotations as matrices within the reverse test's tolerance) and its batch neighbours do not
    notice it.  Before the kernel took a zero centre for an empty sample it divided 0 by 0 and wrote NaN translations."""
    case = ref64.se3_case(family, N, diffuser)
    full = _reverse(case).cpu()
    case["mask"][1] = 0.0
    case["diffuse_mask"][1] = 0.0
    got = _reverse(case).cpu()
    assert torch.isfinite(got).all()
    assert torch.equal(got[1, :, 4:], case["xt7"][1, :, 4:])
    assert torch.equal(got[0], full[0]) and torch.equal(got[2], full[2])
    # the chain on the empty sample: every residue frozen, no centre
    e_rot, e_trans = ref64.se3_oracle_distance(case, diffuser, lengths=[case["lengths"][0], N, case["lengths"][2]], centers=[True, False, True])
    R64, x64 = ref64.se3_ref64(case, diffuser)
    a_rot, a_trans = _errors(got, R64, x64)
    check(f"se3 reverse, one empty sample [{family}]: rotation matrix entries (bound 3 x float32 chain)", a_rot, 3 * e_rot)
    check(f"se3 reverse, one empty sample [{family}]: translations / sample scale (bound 3 x float32 chain)", a_trans, 3 * e_trans)
    assert float((ref64.quat_rot64(got[1, :, :4]) - ref64.quat_rot64(case["xt7"][1, :, :4])).abs().max()) < 3 * e_rot


def test_se3_step_rejects_more_residues_than_a_workgroup_holds():
    """n_res = 2049 is refused by the launcher's own argument check, before any launch."""
    from str2str_amd import ops

    N = 2049
    xt = torch.zeros(1, N, 7, device=DEV)
    xt[..., 0] = 1.0
    ones, z = torch.ones(1, N, device=DEV), torch.zeros(1, N, 3, device=DEV, dtype=torch.float64)
    with pytest.raises(ops.HipLibraryError, match="s2s_se3_step"):
        ops.se3_step(None, xt, ones, ones, torch.ones(1, 8, device=DEV), 0.01, rot_score_in=z, trans_score_in=z)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------- per-residue frame kernels
@pytest.mark.parametrize("M", [1, 255, 256, 257, 1000])
def test_rigid_compose_update_vs_float64(M):
    """compose_q_update_vec against compose_update64: quaternions off unit norm by up to 1e-3, updates up to 10, a 0/1 mask;
    the padded update buffer (32 columns, the pad filled with NaN) read in place gives the same bits.  Bounds (inside the
    project's 1e-6): 4 roundings on the unit quaternion, 2 on the translation's scale."""
    from str2str_amd import ops

    r7, upd, mask = ref64.compose_case(M)
    ref = ref64.compose_update64(r7, upd, mask)
    out = ops.rigid_compose_update(_dev(r7), _dev(upd), _dev(mask))
    padded = torch.full((M, 32), float("nan"))
    padded[:, :6] = upd
    assert torch.equal(out, ops.rigid_compose_update(_dev(r7), _dev(padded), _dev(mask)))
    assert torch.equal(out.cpu()[mask == 0][:, 4:], r7[mask == 0][:, 4:])   # t + 0 * R u
    out = out.cpu().double()
    check("rigid_compose_update vs float64: quaternion", float((out[:, :4] - ref[:, :4]).abs().max()), 4 * EPS32)
    check("rigid_compose_update vs float64: translation / scale", float((out[:, 4:] - ref[:, 4:]).abs().max() / max(1.0, float(ref[:, 4:].abs().max()))),
          2 * EPS32)


@pytest.mark.parametrize("typed", [True, False], ids=["aatype", "no-aatype"])
@pytest.mark.parametrize("M", [1, 257, 600])
def test_frames_to_backbone_vs_float64(M, typed):
    """compute_backbone against backbone64: all 21 residue types cycled (or none given: alanine), psi as raw un-normalised
    (sin, cos) pairs, translations up to +-500 A.  Asking for atom37 only, atom14 only or both returns the same bits; atom37
    slots 5..36 are exactly 0 past the first workgroup too; glycine's CB and the unknown type's atoms are exactly 0, so the
    atom mask derived from the coordinates is the reference's.  Bound (inside the project's 1e-6): 2.5 float32 roundings of the
    coordinate scale."""
    from str2str_amd import ops

    r7, psi, aatype = ref64.backbone_case(M)
    aa = _dev(aatype) if typed else None
    a37_ref, m37_ref, bb5_ref = ref64.backbone64(r7, psi, aatype if typed else None)
    a37, a14 = ops.frames_to_backbone(_dev(r7), _dev(psi), aa, want_atom37=True, want_atom14=True)
    only37, none14 = ops.frames_to_backbone(_dev(r7), _dev(psi), aa, want_atom37=True, want_atom14=False)
    none37, only14 = ops.frames_to_backbone(_dev(r7), _dev(psi), aa, want_atom37=False, want_atom14=True)
    assert none14 is None and none37 is None and torch.equal(a37, only37) and torch.equal(a14, only14)
    a37, a14 = a37.cpu(), a14.cpu()
    assert a37.shape == (M, 37, 3) and a14.shape == (M, 5, 3)
    assert (a37[:, 5:] == 0).all()
    assert torch.equal(a37[:, [0, 1, 2, 4, 3]], a14)
    if typed:
        gly, unk = aatype == 7, aatype == 20
        assert gly.any() and (a14[gly, 4] == 0).all() and (a37[gly, 3] == 0).all() and (a14[unk] == 0).all()
    assert torch.equal((a37 != 0).any(-1), m37_ref)
    scale = max(1.0, float(a37_ref.abs().max()))
    check("frames_to_backbone vs float64: atom37 / coordinate scale", float((a37.double() - a37_ref).abs().max()) / scale, 2.5 * EPS32)
    check("frames_to_backbone vs float64: atom14 / coordinate scale", float((a14.double() - bb5_ref).abs().max()) / scale, 2.5 * EPS32)


# ----------------------------------------------------------------------------------------------- forward-marginal prior
@pytest.mark.parametrize("rows", ["synthetic", "diffuser"])
def test_forward_marginal_prior_vs_float64(diffuser, rows):
    """The prior draw as a pure function of its noise, several CDF rows in one call (row_of_sample = (1, 0, 1)): 2 synthetic
    rows of 9 knots, then the diffuser's 1000-point rows of t = 0.05 and t = 1.  The uniforms sit on np.interp's branches
    (ref64.prior_u): the clamps at both ends, exact knot hits, between knots.  Rotation matrices against prior_rotation64 at
    the bound of the existing prior-sample check; translations are z / 0.1 in float32, exactly."""
    from str2str_amd import ops

    if rows == "synthetic":
        cdf, omega = ref64.synthetic_cdf_rows()
    else:
        sd = diffuser.rot_diffuser
        idx = [int(sd.t_to_idx(torch.tensor([t]))[0]) for t in (0.05, 1.0)]
        assert idx[0] != idx[1]
        cdf, omega = torch.as_tensor(np.stack([sd.cdf_row(i) for i in idx]), dtype=torch.float64), sd.discrete_omega.float().contiguous()
    row_of_sample = (1, 0, 1)
    u = ref64.prior_u(cdf, row_of_sample)
    B, N = u.shape
    g = torch.Generator().manual_seed(11)
    z_axis, z_trans = torch.randn(B, N, 3, generator=g), torch.randn(B, N, 3, generator=g)
    out = ops.forward_marginal(None, _dev(z_axis), _dev(u), _dev(z_trans), _dev(cdf), _dev(torch.tensor(row_of_sample, dtype=torch.int32)),
                               _dev(omega), None).cpu()
    R = ref64.prior_rotation64(z_axis, u, cdf, row_of_sample, omega)
    check(f"prior rotation vs float64 [{rows} cdf rows]: rotation matrix entries", float((ref64.quat_rot64(out[..., :4]) - R).abs().max()), 1.2e-6)
    assert np.array_equal(out[..., 4:].numpy(), z_trans.numpy() / np.float32(0.1))
    # the rows differ where it matters: sample 1 on its own row is not sample 1 on the others' row
    R_other = ref64.prior_rotation64(z_axis, u, cdf, (1, 1, 1), omega)
    assert float((R_other[1] - R[1]).abs().max()) > 1e-2


# ----------------------------------------------------------------------------------------------- ensemble statistics
@pytest.mark.parametrize("k_exclusion", [0, 3])
@pytest.mark.parametrize("L", [2, 63, 257, 600])
def test_ca_sample_stats_vs_numpy(L, k_exclusion):
    """Per-sample clash count and largest adjacent distance equal numpy's float32 values (a pair at exactly 3.0 A is no clash,
    one an ulp closer is); Rg within 1e-13 relative of float64: only the summation order differs, 600 terms x 2^-53 = 7e-14
    at worst (inside the 1e-12 the metric is held to elsewhere)."""
    from str2str_amd import ops

    ca = ref64.walk_ensemble(5, L)
    n_ref, adj_ref, rg_ref = ref64.sample_stats_np(ca, 3.0, k_exclusion)
    n, adj, rg = (x.cpu().numpy() for x in ops.ca_sample_stats(_dev(torch.as_tensor(ca)), 3.0, k_exclusion))
    assert np.array_equal(n, n_ref), (n, n_ref)
    assert np.array_equal(adj, adj_ref)
    if L > 1 + k_exclusion:
        assert n_ref.max() >= 1
    check("ca_sample_stats: radius of gyration vs float64, relative", float(np.abs(rg / rg_ref - 1).max()), 1e-13)


@pytest.mark.parametrize("R,L,offset", [(2, 300, 1), (2, 300, 3), (1, 1500, 1)])
def test_ca_pairwise_distances_equal_numpy(R, L, offset):
    """Bit for bit numpy's float32 distances; L = 1500 has more channels than 4096 x 256 threads: the grid-stride loop."""
    from str2str_amd import ops

    ca = ref64.walk_ensemble(R, L, plant=False)
    got = ops.ca_pairwise_distances(_dev(torch.as_tensor(ca)), offset).cpu().numpy()
    assert got.shape == (R, (L - offset) * (L - offset + 1) // 2)
    assert np.array_equal(got, ref64.pairwise_np(ca, offset))


@pytest.mark.parametrize("R_ref", [1, 65])
def test_ca_pwd_js_vs_numpy(R_ref):
    """L = 70 at offset 3: 2278 channels, so the last workgroup holds two; a single-structure reference (numpy's degenerate
    range) and one longer than a wavefront; unweighted, then float64 per-sample weights.  Unweighted the counts are integers and
    only the 50-term float64 sum and logarithms differ: 2e-15 (the metric's existing bound is 1e-12).  Weighted, a bin's
    weights add in the order the lanes' atomics land, which changes from run to run: up to 130 weights x 2^-53 per bin, through
    the square root at a distance of 0.05 or more: 2e-13 (existing bound 1e-9)."""
    from str2str_amd import ops

    rng = np.random.default_rng(R_ref)
    base = ref64.walk_ensemble(1, 70, plant=False)[0]
    ref = (base + rng.normal(scale=1.0, size=(R_ref, 70, 3))).astype(np.float32)
    pred = (base + rng.normal(scale=1.3, size=(130, 70, 3))).astype(np.float32)
    w = rng.uniform(0.1, 2.0, size=130)
    got = ops.ca_pwd_js(_dev(torch.as_tensor(ref)), _dev(torch.as_tensor(pred)), 3, 50, 1e-6).cpu().numpy()
    assert got.shape == (2278,)
    check(f"ca_pwd_js vs numpy, R_ref={R_ref}: per-channel |JS - numpy|", float(np.abs(got - ref64.js_channels_np(ref, pred)).max()), 2e-15)
    got = ops.ca_pwd_js(_dev(torch.as_tensor(ref)), _dev(torch.as_tensor(pred)), 3, 50, 1e-6, pred_weights=_dev(torch.as_tensor(w))).cpu().numpy()
    check(f"ca_pwd_js weighted vs numpy, R_ref={R_ref}: per-channel |JS - numpy|",
          float(np.abs(got - ref64.js_channels_np(ref, pred, pred_weights=w)).max()), 2e-13)
