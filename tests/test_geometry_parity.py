"""The HIP kernels that carry no matrix product -- the SE(3) step (score and reverse halves), the per-residue frame kernels, the
forward marginal (prior and noising branches) and the ensemble statistics -- against the float64 references of tests/ref64.py, through ``str2str_amd.ops``, at the shapes where
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
import score_cases as sc
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


def _scores(c):
    """The score-only call on a case of score_cases.score_case -> (rot, trans) [B, N, 3] float64 on the CPU."""
    from str2str_amd import ops

    _, rs, ts = ops.se3_step(_dev(c["x0"]), _dev(c["xt"]), _dev(c["mask"]), _dev(torch.ones_like(c["mask"])), _dev(c["p8"]), 0.0,
                             want_next=False, want_scores=True)
    assert rs.dtype == torch.float64 and ts.dtype == torch.float64
    return rs.cpu(), ts.cpu()


@pytest.mark.parametrize("N", sc.SCORE_N)
def test_se3_scores_vs_float64(diffuser, N):
    """The score half of the step (log(R_0^T R_t), the 1000-term IGSO(3) series, the translation score) against score64 on the
    table of tests/score_cases.py: B = 3 at t = (min_t, 0.37, 1), eleven relative angles from exactly 0 to pi - 1e-5 laid
    along the residues, x_t of every orientation class, a full, a gapped and a prefix mask over finite garbage, translations
    up to +-300 A.  Per (angle, sample), residues on the principal and on the wrapped branch of the reference's float32 chain
    judged and recorded apart, both against 3 x the chain's distance from float64 on the principal residues; the translation
    score per sample against 3 x the float32 formula's distance; masked residues exactly 0.  Every figure is recorded before
    the first assertion.

    Before the product quaternion's sign was standardised in the kernel, the wrapped residues missed the bound at every angle
    (measured on an MI355X at t = min_t: |error| 38 at theta = 1e-6, 1.5 at 1e-4, 0.14 at 1e-3, 1.6e-2 at 1e-2, 1.6e-3 at 0.1
    against bounds of 4e-5 .. 5.5e-5; 1.4 .. 2.8 x the bound from theta = 1 up at t = 0.37 and 1) while the principal residues
    sat where they sit now; tests/test_ref64_cpu.py plants the same mistake in the float32 chain."""
    c = sc.score_case(N, diffuser)
    D, Dt = sc.score_d32(diffuser)
    rs, ts = _scores(c)
    assert torch.isfinite(rs).all() and torch.isfinite(ts).all()
    late = []
    for which in ("principal", "wrapped"):
        e = sc.score_family_errors(rs, N, diffuser, which)
        for k in range(len(sc.SCORE_THETA)):
            for b in range(sc.SCORE_B):
                if not torch.isnan(e[k, b]):
                    name = f"se3 rotation score vs float64 [{sc.family_label(k, b)}], {which} residues (bound 3 x D32)"
                    record_margin(name, float(e[k, b]), 3 * float(D[k, b]))
                    late.append((name, float(e[k, b]), 3 * float(D[k, b])))
        ok = ~torch.isnan(e)
        print(f"N={N} {which}: largest error / bound {float((e / (3 * D))[ok].max()) if ok.any() else 0.0:.3f}")
    e_t = sc.trans_sample_errors(ts, N, diffuser)
    for b in range(sc.SCORE_B):
        name = f"se3 translation score vs float64 [t[{b}]] (bound 3 x float32 formula)"
        record_margin(name, float(e_t[b]), 3 * float(Dt[b]))
        late.append((name, float(e_t[b]), 3 * float(Dt[b])))
    failed = [x for x in late if not x[1] < x[2]]
    assert not failed, failed
    masked = c["mask"] == 0
    assert torch.equal(rs[masked], torch.zeros_like(rs[masked])) and torch.equal(ts[masked], torch.zeros_like(ts[masked]))


def test_se3_scores_of_bit_equal_rotations_are_exactly_zero(diffuser):
    """theta = 0 (x_0's quaternion bit-equal to x_t's) under mask 1: the rotation score is exactly 0, as score64 has it, at
    every N of the table -- and with x_0's quaternion negated, which is the same rotation.

    The chain the kernel restates does not return 0 there: invert_quat divides by |q|^2, which is 1 to float32 rounding only,
    so R(q_0^-1) is not the exact transpose of R(q_t) and the product quaternion's vector part is a few 1e-8.  Measured on an
    MI355X before the kernel took v = 0 for q_0 = +-q_t: 475 of the table's 693 such residues not exactly 0, largest |score|
    1.03e-5 at t = min_t (sigma 0.1), 1.8e-7 at t = 0.37, 3.9e-8 at t = 1 (with the product's sign not standardised either:
    39.7, 2.7, 0.53)."""
    flip = torch.tensor([-1.0, -1, -1, -1, 1, 1, 1])
    for sign in ("+", "-"):
        worst, nonzero, total = 0.0, 0, 0
        for N in sc.SCORE_N:
            c = sc.score_case(N, diffuser)
            zero = (c["band"] == 0) & (c["mask"] > 0)
            assert torch.equal(c["x0"][..., :4][zero], c["xt"][..., :4][zero])
            got = _scores(c if sign == "+" else dict(c, x0=c["x0"] * flip))[0][zero]
            worst, nonzero, total = max(worst, float(got.abs().max())), nonzero + int((got != 0).any(-1).sum()), total + int(zero.sum())
        print(f"theta = 0, q_0 = {sign}q_t: largest |rotation score| {worst:.3e}, {nonzero} of {total} residues not exactly 0")
        record_margin(f"se3 rotation score at theta = 0, q_0 = {sign}q_t: largest |score| (required: exactly 0)", worst, 0.0)
        assert nonzero == 0, (sign, worst, nonzero, total)


@pytest.mark.parametrize("family,N", [("ode-c2", 65), ("sde03-c2", 513)])
def test_se3_fused_step_vs_float64(diffuser, family, N):
    """The call the sampler makes -- scores from x_0 and the reverse step in one launch -- against reverse_step64 fed score64's
    scores (ref64.se3_fused_case: x_0 within 2 sigma of x_t, prefix masks, masked centre).  Bound: 3 x the distance of the
    reference's float32 chain (its own score, then its reverse step) from that on the same case."""
    from str2str_amd import ops

    case = ref64.se3_fused_case(family, N, diffuser)
    e_rot, e_trans = ref64.se3_oracle_distance(case, diffuser)
    R64, x64 = ref64.se3_ref64(case, diffuser)
    z_rot, z_trans = _noise(case)
    nxt, rs, ts = ops.se3_step(_dev(case["x0"]), _dev(case["xt7"]), _dev(case["mask"]), _dev(case["diffuse_mask"]), _dev(case["p8"]), _dt(case),
                               probability_flow=case["probability_flow"], center=case["center"], noise_scale=case["noise_scale"],
                               z_rot=z_rot, z_trans=z_trans, want_next=True, want_scores=True)
    a_rot, a_trans = _errors(nxt, R64, x64)
    print(f"{family} N={N}: rot {a_rot:.3e} (chain {e_rot:.3e}), trans {a_trans:.3e} (chain {e_trans:.3e})")
    check(f"se3 fused step vs float64 [{family}, N={N}]: rotation matrix entries (bound 3 x float32 chain)", a_rot, 3 * e_rot)
    check(f"se3 fused step vs float64 [{family}, N={N}]: translations / sample scale (bound 3 x float32 chain)", a_trans, 3 * e_trans)
    assert (rs.cpu()[case["mask"] == 0] == 0).all() and (ts.cpu()[case["mask"] == 0] == 0).all()


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


@pytest.mark.parametrize("N", sc.FM_N)
def test_forward_marginal_noising_vs_float64(diffuser, N):
    """The noising branch (given rigids0_4x4: matrix -> axis-angle, the composition in float64, the VP translation, the blend,
    back to a quaternion) against forward_marginal64 on the table of tests/score_cases.py: row_of_sample = (1, 0, 1) on the
    diffuser's rows of t = 0.05 and 1, params2 at t = (min_t, 0.37, 1), uniforms on np.interp's branches, the planted frames,
    compositions that cross pi, 4 x 4 inputs orthonormal to float32 rounding only, a fifth of the residues frozen.  Bound: 3 x
    the float32 chain's distance on the same draws, at most 5e-6.  Frozen residues: translations bit for bit, rotations inside
    the same bound."""
    from str2str_amd import ops

    c = sc.fm_case(N, diffuser)
    out = ops.forward_marginal(_dev(c["rig0"]), _dev(c["z_axis"]), _dev(c["u"]), _dev(c["z_trans"]), _dev(c["cdf"]),
                               _dev(torch.tensor(c["rows"], dtype=torch.int32)), _dev(c["omega"]), _dev(c["params2"]), _dev(c["diffuse_mask"])).cpu()
    assert torch.isfinite(out).all()
    a_rot, a_trans = sc.fm_errors(out, N, diffuser)
    b_rot, b_trans = sc.fm_bounds(N, diffuser)
    print(f"N={N}: rot {a_rot:.3e} (bound {b_rot:.3e}), trans {a_trans:.3e} (bound {b_trans:.3e})")
    check(f"forward marginal, noising, vs float64 [N={N}]: rotation matrix entries (bound 3 x float32 chain, <= 5e-6)", a_rot, b_rot)
    check(f"forward marginal, noising, vs float64 [N={N}]: translations / sample scale (bound 3 x float32 chain, <= 5e-6)", a_trans, b_trans)
    frozen = c["diffuse_mask"] == 0
    if frozen.any():
        assert torch.equal(out[..., 4:][frozen], c["rig0"][..., :3, 3][frozen])
        R64, _ = sc.fm_ref64(N, diffuser)
        assert float((ref64.quat_rot64(out[..., :4]) - R64)[frozen].abs().max()) < b_rot


def test_forward_marginal_device_noising_vs_float64(diffuser):
    """The same through FrameDiffuser.forward_marginal_device with the noise given (N = 257, t_delta = 0.37): the wrapper's
    CDF-row lookup and params2 against the reference's own formulae (oracle.diffuser.SO3 / R3), which the wrapper does not
    share."""
    from oracle import diffuser as OD

    N, t_delta = 257, 0.37
    c = sc.fm_case(N, diffuser)
    out = diffuser.forward_marginal_device(_dev(c["rig0"]), t_delta, diffuse_mask=_dev(c["diffuse_mask"]),
                                           noise=(_dev(c["z_axis"]), _dev(c["u"]), _dev(c["z_trans"]))).cpu()
    so3, r3 = OD.SO3(), OD.R3()
    t = torch.full((sc.FM_B,), t_delta, dtype=torch.float32)
    mb = r3.marginal_b_t(t)
    args = sc.fm_args(c, cdf_rows=so3.cdf_row(int(so3.t_to_idx(t[0])))[None], row_of_sample=(0, 0, 0), omega_grid=so3.discrete_omega,
                      params2=torch.stack([torch.exp(-0.5 * mb), torch.sqrt(1 - torch.exp(-mb))], -1))
    R64, x64 = ref64.forward_marginal64(**args)
    chain = ref64.forward_marginal_chain32(**args)

    def errors(o):
        e = [ref64.rot_trans_error(ref64.quat_rot64(o[b, :, :4]), o[b, :, 4:], R64[b], x64[b]) for b in range(sc.FM_B)]
        return max(a for a, _ in e), max(b for _, b in e)

    (e_rot, e_trans), (a_rot, a_trans) = errors(chain), errors(out)
    print(f"rot {a_rot:.3e} (chain {e_rot:.3e}), trans {a_trans:.3e} (chain {e_trans:.3e})")
    check("forward_marginal_device, noising, vs float64: rotation matrix entries (bound 3 x float32 chain, <= 5e-6)", a_rot, min(3 * e_rot, sc.FM_CAP))
    check("forward_marginal_device, noising, vs float64: translations / sample scale (bound 3 x float32 chain, <= 5e-6)", a_trans,
          min(3 * e_trans, sc.FM_CAP))


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
