"""Float64 references of the kernels that carry no matrix product, and the seeded inputs their tests share.

Plain numpy / torch on the CPU.  The references hold the mathematics of each operation (a rotation is a matrix, a geodesic
step is a matrix exponential), not the float32 conversion chain of the reference project: tests/test_ref64_cpu.py pins them
to the committed fixtures and measures how far that float32 chain (oracle/) sits from them, and tests/test_geometry_parity.py
holds the HIP kernels to a multiple of that distance.
"""
import functools
import zlib

import numpy as np
import torch

F64 = torch.float64


# ----------------------------------------------------------------------------------------------- rotations
def _f64(a):
    return torch.as_tensor(np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a)).to(F64)


def quat_form64(q):
    """The un-normalised quadratic form of quat_to_rot (w, x, y, z), float64: |q|^2 times a rotation."""
    a, b, c, d = _f64(q).unbind(-1)
    rows = [[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
            [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
            [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]]
    return torch.stack([torch.stack(r, -1) for r in rows], -2)


def quat_rot64(q):
    """Rotation matrix of q / |q|: the sign of q and a 2 pi wrap of its angle do not enter."""
    q = _f64(q)
    return quat_form64(q / q.norm(dim=-1, keepdim=True))


def hat(v):
    v = _f64(v)
    x, y, z = v.unbind(-1)
    o = torch.zeros_like(x)
    return torch.stack([torch.stack([o, -z, y], -1), torch.stack([z, o, -x], -1), torch.stack([-y, x, o], -1)], -2)


def rotvec_exp64(v):
    return torch.linalg.matrix_exp(hat(v))


# ----------------------------------------------------------------------------------------------- SE(3) reverse step
def reverse_step64(xt7, rot_score, trans_score, t, dt, diffuse_mask, mask, center_mode, noise_scale, probability_flow, z_rot, z_trans,
                   diffuser):
    """One reverse step of the IGSO(3) x VP-SDE frame diffusion in float64 -> (R_next [B,N,3,3], x_next [B,N,3]).

    Rotation: R(q_t / |q_t|) exp(hat(-(drift + diff))), drift = -g_r^2 s_r dt h, diff = g_r sqrt(dt) noise_scale z_r (h = 1/2 and
    no diff on the probability-flow ODE).  Translation, in coordinates scaled by 0.1: x - (drift + diff) with
    drift = (-b(t) x / 2 - g_x^2 s_x) dt h, then minus the centre of mass (mode 1: over every residue; mode 2: sum(m x) / sum(m),
    zero for a sample without residues; mode 0: none), then back to Angstrom.  Residues with ``diffuse_mask`` 0 keep their frame.
    ``dt``: a scalar or one value per sample.  The schedule scalars are ``diffuser.step_params(t)``."""
    xt7, rs, ts = _f64(xt7), _f64(rot_score), _f64(trans_score)
    dm, m = _f64(diffuse_mask)[..., None], _f64(mask)[..., None]
    B = xt7.shape[0]
    p8 = diffuser.step_params(torch.as_tensor(t, dtype=torch.float32)).to(F64)
    g2r, bt, g2t, gr, gt = (p8[:, k].reshape(B, 1, 1) for k in (1, 4, 5, 6, 7))
    dt = _f64(dt).reshape(-1, 1, 1).expand(B, 1, 1)
    h = 0.5 if probability_flow else 1.0
    cs = float(diffuser.trans_diffuser.coordinate_scaling)
    zr = torch.zeros_like(rs) if probability_flow else noise_scale * _f64(z_rot)
    zt = torch.zeros_like(ts) if probability_flow else noise_scale * _f64(z_trans)

    R_t = quat_rot64(xt7[..., :4])
    pert = -(-g2r * rs * dt * h + gr * dt.sqrt() * zr)
    R_1 = R_t @ rotvec_exp64(pert)
    R_next = torch.where(dm[..., None] > 0, R_1, R_t)

    x = xt7[..., 4:] * cs
    x1 = x - ((-0.5 * bt * x - g2t * ts) * dt * h + gt * dt.sqrt() * zt)
    if center_mode == 1:
        x1 = x1 - x1.mean(dim=1, keepdim=True)
    elif center_mode == 2:
        cnt = m.sum(dim=1, keepdim=True)
        x1 = x1 - torch.where(cnt > 0, (m * x1).sum(dim=1, keepdim=True) / cnt.clamp(min=1.0), torch.zeros_like(cnt))
    x_next = torch.where(dm > 0, x1 / cs, xt7[..., 4:])
    return R_next, x_next


# ----------------------------------------------------------------------------------------------- SE(3) score
def quat_mul64(p, q):
    """Hamilton product (w, x, y, z), float64.  The vector part adds its terms in the pairs that cancel in conj(q) (x) q, so that
    product is exactly (|q|^2, 0, 0, 0)."""
    a1, b1, c1, d1 = _f64(p).unbind(-1)
    a2, b2, c2, d2 = _f64(q).unbind(-1)
    return torch.stack([(a1 * a2 - b1 * b2) - (c1 * c2 + d1 * d2), (a1 * b2 + b1 * a2) + (c1 * d2 - d1 * c2),
                        (a1 * c2 + c1 * a2) + (d1 * b2 - b1 * d2), (a1 * d2 + d1 * a2) + (b1 * c2 - c1 * b2)], -1)


def relative_rotvec64(q0, qt):
    """The principal rotation vector of R(q0)^T R(qt), angle in [0, pi]: the product of the normalised float64 quaternions with
    its sign standardised (w >= 0), angle = 2 atan2(|xyz|, w).  Bit-equal quaternions give exactly 0."""
    q0, qt = _f64(q0), _f64(qt)
    q0 = q0 / q0.norm(dim=-1, keepdim=True) * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=F64)
    p = quat_mul64(q0, qt / qt.norm(dim=-1, keepdim=True))
    p = torch.where(p[..., :1] < 0, -p, p)
    s = p[..., 1:].norm(dim=-1, keepdim=True)
    theta = 2 * torch.atan2(s, p[..., :1])
    return torch.where(s > 0, p[..., 1:] / s.clamp(min=1e-300) * theta, torch.zeros_like(p[..., 1:]))


def igso3_series64(omega, sigma, L=1000):
    """(f, df / d omega) of the IGSO(3) expansion, oracle/diffuser.py:36-63 term for term, in float64.  ``omega`` and ``sigma``
    broadcast against each other; numpy, a thousand angles at a time."""
    omega, sigma = np.broadcast_arrays(np.asarray(omega, dtype=np.float64), np.asarray(sigma, dtype=np.float64))
    shape = omega.shape
    om, sg = omega.reshape(-1), sigma.reshape(-1)
    ls = np.arange(L, dtype=np.float64)[None]
    f, df = np.empty_like(om), np.empty_like(om)
    for a in range(0, om.size, 1024):
        o, e = om[a:a + 1024, None], sg[a:a + 1024, None]
        w = (2 * ls + 1) * np.exp(-ls * (ls + 1) * e ** 2 / 2)
        hi, dhi = np.sin(o * (ls + 0.5)), (ls + 0.5) * np.cos(o * (ls + 0.5))
        lo, dlo = np.sin(o / 2), 0.5 * np.cos(o / 2)
        f[a:a + 1024] = (w * hi / lo).sum(-1)
        df[a:a + 1024] = (w * (lo * dhi - hi * dlo) / lo ** 2).sum(-1)
    return f.reshape(shape), df.reshape(shape)


def rot_score_of_rotvec64(v, sigma):
    """df / (f + 1e-4) * v / (omega + 1e-6) with omega = |v| + 1e-6 (so3.py:274-309 of the reference), float64.
    ``v`` [B, N, 3], ``sigma`` [B]."""
    v = _f64(v)
    omega = v.norm(dim=-1) + 1e-6
    f, df = igso3_series64(omega.numpy(), np.asarray(_f64(sigma)).reshape(-1, 1))
    return (torch.as_tensor(df) / (torch.as_tensor(f) + 1e-4))[..., None] * v / (omega[..., None] + 1e-6)


def trans_score64(x0, xt, p8, cs):
    """-(cs x_t - e_half cs x_0) / cond_var with the schedule scalars of step_params, float64 (unmasked)."""
    p8 = _f64(p8)
    eh, cv = p8[:, 2].reshape(-1, 1, 1), p8[:, 3].reshape(-1, 1, 1)
    return -(cs * _f64(xt) - eh * (cs * _f64(x0))) / cv


def score64(x0_7, xt_7, t, mask, diffuser):
    """The conditional score of the IGSO(3) x VP-SDE frame diffusion in float64 -> (rot [B,N,3], trans [B,N,3]), a pure function
    of the float32 inputs.  Rotation: v = the principal rotation vector of R(q_0)^T R(q_t) (relative_rotvec64; the rotations are
    quat_rot64 of each quaternion), omega = |v| + 1e-6, score = df / (f + 1e-4) * v / (omega + 1e-6) * mask with the 1000-term
    series at sigma = the float32 bin value ``diffuser.step_params(t)[:, 0]``.  Translation, in coordinates scaled by 0.1:
    -(0.1 x_t - e_half 0.1 x_0) / cond_var * mask."""
    x0, xt, m = _f64(x0_7), _f64(xt_7), _f64(mask)[..., None]
    p8 = diffuser.step_params(torch.as_tensor(t, dtype=torch.float32)).to(F64)
    rot = rot_score_of_rotvec64(relative_rotvec64(x0[..., :4], xt[..., :4]), p8[:, 0])
    trans = trans_score64(x0[..., 4:], xt[..., 4:], p8, float(diffuser.trans_diffuser.coordinate_scaling))
    return rot * m, trans * m


def score_chain32(x0_7, xt_7, p8, mask, standardise=False, cs=0.1):
    """The reference's float32 conversion chain for v (oracle.geometry, as oracle.diffuser.FrameDiffuser.score strings it
    together: inverse quaternion -> matrix -> quaternion, frame -> matrix -> quaternion, product, axis-angle), then the series
    in float64, and the translation score in float32 -> (rot [B,N,3] float64, trans [B,N,3] float64, w [B,N] float32).
    ``w`` is the real part of the float32 product: >= 0 on the principal branch (angle in [0, pi]), < 0 on the wrapped one
    (angle 2 pi - delta, rebuilt as |xyz| angle / sin(angle / 2) next to sin's zero).  ``standardise``: the kernel's contract,
    which negates the product where w < 0 before the axis-angle conversion and takes v = 0 where q_0 = +-q_t component for
    component (one rotation on both sides; the chain's |q|^2 division leaves a few 1e-8 there)."""
    from oracle import geometry as G

    x0, xt = torch.as_tensor(x0_7).float(), torch.as_tensor(xt_7).float()
    q0_inv = G.matrix_to_quaternion(G.quat_to_rot(G.invert_quat(x0[..., :4])))
    qt = G.matrix_to_quaternion(G.quat_to_rot(xt[..., :4]))
    p = G.quat_multiply(q0_inv, qt)
    w = p[..., 0].clone()
    if standardise:
        p = torch.where(p[..., :1] < 0, -p, p)
    v = G.quaternion_to_axis_angle(p)
    if standardise:
        a, b = x0[..., :4], xt[..., :4]
        v = torch.where(((a == b).all(-1) | (a == -b).all(-1))[..., None], torch.zeros_like(v), v)
    m = _f64(mask)[..., None]
    p8 = torch.as_tensor(p8).float()
    rot = rot_score_of_rotvec64(v, p8[:, 0]) * m
    eh, cv = p8[:, 2].reshape(-1, 1, 1), p8[:, 3].reshape(-1, 1, 1)
    csf = torch.tensor(cs, dtype=torch.float32)
    trans = (-(xt[..., 4:] * csf - eh * (x0[..., 4:] * csf)) / cv).double() * m
    return rot, trans, w


# ----------------------------------------------------------------------------------------------- per-residue frame kernels
def compose_update64(rigids7, update6, mask):
    """normalize(q + m q (x) (0, v)) and t + m R(q) u with R the un-normalised quadratic form -> [M, 7] float64."""
    r, u, m = _f64(rigids7), _f64(update6), _f64(mask).reshape(-1, 1)
    q, t = r[:, :4], r[:, 4:]
    a, b, c, d = q.unbind(-1)
    x, y, z = u[:, :3].unbind(-1)
    qv = torch.stack([-b * x - c * y - d * z, a * x + c * z - d * y, a * y - b * z + d * x, a * z + b * y - c * x], -1)
    nq = q + m * qv
    nq = nq / nq.norm(dim=-1, keepdim=True)
    nt = t + m * (quat_form64(q) @ u[:, 3:, None])[..., 0]
    return torch.cat([nq, nt], -1)


def backbone64(rigids7, psi, aatype=None):
    """Idealised backbone atoms of each frame in float64 -> (atom37 [M,37,3], mask37 [M,37] bool, bb5 [M,5,3] in atom14 order
    N, CA, C, O, CB).  O sits in the psi frame: default frame of the residue type, composed with Rx(psi) from the raw
    (sin, cos) pair; the other four sit in the backbone frame."""
    from str2str_amd.data import backbone_tables as bt

    r, psi = _f64(rigids7), _f64(psi)
    M = r.shape[0]
    aa = torch.zeros(M, dtype=torch.long) if aatype is None else torch.as_tensor(aatype).long().cpu()
    pos, amask = _f64(bt.BB_POS)[aa], _f64(bt.BB_MASK)[aa]
    in_psi = torch.as_tensor(bt.BB_GROUP == 3)[aa]
    dflt = _f64(bt.BB_FRAMES)[aa]                      # [M, 2, 4, 4]
    sn, cn = psi[:, 0], psi[:, 1]
    tor = torch.zeros(M, 2, 3, 3, dtype=F64)
    tor[:, :, 0, 0] = 1.0
    tor[:, 0, 1, 1] = tor[:, 0, 2, 2] = 1.0
    tor[:, 1, 1, 1], tor[:, 1, 1, 2], tor[:, 1, 2, 1], tor[:, 1, 2, 2] = cn, -sn, sn, cn
    R = quat_form64(r[:, :4])[:, None]                 # [M, 1, 3, 3]
    G_rot = R @ (dflt[..., :3, :3] @ tor)              # [M, 2, 3, 3]
    G_trans = (R @ dflt[..., :3, 3:])[..., 0] + r[:, None, 4:]
    g = in_psi.long()                                  # [M, 5] -> group slot of each atom
    A_rot = torch.gather(G_rot, 1, g[:, :, None, None].expand(M, 5, 3, 3))
    A_trans = torch.gather(G_trans, 1, g[:, :, None].expand(M, 5, 3))
    bb5 = ((A_rot @ pos[..., None])[..., 0] + A_trans) * amask[..., None]
    atom37 = torch.zeros(M, 37, 3, dtype=F64)
    atom37[:, :3], atom37[:, 3], atom37[:, 4] = bb5[:, :3], bb5[:, 4], bb5[:, 3]
    return atom37, (atom37 != 0).any(-1), bb5


def prior_rotation64(z_axis, u, cdf_rows, row_of_sample, omega_grid):
    """IGSO(3) draw as a matrix: angle = np.interp(u, cdf row of the sample, omega grid), axis = z / |z| -> [B, N, 3, 3]."""
    z, u = _f64(z_axis), np.asarray(_f64(u))
    cdf, om = np.asarray(_f64(cdf_rows)), np.asarray(_f64(omega_grid))
    ang = np.stack([np.interp(u[b], cdf[int(r)], om) for b, r in enumerate(np.asarray(row_of_sample))])
    return rotvec_exp64(z / z.norm(dim=-1, keepdim=True) * torch.as_tensor(ang)[..., None])


def matrix_rot64(m):
    """The rotation a 3 x 3 block that is orthonormal to float32 rounding stands for: matrix -> quaternion (the four-candidate
    formula, in float64) -> quat_rot64, which normalises."""
    from oracle import geometry as G

    return quat_rot64(G.matrix_to_quaternion(_f64(m)))


def forward_marginal64(rig0_4x4, z_axis, u, z_trans, cdf_rows, row_of_sample, omega_grid, params2, diffuse_mask=None, cs=0.1):
    """The noising branch of the forward marginal in float64 -> (R [B,N,3,3], x [B,N,3]), a pure function of the float32 frames
    and noise.  Rotation: R_0 (matrix_rot64 of the 3 x 3 block) times the IGSO(3) draw prior_rotation64; translation, in
    coordinates scaled by 0.1: (e_half 0.1 x_0 + std z) / 0.1 with (e_half, std) = params2 of the sample.  Residues with
    ``diffuse_mask`` 0 keep R_0 and x_0."""
    g = _f64(rig0_4x4)
    R0, x0 = matrix_rot64(g[..., :3, :3]), g[..., :3, 3]
    p2 = _f64(params2)
    eh, std = p2[:, 0].reshape(-1, 1, 1), p2[:, 1].reshape(-1, 1, 1)
    R = R0 @ prior_rotation64(z_axis, u, cdf_rows, row_of_sample, omega_grid)
    x = (eh * (cs * x0) + std * _f64(z_trans)) / cs
    if diffuse_mask is not None:
        dm = _f64(diffuse_mask)[..., None]
        R, x = torch.where(dm[..., None] > 0, R, R0), torch.where(dm > 0, x, x0)
    return R, x


def forward_marginal_chain32(rig0_4x4, z_axis, u, z_trans, cdf_rows, row_of_sample, omega_grid, params2, diffuse_mask=None, cs=0.1):
    """oracle.diffuser.FrameDiffuser.forward_marginal on given noise, float32 with its float64 island (np.interp and
    compose_rotvec), statement for statement -> frames [B, N, 7] float32.  tests/test_ref64_cpu.py holds it bit for bit to the
    oracle's own call under the oracle's draws."""
    from oracle import diffuser as OD
    from oracle import geometry as G

    g = torch.as_tensor(rig0_4x4).float()
    rot_0, trans_0 = G.matrix_to_axis_angle(g[..., :3, :3]), g[..., :3, 3]
    z = torch.as_tensor(z_axis).float()
    x = z / torch.linalg.norm(z, dim=-1, keepdims=True)
    cdf, om, uu = np.asarray(cdf_rows, dtype=np.float64), np.asarray(omega_grid), np.asarray(torch.as_tensor(u).float())
    scal = torch.as_tensor(np.asarray([np.interp(uu[b], cdf[int(r)], om) for b, r in enumerate(np.asarray(row_of_sample))]), dtype=x.dtype)
    rot_t = OD.compose_rotvec(rot_0, x * scal[..., None])
    p2 = torch.as_tensor(params2).float()
    loc = p2[:, 0].reshape(-1, 1, 1) * (trans_0 * cs)
    trans_t = (torch.as_tensor(z_trans).float() * p2[:, 1].reshape(-1, 1, 1) + loc) / cs
    if diffuse_mask is not None:
        m = torch.as_tensor(diffuse_mask, dtype=trans_t.dtype)[..., None]
        rot_t, trans_t = m * rot_t + (1 - m) * rot_0, m * trans_t + (1 - m) * trans_0
    return G.Frames(trans_t, rot_mats=G.axis_angle_to_matrix(rot_t)).to_tensor_7()


# ----------------------------------------------------------------------------------------------- ensemble statistics
def pairwise_np(ca, offset):
    """Upper-triangular CA distances in numpy's float32 arithmetic, np.triu_indices(L, k=offset) order."""
    x = np.asarray(ca, dtype=np.float32)
    r_, c_ = np.triu_indices(x.shape[-2], k=offset)
    if x.ndim == 3 and x.shape[1] > 700:          # the full L x L x 3 difference of a long chain, one sample at a time
        return np.stack([pairwise_np(s, offset) for s in x])
    d = np.sqrt(np.sum((x[..., None, :, :] - x[..., None, :]) ** 2, axis=-1))
    return d[..., r_, c_]


def sample_stats_np(ca, clash_bar=3.0, k_exclusion=0):
    """-> (n_clash [R] int, adjacent_max [R] float32, radius of gyration [R] float64).  Clashes: float32 distances of the pairs
    |i - j| > k_exclusion strictly below the bar; adjacent: largest float32 CA(i)-CA(i+1) distance; Rg in float64."""
    x = np.asarray(ca, dtype=np.float32)
    L = x.shape[1]
    if L > 1 + k_exclusion:
        n_clash = np.sum(pairwise_np(x, k_exclusion + 1) < np.float32(clash_bar), axis=-1).astype(np.int64)
    else:
        n_clash = np.zeros(x.shape[0], dtype=np.int64)
    adj = np.sqrt(np.sum((x[:, :-1] - x[:, 1:]) ** 2, axis=-1)).max(-1)
    xd = x.astype(np.float64)
    rg = np.sqrt(((xd - xd.mean(1, keepdims=True)) ** 2).sum(-1).mean(-1))
    return n_clash, adj, rg


def js_channels_np(ref_ca, pred_ca, offset=3, n_bins=50, pseudo=1e-6, ref_weights=None, pred_weights=None):
    """Per pair channel: histograms of both ensembles' float32 distances over range=(min, max) of the reference ensemble
    (np.histogram, per-sample float64 weights, ones by default) + pseudo, then the Jensen-Shannon distance -> [D] float64."""
    from scipy.spatial.distance import jensenshannon

    dr, dp = pairwise_np(ref_ca, offset), pairwise_np(pred_ca, offset)
    wr = np.ones(len(dr)) if ref_weights is None else np.asarray(ref_weights, dtype=np.float64)
    wp = np.ones(len(dp)) if pred_weights is None else np.asarray(pred_weights, dtype=np.float64)
    lo, hi = dr.min(axis=0), dr.max(axis=0)
    D = dr.shape[1]
    hr, hp = np.empty((D, n_bins)), np.empty((D, n_bins))   # channel-major in memory, as np.apply_along_axis leaves them
    for c in range(D):
        hr[c] = np.histogram(dr[:, c], bins=n_bins, weights=wr, range=(lo[c], hi[c]))[0] + pseudo
        hp[c] = np.histogram(dp[:, c], bins=n_bins, weights=wp, range=(lo[c], hi[c]))[0] + pseudo
    return jensenshannon(hp.T, hr.T, axis=0)


# ----------------------------------------------------------------------------------------------- seeded inputs
def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def unit_quats(rng, shape):
    """Random unit quaternions rounded to float32."""
    q = rng.normal(size=tuple(shape) + (4,))
    return (q / np.linalg.norm(q, axis=-1, keepdims=True)).astype(np.float32)


def _aa_quat(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis]).astype(np.float32)


SE3_B = 3
SE3_N = (1, 64, 65, 256, 257, 513, 2048)
SE3_DT = 0.01
SE3_DT_VEC = (0.01, 0.02, 0.005)
_BRANCH = {"ode": (True, 1.0), "sde": (False, 1.0), "sde03": (False, 0.3)}
# family -> branch, centre mode, masks, step size.  Masks: "ones"; "prefix" = mask = diffuse_mask = prefixes of length
# (N, ceil(N/2), 1); "frozen" = mask of ones, diffuse_mask freezes a random fifth of the residues.
SE3_FAMILIES = {f"{br}-c{c}": (br, c, "prefix" if c == 2 else "ones", "scalar") for br in _BRANCH for c in (0, 1, 2)}
SE3_FAMILIES.update({"ode-c1-frozen": ("ode", 1, "frozen", "scalar"), "sde-c1-frozen": ("sde", 1, "frozen", "scalar"),
                     "sde03-c2-frozen": ("sde03", 2, "frozen", "scalar"), "ode-c1-dtvec": ("ode", 1, "ones", "vec"),
                     "ode-c2-dtvec": ("ode", 2, "prefix", "vec"), "sde03-c2-dtvec": ("sde03", 2, "prefix", "vec"),
                     "sde-c0-dtvec": ("sde", 0, "ones", "vec")})
FRAME_PLANTS = ("identity", "w<0", "pi-1e-4", "1e-7")
SCORE_PLANTS = (0.0, 1e-8, 3.0)   # size of the planted rotation perturbation, rad


def se3_noise(seed, lengths, N):
    """The float64 normals the float32 chain draws when it is run one sample at a time on that sample's leading ``lengths[b]``
    residues after torch.manual_seed(seed + b): rotation noise first, then translation noise.  Padding keeps other draws."""
    B = len(lengths)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed + 1000)
        z_rot, z_trans = torch.randn(B, N, 3, dtype=F64), torch.randn(B, N, 3, dtype=F64)
        for b, n in enumerate(lengths):
            torch.manual_seed(seed + b)
            z_rot[b, :n] = torch.randn(1, n, 3, dtype=F64)[0]
            z_trans[b, :n] = torch.randn(1, n, 3, dtype=F64)[0]
    return z_rot, z_trans


def se3_case(family, N, diffuser):
    """Seeded inputs of one reverse step, CPU tensors: B = 3 at t = (min_t, 0.37, 1), float32 unit-quaternion frames with
    translations up to +-100 A, rotation scores up to +-30, translation scores of a clean structure 3 A away, and the planted
    frames (identity, w < 0, angle pi - 1e-4, angle 1e-7) and scores (rotation perturbation exactly 0 on the ODE branch and
    cancelled to rounding against the noise on the SDE branch, about 1e-8, about 3 rad) at the head of every sample and,
    from N = 64, mirrored at its tail, which the strided residue loop handles."""
    branch, center, masks, dt_kind = SE3_FAMILIES[family]
    pf, ns = _BRANCH[branch]
    B = SE3_B
    rng = _rng("se3", family, N)
    seed = int(rng.integers(1 << 30))
    t = torch.tensor([float(diffuser.min_t), 0.37, 1.0], dtype=torch.float32)
    p8 = diffuser.step_params(t)
    dt = np.asarray(SE3_DT_VEC if dt_kind == "vec" else (SE3_DT,) * B, dtype=np.float64)
    q = unit_quats(rng, (B, N))
    x = rng.uniform(-100.0, 100.0, size=(B, N, 3)).astype(np.float32)
    rs = rng.uniform(-30.0, 30.0, size=(B, N, 3))
    x0 = x.astype(np.float64) + rng.normal(scale=3.0, size=(B, N, 3))
    eh, cv = p8[:, 2].double().numpy()[:, None, None], p8[:, 3].double().numpy()[:, None, None]
    ts = -(0.1 * x.astype(np.float64) - eh * 0.1 * x0) / cv

    mask, dm = np.ones((B, N), dtype=np.float32), np.ones((B, N), dtype=np.float32)
    lengths = [N] * B
    if masks == "prefix":
        lengths = [N, (N + 1) // 2, 1]
        for b, n in enumerate(lengths):
            mask[b, n:] = 0.0
        dm = mask.copy()
    elif masks == "frozen":
        dm = (rng.uniform(size=(B, N)) >= 0.2).astype(np.float32)
        dm[:, :8] = 1.0   # the planted residues at the head move; their mirror images at the tail take their chance
    z_rot, z_trans = se3_noise(seed, lengths, N)

    def plant(b, n, frame, pert):
        if frame is not None:
            axis = rng.normal(size=3)
            q[b, n] = {"identity": np.array([1, 0, 0, 0], dtype=np.float32), "w<0": -q[b, n] if q[b, n, 0] > 0 else q[b, n],
                       "pi-1e-4": _aa_quat(axis, np.pi - 1e-4), "1e-7": _aa_quat(axis, 1e-7)}[frame]
        if pert is not None:
            axis = rng.normal(size=3)
            want = pert * axis / np.linalg.norm(axis)                   # -(drift + diff) = want
            g2r, gr = float(p8[b, 1]), float(p8[b, 6])
            h = 0.5 if pf else 1.0
            diff = 0.0 if pf else gr * np.sqrt(dt[b]) * ns * z_rot[b, n].numpy()
            rs[b, n] = (want + diff) / (g2r * dt[b] * h)

    for b in range(B):
        if N < 8:
            for n in range(N):
                k = (b + n) % 3
                plant(b, n, FRAME_PLANTS[1:][k], SCORE_PLANTS[::-1][k])
        else:
            for k, f in enumerate(FRAME_PLANTS):
                plant(b, k, f, None)
                if N >= 64:
                    plant(b, N - 1 - k, f, None)
            for k, s in enumerate(SCORE_PLANTS):
                plant(b, 4 + k, None, s)
                if N >= 64:
                    plant(b, N - 5 - k, None, s)
    xt7 = torch.as_tensor(np.concatenate([q, x], -1))
    return dict(family=family, N=N, seed=seed, t=t, p8=p8, xt7=xt7, rot_score=torch.as_tensor(rs), trans_score=torch.as_tensor(ts),
                mask=torch.as_tensor(mask), diffuse_mask=torch.as_tensor(dm), lengths=lengths, center=center, probability_flow=pf,
                noise_scale=ns, dt=torch.as_tensor(dt), dt_kind=dt_kind, z_rot=z_rot, z_trans=z_trans)


def se3_fused_case(family, N, diffuser):
    """se3_case plus a clean structure ``x0`` [B, N, 7] and, in place of the case's given scores, score64's: the inputs and the
    float64 statement of the fused call the sampler makes.  x_0 is x_t turned by 0.05 .. 2 sigma of its sample (3 rad at most)
    about a random axis and moved by 3 A: where a trajectory is, and where the chain's float32 series is well conditioned.
    ``wrapped`` [B, N]: the branch of the chain's float32 product quaternion (score_chain32)."""
    case = se3_case(family, N, diffuser)
    rng = _rng("se3-fused", family, N)
    sigma = case["p8"][:, 0].double().numpy()[:, None]
    theta = np.minimum(rng.uniform(0.05, 2.0, size=(SE3_B, N)) * sigma, 3.0)
    axis = rng.normal(size=(SE3_B, N, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    r_conj = np.concatenate([np.cos(theta / 2)[..., None], -np.sin(theta / 2)[..., None] * axis], -1)
    q0 = quat_mul64(case["xt7"][..., :4], r_conj).numpy()            # R_0^T R_t = rot(theta, axis)
    x0 = np.concatenate([q0, case["xt7"][..., 4:].numpy() + rng.normal(scale=3.0, size=(SE3_B, N, 3))], -1).astype(np.float32)
    case["x0"] = torch.as_tensor(x0)
    case["rot_score"], case["trans_score"] = score64(case["x0"], case["xt7"], case["t"], case["mask"], diffuser)
    case["wrapped"] = score_chain32(case["x0"], case["xt7"], case["p8"], case["mask"])[2] < 0
    return case


def se3_ref64(case, diffuser):
    return reverse_step64(case["xt7"], case["rot_score"], case["trans_score"], case["t"], case["dt"], case["diffuse_mask"], case["mask"],
                          case["center"], case["noise_scale"], case["probability_flow"], case["z_rot"], case["z_trans"], diffuser)


def se3_oracle(case, lengths=None, centers=None):
    """The float32 chain (oracle.diffuser.FrameDiffuser.reverse) on the case, one sample at a time on that sample's leading
    ``lengths[b]`` residues with its own dt and the generator seeded as se3_noise seeds it -> per sample (R [n,3,3], x [n,3])
    float64, R from the normalised quaternion of the returned frame.  A case with ``x0`` (se3_fused_case) takes the chain's
    own scores (FrameDiffuser.score, float32 series and all) in place of the given ones: the whole step.  Where the chain's
    product quaternion is on the wrapped branch its rotation score is the noise the float64 suite exposes and would only widen
    the distance; those residues keep the given (score64's) rotation score and the chain does the rest of the step."""
    from oracle import diffuser as OD
    from oracle.geometry import Frames

    od = OD.FrameDiffuser()
    lengths = case["lengths"] if lengths is None else lengths
    out = []
    for b, n in enumerate(lengths):
        sl = (slice(b, b + 1), slice(0, n))
        center = (case["center"] != 0) if centers is None else centers[b]
        rs, ts = case["rot_score"][sl], case["trans_score"][sl]
        if "x0" in case:
            rs, ts = od.score(Frames.from_tensor_7(case["x0"][sl]), Frames.from_tensor_7(case["xt7"][sl]), case["t"][b:b + 1], case["mask"][sl].double())
            rs = torch.where(case["wrapped"][sl][..., None], case["rot_score"][sl], rs)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(case["seed"] + b)
            nxt = od.reverse(Frames.from_tensor_7(case["xt7"][sl]), rs, ts, case["t"][b:b + 1],
                             float(case["dt"][b]), case["diffuse_mask"][sl].double(), center, case["noise_scale"],
                             case["probability_flow"]).to_tensor_7()[0]
        out.append((quat_rot64(nxt[:, :4]), nxt[:, 4:].double()))
    return out


def rot_trans_error(R, x, R64, x64):
    """(largest matrix-entry difference, largest translation difference / max(1, max |x64|)) of one sample."""
    R, x, R64, x64 = _f64(R), _f64(x), _f64(R64), _f64(x64)
    return float((R - R64).abs().max()), float((x - x64).abs().max() / max(1.0, float(x64.abs().max())))


def se3_oracle_distance(case, diffuser, lengths=None, centers=None):
    """(e_rot, e_trans): how far the float32 chain is from float64 on this case, over the residues the chain was run on."""
    R64, x64 = se3_ref64(case, diffuser)
    e_rot = e_trans = 0.0
    for b, (R, x) in enumerate(se3_oracle(case, lengths, centers)):
        n = R.shape[0]
        er, et = rot_trans_error(R, x, R64[b, :n], x64[b, :n])
        e_rot, e_trans = max(e_rot, er), max(e_trans, et)
    return e_rot, e_trans


@functools.lru_cache(maxsize=None)
def _family_distance(family, diffuser):
    e = [se3_oracle_distance(se3_case(family, N, diffuser), diffuser) for N in SE3_N]
    return max(a for a, _ in e), max(b for _, b in e)


def se3_family_distance(family, diffuser):
    """The float32 chain's distance from float64 over every N of a case family: what a tolerance of that family is built on."""
    return _family_distance(family, diffuser)


def compose_case(M):
    """Frames with quaternions off unit norm by up to 1e-3 and translations up to +-50 A, updates up to 10, a 0/1 mask."""
    rng = _rng("compose", M)
    q = unit_quats(rng, (M,)).astype(np.float64) * (1.0 + rng.uniform(-1e-3, 1e-3, size=(M, 1)))
    r7 = np.concatenate([q, rng.uniform(-50.0, 50.0, size=(M, 3))], -1).astype(np.float32)
    upd = rng.uniform(-10.0, 10.0, size=(M, 6)).astype(np.float32)
    mask = (rng.uniform(size=M) < 0.7).astype(np.float32)
    mask[-1] = 1.0
    if M > 2:
        mask[0] = 0.0
    return torch.as_tensor(r7), torch.as_tensor(upd), torch.as_tensor(mask)


def backbone_case(M):
    """Unit-quaternion frames with translations up to +-500 A, psi as raw (sin, cos) pairs of any length up to 2, the 21
    residue types cycled."""
    rng = _rng("backbone", M)
    r7 = np.concatenate([unit_quats(rng, (M,)), rng.uniform(-500.0, 500.0, size=(M, 3)).astype(np.float32)], -1)
    ang, length = rng.uniform(0, 2 * np.pi, size=M), rng.uniform(0.05, 2.0, size=M)
    psi = np.stack([np.sin(ang) * length, np.cos(ang) * length], -1).astype(np.float32)
    aatype = (np.arange(M) + (7 if M == 1 else 0)) % 21          # a single frame: glycine
    return torch.as_tensor(r7), torch.as_tensor(psi), torch.as_tensor(aatype, dtype=torch.long)


def prior_u(cdf_rows, row_of_sample):
    """float32 uniforms [B, N] aimed at np.interp's branches on each sample's own row: 0, below cdf[0], every interior knot
    (rounded to float32: an exact hit where the knot is a float32), midpoints, 1 - 2^-24, cdf[-1] and above it."""
    cdf = np.asarray(cdf_rows, dtype=np.float64)
    out = []
    for r in row_of_sample:
        row = cdf[int(r)]
        knots = row[1:-1] if len(row) <= 16 else row[[1, 2, 17, 250, 499, 500, 750, 997, 998]]
        mids = 0.5 * (knots[:-1] + knots[1:])
        out.append(np.concatenate([[0.0, row[0] - 0.25, row[0]], knots, mids, [0.3, 0.61803, 1.0 - 2.0 ** -24, row[-1], 1.0, 1.5]]))
    n = min(len(u) for u in out)
    return torch.as_tensor(np.stack([u[:n] for u in out]).astype(np.float32))


def synthetic_cdf_rows():
    """Two rows of 9 knots at (k / 8)^2 and (k / 8)^3, every knot a float32, and a 9-point float32 angle grid."""
    k = np.arange(9, dtype=np.float64) / 8.0
    return torch.as_tensor(np.stack([k ** 2, k ** 3])), torch.linspace(0.0, np.pi, 10)[1:].float().contiguous()


def walk_ensemble(R, L, seed=0, plant=True):
    """CA random walks with 3.8 A steps, float32 [R, L, 3].  Planted into every sample (one pair only when L < 4): residues
    0 and L-1 exactly 3.0 A apart and residues 1 and L-2 one float32 ulp closer than 3.0 A, as numpy's float32 distance sees them."""
    rng = _rng("walk", R, L, seed)
    step = rng.normal(size=(R, L, 3))
    ca = np.cumsum(3.8 * step / np.linalg.norm(step, axis=-1, keepdims=True), axis=1).astype(np.float32)
    if plant:
        below = np.nextafter(np.float32(3.0), np.float32(0.0))
        for s in range(R):
            if L >= 4 or s % 2 == 0:
                ca[s, 0], ca[s, L - 1] = (0.0, 0.0, 0.0), (3.0, 0.0, 0.0)
            if L >= 4:
                ca[s, 1], ca[s, L - 2] = (0.0, 0.0, 64.0), (below, 0.0, 64.0)
            else:
                if s % 2 == 1:
                    ca[s, 0], ca[s, L - 1] = (0.0, 0.0, 0.0), (below, 0.0, 0.0)
    return ca
