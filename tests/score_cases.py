"""Seeded case tables, measures and bounds of the SE(3) score and of the noising branch of the forward marginal, shared by
tests/test_ref64_cpu.py (the table's properties, the float32 chain's distance, planted mistakes) and
tests/test_geometry_parity.py (the HIP kernels).  Pure data and float64 / float32 CPU arithmetic (tests/ref64.py).

Score.  B = 3 at t = (min_t, 0.37, 1.0); a *band* is one planted relative angle theta of R_0^T R_t, laid along the residues
(residue n of sample b holds band (n + 4 b) mod 11 and orientation class ((n + 4 b) div 11) mod 16), so one launch per N covers
every band; a *family* is (band, sample).  Every residue carries the branch the reference's float32 chain takes there (real
part of its product quaternion >= 0: principal, < 0: wrapped).  Measure: per family, the largest absolute error of the score
vector against ref64.score64, principal and wrapped residues apart.  Bound for both: 3 x D32, D32 = the distance of the float32
chain (ref64.score_chain32: oracle.geometry in float32 for v, the series in float64) from score64 on the PRINCIPAL residues of
the family over every N of the table.  The quantity does not depend on the representative of the product quaternion, so the
wrapped residues get the principal bound; a D32 taken on the wrapped branch would be the noise it is there to expose.

Forward marginal.  B = 3 with row_of_sample = (1, 0, 1) and params2 at t = (min_t, 0.37, 1.0).  Measure: rotation-matrix entries
and translations over the sample scale (ref64.rot_trans_error) against ref64.forward_marginal64.  Bound: 3 x the distance of
ref64.forward_marginal_chain32 from it on the same draws, pooled per N, never above the project's per-op 5e-6.
"""
import functools

import numpy as np
import torch

import ref64

# ----------------------------------------------------------------------------------------------- score
SCORE_B = 3
SCORE_N = (1, 64, 65, 257, 513, 2048)
SCORE_THETA = (0.0, 1e-6, 1e-4, 1e-3, 1e-2, 0.1, 1.0, 2.0, 3.0, np.pi - 1e-3, np.pi - 1e-5)
SCORE_BAND = ("0", "1e-6", "1e-4", "1e-3", "1e-2", "0.1", "1", "2", "3", "pi-1e-3", "pi-1e-5")
# orientation classes of x_t: the largest quaternion component (by magnitude) and the sign of w; "a~-b": the two largest
# components within 1e-3 of each other with opposite signs, so that x_0 and x_t pick different candidates of the matrix ->
# quaternion conversion.  The classes with w largest are listed three times: the float32 chain is principal there at small
# angles and wrapped on most others, and every band must hold both branches.
SCORE_CLASSES = ("w+", "w-", "w+", "w-", "w+", "w-", "x+", "x-", "y+", "y-", "z+", "z-", "w~-x", "y~-z", "x~-z", "w~-y")
SCORE_MASKS = ("full", "gaps", "prefix")     # of samples 0, 1, 2
_COMP = {"w": 0, "x": 1, "y": 2, "z": 3}


def score_t(diffuser):
    return torch.tensor([float(diffuser.min_t), 0.37, 1.0], dtype=torch.float32)


def _class_quat(rng, cls):
    """A float64 unit quaternion of the orientation class."""
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    if "~" in cls:
        i, j = _COMP[cls[0]], _COMP[cls[-1]]
        rest = [k for k in range(4) if k not in (i, j)]
        a = rng.uniform(0.6, 0.7)
        q[i], q[j] = a, -(a - rng.uniform(-1e-3, 1e-3))
        r = rng.normal(size=2)
        q[rest] = r / np.linalg.norm(r) * np.sqrt(1.0 - q[i] ** 2 - q[j] ** 2)   # at most 0.53: below the pair
        return q
    c = _COMP[cls[0]]
    k = int(np.argmax(np.abs(q)))
    q[[c, k]] = q[[k, c]]
    q[0] = abs(q[0]) if cls[1] == "+" else -abs(q[0])
    if abs(q[0]) < 1e-2:                          # keep the sign of w meaningful
        q[0] = 1e-2 if cls[1] == "+" else -1e-2
        q /= np.linalg.norm(q)
    return q


def _qmul(p, q):
    a1, b1, c1, d1 = p
    a2, b2, c2, d2 = q
    return np.array([a1 * a2 - b1 * b2 - c1 * c2 - d1 * d2, a1 * b2 + b1 * a2 + c1 * d2 - d1 * c2,
                     a1 * c2 - b1 * d2 + c1 * a2 + d1 * b2, a1 * d2 + b1 * c2 - c1 * b2 + d1 * a2])


@functools.lru_cache(maxsize=None)
def _score_case(N, diffuser):
    rng = ref64._rng("score", N)
    B = SCORE_B
    t = score_t(diffuser)
    p8 = diffuser.step_params(t)
    x0 = np.empty((B, N, 7), dtype=np.float32)
    xt = np.empty((B, N, 7), dtype=np.float32)
    band = np.empty((B, N), dtype=np.int64)
    cls = np.empty((B, N), dtype=np.int64)
    for b in range(B):
        for n in range(N):
            k = n + 4 * b
            band[b, n], cls[b, n] = k % len(SCORE_THETA), (k // len(SCORE_THETA)) % len(SCORE_CLASSES)
            qt = _class_quat(rng, SCORE_CLASSES[cls[b, n]])
            theta = SCORE_THETA[band[b, n]]
            axis = rng.normal(size=3)
            axis /= np.linalg.norm(axis)
            r_conj = np.concatenate([[np.cos(theta / 2)], -np.sin(theta / 2) * axis])
            xt[b, n, :4] = qt
            # R_0^T R_t = rot(theta, axis): q_0 = q_t (x) conj(r); theta = 0 is x_0 bit-equal to x_t
            x0[b, n, :4] = xt[b, n, :4] if theta == 0.0 else _qmul(qt, r_conj)
    xt[..., 4:] = rng.uniform(-300.0, 300.0, size=(B, N, 3))
    x0[..., 4:] = xt[..., 4:] + rng.normal(scale=3.0, size=(B, N, 3))
    x0[..., 4:] = np.clip(x0[..., 4:], -300.0, 300.0)

    mask = np.ones((B, N), dtype=np.float32)
    mask[1] = (rng.uniform(size=N) >= 0.2).astype(np.float32)
    if N == 1:
        mask[1] = 0.0
    mask[2, N - N // 4:] = 0.0
    off = mask == 0                               # masked residues hold finite garbage: quaternions of norm 0.5 .. 2, far translations
    n_off = int(off.sum())
    g = rng.normal(size=(n_off, 4))
    g *= (rng.uniform(0.5, 2.0, size=(n_off, 1)) / np.linalg.norm(g, axis=-1, keepdims=True))
    for a, far in ((x0, 1e4), (xt, 3e3)):
        a[off] = np.concatenate([g * rng.choice([-1.0, 1.0]), rng.uniform(-far, far, size=(n_off, 3))], -1).astype(np.float32)
        g = g[::-1]
    x0, xt, mask = torch.as_tensor(x0), torch.as_tensor(xt), torch.as_tensor(mask)
    _, _, w = ref64.score_chain32(x0, xt, p8, mask)
    return dict(N=N, t=t, p8=p8, x0=x0, xt=xt, mask=mask, band=torch.as_tensor(band), cls=torch.as_tensor(cls), wrapped=w < 0)


def score_case(N, diffuser):
    """Inputs of one score launch, CPU tensors (shared: do not modify): x0, xt [3, N, 7] float32 (unit quaternions to float32
    rounding, translations up to +-300 A, x_0 about 3 A from x_t), mask [3, N] (sample 0 full, 1 with gaps, 2 a prefix),
    band / cls [3, N] indices into SCORE_THETA / SCORE_CLASSES, wrapped [3, N] = the branch of the reference's float32 chain."""
    return _score_case(N, diffuser)


@functools.lru_cache(maxsize=None)
def score_ref64(N, diffuser):
    c = score_case(N, diffuser)
    return ref64.score64(c["x0"], c["xt"], c["t"], c["mask"], diffuser)


def score_family_errors(rot, N, diffuser, which):
    """Largest |rot - score64| over the unmasked residues of every (band, sample) on branch ``which`` ("principal" / "wrapped")
    -> [bands, B] float64, NaN where a family has no such residue at this N."""
    c = score_case(N, diffuser)
    err = (ref64._f64(rot) - score_ref64(N, diffuser)[0]).abs().amax(-1)
    sel = (c["mask"] > 0) & (c["wrapped"] if which == "wrapped" else ~c["wrapped"])
    out = torch.full((len(SCORE_THETA), SCORE_B), float("nan"), dtype=torch.float64)
    for k in range(len(SCORE_THETA)):
        for b in range(SCORE_B):
            s = sel[b] & (c["band"][b] == k)
            if s.any():
                out[k, b] = err[b][s].max()
    return out


def trans_sample_errors(trans, N, diffuser):
    """Largest |trans - score64's translation score| per sample -> [B] float64."""
    return (ref64._f64(trans) - score_ref64(N, diffuser)[1]).abs().amax(dim=(1, 2))


def _nanmax(ts):
    return torch.stack([torch.nan_to_num(x, nan=-1.0) for x in ts]).amax(0)


@functools.lru_cache(maxsize=None)
def score_d32(diffuser):
    """(D32 [bands, B], D32 of the translation score [B]): the float32 chain's distance from score64 on the principal residues
    of each family, and per sample for translations, over every N of the table."""
    rot, trans = [], []
    for N in SCORE_N:
        c = score_case(N, diffuser)
        r, tr, _ = ref64.score_chain32(c["x0"], c["xt"], c["p8"], c["mask"])
        rot.append(score_family_errors(r, N, diffuser, "principal"))
        trans.append(trans_sample_errors(tr, N, diffuser))
    d = _nanmax(rot)
    assert (d >= 0).all(), "a family without a principal residue"
    return d, torch.stack(trans).amax(0)


def score_magnitude(theta, sigma):
    """score64's magnitude at relative angle theta: df / (f + 1e-4) * theta / (theta + 2e-6) at omega = theta + 1e-6 (numpy)."""
    theta, sigma = np.broadcast_arrays(np.asarray(theta, dtype=np.float64), np.asarray(sigma, dtype=np.float64))
    f, df = ref64.igso3_series64(theta + 1e-6, sigma)
    return df / (f + 1e-4) * theta / (theta + 2e-6)


def score_jacobian(theta, sigma, h=1e-7):
    """The norm of the Jacobian of v -> s(|v|) v / |v| at |v| = theta: the larger of |d s / d omega| along v (central
    difference, one-sided at theta = 0) and s / theta across it."""
    theta, sigma = np.broadcast_arrays(np.asarray(theta, dtype=np.float64), np.asarray(sigma, dtype=np.float64))
    lo = np.maximum(theta - h, 0.0)
    radial = np.abs(score_magnitude(theta + h, sigma) - score_magnitude(lo, sigma)) / (theta + h - lo)
    return np.maximum(radial, np.abs(score_magnitude(theta, sigma)) / np.maximum(theta, 1e-6))


def score_conditioning(diffuser):
    """(J [bands, B], E64 [bands, B]) of every family at its planted angle and the sample's sigma.

    J = score_jacobian: 2e-6 J is what an error of 2e-6 rad in the float32 chain's rotation vector may cost.  (The radial
    derivative alone does not bound it: at sigma = 1.5, theta = 2 the score's magnitude is at its maximum, d s / d omega = 9e-3,
    and the chain's 9.7e-8 is the error of v's direction times s / theta = 0.27.)

    E64 = the first-order float64 rounding of the two sums themselves, u sum_l (|term_l| + |x_l d term_l / d x_l|) / |f + 1e-4|
    with x_l = omega (l + 1/2) and u = 2^-53: where sigma = 0.1 and theta >= 2 the density is e^-200 and below, f + 1e-4 is
    1e-4, and score64 -- like any float64 evaluation of the formula -- is rounding noise of 1e-8: the chain's distance there is
    the difference of two such evaluations and no derivative explains it."""
    sig = diffuser.step_params(score_t(diffuser))[:, 0].double().numpy()
    th = np.asarray(SCORE_THETA)
    s = score_magnitude(th[:, None], sig[None, :])
    f = ref64.igso3_series64(th[:, None] + 1e-6, sig[None, :])[0]
    J = score_jacobian(th[:, None], sig[None, :])
    ls = np.arange(1000, dtype=np.float64)
    E = np.empty_like(s)
    for k, o in enumerate(th + 1e-6):
        for b, e in enumerate(sig):
            w = (2 * ls + 1) * np.exp(-ls * (ls + 1) * e ** 2 / 2)
            x = o * (ls + 0.5)
            sn, cn, lo, dlo = np.abs(np.sin(x)), np.abs(np.cos(x)), np.sin(o / 2), 0.5 * np.cos(o / 2)
            t_df = w * ((lo * (ls + 0.5) * cn + sn * abs(dlo)) + x * (lo * (ls + 0.5) * sn + cn * abs(dlo))) / lo ** 2
            t_f = w * (sn + x * cn) / lo
            E[k, b] = 2.0 ** -53 * (t_df.sum() + abs(s[k, b]) * t_f.sum()) / abs(f[k, b] + 1e-4)
    return torch.as_tensor(J), torch.as_tensor(E)


def family_label(k, b):
    return f"theta={SCORE_BAND[k]}, t[{b}]"


# ----------------------------------------------------------------------------------------------- forward marginal, noising branch
FM_B = 3
FM_N = (1, 255, 257, 600)
FM_ROWS = (1, 0, 1)
FM_CAP = 5e-6
PI_CROSS = (-1e-2, -1e-4, 1e-6, 1e-4, 1e-2)   # R_0's angle + the drawn angle about the same axis, minus pi


def fm_tables(diffuser):
    """The diffuser's 1000-knot CDF rows of t = 0.05 and t = 1 (float64) and its float32 angle grid."""
    sd = diffuser.rot_diffuser
    idx = [int(sd.t_to_idx(torch.tensor([t]))[0]) for t in (0.05, 1.0)]
    return torch.as_tensor(np.stack([sd.cdf_row(i) for i in idx]), dtype=torch.float64), sd.discrete_omega.float().contiguous()


def fm_params2(diffuser):
    """(e_half, std) per sample at t = (min_t, 0.37, 1.0), as FrameDiffuser.forward_marginal_device forms them."""
    mb = diffuser.trans_diffuser.marginal_b_t(score_t(diffuser))
    return torch.stack([torch.exp(-0.5 * mb), torch.sqrt(1 - torch.exp(-mb))], dim=-1).float().contiguous()


def _rot_matrix(axis, angle):
    return np.asarray(ref64.rotvec_exp64(torch.as_tensor(np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis) * angle)))


@functools.lru_cache(maxsize=None)
def _fm_case(N, diffuser):
    rng = ref64._rng("forward-marginal", N)
    B = FM_B
    cdf, omega = fm_tables(diffuser)
    u_plants = ref64.prior_u(cdf, FM_ROWS).numpy()             # [B, n_u] on np.interp's branches
    n_u = u_plants.shape[1]
    z_axis = rng.normal(size=(B, N, 3)).astype(np.float32)
    z_trans = rng.normal(size=(B, N, 3)).astype(np.float32)
    u = rng.uniform(size=(B, N)).astype(np.float32)
    R0 = np.asarray(ref64.quat_rot64(ref64.unit_quats(rng, (B, N))))
    x0 = rng.uniform(-100.0, 100.0, size=(B, N, 3))
    plants = []
    for b in range(B):
        for n in range(N):
            k = (n + 5 * b) % (n_u + len(ref64.FRAME_PLANTS) + len(PI_CROSS) + 7)
            if k < n_u:                                        # a uniform on one of np.interp's branches
                u[b, n] = u_plants[b, k]
                plants.append((b, n, "u", None))
            elif k < n_u + len(ref64.FRAME_PLANTS):            # a planted R_0
                f = ref64.FRAME_PLANTS[k - n_u]
                axis = rng.normal(size=3)
                q = {"identity": np.array([1.0, 0, 0, 0]), "w<0": None, "pi-1e-4": ref64._aa_quat(axis, np.pi - 1e-4),
                     "1e-7": ref64._aa_quat(axis, 1e-7)}[f]
                if q is not None:                              # ("w<0" has no meaning for a matrix: a random frame stays)
                    R0[b, n] = np.asarray(ref64.quat_rot64(q))
                plants.append((b, n, f, None))
            elif k < n_u + len(ref64.FRAME_PLANTS) + len(PI_CROSS):   # R_0 and the draw about one axis, their angles adding to pi + d
                d = PI_CROSS[k - n_u - len(ref64.FRAME_PLANTS)]
                drawn = float(np.interp(np.float64(u[b, n]), cdf[FM_ROWS[b]].numpy(), omega.double().numpy()))
                R0[b, n] = _rot_matrix(z_axis[b, n].astype(np.float64), np.pi + d - drawn)
                plants.append((b, n, "pi", d))
    g = np.zeros((B, N, 4, 4))
    g[..., :3, :3], g[..., :3, 3], g[..., 3, 3] = R0, x0, 1.0
    dm = (rng.uniform(size=(B, N)) >= 0.2).astype(np.float32)
    if N == 1:
        dm[:, 0] = (1.0, 0.0, 1.0)
    return dict(N=N, rig0=torch.as_tensor(g.astype(np.float32)), z_axis=torch.as_tensor(z_axis), u=torch.as_tensor(u),
                z_trans=torch.as_tensor(z_trans), cdf=cdf, omega=omega, rows=FM_ROWS, params2=fm_params2(diffuser),
                diffuse_mask=torch.as_tensor(dm), plants=tuple(plants))


def fm_case(N, diffuser):
    """Inputs of one noising launch, CPU tensors (shared: do not modify): 4 x 4 frames rounded to float32 (so not exactly
    orthonormal) with translations up to +-100 A, noise with the uniforms of ref64.prior_u, the frames of ref64.FRAME_PLANTS and
    the pi crossings cycled along the residues, a diffuse_mask that freezes a fifth of the residues."""
    return _fm_case(N, diffuser)


def fm_args(c, **over):
    a = dict(rig0_4x4=c["rig0"], z_axis=c["z_axis"], u=c["u"], z_trans=c["z_trans"], cdf_rows=c["cdf"], row_of_sample=c["rows"],
             omega_grid=c["omega"], params2=c["params2"], diffuse_mask=c["diffuse_mask"])
    a.update(over)
    return a


@functools.lru_cache(maxsize=None)
def fm_ref64(N, diffuser):
    return ref64.forward_marginal64(**fm_args(fm_case(N, diffuser)))


def fm_errors(out7, N, diffuser):
    """(rotation-matrix entries, translations / sample scale) of frames [B, N, 7] against forward_marginal64, worst sample."""
    R64, x64 = fm_ref64(N, diffuser)
    out7 = torch.as_tensor(out7).cpu()
    e = [ref64.rot_trans_error(ref64.quat_rot64(out7[b, :, :4]), out7[b, :, 4:], R64[b], x64[b]) for b in range(out7.shape[0])]
    return max(a for a, _ in e), max(b for _, b in e)


@functools.lru_cache(maxsize=None)
def fm_d32(N, diffuser):
    """The float32 chain's distance from forward_marginal64 on the case of this N: (rotation, translation)."""
    return fm_errors(ref64.forward_marginal_chain32(**fm_args(fm_case(N, diffuser))), N, diffuser)


def fm_bounds(N, diffuser):
    e_rot, e_trans = fm_d32(N, diffuser)
    return min(3 * e_rot, FM_CAP), min(3 * e_trans, FM_CAP)
