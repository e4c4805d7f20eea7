"""Frames and diffusion geometry: rigid updates, torsion head, backbone atoms, the SE(3) step and the forward marginal."""
import numpy as np
import torch

from .binding import HipLibraryError, _check, _p, _req, _req_all, _req_opt, _stream, _vp, load_library

_tables_loaded = set()   # device indices that hold the backbone tables


def rigid_compose_update(rigids7, update6, mask, out=None):
    """``update6``: [..., 6] contiguous, or a 2-D [n_frames, ld >= 6] fp32 buffer whose leading six columns are the update (the
    BackboneUpdate layer's padded output, read in place)."""
    lib = load_library()
    _req_all(rigids7=rigids7, update6=update6, mask=mask)
    n = rigids7.numel() // 7
    ld = update6.shape[-1] if (update6.ndim == 2 and update6.shape[0] == n) else 6
    if ld < 6 or update6.numel() != n * ld:
        raise HipLibraryError("rigid_compose_update: update6 must be [..., 6] or [n_frames, ld >= 6]")
    out = torch.empty_like(rigids7) if out is None else out
    _check(lib.s2s_rigid_compose_update(_p(rigids7), _p(update6), _p(mask), _p(out), n, ld, _stream()), "s2s_rigid_compose_update")
    return out


def torsion_head(u, n_rows: int, normalize: bool = True, eps: float = 1e-8, gt_sin_cos=None, fixed_mask=None):
    """psi [n_rows, 2] from the torsion head's raw output ``u`` (2-D, leading two columns; normalised when ``normalize``) and, with
    ``gt_sin_cos`` (a [.., 2] view whose rows are ``gt_sin_cos.stride(-2)`` floats apart) + ``fixed_mask`` [n_rows], blended with the
    input torsion (s2s_torsion_head)."""
    lib = load_library()
    _req(u, name="u")
    if u.ndim != 2 or u.shape[0] != n_rows or u.shape[1] < 2:
        raise HipLibraryError("torsion_head: u must be [n_rows, ld >= 2]")
    gs = 0
    if gt_sin_cos is not None:
        if gt_sin_cos.dtype != torch.float32 or not gt_sin_cos.is_cuda or gt_sin_cos.shape[-1] != 2 or gt_sin_cos.stride(-1) != 1:
            raise HipLibraryError("torsion_head: gt_sin_cos must be a float32 device tensor [..., 2]")
        gs = 2 if gt_sin_cos.is_contiguous() else gt_sin_cos.stride(-2)
        if not gt_sin_cos.is_contiguous() and any(gt_sin_cos.stride(d) != gt_sin_cos.stride(d + 1) * gt_sin_cos.shape[d + 1]
                                                  for d in range(gt_sin_cos.ndim - 2)):
            raise HipLibraryError("torsion_head: gt_sin_cos rows must be evenly strided")
        _req(fixed_mask, name="fixed_mask")
    out = torch.empty(n_rows, 2, device=u.device, dtype=torch.float32)
    _check(lib.s2s_torsion_head(_p(u), u.shape[1], int(bool(normalize)), _p(gt_sin_cos), gs, _p(fixed_mask), float(eps), _p(out), n_rows,
                                _stream()), "s2s_torsion_head")
    return out


def rigid_scale_trans(rigids7, scale: float, divide: bool = False, out=None):
    lib = load_library()
    _req(rigids7, name="rigids7")
    out = torch.empty_like(rigids7) if out is None else out
    _check(lib.s2s_rigid_scale_trans(_p(rigids7), _p(out), rigids7.numel() // 7, scale, int(divide), _stream()), "s2s_rigid_scale_trans")
    return out


def _ensure_tables():
    dev = torch.cuda.current_device()
    if dev in _tables_loaded:
        return
    from ..data import backbone_tables as bt

    lib = load_library()
    pos = np.ascontiguousarray(bt.BB_POS, dtype=np.float32)
    msk = np.ascontiguousarray(bt.BB_MASK, dtype=np.float32)
    grp = np.ascontiguousarray((bt.BB_GROUP == 3).astype(np.int32))
    frm = np.ascontiguousarray(bt.BB_FRAMES, dtype=np.float32)
    _check(lib.s2s_set_backbone_tables(pos.ctypes.data_as(_vp), msk.ctypes.data_as(_vp), grp.ctypes.data_as(_vp),
                                       frm.ctypes.data_as(_vp)), "s2s_set_backbone_tables")
    _tables_loaded.add(dev)


def frames_to_backbone(rigids7, psi, aatype=None, want_atom37=True, want_atom14=False):
    lib = load_library()
    _req_all(rigids7=rigids7, psi=psi)
    _req_opt(torch.int64, aatype=aatype)
    _ensure_tables()
    lead, dev = rigids7.shape[:-1], rigids7.device
    a37 = torch.empty(*lead, 37, 3, device=dev, dtype=torch.float32) if want_atom37 else None
    a14 = torch.empty(*lead, 5, 3, device=dev, dtype=torch.float32) if want_atom14 else None
    _check(lib.s2s_frames_to_backbone(_p(rigids7), _p(psi), _p(aatype), _p(a14), _p(a37), rigids7.numel() // 7, _stream()), "s2s_frames_to_backbone")
    return a37, a14


def se3_step(x0_7, xt_7, mask, diffuse_mask, params8, dt, coordinate_scaling: float = 0.1, probability_flow=True,
             center=True, noise_scale: float = 1.0, z_rot=None, z_trans=None, want_next=True, want_scores=False, rot_score_in=None, trans_score_in=None):
    """``dt``: the trajectory's step size (a float), or a float64 device tensor [B] with one step size per sample (a batch that holds
    trajectories of different t_delta)."""
    lib = load_library()
    B, N = mask.shape
    dt_vec = None
    if torch.is_tensor(dt):
        dt_vec = _req(dt, torch.float64, "dt")
        if dt_vec.shape != (B,):
            raise HipLibraryError("se3_step: a per-sample dt must be [B] float64")
        dt = 0.0
    _req_all(xt_7=xt_7, mask=mask, diffuse_mask=diffuse_mask, params8=params8)
    if rot_score_in is not None:
        _req_all(torch.float64, rot_score_in=rot_score_in, trans_score_in=trans_score_in)
    else:
        _req(x0_7, name="x0_7")
    if params8.shape != (B, 8):
        raise HipLibraryError("params8 must be [B, 8]")
    if not probability_flow:
        _req_all(torch.float64, z_rot=z_rot, z_trans=z_trans)
    dev = xt_7.device
    nxt = torch.empty(B, N, 7, device=dev, dtype=torch.float32) if want_next else None
    rs = torch.empty(B, N, 3, device=dev, dtype=torch.float64) if want_scores else None
    ts = torch.empty(B, N, 3, device=dev, dtype=torch.float64) if want_scores else None
    _check(lib.s2s_se3_step(_p(x0_7), _p(xt_7), _p(mask), _p(diffuse_mask), _p(params8), _p(z_rot), _p(z_trans), _p(rot_score_in),
                            _p(trans_score_in), _p(nxt), _p(rs), _p(ts), B, N, float(dt), _p(dt_vec), float(coordinate_scaling),
                            int(bool(probability_flow)), int(center), float(noise_scale), _stream()), "s2s_se3_step")
    return nxt, rs, ts


def forward_marginal(rigids0_4x4, z_axis, u01, z_trans, cdf_rows, row_of_sample, omega_grid, params2, diffuse_mask=None, coordinate_scaling: float = 0.1):
    """Forward marginal (``rigids0_4x4`` [B,N,4,4]) or prior sample (``None``) from caller-drawn noise -> rigids_t7 [B,N,7]."""
    lib = load_library()
    B, N = u01.shape
    _req_all(z_axis=z_axis, u01=u01, z_trans=z_trans, omega_grid=omega_grid)
    _req(cdf_rows, torch.float64, "cdf_rows"); _req(row_of_sample, torch.int32, "row_of_sample")
    if z_axis.shape != (B, N, 3) or z_trans.shape != (B, N, 3) or cdf_rows.ndim != 2 or cdf_rows.shape[1] != omega_grid.numel() \
            or row_of_sample.shape != (B,):
        raise HipLibraryError("forward_marginal: bad shapes")
    if rigids0_4x4 is not None:
        _req_all(rigids0_4x4=rigids0_4x4, params2=params2)
        if rigids0_4x4.shape != (B, N, 4, 4) or params2.shape != (B, 2):
            raise HipLibraryError("forward_marginal: rigids0_4x4 must be [B,N,4,4] and params2 [B,2]")
    _req_opt(diffuse_mask=diffuse_mask)
    out = torch.empty(B, N, 7, device=u01.device, dtype=torch.float32)
    _check(lib.s2s_forward_marginal(_p(rigids0_4x4), _p(z_axis), _p(u01), _p(z_trans), _p(cdf_rows), _p(row_of_sample),
                                    _p(omega_grid), omega_grid.numel(), _p(params2), _p(diffuse_mask), float(coordinate_scaling),
                                    _p(out), B, N, _stream()), "s2s_forward_marginal")
    return out
