"""Attention cores: invariant point attention (fp32 and split-f16 operands) and the encoder's self-attention."""
from typing import Optional

import torch

from .binding import HipLibraryError, _check, _p, _req, _req_all, _req_opt, _stream, _timed, load_library
from .packing import padded_len, xp_alloc
from .range_guard import range_flag


def ipa_prep_points(rigids7, q_pts_lin, kv_pts_lin, n_heads=8, n_qk=8, n_v=12):
    lib = load_library()
    B, N = rigids7.shape[0], rigids7.shape[1]
    _req_all(rigids7=rigids7, q_pts_lin=q_pts_lin, kv_pts_lin=kv_pts_lin)
    dev = rigids7.device
    q_pts = torch.empty(B, N, n_heads, n_qk * 3, device=dev, dtype=torch.float32)
    k_pts = torch.empty(B, N, n_heads, n_qk * 3, device=dev, dtype=torch.float32)
    v_pts = torch.empty(B, N, n_heads, 64, device=dev, dtype=torch.float32)
    _check(lib.s2s_ipa_prep_points(_p(rigids7), _p(q_pts_lin), _p(kv_pts_lin), _p(q_pts), _p(k_pts), _p(v_pts), B * N,
                                   n_heads, n_qk, n_v, 64, _stream()), "s2s_ipa_prep_points")
    return q_pts, k_pts, v_pts


def ipa_attention(q, kv, q_pts, k_pts, v_pts, attn_bias, pair_z, mask, rigids7, head_w_scaled, n_heads=8, c_hidden=256,
                  n_qk=8, n_v=12, c_pz=32, inf=1e5, eps=1e-8, out=None, logits_inplace=False):
    """Attention core + pair term.  ``attn_bias`` is head-major [B,H,N,N] (as ``pair_project`` writes it); with
    ``logits_inplace`` the masked logits overwrite it (the model does not reuse the bias).  Two launches:
    s2s_ipa_attention (o, o_pt, logits, row statistics) and s2s_ipa_opair (streams pair_z once for all heads)."""
    lib = load_library()
    B, N = mask.shape
    _req_all(q=q, kv=kv, q_pts=q_pts, k_pts=k_pts, v_pts=v_pts, attn_bias=attn_bias, pair_z=pair_z, mask=mask, rigids7=rigids7, head_w=head_w_scaled)
    if attn_bias.shape != (B, n_heads, N, N) or pair_z.shape != (B, N, N, c_pz):
        raise HipLibraryError("ipa_attention: attn_bias must be [B,H,N,N] and pair_z [B,N,N,c_pz]")
    feat = n_heads * (c_hidden + 4 * n_v + c_pz)
    out = torch.empty(B, N, feat, device=q.device, dtype=torch.float32) if out is None else out
    logits = attn_bias if logits_inplace else torch.empty_like(attn_bias)
    stats = torch.empty(B, n_heads, N, 2, device=q.device, dtype=torch.float32)

    def launch():   # (the pair term runs only behind a core that launched: rc 0)
        return (lib.s2s_ipa_attention(_p(q), _p(kv), _p(q_pts), _p(k_pts), _p(v_pts), _p(attn_bias), _p(logits), _p(stats), _p(mask),
                                      _p(rigids7), _p(head_w_scaled), _p(out), B, N, n_heads, c_hidden, n_qk, n_v, c_pz, inf, eps, _stream())
                or lib.s2s_ipa_opair(_p(logits), _p(stats), _p(pair_z), _p(out), B, N, n_heads, c_pz, feat, n_heads * (c_hidden + 4 * n_v), N, _stream()))

    _check(_timed("s2s_ipa_attention", launch), "s2s_ipa_attention/s2s_ipa_opair")
    return out


def ipa_prep_points_f16(rigids7, q_pts_lin, kv_pts_lin, head_w_scaled, n_heads=8, n_qk=8, n_v=12, c_hidden=256, s_xp=None):
    """Global-frame points of a block as MFMA fragments (two f16 planes per fragment group) + the squared-norm terms of the logits
    (s2s_ipa_prep_points_f16).  ANY n_res: the arrays hold padded_len(n_res) rows per sample (padded rows: zero points, k2 = -1e9).
    rigids7 [B,N,7].  -> (qp_xp, kp_xp, vp_vf, q2, k2)
    With ``s_xp`` (packed planes of the block's input s [B*N, 256]; folded projections, ``fold_ipa_weights``) the same launch also
    writes the K / V operands every head shares: -> (..., k_shared, v_shared), k_shared = the rows of s_xp gathered into the padded
    per-sample layout (None when n_res % 32 == 0: s_xp itself is the K operand), v_shared = the same values as A fragments."""
    lib = load_library()
    _req_all(rigids7=rigids7, q_pts_lin=q_pts_lin, kv_pts_lin=kv_pts_lin, head_w=head_w_scaled)
    if rigids7.ndim != 3:
        raise HipLibraryError("ipa_prep_points_f16: rigids7 must be [B,N,7]")
    B, N = rigids7.shape[:2]
    dev, rt = rigids7.device, B * padded_len(N) // 32
    qp = torch.empty(rt * n_heads * 2 * 2 * 64 * 8, dtype=torch.int16, device=dev)
    kp = torch.empty_like(qp)
    vp = torch.empty(rt * n_heads * 4 * 2 * 64 * 8, dtype=torch.int16, device=dev)
    q2 = torch.empty(rt, n_heads, 32, dtype=torch.float32, device=dev)
    k2 = torch.empty_like(q2)
    k_sh = v_sh = None
    if s_xp is not None:
        _req(s_xp, torch.int16, "s_xp")
        if s_xp.numel() != ((B * N + 31) // 32) * 32 * 256 * 2:
            raise HipLibraryError("ipa_prep_points_f16: s_xp must hold the packed planes of a [B*N, 256] activation")
        v_sh = torch.empty(rt * 32 * 256 * 2, dtype=torch.int16, device=dev)
        k_sh = None if N % 32 == 0 else torch.empty_like(v_sh)
    _check(lib.s2s_ipa_prep_points_f16(_p(rigids7), _p(q_pts_lin), _p(kv_pts_lin), _p(head_w_scaled), _p(qp), _p(kp), _p(vp), _p(q2),
                                       _p(k2), B, N, n_heads, n_qk, n_v, c_hidden, _p(s_xp), _p(k_sh), _p(v_sh), _p(range_flag()),
                                       _stream()), "s2s_ipa_prep_points_f16")
    return (qp, kp, vp, q2, k2) if s_xp is None else (qp, kp, vp, q2, k2, k_sh, v_sh)


def ipa_attention_f16(q_xp, k_xp, v_vf, points, attn_bias, pair_z, mask, rigids7, n_heads=8, c_hidden=256, n_qk=8, n_v=12,
                      c_pz=32, inf=1e5, eps=1e-8, logits_inplace=False):
    """Attention core on pre-split f16 pair operands + pair term (s2s_ipa_attention_f16w + s2s_ipa_opair), ANY n_res.
    ``points`` = ipa_prep_points_f16(...); for a ragged length the operand arrays hold padded_len(n_res) rows per sample (q/k from
    node_linear(row_map=...), v from node_linear_vfrag(row_map=...)) and the logits get their own padded buffer.
    -> (feats fp32 [B,N,feat] with the o_pt / o_pair columns valid, feats_xp packed planes with the o columns valid); the
    caller packs columns H*c_hidden.. of ``feats`` into ``feats_xp`` (ops.pack_planes) to complete linear_out's input."""
    lib = load_library()
    B, N = mask.shape
    qp, kp, vp, q2, k2 = points
    _req_all(attn_bias=attn_bias, pair_z=pair_z, mask=mask, rigids7=rigids7, q2=q2, k2=k2)
    _req_all(torch.int16, q_xp=q_xp, k_xp=k_xp, v_vf=v_vf, qp_xp=qp, kp_xp=kp, vp_vf=vp)
    NP = padded_len(N)
    if attn_bias.shape != (B, n_heads, N, N) or pair_z.shape != (B, N, N, c_pz):
        raise HipLibraryError("ipa_attention_f16: attn_bias must be [B,H,N,N] and pair_z [B,N,N,c_pz]")
    # K / V arrays of one head's size: one image serves every head (folded projections: both are the block's input s)
    n_kv = 1 if (k_xp.numel() * n_heads == q_xp.numel() and n_heads > 1) else n_heads
    if (q_xp.numel() != B * NP * n_heads * c_hidden * 2 or v_vf.numel() != k_xp.numel() or q2.numel() != B * NP * n_heads
            or k_xp.numel() * (n_heads // n_kv) != q_xp.numel()):
        raise HipLibraryError("ipa_attention_f16: operand arrays do not hold padded_len(n_res) rows per sample")
    feat = n_heads * (c_hidden + 4 * n_v + c_pz)
    out = torch.empty(B, N, feat, device=mask.device, dtype=torch.float32)
    out_xp = xp_alloc(B * N, feat, mask.device)
    if NP != N:
        logits = torch.empty(B, n_heads, NP, NP, device=mask.device, dtype=torch.float32)
    else:
        logits = attn_bias if logits_inplace else torch.empty_like(attn_bias)
    stats = torch.empty(B, n_heads, N, 2, device=mask.device, dtype=torch.float32)

    def launch():   # (the pair term runs only behind a core that launched: rc 0)
        return (lib.s2s_ipa_attention_f16w(_p(q_xp), _p(k_xp), _p(v_vf), _p(qp), _p(kp), _p(vp), _p(q2), _p(k2), _p(attn_bias), _p(logits),
                                           _p(stats), _p(mask), _p(rigids7), _p(out), _p(out_xp), feat // 16, B, N, n_heads, c_hidden,
                                           n_qk, n_v, c_pz, inf, eps, n_kv, _stream())
                or lib.s2s_ipa_opair(_p(logits), _p(stats), _p(pair_z), _p(out), B, N, n_heads, c_pz, feat, n_heads * (c_hidden + 4 * n_v), NP, _stream()))

    _check(_timed("s2s_ipa_attention", launch), "s2s_ipa_attention_f16w/s2s_ipa_opair")
    return out, out_xp


def encoder_attention(qkv: torch.Tensor, key_bias: Optional[torch.Tensor], n_samples: int, n_res: int, n_heads: int = 4,
                      want_f32: bool = False, want_xp: bool = True, arith: str = "f32"):
    """Self-attention core of one encoder layer on the in_proj output qkv [B*N, 3*D] -> (fp32 [B*N, D] or None, packed planes or
    None).  ``key_bias`` [B,N] is added to the logits of key j (None = zeros).  ``arith``: "f32" = exact fp32 MFMA, "f16x3" = split-f16
    MFMA (str2str_amd/arith.py)."""
    lib = load_library()
    _req(qkv, name="qkv")
    M, D3 = qkv.shape
    D = D3 // 3
    if M != n_samples * n_res or D % n_heads:
        raise HipLibraryError("encoder_attention: bad shapes")
    _req_opt(key_bias=key_bias)
    out = torch.empty(M, D, device=qkv.device, dtype=torch.float32) if want_f32 else None
    oxp = xp_alloc(M, D, qkv.device) if want_xp else None
    if arith not in ("f32", "f16x3"):
        raise HipLibraryError(f"encoder_attention: arith {arith!r}")
    fn = lib.s2s_encoder_attention_f16x3 if arith == "f16x3" else lib.s2s_encoder_attention
    rw = _p(range_flag()) if want_xp or arith == "f16x3" else None   # (the fp32 kernel splits only what it writes to out_xp)
    _check(_timed("s2s_encoder_attention", lambda: fn(_p(qkv), _p(key_bias), _p(out), _p(oxp), n_samples, n_res, n_heads, D // n_heads,
                                                      rw, _stream())), "s2s_encoder_attention")
    return out, oxp
