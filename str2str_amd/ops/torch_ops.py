"""``torch.ops.str2str_amd.*``: the schemas, and the adapters between their flat argument lists and the wrappers."""
import torch

from .attention import encoder_attention, ipa_attention, ipa_attention_f16, ipa_prep_points, ipa_prep_points_f16
from .binding import _opt_int
from .geometry import forward_marginal, frames_to_backbone, rigid_compose_update, rigid_scale_trans, se3_step, torsion_head
from .node import (embed_assemble, ipa_projections, node_chain, node_linear, node_linear_f32, node_linear_multi, node_linear_vfrag, pack_planes,
                   row_layernorm)
from .packing import PairByClass, PairTiled
from .pair import edge_embed, edge_embed_classes_f16x3, edge_embed_f16x3, edge_transition, edge_transition_f16x3, pair_project

_registered = False   # rebound by register_torch_ops: read it there only


def _ln3(g, b, eps):
    return None if g is None else (g, b, eps)


# (the dispatcher passes positional arguments up to the last one the caller gave: the implementations carry the schema's defaults)
def _op_node_linear(xp, wpk, bias, n_rows, k_in, n_out, tiles, pre_scale=None, relu=False, pre_mask=None, residual=None, ln_gamma=None,
                    ln_beta=None, ln_eps=0.0, post_mask=None, out_f32=None, out_col0=0, want_f32=True, out_xp=None, out_xp_k=-1,
                    out_xp_k0=0, want_xp=False, map_pad=0, map_src=0):
    return node_linear(xp, wpk, bias, n_rows, k_in, n_out, tiles, pre_scale=pre_scale, relu=relu, pre_mask=pre_mask, residual=residual,
                       ln=_ln3(ln_gamma, ln_beta, ln_eps), post_mask=post_mask, out_f32=out_f32, out_col0=out_col0, want_f32=want_f32,
                       out_xp=out_xp, out_xp_k=_opt_int(out_xp_k), out_xp_k0=out_xp_k0, want_xp=want_xp,
                       row_map=(map_pad, map_src) if map_pad else None)


def _op_node_linear_f32(x, wpk32, bias, n_rows, k_in, n_out, tiles, pre_scale=None, relu=False, pre_mask=None, residual=None, ln_gamma=None,
                        ln_beta=None, ln_eps=0.0, post_mask=None, out=None, out_col0=0):
    return node_linear_f32(x, wpk32, bias, n_rows, k_in, n_out, tiles, pre_scale=pre_scale, relu=relu, pre_mask=pre_mask,
                           residual=residual, ln=_ln3(ln_gamma, ln_beta, ln_eps), post_mask=post_mask, out=out, out_col0=out_col0)


def _op_edge_transition_f16x3_chain(edge, in_tiled, B, N, node_ab, node_p, wstream, b2, gamma, beta, mask, ln_eps, proj_bias64,
                                    out_layout, prescale_exp=0, ab_kernel_form=False, in_rec=0):
    """The trunk's form of the edge transition: pair tensor in either layout (``edge`` = the flat tiled buffer when ``in_tiled``; the
    flat buffer of a ``PairByClass`` with records of ``in_rec`` floats when that is not 0), the
    next IPA block's projections fused in when ``proj_bias64`` is given (``wstream`` is then the 31-stage stream).
    -> (pair tensor (row-major [B,N,N,128] | flat tiled buffer | None), attn_bias | None, pair_z | None)"""
    e = PairByClass(B, N, edge, in_rec) if in_rec else (PairTiled(B, N, buf=edge) if in_tiled else edge)
    r = edge_transition_f16x3(e, node_ab, node_p, wstream, b2, gamma, beta, mask, ln_eps,
                              proj=None if proj_bias64 is None else (wstream, proj_bias64), out_layout=out_layout, prescale_exp=prescale_exp,
                              ab_kernel_form=ab_kernel_form)
    z, bias, pz = r if proj_bias64 is not None else (r, None, None)
    return (z.buf if isinstance(z, PairTiled) else z), bias, pz


_TORCH_OPS = {
    # ---- pair stream
    "edge_transition(Tensor edge, Tensor node_ab, Tensor node_p, Tensor w1p, Tensor w2p, Tensor wfp, Tensor b2, "
    "Tensor bf, Tensor gamma, Tensor beta, Tensor? mask, float ln_eps) -> Tensor": lambda *a: edge_transition(*a),
    "edge_transition_f16x3(Tensor edge, Tensor node_ab, Tensor node_p, Tensor wstream, Tensor b2, "
    "Tensor gamma, Tensor beta, Tensor? mask, float ln_eps, int prescale_exp=0) -> Tensor":
        lambda e, nab, np_, ws, b2, g, b, m, eps, pe=0: edge_transition_f16x3(e, nab, np_, ws, b2, g, b, m, eps, prescale_exp=pe),
    "edge_transition_f16x3_chain(Tensor edge, bool in_tiled, int B, int N, Tensor node_ab, Tensor node_p, Tensor wstream, Tensor b2, "
    "Tensor gamma, Tensor beta, Tensor? mask, float ln_eps, Tensor? proj_bias64, str out_layout, int prescale_exp=0, "
    "bool ab_kernel_form=False, int in_rec=0) -> (Tensor?, Tensor?, Tensor?)": _op_edge_transition_f16x3_chain,
    "edge_embed(Tensor node_a, Tensor node_b, Tensor rel_table, Tensor bin_table, Tensor bin_lower, Tensor residue_idx, Tensor ca, "
    "Tensor w2p, Tensor w3p, Tensor b2, Tensor b3, Tensor gamma, Tensor beta, Tensor? mask, int rel_offset, float ln_eps) -> Tensor":
        lambda *a: edge_embed(*a),
    "edge_embed_f16x3(Tensor node_a, Tensor node_b, Tensor rel_table, Tensor bin_table, Tensor bin_lower, Tensor residue_idx, Tensor ca, "
    "Tensor wstream, Tensor b2, Tensor b3, Tensor gamma, Tensor beta, Tensor? mask, int rel_offset, float ln_eps) -> Tensor":
        lambda *a: edge_embed_f16x3(*a),
    "edge_embed_classes_f16x3(Tensor node_a2, Tensor node_b2, Tensor fixed_cls, Tensor rel_table, Tensor bin_table, Tensor bin_lower, "
    "Tensor residue_idx, Tensor ca, Tensor wstream, Tensor b2, Tensor b3, Tensor gamma, Tensor beta, Tensor? mask, int rel_offset, "
    "float ln_eps) -> Tensor": lambda *a: edge_embed_classes_f16x3(*a),
    "pair_project(Tensor edge, Tensor wp, Tensor bias64) -> (Tensor, Tensor)": lambda *a: pair_project(*a),
    # ---- attention
    "ipa_prep_points(Tensor rigids7, Tensor q_pts_lin, Tensor kv_pts_lin, int n_heads=8, int n_qk=8, int n_v=12) -> (Tensor, Tensor, Tensor)":
        lambda *a: ipa_prep_points(*a),
    "ipa_attention(Tensor q, Tensor kv, Tensor q_pts, Tensor k_pts, Tensor v_pts, Tensor attn_bias, Tensor pair_z, "
    "Tensor mask, Tensor rigids7, Tensor head_w) -> Tensor": lambda *a: ipa_attention(*a),
    "ipa_prep_points_f16(Tensor rigids7, Tensor q_pts_lin, Tensor kv_pts_lin, Tensor head_w, int n_heads=8, int n_qk=8, int n_v=12, "
    "int c_hidden=256) -> (Tensor, Tensor, Tensor, Tensor, Tensor)": lambda *a: ipa_prep_points_f16(*a),
    "ipa_prep_points_shared_kv(Tensor rigids7, Tensor q_pts_lin, Tensor kv_pts_lin, Tensor head_w, Tensor s_xp, int n_heads=8, int n_qk=8, "
    "int n_v=12, int c_hidden=256) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor?, Tensor)":
        lambda r7, qp, kvp, hw, s_xp, h=8, nq=8, nv=12, c=256: ipa_prep_points_f16(r7, qp, kvp, hw, h, nq, nv, c, s_xp),
    "ipa_attention_f16w(Tensor q_xp, Tensor k_xp, Tensor v_vf, Tensor qp_xp, Tensor kp_xp, Tensor vp_vf, Tensor q2, Tensor k2, "
    "Tensor(a!) attn_bias, Tensor pair_z, Tensor mask, Tensor rigids7, int n_heads=8, int c_hidden=256, int n_qk=8, int n_v=12, int c_pz=32, "
    "float inf=1e5, float eps=1e-8, bool logits_inplace=False) -> (Tensor, Tensor)":
        lambda q, k, v, qp, kp, vp, q2, k2, ab, pz, m, r7, *rest: ipa_attention_f16(q, k, v, (qp, kp, vp, q2, k2), ab, pz, m, r7, *rest),
    "encoder_attention(Tensor qkv, Tensor? key_bias, int n_samples, int n_res, int n_heads=4, bool want_f32=False, bool want_xp=True, "
    "str arith='f32') -> (Tensor?, Tensor?)": lambda *a: encoder_attention(*a),
    # ---- node stream
    "node_linear(Tensor xp, Tensor wpk, Tensor? bias, int n_rows, int k_in, int n_out, int tiles, Tensor? pre_scale=None, bool relu=False, "
    "Tensor? pre_mask=None, Tensor? residual=None, Tensor? ln_gamma=None, Tensor? ln_beta=None, float ln_eps=0.0, Tensor? post_mask=None, "
    "Tensor(a!)? out_f32=None, int out_col0=0, bool want_f32=True, Tensor(b!)? out_xp=None, int out_xp_k=-1, int out_xp_k0=0, "
    "bool want_xp=False, int map_pad=0, int map_src=0) -> (Tensor?, Tensor?)": _op_node_linear,
    "node_linear_f32(Tensor x, Tensor wpk32, Tensor? bias, int n_rows, int k_in, int n_out, int tiles, Tensor? pre_scale=None, "
    "bool relu=False, Tensor? pre_mask=None, Tensor? residual=None, Tensor? ln_gamma=None, Tensor? ln_beta=None, float ln_eps=0.0, "
    "Tensor? post_mask=None, Tensor(a!)? out=None, int out_col0=0) -> Tensor": _op_node_linear_f32,
    "node_linear_vfrag(Tensor xp, Tensor wpk, Tensor? bias, int n_rows, int k_in, int n_out, int tiles_per_head=8, int map_pad=0, "
    "int map_src=0) -> Tensor":
        lambda xp, w, b, m, k, n, tph=8, mp=0, ms=0: node_linear_vfrag(xp, w, b, m, k, n, tph, row_map=(mp, ms) if mp else None),
    "ipa_projections(Tensor s_xp, Tensor[] q, Tensor[] k, Tensor[] v, Tensor[] qp, Tensor[] kvp, int[] dims, int n_rows, int n_rows_padded, "
    "int map_pad=0, int map_src=0) -> (Tensor, Tensor?, Tensor?, Tensor, Tensor)":      # (k / v: empty lists = absent, folded projections)
        lambda s_xp, q, k, v, qp, kvp, dims, m, mo, mp=0, ms=0: ipa_projections(
            s_xp, *[({"w": t[0], "b": t[1], "k": dims[3 * i], "n": dims[3 * i + 1], "tg": dims[3 * i + 2]} if len(t) else None)
                    for i, t in enumerate((q, k, v, qp, kvp))],
            m, mo, (mp, ms) if mp else None),
    "embed_assemble(Tensor t_img, Tensor node_const, Tensor fa, Tensor fb, int n_samples, int n_res, bool planes, bool b_col_blocked) "
    "-> (Tensor, Tensor, Tensor)": lambda *a: embed_assemble(*a),
    "node_linear_multi(Tensor xp, Tensor[] w, Tensor[] bias, Tensor[] pre_scale, int[] dims, Tensor(a!)[] out_f32, Tensor(b!)[] out_xp) -> ()":
        lambda *a: node_linear_multi(*a),
    "node_chain(Tensor xp, Tensor[] w_row, Tensor[] bias, bool[] relu, int n_rows, int width, Tensor? pre_mask=None, Tensor? residual=None, "
    "Tensor? ln_gamma=None, Tensor? ln_beta=None, float ln_eps=0.0, Tensor? post_mask=None, Tensor(a!)? out_f32=None, int out_col0=0, "
    "bool want_f32=True, Tensor(b!)? out_xp=None, int out_xp_k=-1, int out_xp_k0=0, bool want_xp=False, int k_in0=-1, "
    "Tensor? mid_residual=None, Tensor(c!)? mid_out_f32=None, Tensor? mid_ln_gamma=None, Tensor? mid_ln_beta=None, float mid_ln_eps=0.0) "
    "-> (Tensor?, Tensor?)":
        lambda xp, w, b, r, m, wd, pm=None, res=None, g=None, be=None, eps=0.0, pom=None, of=None, oc=0, wf=True, ox=None, ok=-1, ok0=0, wx=False,
        k0=-1, mr=None, mo=None, mg=None, mb=None, me=0.0: node_chain(
            xp, w, b, r, m, wd, pm, res, g, be, eps, pom, of, oc, wf, ox, _opt_int(ok), ok0, wx, _opt_int(k0), mr, mo, _ln3(mg, mb, me)),
    "row_layernorm(Tensor x, int n_rows, int n_cols, Tensor gamma, Tensor beta, float eps, Tensor? post_mask=None, Tensor(a!)? out_f32=None, "
    "int out_col0=0, bool want_f32=True, Tensor(b!)? out_xp=None, int out_xp_k=-1, int out_xp_k0=0, bool want_xp=False) -> (Tensor?, Tensor?)":
        lambda x, m, n, g, b, eps, pm=None, of=None, oc=0, wf=True, ox=None, ok=-1, ok0=0, wx=False: row_layernorm(
            x, m, n, g, b, eps, pm, of, oc, wf, ox, _opt_int(ok), ok0, wx),
    "pack_planes(Tensor x, int col0=0, int n_cols=-1, Tensor(a!)? out=None, int out_k=-1, int k0=0, Tensor? row_scale=None) -> Tensor":
        lambda x, c0=0, nc=-1, out=None, ok=-1, k0=0, rs=None: pack_planes(x, c0, _opt_int(nc), out, _opt_int(ok), k0, rs),
    # ---- frames / diffusion geometry
    "se3_step(Tensor x0_7, Tensor xt_7, Tensor mask, Tensor diffuse_mask, Tensor params8, float dt) -> Tensor":
        lambda x0, xt, m, dm, p8, dt: se3_step(x0, xt, m, dm, p8, dt)[0],
    "forward_marginal(Tensor? rigids0_4x4, Tensor z_axis, Tensor u01, Tensor z_trans, Tensor cdf_rows, Tensor row_of_sample, "
    "Tensor omega_grid, Tensor? params2, Tensor? diffuse_mask=None, float coordinate_scaling=0.1) -> Tensor":
        lambda *a: forward_marginal(*a),
    "rigid_compose_update(Tensor rigids7, Tensor update6, Tensor mask) -> Tensor": lambda *a: rigid_compose_update(*a),
    "rigid_scale_trans(Tensor rigids7, float scale, bool divide=False) -> Tensor": lambda *a: rigid_scale_trans(*a),
    "torsion_head(Tensor u, int n_rows, bool normalize=True, float eps=1e-8, Tensor? gt_sin_cos=None, Tensor? fixed_mask=None) -> Tensor":
        lambda *a: torsion_head(*a),
    "frames_to_backbone(Tensor rigids7, Tensor psi, Tensor? aatype) -> Tensor": lambda r, p, a: frames_to_backbone(r, p, a)[0],
}


def register_torch_ops():
    """Expose every tensor entry point of the library as ``torch.ops.str2str_amd.<name>`` (CUDA/HIP dispatch key only).
    The model's modules reach their kernels through these ops (``node_apply``, ``encoder_attention``, the attention and
    edge-transition call sites in node.py and in models/net): ``torch.ops.str2str_amd`` is the operator surface, this package its
    implementation over the C ABI.  Called once when the package is imported: defining the schemas needs no GPU and no library; the
    kernels behind them load the shared object on first use."""
    global _registered
    if _registered:
        return
    lib = torch.library.Library("str2str_amd", "DEF")
    impl = torch.library.Library("str2str_amd", "IMPL", "CUDA")
    for schema, fn in _TORCH_OPS.items():
        lib.define(schema)
        impl.impl(schema.split("(")[0], fn)
    register_torch_ops._libs = (lib, impl)  # keep alive
    _registered = True
