"""The node stream of a trunk block as plain formulas: dtype-generic, plain torch, no ``ops``.

``layer`` is the epilogue contract of the node kernels (csrc/node_gemm.hip, "Epilogue shared by ..."):
    v = (x W^T) * pre_scale[row] + b;  relu;  v *= pre_mask[row];  v += residual;  LayerNorm;  v *= post_mask[row]
and every stage of ``TranslationIPA.forward`` (models/net/ipa.py) below is a few calls of it, in the order the trunk runs them.
A stage takes its inputs ([M, c] rows, M = B N) and the reference-keyed state dict and returns its output in ``dtype``; float64 is
the reference of the parity tests, float32 the chain whose distance from float64 sets their bound (tests/node_cases.py).

``L`` (default ``layer``) lets a caller evaluate a stage with another layer function: the CPU emulation of the f16 planes
(``matmul=split_f16x3``), or a planted mistake.  ``trace``: a list that receives one record per layer (inputs, weights, the value in
front of the LayerNorm, the output) -- what the measure and the format's floor are computed from.
"""
import functools

import torch

TRUNK = "translator.trunk."
TORSION = "translator.torsion_pred"


def layer_norm(v, gamma, beta, eps):
    """Two-pass LayerNorm over the last dimension (biased variance, eps inside the root)."""
    mean = v.mean(dim=-1, keepdim=True)
    d = v - mean
    var = (d * d).mean(dim=-1, keepdim=True)
    return d / torch.sqrt(var + eps) * gamma + beta


def matmul(x, w):
    """x W^T.  In float32 the sum over k is a dot product written as a loop: acc += x_k w_k, left to right, every product and every
    addition rounded to float32 -- the same figures on every machine.  (A library GEMM blocks and threads the sum as it likes, and
    the float32 chain's distance from float64, which sets the bounds, would differ from machine to machine with it.)"""
    if x.dtype != torch.float32:
        return x @ w.t()
    acc = x[:, :1] * w[:, 0]
    for k in range(1, x.shape[1]):
        p = x[:, k:k + 1] * w[:, k]      # (a product of its own, then the addition: nothing a build could contract into an FMA)
        acc = acc + p
    return acc


def layer(x, w, b=None, pre_scale=None, relu=False, pre_mask=None, residual=None, ln=None, post_mask=None, *, dtype=torch.float64,
          trace=None, matmul=matmul):
    """One node layer: x [M, K], w [n, K], b [n], pre_scale / pre_mask / post_mask [M], residual [M, >= n] (its leading n columns),
    ln = (gamma, beta, eps).  -> [M, n] in ``dtype``."""
    c = lambda t: None if t is None else t.to(dtype)  # noqa: E731
    x, w, b, pre_scale, pre_mask, residual, post_mask = (c(t) for t in (x, w, b, pre_scale, pre_mask, residual, post_mask))
    n = w.shape[0]
    v = matmul(x, w).to(dtype)
    if pre_scale is not None:
        v = v * pre_scale[:, None]
    if b is not None:
        v = v + b
    if relu:
        v = torch.relu(v)
    if pre_mask is not None:
        v = v * pre_mask[:, None]
    if residual is not None:
        v = v + residual[:, :n]
    out = v
    if ln is not None:
        out = layer_norm(v, c(ln[0]), c(ln[1]), ln[2])
    if post_mask is not None:
        out = out * post_mask[:, None]
    if trace is not None:
        trace.append(dict(x=x, w=w, b=b, pre_scale=pre_scale, relu=relu, pre_mask=pre_mask, residual=residual, ln=ln, post_mask=post_mask,
                          pre_ln=v, out=out))
    return out


def row_map_index(n_rows, n_pad, n_src):
    """Input row of every output row under a padded row map: output row (sample, n), n < n_pad, reads input row
    sample * n_src + min(n, n_src - 1) (the padded rows repeat the sample's last row)."""
    r = torch.arange(n_rows)
    return (r // n_pad) * n_src + torch.clamp(r % n_pad, max=n_src - 1)


# ------------------------------------------------------------------------------------------ the f16 planes, emulated on the CPU
def split_planes(t, flush_subnormals=False):
    """fp32 -> the f16 pair (t_h = rn16(t), t_l = rn16(t - t_h)), as float64 tensors.  ``flush_subnormals``: the low plane with f16
    subnormals flushed to zero (a planted mistake, never the format)."""
    t = t.float()
    h = t.half()
    lo = (t - h.float()).half()
    if flush_subnormals:
        lo = torch.where(lo.float().abs() < 2.0 ** -14, torch.zeros_like(lo), lo)
    return h.double(), lo.double()


def split_f16x3(x, w, drop_xl=False, drop_wl=False, flush_subnormals=False):
    """x W^T in the plane arithmetic of the node kernels: x -> (x_h, x_l), 32 w -> (W_h, W_l), the three products
    W_h x_h + W_h x_l + W_l x_h accumulated in float64, then x 1/32.  CPU only: what the FORMAT loses, with no fp32 accumulation."""
    xh, xl = split_planes(x, flush_subnormals)
    wh, wl = split_planes(32.0 * w.float(), flush_subnormals)
    acc = xh @ wh.t()
    if not drop_xl:
        acc = acc + xl @ wh.t()
    if not drop_wl:
        acc = acc + xh @ wl.t()
    return acc * (1.0 / 32.0)


def f16x3_layer(**flags):
    """``layer`` with the emulated plane product (epilogue in float64)."""
    return functools.partial(layer, matmul=functools.partial(split_f16x3, **flags))


# ------------------------------------------------------------------------------------------ weights
def lin(sd, p):
    return sd[p + ".weight"], sd[p + ".bias"]


def ln_of(sd, p, eps=1e-5):
    return sd[p + ".weight"], sd[p + ".bias"], eps


def n_encoder_layers(sd, b):
    n = 0
    while f"{TRUNK}transformer_{b}.layers.{n}.linear1.weight" in sd:
        n += 1
    return n


# ------------------------------------------------------------------------------------------ the stages, in the trunk's order
def linear_out(sd, b, feats, s, mask, dtype=torch.float64, L=layer, trace=None):
    """LN(mask * (W feats + b) + s): linear_out of IPA block ``b``, the mask, the residual and ipa_ln (reference ipa.py:266,353-354)."""
    return L(feats, *lin(sd, f"{TRUNK}ipa_{b}.linear_out"), pre_mask=mask, residual=s, ln=ln_of(sd, f"{TRUNK}ipa_ln_{b}"), dtype=dtype, trace=trace)


def skip_embed(sd, b, init_node, dtype=torch.float64, L=layer, trace=None):
    """skip_embed(init_node): columns 256..319 of the transformer input (reference ipa.py:356)."""
    return L(init_node, *lin(sd, f"{TRUNK}skip_embed_{b}"), dtype=dtype, trace=trace)


def transformer_input(x_ln, skip):
    return torch.cat([x_ln, skip], dim=-1)


def in_proj(sd, b, l, x, dtype=torch.float64, L=layer, trace=None):
    p = f"{TRUNK}transformer_{b}.layers.{l}.self_attn."
    return L(x, sd[p + "in_proj_weight"], sd[p + "in_proj_bias"], dtype=dtype, trace=trace)


def post_attention(sd, b, l, x, sa, dtype=torch.float64, L=layer, trace=None):
    """x1 = norm1(x + out_proj(sa)); norm2(x1 + linear2(relu(linear1(x1)))) -> (x1, output)."""
    p = f"{TRUNK}transformer_{b}.layers.{l}."
    x1 = L(sa, *lin(sd, p + "self_attn.out_proj"), residual=x, ln=ln_of(sd, p + "norm1"), dtype=dtype, trace=trace)
    h = L(x1, *lin(sd, p + "linear1"), relu=True, dtype=dtype, trace=trace)
    return x1, L(h, *lin(sd, p + "linear2"), residual=x1, ln=ln_of(sd, p + "norm2"), dtype=dtype, trace=trace)


def node_transition(sd, b, s, x, mask, dtype=torch.float64, L=layer, trace=None, hidden=None):
    """s' = mask * LN_nt(n + lin3(relu(lin2(relu(lin1(n)))))), n = s + linear(x) (reference ipa.py:358-360, layers.py:128-145).
    ``hidden``: a list that receives the two hidden activations."""
    p = f"{TRUNK}node_transition_{b}."
    n = L(x, *lin(sd, f"{TRUNK}linear_{b}"), residual=s, dtype=dtype, trace=trace)
    h1 = L(n, *lin(sd, p + "linear_1"), relu=True, dtype=dtype, trace=trace)
    h2 = L(h1, *lin(sd, p + "linear_2"), relu=True, dtype=dtype, trace=trace)
    if hidden is not None:
        hidden += [h1, h2]
    return L(h2, *lin(sd, p + "linear_3"), residual=n, ln=ln_of(sd, p + "ln"), post_mask=mask, dtype=dtype, trace=trace)


def backbone_update(sd, b, s1, diffuse_mask, dtype=torch.float64, L=layer, trace=None):
    """W (diffuse_mask * s') + b, 6 columns (reference ipa.py:361)."""
    return L(s1, *lin(sd, f"{TRUNK}bb_update_{b}.linear"), pre_scale=diffuse_mask, dtype=dtype, trace=trace)


def edge_node_parts(sd, b, s1, dtype=torch.float64, L=layer, trace=None, prefix=None):
    """The EdgeTransition's per-node parts from the unfolded formula (reference layers.py:170-185; EdgeTransition.node_layers):
    n' = initial_embed(s'), A = W1[:, ce:ce+cb] n' + b1, B = W1[:, ce+cb:] n', G = C (Wf[:, ce+cb:] n' + bf) with the centring
    C = I - 1 1^T / 128 over the final layer's output channels: the layer stands in front of a LayerNorm, which removes the common
    component, and the product packs it centred (layers.centred; ``centre``).
    -> (n' [M, 128], [A | 32 B | 32 G] [M, 896]: the form the f16x3 pair kernel reads)."""
    p = f"{TRUNK}edge_transition_{b}." if prefix is None else prefix
    n_p = L(s1, *lin(sd, p + "initial_embed"), dtype=dtype, trace=trace)
    cb = n_p.shape[-1]
    (w1, b1), (wf, bf) = lin(sd, p + "trunk.0"), lin(sd, p + "final_layer")
    ce = w1.shape[1] - 2 * cb
    A = L(n_p, w1[:, ce:ce + cb], b1, dtype=dtype, trace=trace)
    Bc = L(n_p, w1[:, ce + cb:], None, dtype=dtype, trace=trace)
    G = L(n_p, centre(wf[:, ce + cb:]), centre(bf), dtype=dtype, trace=trace)
    return n_p, torch.cat([A, 32.0 * Bc, 32.0 * G], dim=-1)


def centre(w):
    """C w over dim 0 (the output channels) in float64: weights [n, K] or a bias [n] of a layer in front of a LayerNorm."""
    w = w.double()
    return w - w.mean(dim=0, keepdim=True)


def torsion_head(sd, s1, gt=None, fixed=None, eps=1e-8, dtype=torch.float64, L=layer, trace=None):
    """u / sqrt(max(sum u^2, eps)) of linear_final(s' + linear_2(relu(linear_1(s')))) (reference layers.py:199-213), blended with the
    input torsion ``gt`` [M, 2] under the fixed mask [M] (denoising_ipa.py:192-193).  -> (u [M, 2], psi [M, 2])."""
    h = L(s1, *lin(sd, TORSION + ".linear_1"), relu=True, dtype=dtype, trace=trace)
    t2 = L(h, *lin(sd, TORSION + ".linear_2"), residual=s1, dtype=dtype, trace=trace)
    u = L(t2, *lin(sd, TORSION + ".linear_final"), dtype=dtype, trace=trace)
    return u, torsion_normalise(u, gt, fixed, eps, dtype)


def torsion_normalise(u, gt=None, fixed=None, eps=1e-8, dtype=torch.float64):
    u = u.to(dtype)
    psi = u / torch.sqrt(torch.clamp((u * u).sum(dim=-1, keepdim=True), min=eps))
    if gt is not None:
        f = fixed.to(dtype)[:, None]
        psi = gt.to(dtype) * f + psi * (1 - f)
    return psi
