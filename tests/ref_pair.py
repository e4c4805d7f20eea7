"""The pair stream of a trunk block as plain formulas: dtype-generic, plain torch, no ``ops``.

``edge_transition`` states the EdgeTransition (reference layers.py:170-185) at the two contract levels the product has:
  from the per-node vectors   ``parts`` = (n' [B, N, 128], [A_i + b1 | B_j | G_j] [B, N, 896]): the contract of ``EdgeTransition.pair_mlp``
                              and ``ops.edge_transition_f16x3`` (how the vectors come from s: ``ref_node.edge_node_parts``)
  from (node, edge)           ``s`` [B, N, 256]: ``EdgeTransition.forward``
In both, per pair p = (sample, i, j), a row of M = B N N:
    h1 = relu(W1[:, :128] e + A_i + B_j),  h2 = relu(W2 h1 + b2),
    y  = Wf[:, :256] (h2[:256] + [e | n'_i]) + Wf[:, 256:] h2[256:] + G_j,   out = LayerNorm(y) m_i m_j
(G_j = Wf[:, 256:] n'_j + bf: the j-side residual of h2 + [e | n'_i | n'_j] taken through the final layer on the node side).

The three layers are ``ref_node.layer`` records (A_i + B_j and G_j as per-row biases), so ``trace``, ``L`` (the CPU emulation of the
f16 planes, ``ref_node.f16x3_layer``) and ``node_cases.floors`` work on them as on the node stream; the final layer's record names
h2 as the part of its input that is an earlier output (``x_from``).  ``exp`` = e is the block exponent of the f16x3 kernel: the
operator does not change (the scaling is exact), the records of the two layers that read hidden activations carry it for the
format's floor.  ``wrong`` plants one mistake (tests/test_pair_parity_cpu.py).

The next IPA block's projection of the result is ``ref_embed.pair_projection64`` / ``pair_projection32``; ``projection`` calls them
and returns, next to their outputs, the record (rows of [attn_bias (8) | pair_z (32)]) that the measure and the floor need.
"""
import functools

import torch

import ref_embed as RE
import ref_node as RN

WRONG = ("ij_swapped", "b2_dropped", "residual_from_h1", "j_residual_missing", "mask_i_only", "ln_eps_unscaled",
         "projection_of_unmasked_row", "attn_bias_pair_major", "ragged_last_pair_from_neighbour")


def pair_index(B, N, device="cpu"):
    """-> (row of residue i, row of residue j) in [B N] for every pair row p = (sample, i, j) of [B N N]."""
    p = torch.arange(B * N * N, device=device)
    return p // N, (p // (N * N)) * N + p % N


def scaled_planes_layer(exp, **flags):
    """``ref_node.layer`` with the plane product on 2^-exp x the input (the block exponent), result x 2^exp."""
    def mm(x, w):
        return RN.split_f16x3(x * 2.0 ** -exp, w, **flags) * 2.0 ** exp
    return functools.partial(RN.layer, matmul=mm)


def edge_transition(sd, prefix, edge, mask=None, s=None, parts=None, dtype=torch.float64, L=RN.layer, trace=None, exp=0, L_hidden=None,
                    wrong=None):
    """-> out [B, N, N, 128] in ``dtype``.  ``prefix``: "translator.trunk.edge_transition_0." style.  ``L_hidden``: the layer function
    of the two layers that read hidden activations (default ``L``)."""
    assert wrong is None or wrong in WRONG, wrong
    B, N = edge.shape[:2]
    M, dev = B * N * N, edge.device
    Lh = L if L_hidden is None else L_hidden
    ii, jj = pair_index(B, N, dev)
    src = None
    if parts is None:
        k0 = 0 if trace is None else len(trace)
        n_p, ab = RN.edge_node_parts(sd, None, s.reshape(B * N, -1), dtype=dtype, L=L, trace=trace, prefix=prefix)
        A, Bc, G = ab[:, :384], ab[:, 384:768] / 32.0, ab[:, 768:] / 32.0
        if trace is not None:
            src = [r["out"] for r in trace[k0:k0 + 4]]      # n', A, B, G: their floors go on into the pair layers
    else:
        n_p, ab = (t.reshape(B * N, -1).to(dtype) for t in parts)
        A, Bc, G = ab[:, :384], ab[:, 384:768], ab[:, 768:]
    (w1, _), (w2, b2), (wf, _) = (RN.lin(sd, prefix + n) for n in ("trunk.0", "trunk.2", "final_layer"))
    ln = RN.ln_of(sd, prefix + "layer_norm")
    if wrong == "ln_eps_unscaled":
        ln = (ln[0], ln[1], ln[2] * 4.0 ** exp)
    if wrong == "ij_swapped":
        ii, jj = jj, ii
    e = edge.reshape(M, -1)
    h1 = L(e, w1[:, :e.shape[1]], A[ii] + Bc[jj], relu=True, dtype=dtype, trace=trace)
    h2 = Lh(h1, w2, None if wrong == "b2_dropped" else b2, relu=True, dtype=dtype, trace=trace)
    r = torch.cat([e.to(dtype), n_p[ii], torch.zeros_like(n_p[jj])], dim=-1)
    g = G[jj]
    if wrong == "j_residual_missing":
        g = g - n_p[jj] @ wf[:, 256:].to(g).t()
    m = None
    if mask is not None:
        mm = mask.reshape(B * N).to(dev)
        m = mm[ii] if wrong == "mask_i_only" else mm[ii] * mm[jj]
    out = Lh((h1 if wrong == "residual_from_h1" else h2) + r, wf, g, ln=ln, post_mask=m, dtype=dtype, trace=trace)
    if trace is not None:
        trace[-1]["x_from"] = h2
        trace[-2]["exp"] = trace[-1]["exp"] = exp
        if src is not None:
            trace[-3]["b_from"] = [(src[1], ii), (src[2], jj)]
            trace[-1]["b_from"] = [(src[3], jj)]
            trace[-1]["x_add_from"] = [(src[0], ii, 128)]
    if wrong == "ragged_last_pair_from_neighbour" and M > 1:
        out = out.clone()
        out[M - 1] = out[M - 2]
    return out.reshape(B, N, N, -1)


def projection(sd, ipa_prefix, out, rec=None, dtype=torch.float64, wrong=None, unmasked=None):
    """attn_bias [B, 8, N, N] (head-major) and pair_z [B, N, N, 32] of ``out`` [B, N, N, 128] in ``dtype`` (float64 | float32), as rows
    [M, 40] = [attn_bias | pair_z]; with ``rec`` (the trace record whose output ``out`` is) also the projection's own record."""
    B, N = out.shape[:2]
    z = unmasked if wrong == "projection_of_unmasked_row" else out
    ab, pz = RE.pair_projection64(sd, ipa_prefix, z) if dtype == torch.float64 else RE.pair_projection32(sd, ipa_prefix, z)
    if wrong == "attn_bias_pair_major":
        ab = ab.permute(0, 2, 3, 1).contiguous().view(B, 8, N, N)
    rows = proj_rows(ab, pz)
    if rec is None:
        return rows
    w = torch.cat([sd[f"{ipa_prefix}.linear_b.weight"], sd[f"{ipa_prefix}.down_z.weight"]]).to(out.device).double()
    b = torch.cat([sd[f"{ipa_prefix}.linear_b.bias"], sd[f"{ipa_prefix}.down_z.bias"]]).to(out.device).double()
    return rows, dict(x=rec["out"], w=w, b=b, pre_scale=None, relu=False, pre_mask=None, residual=None, ln=None, post_mask=None, pre_ln=rows,
                      out=rows)


def proj_rows(attn_bias, pair_z):
    """(attn_bias [B, 8, N, N], pair_z [B, N, N, 32]) -> rows [B N N, 40]."""
    B, _, N, _ = attn_bias.shape
    return torch.cat([attn_bias.permute(0, 2, 3, 1).reshape(B * N * N, 8), pair_z.reshape(B * N * N, 32)], dim=-1)
