"""The attention cores as formulas, dtype-generic, in plain torch: what s2s_ipa_attention / s2s_ipa_attention_f16w + s2s_ipa_opair
and s2s_encoder_attention compute, stated once and evaluated in float64 (the reference) or float32 ("the float32 chain", whose
distance from float64 sets the bounds of tests/attention_cases.py).

``ipa_features`` follows oracle/net.py::ipa (reference ipa.py:100-268) from the point where the pair projections exist: inputs
are the block's node activation s, the head-major attention bias [B, H, N, N] (linear_b of z) and pair_z [B, N, N, 32] (down_z
of z), as ``InvariantPointAttention.attention`` receives them.  It returns the sections of linear_out's input separately, plus
``as`` = sum_j a_ij s_j per head: the first 2048 columns of the folded path (models/net/ipa.py _folded_packs), which feeds W_v into
linear_out.

``mutate`` plants one mistake of the kind a pipelined kernel makes (MUTATIONS); tests/test_attention_parity_cpu.py checks that
each exceeds the bound of its family on some case of the table, so a kernel making it cannot pass.
"""
import math

import torch
import torch.nn.functional as F

SECTIONS = ("o", "as", "o_pt", "o_norm", "o_pair")
TILE = 32   # residues per key tile of the attention kernels
MUTATIONS = ("max_misses_last_tile", "key_mask_shifted_one_tile", "mask_of_next_sample", "norm_before_inverse_frame",
             "opair_sum_misses_last_tile")


def ipa_weights(sd, prefix):
    """The block's tensors out of a state dict, keyed without the prefix."""
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def quat_to_rot(q):
    """rigid_utils.py:187-207 (the quaternion is used as it is, not normalised)."""
    a, b, c, d = q.unbind(-1)
    return torch.stack([torch.stack([a * a + b * b - c * c - d * d, 2 * b * c - 2 * a * d, 2 * b * d + 2 * a * c], -1),
                        torch.stack([2 * b * c + 2 * a * d, a * a - b * b + c * c - d * d, 2 * c * d - 2 * a * b], -1),
                        torch.stack([2 * b * d - 2 * a * c, 2 * c * d + 2 * a * b, a * a - b * b - c * c + d * d], -1)], -2)


def _last_tile_start(N):
    return (N - 1) // TILE * TILE


def ipa_features(weights, s, attn_bias, pair_z, rigids7, mask, dtype=torch.float64, n_heads=8, n_qk=8, n_v=12, inf=1e5, eps=1e-8,
                 mutate=None):
    """-> dict(logits [B,H,N,N], probs [B,H,N,N], o [B,N,H*C], as [B,N,H*c_s], o_pt [B,N,3*H*Pv] (x | y | z), o_norm [B,N,H*Pv],
    o_pair [B,N,H*c_pz]); cat(o, o_pt, o_norm, o_pair) is linear_out's input, cat(as, ...) the folded linear_out's."""
    assert mutate is None or mutate in MUTATIONS, mutate
    c = lambda t: t.to(dtype)  # noqa: E731
    w = {k: c(v) for k, v in weights.items()}
    s, attn_bias, pair_z, rigids7, mask = c(s), c(attn_bias), c(pair_z), c(rigids7), c(mask)
    B, N, _ = s.shape
    H, Pq, Pv = n_heads, n_qk, n_v
    lin = lambda x, p: F.linear(x, w[p + ".weight"], w[p + ".bias"])  # noqa: E731
    C = w["linear_q.weight"].shape[0] // H
    q = lin(s, "linear_q").view(B, N, H, C)
    k, v = lin(s, "linear_kv").view(B, N, H, 2 * C).split(C, dim=-1)
    R, T = quat_to_rot(rigids7[..., :4]), rigids7[..., 4:]

    def pts(name):   # local points, coordinate-major in the projection -> global frame [B, N, H, P, 3]
        x = lin(s, name)
        x = torch.stack(x.split(x.shape[-1] // 3, dim=-1), dim=-1)
        return (torch.einsum("bnij,bnpj->bnpi", R, x) + T[:, :, None, :]).view(B, N, H, -1, 3)

    q_pts = pts("linear_q_points")
    k_pts, v_pts = pts("linear_kv_points").split([Pq, Pv], dim=-2)

    hw = F.softplus(w["head_weights"]) * math.sqrt(1.0 / (3 * (Pq * 9.0 / 2)))
    logits = torch.einsum("bihc,bjhc->bhij", q, k) * math.sqrt(1.0 / (3 * C)) + math.sqrt(1.0 / 3) * attn_bias
    for h in range(H):   # the point term with explicit differences, one head at a time (memory)
        d = q_pts[:, :, None, h] - k_pts[:, None, :, h]                      # [B, N, N, Pq, 3]
        logits[:, h] += (d * d).sum(dim=(-1, -2)) * (-0.5 * hw[h])
    key_mask = mask
    if mutate == "key_mask_shifted_one_tile":
        key_mask = torch.cat([mask.new_ones(B, min(TILE, N)), mask[:, : max(N - TILE, 0)]], dim=1)
    elif mutate == "mask_of_next_sample":
        key_mask = mask.roll(-1, dims=0)
    logits = logits + inf * (mask[:, None, :, None] * key_mask[:, None, None, :] - 1.0)

    j0 = _last_tile_start(N)
    if mutate == "max_misses_last_tile" and j0 > 0:
        # the row maximum of the keys before the last tile, exponentials formed and clamped as float32 forms them
        m = logits[..., :j0].amax(dim=-1, keepdim=True)
        e = torch.exp((logits - m).float()).to(dtype)
        probs = e / e.sum(dim=-1, keepdim=True)
    else:
        probs = torch.softmax(logits, dim=-1)

    o = torch.einsum("bhij,bjhc->bihc", probs, v).reshape(B, N, H * C)
    a_s = torch.einsum("bhij,bjc->bihc", probs, s).reshape(B, N, -1)
    o_glob = torch.einsum("bhij,bjhpd->bihpd", probs, v_pts)                  # [B, N, H, Pv, 3]
    o_loc = torch.einsum("bnji,bnhpj->bnhpi", R, o_glob - T[:, :, None, None, :])
    o_norm = torch.sqrt(((o_glob if mutate == "norm_before_inverse_frame" else o_loc) ** 2).sum(-1) + eps).reshape(B, N, H * Pv)
    o_pt = o_loc.reshape(B, N, H * Pv, 3).permute(0, 1, 3, 2).reshape(B, N, 3 * H * Pv)
    a_pair = probs
    if mutate == "opair_sum_misses_last_tile" and j0 > 0:
        e = torch.exp(logits - logits.amax(dim=-1, keepdim=True))
        a_pair = e / e[..., :j0].sum(dim=-1, keepdim=True).clamp_min(torch.finfo(dtype).tiny)
    o_pair = torch.einsum("bhij,bijc->bihc", a_pair, pair_z).reshape(B, N, -1)
    return {"logits": logits, "probs": probs, "o": o, "as": a_s, "o_pt": o_pt, "o_norm": o_norm, "o_pair": o_pair}


def ipa_linear_out(weights, f, dtype=torch.float32):
    """linear_out on cat(o, o_pt, o_norm, o_pair): the block's output, as oracle.net.ipa returns it."""
    feats = torch.cat([f["o"], f["o_pt"], f["o_norm"], f["o_pair"]], dim=-1).to(dtype)
    return F.linear(feats, weights["linear_out.weight"].to(dtype), weights["linear_out.bias"].to(dtype))


def encoder_attention(qkv, key_bias, B, N, n_heads=4, dtype=torch.float64):
    """softmax(q k^T / sqrt(dh) + key_bias) v of one nn.TransformerEncoderLayer: qkv [B*N, 3 D] (q | k | v, heads contiguous),
    key_bias [B, N] added to the logits of key j (may hold -inf; None = zeros) -> [B*N, D]."""
    qkv = qkv.to(dtype)
    D = qkv.shape[1] // 3
    dh = D // n_heads
    q, k, v = (t.reshape(B, N, n_heads, dh) for t in qkv.split(D, dim=1))
    logits = torch.einsum("bihc,bjhc->bhij", q * (1.0 / math.sqrt(dh)), k)
    if key_bias is not None:
        logits = logits + key_bias.to(dtype)[:, None, None, :]
    probs = torch.softmax(logits, dim=-1)
    return torch.einsum("bhij,bjhc->bihc", probs, v).reshape(B * N, D), logits, probs
