"""Float64 statement of the embedder (EmbeddingModule.forward, denoising_ipa.py:107-159) and of the first IPA block's pair
projection (ipa.py:177,253), for tests/test_embedding_parity*.py.

The input FEATURES stay float32, built exactly as oracle/net.py::embedding builds them (same timestep_embedding,
positional_embedding, calc_distogram formula, same concatenation order): sin of t * 10000 or of a residue number near 1e5 is
ill-conditioned, and the reference defines those values in float32 -- so the float64 reference starts from the reference's own
feature bits.  Everything after them (three Linears, two relus, LayerNorm, masks, the projection) is float64.

``mutate`` plants one wrong formula (the mutations tests/test_embedding_parity_cpu.py must see separated from the right one by
10 x the GPU bound); ``force_bin`` replaces the distogram one-hot of every pair by bin k (-1: no bin), which is how the GPU test
reads off which bin a kernel used.
"""
import torch
import torch.nn.functional as F

from oracle.net import positional_embedding, timestep_embedding

NUM_BINS, MIN_BIN, MAX_BIN = 22, 1e-5, 20.0
MUTATIONS = ("rel_sign", "rel_off_by_one", "fixed_row_col_swapped", "t_of_previous_sample", "bin_plus_one", "upper_edge_le")


def bin_edges32():
    """(lower [22], upper [22]) float32, as calc_distogram forms them (last upper = 1e8)."""
    lower = torch.linspace(MIN_BIN, MAX_BIN, NUM_BINS)
    return lower, torch.cat([lower[1:], lower.new_tensor([1e8])], dim=-1)


def distogram32(pos, mutate=None):
    """oracle.net.calc_distogram, with the two bin mutations."""
    d = torch.linalg.norm(pos[..., :, None, :] - pos[..., None, :, :], dim=-1)[..., None]
    lower, upper = bin_edges32()
    hot = ((d > lower) * ((d <= upper) if mutate == "upper_edge_le" else (d < upper))).type(pos.dtype)
    if mutate == "bin_plus_one":   # bin k -> k + 1 (the last one drops out)
        hot = torch.cat([torch.zeros_like(hot[..., :1]), hot[..., :-1]], dim=-1)
    return hot


def features32(residue_idx, t, fixed_mask, sc_ca, self_conditioning=True, mutate=None, force_bin=None, init=32):
    """-> node features [B, L, 65], pair features [B, L*L, 120 (98 without self-conditioning)], float32, on the CPU."""
    assert mutate is None or mutate in MUTATIONS, mutate
    residue_idx, t, fixed_mask = residue_idx.cpu(), t.cpu().float(), fixed_mask.cpu()
    B, L = residue_idx.shape
    fixed = fixed_mask[..., None].float()
    if mutate == "t_of_previous_sample":
        t = torch.roll(t, 1, 0)
    t_embed = torch.tile(timestep_embedding(t, init)[:, None, :], (1, L, 1))
    t_embed = torch.cat([t_embed, fixed], dim=-1)
    row = torch.tile(t_embed[:, :, None, :], (1, 1, L, 1))
    col = torch.tile(t_embed[:, None, :, :], (1, L, 1, 1))
    if mutate == "fixed_row_col_swapped":
        row, col = row.clone(), col.clone()
        row[..., -1], col[..., -1] = fixed[:, None, :, 0].expand(B, L, L), fixed[:, :, None, 0].expand(B, L, L)
    pair = [torch.cat([row, col], dim=-1).float().reshape(B, L * L, -1)]
    node = [t_embed, positional_embedding(residue_idx, init)]
    rel = (residue_idx[:, :, None] - residue_idx[:, None, :]).reshape(B, L * L)
    if mutate == "rel_sign":
        rel = -rel
    elif mutate == "rel_off_by_one":
        rel = rel + 1
    pair.append(positional_embedding(rel, init))
    if self_conditioning:
        if force_bin is None:
            hot = distogram32(sc_ca.cpu().float(), mutate)
        else:
            hot = torch.zeros(B, L, L, NUM_BINS)
            if force_bin >= 0:
                hot[..., force_bin] = 1.0
        pair.append(hot.reshape(B, L * L, -1))
    return torch.cat(node, dim=-1).float(), torch.cat(pair, dim=-1).float()


def _mlp64(x32, sd, p, dev, rows=16384):
    """Linear, relu, Linear, relu, Linear, LayerNorm in float64 on float32 features, ``rows`` rows at a time."""
    w = {k: sd[f"{p}.{k}"].to(dev).double() for k in ("0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias", "5.weight", "5.bias")}
    flat = x32.reshape(-1, x32.shape[-1])
    out = torch.empty(flat.shape[0], w["4.bias"].shape[0], dtype=torch.float64, device=dev)
    for r0 in range(0, flat.shape[0], rows):
        x = flat[r0:r0 + rows].to(dev).double()
        x = F.relu(F.linear(x, w["0.weight"], w["0.bias"]))
        x = F.relu(F.linear(x, w["2.weight"], w["2.bias"]))
        x = F.linear(x, w["4.weight"], w["4.bias"])
        out[r0:r0 + rows] = F.layer_norm(x, (x.shape[-1],), w["5.weight"], w["5.bias"], 1e-5)
    return out.reshape(*x32.shape[:-1], -1)


def embedding64(sd, residue_idx, t, fixed_mask, sc_ca, node_mask=None, prefix="embedder.", self_conditioning=True, mutate=None,
                force_bin=None, device="cpu"):
    """-> node [B, L, 256], edge [B, L, L, 128] in float64 on ``device`` (node x m_i, edge x m_i m_j under ``node_mask``).
    ``sd``: a reference-keyed state dict (``prefix`` "" for a stand-alone module's)."""
    B, L = residue_idx.shape
    init = (sd[prefix + "node_embed.0.weight"].shape[1] - 1) // 2
    node32, pair32 = features32(residue_idx, t, fixed_mask, sc_ca, self_conditioning, mutate, force_bin, init)
    node = _mlp64(node32, sd, prefix + "node_embed", device)
    edge = _mlp64(pair32, sd, prefix + "edge_embed", device).reshape(B, L, L, -1)
    return apply_mask(node, edge, node_mask)


def apply_mask(node, edge, node_mask):
    if node_mask is None:
        return node, edge
    m = node_mask.to(node.device).to(node.dtype)
    return node * m[..., None], edge * (m[:, :, None] * m[:, None, :])[..., None]


def pair_projection64(sd, ipa_prefix, edge64):
    """-> attn_bias [B, 8, L, L] (head-major, as the kernels write it), pair_z [B, L, L, 32] in float64."""
    dev = edge64.device
    lin = lambda n: F.linear(edge64, sd[f"{ipa_prefix}.{n}.weight"].to(dev).double(), sd[f"{ipa_prefix}.{n}.bias"].to(dev).double())  # noqa: E731
    return lin("linear_b").permute(0, 3, 1, 2).contiguous(), lin("down_z")


def pair_projection32(sd, ipa_prefix, edge32):
    """The float32 chain's projection (oracle.net.ipa's two F.linear calls on the pair tensor)."""
    lin = lambda n: F.linear(edge32, sd[f"{ipa_prefix}.{n}.weight"], sd[f"{ipa_prefix}.{n}.bias"])  # noqa: E731
    return lin("linear_b").permute(0, 3, 1, 2).contiguous(), lin("down_z")
