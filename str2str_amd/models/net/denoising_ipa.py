"""``EmbeddingModule`` and ``DenoisingNet`` (the SE(3) score network entry) on the HIP kernels.

Interface and parameter names follow the reference's ``src/models/net/denoising_ipa.py``
(get_positional_embedding :13-31, get_timestep_embedding :34-46, EmbeddingModule :49-159,
DenoisingNet :162-211).  The N x N edge embedding never builds the [B, N^2, 120] feature tensor:
its first Linear is a sum of four table rows (row part, column part, relative-position table,
distogram-bin table) gathered inside ``s2s_edge_embed`` (csrc/pair_mlp.hip), which then runs the two
128x128 layers on fp32 MFMA, LayerNorm and the edge mask and writes z once.
"""
from __future__ import annotations

import math
import os
from functools import partial
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from ... import ops
from ...arith import default_arith
from ...common.all_atom import compute_backbone
from ...common.rigid_utils import Rigid
from .ipa import TranslationIPA  # noqa: F401  (re-exported like the reference module)
from .layers import DerivedCache, centred


def get_positional_embedding(indices: torch.Tensor, embedding_dim: int, max_len: int = 2056) -> torch.Tensor:
    K = torch.arange(embedding_dim // 2, device=indices.device)
    arg = indices[..., None] * math.pi / (max_len ** (2 * K[None] / embedding_dim))
    return torch.cat([torch.sin(arg), torch.cos(arg)], dim=-1)


def get_timestep_embedding(timesteps: torch.Tensor, embedding_dim: int, max_len: int = 10000) -> torch.Tensor:
    assert timesteps.ndim == 1
    timesteps = timesteps * max_len
    half = embedding_dim // 2
    freq = torch.exp(torch.arange(half, dtype=torch.float, device=timesteps.device) * -(math.log(max_len) / (half - 1)))
    emb = timesteps.float()[:, None] * freq[None, :]
    emb = torch.cat([torch.sin(emb), torch.cos(emb)], dim=1)
    if embedding_dim % 2 == 1:
        emb = F.pad(emb, (0, 1), mode="constant")
    return emb


class EmbeddingModule(nn.Module):
    launch_switches = ("arith", "node_arith")   # attributes set below that select launches: part of sampler._graph_key
    launch_modes = ("ee_classes", "et_by_class")   # ... and the string-valued ones (S2S_EE_CLASSES, S2S_ET_BY_CLASS), part of the key in the same way

    def __init__(self, init_embed_size: int, node_embed_size: int, edge_embed_size: int, num_bins: int = 22,
                 min_bin: float = 1e-5, max_bin: float = 20.0, self_conditioning: bool = True):
        super().__init__()
        pos_embed_size = t_embed_size = init_embed_size
        node_in = t_embed_size + 1 + pos_embed_size
        edge_in = (t_embed_size + 1) * 2 + pos_embed_size
        self.node_embed = nn.Sequential(
            nn.Linear(node_in, node_embed_size), nn.ReLU(), nn.Linear(node_embed_size, node_embed_size), nn.ReLU(),
            nn.Linear(node_embed_size, node_embed_size), nn.LayerNorm(node_embed_size),
        )
        self.self_conditioning = self_conditioning
        if self_conditioning:
            edge_in += num_bins
        self.edge_embed = nn.Sequential(
            nn.Linear(edge_in, edge_embed_size), nn.ReLU(), nn.Linear(edge_embed_size, edge_embed_size), nn.ReLU(),
            nn.Linear(edge_embed_size, edge_embed_size), nn.LayerNorm(edge_embed_size),
        )
        self.time_embed = partial(get_timestep_embedding, embedding_dim=t_embed_size)
        self.position_embed = partial(get_positional_embedding, embedding_dim=pos_embed_size)
        self._dims = (init_embed_size, num_bins, float(min_bin), float(max_bin), edge_embed_size)
        self._wcache, self._w16cache, self._proj_cache, self._idx_cache, self._fixed_cache = (DerivedCache() for _ in range(5))
        self.arith = default_arith()   # edge embedding kernels: "f16x3" (split-f16 MFMA, default) | "f32" (exact fp32 MFMA), str2str_amd/arith.py
        self.node_arith = default_arith()   # the node MLP (node-stream family: follows the trunk)
        # the edge embedding by class (ops.edge_embed_classes_f16x3): "auto" where it is legal and pays, "1" wherever it is legal, "0" never
        self.ee_classes = os.environ.get("S2S_EE_CLASSES", "auto")
        if self.ee_classes not in ("auto", "0", "1"):
            raise ValueError(f"S2S_EE_CLASSES={self.ee_classes!r}: expected auto, 0 or 1")
        # behind the class path, the pair tensor by class (ops.PairByClass: the first EdgeTransition reads the table, z is not materialised):
        # "auto" / "1" wherever DenoisingNet.forward can take it, "0" never
        self.et_by_class = os.environ.get("S2S_ET_BY_CLASS", "auto")
        if self.et_by_class not in ("auto", "0", "1"):
            raise ValueError(f"S2S_ET_BY_CLASS={self.et_by_class!r}: expected auto, 0 or 1")
        self._mask01_cache = DerivedCache()

    # ---- derived tensors
    def _weights(self):
        e0, e2, e4 = self.edge_embed[0], self.edge_embed[2], self.edge_embed[4]
        ie, nb = self._dims[0], self._dims[1]
        t1 = ie + 1

        def build():
            w0 = e0.weight.float()
            n0 = self.node_embed[0]
            wn = n0.weight.float()
            out = {
                # first Linear of both MLPs split by feature block: the timestep embedding is one vector per
                # SAMPLE, so its image is a [B, width] GEMM; the fixed-mask column and the positional block are
                # added per residue.  (Also avoids K = 33 / 65 GEMMs, which hit slow BLAS paths at some row counts.)
                "w_row_t": w0[:, :ie].contiguous(), "w_row_f": w0[:, ie].contiguous(),
                "w_col_t": w0[:, t1:t1 + ie].contiguous(), "w_col_f": w0[:, t1 + ie].contiguous(),
                "w_rel": w0[:, 2 * t1:2 * t1 + ie].contiguous(), "b0": e0.bias.float().contiguous(),
                "wn_t": wn[:, :ie].contiguous(), "wn_f": wn[:, ie].contiguous(), "wn_pos": wn[:, t1:t1 + ie].contiguous(),
                "bn0": n0.bias.float().contiguous(),
                # the three timestep blocks as ONE [512, ie] matrix (+ biases): a chunk shares one t, so their images are three slices
                # of one elementwise product + row sum instead of three of each
                "w_t_cat": torch.cat([wn[:, :ie], w0[:, :ie], w0[:, t1:t1 + ie]], dim=0).contiguous(),
                "b_t_cat": torch.cat([n0.bias.float(), e0.bias.float(), torch.zeros_like(e0.bias.float())]).contiguous(),
                # the last layer stands in front of the LayerNorm: weights and bias centred over the output channels (layers.centred)
                "w3c": centred(e4.weight), "b3c": centred(e4.bias),
                "w2p": ops.pack_weight(e2.weight.float()), "w3p": ops.pack_weight(centred(e4.weight)),
                "node_mlp": [ops.pack_node_layer(self.node_embed[2].weight, self.node_embed[2].bias),
                             ops.pack_node_layer(self.node_embed[4].weight, self.node_embed[4].bias, True)],
            }
            if self.self_conditioning:
                out["bin_tab"] = w0[:, 2 * t1 + ie:2 * t1 + ie + nb].t().contiguous()
            else:  # no distogram columns: a single zero row that is never selected (ca = 0 -> no bin)
                out["bin_tab"] = w0.new_zeros(1, w0.shape[0])
            out["bin_tab_cb"] = ops.column_blocked(out["bin_tab"])  # gather layout of the split-f16 kernel
            out["bin_lower"] = torch.linspace(self._dims[2], self._dims[3], nb).to(w0.device)
            return out

        ne = self.node_embed
        return self._wcache.get([e0.weight, e0.bias, e2.weight, e4.weight, e4.bias, ne[0].weight, ne[0].bias, ne[2].weight, ne[2].bias,
                                 ne[4].weight, ne[4].bias], build)

    def _fixed_terms(self, fixed_mask: torch.Tensor, w: dict, dev, node_pos: torch.Tensor):
        """Per-target constants of the first layers that do not depend on t: (node MLP: fixed-mask column + positional image [B,L,256],
        edge row term [B,L,128], (edge column term in the f16x3 kernel's gather layout [B,32,L,4], the same row-major), class terms).
        Cached on the mask tensor, the positional image and the weights.
        Class terms (the edge embedding by class, ops.edge_embed_classes_f16x3): None unless the mask is exactly 0/1 -- one host read
        per target, here -- else {n_fixed: how many of the two values occur, fixed_cls [B,L] int32: each residue's index among them,
        fa2 / fb2 / nc2: the edge row / column terms and a zero node term of a pseudo-sample of n_fixed residues whose mask runs over
        those values (the same products as above, so ``embed_assemble`` gives the same floats as for the chunk's residues)}."""
        def build():
            fixed = fixed_mask.to(dev)[..., None].float()
            B, L = fixed.shape[:2]
            vals = torch.unique(fixed).cpu().tolist()
            cls = None
            if vals and all(v in (0.0, 1.0) for v in vals):
                f2 = torch.tensor(vals, device=dev, dtype=torch.float32).view(1, -1, 1)
                cls = {"n_fixed": len(vals),
                       "fixed_cls": ((fixed[..., 0] > 0) if len(vals) == 2 else torch.zeros_like(fixed[..., 0])).to(torch.int32).contiguous(),
                       "fa2": (f2 * w["w_row_f"]).contiguous(),
                       "fb2": (f2[:, None] * w["w_col_f"].view(1, 32, 1, 4)).expand(1, 32, len(vals), 4).contiguous(),
                       "nc2": torch.zeros(len(vals), w["wn_f"].shape[0], device=dev)}
            return ((fixed * w["wn_f"] + node_pos).contiguous(), (fixed * w["w_row_f"]).contiguous(),
                    ((fixed[:, None] * w["w_col_f"].view(1, 32, 1, 4)).expand(B, 32, L, 4).contiguous(), (fixed * w["w_col_f"]).contiguous()), cls)

        return self._fixed_cache.get([fixed_mask, w["wn_f"], node_pos], build)

    def _mask_is_01(self, node_mask: Optional[torch.Tensor]) -> bool:
        """Whether the node mask is exactly 0/1 (or absent): one host read per mask tensor, cached like the per-target terms."""
        if node_mask is None:
            return True
        return self._mask01_cache.get([node_mask], lambda: (bool(((node_mask == 0) | (node_mask == 1)).all()),))[0]

    def time_images(self, t_emb: torch.Tensor) -> torch.Tensor:
        """[n, 32] timestep embeddings -> [n, 512] first-layer images + biases [node MLP | edge row | edge column] (one row per
        step of a schedule: the sampler evaluates this once per trajectory and hands ``forward`` a row as ``t_img``).  Elementwise
        product + sum over the 32 embedding channels (no library GEMM), the same expression ``forward`` evaluates for a single t."""
        w = self._weights()
        t_emb = t_emb.to(w["b0"].device).reshape(-1, t_emb.shape[-1]).float()
        return ((w["w_t_cat"][None] * t_emb[:, None, :]).sum(-1) + w["b_t_cat"]).contiguous()

    def _index_tables(self, residue_idx: torch.Tensor, w_rel: torch.Tensor, wn_pos: torch.Tensor):
        """Per-target constants: first-layer image of the node positional features and the relative-position
        table rel_tab[d + off] = W_rel . posemb(d).  Cached on the index tensor (one host sync per target)."""
        return self._tables(residue_idx, w_rel, wn_pos)[:4]

    def _tables(self, residue_idx, w_rel, wn_pos):
        """``_index_tables`` + the relative-position table in the f16x3 kernel's column-blocked gather layout."""
        def build():
            idx_cpu = residue_idx.detach().cpu()
            span = int(idx_cpu.max() - idx_cpu.min())
            d = torch.arange(-span, span + 1)
            dev = w_rel.device
            rel = _table_linear(self.position_embed(d).float().to(dev), w_rel)
            node_pos = _table_linear(self.position_embed(idx_cpu).float().to(dev), wn_pos)  # [B, L, node width]
            return rel, span, node_pos, residue_idx.to(dev).contiguous(), ops.column_blocked(rel)

        return self._idx_cache.get([residue_idx, w_rel, wn_pos], build)

    def forward(self, *args, **kw):
        """``embed`` in the reference's shape (:107-159) -> node_embed, edge_embed (, (attn_bias, pair_z) with ``next_proj``)."""
        node_embed, _, edge_embed, proj = self.embed(*args, **kw)
        return (node_embed, edge_embed) if proj is None else (node_embed, edge_embed, proj)

    def embed(self, residue_idx, t, fixed_mask, self_conditioning_ca, node_mask: Optional[torch.Tensor] = None,
              next_proj=None, t_emb: Optional[torch.Tensor] = None, edge_layout: str = "rowmajor", t_img: Optional[torch.Tensor] = None):
        """-> node_embed [B,N,D_node], the same in the node stream's activation format (what the trunk's first projections and every
        skip_embed read), edge_embed [B,N,N,D_edge], projections or None (reference :107-159; ``edge_layout`` "tiled": as an
        ``ops.PairTiled`` for the trunk's f16x3 pair kernels, arithmetic "f16x3" only; "by_class": as an ``ops.PairByClass`` where the
        call takes the class path and ``next_proj`` is given, "tiled" otherwise).  ``t`` may live on
        the host (the sampler knows it there): its embedding is then computed on the host and uploaded.
        ``node_mask`` optionally fuses DenoisingNet's mask multiplies (reference :186-187); ``next_proj`` (packed
        pair-projection weights of the first IPA block) makes the last value the block's (attn_bias, pair_z)."""
        w = self._weights()
        dev = w["b0"].device
        if dev.type != "cuda":
            raise ops.HipLibraryError("EmbeddingModule runs on the HIP device only (no CPU fallback)")
        if self._dims[4] != 128:
            raise ops.HipLibraryError("edge_embed kernel is built for edge_embed_size=128")
        B, L = residue_idx.shape
        rel_tab, span, node_pos, idx_dev, rel_cb = self._tables(residue_idx, w["w_rel"], w["wn_pos"])
        # [B, 32]; evaluated once per DISTINCT t (a sampler chunk shares one t, and the host sin/cos of arguments up to 1e4 rad
        # costs ~40 us per element): same values, row for row
        if t_img is not None:   # the sampler's form: the timestep block's first-layer image of this step, computed with the schedule
            t_emb = None
        elif t_emb is not None:   # the sampler uploads the embeddings of the whole schedule once: no per-step H2D copy
            t_emb = t_emb.to(dev).reshape(-1, t_emb.shape[-1])                 # (a host->device copy here would make the
        else:                                                                  #  host wait for the GPU every evaluation)
            t_u, t_inv = torch.unique(t.detach().reshape(-1), return_inverse=True)
            t_emb = self.time_embed(t_u)[t_inv].to(dev)
        ne = self.node_embed
        mask = None if node_mask is None else node_mask.to(dev).float().contiguous()
        nn_, ne_ = w["wn_t"].shape[0], w["w_row_t"].shape[0]
        single_t = t_img is not None or t_emb.shape[0] == 1
        M = B * L
        f16 = self.arith == "f16x3"
        cls = None
        if single_t:
            # one timestep for the whole chunk (every sampler call): the three [*, 32] first-layer images are one row each -- a 32-term dot
            # product per output channel, evaluated elementwise for all three blocks at once (or handed in as t_img); the fixed-mask and
            # positional terms do not depend on t and are cached.  What is left per evaluation -- relu(t + const) into the node
            # stream's format and the two operand arrays of the edge embedding -- is ONE launch (s2s_embed_assemble; a network
            # evaluation of a small chunk is launch-latency bound: 22 tiny launches here in round 3)
            # (t_img [B, 512]: one image per sample -- trajectories of different t_delta in one batch, sampler.forward_backward_deltas;
            #  the kernel adds row sample of it instead of the one shared row: the same sums per element)
            per_sample = t_img is not None and t_img.ndim == 2 and t_img.shape[0] == B and B > 1
            img = (t_img if per_sample else t_img.reshape(-1)) if t_img is not None else (w["w_t_cat"] * t_emb).sum(-1) + w["b_t_cat"]
            Fn, Fa, Fb, cls = self._fixed_terms(fixed_mask, w, dev, node_pos)
            h_act, node_a, node_b = torch.ops.str2str_amd.embed_assemble(img.contiguous(), Fn, Fa, Fb[0] if f16 else Fb[1], B, L,
                                                                         self.node_arith == "f16x3", f16)
        else:
            fixed = fixed_mask.to(dev)[..., None].float()
            tl = lambda wt, b=None: _table_linear(t_emb, wt, b)  # noqa: E731
            h = F.relu(tl(w["wn_t"], w["bn0"])[:, None, :] + fixed * w["wn_f"] + node_pos)
            h_act = ops.to_act(h.reshape(M, -1).contiguous(), self.node_arith)
        # layers 2, 3 + LayerNorm (+ DenoisingNet's node mask) on the fused node kernels; the packed planes of the result are
        # what the trunk's first projections and every skip_embed read
        nw = w["node_mlp"]
        node_embed, node_act = ops.node_apply_chain(h_act, nw, M, (True, False), ln=(ne[5].weight, ne[5].bias, ne[5].eps),
                                                          post_mask=None if mask is None else mask.reshape(M), want_xp=True)
        node_embed = node_embed.view(B, L, -1)
        if not single_t:
            node_a = (tl(w["w_row_t"], w["b0"])[:, None, :] + fixed * w["w_row_f"]).expand(B, L, -1).contiguous()
            if f16:
                node_b = (tl(w["w_col_t"]).view(-1, 32, 1, 4) + fixed[:, None] * w["w_col_f"].view(1, 32, 1, 4)).expand(B, 32, L, 4).contiguous()
            else:
                node_b = (tl(w["w_col_t"])[:, None, :] + fixed * w["w_col_f"]).expand(B, L, -1).contiguous()
        ca = self_conditioning_ca.to(dev).float().contiguous() if self.self_conditioning else node_a.new_zeros(B, L, 3)
        e2, e4, ln = self.edge_embed[2], self.edge_embed[4], self.edge_embed[5]
        if f16:
            e2w = e2.weight
            ws = self._w16cache.get([e2w, w["w3c"]], lambda: ops.pack_f16x3_embed_stream(e2w.float(), w["w3c"]))
            proj = None
            if next_proj is not None:  # 5-stage stream: W2 | W3 | the first IPA block's projection stage
                stream = self._proj_cache.get([ws, next_proj["wp_f16x2"]], lambda: torch.cat([ws, next_proj["wp_f16x2"]]))
                proj = (stream, next_proj["b64"])
            # one timestep for the chunk and 0/1 masks: a pair's MLP input depends only on its class (fixed_i, fixed_j, d, bin) -- the MLP
            # once per class row, then a copy per pair, where the table is small against the pairs (ops.edge_embed_classes_eligible)
            by_class = cls is not None and ops.edge_embed_classes_eligible(
                self.ee_classes, self.arith, single_t and not per_sample, cls["n_fixed"], self._mask_is_01(node_mask), rel_cb.shape[1],
                w["bin_tab_cb"].shape[1], B, L)
            if edge_layout == "by_class" and not (by_class and next_proj is not None):
                edge_layout = "tiled"
            if by_class:
                # the two operand rows per fixed-mask value, by the launch that made the chunk's: the same sums, the same floats
                _, node_a2, node_b2 = torch.ops.str2str_amd.embed_assemble(img.contiguous(), cls["nc2"], cls["fa2"], cls["fb2"], 1,
                                                                           cls["n_fixed"], False, True)
                edge_embed = ops.edge_embed_classes_f16x3(node_a2, node_b2, cls["fixed_cls"], rel_cb, w["bin_tab_cb"], w["bin_lower"], idx_dev,
                                                          ca, ws, e2.bias, w["b3c"], ln.weight, ln.bias, mask, span, ln.eps, proj=proj,
                                                          out_layout=edge_layout)
            else:
                edge_embed = ops.edge_embed_f16x3(node_a, node_b, rel_cb, w["bin_tab_cb"], w["bin_lower"], idx_dev, ca, ws, e2.bias,
                                                  w["b3c"], ln.weight, ln.bias, mask, span, ln.eps, proj=proj, column_blocked_tables=True,
                                                  out_layout=edge_layout)
        else:
            if edge_layout != "rowmajor":
                raise ops.HipLibraryError("EmbeddingModule: the tiled pair layout belongs to the f16x3 kernels")
            edge_embed = ops.edge_embed(node_a, node_b, rel_tab, w["bin_tab"], w["bin_lower"], idx_dev, ca, w["w2p"],
                                        w["w3p"], e2.bias, w["b3c"], ln.weight, ln.bias, mask, span, ln.eps,
                                        proj=None if next_proj is None else (next_proj["wp"], next_proj["b64"]))
        if next_proj is not None:
            edge_embed, *proj = edge_embed
            return node_embed, node_act, edge_embed, tuple(proj)
        return node_embed, node_act, edge_embed, None


def _table_linear(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [..., 32] W^T (+ b) for the per-target / per-timestep tables of the embedder, on the exact fp32 node kernel
    (s2s_node_linear_f32): the package has no library GEMM path."""
    layer = ops.pack_node_layer(w, b if b is not None else torch.zeros(w.shape[0], device=w.device))
    lead, n = x.shape[:-1], x.numel() // x.shape[-1]
    y, _ = ops.node_apply(x.reshape(n, x.shape[-1]).float().contiguous(), layer, n)
    return y[:, : w.shape[0]].reshape(*lead, w.shape[0]).contiguous()


class DenoisingNet(nn.Module):
    def __init__(self, embedder: nn.Module, translator: nn.Module):
        super().__init__()
        self.embedder = embedder
        self.translator = translator
        self.backbone_in_forward = True  # the sampler turns this off inside its loop (result unused there)

    @staticmethod
    def blend_psi(psi: torch.Tensor, torsion_angles_sin_cos: torch.Tensor, fixed_mask: torch.Tensor) -> torch.Tensor:
        """gt_psi * fixed + psi * (1 - fixed) (reference :192-193; the result takes the features' dtype, as there)."""
        gt_psi = torsion_angles_sin_cos.to(psi.device)[..., 2, :]
        fixed_mask = fixed_mask.to(psi.device).type(torch.float)
        return gt_psi * fixed_mask[..., None] + psi * (1 - fixed_mask[..., None])

    def forward(self, batch: dict, as_tensor_7: bool = False, defer_psi_blend: bool = False) -> dict:
        """reference :171-211: {'rigids', 'psi', 'atom37', 'atom14'} (+ 'rigids7', the frames as one tensor).
        ``defer_psi_blend`` (the sampler's loop): 'psi' is the torsion head's own output and 'psi_deferred' is set -- the blend with the
        input torsion under the fixed mask (:192-193; float64 for float64 features) feeds nothing inside the loop, the sampler
        applies it once to the last evaluation (``blend_psi``)."""
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise ops.HipLibraryError(
                "DenoisingNet.forward needs the HIP device (MI355X): the sampling path has no CPU fallback")
        node_mask = batch["residue_mask"].to(dev).type(torch.float)
        fixed_mask = batch["fixed_mask"].to(dev).type(torch.float)
        fuse = getattr(self.translator, "fuse_pair_projection", False)
        # between the f16x3 pair kernels (embedding -> EdgeTransition 0 -> 1 -> ..) the pair tensor travels in their tiled layout
        # (producer and consumer both on their f16x3 kernels; the consumer of the embedding's pair tensor is EdgeTransition 0)
        et0 = self.translator.trunk["edge_transition_0"] if "edge_transition_0" in getattr(self.translator, "trunk", {}) else None
        tiled = fuse and getattr(self.embedder, "arith", None) == "f16x3" and getattr(et0, "arith", None) == "f16x3"
        node_embed, node_act, edge_embed, first_proj = self.embedder.embed(
            residue_idx=batch["residue_idx"], t=batch["t"], fixed_mask=fixed_mask, self_conditioning_ca=batch["sc_ca_t"], node_mask=node_mask,
            t_emb=batch.get("t_emb"), t_img=batch.get("t_img"), next_proj=self.translator.trunk["ipa_0"].pair_proj_weights() if fuse else None,
            **({"edge_layout": "by_class" if getattr(self.embedder, "et_by_class", "0") != "0" else "tiled"} if tiled else {}))
        tb = dict(batch)
        tb["residue_mask"], tb["fixed_mask"] = node_mask, fixed_mask
        tb["rigids_t"] = batch["rigids_t"].to(dev)
        tb["_node_embed_act"] = node_act
        model_out = self.translator(node_embed, edge_embed, tb, **({"_first_proj": first_proj} if fuse else {}))
        if model_out.get("psi_blended") or defer_psi_blend:     # (the torsion head's kernel blends float32 features in its own launch)
            psi_pred = model_out["psi"]
        else:
            psi_pred = self.blend_psi(model_out["psi"], batch["torsion_angles_sin_cos"], fixed_mask)
        rigids_pred = model_out["out_rigids"]
        out = {"rigids": rigids_pred, "psi": psi_pred, "rigids7": model_out["out_rigids7"]}
        if defer_psi_blend and not model_out.get("psi_blended"):
            out["psi_deferred"] = True
        if self.backbone_in_forward:
            aatype = batch["aatype"].to(dev) if "aatype" in batch else None
            bb = compute_backbone(rigids_pred, psi_pred, aatype=aatype, _rigids7=model_out["out_rigids7"])
            out["atom37"], out["atom14"] = bb[0], bb[-1]
        if as_tensor_7:
            out["rigids"] = model_out["out_rigids7"]
        return out
