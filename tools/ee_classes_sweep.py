"""Edge embedding by class against the present kernel, per shape: `EmbeddingModule.embed` with ee_classes "0" / "1" alternating, every
launch of the family between its own pair of HIP events (s2s_edge_embed_f16x3 | s2s_edge_embed_classes_f16x3 + s2s_edge_embed_expand).
Where the class-row threshold `ops.EE_CLASS_R` comes from (profiles/r07_ee_classes_threshold.md).

    python tools/ee_classes_sweep.py        [OUT.json]  -> one JSON line per (B, N, fixed values present) (and the list in OUT.json)
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from str2str_amd import ops  # noqa: E402
from str2str_amd.factory import build_synthetic_net  # noqa: E402

dev = "cuda:0"
net = build_synthetic_net(seed=0, sigma_final=0.002, device=dev)
emb = net.embedder
proj = net.translator.trunk["ipa_0"].pair_proj_weights()
lib = ops.load_library()
from str2str_amd.models.net.denoising_ipa import get_timestep_embedding  # noqa: E402
T_IMG = emb.time_images(get_timestep_embedding(torch.full((1,), 0.37), 32))[0]
EV = {}


def wrap(name):
    f = getattr(lib, name)

    def g(*a):
        a0, b0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a0.record()
        rc = f(*a)
        b0.record()
        EV.setdefault(name, []).append((a0, b0))
        return rc
    setattr(lib, name, g)


for n in ("s2s_edge_embed_f16x3", "s2s_edge_embed_classes_f16x3", "s2s_edge_embed_expand"):
    wrap(n)

SHAPES = [(100, 35), (400, 35), (1000, 35), (4000, 35), (16, 80), (64, 80), (256, 80), (1000, 80), (1, 256), (4, 256), (16, 256), (128, 256)]
rows_out = []
gen = torch.Generator().manual_seed(5)
for nf in (1, 2):
    for B, N in SHAPES:
        idx = torch.arange(N)[None].repeat(B, 1)
        t = torch.full((B,), 0.37)
        fixed = torch.zeros(B, N, device=dev)
        if nf == 2:
            fixed[:, ::3] = 1.0
        ca = (8.0 * torch.randn(B, N, 3, generator=gen)).to(dev)
        mask = torch.ones(B, N, device=dev)
        rec = dict(B=B, N=N, n_fixed=nf, pairs=B * N * N, rows=ops.edge_embed_class_rows(nf, 2 * (N - 1) + 1, 22))
        for mode in ("0", "1", "0", "1"):
            emb.ee_classes = mode
            for rep in range(6):
                if rep == 1:
                    torch.cuda.synchronize()
                    EV.clear()
                r = emb.embed(idx, None, fixed, ca, node_mask=mask, next_proj=proj, edge_layout="tiled", t_img=T_IMG)
            torch.cuda.synchronize()
            for k, ev in EV.items():
                rec.setdefault(k.replace("s2s_edge_embed_", "") + "_us", []).append(round(1e3 * sum(a.elapsed_time(b) for a, b in ev) / len(ev), 1))
            del r
        rows_out.append(rec)
        print(json.dumps(rec), flush=True)
if len(sys.argv) > 1:
    json.dump(rows_out, open(sys.argv[1], "w"), indent=1)
