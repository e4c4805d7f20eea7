"""The expansion kernel of the edge embedding by class (s2s_edge_embed_expand) alone, on a table of arbitrary values, against the
present launch (s2s_edge_embed_f16x3) and the whole class path in one process, at cfg2's shape; the two paths' outputs compared as
int32 (profiles/r07_ee_classes_stop_rule.md).

    [EE_B=128 EE_N=256] python tools/ee_classes_stop_rule.py     [OUT.json]  -> JSON on stdout (and in OUT.json)
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from str2str_amd import ops  # noqa: E402
from str2str_amd.factory import build_synthetic_net  # noqa: E402
from str2str_amd.ops.binding import _p, _stream  # noqa: E402

B, N = int(os.environ.get("EE_B", 128)), int(os.environ.get("EE_N", 256))
dev = "cuda:0"
net = build_synthetic_net(seed=0, sigma_final=0.002, device=dev)
emb = net.embedder
proj = net.translator.trunk["ipa_0"].pair_proj_weights()
gen = torch.Generator().manual_seed(5)
idx = torch.arange(N)[None].repeat(B, 1)
t = torch.full((B,), 0.37)
fixed = torch.zeros(B, N, device=dev)
ca = (8.0 * torch.randn(B, N, 3, generator=gen)).to(dev)
mask = torch.ones(B, N, device=dev)
from str2str_amd.models.net.denoising_ipa import get_timestep_embedding  # noqa: E402
T_IMG = emb.time_images(get_timestep_embedding(torch.full((1,), 0.37), 32))[0]
out = {}


def run(mode, reps=5):
    emb.ee_classes = mode
    r = emb.embed(idx, None, fixed, ca, node_mask=mask, next_proj=proj, edge_layout="tiled", t_img=T_IMG)
    torch.cuda.synchronize()
    with ops.KernelTimer("s2s_edge_embed") as kt:
        for _ in range(reps):
            r = emb.embed(idx, None, fixed, ca, node_mask=mask, next_proj=proj, edge_layout="tiled", t_img=T_IMG)
        ms, n = kt.mean_ms("s2s_edge_embed")
    return ms, r


res = {}
ms0, r0 = run("0")
ms1, r1 = run("1")
ms0b, _ = run("0")
ms1b, _ = run("1")
res["present_ms"] = [ms0, ms0b]
res["classes_ms"] = [ms1, ms1b]
z0, z1 = r0[2].buf, r1[2].buf
res["z_bits_equal"] = bool(torch.equal(z0.view(torch.int32), z1.view(torch.int32)))
res["attn_bias_bits_equal"] = bool(torch.equal(r0[3][0].view(torch.int32), r1[3][0].view(torch.int32)))
res["pair_z_bits_equal"] = bool(torch.equal(r0[3][1].view(torch.int32), r1[3][1].view(torch.int32)))
res["node_equal"] = bool(torch.equal(r0[0], r1[0]))
print(json.dumps(res), flush=True)

# expansion alone on a table of arbitrary values
lib = ops.load_library()
w = emb._weights()
rel_tab, span, node_pos, idx_dev, rel_cb = emb._tables(idx, w["w_rel"], w["wn_pos"])
n_rel, n_bins = rel_cb.shape[1], w["bin_tab_cb"].shape[1]
rows = ops.edge_embed_class_rows(1, n_rel, n_bins)
res["rows"] = rows
table = torch.randn(rows, 168, device=dev)
cls = torch.zeros(B, N, dtype=torch.int32, device=dev)
zt = ops.PairTiled(B, N, dev)
ab, pz = torch.empty(B, 8, N, N, device=dev), torch.empty(B, N, N, 32, device=dev)
zr = r0[2].buf.new_empty(B, N, N, 128)
for name, o, tiled in (("expand_tiled_ms", zt.buf, 1), ("expand_rowmajor_ms", zr, 0)):
    def go():
        rc = lib.s2s_edge_embed_expand(_p(table), _p(cls), _p(w["bin_lower"]), _p(idx_dev), _p(ca), _p(mask), _p(proj["b64"]), _p(o), tiled,
                                       _p(ab), _p(pz), B, N, span, n_rel, n_bins, _stream())
        assert rc == 0, rc
    go()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(5):
        go()
    b.record()
    torch.cuda.synchronize()
    res[name] = a.elapsed_time(b) / 5
res["B"], res["N"] = B, N
print(json.dumps(res), flush=True)
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
