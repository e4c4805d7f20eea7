"""Stop rule of the first edge transition reading by class (profiles/r08_et_by_class_stop_rule.md): the expansion of the edge embedding's
class table + EdgeTransition 0, as they run today (tiled z materialised, then read back) against the by-class pair (the expansion writes
one class index per pair, the transition reads its rows out of the table), in one process at cfg2's shape, on the table the table kernel
computes for a noised synthetic chain; the two paths' outputs compared as int32.

    [ET_B=128 ET_N=256 ET_NOISE=10] [STR2STR_HIP_LIB=variant.so] python tools/et_by_class_stop_rule.py [OUT.json]  -> JSON on stdout

Times are HIP events on the launch stream around the library calls (ops.KernelTimer): "embed" = table kernel + expansion (the table
kernel is the same launch in both), "et" = the transition; 5 launches after a warm-up each, two interleaved series.  A library variant
is measured by a second run of this script; the variants of the profile (non-temporal table loads, another slot for the class-index request)
were built from the source at commit 2f5af7f, which had a build-time switch for each.
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from str2str_amd import ops  # noqa: E402
from str2str_amd.factory import build_synthetic_net  # noqa: E402
from str2str_amd.models.net.denoising_ipa import get_timestep_embedding  # noqa: E402
from str2str_amd.synth import synth_chain  # noqa: E402

B, N, NOISE = int(os.environ.get("ET_B", 128)), int(os.environ.get("ET_N", 256)), float(os.environ.get("ET_NOISE", 10.0))
dev = "cuda:0"
net = build_synthetic_net(seed=0, sigma_final=0.002, device=dev)
emb, trunk = net.embedder, net.translator.trunk
emb.ee_classes = "1"
et = trunk["edge_transition_0"]
proj0, proj1 = trunk["ipa_0"].pair_proj_weights(), trunk["ipa_1"].pair_proj_weights()
gen = torch.Generator().manual_seed(5)
feats = synth_chain(N)
ca0 = feats["rigidgroups_gt_frames"][..., 0, :3, 3].reshape(1, N, 3).float()
ca = (ca0 + NOISE * torch.randn(B, N, 3, generator=gen)).to(dev)      # every replica its own noise: the classes in use are the sampler's
idx = torch.arange(N)[None].repeat(B, 1)
fixed = torch.zeros(B, N, device=dev)
mask = torch.ones(B, N, device=dev)
T_IMG = emb.time_images(get_timestep_embedding(torch.full((1,), 0.37), 32))[0]
NAMES = ("s2s_edge_embed", "s2s_edge_transition")


def run(layout, reps=5):
    def once():
        _, act, edge, _ = emb.embed(idx, None, fixed, ca, node_mask=mask, next_proj=proj0, edge_layout=layout, t_img=T_IMG)
        n_p, node_ab = et.node_parts(act, B * N, kernel_form=True)
        return edge, et.pair_mlp(edge, node_ab.view(B, N, -1), n_p.view(B, N, -1), mask, proj1, out_layout="tiled", ab_kernel_form=True)

    edge, r = once()
    torch.cuda.synchronize()
    with ops.KernelTimer(*NAMES) as kt:
        for _ in range(reps):
            edge, r = once()
        ms = [kt.mean_ms(n)[0] for n in NAMES]
    return ms, edge, r


res = {"B": B, "N": N, "noise": NOISE, "lib": os.environ.get("STR2STR_HIP_LIB", "")}
series = {"tiled": [], "by_class": []}
keep = {}
for _ in range(2):
    for layout in ("tiled", "by_class"):
        ms, edge, r = run(layout)
        series[layout].append({"embed_ms": ms[0], "et_ms": ms[1], "pair_ms": ms[0] + ms[1]})
        keep[layout] = (edge, r)
        del edge, r
res["series"] = series
mean = lambda xs: sum(xs) / len(xs)  # noqa: E731
res["present_pair_ms"] = mean([s["pair_ms"] for s in series["tiled"]])
res["new_pair_ms"] = mean([s["pair_ms"] for s in series["by_class"]])
res["gain_ms"] = res["present_pair_ms"] - res["new_pair_ms"]
(e0, r0), (e1, r1) = keep["tiled"], keep["by_class"]
assert isinstance(e1, ops.PairByClass), type(e1)
res["classes_in_use"] = int(torch.unique(e1.index).numel())
n_out = B * N * N * 128   # (whole 32-pair blocks are whole [16][2][32][4] units: the pairs past the end of a ragged last block are never written)
z0, z1 = (r0[0].buf, r1[0].buf) if n_out == r0[0].buf.numel() else (ops.pair_untiled(r0[0]), ops.pair_untiled(r1[0]))
res["z_out_bits_equal"] = bool(torch.equal(z0.view(torch.int32), z1.view(torch.int32)))
res["attn_bias_bits_equal"] = bool(torch.equal(r0[1].view(torch.int32), r1[1].view(torch.int32)))
res["pair_z_bits_equal"] = bool(torch.equal(r0[2].view(torch.int32), r1[2].view(torch.int32)))
res["range_flag"] = int(ops.range_flag_read(torch.device(dev)))
print(json.dumps(res), flush=True)
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
