"""EmbeddingModule.forward on the HIP kernels (s2s_embed_assemble, the node MLP, s2s_edge_embed / s2s_edge_embed_f16x3 with and without
the fused pair projection, row-major and tiled) against the float64 statement of the reference formula (tests/ref_embed.py), in both
arithmetics, through every way the module receives the timestep, at the shapes and residue numberings of tests/embed_cases.py.

Bound: 3 x the pooled distance of the reference's float32 chain from float64 over the case table (embed_cases.rule_bound; the
kernels are that chain with another summation order), never more than the project's 5e-6 of the output scale; on an MI355X that
rule already sits within 1.4 x to 4 x of the achieved margins (embed_cases.bound, profiles/parity_margins.json).  No pair, residue
or sample is left out of a comparison and no number of differing pairs is allowed: the cases are clear of the distogram's bin
edges, so one wrong pair fails.  The bin edges themselves are held by the exact-edge case, where the bin a kernel used is read off
its output.
"""
import functools

import pytest
import torch

import embed_cases as EC
import ref_embed
from conftest import record_margin, synth_sd
from str2str_amd.arith import use_arith

pytestmark = pytest.mark.gpu

DEV = "cuda"
MODES = ["f16x3", "f32"]
ENTRIES = ("t", "t_emb", "t_img", "t_img_rows")   # t on the host | one t_emb row | one shared t_img row | t_img [B, 512]
SHARED = ("t_emb", "t_img")                       # the forms that mean: sample 0's t on every sample


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module")
def net():
    from str2str_amd.factory import build_synthetic_net

    return build_synthetic_net(seed=0, sigma_final=0.02, device=DEV)


@pytest.fixture(scope="module")
def sd():
    return synth_sd(0, 0.02)


def call(emb, c, entry, masked, residue_idx=None, fixed_mask=None, **kw):
    """The module on case ``c`` with the timestep handed in as ``entry``."""
    from str2str_amd.models.net.denoising_ipa import get_timestep_embedding

    t = c["t"]
    if entry == "t":
        tk = dict(t=t)
    elif entry == "t_emb":
        tk = dict(t=None, t_emb=get_timestep_embedding(t[:1], 32))
    elif entry == "t_img":
        tk = dict(t=None, t_img=emb.time_images(get_timestep_embedding(t[:1], 32))[0])
    else:
        tk = dict(t=None, t_img=emb.time_images(get_timestep_embedding(t, 32)))
    return emb(residue_idx=c["residue_idx"] if residue_idx is None else residue_idx,
               fixed_mask=c["fixed_mask"].to(DEV) if fixed_mask is None else fixed_mask, self_conditioning_ca=c["ca"].to(DEV),
               node_mask=c["node_mask"].to(DEV) if masked else None, **tk, **kw)


@functools.lru_cache(maxsize=None)
def _ref_of_table_case(name, shared):
    c = EC.case(name)
    return ref_embed.embedding64(synth_sd(0, 0.02), *EC.inputs(EC.shared_t(c) if shared else c), device=DEV)


def reference(c, entry, masked):
    """(node64, edge64) on the device for a case of the table: evaluated once per (case, shared t or not), masked afterwards."""
    node, edge = _ref_of_table_case(c["name"], entry in SHARED and c["B"] > 1)
    return ref_embed.apply_mask(node, edge, c["node_mask"] if masked else None)


def _explain(sd, c, entry, masked, got_edge, where, bound):
    """Which planted mistake of the reference, if any, reproduces the kernel's row at the worst pair."""
    b, i, j = where
    cc = EC.shared_t(c) if entry in SHARED else c
    hits = []
    for m in ref_embed.MUTATIONS:
        _, e = ref_embed.embedding64(sd, *EC.inputs(cc), node_mask=c["node_mask"] if masked else None, mutate=m, device=DEV)
        if float((got_edge[b, i, j].double() - e[b, i, j]).abs().max()) < bound:
            hits.append(m)
    idx = c["residue_idx"]
    d = float(torch.linalg.norm(c["ca"][b, i] - c["ca"][b, j]))
    return (f"pair (b={b}, i={i}, j={j}): idx_i - idx_j = {int(idx[b, i] - idx[b, j])}, fixed = ({int(c['fixed_mask'][b, i])}, "
            f"{int(c['fixed_mask'][b, j])}), |ca_i - ca_j| = {d:.6f}, t = {float(cc['t'][b])}; matches the reference mutated by: {hits or 'none'}")


def compare(sd, arith, output, got, ref, label, mask=None, explain=None):
    """max |got - float64| under the bound in force, over EVERY entry; masked entries exactly 0; everything finite."""
    assert got.shape == ref.shape, (label, output, got.shape, ref.shape)
    assert torch.isfinite(got).all(), (label, output)
    err = (got.double() - ref).abs()
    achieved, b = float(err.max()), EC.bound(sd, output, arith)
    record_margin(f"embedder {arith} vs float64: {output}", achieved, b)
    print(f"{label} {arith} {output}: {achieved:.3e} (bound {b:.3e})")
    if mask is not None:
        assert (got[mask == 0] == 0).all(), (label, output, "a masked entry is not exactly 0")
    if not achieved < b:
        where = tuple(int(v) for v in (err == err.max()).nonzero()[0])
        n_bad = int((err.reshape(-1, err.shape[-1]).amax(-1) >= b).sum()) if output != "attn_bias" else int((err >= b).sum())
        more = explain(where[:3], b) if explain is not None else ""
        raise AssertionError(f"{label} {arith} {output}: {achieved:.3e} >= {b:.3e} at {where}; {n_bad} rows off. {more}")


def check_node_edge(sd, arith, c, entry, masked, node, edge, label=None):
    label = label or f"{c['name']} {entry}{' masked' if masked else ''}"
    rn, re = reference(c, entry, masked)
    m = c["node_mask"].to(DEV) if masked else None
    compare(sd, arith, "node", node, rn, label, mask=m)
    compare(sd, arith, "edge", edge, re, label, mask=None if m is None else m[:, :, None] * m[:, None, :],
            explain=lambda w, b: _explain(sd, c, entry, masked, edge, w, b))


# ------------------------------------------------------------------------------------------------ module against embedding64
def _plan(name):
    """[(entry, masked)]: small cases take every timestep entry with and without node_mask; the large shapes run once per
    arithmetic and entry family (the sampler's per-sample t_img masked, t on the host unmasked)."""
    if name in EC.LARGE:
        return [("t_img_rows", True), ("t", False)] if name != "n257-gaps" else [("t_img_rows", True)]
    return [(e, m) for e in ENTRIES for m in (False, True)]


@pytest.mark.parametrize("arith", MODES)
@pytest.mark.parametrize("name", EC.NAMES)
def test_module_vs_float64(net, sd, name, arith, monkeypatch):
    """Node and edge embedding of one case through each timestep entry; (5, 24) runs under the per-launch pair budget
    S2S_EE_MAX_PAIRS = 2 N N + 7 (launches of 2 + 2 + 1 samples), so the pointer offsets of a split launch are held to the
    reference too and not only to the unsplit launch."""
    c = EC.case(name)
    if c["max_pairs"]:
        monkeypatch.setenv("S2S_EE_MAX_PAIRS", str(c["max_pairs"]))
    with use_arith(net, arith):
        for entry, masked in _plan(name):
            node, edge = call(net.embedder, c, entry, masked)
            check_node_edge(sd, arith, c, entry, masked, node, edge)


@pytest.mark.parametrize("arith", MODES)
def test_many_tiles_unmasked_t_on_host(net, sd, arith):
    """(2, 257) once more per arithmetic without a mask and with t on the host (the multi-t branch at more than 1024 tiles)."""
    c = EC.case("n257-gaps")
    with use_arith(net, arith):
        node, edge = call(net.embedder, c, "t", False)
    check_node_edge(sd, arith, c, "t", False, node, edge)


# ------------------------------------------------------------------------------------------------ fused pair projection
@pytest.mark.parametrize("arith", MODES)
@pytest.mark.parametrize("name", ["n1", "n7-gaps", "n32-break", "n37-perm", "n24-split", "n130-break", "n257-gaps"])
def test_fused_projection_vs_float64(net, sd, name, arith, monkeypatch):
    """With the first IPA block's projection fused into the producer: the pair tensor is bit for bit the one of the call without it,
    and attn_bias [B, 8, L, L] / pair_z [B, L, L, 32] meet pair_projection64 of the float64 (masked) pair tensor.  f16x3 with the
    tiled output layout: pair_untiled of it is the row-major result bit for bit, same projections -- the link that puts the tiled
    layout under the float64 comparison."""
    from str2str_amd import ops

    c = EC.case(name)
    if c["max_pairs"]:
        monkeypatch.setenv("S2S_EE_MAX_PAIRS", str(c["max_pairs"]))
    entry, masked = "t_img_rows", name != "n1"
    proj = net.translator.trunk["ipa_0"].pair_proj_weights()
    with use_arith(net, arith):
        node0, edge0 = call(net.embedder, c, entry, masked)
        node, edge, (bias, pz) = call(net.embedder, c, entry, masked, next_proj=proj)
        assert torch.equal(edge, edge0) and torch.equal(node, node0)
        if arith == "f16x3":
            _, tiled, (bias_t, pz_t) = call(net.embedder, c, entry, masked, next_proj=proj, edge_layout="tiled")
            assert isinstance(tiled, ops.PairTiled) and torch.equal(ops.pair_untiled(tiled), edge)
            assert torch.equal(bias_t, bias) and torch.equal(pz_t, pz)
            assert torch.equal(ops.pair_untiled(call(net.embedder, c, entry, masked, edge_layout="tiled")[1]), edge)
    label = f"{name} fused projection"
    check_node_edge(sd, arith, c, entry, masked, node, edge, label)
    ab64, pz64 = ref_embed.pair_projection64(sd, EC.IPA0, reference(c, entry, masked)[1])
    compare(sd, arith, "attn_bias", bias, ab64, label)
    compare(sd, arith, "pair_z", pz, pz64, label)


# ------------------------------------------------------------------------------------------------ the bin edges themselves
@pytest.mark.parametrize("arith", MODES)
@pytest.mark.parametrize("axis,entry", [(0, "t"), (1, "t_img_rows")])
def test_exact_edge_case_bins(net, sd, axis, entry, arith):
    """72 two-residue samples whose CA distance is a float32 bin edge, its neighbours one ulp up and down, 0, 5e-6, 25, 9.9e7, 1e8
    and 2e8 (exact in float32).  The bin the kernel used = the one forced-bin evaluation of embedding64 (22 bins or none) that lies
    within the bound of the kernel's row; it must be unique and equal the reference's (embed_cases.exact_edge_case), for pair (0, 1)
    and the transposed pair (1, 0) of every sample.  The whole output is compared as well."""
    c = EC.exact_edge_case(axis)
    with use_arith(net, arith):
        node, edge = call(net.embedder, c, entry, False)
    forced = torch.stack([ref_embed.embedding64(sd, *EC.inputs(c), force_bin=k, device=DEV)[1] for k in range(-1, 22)])   # [23, 72, 2, 2, 128]
    b = EC.bound(sd, "edge", arith)
    within = (edge.double()[None] - forced).abs().amax(-1) < b                                                           # [23, 72, 2, 2]
    assert (within.sum(0) == 1).all(), ("the kernel's row matches no forced bin, or several", (within.sum(0) != 1).nonzero()[:8])
    used = within.int().argmax(0) - 1
    want = c["bins"].to(DEV)
    for i, j in ((0, 1), (1, 0)):
        wrong = (used[:, i, j] != want).nonzero().flatten()
        assert wrong.numel() == 0, (f"pair ({i}, {j})", [(int(s), float(c["ca"][s, 1, axis]), int(used[s, i, j]), int(want[s])) for s in wrong[:8]])
    assert (used[:, 0, 0] == -1).all() and (used[:, 1, 1] == -1).all()
    rn, re = ref_embed.embedding64(sd, *EC.inputs(c), device=DEV)
    compare(sd, arith, "node", node, rn, c["name"])
    compare(sd, arith, "edge", edge, re, c["name"])


# ------------------------------------------------------------------------------------------------ no self-conditioning
@pytest.mark.parametrize("arith", MODES)
def test_module_without_self_conditioning(sd, arith):
    """A stand-alone EmbeddingModule(32, 256, 128, self_conditioning=False) with the synthetic embedder weights (first edge layer
    cut to its 98 non-distogram columns) at (2, 37), against embedding64(..., self_conditioning=False) of its own state_dict().
    The CA argument is ignored: non-zero CA gives the bits of zero CA."""
    from str2str_amd.models.net.denoising_ipa import EmbeddingModule

    emb = EmbeddingModule(32, 256, 128, self_conditioning=False)
    own = {k[len("embedder."):]: v.clone() for k, v in sd.items() if k.startswith("embedder.")}
    own["edge_embed.0.weight"] = own["edge_embed.0.weight"][:, :98].contiguous()
    emb.load_state_dict(own, strict=True)
    emb = emb.to(DEV).eval()
    full = EC.case("n37-gaps")
    c = {k: (v[:2] if isinstance(v, torch.Tensor) else v) for k, v in full.items()}
    c["B"] = 2
    own_sd = {k: v.detach().cpu() for k, v in emb.state_dict().items()}
    with use_arith(emb, arith):
        for entry, masked in (("t", False), ("t_img_rows", True), ("t_img", True)):
            node, edge = call(emb, c, entry, masked)
            cc = EC.shared_t(c) if entry in SHARED else c
            rn, re = ref_embed.embedding64(own_sd, *EC.inputs(cc), node_mask=c["node_mask"] if masked else None, prefix="",
                                           self_conditioning=False, device=DEV)
            compare(sd, arith, "node", node, rn, f"no self-conditioning {entry}")
            compare(sd, arith, "edge", edge, re, f"no self-conditioning {entry}")
            zero = dict(c)
            zero["ca"] = torch.zeros_like(c["ca"])
            assert torch.equal(call(emb, zero, entry, masked)[1], edge)


# ------------------------------------------------------------------------------------------------ host-side caches
@pytest.mark.parametrize("entry", ["t_img_rows", "t"])
@pytest.mark.parametrize("arith", MODES)
def test_caches_cannot_serve_stale_tables(net, sd, arith, entry):
    """The per-target tables are cached on tensor identity and version.  On one module: case A; residue_idx changed IN PLACE to a
    numbering of another span; a NEW tensor with A's numbers; fixed_mask changed in place; edge_embed[0].weight scaled in place,
    then restored.  Every evaluation against embedding64 of the inputs as they were at that call."""
    emb = net.embedder
    A = EC.case("n7-gaps")
    B, N = A["B"], A["N"]
    idx, fixed = A["residue_idx"].clone(), A["fixed_mask"].clone().to(DEV)
    w0 = emb.edge_embed[0].weight
    keep = w0.detach().clone()

    def step(what, sd_now=sd):
        node, edge = call(emb, A, entry, True, residue_idx=idx, fixed_mask=fixed)
        rn, re = ref_embed.embedding64(sd_now, idx.clone(), A["t"], fixed.cpu(), A["ca"], node_mask=A["node_mask"], device=DEV)
        compare(sd, arith, "node", node, rn, f"caches: {what}")
        compare(sd, arith, "edge", edge, re, f"caches: {what}")

    try:
        with use_arith(net, arith):
            step("case A")
            idx.copy_(EC.numbering("break", B, N, None))
            step("residue_idx changed in place (span 57 -> 1006)")
            idx = A["residue_idx"].clone()
            step("a new tensor with A's numbering")
            fixed.copy_(1.0 - fixed)
            step("fixed_mask changed in place")
            w0.mul_(2.0)
            scaled = dict(sd)
            scaled["embedder.edge_embed.0.weight"] = sd["embedder.edge_embed.0.weight"] * 2.0
            step("edge_embed[0].weight scaled in place", scaled)
            w0.mul_(0.5)
            assert torch.equal(w0, keep)
            step("edge_embed[0].weight restored")
    finally:
        w0.copy_(keep)
