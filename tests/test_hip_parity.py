"""HIP path (through the C ABI) vs the reference-generated golden fixtures and vs the CPU oracle on
the same seeded inputs.  Needs a real MI355X: every test is marked ``gpu``.

Tolerances (float32 path; the reference itself is float32).  Every bound is at most ~5x the margin achieved on an MI355X
(profiles/parity_margins.json), so a regression of one order of magnitude fails:
  per-op            <= 5e-6 relative to the output scale (1e-6 for the pure geometry kernels)
  one network eval  <= 1e-4 absolute on frames (the oracle itself meets the reference at 2e-4)
  free-running trajectory with contractive weights: backbone RMSD <= 1e-4 Angstrom (north star; achieved <= 3.4e-5)
"""
import os
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import T, backbone_rmsd, golden, maxdiff, record_margin, synth_sd
from str2str_amd.arith import use_arith

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def rel(a, b):
    b = np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, dtype=np.float64)
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def _test_name():
    import os

    return os.environ.get("PYTEST_CURRENT_TEST", "?").split("::")[-1].split(" ")[0]


def check(name, achieved, bound):
    """assert achieved < bound, and keep the achieved margin for profiles/parity_margins.json"""
    record_margin(name, achieved, bound)
    assert achieved < bound, (name, achieved, bound)


@pytest.fixture(scope="module")
def net_rough():
    from str2str_amd.factory import build_synthetic_net

    return build_synthetic_net(seed=0, sigma_final=0.02, device=DEV)


@pytest.fixture(scope="module")
def net_smooth():
    from str2str_amd.factory import build_synthetic_net

    return build_synthetic_net(seed=0, sigma_final=0.002, device=DEV)


@pytest.fixture(scope="module")
def diffuser(tmp_path_factory):
    from str2str_amd.factory import build_diffuser

    return build_diffuser(str(tmp_path_factory.mktemp("so3cache")))


def test_native_library_is_loaded():
    from str2str_amd import ops

    ops.load_library()
    maps = open("/proc/self/maps").read()
    assert "libstr2str_hip.so" in maps
    assert torch.cuda.is_available() and "gfx950" in torch.cuda.get_device_properties(0).gcnArchName


def test_ops_reject_cpu_tensors():
    from str2str_amd import ops

    with pytest.raises(ops.HipLibraryError):
        ops.rigid_compose_update(torch.zeros(4, 7), torch.zeros(4, 6), torch.ones(4))


def test_rigid_compose_update_golden():
    from str2str_amd import ops

    g = golden("prims.npz")
    r7 = torch.cat([T(g["q"]), T(g["t"])], -1).to(DEV).contiguous()
    out = ops.rigid_compose_update(r7, T(g["upd"]).to(DEV).contiguous(), T(g["msk"])[:, 0].to(DEV).contiguous())
    assert maxdiff(out.cpu(), g["comp7"]) < 1e-6
    # scale / unscale are exact IEEE mul / div
    x = ops.rigid_scale_trans(r7, 0.1, divide=False).cpu()
    assert maxdiff(x[..., 4:], T(g["t"]) * 0.1) == 0 and maxdiff(x[..., :4], g["q"]) == 0
    y = ops.rigid_scale_trans(r7, 0.1, divide=True).cpu()
    assert maxdiff(y[..., 4:], T(g["t"]) / 0.1) == 0


def test_frames_to_backbone_golden():
    from str2str_amd.common.all_atom import compute_backbone
    from str2str_amd.common.rigid_utils import Rigid

    g = golden("backbone.npz")
    r = Rigid.from_tensor_7(T(g["rigids7"]).to(DEV))
    a37, m37, _, a14 = compute_backbone(r, T(g["psi"]).to(DEV), T(g["aatype"]).to(DEV))
    assert maxdiff(a37.cpu(), g["atom37"]) < 1e-5
    assert maxdiff(a14.cpu()[..., :5, :], g["atom14"][..., :5, :]) < 1e-5
    assert (m37.cpu().numpy() == g["mask37"]).all()


def _assert_rot_score_close(got, ref32, anchors, what=""):
    """Float64-anchored bound, every term produced by the REFERENCE's own functions (tests/golden/make_golden_score64.py):
        |ours - s64| <= |ref32 - s64| + 2 spread32 + alg32 + 4e-5 |s64|        per residue, nothing excluded
    s64 = the reference's series functions in float64 on its float32 rotation vector; spread32 = largest change of the float32
    reference's own output under one-ulp jitter of its inputs (64 draws); alg32 = 2-ulp libm sensitivity of
    omega = |xyz| angle / sin(angle/2) next to the 2 pi wrap, by finite difference on the float64 series.  The bound is
    validated against the reference on CPU (test_oracle_golden.py::test_rot_score_bound_covers_reference_chain_error).
    ``anchors`` = (s64, spread32, alg32).  Returns the mask of residues where the reference is float32-well-conditioned."""
    s64, spread, alg = (np.asarray(x, dtype=np.float64) for x in anchors)
    got, ref32 = np.asarray(got, dtype=np.float64), np.asarray(ref32, dtype=np.float64)
    mag = np.linalg.norm(s64, axis=-1)
    e_hip = np.linalg.norm(got - s64, axis=-1)
    e_ref = np.linalg.norm(ref32 - s64, axis=-1)
    tol = e_ref + 2 * spread + alg + 4e-5 * mag
    assert np.isfinite(got).all()
    ratio = float((e_hip / np.maximum(tol, 1e-300)).max())
    record_margin(f"rot_score[{what}]: max |ours-s64| / (|ref32-s64| + 2 spread32 + alg32 + 4e-5|s|)", ratio, 1.0)
    assert (e_hip <= tol).all(), (what, ratio)
    good = ((e_ref + 2 * spread + alg) <= 1e-5 * mag) & (mag > 0)
    if good.any():  # where the reference is float32-accurate, so are we -- against the reference's own value
        rel32 = float((np.linalg.norm(got - ref32, axis=-1)[good] / mag[good]).max())
        record_margin(f"rot_score[{what}]: max rel |ours-ref32| on well-conditioned residues", rel32, 4e-5)
        assert rel32 < 4e-5, (what, rel32)
    return good


def _anchors(prefix, idx=None, sel=None):
    g = golden("score64.npz")
    out = [g[f"{prefix}_score64"], g[f"{prefix}_spread32"], g[f"{prefix}_alg32"]]
    if idx is not None:
        out = [a[idx] for a in out]
    if sel is not None:
        out = [a[sel] for a in out]
    return out


def _edge_transition_module(net):
    return net.translator.trunk["edge_transition_0"]


MODES = ["f16x3", "f32"]   # the two arithmetics of every matrix product (str2str_amd/arith.py)


@pytest.mark.parametrize("mode", MODES)
def test_edge_transition_golden(net_rough, mode):
    g = golden("edge_transition.npz")
    et = _edge_transition_module(net_rough)
    with use_arith(net_rough, mode):
        out = et(T(g["node"]).to(DEV), T(g["edge"]).to(DEV))
    check(f"{_test_name()}: rel err", rel(out, g["out"]), 5e-6)


@pytest.mark.parametrize("N,amp", [(48, 3.0), (512, 3.0), (48, 900.0)])
def test_edge_transition_f16x3_is_fp32_equivalent(net_rough, N, amp):
    """f16x3 (two-way f16 split, three products per block, fp32 accumulate) vs the exact fp32-MFMA kernel on the same inputs: the two
    differ by fp32 rounding only, and the split kernel is no further from a float64 evaluation than the fp32 one.  N = 512 is the
    BASELINE configs[3] length (262 144 pairs per sample: every persistent workgroup walks ~8 tiles); amp = 900 drives the hidden
    activations to several thousand (the magnitudes of a trained checkpoint rather than of an initialisation) -- still inside f16's
    range: same accuracy, and the range guard stays quiet."""
    import torch.nn.functional as F

    from str2str_amd import ops

    et = _edge_transition_module(net_rough)
    g = torch.Generator().manual_seed(77)
    Bn = 2 if N < 100 else 1
    node = torch.randn(Bn, N, 256, generator=g).to(DEV)
    edge = (amp * torch.randn(Bn, N, N, 128, generator=g)).to(DEV)
    outs = {}
    for mode in ("f32", "f16x3"):
        with use_arith(net_rough, mode):
            ops.range_flag_reset()
            outs[mode] = et(node, edge)
            assert ops.range_flag_read() == 0
    # float64 evaluation of the reference formula (layers.py:170-185) on the GPU, in row blocks
    e32 = e16 = 0.0
    with torch.no_grad():
        n = et.initial_embed(node).double()
        for i0 in range(0, N, 64):
            i1 = min(N, i0 + 64)
            x = torch.cat([edge[:, i0:i1].double(), n[:, i0:i1, None, :].expand(Bn, i1 - i0, N, -1), n[:, None, :, :].expand(Bn, i1 - i0, N, -1)], -1)
            h = F.relu(F.linear(x, et.trunk[0].weight.double(), et.trunk[0].bias.double()))
            h = F.relu(F.linear(h, et.trunk[2].weight.double(), et.trunk[2].bias.double()))
            y = F.linear(h + x, et.final_layer.weight.double(), et.final_layer.bias.double())
            ref = F.layer_norm(y, (128,), et.layer_norm.weight.double(), et.layer_norm.bias.double(), et.layer_norm.eps)
            e32 = max(e32, float((outs["f32"][:, i0:i1].double() - ref).abs().max()))
            e16 = max(e16, float((outs["f16x3"][:, i0:i1].double() - ref).abs().max()))
            hmax = max(float(h.abs().max()), float(x.abs().max())) if i0 == 0 else hmax
    assert (hmax > 2000.0) == (amp > 100), hmax
    record_margin(f"edge transition f16x3 N={N} amp={amp:g} (hidden max {hmax:.3g}): max |out - float64| (fp32 kernel: {e32:.2e})", e16, 3 * e32 + 1e-6)
    assert float((outs["f32"] - outs["f16x3"]).abs().max()) < 1e-5
    assert e16 < 1e-5 and e16 < 3 * e32 + 1e-6, (e32, e16)


def test_edge_transition_block_exponent(net_rough):
    """``prescale_exp`` (include/str2str_hip.h, s2s_edge_transition_f16x3): the hidden activations as f16 planes of 2^-e x their value.
    On ordinary magnitudes e = 5 changes the result by rounding only (subnormal spacing of the low plane); with the first hidden
    layer scaled by 8e3 (both hidden layers' activations ~1e5 > 2^15; the weights keep their ordinary size, so the fixed 2^5 weight
    packing keeps its precision) the unscaled kernel raises the range flag, e = 5 keeps it quiet and stays as close to a float64
    evaluation as the exact fp32 kernel."""
    import copy

    import torch.nn.functional as F

    from str2str_amd import ops

    et = copy.deepcopy(_edge_transition_module(net_rough))
    g = torch.Generator().manual_seed(78)
    Bn, N = 2, 48
    node = torch.randn(Bn, N, 256, generator=g).to(DEV)
    edge = (3.0 * torch.randn(Bn, N, N, 128, generator=g)).to(DEV)

    def run(e, arith="f16x3"):
        et.prescale_exp, et.arith = e, arith
        ops.range_flag_reset()
        out = et(node, edge)
        return out, ops.range_flag_read()

    with torch.no_grad():
        o0, f0 = run(0)
        o5, f5 = run(5)
        assert f0 == 0 and f5 == 0
        check("edge transition block exponent 5 vs 0, ordinary magnitudes: max |diff|", float((o0 - o5).abs().max()), 8e-6)
        et.trunk[0].weight.mul_(8.0e3); et.trunk[0].bias.mul_(8.0e3)
        o32, _ = run(0, "f32")
        _, f0 = run(0)
        o5, f5 = run(5)
        assert f0 & 4 and f5 == 0, (f0, f5)
        n = et.initial_embed(node).double()
        x = torch.cat([edge.double(), n[:, :, None, :].expand(Bn, N, N, -1), n[:, None, :, :].expand(Bn, N, N, -1)], -1)
        h1 = F.relu(F.linear(x, et.trunk[0].weight.double(), et.trunk[0].bias.double()))
        h = F.relu(F.linear(h1, et.trunk[2].weight.double(), et.trunk[2].bias.double()))
        y = F.linear(h + x, et.final_layer.weight.double(), et.final_layer.bias.double())
        ref = F.layer_norm(y, (128,), et.layer_norm.weight.double(), et.layer_norm.bias.double(), et.layer_norm.eps)
        assert float(h1.abs().max()) > 2.0 ** 15 and float(h.abs().max()) > 2.0 ** 15
        e32, e5 = float((o32.double() - ref).abs().max()), float((o5.double() - ref).abs().max())
        check(f"edge transition block exponent 5, hidden max {float(h1.abs().max()):.3g}: max |out - float64| (fp32 kernel: {e32:.2e})",
              e5, 3 * e32 + 1e-6)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,N", [(1, 5), (2, 37), (3, 64)])
def test_edge_transition_vs_oracle(net_rough, B, N, mode):
    from oracle import net as ON

    sd = synth_sd(0, 0.02)
    g = torch.Generator().manual_seed(100 + N)
    node = torch.randn(B, N, 256, generator=g)
    edge = torch.randn(B, N, N, 128, generator=g)
    mask = (torch.rand(B, N, generator=g) > 0.2).float()
    ref = ON.edge_transition(sd, "translator.trunk.edge_transition_0", node, edge) * (mask[:, :, None] * mask[:, None, :])[..., None]
    with use_arith(net_rough, mode):
        out = _edge_transition_module(net_rough)(node.to(DEV), edge.to(DEV), edge_mask_1d=mask.to(DEV))
    check(f"{_test_name()}: rel err", rel(out, ref), 5e-6)


@pytest.mark.parametrize("mode", MODES)
def test_edge_embed_golden(net_rough, mode):
    g = golden("embedding.npz")
    with use_arith(net_rough, mode):
        node, edge = net_rough.embedder(residue_idx=T(g["residue_idx"]), t=T(g["t"]), fixed_mask=T(g["fixed_mask"]).to(DEV),
                                        self_conditioning_ca=T(g["sc_ca"]).to(DEV))
        # with the first IPA block's projection fused into the producer (what the network does)
        ipa0 = net_rough.translator.trunk["ipa_0"]
        _, edge2, (bias, pz) = net_rough.embedder(residue_idx=T(g["residue_idx"]), t=T(g["t"]), fixed_mask=T(g["fixed_mask"]).to(DEV),
                                                  self_conditioning_ca=T(g["sc_ca"]).to(DEV), next_proj=ipa0.pair_proj_weights())
    assert torch.equal(edge, edge2)
    assert rel(bias, ipa0.linear_b(edge).permute(0, 3, 1, 2)) < 2e-5 and rel(pz, ipa0.down_z(edge)) < 2e-5
    check(f"{_test_name()}: rel err", rel(node, g["node"]), 5e-6)
    d = np.abs(edge.cpu().numpy() - g["edge"]).max(-1)
    # a pair whose CA distance sits within 1 ulp of a distogram edge may legitimately land in the
    # neighbouring bin (SURVEY.md §7 "discontinuities"): allow none here except the constructed edge pair
    bad = np.argwhere(d > 5e-5)
    assert len(bad) <= 2, (len(bad), bad[:8], d.max())


def test_edge_embed_launch_split(net_rough, monkeypatch):
    """The split-precision edge embedding keeps pair indices 32-bit inside a launch and splits the samples over launches beyond
    2^31 pairs; S2S_EE_MAX_PAIRS lowers that budget so the split (pointer offsets of every per-sample array) is exercised here:
    5 samples, one launch vs launches of 2 + 2 + 1 samples, bit-identical outputs incl. the fused projection."""
    g = torch.Generator().manual_seed(3)
    B, N = 5, 24
    idx = torch.arange(N)[None].repeat(B, 1)
    t = torch.rand(B, generator=g)
    fixed = (torch.rand(B, N, generator=g) > 0.7).float().to(DEV)
    ca = (torch.randn(B, N, 3, generator=g) * 8).to(DEV)
    mask = (torch.rand(B, N, generator=g) > 0.1).float().to(DEV)
    proj = net_rough.translator.trunk["ipa_0"].pair_proj_weights()
    outs = []
    for cap in (None, 2 * N * N + 7):
        if cap is None:
            monkeypatch.delenv("S2S_EE_MAX_PAIRS", raising=False)
        else:
            monkeypatch.setenv("S2S_EE_MAX_PAIRS", str(cap))
        _, edge, (bias, pz) = net_rough.embedder(residue_idx=idx, t=t, fixed_mask=fixed, self_conditioning_ca=ca, node_mask=mask,
                                                 next_proj=proj)
        outs.append((edge.clone(), bias.clone(), pz.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,N", [(2, 32), (3, 7), (1, 75), (5, 24), (20, 6)])
def test_pair_kernels_tiled_layout_is_bit_identical(net_rough, B, N, monkeypatch):
    """Between themselves the f16x3 pair kernels pass the pair tensor in their TILED layout (32-pair blocks in wavefront order: whole
    cache lines per load / store instruction; include/str2str_hip.h "Pair-tensor layouts").  Same numbers, other addresses: embedding
    -> tiled == row-major embedding; EdgeTransition tiled in / tiled out / no output == the row-major call, incl. the fused projections;
    partial last blocks (B N N not a multiple of 32) and launch splits (5 x 24 x 24 pairs in launches of 2 samples; 20 x 6 x 6 with a
    budget of 10 samples, which the launcher lowers to 8 = whole blocks)."""
    from str2str_amd import ops

    g = torch.Generator().manual_seed(11 + N)
    idx = torch.arange(N)[None].repeat(B, 1)
    t = torch.rand(B, generator=g)
    fixed = (torch.rand(B, N, generator=g) > 0.7).float().to(DEV)
    ca = (torch.randn(B, N, 3, generator=g) * 8).to(DEV)
    mask = (torch.rand(B, N, generator=g) > 0.1).float().to(DEV)
    tr = net_rough.translator.trunk
    if B >= 5:
        monkeypatch.setenv("S2S_EE_MAX_PAIRS", str(B // 2 * N * N + 7))
        monkeypatch.setenv("S2S_ET_MAX_PAIRS", str(B // 2 * N * N + 7))
    with use_arith(net_rough, "f16x3"):
        kw = dict(residue_idx=idx, t=t, fixed_mask=fixed, self_conditioning_ca=ca, node_mask=mask, next_proj=tr["ipa_0"].pair_proj_weights())
        node, z_row, (b_row, pz_row) = net_rough.embedder(**kw)
        _, z_til, (b_til, pz_til) = net_rough.embedder(**kw, edge_layout="tiled")
        assert isinstance(z_til, ops.PairTiled) and torch.equal(ops.pair_untiled(z_til), z_row)
        assert torch.equal(b_row, b_til) and torch.equal(pz_row, pz_til)
        assert torch.equal(ops.pair_untiled(ops.pair_tiled(z_row)), z_row)
        et = tr["edge_transition_0"]
        n_p, node_ab = et.node_parts(ops.to_act(node.reshape(B * N, -1).contiguous(), "f16x3"), B * N)
        args = (node_ab.view(B, N, -1), n_p.view(B, N, -1), mask, tr["ipa_1"].pair_proj_weights())
        o_row, ob_row, opz_row = et.pair_mlp(z_row, *args)
        o_til, ob_til, opz_til = et.pair_mlp(z_til, *args, out_layout="tiled")
        assert torch.equal(ops.pair_untiled(o_til), o_row) and torch.equal(ob_til, ob_row) and torch.equal(opz_til, opz_row)
        o_mix, _, _ = et.pair_mlp(z_til, *args)                          # tiled in, row-major out
        assert torch.equal(o_mix, o_row)
        o_none, ob_none, opz_none = et.pair_mlp(z_row, *args, out_layout="none")
        assert o_none is None and torch.equal(ob_none, ob_row) and torch.equal(opz_none, opz_row)
        plain = et.pair_mlp(ops.pair_tiled(z_row), args[0], args[1], mask, None, out_layout="tiled")   # without the fused projection
        assert torch.equal(ops.pair_untiled(plain), et.pair_mlp(z_row, args[0], args[1], mask, None))
        with pytest.raises(ops.HipLibraryError):
            et.pair_mlp(z_row, args[0], args[1], mask, None, out_layout="none")
    with use_arith(net_rough, "f32"), pytest.raises(ops.HipLibraryError):
        et.pair_mlp(z_til, *args)


def test_pair_project_vs_linear(net_rough):
    from str2str_amd import ops

    ipa = net_rough.translator.trunk["ipa_1"]
    g = torch.Generator().manual_seed(7)
    z = torch.randn(2, 19, 19, 128, generator=g).to(DEV)
    d = ipa._derived()
    b, pz = ops.pair_project(z, d["wp"], d["b64"])
    # the attention bias is written head-major [B,H,N,N] (the layout s2s_ipa_attention streams per head)
    assert b.shape == (2, 8, 19, 19)
    assert rel(b, ipa.linear_b(z).permute(0, 3, 1, 2)) < 1e-5 and rel(pz, ipa.down_z(z)) < 1e-5


def test_ipa_golden(net_rough):
    from str2str_amd.common.rigid_utils import Rigid

    g = golden("ipa.npz")
    ipa = net_rough.translator.trunk["ipa_0"]
    out = ipa(T(g["s"]).to(DEV), T(g["z"]).to(DEV), Rigid.from_tensor_7(T(g["rigids7"]).to(DEV)), T(g["mask"]).to(DEV))
    valid = T(g["mask"]).bool().numpy()
    check(f"{_test_name()}: rel err", rel(out.cpu().numpy()[valid], g["out"][valid]), 5e-6)


def _ipa_case(B, N, seed_off=200):
    g = torch.Generator().manual_seed(seed_off + N)
    s = torch.randn(B, N, 256, generator=g)
    z = torch.randn(B, N, N, 128, generator=g)
    q = torch.randn(B, N, 4, generator=g)
    r7 = torch.cat([q / q.norm(dim=-1, keepdim=True), torch.randn(B, N, 3, generator=g)], -1)
    mask = torch.ones(B, N)
    if N > 8:
        mask[-1, -3:] = 0
    return s, z, r7, mask


# Every length runs the default f16 kernel (csrc/ipa_attention_f16w.hip).  32 / 64 = one / two key tiles (the short-stream paths of
# the two-phase pipeline), 96 = odd tile count (a wave without a tile of its own), 256 / 512 = the BASELINE lengths, (3, 64) =
# three samples in one launch of the short kernel (24 (sample, head) pairs: no persistent workgroup sees a second work item here --
# the largest case, (1, 512), has 32 items on one workgroup per CU; batches with more items than workgroups are
# tests/test_attention_parity.py::test_ipa_more_items_than_workgroups); 7 / 37 / 40 / 73 / 300 = ragged lengths (operands padded per
# sample to whole tiles: a single partial tile, a partial second tile, samples whose rows straddle row tiles of the flat [B N]
# layout, three query blocks + two chunks in s2s_ipa_opair)
@pytest.mark.parametrize("B,N", [(1, 7), (2, 32), (3, 37), (2, 40), (2, 73), (1, 96), (3, 64), (1, 256), (1, 300), (1, 512)])
def test_ipa_vs_oracle(net_rough, B, N):
    from oracle import geometry as OG
    from oracle import net as ON
    from str2str_amd.common.rigid_utils import Rigid

    sd = synth_sd(0, 0.02)
    s, z, r7, mask = _ipa_case(B, N)
    ref = ON.ipa(sd, "translator.trunk.ipa_2", s, z, OG.Frames.from_tensor_7(r7), mask)
    ipa = net_rough.translator.trunk["ipa_2"]
    assert ipa.arith == "f16x3" and ipa.use_f16(N, B * N)
    out = ipa(s.to(DEV), z.to(DEV), Rigid.from_tensor_7(r7.to(DEV)), mask.to(DEV))
    valid = mask.bool().numpy()
    check(f"{_test_name()}: rel err", rel(out.cpu().numpy()[valid], ref.numpy()[valid]), 5e-6)


@pytest.mark.parametrize("B,N", [(2, 40), (1, 300), (3, 64)])
def test_ipa_fp32_kernel_vs_oracle(net_rough, B, N):
    """The exact fp32-operand attention kernel with the fp32 node layers (arith "f32": the range-safe path) against the oracle."""
    from oracle import geometry as OG
    from oracle import net as ON
    from str2str_amd.common.rigid_utils import Rigid

    sd = synth_sd(0, 0.02)
    s, z, r7, mask = _ipa_case(B, N)
    ref = ON.ipa(sd, "translator.trunk.ipa_2", s, z, OG.Frames.from_tensor_7(r7), mask)
    ipa = net_rough.translator.trunk["ipa_2"]
    with use_arith(net_rough, "f32"):
        assert not ipa.use_f16(N, B * N)
        out = ipa(s.to(DEV), z.to(DEV), Rigid.from_tensor_7(r7.to(DEV)), mask.to(DEV))
    valid = mask.bool().numpy()
    check(f"{_test_name()}: rel err", rel(out.cpu().numpy()[valid], ref.numpy()[valid]), 5e-6)


@pytest.mark.parametrize("N", [64, 75, 20], ids=["aligned64", "ragged75", "ragged20"])
def test_ipa_f16_kernel_matches_fp32_operand_kernel(net_rough, N):
    """The two attention kernels side by side on the same inputs (ops level, through the C ABI): s2s_ipa_attention_f16w on operands
    pre-split by the GEMM epilogues / the point kernel (ragged lengths through the per-sample padded row map) vs s2s_ipa_attention
    on the fp32 projections -- o (decoded from the packed planes), o_pt and o_pair columns.  Several work items per persistent
    workgroup chain."""
    from str2str_amd import ops

    ipa = net_rough.translator.trunk["ipa_1"]
    B, H = 3, 8
    M = B * N
    NP = ops.padded_len(N)
    rmap, Mo = ((NP, N), B * NP) if NP != N else (None, M)
    g = torch.Generator().manual_seed(11)
    s = torch.randn(M, 256, generator=g).to(DEV)
    q4 = torch.randn(B, N, 4, generator=g)
    r7 = torch.cat([q4 / q4.norm(dim=-1, keepdim=True), torch.randn(B, N, 3, generator=g)], -1).contiguous().to(DEV)
    bias = torch.randn(B, H, N, N, generator=g).to(DEV)
    pz = torch.randn(B, N, N, 32, generator=g).to(DEV)
    mask = torch.ones(B, N)
    mask[1, -5:] = 0
    mask = mask.to(DEV)
    with torch.no_grad():
        w, d = ipa.node_packs(), ipa._derived()
        s_xp = ops.pack_planes(s)
        lin = lambda x, **kw: ops.node_apply(s_xp, x, M, **kw)  # noqa: E731
        linp = lambda x, **kw: ops.node_apply(s_xp, x, Mo, row_map=rmap, **kw)  # noqa: E731
        _, q_xp = linp(w["q"], want_f32=False, want_xp=True)
        _, k_xp = linp(w["k"], want_f32=False, want_xp=True)
        v_vf = ops.node_linear_vfrag(s_xp, w["v"]["w"], w["v"]["b"], Mo, 256, 2048, 8, row_map=rmap)
        qp, _ = lin(w["qp"])
        kvp, _ = lin(w["kvp"])
        pts = ops.ipa_prep_points_f16(r7, qp, kvp, d["hw"])
        bias_in = bias.clone()
        feats, fxp = ops.ipa_attention_f16(q_xp, k_xp, v_vf, pts, bias_in, pz, mask, r7)
        assert torch.equal(bias_in, bias)   # not in place unless asked
        q, _ = lin(w["q"])
        kv, _ = lin(w["kv"])
        q_pts, k_pts, v_pts = ops.ipa_prep_points(r7, qp.view(B, N, -1), kvp.view(B, N, -1), 8, 8, 12)
        ref = ops.ipa_attention(q.view(B, N, H, -1), kv.view(B, N, H, -1), q_pts, k_pts, v_pts, bias, pz, mask, r7, d["hw"]).view(M, -1)
    got = ops.unpack_planes(fxp, M, 2688)
    got[:, 2048:] = feats.view(M, -1)[:, 2048:]
    valid = mask.reshape(-1).bool()
    assert torch.isfinite(got[valid]).all()
    for name, sl in (("o", slice(0, 2048)), ("o_pt", slice(2048, 2432)), ("o_pair", slice(2432, 2688))):
        check(f"ipa f16w N={N} vs fp32-operand kernel, {name}", rel(got[valid][:, sl], ref[valid][:, sl]), 3.5e-6)


def test_se3_step_golden(diffuser):
    from str2str_amd.common.rigid_utils import Rigid

    g = golden("score_reverse.npz")
    t, mask = T(g["t"]), T(g["mask"])
    x0, xt = T(g["x0"]).to(DEV), T(g["xt"]).to(DEV)
    sc = diffuser.score(Rigid.from_tensor_7(x0), Rigid.from_tensor_7(xt), t, mask.to(DEV))
    assert sc["rot_score"].dtype == torch.float64
    assert rel(sc["trans_score"], g["trans_score"]) < 1e-5
    _assert_rot_score_close(sc["rot_score"].cpu().numpy(), g["rot_score"], _anchors("sr"), "score_reverse")
    # reverse from the reference's own scores (probability-flow ODE)
    nxt = diffuser.reverse(Rigid.from_tensor_7(xt), T(g["rot_score"]).to(DEV), T(g["trans_score"]).to(DEV), t, float(g["dt"]),
                           mask.to(DEV), True, 1.0, True)
    assert maxdiff(nxt.to_tensor_7().cpu(), g["next7"]) < 5e-6
    # SDE branch: same host generator state as the fixture -> same noise
    torch.manual_seed(99)
    nxt = diffuser.reverse(Rigid.from_tensor_7(xt), T(g["rot_score"]).to(DEV), T(g["trans_score"]).to(DEV), t, float(g["dt"]),
                           mask.to(DEV), True, 1.0, False)
    assert maxdiff(nxt.to_tensor_7().cpu(), g["next7_sde"]) < 5e-6


def test_so3_score_grid(diffuser):
    from str2str_amd import ops

    g = golden("so3_score.npz")
    t = T(g["t"])
    vec = T(g["vec"])
    B, N = vec.shape[:2]
    # build x0 = identity frames, xt = rotation exp(vec): log(R0^T Rt) = vec
    from str2str_amd.common import rotation3d

    qt = rotation3d.axis_angle_to_quaternion(vec)
    qt = rotation3d.matrix_to_quaternion(rotation3d.quaternion_to_matrix(qt))
    xt = torch.cat([qt, torch.zeros(B, N, 3)], -1).to(DEV).contiguous()
    x0 = torch.zeros(B, N, 7)
    x0[..., 0] = 1
    p8 = diffuser.step_params(t).to(DEV)
    ones = torch.ones(B, N, device=DEV)
    _, rs, _ = ops.se3_step(x0.to(DEV), xt, ones, ones, p8, dt=0.0, want_next=False, want_scores=True)
    # without sign standardisation the reference chain wraps some rotations to angle 2*pi - theta;
    # compare on the unambiguous range
    ang = vec.norm(dim=-1).numpy()
    ok = ang < 1.5  # w > |xyz|: candidate 0 of matrix_to_quaternion, no 2*pi wrap
    good = _assert_rot_score_close(rs.cpu().numpy()[ok], g["score"][ok], _anchors("grid", sel=ok), "omega grid")
    assert good.sum() > 20


def _batch(g, dev):
    out = {}
    for k, v in g.items():
        if k.startswith("in_"):
            t = T(v)
            out[k[3:]] = t if k[3:] in ("t", "residue_idx") else t.to(dev)
    return out


def test_denoising_net_golden(net_rough):
    # b1n256 / b1n512: one reference evaluation at the BASELINE configs[1] / configs[3] lengths
    for tag in ("b1n10", "b2n16", "b1n256", "b1n512"):
        g = golden(f"net_{tag}.npz")
        out = net_rough(_batch(g, DEV))
        check(f"net golden {tag}: max |frames - reference|", maxdiff(out["rigids"].to_tensor_7().cpu(), g["rigids7"]), 1e-4)
        check(f"net golden {tag}: max |psi - reference|", maxdiff(out["psi"].cpu(), g["psi"]), 3e-5)
        check(f"net golden {tag}: max |backbone atoms - reference| (A)", maxdiff(out["atom37"].cpu()[..., :5, :], g["atom37"]), 1.2e-4)
        assert float(out["atom37"][..., 5:, :].abs().max()) == 0


def test_network_is_independent_of_the_pair_layout(net_rough, monkeypatch):
    """The network chains its f16x3 pair kernels in their tiled layout and lets the last EdgeTransition write no pair tensor; with the
    embedding handed over row-major instead (its EdgeTransition then reads row-major and writes tiled) and with the tiled layout
    switched off altogether (every pair tensor row-major, every EdgeTransition writing its output) the frames are bit-identical."""
    g = golden("net_b2n16.npz")
    batch = _batch(g, DEV)
    ref = net_rough(batch)["rigids"].to_tensor_7().clone()
    emb_fwd = type(net_rough.embedder).forward
    monkeypatch.setattr(type(net_rough.embedder), "forward", lambda self, *a, edge_layout="rowmajor", **k: emb_fwd(self, *a, **k))
    mixed = net_rough(batch)["rigids"].to_tensor_7().clone()          # embedding row-major, trunk tiled
    assert torch.equal(mixed, ref)
    et_cls = type(net_rough.translator.trunk["edge_transition_0"])
    pair_mlp = et_cls.pair_mlp
    monkeypatch.setattr(et_cls, "pair_mlp", lambda self, *a, out_layout="rowmajor", **k: pair_mlp(self, *a, **k))
    plain = net_rough(batch)["rigids"].to_tensor_7()                  # nothing tiled, nothing skipped
    assert torch.equal(plain, ref)


def test_teacher_forced_trajectory(net_rough, diffuser):
    """All 20 steps of a reference trajectory, each re-done from the reference's own step inputs."""
    from str2str_amd.synth import synth_chain

    g = golden("traj_teacher_n16.npz")
    B = int(g["B"])
    feats = synth_chain(int(g["n_res"]))
    f = {k: v.repeat(B, *(1,) * (v.ndim - 1)).to(DEV) for k, v in feats.items()
         if k in ("aatype", "residue_mask", "fixed_mask", "torsion_angles_sin_cos")}
    f["residue_idx"] = feats["residue_idx"].repeat(B, 1)
    dt = float(g["dt"])
    mask = f["residue_mask"].float().contiguous()
    worst_x0 = worst_next = 0.0
    n_good = n_total = 0
    for i, t in enumerate(g["ts"]):
        f["t"] = torch.full((B,), float(t), dtype=torch.float32)
        f["rigids_t"] = T(g["rigids_t"][i]).to(DEV)
        f["sc_ca_t"] = T(g["sc_ca_t"][i]).to(DEV)
        out = net_rough(f)
        worst_x0 = max(worst_x0, maxdiff(out["rigids7"].cpu(), g["x0"][i]))
        if i < len(g["ts"]) - 1:
            p8 = diffuser.step_params(f["t"]).to(DEV)
            nxt, rs, tsc = diffuser.step(T(g["x0"][i]).to(DEV), f["rigids_t"].contiguous(), p8, dt, mask, mask,
                                         want_scores=True)
            good = _assert_rot_score_close(rs.cpu().numpy(), g["rot_score"][i], _anchors("tf", idx=i), f"teacher-forced step {i}")
            assert rel(tsc, g["trans_score"][i]) < 1e-5
            # frames of residues whose rotation score is well conditioned in the reference's own float32
            n_good += int(good.sum())
            n_total += int(good.size)
            if good.any():
                worst_next = max(worst_next, maxdiff(nxt.cpu()[T(good)], g["next7"][i][good]))
            # translations do not depend on the rotation score at all
            assert maxdiff(nxt.cpu()[..., 4:], g["next7"][i][..., 4:]) < 2e-5
    check("teacher-forced: worst |x0 - reference| over 20 steps", worst_x0, 1.2e-4)
    # how much of the trajectory the next-frame check covers (the rest: residues where the bound above proves the reference's own
    # float32 rotation score is rounding noise; their TRANSLATIONS are still checked, two lines up)
    record_margin(f"teacher-forced: well-conditioned residue-steps checked for next frames: {n_good} of {n_total} (fraction NOT checked)",
                  1.0 - n_good / max(n_total, 1), 1.0)
    assert n_good > 100, n_good
    check("teacher-forced: worst |next frames - reference| on well-conditioned residues", worst_next, 4e-6)


@pytest.mark.parametrize("mode", MODES)
def test_free_running_trajectory_rmsd_both_arithmetics(net_smooth, diffuser, mode):
    """The 1e-4 Angstrom criterion holds in either arithmetic of the whole network (split-f16 default, exact fp32 MFMA)."""
    from str2str_amd.common.rigid_utils import Rigid
    from str2str_amd.sampler import forward_backward
    from str2str_amd.synth import synth_chain

    g = golden("traj_free_cfg1_n64_s20.npz")
    N, B = int(g["n_res"]), int(g["B"])
    feats = synth_chain(N)
    rig0 = Rigid.from_tensor_4x4(feats["rigidgroups_gt_frames"][..., 0, :, :].repeat(B, 1, 1, 1))
    with use_arith(net_smooth, mode):
        torch.manual_seed(int(g["seed"]))
        a37 = forward_backward(net_smooth, diffuser, feats, rig0, float(g["t_delta"]),
                               num_timesteps=int(g["num_timesteps"]), device=DEV)
    rmsd = backbone_rmsd(a37.cpu().numpy()[..., :5, :], g["atom37"])
    check(f"free-running cfg1_n64_s20 in arith {mode}: backbone RMSD vs reference (A)", rmsd, 1e-4)




@pytest.mark.parametrize("mode", MODES)
def test_pair_kernels_many_tiles_per_workgroup(net_rough, mode, monkeypatch):
    """More 128-pair tiles than CUs (B*N*N/128 = 1024): every persistent workgroup of the pair kernels walks several
    tiles, with and without the fused projection (odd / even number of weight stages).  Checked against a float64
    evaluation of the reference formulas (layers.py:170-185, ipa.py:177,253)."""
    et, ipa1 = net_rough.translator.trunk["edge_transition_0"], net_rough.translator.trunk["ipa_1"]
    B, N = 2, 256
    gen = torch.Generator().manual_seed(21)
    node = torch.randn(B, N, 256, generator=gen).to(DEV)
    edge = torch.randn(B, N, N, 128, generator=gen).to(DEV)
    n = et.initial_embed(node).double()
    x = torch.cat([edge.double(), n[:, :, None, :].expand(B, N, N, -1), n[:, None, :, :].expand(B, N, N, -1)], -1)
    hcur = x
    for lyr in et.trunk:
        hcur = F.linear(hcur, lyr.weight.double(), lyr.bias.double()) if isinstance(lyr, torch.nn.Linear) else F.relu(hcur)
    ref = F.layer_norm(F.linear(hcur + x, et.final_layer.weight.double(), et.final_layer.bias.double()), (128,),
                       et.layer_norm.weight.double(), et.layer_norm.bias.double(), et.layer_norm.eps)
    del x, hcur
    with use_arith(net_rough, mode):
        plain = et(node, edge)
        out, bias, pz = et(node, edge, next_proj=ipa1.pair_proj_weights())
        if mode == "f16x3":   # the launch split beyond 2^29 pairs, exercised through the per-launch pair budget hook: bit-identical
            monkeypatch.setenv("S2S_ET_MAX_PAIRS", str(N * N + 5))
            out2, bias2, pz2 = et(node, edge, next_proj=ipa1.pair_proj_weights())
            monkeypatch.delenv("S2S_ET_MAX_PAIRS")
            assert torch.equal(out2, out) and torch.equal(bias2, bias) and torch.equal(pz2, pz)
    check(f"edge transition {mode}, 1024 tiles: max |out - float64|", float(max((plain.double() - ref).abs().max(), (out.double() - ref).abs().max())), 1.5e-5)
    assert rel(bias, ipa1.linear_b(out).permute(0, 3, 1, 2)) < 5e-6 and rel(pz, ipa1.down_z(out)) < 5e-6
    # edge embedding over many tiles: each arithmetic against the float64 statement of the reference formula (tests/ref_embed.py),
    # on CA clear of the distogram's bin edges (every correct float32 distance picks the same bin): no differing pair is allowed
    import embed_cases
    import ref_embed

    emb = net_rough.embedder
    ridx = torch.arange(N)[None].repeat(B, 1)
    ca, _ = embed_cases.clear_of_bin_edges(torch.randn(B, N, 3, generator=gen) * 8, gen)
    t, fixed = torch.full((B,), 0.4), torch.zeros(B, N)
    sd = synth_sd(0, 0.02)
    with use_arith(net_rough, mode):
        node_e, edge_e, (bias_e, pz_e) = emb(residue_idx=ridx, t=t, fixed_mask=fixed.to(DEV), self_conditioning_ca=ca.to(DEV),
                                            next_proj=net_rough.translator.trunk["ipa_0"].pair_proj_weights())
    node64, edge64 = ref_embed.embedding64(sd, ridx, t, fixed, ca, device=DEV)
    bias64, pz64 = ref_embed.pair_projection64(sd, embed_cases.IPA0, edge64)
    for what, got, want in (("node", node_e, node64), ("edge", edge_e, edge64), ("attn_bias", bias_e, bias64), ("pair_z", pz_e, pz64)):
        check(f"edge embedding {mode}, 1024 tiles: max |{what} - float64|", float((got.double() - want).abs().max()), embed_cases.bound(sd, what, mode))


def test_torch_ops_registration(net_rough):
    """The kernels are also reachable as torch.ops.str2str_amd.* (SURVEY 8b): same results as the ops module."""
    from str2str_amd import ops

    ops.register_torch_ops()
    g = golden("prims.npz")
    r7 = torch.cat([T(g["q"]), T(g["t"])], -1).to(DEV).contiguous()
    upd, msk = T(g["upd"]).to(DEV).contiguous(), T(g["msk"])[:, 0].to(DEV).contiguous()
    a = torch.ops.str2str_amd.rigid_compose_update(r7, upd, msk)
    assert torch.equal(a, ops.rigid_compose_update(r7, upd, msk))
    et = _edge_transition_module(net_rough)
    pk = et._packed()
    gen = torch.Generator().manual_seed(3)
    node, edge = torch.randn(1, 9, 256, generator=gen).to(DEV), torch.randn(1, 9, 9, 128, generator=gen).to(DEV)
    n_p, node_ab = et.node_parts(ops.pack_planes(node.reshape(9, 256)), 9)
    o = torch.ops.str2str_amd.edge_transition_f16x3(edge, node_ab.view(1, 9, -1), n_p.view(1, 9, -1), pk["wstream_f16"], et.trunk[2].bias,
                                                    et.layer_norm.weight, et.layer_norm.bias, None, et.layer_norm.eps)
    assert torch.equal(o, et(node, edge))


def test_every_torch_op_equals_its_ops_function(net_rough, diffuser):
    """every tensor entry point of include/str2str_hip.h is a ``torch.ops.str2str_amd.*`` operator, and the modules call
    their kernels through them.  One call per registered op against the ``ops`` function behind it, bit for bit; and the op table is
    complete: every ``s2s_*`` export that takes device tensors is reachable from an op."""
    from str2str_amd import ops

    K = torch.ops.str2str_amd
    names = {sch.split("(")[0] for sch in ops.torch_ops._TORCH_OPS}
    assert names >= {"edge_transition", "edge_transition_f16x3", "edge_transition_f16x3_chain", "edge_embed", "edge_embed_f16x3", "pair_project",
                     "ipa_prep_points", "ipa_attention", "ipa_prep_points_f16", "ipa_prep_points_shared_kv", "ipa_attention_f16w", "encoder_attention", "node_linear",
                     "node_linear_f32", "node_linear_vfrag", "ipa_projections", "node_linear_multi", "node_chain", "row_layernorm", "embed_assemble", "pack_planes", "se3_step", "forward_marginal", "rigid_compose_update",
                     "rigid_scale_trans", "torsion_head", "frames_to_backbone"}
    gen = torch.Generator().manual_seed(11)
    rn = lambda *sh: torch.randn(*sh, generator=gen).to(DEV)
    eq = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b)) if isinstance(a, (tuple, list)) else torch.equal(a, b)
    B, N, M = 2, 48, 96      # (M a multiple of 32: a packed-planes buffer has no rows beyond M whose bytes nobody writes)
    tr = net_rough.translator.trunk
    ipa, et = tr["ipa_0"], tr["edge_transition_0"]
    w, d = ipa.node_packs(), ipa._derived()
    # ---- node stream
    x = rn(M, 256)
    xp = K.pack_planes(x)
    assert torch.equal(xp, ops.pack_planes(x))
    lay = w["q"]
    a = K.node_linear(xp, lay["w"], lay["b"], M, lay["k"], lay["n"], lay["tg"], None, True, None, None, None, None, 0.0, None, None, 0, True,
                      None, -1, 0, True)
    b = ops.node_linear(xp, lay["w"], lay["b"], M, lay["k"], lay["n"], lay["tg"], relu=True, want_xp=True)
    assert eq(a, b)
    a = K.node_linear_f32(x, lay["w32"], lay["b"], M, lay["k"], lay["n"], lay["tg"], None, True)
    assert torch.equal(a, ops.node_linear_f32(x, lay["w32"], lay["b"], M, lay["k"], lay["n"], lay["tg"], relu=True))
    NP = ops.padded_len(N)
    a = K.node_linear_vfrag(xp, w["v"]["w"], w["v"]["b"], B * NP, w["v"]["k"], w["v"]["n"], 8, NP, N)
    v_vf = ops.node_linear_vfrag(xp, w["v"]["w"], w["v"]["b"], B * NP, w["v"]["k"], w["v"]["n"], 8, row_map=(NP, N))
    assert torch.equal(a, v_vf)
    # the five projections of an IPA block in one launch == the five launches
    names = ("q", "k", "v", "qp", "kvp")
    dims = [x_ for n_ in names for x_ in (w[n_]["k"], w[n_]["n"], w[n_]["tg"])]
    five = K.ipa_projections(xp, *[[w[n_]["w"], w[n_]["b"]] for n_ in names], dims, M, B * NP, NP, N)
    assert torch.equal(five[0], ops.node_apply(xp, w["q"], B * NP, row_map=(NP, N), want_f32=False, want_xp=True)[1])
    assert torch.equal(five[1], ops.node_apply(xp, w["k"], B * NP, row_map=(NP, N), want_f32=False, want_xp=True)[1])
    assert torch.equal(five[2], v_vf)
    assert torch.equal(five[3], ops.node_apply(xp, w["qp"], M)[0]) and torch.equal(five[4], ops.node_apply(xp, w["kvp"], M)[0])
    # ... and with the folded projections (k / v absent): three problems in the launch
    fdims = [x_ for n_ in ("qf", None, None, "qp", "kvp") for x_ in ((w[n_]["k"], w[n_]["n"], w[n_]["tg"]) if n_ else (0, 0, 0))]
    three = K.ipa_projections(xp, [w["qf"]["w"], w["qf"]["b"]], [], [], [w["qp"]["w"], w["qp"]["b"]], [w["kvp"]["w"], w["kvp"]["b"]], fdims,
                              M, B * NP, NP, N)
    assert three[1] is None and three[2] is None and torch.equal(three[3], five[3]) and torch.equal(three[4], five[4])
    assert torch.equal(three[0], ops.node_apply(xp, w["qf"], B * NP, row_map=(NP, N), want_f32=False, want_xp=True)[1])
    r7s = torch.cat([torch.nn.functional.normalize(rn(B, N, 4), dim=-1), rn(B, N, 3)], -1).contiguous()
    sh_op = K.ipa_prep_points_shared_kv(r7s, five[3], five[4], d["hw"], xp)
    sh_fn = ops.ipa_prep_points_f16(r7s, five[3], five[4], d["hw"], s_xp=xp)
    assert len(sh_op) == 7 and all((a_ is None and b_ is None) or torch.equal(a_, b_) for a_, b_ in zip(sh_op, sh_fn))
    # layers of one input in one launch (the trunk: four skip_embeds; BackboneUpdate + the EdgeTransition's per-node parts) == the launches
    nl, tw = et.node_layers(), net_rough.translator._node_weights()
    dmk = torch.rand(M, generator=gen).to(DEV)
    xf, xa = torch.zeros(M, 320, device=DEV), torch.zeros_like(ops.xp_alloc(M, 320, DEV))
    specs = [(tw[0]["bb"], dict(pre_scale=dmk)), (nl["init"], {}), (nl["ab_s"], {}),
             (tw["tor"]["l1"], dict(relu=True, want_f32=False, want_xp=True)),
             (tw[0]["skip"], dict(out_f32=xf, out_col0=256, out_xp=xa, out_xp_k=320, out_xp_k0=256))]
    multi = ops.node_apply_multi(xp, specs, M)
    xf1, xa1 = torch.zeros(M, 320, device=DEV), torch.zeros_like(xa)
    specs[4][1].update(out_f32=xf1, out_xp=xa1)
    for (layer, kw), got in zip(specs, multi):
        want = ops.node_apply(xp, layer, M, **kw)
        assert all((a_ is None and b_ is None) or torch.equal(a_, b_) for a_, b_ in zip(got, want))
    assert torch.equal(xf, xf1) and torch.equal(xa, xa1)
    # the folded per-node part of the edge transition (W_ab (W_ie s + b_ie) + b_ab as one layer from s) against the two-layer form
    n_p2, ab2 = et.node_parts(xp, M)
    assert torch.equal(multi[1][0], n_p2) and rel(multi[2][0], ab2) < 2e-6
    # a chain of square layers in one launch (hidden activations in registers) == the launches, bit for bit: NodeTransition (3 x 256,
    # residual + LayerNorm + mask), an encoder layer's feed-forward (2 x 320, residual + LayerNorm); several workgroups + a ragged last tile
    for Mc in (M, 5 * 128 + 40):
        xc, resc, pmc = ops.pack_planes(rn(Mc, 256)), rn(Mc, 256), (torch.rand(Mc, generator=gen) > 0.2).float().to(DEV)
        ntm = tr["node_transition_0"]
        lyr = [tw[0]["nt1"], tw[0]["nt2"], tw[0]["nt3"]]
        kwc = dict(residual=resc, ln=(ntm.ln.weight, ntm.ln.bias, ntm.ln.eps), post_mask=pmc, want_xp=True)
        _, h1_ = ops.node_apply(xc, lyr[0], Mc, relu=True, want_f32=False, want_xp=True)
        _, h2_ = ops.node_apply(h1_, lyr[1], Mc, relu=True, want_f32=False, want_xp=True)
        want = ops.node_apply(h2_, lyr[2], Mc, **kwc)
        got = ops.node_apply_chain(xc, lyr, Mc, (True, True, False), **kwc)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), Mc
        # ... and with trunk.linear (320 -> 256, + residual, fp32 result stored and read back as the last layer's residual) in front
        x4, res4 = ops.pack_planes(rn(Mc, 320)), rn(Mc, 320)
        n_want, n_a_ = ops.node_apply(x4, tw[0]["lin"], Mc, residual=res4, want_xp=True)
        _, h1_ = ops.node_apply(n_a_, lyr[0], Mc, relu=True, want_f32=False, want_xp=True)
        _, h2_ = ops.node_apply(h1_, lyr[1], Mc, relu=True, want_f32=False, want_xp=True)
        kw4 = dict(ln=(ntm.ln.weight, ntm.ln.bias, ntm.ln.eps), post_mask=pmc, want_xp=True)
        want = ops.node_apply(h2_, lyr[2], Mc, residual=n_want, **kw4)
        n_got = torch.full((Mc, 256), float("nan"), device=DEV)
        got = ops.node_apply_chain(x4, [tw[0]["lin"]] + lyr, Mc, (False, True, True, False), first_residual=res4, first_out_f32=n_got,
                                   residual=n_got, **kw4)
        assert torch.equal(n_got, n_want) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), Mc
        enc = tr["transformer_0"].layers[0]
        lw0 = tw[0]["layers"][0]
        xe, rese = ops.pack_planes(rn(Mc, 320)), rn(Mc, 320)
        kwe = dict(residual=rese, ln=(enc.norm2.weight, enc.norm2.bias, enc.norm2.eps), want_xp=True)
        _, ha_ = ops.node_apply(xe, lw0["l1"], Mc, relu=True, want_f32=False, want_xp=True)
        want = ops.node_apply(ha_, lw0["l2"], Mc, **kwe)
        got = ops.node_apply_chain(xe, [lw0["l1"], lw0["l2"]], Mc, (True, False), **kwe)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), Mc
        # ... and the layer's whole post-attention half: out_proj + residual + norm1 (stored: norm2's residual), linear1, relu, linear2 +
        # residual + norm2 (reference ipa.py:312-317) as ONE launch -- the kernel itself (s2s_node_chain with the first layer's LayerNorm;
        # node_apply_chain would pick the separate launches at this row count) and through node_apply_chain
        ln1 = (enc.norm1.weight, enc.norm1.bias, enc.norm1.eps)
        x1_want, x1a_ = ops.node_apply(xe, lw0["o"], Mc, residual=rese, ln=ln1, want_xp=True)
        _, ha_ = ops.node_apply(x1a_, lw0["l1"], Mc, relu=True, want_f32=False, want_xp=True)
        want = ops.node_apply(ha_, lw0["l2"], Mc, residual=x1_want, ln=kwe["ln"], want_xp=True)
        lyr3 = [lw0["o"], lw0["l1"], lw0["l2"]]
        x1_got = torch.full((Mc, 320), float("nan"), device=DEV)
        got = ops.node_chain(xe, [L_["w_row"] for L_ in lyr3], [L_["b"] for L_ in lyr3], [False, True, False], Mc, 320, residual=x1_got,
                             ln_gamma=enc.norm2.weight, ln_beta=enc.norm2.bias, ln_eps=enc.norm2.eps, want_xp=True, mid_residual=rese,
                             mid_out_f32=x1_got, mid_ln=ln1)
        assert torch.equal(x1_got, x1_want) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), Mc
        x1_got2 = torch.full((Mc, 320), float("nan"), device=DEV)
        got = ops.node_apply_chain(xe, lyr3, Mc, (False, True, False), first_residual=rese, first_out_f32=x1_got2, first_ln=ln1,
                                   residual=x1_got2, ln=kwe["ln"], want_xp=True)
        assert torch.equal(x1_got2, x1_want) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), Mc
    # the embedder's per-evaluation assembly: one launch == the elementwise expressions it replaced, bit for bit (fp32 adds, relu, split)
    Le = 40
    timg, ncst, fa_ = rn(512), rn(B * Le, 256), rn(B, Le, 128)
    fb_cb, fb_rm = rn(B, 32, Le, 4), rn(B, Le, 128)
    h_want = torch.relu(timg[:256] + ncst)
    for planes in (True, False):
        for cb in (True, False):
            got = K.embed_assemble(timg, ncst, fa_, fb_cb if cb else fb_rm, B, Le, planes, cb)
            assert eq(got, ops.embed_assemble(timg, ncst, fa_, fb_cb if cb else fb_rm, B, Le, planes, cb))
            assert torch.equal(got[0], ops.pack_planes(h_want) if planes else h_want)
            assert torch.equal(got[1], timg[256:384] + fa_)
            assert torch.equal(got[2], (timg[384:].view(32, 1, 4) + fb_cb) if cb else (timg[384:] + fb_rm))
    got = K.embed_assemble(timg, ncst[:Le].contiguous(), fa_, fb_cb, B, Le, True, True)          # node constants shared by the samples
    assert torch.equal(got[0], ops.pack_planes(torch.relu(timg[:256] + ncst[:Le]).repeat(B, 1)))
    # linear_out (K = 2688) on few rows runs as a narrow-block GEMM + the LayerNorm on its own (s2s_row_layernorm): bitwise the fused layer
    lo, lnm = w["out"], tr["ipa_ln_0"]
    fx = ops.pack_planes(rn(M, 2688))
    res, pmk = rn(M, 256), (torch.rand(M, generator=gen) > 0.2).float().to(DEV)
    fused = ops.node_linear(fx, lo["w"], lo["b"], M, lo["k"], lo["n"], lo["tg"], pre_mask=pmk, residual=res,
                            ln=(lnm.weight, lnm.bias, lnm.eps), post_mask=pmk, want_xp=True)
    split = ops.node_apply(fx, lo, M, pre_mask=pmk, residual=res, ln=(lnm.weight, lnm.bias, lnm.eps), post_mask=pmk, want_xp=True)
    assert "w_n" in lo and eq(fused, split)
    pre = rn(M, 320)
    l2n = tr["transformer_0"].layers[0].norm2
    a = K.row_layernorm(pre, M, 320, l2n.weight, l2n.bias, l2n.eps, None, None, 0, True, None, -1, 0, True)
    assert eq(a, ops.row_layernorm(pre, M, 320, l2n.weight, l2n.bias, l2n.eps, want_xp=True))
    ref = torch.nn.functional.layer_norm(pre.double(), (320,), l2n.weight.double(), l2n.bias.double(), l2n.eps)
    assert (a[0].double() - ref).abs().max() < 1e-5
    qkv = rn(M, 960)
    for ar in MODES:
        assert eq([t for t in K.encoder_attention(qkv, None, B, N, 4, True, True, ar)], [t for t in ops.encoder_attention(qkv, None, B, N, 4, True, True, ar)])
    # ---- attention
    r7 = torch.cat([torch.nn.functional.normalize(rn(B, N, 4), dim=-1), rn(B, N, 3)], -1).contiguous()
    qp_lin, kvp_lin = ops.node_apply(xp, w["qp"], M)[0], ops.node_apply(xp, w["kvp"], M)[0]
    pts = K.ipa_prep_points_f16(r7, qp_lin, kvp_lin, d["hw"])
    assert eq(pts, ops.ipa_prep_points_f16(r7, qp_lin, kvp_lin, d["hw"]))
    p32 = K.ipa_prep_points(r7, qp_lin.view(B, N, -1), kvp_lin.view(B, N, -1))
    assert eq(p32, ops.ipa_prep_points(r7, qp_lin.view(B, N, -1), kvp_lin.view(B, N, -1)))
    z = rn(B, N, N, 128)
    bias, pz = K.pair_project(z, d["wp"], d["b64"])
    assert eq((bias, pz), ops.pair_project(z, d["wp"], d["b64"]))
    mask = torch.ones(B, N, device=DEV)
    q_xp = ops.node_apply(xp, w["q"], B * NP, row_map=(NP, N), want_f32=False, want_xp=True)[1]
    k_xp = ops.node_apply(xp, w["k"], B * NP, row_map=(NP, N), want_f32=False, want_xp=True)[1]
    a = K.ipa_attention_f16w(q_xp, k_xp, v_vf, *pts, bias, pz, mask, r7)
    b = ops.ipa_attention_f16(q_xp, k_xp, v_vf, pts, bias, pz, mask, r7)
    # (each output carries half of linear_out's input: the fp32 tensor the o_pt / o_pair columns, the planes the o columns)
    assert torch.equal(a[0][..., 2048:], b[0][..., 2048:])
    assert torch.equal(ops.unpack_planes(a[1], M, a[0].shape[-1])[:, :2048], ops.unpack_planes(b[1], M, b[0].shape[-1])[:, :2048])
    q32, kv32 = ops.node_apply(x, w["q"], M)[0].view(B, N, 8, -1), ops.node_apply(x, w["kv"], M)[0].view(B, N, 8, -1)
    assert torch.equal(K.ipa_attention(q32, kv32, *p32, bias, pz, mask, r7, d["hw"]), ops.ipa_attention(q32, kv32, *p32, bias, pz, mask, r7, d["hw"]))
    # ---- pair stream
    node = rn(B, N, 256)
    n_p, node_ab = et.node_parts(ops.pack_planes(node.reshape(M, 256)), M)
    n_p, node_ab = n_p.view(B, N, -1), node_ab.view(B, N, -1)
    pk, pk32 = et._packed(), et._packed_f32()
    common = (et.trunk[2].bias, et.final_layer.bias, et.layer_norm.weight, et.layer_norm.bias, mask, et.layer_norm.eps)
    ab32 = node_ab[..., :768].contiguous()    # the exact kernel takes the first layer's two halves; the final layer's bias as an argument
    assert torch.equal(K.edge_transition(z, ab32, n_p, pk32["w1p"], pk32["w2p"], pk32["wfp"], *common),
                       ops.edge_transition(z, ab32, n_p, pk32["w1p"], pk32["w2p"], pk32["wfp"], *common))
    common = common[:1] + common[2:]          # (f16x3: the final layer's bias rides in node_ab's third group)
    nxt = tr["ipa_1"].pair_proj_weights()
    stream = torch.cat([pk["wstream_f16"], nxt["wp_f16x2"]])
    zt = ops.pair_tiled(z)
    a = K.edge_transition_f16x3_chain(zt.buf, True, B, N, node_ab, n_p, stream, *common, nxt["b64"], "tiled")
    b = ops.edge_transition_f16x3(zt, node_ab, n_p, pk["wstream_f16"], *common, proj=(stream, nxt["b64"]), out_layout="tiled")
    assert torch.equal(a[0], b[0].buf) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert torch.equal(et.pair_mlp(zt, node_ab, n_p, mask, nxt, out_layout="tiled")[0].buf, b[0].buf)     # the module goes through the op
    emb = net_rough.embedder
    wts = emb._weights()
    args = dict(residue_idx=torch.arange(N)[None].repeat(B, 1), t=torch.full((B,), 0.4), fixed_mask=torch.zeros(B, N).to(DEV),
                self_conditioning_ca=rn(B, N, 3))
    with use_arith(net_rough, "f32", families=("edge_embed",)):
        e32 = emb(**args)[1]
    rel_tab, span, node_pos, idx_dev = emb._index_tables(args["residue_idx"], wts["w_rel"], wts["wn_pos"])
    assert e32.shape == (B, N, N, 128) and torch.isfinite(e32).all()      # (the fp32 embedding op is exercised through its module; its
    #                                                                        flat form is held to ops.edge_embed by test_edge_embed_golden)
    # ---- frames
    assert torch.equal(K.rigid_scale_trans(r7, 0.1, False), ops.rigid_scale_trans(r7, 0.1))
    u32 = rn(M, 32)
    u32[3, :2] = 0.0                                                  # the clamp: 0 / sqrt(eps)
    th = K.torsion_head(u32, M, True, 1e-8)
    u2 = u32[:, :2]
    assert torch.equal(th, ops.torsion_head(u32, M)) and torch.equal(th, u2 / torch.sqrt(torch.clamp(torch.sum(u2 ** 2, dim=-1, keepdim=True), min=1e-8)))
    gt, fx = rn(B, N, 7, 2)[..., 2, :], (torch.rand(M, generator=gen) > 0.5).float().to(DEV)
    assert torch.equal(K.torsion_head(u32, M, False, 1e-8, gt, fx), gt.reshape(M, 2) * fx[:, None] + u2 * (1 - fx[:, None]))
    upd32 = rn(M, 32)
    assert torch.equal(ops.rigid_compose_update(r7, upd32, mask), ops.rigid_compose_update(r7, upd32[:, :6].contiguous().view(B, N, 6), mask))
    psi = torch.nn.functional.normalize(rn(B, N, 2), dim=-1)
    aat = torch.randint(0, 21, (B, N), generator=gen).to(DEV)
    assert torch.equal(K.frames_to_backbone(r7, psi, aat), ops.frames_to_backbone(r7, psi, aat)[0])
    p8 = diffuser.step_params(torch.full((B,), 0.5)).to(DEV)
    x0 = torch.cat([torch.nn.functional.normalize(rn(B, N, 4), dim=-1), rn(B, N, 3)], -1).contiguous()
    assert torch.equal(K.se3_step(x0, r7, mask, mask, p8, 0.01), ops.se3_step(x0, r7, mask, mask, p8, 0.01)[0])
    fm = diffuser.forward_marginal_device   # the forward-marginal op is what the diffuser's device mode launches
    torch.cuda.manual_seed(3); a = fm(None, None, shape=(B, N))
    torch.cuda.manual_seed(3); b = fm(None, None, shape=(B, N))
    assert torch.equal(a, b) and a.shape == (B, N, 7)


def test_small_node_modules_run_on_the_node_kernel(net_rough):
    """NodeTransition / TorsionAngleHead / BackboneUpdate keep the reference's ``forward`` (layers.py:128-145,188-241) for callers outside
    the sampler; their Linear layers run on the package's node kernel (no library GEMM anywhere in the package), agree with the float64
    evaluation of the same modules, and refuse a CPU tensor instead of silently taking another path."""
    from str2str_amd import ops

    tr = net_rough.translator
    gen = torch.Generator().manual_seed(2)
    s = torch.randn(2, 19, 256, generator=gen).to(DEV)
    nt, bb, tor = tr.trunk["node_transition_0"], tr.trunk["bb_update_0"], tr.torsion_pred

    def f64(mod, x):
        import copy
        import torch.nn as nn
        m = copy.deepcopy(mod).double().cpu()
        for sub in m.modules():      # the float64 twin evaluates its Linear layers as plain nn.Linear
            if isinstance(sub, nn.Linear):
                sub.forward = nn.Linear.forward.__get__(sub)
        return m(x.double().cpu())

    for mod in (nt, bb, tor):
        got, want = mod(s), f64(mod, s)
        assert got.shape == want.shape and (got.double().cpu() - want).abs().max() < 2e-5 * max(1.0, want.abs().max().item())
        with pytest.raises(ops.HipLibraryError):
            mod(s.cpu())


def test_range_guard_flags_every_f16_producer():
    """Every kernel that splits fp32 values into f16 planes reports a value beyond 2^15 into the range flag passed with the call (one bit per
    kernel family, csrc/range_flag.h), and stays quiet on in-range data -- ops level, through the C ABI."""
    from str2str_amd import ops
    from str2str_amd.factory import build_synthetic_net

    net = build_synthetic_net(seed=0, sigma_final=0.02, device=DEV)
    g = torch.Generator().manual_seed(5)
    M, K = 70, 256
    x = torch.randn(M, K, generator=g).to(DEV)
    layer = ops.pack_node_layer((torch.randn(256, K, generator=g) / 16).to(DEV), torch.zeros(256, device=DEV), True)

    def flags(fn):
        ops.range_flag_reset()
        fn()
        return ops.range_flag_read()

    assert flags(lambda: ops.pack_planes(x)) == 0
    big = x.clone(); big[13, 77] = 4.0e4
    assert flags(lambda: ops.pack_planes(big)) == 2
    # magnitude buckets (headroom): nothing is recorded below 2^8; a maximum in [2^(8+e), 2^(9+e)) reports the bucket's upper edge / 2^15
    assert flags(lambda: ops.pack_planes(x)) == 0 and ops.range_headroom()["node"] == 2.0 ** -7
    mid = x.clone(); mid[5, 9] = -1000.0
    assert flags(lambda: ops.pack_planes(mid)) == 0 and ops.range_headroom() == {"node": 2.0 ** -5, "edge_transition": 2.0 ** -7,
                                                                                 "edge_embed": 2.0 ** -7, "ipa": 2.0 ** -7}
    assert flags(lambda: ops.pack_planes(big)) == 2 and ops.range_headroom()["node"] == 2.0
    inf = x.clone(); inf[1, 1] = float("inf")
    assert flags(lambda: ops.pack_planes(inf)) == 2
    xp = ops.pack_planes(x)
    assert flags(lambda: ops.node_apply(xp, layer, M, want_xp=True)) == 0
    assert flags(lambda: ops.node_apply(xp, layer, M, want_xp=True, pre_scale=torch.full((M,), 3.0e4, device=DEV))) == 1
    assert flags(lambda: ops.node_apply(xp, layer, M, want_xp=False, pre_scale=torch.full((M,), 3.0e4, device=DEV))) == 0   # fp32 output only: nothing is split
    et = net.translator.trunk["edge_transition_0"]
    node = torch.randn(1, 20, 256, generator=g).to(DEV)
    edge = torch.randn(1, 20, 20, 128, generator=g).to(DEV)
    assert flags(lambda: et(node, edge)) == 0
    assert flags(lambda: et(node, edge * 5.0e4)) & 4            # the edge row itself leaves the range
    hot = edge.clone(); hot[0, 3, 4] *= 2.0e4                    # ONE pair of the 400 leaves the range
    assert flags(lambda: et(node, hot)) & 4
    emb = net.embedder
    args = dict(residue_idx=torch.arange(20)[None], t=torch.full((1,), 0.4), fixed_mask=torch.zeros(1, 20).to(DEV),
                self_conditioning_ca=torch.randn(1, 20, 3, generator=g).to(DEV))
    assert flags(lambda: emb(**args)) == 0
    emb.edge_embed[0].weight.mul_(1.0e5)                           # first-layer rows (gathered tables) beyond the range
    assert flags(lambda: emb(**args)) & 8
    # the points are formed relative to an origin of the sample's own (csrc/ipa_attention_f16w.hip, sample_origin): a whole chain at
    # 40 000 (nm / 10) stays in range, one residue 80 000 away from the rest of its chain does not -- its points overflow
    r7 = torch.zeros(1, 32, 7, device=DEV); r7[..., 0] = 1; r7[..., 4:] = 4.0e4
    ipa = net.translator.trunk["ipa_0"]
    d = ipa._derived()
    qp = torch.zeros(32, 192, device=DEV); kvp = torch.zeros(32, 480, device=DEV)
    assert flags(lambda: ops.ipa_prep_points_f16(r7, qp, kvp, d["hw"])) == 0
    r7[0, 5, 4:] = -4.0e4
    assert flags(lambda: ops.ipa_prep_points_f16(r7, qp, kvp, d["hw"])) == 16
    qkv = torch.randn(64, 960, generator=g).to(DEV)
    for ar in MODES:   # the exact kernel reports what it writes as planes, the f16x3 kernel also the q / k / v it splits
        assert flags(lambda: ops.encoder_attention(qkv, None, 2, 32, arith=ar)) == 0
        assert flags(lambda: ops.encoder_attention(qkv * 1.0e5, None, 2, 32, arith=ar)) == 32


def test_range_buffer_is_per_call_across_streams():
    """The C ABI takes the range guard's buffer with each call (include/str2str_hip.h): two streams with two buffers each see only their
    own call's report, and a call with range_words = NULL records nothing anywhere."""
    import ctypes

    from str2str_amd import ops

    lib = ops.load_library()
    g = torch.Generator().manual_seed(9)
    M, K = 64, 256
    ok = torch.randn(M, K, generator=g).to(DEV)
    big = ok.clone(); big[7, 33] = 4.0e4
    words_a, words_b = (torch.zeros(8, dtype=torch.int32, device=DEV) for _ in range(2))
    xp_a, xp_b = ops.xp_alloc(M, K, DEV), ops.xp_alloc(M, K, DEV)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    ops.range_flag_reset()
    torch.cuda.synchronize()

    def pack(x, xp, words, stream):
        assert lib.s2s_pack_planes(ops.binding._p(x), M, K, 0, K, ops.binding._p(xp), K // 16, 0, None, ops.binding._p(words),
                                   ctypes.c_void_p(stream.cuda_stream)) == 0

    pack(big, xp_a, words_a, sa)
    pack(ok, xp_b, words_b, sb)
    torch.cuda.synchronize()
    assert words_a[0].item() == 2 and not words_b.any()
    words_a.zero_()
    pack(big, xp_a, None, sa)
    torch.cuda.synchronize()
    assert not words_a.any() and not words_b.any() and not ops.range_flag().any()


@pytest.mark.parametrize("where,scale,why,fams", [("et", 8.0e3, "edge transition", ()),
                                                  ("et", 3.0e4, "a weight does not fit", ("node", "edge_transition", "edge_embed", "ipa")),
                                                  ("nt", 1.0e3, "node GEMM", ("node",))], ids=["activation", "weight", "node-activation"])
def test_range_guard_falls_back_per_kernel_family(diffuser, caplog, where, scale, why, fams):
    """A network that leaves f16's range in ONE place (a layer scaled by s, the next by 1 / s: the same function in exact arithmetic --
    "et": EdgeTransition 1, s = 8e3: hidden activations beyond 2^15, s = 3e4: the weights themselves beyond the f16x3 packing;
    "nt": NodeTransition 0, hidden activations beyond 2^15) is sampled in the default arithmetic: the first chunk raises the range
    flag (or the packing refuses the weight) and is re-run with ONLY the kernel family that raised it on its exact fp32 kernels
    (every family for an unpackable weight); the result IS that mixed arithmetic's (bit for bit, same noise) and within rounding of
    the all-fp32 network's, a warning names the cause and the family, the demotion persists (``net.range_fallback``), the other
    families stay on f16x3 -- an overflow in the node stream does not cost the edge transitions their 3x -- and nothing is non-finite.
    The edge transitions themselves are NOT demoted for an activation (case "activation": 8e3 x the hidden layer, ~2^17): their
    kernel gets a block exponent (``prescale_exp`` 5, ``net.range_prescale``) and every family ends on f16x3; the result is bit for
    bit that of the network with the exponent set by hand, and within rounding of the all-fp32 network's.
    The un-scaled network, same seed, never leaves f16x3."""
    import logging

    from str2str_amd import ops
    from str2str_amd.arith import FAMILIES
    from str2str_amd.common.rigid_utils import Rigid
    from str2str_amd.factory import build_synthetic_net
    from str2str_amd.sampler import forward_backward
    from str2str_amd.synth import synth_chain

    N, B, S = 21, 3, 5
    feats = synth_chain(N)
    rig0 = Rigid.from_tensor_4x4(feats["rigidgroups_gt_frames"][..., 0, :, :].repeat(B, 1, 1, 1))

    def build(scale):
        net = build_synthetic_net(seed=0, sigma_final=0.002, device=DEV)
        with torch.no_grad():
            if where == "et":
                et = net.translator.trunk["edge_transition_1"]
                et.trunk[0].weight.mul_(scale); et.trunk[0].bias.mul_(scale)
                et.trunk[2].weight.div_(scale)
            else:
                # hidden activations x 1e3, then x 1e4 (ReLU is positively homogeneous: linear_3 / 1e4 restores the function); the
                # factor is spread over two layers so that the weights themselves still fit the f16x3 packing
                nt = net.translator.trunk["node_transition_0"]
                k1, k2 = (scale, 100.0) if scale > 1.0 else (1.0, 1.0)
                nt.linear_1.weight.mul_(k1); nt.linear_1.bias.mul_(k1)
                nt.linear_2.weight.mul_(k2); nt.linear_2.bias.mul_(k1 * k2)
                nt.linear_3.weight.div_(k1 * k2)
        return net

    def run(net, **kw):
        torch.manual_seed(9)
        return forward_backward(net, diffuser, feats, rig0, 1.0, num_timesteps=S, device=DEV, **kw).clone()

    plain = build(1.0)
    ref_plain = run(plain)
    assert not getattr(plain, "range_fallback", None)
    hot = build(scale)
    with use_arith(hot, "f32"):
        want_all = run(hot)                               # the exact arithmetic on the scaled network
    assert backbone_rmsd(want_all.cpu().numpy()[..., :5, :], ref_plain.cpu().numpy()[..., :5, :]) < 1e-3   # (the same function up to rounding)
    ets = [m for m in hot.modules() if hasattr(m, "prescale_exp")]
    presc = where == "et" and not fams                   # the edge transitions answer an activation with a block exponent
    if presc:
        for m in ets:
            m.prescale_exp = 5
    with use_arith(hot, "f32", families=fams):
        want = run(hot)                                   # only the offending family exact / the exponent set by hand
    for m in ets:
        m.prescale_exp = 0
    assert backbone_rmsd(want.cpu().numpy()[..., :5, :], want_all.cpu().numpy()[..., :5, :]) < 1e-4
    with caplog.at_level(logging.WARNING, logger="str2str_amd.sampler"):
        got = run(hot)
    msgs = [r.getMessage() for r in caplog.records]
    assert any("range guard" in m and why in m for m in msgs), msgs
    assert (getattr(hot, "range_fallback", None) or frozenset()) == frozenset(fams) and torch.isfinite(got).all()
    if presc:
        assert hot.range_prescale == {"edge_transition": 5} and {int(m.prescale_exp) for m in ets} == {5}
        assert any("block exponent" in m for m in msgs)
    assert set(FAMILIES) - set(getattr(hot, "range_fallback", None) or ()) or len(fams) == len(FAMILIES)
    assert torch.equal(got, want)
    assert torch.equal(run(hot), want)                   # later chunks go straight to the demoted form
    assert {m.arith for m in hot.modules() if hasattr(m, "arith")} == {"f16x3"}     # (the switches themselves are untouched between chunks)
    # SDE branch: the re-run re-draws the noise of the first pass from the saved generator state, so it equals a plain run of the
    # mixed arithmetic under the same seed, and leaves the generator where one pass leaves it
    hot2 = build(scale)
    ets2 = [m for m in hot2.modules() if hasattr(m, "prescale_exp")]
    for m in ets2:
        m.prescale_exp = 5 if presc else 0
    with use_arith(hot2, "f32", families=fams):
        want_sde = run(hot2, probability_flow=False)
        end_state = torch.get_rng_state()
    for m in ets2:
        m.prescale_exp = 0
    assert torch.equal(run(hot2, probability_flow=False), want_sde)
    assert (getattr(hot2, "range_fallback", None) or frozenset()) == frozenset(fams)
    assert torch.equal(torch.get_rng_state(), end_state)
    # what the guard saw: the offending family's bucket is at or above 2^15, the others well below
    head = ops.range_headroom()
    assert set(head) == set(FAMILIES)


def test_range_guard_covers_merged_t_deltas(diffuser, caplog):
    """The t_deltas of a target as one growing batch (``forward_backward_deltas``) run under the same range guard as a single
    trajectory: a network whose EdgeTransition hidden layer leaves f16's range (8e3 x, restored by the next layer) raises the flag in
    the merged pass, the edge transitions get their block exponent, the pass is repeated from the same start frames and host noise,
    and the samples are bit for bit those of the t_delta-by-t_delta run of the network with the exponent set by hand; the host
    generator ends where one pass leaves it."""
    import logging

    from str2str_amd.factory import build_synthetic_net
    from str2str_amd.sampler import forward_backward_deltas, rank_chunk_slices
    from str2str_amd.synth import synth_chain

    def build():
        net = build_synthetic_net(seed=0, sigma_final=0.002, device=DEV)
        with torch.no_grad():
            et = net.translator.trunk["edge_transition_1"]
            et.trunk[0].weight.mul_(8.0e3); et.trunk[0].bias.mul_(8.0e3)
            et.trunk[2].weight.div_(8.0e3)
        return net

    feats = synth_chain(21)
    gt4 = feats["rigidgroups_gt_frames"][..., 0, :, :]
    chunks, deltas = rank_chunk_slices(4, 3, 0, 1), [0.4, 0.7]
    kw = dict(num_timesteps=10, device=DEV, rng="host", probability_flow=True)
    ref_net = build()
    for m in ref_net.modules():
        if hasattr(m, "prescale_exp"):
            m.prescale_exp = 5
    os.environ["S2S_MERGE_DELTAS"] = "0"
    try:
        torch.manual_seed(12)
        want = forward_backward_deltas(ref_net, diffuser, feats, gt4, chunks, deltas, **kw)
        end_state = torch.get_rng_state()
    finally:
        del os.environ["S2S_MERGE_DELTAS"]
    assert not getattr(ref_net, "range_fallback", None)
    hot = build()
    torch.manual_seed(12)
    with caplog.at_level(logging.WARNING, logger="str2str_amd.sampler"):
        got = forward_backward_deltas(hot, diffuser, feats, gt4, chunks, deltas, **kw)
    assert any("range guard" in r.getMessage() and "block exponent" in r.getMessage() for r in caplog.records)
    assert hot.range_prescale == {"edge_transition": 5} and not getattr(hot, "range_fallback", None)
    assert all(torch.isfinite(g).all() and torch.equal(g, w) for g, w in zip(got, want))
    assert torch.equal(torch.get_rng_state(), end_state)


@pytest.mark.parametrize("fixture", ["net_b2n24_trained_like.npz", "net_b1n256_trained_like.npz"])
def test_trained_like_magnitudes_golden(fixture):
    """One evaluation (B = 2, N = 24; B = 1, N = 256: the bench shape) with trained-like weight magnitudes (LayerNorm gains up to 10, dense weights 2x the fan-in scale: hidden
    activations of several tens, an ill-conditioned network) against the reference.  The yardstick is the reference's OWN float32
    uncertainty on this input (``ref_spread``: its output under 1 / 2 / 4 / 8 CPU threads and one-ulp jitter of its float inputs,
    tests/golden/make_golden_configs.py --trained): both arithmetics of this build must stay within 3x of it, without touching
    the range guard."""
    from str2str_amd import ops
    from str2str_amd.factory import build_net
    from str2str_amd.synth import synth_state_dict

    g = golden(fixture)
    tag = fixture.split("_")[1]
    net = build_net().to(DEV).eval()
    man = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict(synth_state_dict(man, seed=0, sigma_final=0.02, style="trained_like"))
    spread, spread_psi = float(g["ref_spread"]), float(g["ref_psi_spread"])
    for mode in MODES:
        with use_arith(net, mode):
            ops.range_flag_reset()
            out = net(_batch(g, DEV))
            assert ops.range_flag_read() == 0
        check(f"trained-like net golden {tag} [{mode}]: max |frames - reference| (reference's own float32 spread {spread:.1e})",
              maxdiff(out["rigids"].to_tensor_7().cpu(), g["rigids7"]), 3 * spread)
        check(f"trained-like net golden {tag} [{mode}]: max |psi - reference| (spread {spread_psi:.1e})", maxdiff(out["psi"].cpu(), g["psi"]),
              3 * spread_psi)


def test_hip_graph_replay_is_bit_identical(net_smooth, diffuser, monkeypatch):
    """The captured-graph replay of the network evaluation (used for tiny, launch-bound chunks) gives the same bits."""
    from str2str_amd.common.rigid_utils import Rigid
    from str2str_amd.sampler import forward_backward
    from str2str_amd.synth import synth_chain

    N, B = 24, 3
    feats = synth_chain(N)
    rig0 = Rigid.from_tensor_4x4(feats["rigidgroups_gt_frames"][..., 0, :, :].repeat(B, 1, 1, 1))
    outs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("S2S_HIP_GRAPH", mode)
        torch.manual_seed(11)
        outs[mode] = forward_backward(net_smooth, diffuser, feats, rig0, 1.0, num_timesteps=6, device=DEV).clone()
    assert torch.isfinite(outs["1"]).all() and torch.equal(outs["0"], outs["1"])


def test_hip_graph_cache_survives_other_shapes(net_smooth, diffuser, monkeypatch):
    """A cached graph is replayed after evaluations of OTHER shapes / targets rebuilt the embedder's per-target tables (the default
    config's chunks of 64 + 36 replicas do exactly this every t_delta): capture A, capture B, churn the allocator, replay A --
    still the eager result, bit for bit.  (The captured kernels read those tables through raw pointers; the graph object owns them.)"""
    from str2str_amd import sampler
    from str2str_amd.common.rigid_utils import Rigid
    from str2str_amd.synth import synth_chain

    def run(N, B, seed, mode):
        monkeypatch.setenv("S2S_HIP_GRAPH", mode)
        feats = synth_chain(N)
        feats["residue_idx"] = feats["residue_idx"] + 3 * N      # another residue numbering per target: other tables
        rig0 = Rigid.from_tensor_4x4(feats["rigidgroups_gt_frames"][..., 0, :, :].repeat(B, 1, 1, 1))
        torch.manual_seed(seed)
        return sampler.forward_backward(net_smooth, diffuser, feats, rig0, 1.0, num_timesteps=5, device=DEV).clone()

    sampler._GRAPH_CACHE.clear()
    eager_a, eager_b = run(20, 3, 1, "0"), run(13, 2, 2, "0")
    a1 = run(20, 3, 1, "1")
    b1 = run(13, 2, 2, "1")          # frees / replaces the single-slot tables shape A was captured with
    assert len(sampler._GRAPH_CACHE) == 2
    torch.cuda.empty_cache()
    junk = [torch.full((1 << 18,), float("nan"), device=DEV) for _ in range(64)]   # whatever was freed gets overwritten
    a2 = run(20, 3, 1, "1")          # cache hit: replays graph A
    del junk
    assert len(sampler._GRAPH_CACHE) == 2
    assert torch.equal(a1, eager_a) and torch.equal(b1, eager_b) and torch.equal(a2, eager_a)


def test_graph_pins_every_derived_tensor_of_the_modules(net_smooth, diffuser, monkeypatch):
    """After a real (eager) evaluation, every tensor that module state holds -- reachable from any module's ``vars()`` through dicts, lists
    and tuples -- and that is no parameter or buffer is one ``sampler._graph_read_tensors`` pins, by identity: module state keeps derived
    device tensors in ``layers.DerivedCache`` slots only.  A bare cached attribute (which a captured graph would read after the next
    evaluation freed it) fails here."""
    from str2str_amd import sampler
    from str2str_amd.common.rigid_utils import Rigid
    from str2str_amd.synth import synth_chain

    def tensors(x, out):
        if torch.is_tensor(x):
            out.append(x)
        elif isinstance(x, (dict, list, tuple)):
            for v in (x.values() if isinstance(x, dict) else x):
                tensors(v, out)
        return out

    N, B = 12, 2
    feats = synth_chain(N)
    rig0 = Rigid.from_tensor_4x4(feats["rigidgroups_gt_frames"][..., 0, :, :].repeat(B, 1, 1, 1))
    monkeypatch.setenv("S2S_HIP_GRAPH", "0")
    torch.manual_seed(3)
    assert torch.isfinite(sampler.forward_backward(net_smooth, diffuser, feats, rig0, 1.0, num_timesteps=2, device=DEV)).all()
    own = {id(t) for t in list(net_smooth.parameters()) + list(net_smooth.buffers())}
    pinned = {id(t) for t in sampler._graph_read_tensors(net_smooth)}
    assert len(pinned) > 100
    loose = [(type(m).__name__, name, tuple(t.shape)) for m in net_smooth.modules() for name, v in vars(m).items()
             for t in tensors(v, []) if id(t) not in own and id(t) not in pinned]
    assert not loose, loose


def test_hip_graph_key_separates_a_launch_switch(net_smooth, diffuser, monkeypatch):
    """A switch that selects kernels (``fold`` of the IPA blocks, declared in ``launch_switches``) is part of the graph key: flipping it
    captures a second graph instead of replaying the first, and each replay is its own eager run bit for bit."""
    from str2str_amd import sampler
    from str2str_amd.common.rigid_utils import Rigid
    from str2str_amd.synth import synth_chain

    N, B = 20, 3
    feats = synth_chain(N)
    rig0 = Rigid.from_tensor_4x4(feats["rigidgroups_gt_frames"][..., 0, :, :].repeat(B, 1, 1, 1))
    ipas = [m for m in net_smooth.modules() if type(m).__name__ == "InvariantPointAttention"]
    keep = [m.fold for m in ipas]

    def run(mode, fold):
        monkeypatch.setenv("S2S_HIP_GRAPH", mode)
        for m, k in zip(ipas, keep):
            m.fold = k if fold else False
        torch.manual_seed(7)
        return sampler.forward_backward(net_smooth, diffuser, feats, rig0, 1.0, num_timesteps=5, device=DEV).clone()

    assert len(ipas) == 4 and all(keep)
    sampler._GRAPH_CACHE.clear()
    try:
        graph_default = run("1", True)
        graph_unfolded = run("1", False)
        assert len(sampler._GRAPH_CACHE) == 2
        eager_unfolded, eager_default = run("0", False), run("0", True)
    finally:
        for m, k in zip(ipas, keep):
            m.fold = k
    assert torch.isfinite(graph_default).all() and torch.equal(graph_unfolded, eager_unfolded) and torch.equal(graph_default, eager_default)

def test_cfg4_shape_n512_arithmetics_agree_and_shard(net_smooth, diffuser):
    """BASELINE configs[3] shape (N = 512), properties that need no reference (the reference-generated N = 512 evaluation and
    trajectory are in test_denoising_net_golden / test_free_running_trajectory_rmsd[n512_s10]): the default f16x3 arithmetic and
    the exact-fp32 arithmetic give the same conformations, replica sharding reproduces the single-process result, everything
    finite; N = 512 exercises 4 query blocks per head and the persistent tile loops."""
    from str2str_amd.common.rigid_utils import Rigid
    from str2str_amd.sampler import forward_backward
    from str2str_amd.synth import synth_chain

    N, B, S = 512, 3, 3
    feats = synth_chain(N)
    rig0 = Rigid.from_tensor_4x4(feats["rigidgroups_gt_frames"][..., 0, :, :].repeat(B, 1, 1, 1))
    outs = {}
    for mode in MODES:
        with use_arith(net_smooth, mode):
            torch.manual_seed(5)
            outs[mode] = forward_backward(net_smooth, diffuser, feats, rig0, 0.5, num_timesteps=2 * S, device=DEV).cpu().numpy()
    assert np.isfinite(outs["f16x3"]).all() and outs["f16x3"].shape == (B, N, 37, 3)
    check("N = 512 trajectory, f16x3 vs exact fp32 arithmetic (RMSD, A)", backbone_rmsd(outs["f16x3"][..., :5, :], outs["f32"][..., :5, :]), 5e-5)
    parts = []
    for r in range(2):
        torch.manual_seed(5)
        parts.append(forward_backward(net_smooth, diffuser, feats, rig0, 0.5, num_timesteps=2 * S, device=DEV, shard=(r, 2)).cpu().numpy())
    assert np.array_equal(np.concatenate(parts), outs["f16x3"])      # a replica's trajectory does not depend on which ranks' chunk it is in

@pytest.mark.parametrize("tag", ["n16_s20", "n12_prior", "n24_delta", "cfg1_n64_s20", "n256_s5", "n256_s100", "n512_s10"])
def test_free_running_trajectory_rmsd(net_smooth, diffuser, tag):
    """Same input, same seed, contractive synthetic weights: backbone RMSD vs the reference <= 1e-4 A.
    n256_s100 is the HEADLINE workload as the reference itself runs it (BASELINE configs[1]: 256 residues, 100 denoise
    steps + the self-conditioning evaluation, B = 2 replicas): final coordinates AND the frames entering steps 25 / 50 / 75 /
    99 are compared, so a divergence would be located, not just detected.  n512_s10 = BASELINE configs[3]'s chain length (N = 512,
    10 + 1 evaluations, B = 1) on the default f16x3 arithmetic."""
    from str2str_amd.common.rigid_utils import Rigid
    from str2str_amd.sampler import forward_backward
    from str2str_amd.synth import synth_chain

    g = golden(f"traj_free_{tag}.npz")
    N, B = int(g["n_res"]), int(g["B"])
    feats = synth_chain(N)
    rig0 = Rigid.from_tensor_4x4(feats["rigidgroups_gt_frames"][..., 0, :, :].repeat(B, 1, 1, 1))
    torch.manual_seed(int(g["seed"]))
    marks = sorted(int(k[len("rigids_t_step"):]) for k in g if k.startswith("rigids_t_step"))
    trace = [] if marks else None
    a37 = forward_backward(net_smooth, diffuser, feats, rig0, float(g["t_delta"]), num_timesteps=int(g["num_timesteps"]),
                           device=DEV, trace=trace)
    for k in marks:  # translations in Angstrom, quaternions up to sign-free float32 agreement
        want = g[f"rigids_t_step{k}"]
        got = trace[k]["rigids_t"].cpu().numpy()
        dq = np.minimum(np.abs(got[..., :4] - want[..., :4]).max(-1), np.abs(got[..., :4] + want[..., :4]).max(-1))  # q ~ -q
        d = float(max(dq.max(), np.abs(got[..., 4:] - want[..., 4:]).max()))
        record_margin(f"free-running {tag}: max |frames entering step {k} - reference|", d, 1e-4)
        assert d < 1e-4, (tag, k, d)
    rmsd = backbone_rmsd(a37.cpu().numpy()[..., :5, :], g["atom37"])
    record_margin(f"free-running {tag}: backbone RMSD vs reference (A)", rmsd, 1e-4)
    assert rmsd < 1e-4, (tag, rmsd)


def test_merged_chunks_equal_chunk_by_chunk(net_smooth, diffuser, monkeypatch):
    """The reference's replica chunks (diffusion_module.py:341-351) are the unit of its host noise stream, not of the arithmetic:
    ``forward_backward_chunks`` draws chunk by chunk in the reference's order and samples the chunks that fit the pair budget as ONE
    trajectory.  Bit for bit the chunk-by-chunk run (S2S_MERGE_CHUNKS=0 = the reference's control flow), the host generator ends
    where that run leaves it, and a rank's part of the merged run is the matching part of the single-process run."""
    from str2str_amd.sampler import forward_backward_chunks, merge_chunk_groups, rank_chunk_slices
    from str2str_amd.synth import synth_chain

    for n_res, t_delta in ((20, 0.5), (40, 1.0)):
        feats = synth_chain(n_res)
        gt4 = feats["rigidgroups_gt_frames"][..., 0, :, :]
        kw = dict(num_timesteps=8, device=DEV, rng="host", probability_flow=True)
        chunks = rank_chunk_slices(7, 3, 0, 1)                      # 3 + 3 + 1 replicas
        assert len(merge_chunk_groups(chunks, n_res)) == 1
        monkeypatch.setenv("S2S_MERGE_CHUNKS", "0")
        torch.manual_seed(21)
        ref = forward_backward_chunks(net_smooth, diffuser, feats, gt4, chunks, t_delta, **kw)
        state_ref = torch.get_rng_state()
        monkeypatch.setenv("S2S_MERGE_CHUNKS", "1")
        torch.manual_seed(21)
        got = forward_backward_chunks(net_smooth, diffuser, feats, gt4, chunks, t_delta, **kw)
        assert got.shape == ref.shape == (7, n_res, 37, 3)
        assert torch.equal(got.cpu(), ref.cpu())
        assert torch.equal(torch.get_rng_state(), state_ref)
        # a pair budget in between: (3 + 3) | 1
        torch.manual_seed(21)
        two = forward_backward_chunks(net_smooth, diffuser, feats, gt4, chunks, t_delta, max_pairs=6 * n_res * n_res, **kw)
        assert torch.equal(two.cpu(), ref.cpu())
        # two ranks, back to back on this GPU: rank-major concatenation of the merged runs == the single-process run
        parts = []
        for r in range(2):
            torch.manual_seed(21)
            parts.append(forward_backward_chunks(net_smooth, diffuser, feats, gt4, rank_chunk_slices(7, 3, r, 2), t_delta, **kw))
        assert parts[0].shape[0] == 4 and parts[1].shape[0] == 3
        assert torch.equal(torch.cat(parts).cpu(), ref.cpu())
    # the SDE with host noise keeps one trajectory per chunk (its per-step draws are part of the trajectory)
    assert len(merge_chunk_groups(chunks, 20, mergeable=False)) == 3


def test_merged_t_deltas_equal_one_at_a_time(net_smooth, diffuser, monkeypatch):
    """The t_deltas of a target (the outer loop of the reference's predict_step, diffusion_module.py:341-367) as ONE growing batch
    (``forward_backward_deltas``: trajectories aligned at their end, per-sample timestep image / step parameters / step size) --
    bit for bit the t_delta-by-t_delta run (S2S_MERGE_DELTAS=0), in both noise modes, with the host generator ending where the
    reference's control flow leaves it; a pair budget in between and a rank's slice give the same samples."""
    from str2str_amd.sampler import forward_backward_chunks, forward_backward_deltas, merge_delta_groups, rank_chunk_slices, schedule
    from str2str_amd.synth import synth_chain

    deltas = [0.3, 0.5, 0.8]                                         # 6, 10, 16 steps of 20 timesteps
    for n_res, rng in ((20, "host"), (40, "host"), (33, "device")):
        feats = synth_chain(n_res)
        gt4 = feats["rigidgroups_gt_frames"][..., 0, :, :]
        kw = dict(num_timesteps=20, device=DEV, rng=rng, probability_flow=True)
        chunks = rank_chunk_slices(5, 3, 0, 1)                       # 3 + 2 replicas
        steps = [schedule(d, 20, 0.01)[1] for d in deltas]
        assert steps == [6, 10, 16] and merge_delta_groups(steps, 5, n_res) == [[0, 1, 2]]
        monkeypatch.setenv("S2S_MERGE_DELTAS", "0")
        torch.manual_seed(33); torch.cuda.manual_seed(33)
        ref = forward_backward_deltas(net_smooth, diffuser, feats, gt4, chunks, deltas, **kw)
        state_ref = torch.get_rng_state()
        torch.manual_seed(33); torch.cuda.manual_seed(33)
        one = [forward_backward_chunks(net_smooth, diffuser, feats, gt4, chunks, d, **kw) for d in deltas]   # (= what the switch selects)
        assert all(torch.equal(a, b) for a, b in zip(ref, one))
        monkeypatch.setenv("S2S_MERGE_DELTAS", "1")
        torch.manual_seed(33); torch.cuda.manual_seed(33)
        got = forward_backward_deltas(net_smooth, diffuser, feats, gt4, chunks, deltas, **kw)
        assert len(got) == 3 and all(g.shape == (5, n_res, 37, 3) for g in got)
        for g, r in zip(got, ref):
            assert torch.isfinite(g).all() and torch.equal(g.cpu(), r.cpu())
        assert torch.equal(torch.get_rng_state(), state_ref)
        assert not torch.equal(got[0], got[2])
        # a pair budget that holds two t_deltas: (0.3, 0.5) | 0.8
        torch.manual_seed(33); torch.cuda.manual_seed(33)
        two = forward_backward_deltas(net_smooth, diffuser, feats, gt4, chunks, deltas, max_pairs=2 * 5 * n_res * n_res, **kw)
        assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(two, ref))
        if rng == "host":   # two ranks, back to back on this GPU: rank-major concatenation == the single-process run, per t_delta
            parts = []
            for r in range(2):
                torch.manual_seed(33)
                parts.append(forward_backward_deltas(net_smooth, diffuser, feats, gt4, rank_chunk_slices(5, 3, r, 2), deltas, **kw))
            for k in range(3):
                assert torch.equal(torch.cat([parts[0][k], parts[1][k]]).cpu(), ref[k].cpu())
    # descending t_deltas (the longest trajectory is not the last one drawn): everything is drawn up front, same samples
    feats = synth_chain(20)
    gt4 = feats["rigidgroups_gt_frames"][..., 0, :, :]
    kw = dict(num_timesteps=20, device=DEV, rng="host", probability_flow=True)
    monkeypatch.setenv("S2S_MERGE_DELTAS", "0")
    torch.manual_seed(4)
    ref = forward_backward_deltas(net_smooth, diffuser, feats, gt4, chunks, deltas[::-1], **kw)
    state_ref = torch.get_rng_state()
    monkeypatch.setenv("S2S_MERGE_DELTAS", "1")
    torch.manual_seed(4)
    got = forward_backward_deltas(net_smooth, diffuser, feats, gt4, chunks, deltas[::-1], **kw)
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(got, ref)) and torch.equal(torch.get_rng_state(), state_ref)
    # the SDE with host noise (one chunk per batch, its step draws used inside the loop) through the chunk and t_delta drivers: the
    # chunks sampled one by one in stream order under the same seed, by value and by generator state
    from str2str_amd.common.rigid_utils import Rigid
    from str2str_amd.sampler import forward_backward

    kw = dict(num_timesteps=20, device=DEV, rng="host", probability_flow=False)
    torch.manual_seed(8)
    got = forward_backward_deltas(net_smooth, diffuser, feats, gt4, chunks, [0.3, 0.5], **kw)
    state_got = torch.get_rng_state()
    torch.manual_seed(8)
    for d, g in zip([0.3, 0.5], got):
        one = [forward_backward(net_smooth, diffuser, feats, Rigid.from_tensor_4x4(gt4.repeat(bsz, 1, 1, 1)), d, replica_slice=(lo, hi), **kw)
               for bsz, lo, hi in chunks]
        assert g.shape == (5, 20, 37, 3) and torch.equal(g, torch.cat(one))
    assert torch.equal(torch.get_rng_state(), state_got)


def test_sharded_sampler_equals_single(net_smooth, diffuser):
    """Replica sharding (2 'ranks' run back to back on one GPU) reproduces the unsharded chunk."""
    from str2str_amd.common.rigid_utils import Rigid
    from str2str_amd.sampler import forward_backward
    from str2str_amd.synth import synth_chain

    feats = synth_chain(12)
    rig0 = Rigid.from_tensor_4x4(feats["rigidgroups_gt_frames"][..., 0, :, :].repeat(5, 1, 1, 1))
    kw = dict(num_timesteps=6, device=DEV)
    torch.manual_seed(5)
    full = forward_backward(net_smooth, diffuser, feats, rig0, 1.0, **kw)
    parts = []
    for r in range(2):
        torch.manual_seed(5)
        parts.append(forward_backward(net_smooth, diffuser, feats, rig0, 1.0, shard=(r, 2), **kw))
    assert parts[0].shape[0] == 3 and parts[1].shape[0] == 2
    # every kernel of the path treats a sample (a row, a pair) independently of its neighbours in the batch: bit for bit
    assert torch.equal(torch.cat(parts).cpu(), full.cpu())


def test_predict_step_entry_writes_reference_layout(tmp_path, monkeypatch):
    """eval.py task_name=inference end to end on a bundled PDB: output tree, MODEL counts, and — because the
    host generator is advanced exactly like the reference's (incl. the two unused float64 draws per step) —
    chunk 2 of the replicas also matches the oracle run chunk after chunk under the same seed."""
    import os
    import sys

    from conftest import GOLDEN, ROOT
    from oracle import diffuser as OD
    from oracle import geometry as OG
    from oracle import net as ON
    from str2str_amd.common import protein
    from str2str_amd.data.components.dataset import ProteinFeatureTransform

    monkeypatch.setenv("TEST_DATA", os.path.join(GOLDEN, "pdb"))
    monkeypatch.setenv("CACHE_DIR", str(tmp_path / "cache"))
    monkeypatch.setenv("PROJECT_ROOT", str(tmp_path))
    sys.path.insert(0, ROOT)
    import eval as entry

    args = ["task_name=inference", "ckpt_path=null", "data.dataset.accession_code_fillter=[CLN025]",
            "model.inference.n_replica=3", "model.inference.replica_per_batch=2", "model.inference.num_timesteps=10",
            "model.inference.delta_min=0.5", "model.inference.delta_max=0.6", "model.inference.delta_step=0.1",
            "extras.print_config=false"]
    all_dir = entry.main(args)
    samples = os.path.dirname(all_dir)
    assert sorted(os.listdir(samples)) == ["0.5", "0.6", "all_delta"]
    txt = open(os.path.join(samples, "0.5", "CLN025.pdb")).read()
    assert txt.count("MODEL ") == 3 and txt.endswith("END") and all(len(l) == 80 for l in txt.split("\n")[:-1])
    assert open(os.path.join(all_dir, "CLN025.pdb")).read().count("MODEL ") == 6

    # same objects, but seeded right before sampling (model construction itself consumes the generator)
    from str2str_amd.synth import synth_state_dict
    from str2str_amd.utils import config as C

    cfg = C.compose(os.path.join(ROOT, "configs"), "eval.yaml", args)
    model = C.instantiate(cfg.model)
    man = [(k, tuple(v.shape)) for k, v in model.net.state_dict().items()]
    model.net.load_state_dict(synth_state_dict(man, seed=0, sigma_final=0.002))
    model = model.to(DEV).eval()
    batch = C.instantiate(cfg.data).test_dataloader()[0]
    batch = {k: (v.to(DEV) if torch.is_tensor(v) and k != "residue_idx" else v) for k, v in batch.items()}
    torch.manual_seed(11)
    all_dir = model.predict_step(batch, 0)
    txt = open(os.path.join(os.path.dirname(all_dir), "0.5", "CLN025.pdb")).read()

    # oracle, same seed, same chunking (2 + 1 replicas), t_delta = 0.5 first
    feats = ProteinFeatureTransform(strip_missing_residues=False, recenter_and_scale=False)(
        protein.from_pdb_string(open(os.path.join(GOLDEN, "pdb", "CLN025.pdb")).read()).to_dict())
    sd = synth_sd(0, 0.002)
    d = OD.FrameDiffuser()
    torch.manual_seed(11)
    ref = []
    for B in (2, 1):
        f = {k: feats[k][None].repeat(B, *(1,) * feats[k].ndim) for k in
             ("aatype", "residue_mask", "fixed_mask", "residue_idx", "torsion_angles_sin_cos")}
        rig0 = OG.Frames.from_tensor_4x4(feats["rigidgroups_gt_frames"][None, :, 0].repeat(B, 1, 1, 1))
        ref.append(OD.forward_backward(lambda b: ON.denoising_net(sd, b), d, f, rig0, 0.5, num_timesteps=10))
    ref = np.concatenate(ref)[..., :5, :]
    got = np.array([[float(l[30:38]), float(l[38:46]), float(l[46:54])] for l in txt.split("\n") if l.startswith("ATOM")])
    want = []
    aat = feats["aatype"].numpy()
    for m in range(3):
        for i in range(ref.shape[1]):
            for a in range(5):
                if a == 3 and aat[i] == 7:
                    continue  # GLY has no CB line
                want.append(ref[m, i, a])
    want = np.array(want)
    assert got.shape == want.shape and np.abs(got - want).max() < 2e-3, np.abs(got - want).max()

    # evaluation step (src/eval.py:47-99) on the samples just written: device metrics -> the reference's tab-separated csv
    import glob

    mean = entry.evaluate_prediction(all_dir, os.path.join(GOLDEN, "pdb"), tag="t")
    files = glob.glob(os.path.join(os.path.dirname(os.path.dirname(all_dir)), "metrics_t_*.csv"))
    assert len(files) == 1
    rows = [ln.rstrip("\n").split("\t") for ln in open(files[0])]
    assert rows[0] == ["", "val_clash", "val_bond", "js_pwd", "js_rg", "js_tica"] and [r[0] for r in rows[1:]] == ["CLN025", "mean"]
    assert 0.0 <= float(mean["val_clash"]) <= 1.0 and 0.0 <= float(mean["js_pwd"]) <= 1.0


def _torchrun(n, script_args, env_extra, cwd, timeout=240):
    import os
    import socket
    import subprocess
    import sys

    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ, **env_extra)
    env.pop("PYTEST_CURRENT_TEST", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port)] + script_args
    return subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)


def test_js_tica_device_distances_and_tica():
    """metrics.js_tica (reference src/metrics/metrics.py:169-200): pairwise distances from the device equal numpy's, the TICA
    projection finds the slow coordinate of a synthetic trajectory, an ensemble scores 0 against itself and > 0 against a
    different one, and the score does not depend on which estimator's scale / sign convention produced the components."""
    from str2str_amd.metrics import metrics as M

    rng = np.random.default_rng(0)
    T_, L = 400, 12
    slow = np.cumsum(rng.normal(size=T_)) * 0.05                      # a slow coordinate (random walk) ...
    base = rng.normal(size=(L, 3)) * 4
    ca = base[None] + rng.normal(size=(T_, L, 3)) * 0.05
    ca[:, -1, 0] += slow                                              # ... moving the last residue along x
    pw = M.pairwise_distance_ca(ca)
    d = np.linalg.norm(ca[:, :, None] - ca[:, None], axis=-1)
    r_, c_ = np.triu_indices(L, k=1)
    assert pw.shape == (T_, L * (L - 1) // 2) and np.abs(pw - d[:, r_, c_]).max() < 1e-5
    mean, proj = M.tica_fit(pw, lagtime=20, dim=2)
    tic0 = (pw - mean) @ proj[:, 0]
    assert abs(np.corrcoef(tic0, slow)[0, 1]) > 0.9
    other = base[None] + rng.normal(size=(T_, L, 3)) * 0.05
    res, tics = M.js_tica({"target": ca, "pred": other, "same": ca.copy()}, ref_key="target")
    assert res["target"] == 0.0 and res["same"] == 0.0 and 0.05 < res["pred"] <= 1.0 and tics["pred"].shape == (T_, 2)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_js_tica_and_weighted_metrics_match_the_reference_driven_fixture(tag):
    """metrics.js_tica / js_pwd / js_rg incl. per-sample ``weights=`` (reference src/metrics/metrics.py:139-217) on the device path,
    against tests/golden/tica.npz: the values the REFERENCE's functions returned.  For js_tica the estimator behind the reference's
    call is the third-party deeptime TICA (0.4.4), absent here -- the fixture was produced by the reference's js_tica driving the
    restatement of its published algorithm in oracle/tica.py (make_golden_tica.py), not by a run of deeptime; js_pwd / js_rg with
    weights are the reference alone.  Rounded scores equal, projections to 1e-6 of their scale, weighted per-channel js_pwd to 1e-9."""
    from str2str_amd import ops
    from str2str_amd.metrics import metrics as M

    g = golden("tica.npz")
    d = {"target": g[f"{tag}_target"], "pred": g[f"{tag}_pred"]}
    w, lag = g[f"{tag}_weights"], int(g[f"{tag}_lag"])
    # the features: numpy's float32 arithmetic on the device, bit for bit (reference pairwise_distance_ca, metrics.py:38-50)
    for k_off in (1, 3):
        x = d["pred"]
        dm = np.sqrt(np.sum((x[..., None, :, :] - x[..., None, :]) ** 2, axis=-1))
        r_, c_ = np.triu_indices(x.shape[1], k=k_off)
        assert np.array_equal(M.pairwise_distance_ca(x, k=k_off), dm[..., r_, c_])
    res, tics = M.js_tica(d, ref_key="target", lagtime=lag)
    assert res["target"] == 0.0 and abs(res["pred"] - float(g[f"{tag}_js_tica"])) < 1.5e-4, (res, g[f"{tag}_js_tica"])
    for k in ("target", "pred"):
        scale = np.abs(g[f"{tag}_tic_{k}"]).max()
        check(f"js_tica {tag}: |projection - reference-driven restatement| / scale ({k})", float(np.abs(tics[k] - g[f"{tag}_tic_{k}"]).max() / scale), 1e-6)
    assert abs(M.js_tica(d, ref_key="target", lagtime=lag, weights={"pred": w}, return_tic=False)["pred"] - float(g[f"{tag}_js_tica_w"])) < 1.5e-4
    assert M.js_pwd(d, ref_key="target", weights={"pred": w})["pred"] == float(g[f"{tag}_js_pwd_w"])
    assert M.js_rg(d, ref_key="target", weights={"pred": w})["pred"] == float(g[f"{tag}_js_rg_w"])
    ch = ops.ca_pwd_js(T(d["target"]).to(DEV), T(d["pred"]).to(DEV), 3, 50, 1e-6, pred_weights=T(w).to(DEV)).cpu().numpy()
    check(f"js_pwd weighted {tag}: per-channel |JS - reference|", float(np.abs(ch - g[f"{tag}_js_pwd_w_channels"]).max()), 1e-9)
    # weights of ones are the unweighted metric, bit for bit in the rounded score
    ones = {"pred": np.ones(len(w)), "target": np.ones(len(d["target"]))}
    assert M.js_pwd(d, weights=ones) == M.js_pwd(d) and M.js_rg(d, weights=ones) == M.js_rg(d)


def test_multirank_entry_points_share_one_gpu(tmp_path):
    """The N > 1 control flow of BOTH entry points, launched exactly as the driver launches them (torch.distributed.run, one
    process per rank), with two ranks sharing this box's single GPU through the gloo test hooks (RCCL wants a GPU per rank; the
    collective backend is the only thing that differs from an 8-GPU node):
      bench.py --gpus 2: rendezvous, barriers, max-over-ranks timing, gather to rank 0, ONE JSON line with both per-rank rates;
      eval.py on 2 ranks writes the same PDB files, byte for byte, as eval.py on 1 rank (real sampler, replica-range sharding,
      host noise drawn identically on every rank and sliced, one gather per t_delta)."""
    import json
    import os

    from conftest import GOLDEN, ROOT

    r = _torchrun(2, ["bench.py", "--gpus", "2", "--config", "cfg2", "--n-res", "32", "--replicas", "4", "--denoise-steps", "6", "--steps", "2",
                      "--warmup", "1", "--no-cpu-baseline"], {"S2S_BENCH_BACKEND": "gloo"}, ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]            # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["distributed"]["world_size"] == 2 and d["distributed"]["backend"] == "gloo"
    rates = d["distributed"]["per_rank_conformations_per_s"]
    assert len(rates) == 2 and all(np.isfinite(x) and x > 0 for x in rates) and np.isfinite(d["value"]) and d["value"] > 0
    assert d["value"] <= sum(rates) * 1.001              # whole-job rate = all replicas / the slowest rank's time
    assert d["scaling"] == "weak" and d["config"]["replicas_per_gpu"] == 4
    assert d["distributed"]["ranks_seen"] == [0, 1] and d["distributed"]["devices_seen"] == 1     # the preflight saw both processes (one shared GPU here)
    assert set(d["config"]["range_headroom"]) == {"node", "edge_transition", "edge_embed", "ipa"} and d["config"]["range_fallback"] == []

    outs = {}
    for n in (1, 2):
        root = tmp_path / f"w{n}"
        env = {"S2S_DIST_BACKEND": "gloo", "TEST_DATA": os.path.join(GOLDEN, "pdb"), "CACHE_DIR": str(tmp_path / "cache"),
               "PROJECT_ROOT": str(root)}
        args = ["eval.py", "task_name=inference", "ckpt_path=null", "seed=7", "data.dataset.accession_code_fillter=[CLN025,2JOF]",
                "model.inference.n_replica=5", "model.inference.replica_per_batch=2", "model.inference.num_timesteps=6",
                "model.inference.delta_min=0.5", "model.inference.delta_max=0.6", "model.inference.delta_step=0.1",
                "extras.print_config=false", f"paths.output_dir={root}/out"]
        r = _torchrun(n, args, env, ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        files = {}
        for dp, _, fs in os.walk(root):
            for f in fs:
                if f.endswith(".pdb"):
                    files[os.path.relpath(os.path.join(dp, f), root)] = open(os.path.join(dp, f)).read()
        outs[n] = files
    assert len(outs[1]) == 6 and set(outs[1]) == set(outs[2])      # 2 targets x (0.5, 0.6, all_delta)
    for k in outs[1]:
        assert outs[1][k].count("MODEL ") in (5, 10) and outs[1][k] == outs[2][k], k


def test_bench_and_eval_start_their_own_ranks_from_a_bare_shell(tmp_path):
    """`python bench.py --gpus 2 ...` and `python eval.py trainer.devices=2 ...` typed into a bare shell (no torch.distributed.run, no
    WORLD_SIZE): the entry points launch their own ranks (str2str_amd/utils/launch.py; the reference's `trainer=ddp` needs no launcher
    either, src/eval.py:129,154).  Two ranks share this box's GPU through the gloo hooks."""
    import json
    import os
    import subprocess
    import sys

    from conftest import GOLDEN, ROOT

    bare = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "PYTEST_CURRENT_TEST")}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--n-res", "32", "--replicas", "3", "--denoise-steps", "4", "--steps", "1", "--warmup", "0",
                        "--no-cpu-baseline", "--no-kernel-table"], cwd=ROOT, env=dict(bare, S2S_BENCH_BACKEND="gloo"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["distributed"]["ranks_seen"] == [0, 1] and d["distributed"]["backend"] == "gloo" and d["value"] > 0
    outs = {}
    for n in (1, 2):
        root = tmp_path / f"bare{n}"
        env = dict(bare, S2S_DIST_BACKEND="gloo", TEST_DATA=os.path.join(GOLDEN, "pdb"), CACHE_DIR=str(tmp_path / "cache"), PROJECT_ROOT=str(root))
        r = subprocess.run([sys.executable, "eval.py", "task_name=inference", "ckpt_path=null", "seed=7", "data.dataset.accession_code_fillter=[CLN025]",
                            f"trainer.devices={n}", "model.inference.n_replica=3", "model.inference.replica_per_batch=2", "model.inference.num_timesteps=4",
                            "model.inference.delta_min=0.5", "model.inference.delta_max=0.5", "extras.print_config=false", f"paths.output_dir={root}/out"],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[n] = open(os.path.join(root, "out", "samples", "all_delta", "CLN025.pdb")).read()
    assert outs[1].count("MODEL ") == 3 and outs[1] == outs[2]


def test_rccl_one_rank_job_runs_the_device_collectives(tmp_path):
    """The `nccl` backend (= RCCL) on this MI355X: a ONE-rank torch.distributed.run job of each entry point -- librccl is loaded, the
    communicator is bound to the device (`device_id`), and DEVICE tensors go through the same gathers an 8-GPU node runs
    (gather_replicas, predict_mixed's flat gather, bench.py's gather + all_reduce + all_gather): the branch the gloo rehearsals
    cannot reach.  The files of the 1-rank RCCL job equal those of the plain single-process run byte for byte."""
    import json
    import os
    import subprocess
    import sys

    from conftest import GOLDEN, ROOT

    script = tmp_path / "rccl_gather.py"
    script.write_text(
        "import os, sys, torch, torch.distributed as dist\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from str2str_amd.models.diffusion_module import gather_replicas\n"
        "dev = torch.device('cuda', int(os.environ['LOCAL_RANK']))\n"
        "torch.cuda.set_device(dev)\n"
        "dist.init_process_group('nccl', device_id=dev)\n"
        "x = torch.zeros(5, 9, 37, 3, device=dev)\n"
        "x[:, :, :5] = torch.randn(5, 9, 5, 3, device=dev)\n"
        "out = gather_replicas(x, 5)\n"
        "assert out.is_cuda and torch.equal(out, x), 'device gather'\n"
        "t = torch.ones(3, device=dev)\n"
        "dist.all_reduce(t)\n"
        "torch.cuda.synchronize()\n"
        "print('RCCL_OK', dist.get_backend(), dist.get_world_size(), tuple(out.shape), flush=True)\n"
        "dist.barrier()\n"
        "dist.destroy_process_group()\n")
    r = _torchrun(1, [str(script)], {}, ROOT, timeout=300)
    assert r.returncode == 0 and "RCCL_OK nccl 1 (5, 9, 37, 3)" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])

    r = _torchrun(1, ["bench.py", "--gpus", "1", "--n-res", "32", "--replicas", "4", "--denoise-steps", "4", "--steps", "1", "--warmup", "0",
                      "--no-cpu-baseline", "--no-kernel-table", "--no-other-configs"], {}, ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["distributed"]["backend"] == "nccl" and d["distributed"]["world_size"] == 1 and d["distributed"]["devices_seen"] == 1 and d["value"] > 0
    out = os.path.join(ROOT, "gpurun_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "rccl_one_rank_bench_line.json"), "w") as f:   # (copied to profiles/ for the record)
        json.dump(d, f)

    base = ["eval.py", "task_name=inference", "ckpt_path=null", "seed=7", "model.inference.n_replica=3", "model.inference.num_timesteps=4",
            "model.inference.delta_min=0.5", "model.inference.delta_max=0.6", "model.inference.delta_step=0.1", "extras.print_config=false"]
    for tag, extra in (("step", ["data.dataset.accession_code_fillter=[CLN025]", "model.inference.replica_per_batch=2"]),
                       ("mixed", ["data.dataset.accession_code_fillter=[CLN025,2JOF]", "model.inference.mixed_batch=true"])):
        files = {}
        for how in ("plain", "rccl"):
            root = tmp_path / f"{tag}_{how}"
            env = {"TEST_DATA": os.path.join(GOLDEN, "pdb"), "CACHE_DIR": str(tmp_path / "cache"), "PROJECT_ROOT": str(root)}
            args = base + extra + [f"paths.output_dir={root}/out"]
            if how == "rccl":
                r = _torchrun(1, args, env, ROOT, timeout=300)
            else:
                bare = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "PYTEST_CURRENT_TEST")}
                r = subprocess.run([sys.executable] + args, cwd=ROOT, env=dict(bare, **env), capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, (tag, how, r.stderr[-2000:])
            files[how] = {os.path.relpath(os.path.join(dp, f), root): open(os.path.join(dp, f)).read()
                          for dp, _, fs in os.walk(root) for f in fs if f.endswith(".pdb")}
        assert files["plain"] and files["plain"] == files["rccl"], tag


def test_bench_plain_run_dumps_what_the_full_run_computes(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` (the plain run) times K steps and prints the headline fields only; --dump-outputs
    writes the last timed step's backbone in float32, the same from run to run and the same as under --full, whose per-launch
    timers and extra kernel-table step leave the sampled coordinates alone."""
    import json
    import os
    import subprocess
    import sys

    from conftest import ROOT

    bare = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "PYTEST_CURRENT_TEST")}
    shape = ["--gpus", "1", "--n-res", "32", "--replicas", "4", "--denoise-steps", "4", "--steps", "3", "--warmup", "1"]
    lines, dumps = {}, {}
    for tag, extra in (("a", []), ("b", []), ("full", ["--full", "--no-cpu-baseline"])):
        out = tmp_path / tag
        r = subprocess.run([sys.executable, "bench.py"] + shape + extra + ["--dump-outputs", str(out)], cwd=ROOT, env=bare,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(got) == 1, r.stdout[-2000:]
        lines[tag] = json.loads(got[0])
        assert os.listdir(out) == ["backbone.npy"]
        dumps[tag] = np.load(out / "backbone.npy")
    d = lines["a"]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["higher_is_better"] is True
    assert d["unit"] == "conformations/s" and d["dtype"].startswith("f32")
    assert not {"roofline", "ipa_kernel", "kernel_times", "cpu_baseline", "other_configs"} & set(d)
    assert {"roofline", "ipa_kernel", "kernel_times"} <= set(lines["full"])
    assert dumps["a"].dtype == np.float32 and dumps["a"].shape == (4, 32, 5, 3) and np.isfinite(dumps["a"]).all()
    assert np.array_equal(dumps["a"], dumps["b"]) and np.array_equal(dumps["a"], dumps["full"])


def test_full_size_batch_is_invariant_at_the_headline_shape(net_smooth, diffuser):
    """BASELINE configs[1] at its FULL batch: 128 replicas of the 256-residue chain as ONE trajectory (n_replica 128 in the reference's
    chunks of replica_per_batch 2, merged: 8 388 608 pairs per launch, the persistent workgroups walk many tiles each) for the 5 + 1
    evaluations of the `traj_free_n256_s5` fixture.  A replica's result must not depend on its batch (reference
    diffusion_module.py:341-352: chunks are independent): replicas 0-1 are the reference's own B = 2 run of the fixture (< 1e-4 A) and
    equal this build's B = 2 launch BIT FOR BIT; a 2-rank shard of the 128 (64 + 64) equals the single run bit for bit."""
    from str2str_amd.common.rigid_utils import Rigid
    from str2str_amd.sampler import forward_backward, forward_backward_chunks, rank_chunk_slices
    from str2str_amd.synth import synth_chain

    g = golden("traj_free_n256_s5.npz")
    N, S = int(g["n_res"]), int(g["num_timesteps"])
    assert (N, int(g["B"])) == (256, 2)
    feats = synth_chain(N)
    gt4 = feats["rigidgroups_gt_frames"][..., 0, :, :]
    kw = dict(num_timesteps=S, device=DEV)
    torch.manual_seed(int(g["seed"]))
    full = forward_backward_chunks(net_smooth, diffuser, feats, gt4, rank_chunk_slices(128, 2, 0, 1), float(g["t_delta"]), **kw)
    assert tuple(full.shape) == (128, N, 37, 3) and torch.isfinite(full).all()
    rmsd = backbone_rmsd(full[:2].cpu().numpy()[..., :5, :], g["atom37"])
    record_margin("full batch B=128, N=256: replicas 0-1 backbone RMSD vs the reference's B=2 run (A)", rmsd, 1e-4)
    assert rmsd < 1e-4, rmsd
    torch.manual_seed(int(g["seed"]))
    two = forward_backward(net_smooth, diffuser, feats, Rigid.from_tensor_4x4(gt4.repeat(2, 1, 1, 1)), float(g["t_delta"]), **kw)
    assert torch.equal(two, full[:2])
    ca = full[:, :, 1].reshape(128, -1)
    assert float(torch.cdist(ca, ca).fill_diagonal_(1e9).min()) > 1e-2        # 128 different conformations
    parts = []
    for r in range(2):
        torch.manual_seed(int(g["seed"]))
        parts.append(forward_backward_chunks(net_smooth, diffuser, feats, gt4, rank_chunk_slices(128, 2, r, 2), float(g["t_delta"]), **kw))
    assert parts[0].shape[0] == 64 and torch.equal(torch.cat(parts), full)


def test_full_size_batch_is_invariant_at_n512(net_smooth, diffuser):
    """BASELINE configs[3]'s chain length at the largest batch a trajectory holds (32 replicas x 512^2 = 8 388 608 pairs per launch: the
    pair budget of a merged trajectory; the bench's 128 replicas per GPU run as four of these), for the 10 + 1 evaluations of the
    `traj_free_n512_s10` fixture: replica 0 is the reference's own B = 1 run (< 1e-4 A) and equals this build's B = 1 launch bit for
    bit; a 2-rank shard of the 32 equals the single run bit for bit."""
    from str2str_amd.common.rigid_utils import Rigid
    from str2str_amd.sampler import forward_backward, forward_backward_chunks, rank_chunk_slices

    from str2str_amd.synth import synth_chain

    g = golden("traj_free_n512_s10.npz")
    N, S = int(g["n_res"]), int(g["num_timesteps"])
    assert (N, int(g["B"])) == (512, 1)
    feats = synth_chain(N)
    gt4 = feats["rigidgroups_gt_frames"][..., 0, :, :]
    kw = dict(num_timesteps=S, device=DEV)
    torch.manual_seed(int(g["seed"]))
    full = forward_backward_chunks(net_smooth, diffuser, feats, gt4, rank_chunk_slices(32, 1, 0, 1), float(g["t_delta"]), **kw)
    assert tuple(full.shape) == (32, N, 37, 3) and torch.isfinite(full).all()
    rmsd = backbone_rmsd(full[:1].cpu().numpy()[..., :5, :], g["atom37"])
    record_margin("full batch B=32, N=512: replica 0 backbone RMSD vs the reference's B=1 run (A)", rmsd, 1e-4)
    assert rmsd < 1e-4, rmsd
    torch.manual_seed(int(g["seed"]))
    one = forward_backward(net_smooth, diffuser, feats, Rigid.from_tensor_4x4(gt4.repeat(1, 1, 1, 1)), float(g["t_delta"]), **kw)
    assert torch.equal(one, full[:1])
    parts = []
    for r in range(2):
        torch.manual_seed(int(g["seed"]))
        parts.append(forward_backward_chunks(net_smooth, diffuser, feats, gt4, rank_chunk_slices(32, 1, r, 2), float(g["t_delta"]), **kw))
    assert parts[0].shape[0] == 16 and torch.equal(torch.cat(parts), full)


@pytest.mark.parametrize("cfg,extra", [("cfg4", ["--n-res", "32", "--replicas", "2", "--denoise-steps", "3"]),
                                       ("cfg5", ["--replicas", "1", "--denoise-steps", "2"])])
def test_bench_world8_rehearsal(cfg, extra):
    """The 8-rank plans of BASELINE configs[3] / configs[4] as the driver would launch them on an 8-GPU node (torch.distributed.run,
    --gpus 8), eight ranks sharing this box's GPU through the gloo hook, tiny shapes: rendezvous, the preflight that proves eight
    processes were seen, every rank's share of the plan, the gathers to rank 0 (cfg5: one padded flat buffer), ONE JSON line."""
    import json

    from conftest import ROOT

    r = _torchrun(8, ["bench.py", "--gpus", "8", "--config", cfg, "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-kernel-table"] + extra,
                  {"S2S_BENCH_BACKEND": "gloo"}, ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["distributed"]["ranks_seen"] == list(range(8))
    rates = d["distributed"]["per_rank_conformations_per_s"]
    assert len(rates) == 8 and all(np.isfinite(x) and x > 0 for x in rates) and np.isfinite(d["value"]) and d["value"] > 0


def test_eval_entry_mixed_batch(tmp_path, monkeypatch):
    """BASELINE configs[4] through the drop-in entry: ``eval.py ... model.inference.mixed_batch=true`` samples ALL targets in
    length-bucketed padded batches (DiffusionLitModule.predict_mixed) and writes the reference's output tree; under a fixed seed the
    files are exactly what ``sampler.sample_mixed_lengths`` returns for the same targets (which the cfg5 fixture test holds to the
    reference's per-chain runs), and a 2-rank launch writes the same tree."""
    import os
    import sys

    from conftest import GOLDEN, ROOT
    from str2str_amd.sampler import sample_mixed_lengths
    from str2str_amd.synth import synth_state_dict
    from str2str_amd.utils import config as C

    monkeypatch.setenv("TEST_DATA", os.path.join(GOLDEN, "pdb"))
    monkeypatch.setenv("CACHE_DIR", str(tmp_path / "cache"))
    monkeypatch.setenv("PROJECT_ROOT", str(tmp_path))
    sys.path.insert(0, ROOT)
    import eval as entry

    args = ["task_name=inference", "ckpt_path=null", "seed=3", "data.dataset.accession_code_fillter=[CLN025,2JOF,1FME]",
            "model.inference.mixed_batch=true", "model.inference.n_replica=3", "model.inference.num_timesteps=6",
            "model.inference.delta_min=0.5", "model.inference.delta_max=0.6", "model.inference.delta_step=0.1",
            "extras.print_config=false", f"paths.output_dir={tmp_path}/out"]
    all_dir = entry.main(args)
    samples = os.path.dirname(all_dir)
    assert sorted(os.listdir(samples)) == ["0.5", "0.6", "all_delta"]
    for code, n in (("CLN025", 10), ("2JOF", 20), ("1FME", 28)):
        txt = open(os.path.join(samples, "0.5", f"{code}.pdb")).read()
        assert txt.count("MODEL ") == 3 and txt.count(" CA ") == 3 * n
        assert open(os.path.join(all_dir, f"{code}.pdb")).read().count("MODEL ") == 6

    cfg = C.compose(os.path.join(ROOT, "configs"), "eval.yaml", args)
    model = C.instantiate(cfg.model)
    man = [(k, tuple(v.shape)) for k, v in model.net.state_dict().items()]
    model.net.load_state_dict(synth_state_dict(man, seed=0, sigma_final=0.002))
    model = model.to(DEV).eval()
    batches = list(C.instantiate(cfg.data).test_dataloader())
    torch.manual_seed(3)
    model.predict_mixed(batches)
    torch.manual_seed(3)
    want = sample_mixed_lengths(model.net, model.diffuser, batches, 3, 0.5, num_timesteps=6, device=DEV)
    # the per-batch host seeding leaves no trace in the process-global generators: the run seed is still the seed, and the
    # caller's stream continues where it was
    after = (torch.initial_seed(), float(torch.rand(1)), float(np.random.get_state()[1][0]))
    torch.manual_seed(3)
    assert after[:2] == (3, float(torch.rand(1)))
    for k, b in enumerate(batches):
        code = b["accession_code"][0]
        got = model.last_samples[(code, 0.5)]
        assert torch.isfinite(got).all() and torch.equal(got, torch.cat([p for _, p in want[k]]))
        xyz = np.array([[float(l[30:38]), float(l[38:46]), float(l[46:54])] for l in
                        open(os.path.join(samples, "0.5", f"{code}.pdb")).read().split("\n") if l.startswith("ATOM") and l[12:16].strip() == "CA"])
        assert np.abs(xyz - got.cpu().numpy()[:, :, 1].reshape(-1, 3)).max() < 1e-3     # the CLI run under the same seed wrote these samples

    env = {"S2S_DIST_BACKEND": "gloo", "TEST_DATA": os.path.join(GOLDEN, "pdb"), "CACHE_DIR": str(tmp_path / "cache"),
           "PROJECT_ROOT": str(tmp_path / "w2")}
    r = _torchrun(2, ["eval.py"] + args[:-1] + [f"paths.output_dir={tmp_path}/w2/out"], env, ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    for code in ("CLN025", "2JOF", "1FME"):
        txt = open(os.path.join(tmp_path, "w2", "out", "samples", "all_delta", f"{code}.pdb")).read()
        assert txt.count("MODEL ") == 6
        # every rank starts from the same run seed: the replicas it samples must still be different conformations (per-batch host
        # seeds, sampler.mixed_batch_seed) -- no two MODELs of a target coincide
        ca = [np.array([[float(l[30:38]), float(l[38:46]), float(l[46:54])] for l in m.split("\n") if l.startswith("ATOM") and l[12:16].strip() == "CA"])
              for m in txt.split("MODEL ")[1:]]
        assert len(ca) == 6 and all(np.abs(ca[i] - ca[j]).max() > 1e-2 for i in range(6) for j in range(i))


def test_cfg3_science2011_all_targets_vs_reference(tmp_path, monkeypatch):
    """BASELINE configs[2]: every one of the 12 Science2011 targets (10 ... 80 residues, all ragged for the 32-residue tiles) from its
    PDB file through the Hydra config, the datamodule / featuriser and ``predict_step`` (3 replicas, t_delta 0.5, 10 + 1
    evaluations) -- against the REFERENCE's run of the same target under the same seed (tests/golden/make_golden_configs.py --cfg3:
    the reference's own ProteinFeatureTransform + its predict_step control flow).  Device tensors at RMSD < 1e-4 A; the written
    multi-MODEL PDB text at its 3-decimal resolution."""
    import os

    from conftest import GOLDEN, ROOT
    from str2str_amd.synth import synth_state_dict
    from str2str_amd.utils import config as C

    g = golden("cfg3_science2011.npz")
    monkeypatch.setenv("TEST_DATA", os.path.join(GOLDEN, "pdb"))
    monkeypatch.setenv("CACHE_DIR", str(tmp_path / "cache"))
    monkeypatch.setenv("PROJECT_ROOT", str(tmp_path))
    args = ["task_name=inference", "ckpt_path=null", f"model.inference.n_replica={int(g['B'])}", "model.inference.replica_per_batch=8",
            f"model.inference.num_timesteps={int(g['num_timesteps'])}", f"model.inference.delta_min={float(g['t_delta'])}",
            f"model.inference.delta_max={float(g['t_delta'])}", "model.inference.delta_step=0.1", "extras.print_config=false"]
    cfg = C.compose(os.path.join(ROOT, "configs"), "eval.yaml", args)
    model = C.instantiate(cfg.model)
    man = [(k, tuple(v.shape)) for k, v in model.net.state_dict().items()]
    model.net.load_state_dict(synth_state_dict(man, seed=0, sigma_final=0.002))
    model = model.to(DEV).eval()
    batches = C.instantiate(cfg.data).test_dataloader()
    codes = sorted({k.split("/")[0] for k in g if "/" in k})
    assert len(batches) == len(codes) == 12
    seen = set()
    for batch in batches:
        code = batch["accession_code"][0]
        batch = {k: (v.to(DEV) if torch.is_tensor(v) and k != "residue_idx" else v) for k, v in batch.items()}
        torch.manual_seed(int(g[f"{code}/seed"]))
        all_dir = model.predict_step(batch, 0)
        got = model.last_samples[float(g["t_delta"])].cpu().numpy()[..., :5, :]
        want = g[f"{code}/atom37"]
        assert got.shape == want.shape, (code, got.shape, want.shape)
        check(f"cfg3 {code} (N = {want.shape[1]}): backbone RMSD vs the reference (A)", backbone_rmsd(got, want), 1e-4)
        txt = open(os.path.join(os.path.dirname(all_dir), f"{float(g['t_delta'])}", f"{code}.pdb")).read()
        assert txt.count("MODEL ") == int(g["B"])
        xyz = np.array([[float(l[30:38]), float(l[38:46]), float(l[46:54])] for l in txt.split("\n") if l.startswith("ATOM")])
        aat = batch["aatype"][0].cpu().numpy()
        keep = np.array([[not (a == 3 and aat[i] == 7) for a in range(5)] for i in range(want.shape[1])])   # GLY has no CB line
        assert np.abs(xyz - want[:, keep]. reshape(-1, 3)).max() < 1e-3, code
        seen.add(code)
    assert seen == set(codes)


def test_cfg5_padded_mixed_batch_vs_reference_per_chain(net_smooth, diffuser):
    """BASELINE configs[4]: chains of different length in ONE padded, masked batch -- each chain against the REFERENCE's own
    un-padded run of that chain alone (tests/golden/make_golden_configs.py --cfg5: lengths 12, 33 and 71 / 214 / 323 of the seed-5
    draw; 2 replicas, 4 + 1 evaluations, started from the reference's noised frames).  The reference cannot batch chains
    (diffusion_module.py:249); exact padding must make the batch equal to its per-chain runs, not just to our own."""
    from str2str_amd.sampler import plan_mixed_work, sample_mixed_lengths
    from str2str_amd.synth import synth_chain

    g = golden("cfg5_mixed_lengths.npz")
    lens = [int(x) for x in g["lens"]]
    R, S = int(g["R"]), int(g["num_timesteps"])
    targets = [synth_chain(n, frame_seed=3 + n, aatype_seed=4 + n) for n in lens]
    inits = [T(g[f"n{n}/first_rigids_t"]) for n in lens]
    plan = plan_mixed_work(lens, R, 1, launch_floor_ms=1e9)   # everything in one padded batch (n_pad = 323)
    assert len(plan[0]) == 1 and plan[0][0]["n_pad"] == max(lens)
    one = sample_mixed_lengths(net_smooth, diffuser, targets, R, float(g["t_delta"]), num_timesteps=S, device=DEV, rigids_t_init=inits, plan=plan)
    auto = sample_mixed_lengths(net_smooth, diffuser, targets, R, float(g["t_delta"]), num_timesteps=S, device=DEV, rigids_t_init=inits)
    for k, n in enumerate(lens):
        for name, res in (("one padded batch", one), ("planner's batches", auto)):
            got = torch.cat([p for _, p in res[k]]).cpu().numpy()[..., :5, :]
            check(f"cfg5 N={n} in {name}: backbone RMSD vs the reference's un-padded run (A)", backbone_rmsd(got, g[f"n{n}/atom37"]), 1e-4)


def test_mixed_length_padded_batch_equals_unpadded_runs(net_smooth, diffuser):
    """BASELINE configs[4] semantics: chains of different length in padded batches; every chain must equal its own un-padded
    single-chain run (same initial noised frames).  Lengths drawn like the cfg5 workload (U[64, 384], seed 5) plus two short
    ones, 2 replicas each, through the FLOP-weighted planner: as one process and as 2 'ranks' run back to back."""
    from str2str_amd.common.rigid_utils import Rigid
    from str2str_amd.sampler import denoise_loop, plan_mixed_work, sample_mixed_lengths, schedule
    from str2str_amd.synth import synth_chain

    lens = [12, 33] + [int(x) for x in np.random.default_rng(5).integers(64, 385, size=32)[:6]]
    R, S = 2, 4
    targets = [synth_chain(n, frame_seed=3 + n, aatype_seed=4 + n) for n in lens]
    torch.manual_seed(3)
    inits = []
    for tg in targets:
        rig0 = Rigid.from_tensor_4x4(tg["rigidgroups_gt_frames"][..., 0, :, :].repeat(R, 1, 1, 1))
        inits.append(diffuser.forward_marginal(rig0, 1.0 * torch.ones(R), tg["residue_mask"].repeat(R, 1))["rigids_t"])
    plan = plan_mixed_work(lens, R, 1, launch_floor_ms=1e9)   # force everything into as few padded batches as memory allows
    assert len(plan[0]) == 1 and plan[0][0]["n_pad"] == max(lens)
    mixed = sample_mixed_lengths(net_smooth, diffuser, targets, R, 1.0, num_timesteps=S, device=DEV, rigids_t_init=inits, plan=plan)
    halves = [sample_mixed_lengths(net_smooth, diffuser, targets, R, 1.0, num_timesteps=S, device=DEV, rigids_t_init=inits,
                                   shard=(r, 2)) for r in range(2)]
    T, n, dt, ts = schedule(1.0, S, 0.01)
    for k, (tg, init) in enumerate(zip(targets, inits)):
        f = {kk: tg[kk].to(DEV).repeat(R, *(1,) * (tg[kk].ndim - 1)) for kk in
             ("aatype", "residue_mask", "fixed_mask", "residue_idx", "torsion_angles_sin_cos")}
        f["residue_idx"] = tg["residue_idx"].repeat(R, 1)
        alone, _, _ = denoise_loop(net_smooth, diffuser, f, init.to(DEV).float().contiguous(), ts, dt, min_t=0.01)
        alone = alone.cpu().numpy()[..., :5, :]
        (lo, got), = mixed[k]
        assert lo == 0 and got.shape == (R, lens[k], 37, 3)
        check(f"mixed-length padded batch vs un-padded run, N={lens[k]} (RMSD, A)", backbone_rmsd(got.cpu().numpy()[..., :5, :], alone), 1.5e-5)
        parts = sorted(halves[0][k] + halves[1][k], key=lambda x: x[0])
        both = torch.cat([p for _, p in parts]).cpu().numpy()[..., :5, :]
        assert [lo for lo, _ in parts] == [0, 1] and both.shape[0] == R
        check(f"mixed-length 2-rank plan vs un-padded run, N={lens[k]} (RMSD, A)", backbone_rmsd(both, alone), 1.5e-5)


def _q_sign_free(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    dq = np.minimum(np.abs(a[..., :4] - b[..., :4]).max(-1), np.abs(a[..., :4] + b[..., :4]).max(-1))
    return float(max(dq.max(), np.abs(a[..., 4:] - b[..., 4:]).max()))


def test_forward_marginal_device_reproduces_reference_draws(diffuser):
    """the device forward marginal / prior (s2s_forward_marginal) is the reference's arithmetic
    (frame.py:36-107, :212-255) as a pure function of the noise: fed the draws the REFERENCE made for the committed fixture
    (same host generator state, same order: axis normals, inverse-CDF uniforms, translation normals) it returns the
    reference's frames."""
    from str2str_amd.common.rigid_utils import Rigid

    g = golden("forward_marginal.npz")
    gt4, mask = T(g["gt4"]), T(g["mask"])
    B, N = mask.shape
    torch.manual_seed(int(g["seed_fm"]))
    noise = (torch.randn(B, N, 3), torch.rand(B, N), torch.randn(B, N, 3))
    got = diffuser.forward_marginal_device(gt4.to(DEV), float(g["t_delta"]), mask.to(DEV), noise=noise)
    check("forward marginal (device) vs reference frames", _q_sign_free(got.cpu().numpy(), g["rigids_t"]), 2e-6)
    torch.manual_seed(int(g["seed_prior"]))
    noise = (torch.randn(B, N, 3), torch.rand(B, N), torch.randn(B, N, 3))
    got = diffuser.forward_marginal_device(None, None, shape=(B, N), noise=noise)
    check("prior sample (device) vs reference frames", _q_sign_free(got.cpu().numpy(), g["prior"]), 1.2e-6)
    # host path of this build on fresh draws == device path on the same draws (larger sample, all four t regimes)
    rig0 = Rigid.from_tensor_4x4(gt4[:1].repeat(64, 1, 1, 1))
    for td in (0.05, 0.35, 1.0):
        torch.manual_seed(5)
        host = diffuser.forward_marginal(rig0, td * torch.ones(64), torch.ones(64, N))["rigids_t"]
        torch.manual_seed(5)
        noise = (torch.randn(64, N, 3), torch.rand(64, N), torch.randn(64, N, 3))
        dev = diffuser.forward_marginal_device(rig0.to_tensor_4x4().to(DEV), td, noise=noise)
        check(f"forward marginal device vs host, t={td}", _q_sign_free(dev.cpu().numpy(), host.numpy()), 3e-6)


def test_forward_marginal_device_distribution(diffuser):
    """Throughput mode draws on the device generator (Philox): the rotation-angle and translation distributions must be the
    host sampler's (two-sample Kolmogorov-Smirnov, 20k draws each)."""
    from scipy.stats import ks_2samp

    from str2str_amd.common import rotation3d
    from str2str_amd.common.rigid_utils import Rigid

    B, N, td = 200, 100, 0.35
    eye = torch.eye(4)[None, None].repeat(B, N, 1, 1)
    torch.manual_seed(1)
    host = diffuser.forward_marginal(Rigid.from_tensor_4x4(eye), td * torch.ones(B), torch.ones(B, N))["rigids_t"]
    torch.cuda.manual_seed(2)
    dev = diffuser.forward_marginal_device(eye.to(DEV), td).cpu()

    def angle(r7):
        return rotation3d.quaternion_to_axis_angle(r7[..., :4]).norm(dim=-1).reshape(-1).numpy()

    ah, ad = np.minimum(angle(host), 2 * np.pi - angle(host)), np.minimum(angle(dev), 2 * np.pi - angle(dev))
    p_ang = ks_2samp(ah, ad).pvalue
    p_tr = ks_2samp(host[..., 4:].reshape(-1).numpy(), dev[..., 4:].reshape(-1).numpy()).pvalue
    record_margin("forward marginal device vs host: KS p-value rotation angle (must exceed 1e-3)", 1 - p_ang, 1 - 1e-3)
    assert p_ang > 1e-3 and p_tr > 1e-3, (p_ang, p_tr)
    # and a rank-seeded throughput-mode trajectory runs end to end with no host noise


def test_host_start_frames_thread_count_and_draw_skipping_change_nothing(net_smooth, diffuser, monkeypatch):
    """Parity mode's host-side shortcuts: start frames assembled on one intra-op thread (S2S_HOST_FM_THREADS) and the ODE's unused
    step draws skipped by fast-forwarding the generator (S2S_HOST_RNG_FAST) -- same samples bit for bit, same generator state
    afterwards, torch's thread count left as it was."""
    from str2str_amd.common.rigid_utils import Rigid
    from str2str_amd.sampler import forward_backward
    from str2str_amd.synth import synth_chain

    feats = synth_chain(24)
    rig0 = Rigid.from_tensor_4x4(feats["rigidgroups_gt_frames"][..., 0, :, :].repeat(5, 1, 1, 1))
    keep, outs, states = torch.get_num_threads(), [], []
    for fm, fast in (("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")):
        monkeypatch.setenv("S2S_HOST_FM_THREADS", fm)
        monkeypatch.setenv("S2S_HOST_RNG_FAST", fast)
        torch.manual_seed(21)
        outs.append(forward_backward(net_smooth, diffuser, feats, rig0, 0.6, num_timesteps=10, device=DEV).cpu())
        states.append(torch.get_rng_state())
        assert torch.get_num_threads() == keep
    assert all(torch.equal(outs[0], o) for o in outs[1:]) and all(torch.equal(states[0], st) for st in states[1:])


def test_empty_replica_slice_keeps_host_generator_in_lockstep(net_smooth, diffuser):
    """A rank whose slice of a chunk is empty (more ranks than replicas, remainder chunks) must consume the chunk's host draws
    exactly like a rank that samples it, or every later chunk / t_delta / target would see a different noise stream."""
    from str2str_amd.common.rigid_utils import Rigid
    from str2str_amd.sampler import forward_backward
    from str2str_amd.synth import synth_chain

    feats = synth_chain(10)
    rig0 = Rigid.from_tensor_4x4(feats["rigidgroups_gt_frames"][..., 0, :, :].repeat(3, 1, 1, 1))
    states = []
    for sl in ((0, 3), (0, 0), (1, 2)):
        for pf in (True, False):
            torch.manual_seed(9)
            out = forward_backward(net_smooth, diffuser, feats, rig0, 0.5, num_timesteps=8, device=DEV, replica_slice=sl,
                                   probability_flow=pf)
            assert out.shape[0] == sl[1] - sl[0]
            states.append(torch.get_rng_state())
    assert all(torch.equal(states[0], s) for s in states[1:])


def test_throughput_mode_runs_without_host_noise(net_smooth, diffuser):
    """rng='device': forward marginal and step noise on the device generator; finite, replica-distinct, seed-reproducible."""
    from str2str_amd.common.rigid_utils import Rigid
    from str2str_amd.sampler import forward_backward
    from str2str_amd.synth import synth_chain

    feats = synth_chain(16)
    rig0 = Rigid.from_tensor_4x4(feats["rigidgroups_gt_frames"][..., 0, :, :].repeat(4, 1, 1, 1))
    outs = []
    for pf in (True, False):
        for rep in range(2):
            torch.cuda.manual_seed(77)
            host_state = torch.get_rng_state()
            outs.append(forward_backward(net_smooth, diffuser, feats, rig0, 0.7, num_timesteps=6, device=DEV, rng="device",
                                         probability_flow=pf).cpu())
            assert torch.equal(host_state, torch.get_rng_state())   # the host generator is not touched
        assert torch.isfinite(outs[-1]).all() and torch.equal(outs[-1], outs[-2])
        assert float((outs[-1][0] - outs[-1][1]).abs().max()) > 1e-2
    prior = forward_backward(net_smooth, diffuser, feats, rig0, -1.0, num_timesteps=6, device=DEV, rng="device")
    assert torch.isfinite(prior).all()


@pytest.mark.parametrize("M,K,N", [(70, 256, 256), (128, 320, 960), (33, 2688, 256), (257, 256, 192), (64, 128, 768), (40, 256, 6)])
def test_node_linear_vs_float64(M, K, N):
    """s2s_node_linear (split-f16 MFMA, packed-plane activations) and s2s_node_linear_f32 (exact fp32 MFMA, fp32 activations: the
    range-safe arithmetic) against a float64 evaluation of LayerNorm(residual + mask * relu(scale * x W^T + b)) * mask -- every
    epilogue stage on -- for the trunk's layer shapes (ragged row counts, K = 2688 of linear_out, a 6-wide head padded to 32); the
    packed-plane output decodes to the fp32 output to the last bit or two (x_h + x_l: 22 bits + the residue's sign)."""
    from str2str_amd import ops

    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    n_pad = -(-N // 32) * 32
    whole = n_pad // 32 in ops.NODE_TG
    tg = ops.node_tiles(n_pad, whole_row=whole)
    wpk = ops.pack_node_weight(w, tg)
    bias = torch.zeros(n_pad, device=DEV); bias[:N] = b
    xp = ops.pack_planes(x)
    def planes_ok(xp_, ref_, k_):   # |x - (x_h + x_l)| <= 2^-24 |x| (+ f16's subnormal quantum for the residue of small values)
        return bool(((ops.unpack_planes(xp_, M, k_) - ref_).abs() <= 2.0 ** -23 * ref_.abs() + 2.0 ** -24).all())

    assert planes_ok(xp, x, K)
    y, yxp = ops.node_linear(xp, wpk, bias, M, K, n_pad, tg, want_xp=True)
    ref = (x.double() @ w.double().t() + b.double())
    check(f"node_linear plain M{M} K{K} N{N}", rel(y[:, :N], ref), 2e-6)
    assert float(y[:, N:].abs().max()) == 0 if n_pad > N else True
    assert planes_ok(yxp, y, n_pad)
    layer = ops.pack_node_layer(w, b, whole)
    assert layer["tg"] == tg and torch.equal(layer["w"], wpk)
    y32, y32b = ops.node_apply(x, layer, M)                       # fp32 input -> the exact fp32-MFMA kernel
    assert y32 is y32b and y32.shape == (M, n_pad)
    check(f"node_linear_f32 plain M{M} K{K} N{N}", rel(y32[:, :N], ref), 2e-6)
    if whole:
        scale = (torch.rand(M, generator=g) + 0.5).to(DEV)
        mask = (torch.rand(M, generator=g) > 0.3).float().to(DEV)
        res = torch.randn(M, n_pad + 32, generator=g).to(DEV)    # wider leading dimension on purpose
        ga, be = (1 + 0.1 * torch.randn(n_pad, generator=g)).to(DEV), (0.1 * torch.randn(n_pad, generator=g)).to(DEV)
        out = torch.full((M, n_pad + 64), -7.0, device=DEV)
        y, yxp = ops.node_linear(xp, wpk, bias, M, K, n_pad, tg, pre_scale=scale, relu=True, pre_mask=mask, residual=res,
                                 ln=(ga, be, 1e-5), post_mask=mask, out_f32=out, out_col0=32, want_xp=True, out_xp_k=n_pad + 64,
                                 out_xp_k0=64)
        wz = torch.zeros(n_pad, K, device=DEV, dtype=torch.float64); wz[:N] = w.double()
        v = torch.relu((x.double() * scale.double()[:, None]) @ wz.t() + bias.double()) * mask.double()[:, None] + res[:, :n_pad].double()
        ref = F.layer_norm(v, (n_pad,), ga.double(), be.double(), 1e-5) * mask.double()[:, None]
        check(f"node_linear fused epilogue M{M} K{K} N{N}", rel(out[:, 32:32 + n_pad], ref), 5e-6)
        assert float((out[:, :32] + 7).abs().max()) == 0 and float((out[:, 32 + n_pad:] + 7).abs().max()) == 0
        out32 = torch.full((M, n_pad + 64), -7.0, device=DEV)
        ops.node_apply(x, layer, M, pre_scale=scale, relu=True, pre_mask=mask, residual=res, ln=(ga, be, 1e-5), post_mask=mask,
                       out_f32=out32, out_col0=32)
        check(f"node_linear_f32 fused epilogue M{M} K{K} N{N}", rel(out32[:, 32:32 + n_pad], ref), 5e-6)
        assert float((out32[:, :32] + 7).abs().max()) == 0 and float((out32[:, 32 + n_pad:] + 7).abs().max()) == 0


@pytest.mark.parametrize("M", [256, 77])
def test_node_linear_vfrag_equals_plain_output(M):
    """The operand-swapped GEMM (s2s_node_linear_vfrag: result stored as f16 pair A fragments over 32-row tiles, the value operand
    of the IPA's PV product) decodes to the plain s2s_node_linear output: same products, same accumulation order per element
    up to the MFMA's internal order -> compared against float64 like the plain kernel, and the split itself is exact."""
    from str2str_amd import ops

    K, N, tph = 256, 2048, 8
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, K, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    wpk = ops.pack_node_weight(w, 8)
    xp = ops.pack_planes(x)
    vf = ops.node_linear_vfrag(xp, wpk, b, M, K, N, tph)
    RT = (M + 31) // 32
    fr = vf.view(torch.float16).reshape(RT, N // 32 // tph, tph, 2, 2, 2, 32, 8).float().sum(4)   # [RT, H, ct, u, h, c, j]
    u = torch.arange(2)[:, None, None]; h = torch.arange(2)[None, :, None]; j = torch.arange(8)[None, None, :]
    r = 8 * u + j
    row = ((r & 3) + 8 * (r >> 2) + 4 * h).to(DEV)                                                  # [u, h, j]
    y = torch.zeros(RT, 32, N, device=DEV)
    cols = fr.permute(0, 3, 4, 6, 1, 2, 5).reshape(RT, 2, 2, 8, N)                                  # [RT, u, h, j, col]
    y[:, row.reshape(-1)] = cols.reshape(RT, 32, N)
    y = y.reshape(-1, N)
    ref = x.double() @ w.double().t() + b.double()
    check(f"node_linear_vfrag M{M}", rel(y[:M], ref), 2e-6)
    assert float(y[M:].abs().max()) == 0 if RT * 32 > M else True
    y_plain, _ = ops.node_linear(xp, wpk, b, M, K, N, 8)
    check(f"node_linear_vfrag vs plain M{M}", rel(y[:M], y_plain.double()), 1e-6)


@pytest.mark.parametrize("arith", MODES)
@pytest.mark.parametrize("B,N", [(2, 37), (1, 256), (3, 130)])
def test_encoder_attention_vs_torch(net_rough, B, N, arith):
    """s2s_encoder_attention (exact fp32 MFMA) and s2s_encoder_attention_f16x3 (split-f16 MFMA, the default) against torch's own nn.TransformerEncoder (the module the reference calls, ipa.py:357) in float64
    on the same parameters: full 2-layer encoder through the fused node kernels (in_proj -> attention -> out_proj + LN ->
    feed-forward + LN) with a partial FLOAT key-padding mask (added to the logits), and the exact-padding variant (-inf)."""
    import copy

    from str2str_amd import ops

    tr = net_rough.translator
    enc = tr.trunk["transformer_1"]
    W = tr._node_weights()[1]["layers"]
    g = torch.Generator().manual_seed(B * 1000 + N)
    x = torch.randn(B, N, 320, generator=g).to(DEV)
    mask = torch.ones(B, N); mask[-1, -5:] = 0
    pad = (1.0 - mask).to(DEV)
    ref_enc = copy.deepcopy(enc).double()
    M = B * N

    def run(key_bias):
        xf = x.reshape(M, 320).contiguous()
        xx = ops.pack_planes(xf)
        for layer, lw in zip(enc.layers, W):
            lin = lambda xp, w, **kw: ops.node_apply(xp, w, M, **kw)  # noqa: E731
            qkv, _ = lin(xx, lw["in"])
            sa32, sa_xp = ops.encoder_attention(qkv, key_bias, B, N, 4, want_f32=True, arith=arith)
            assert bool(((ops.unpack_planes(sa_xp, M, 320) - sa32).abs() <= 2.0 ** -23 * sa32.abs() + 2.0 ** -24).all())
            x1, x1x = lin(sa_xp, lw["o"], residual=xf, ln=(layer.norm1.weight, layer.norm1.bias, layer.norm1.eps), want_xp=True)
            _, hx = lin(x1x, lw["l1"], relu=True, want_f32=False, want_xp=True)
            xf, xx = lin(hx, lw["l2"], residual=x1, ln=(layer.norm2.weight, layer.norm2.bias, layer.norm2.eps), want_xp=True)
        return xf.view(B, N, 320)

    # float mask: added to the logits (what the reference's call does with src_key_padding_mask = 1 - mask)
    ref = ref_enc(x.double().transpose(0, 1), src_key_padding_mask=pad.double()).transpose(0, 1)
    check(f"encoder (float mask) B{B} N{N} {arith}", rel(run(pad.contiguous()), ref), 2e-6)
    # exact padding: padded keys removed (bool mask in torch)
    ref = ref_enc(x.double().transpose(0, 1), src_key_padding_mask=pad.bool()).transpose(0, 1)
    got = run(torch.where(pad > 0, float("-inf"), 0.0).contiguous())
    valid = mask.bool().numpy()
    check(f"encoder (exact padding) B{B} N{N} {arith}", rel(got.cpu().numpy()[valid], ref.cpu().numpy()[valid]), 2e-6)


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_ensemble_metrics_match_reference(tag):
    """validity / bonding validity / js_pwd / js_rg on the device against the values the REFERENCE's
    src/metrics/metrics.py returned for the same float32 CA ensembles (tests/golden/make_golden_metrics.py; case c has a
    single-structure target: numpy's degenerate-range rule).  The per-channel js_pwd values are checked un-rounded: the
    histogram counts must be numpy's."""
    from str2str_amd import ops
    from str2str_amd.metrics import metrics as M

    g = golden("metrics.npz")
    d = {"target": g[f"{tag}_target"], "pred": g[f"{tag}_pred"]}
    v, b = M.validity(d), M.bonding_validity(d)
    assert [v["target"], v["pred"]] == list(g[f"{tag}_validity"]) and [b["target"], b["pred"]] == list(g[f"{tag}_bonding"])
    ch = ops.ca_pwd_js(torch.as_tensor(d["target"]).to(DEV), torch.as_tensor(d["pred"]).to(DEV)).cpu().numpy()
    check(f"js_pwd per-channel vs reference [{tag}]", float(np.abs(ch - g[f"{tag}_js_pwd_channels"]).max()), 1e-12)
    assert M.js_pwd(d)["pred"] == float(g[f"{tag}_js_pwd"]) and M.js_pwd(d)["target"] == 0.0
    check(f"radius of gyration vs reference [{tag}]", float(np.abs(M.radius_of_gyration(d["pred"]) - g[f"{tag}_rg_pred"]).max()), 1.5e-6)
    check(f"js_rg vs reference [{tag}]", abs(M.js_rg(d)["pred"] - float(g[f"{tag}_js_rg"])), 2.1e-3)


@pytest.mark.parametrize("B,N", [(2, 64), (3, 37), (1, 300)])
def test_ipa_shared_kv_operands_are_the_planes_of_s(B, N):
    """Folded projections (models/net/ipa.py _folded_packs): s2s_ipa_prep_points_f16 with s_xp emits the K / V operands every head
    shares.  They are the f16 planes of s MOVED (exact): v_shared decodes -- through the decoder of the A-fragment layout used for
    s2s_node_linear_vfrag -- to s in the padded per-sample rows (a padded row repeats the sample's last row), k_shared (ragged
    lengths only) to the same rows as packed planes, bit for bit."""
    from str2str_amd import ops

    H, M, NP = 8, B * N, ops.padded_len(N)
    g = torch.Generator().manual_seed(5 + N)
    s = (torch.randn(M, 256, generator=g) * 3).to(DEV)
    q4 = torch.randn(B, N, 4, generator=g)
    r7 = torch.cat([q4 / q4.norm(dim=-1, keepdim=True), torch.randn(B, N, 3, generator=g)], -1).contiguous().to(DEV)
    qp, kvp = torch.randn(M, 192, generator=g).to(DEV), torch.randn(M, 480, generator=g).to(DEV)
    hw = torch.rand(H, generator=g).to(DEV)
    s_xp = ops.pack_planes(s)
    base = ops.ipa_prep_points_f16(r7, qp, kvp, hw)
    *pts, k_sh, v_sh = torch.ops.str2str_amd.ipa_prep_points_shared_kv(r7, qp, kvp, hw, s_xp)
    for a, b in zip(base, pts):
        assert torch.equal(a, b)                                     # the point operands do not change
    rows = (torch.arange(B)[:, None] * N + torch.arange(NP).clamp(max=N - 1)[None, :]).reshape(-1).to(DEV)
    planes = s_xp.view(torch.float16).reshape(-1, 16, 2, 2, 32, 8)   # [RT, ks, plane, g, m, j]
    ks = torch.arange(16)[:, None, None]; gg = torch.arange(2)[None, :, None]; j = torch.arange(8)[None, None, :]
    r = 8 * (ks & 1) + j
    chan = (32 * (ks >> 1) + (r & 3) + 8 * (r >> 2) + 4 * gg).reshape(-1).to(DEV)
    want = []
    for p in range(2):                                               # plane p of s as [rows, 256] f16, then the padded rows
        x = torch.zeros(planes.shape[0], 32, 256, dtype=torch.float16, device=DEV)
        x[:, :, chan] = planes[:, :, p].permute(0, 3, 1, 2, 4).reshape(planes.shape[0], 32, -1)
        want.append(x.reshape(-1, 256)[rows])
    RT = B * NP // 32
    fr = v_sh.view(torch.float16).reshape(RT, 8, 2, 2, 2, 32, 8)      # [RT, ct, u, plane, h, c, j]
    u = torch.arange(2)[:, None, None]; h = torch.arange(2)[None, :, None]
    rr = 8 * u + j
    row = ((rr & 3) + 8 * (rr >> 2) + 4 * h).reshape(-1).to(DEV)
    for p in range(2):
        y = torch.zeros(RT, 32, 256, dtype=torch.float16, device=DEV)
        y[:, row] = fr[:, :, :, p].permute(0, 2, 3, 5, 1, 4).reshape(RT, 32, 256)   # [RT, (u h j), (ct c)]
        assert torch.equal(y.reshape(-1, 256), want[p]), f"v_shared plane {p}"
    if N % 32 == 0:
        assert k_sh is None                                          # s_xp itself is the K operand
    else:
        kp = k_sh.view(torch.float16).reshape(RT, 16, 2, 2, 32, 8)
        for p in range(2):
            x = torch.zeros(RT, 32, 256, dtype=torch.float16, device=DEV)
            x[:, :, chan] = kp[:, :, p].permute(0, 3, 1, 2, 4).reshape(RT, 32, -1)
            assert torch.equal(x.reshape(-1, 256), want[p]), f"k_shared plane {p}"


@pytest.mark.parametrize("B,N", [(2, 64), (3, 37), (1, 256)])
def test_ipa_folded_projections_equal_the_per_head_path(B, N):
    """The default f16 path reads s as the K and V operand of every head, with W_k folded into q' = (W_k^T W_q) s + W_k^T b_q and
    W_v / b_v into linear_out (reference grouping: ipa.py:131-143,183-190,229-252,259-266).  The block's output equals the
    per-head path's (same kernels, reference grouping) and the exact fp32 path's to fp32 rounding -- also with masked residues."""
    from str2str_amd import ops
    from str2str_amd.models.net.ipa import InvariantPointAttention

    torch.manual_seed(3)
    ipa = InvariantPointAttention(256, 128, 256, 8, 8, 12).to(DEV)
    with torch.no_grad():
        for p in ipa.parameters():
            p.copy_(torch.randn_like(p) * 0.08)
    H, M = 8, B * N
    g = torch.Generator().manual_seed(17 + N)
    s = torch.randn(M, 256, generator=g).to(DEV)
    q4 = torch.randn(B, N, 4, generator=g)
    r7 = torch.cat([q4 / q4.norm(dim=-1, keepdim=True), torch.randn(B, N, 3, generator=g)], -1).contiguous().to(DEV)
    bias, pz = torch.randn(B, H, N, N, generator=g).to(DEV), torch.randn(B, N, N, 32, generator=g).to(DEV)
    mask = torch.ones(B, N)
    mask[-1, -3:] = 0
    mask = mask.to(DEV)
    s = s * mask.reshape(-1, 1)                                      # (the trunk hands masked activations to the block)
    s_xp = ops.pack_planes(s)

    def block(act):
        feats = ipa.attention(act, B, N, r7, mask, (bias.clone(), pz))
        return ops.node_apply(feats, ipa.out_pack(feats), M)[0].double()

    with torch.no_grad():
        ipa.arith = "f32"
        ref = block(s)
        ipa.arith, ipa.fold = "f16x3", True
        assert ipa.folded
        out_f = block(s_xp)
        ipa.fold = False
        out_h = block(s_xp)
    valid = mask.reshape(-1).bool()
    check(f"IPA block B{B} N{N}: folded projections vs exact fp32 path", rel(out_f[valid], ref[valid]), 5e-6)
    check(f"IPA block B{B} N{N}: per-head projections vs exact fp32 path", rel(out_h[valid], ref[valid]), 5e-6)
    check(f"IPA block B{B} N{N}: folded vs per-head projections", rel(out_f[valid], out_h[valid]), 5e-6)
