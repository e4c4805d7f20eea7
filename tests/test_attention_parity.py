"""The attention cores on the HIP kernels against the float64 statement of their formulas (tests/ref_attention.py), section by
section of linear_out's input, at the inputs of tests/attention_cases.py: a flat and a PEAKED softmax (rows whose logits span
more than float32's exp range, the maximum arriving in every key tile), frames at the origin and 100 A away from it, a mask of
another kind on every sample (gaps, prefixes, a whole key tile, a whole sample), every length at which the kernels take another
path, and batches with more work items than persistent workgroups.

  InvariantPointAttention.attention   folded f16 (s2s_ipa_attention_short<1|2> up to 64 residues, s2s_ipa_attention_f16w beyond),
                                      per-head f16 (fold = False: the streaming kernel at every length, its NT < 3 branch included),
                                      arith "f32" (s2s_ipa_attention); each with s2s_ipa_opair and the point preparation kernels
  ops.ipa_attention_f16               logits in place and not: bit-identical features
  ops.encoder_attention               both arithmetics, want_f32 and the packed planes

Measure: max |got - float64| / max(1, max |float64| of the section) over every VALID query row.  Masked query rows must be finite
and are otherwise left out (the formula adds -1e5 to their logits, which quantises them to 2^-7 in float32; the trunk multiplies
those rows by the mask) -- the only exclusion.  Bound: attention_cases.bound, 3 x the float32 chain's own distance from float64
pooled over the family, flat families never above 5e-6; it is computed from ref_attention alone.  On an MI355X the kernels use
0.15 to 0.88 of it (profiles/parity_margins.json; closest: the fp32 kernel's o_pt with moved frames, 4.4e-6 of 5e-6, and o_pair on
the flat family, 1.4e-6 of 1.8e-6).
"""
import pytest
import torch

import attention_cases as AC
import ref_attention as RA
from conftest import record_margin, synth_sd

pytestmark = pytest.mark.gpu

DEV = "cuda"
BLOCK = "ipa_2"
PATHS = {"folded": ("f16x3", True, ("as", "o_pt", "o_norm", "o_pair")),
         "per-head": ("f16x3", False, ("o", "o_pt", "o_norm", "o_pair")),
         "f32": ("f32", True, ("o", "o_pt", "o_norm", "o_pair"))}
WIDTH = {"o": 2048, "as": 2048, "o_pt": 288, "o_norm": 96, "o_pair": 256}


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module")
def net():
    from str2str_amd.factory import build_synthetic_net

    return build_synthetic_net(seed=0, sigma_final=0.02, device=DEV)


@pytest.fixture(scope="module")
def weights():
    return RA.ipa_weights(synth_sd(0, 0.02), f"translator.trunk.{BLOCK}.")


def split_sections(feats, names):
    out, c0 = {}, 0
    for n in names:
        out[n] = feats[..., c0:c0 + WIDTH[n]]
        c0 += WIDTH[n]
    assert c0 == feats.shape[-1]
    return out


def run_block(net, path, c):
    """ipa.attention on case ``c`` through ``path`` -> {section: [B, N, cols] fp32}."""
    from str2str_amd import ops

    arith, fold, names = PATHS[path]
    ipa = net.translator.trunk[BLOCK]
    B, N = c["B"], c["N"]
    M = B * N
    s = c["s"].reshape(M, -1).contiguous().to(DEV)
    keep = ipa.arith, ipa.fold
    try:
        ipa.arith, ipa.fold = arith, fold
        ops.range_flag_reset()
        act = ops.to_act(s, arith)
        assert ipa.use_f16(N, M) == (arith == "f16x3") and (ipa.folded or path != "folded")
        feats = ipa.attention(act, B, N, c["r7"].to(DEV), c["mask"].to(DEV), (c["bias"].clone().to(DEV), c["pz"].to(DEV)))
        if feats.dtype == torch.int16:
            feats = ops.unpack_planes(feats, M, 2688)
        assert ops.range_flag_read() == 0, ("the case left the f16 range", ops.range_flag_names(ops.range_flag_read()))
    finally:
        ipa.arith, ipa.fold = keep
    return split_sections(feats.view(B, N, -1), names)


def compare(weights, path, c, got, ref, label=None):
    """Every section of ``got`` against float64 under the family's bound; prints every figure, then asserts."""
    label = label or c["name"]
    failures = []
    for name, g in got.items():
        assert g.shape == ref[name].shape, (label, name, g.shape, ref[name].shape)
        assert bool(torch.isfinite(g).all()), (label, path, name, "not finite (masked query rows must be finite too)")
        err = AC.section_error(g, ref[name], c["mask"])
        if err != err:          # no valid row in the whole batch: the finiteness check is all there is
            continue
        b = AC.bound(weights, c["family"], name)
        record_margin(f"attention {path} vs float64: {c['family']} {name}", err, b)
        print(f"{label} {path} {name}: {err:.3e} (bound {b:.3e})")
        if not err < b:
            d = (g.cpu().double() - ref[name]).abs() * c["mask"][..., None]
            w = tuple(int(v) for v in (d == d.max()).nonzero()[0])
            failures.append(f"{name}: {err:.3e} >= {b:.3e}, worst at (b, i, col) = {w}, mask kind {c['kinds'][w[0]]}")
    assert not failures, (label, path, failures)


# ------------------------------------------------------------------------------------------------ the block, three paths
@pytest.mark.parametrize("N", AC.LENGTHS)
@pytest.mark.parametrize("family", AC.FAMILIES)
@pytest.mark.parametrize("path", list(PATHS))
def test_ipa_vs_float64(net, weights, path, family, N):
    c = AC.case(family, N)
    compare(weights, path, c, run_block(net, path, c), AC.features64(weights, c))


def _cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _workgroups(cu):
    return cu // 8 * 8 if cu >= 8 else cu      # s2s_ipa_attention_f16w: one persistent workgroup per CU, a multiple of 8


@pytest.mark.parametrize("family", ["flat", "peaked"])
@pytest.mark.parametrize("path,N,per", [("per-head", 32, 8), ("folded", 96, 8), ("folded", 129, 16)],
                         ids=["per-head-n32", "folded-n96", "folded-ragged-n129-xcd-remap"])
def test_ipa_more_items_than_workgroups(net, weights, path, N, per, family):
    """B = CUs / 8 + 1 samples (8 heads x 1 query block each) or CUs / 16 + 1 (x 2 query blocks, ragged: the XCD remap is on):
    some workgroup runs a second work item behind its first -- the image stream across items, the prefetched scalars and query
    fragments of the next item -- on samples that all differ in data and mask."""
    cu = _cu()
    B = cu // per + 1
    n_qb = (N + 127) // 128
    items = B * 8 * n_qb
    assert items > _workgroups(cu) and items > cu, (items, cu)
    if n_qb > 1:
        assert items % 8 == 0 and _workgroups(cu) % 8 == 0     # (the launcher's condition for the remap)
    c = AC.many_items_case(family, N, B)
    assert len(set(c["kinds"])) == min(B, len(AC.MASK_KINDS))
    compare(weights, path, c, run_block(net, path, c), AC.features64(weights, c, many=True))


# ------------------------------------------------------------------------------------------------ ops level: logits in place
def test_ops_ipa_attention_f16_logits_in_place_or_not(net, weights):
    """ops.ipa_attention_f16 on per-head operands at (3, 96), peaked: with the masked logits written over the bias
    (what the block does) and into a buffer of their own -- the features are the same bits, the bias is untouched unless asked, and
    they meet float64."""
    from str2str_amd import ops

    c = AC.case("peaked", 96)
    B, N = c["B"], c["N"]
    M = B * N
    ipa = net.translator.trunk[BLOCK]
    w, d = ipa.node_packs(), ipa._derived()
    s_xp = ops.pack_planes(c["s"].reshape(M, -1).contiguous().to(DEV))
    r7, mask, pz = c["r7"].to(DEV), c["mask"].to(DEV), c["pz"].to(DEV)
    lin = lambda x, **kw: ops.node_apply(s_xp, x, M, **kw)  # noqa: E731
    _, q_xp = lin(w["q"], want_f32=False, want_xp=True)
    _, k_xp = lin(w["k"], want_f32=False, want_xp=True)
    v_vf = ops.node_linear_vfrag(s_xp, w["v"]["w"], w["v"]["b"], M, 256, 2048, 8)
    qp, _ = lin(w["qp"])
    kvp, _ = lin(w["kvp"])
    pts = ops.ipa_prep_points_f16(r7, qp, kvp, d["hw"])
    out = []
    for inplace in (False, True):
        bias = c["bias"].clone().to(DEV)
        feats, fxp = ops.ipa_attention_f16(q_xp, k_xp, v_vf, pts, bias, pz, mask, r7, logits_inplace=inplace)
        assert torch.equal(bias.cpu(), c["bias"]) != inplace
        got = ops.unpack_planes(fxp, M, 2688)
        got[:, 2048:] = feats.view(M, -1)[:, 2048:]
        out.append(got)
    assert torch.equal(out[0], out[1])
    compare(weights, "per-head", c, split_sections(out[0].view(B, N, -1), PATHS["per-head"][2]), AC.features64(weights, c),
            label="ops.ipa_attention_f16 " + c["name"])


# ------------------------------------------------------------------------------------------------ the encoder's attention
@pytest.mark.parametrize("N", AC.ENC_LENGTHS)
@pytest.mark.parametrize("family", AC.ENC_FAMILIES)
@pytest.mark.parametrize("arith", ["f16x3", "f32"])
def test_encoder_attention_vs_float64(arith, family, N):
    """ops.encoder_attention(want_f32=True) against softmax(q k^T / sqrt(dh) + key_bias) v in float64 with every key_bias variant
    (none, float padding, -inf prefixes that leave whole trailing tiles masked, -inf on the whole first key tile); the packed planes
    of the same call decode to the fp32 output within the planes' rounding."""
    from str2str_amd import ops

    b = AC.encoder_bound(family)
    failures = []
    for kind in AC.ENC_BIAS:
        c = AC.encoder_case(family, N, kind)
        M = c["B"] * N
        ops.range_flag_reset()
        kb = None if c["key_bias"] is None else c["key_bias"].contiguous().to(DEV)
        out, oxp = ops.encoder_attention(c["qkv"].to(DEV), kb, c["B"], N, AC.ENC_HEADS, want_f32=True, arith=arith)
        assert ops.range_flag_read() == 0
        assert bool(torch.isfinite(out).all()), (c["name"], arith, "not finite")
        assert bool(((ops.unpack_planes(oxp, M, AC.ENC_D) - out).abs() <= 2.0 ** -23 * out.abs() + 2.0 ** -24).all()), (c["name"], "planes")
        err = AC.encoder_error(out, AC.encoder_ref(family, N, kind, torch.float64)[0])
        record_margin(f"encoder attention {arith} vs float64: {family}", err, b)
        print(f"{c['name']} {arith}: {err:.3e} (bound {b:.3e})")
        if not err < b:
            failures.append(f"{kind}: {err:.3e} >= {b:.3e}")
    assert not failures, (family, N, arith, failures)
