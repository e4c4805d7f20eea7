"""The node stream on the HIP kernels (csrc/node_gemm.hip behind str2str_amd/ops/node.py) against the float64 statement of its
formulas (tests/ref_node.py, evaluated with torch on the device), at the cases of tests/node_cases.py: row counts around one
32-row tile and one 128-row workgroup and a ragged last tile, and the families flat, trained-like (x 150), offset (LayerNorm rows
c_row + N(0, 1), |c_row| up to 30), small (row r at scale 2^-(r mod 16), weights x 1, 2^-6, 2^-10) and masked.

  single layers     s2s_node_linear with the wide and the narrow ("w_s") column blocks, ops.node_apply (linear_out: the narrow GEMM
                    + s2s_row_layernorm split up to SMALL_ROWS, the fused layer beyond; the packing switch at NARROW_MAX_WORK),
                    s2s_node_linear_f32, s2s_row_layernorm alone, s2s_node_linear_vfrag with and without a row map
  outputs           fp32, planes (decode to the fp32 output within the pair format's error), sentinel-filled wider buffers, padding
                    columns exactly zero, padded row-map rows equal to the sample's last row
  s2s_node_linear_multi   2, 4 and 6 problems: the trunk's launches (four skip_embeds; backbone update + EdgeTransition parts; backbone
                    update + torsion head's first layer), every problem against float64
  s2s_node_chain    2, 3 and 4 layers of widths 256 and 320, the 320 -> 256 first layer with its aliased residual, mid_ln, and
                    node_apply_chain where its policy picks the one-launch form for width 320
  one trunk block   the ops calls of TranslationIPA.forward in its order on given attention outputs, B N = 2 x 37, gapped and partly
                    fixed masks: every stage output, upd, A | 32 B | 32 G against the unfolded formula, psi

Measure and bound: node_cases (per row, no floor; 3 x D32 + F, F = the f16 pair format's a-priori floor, zero for arith "f32").
The small family is asserted with F in the bound: it holds only if conversions and MFMA keep f16 subnormals in these kernels.
Every figure is printed before it is asserted and recorded (profiles/parity_margins.json).
On an MI355X the kernels use up to 0.86 of the bound (closest: the fp32 kernel's linear_out on the offset family, 4.3e-6 of 5e-6;
with the LayerNorm's mean left as the plain first sum the offset family stood at 5.0e-6 .. 5.4e-6 in both arithmetics).
"""
import pytest
import torch

import node_cases as NC
import ref_node as RN
from conftest import record_margin, synth_sd

pytestmark = pytest.mark.gpu

DEV = "cuda"
ARITHS = ("f16x3", "f32")
T = RN.TRUNK


@pytest.fixture(autouse=True)
def _no_grad():
    from str2str_amd import ops

    with torch.no_grad():
        ops.range_flag_reset()
        yield
        assert ops.range_flag_read() == 0, ("a case left the f16 range", ops.range_flag_names(ops.range_flag_read()))


@pytest.fixture(scope="module")
def net():
    from str2str_amd.factory import build_synthetic_net

    return build_synthetic_net(seed=0, sigma_final=0.02, device=DEV)


def dev(t):
    if isinstance(t, tuple):
        return tuple(dev(v) for v in t)
    return t.to(DEV).contiguous() if torch.is_tensor(t) else t


def epilogue_of(kw):
    return {k: kw[k] for k in ("pre_scale", "relu", "pre_mask", "residual", "ln", "post_mask") if kw.get(k) is not None and kw.get(k) is not False}


_PACKS = {}


def packed(key, w, b, whole):
    from str2str_amd import ops

    if key not in _PACKS:
        _PACKS[key] = ops.pack_node_layer(dev(w), None if b is None else dev(b), whole)
    return _PACKS[key]


def judge(label, family, arith, got, rec, d32, floor, fails, margin=None):
    """``got`` [M, >= n] against a float64 record: prints and records the figure, checks the exact rows and the padding columns,
    appends a line to ``fails`` when the bound is missed."""
    n = rec["out"].shape[1]
    assert bool(torch.isfinite(got).all()), (label, "not finite")
    if got.shape[1] > n:
        assert float(got[:, n:].abs().max()) == 0, (label, "padding columns of a narrow head must be exactly zero")
    g = got[:, :n]
    a, b, r = NC.check_rows(g, rec, d32, floor if arith == "f16x3" else None, NC.capped(family))
    record_margin(margin or label, a, b)
    record_margin((margin or label) + " [achieved / bound]", a / b, 1.0)    # (the closest case of the label, whatever its bound)
    print(f"{label}: {a:.3e} (bound {b:.3e}, row {r})")
    rows, want = NC.exact_rows(rec)
    assert torch.equal(g.double()[rows], want[rows]), (label, "rows that must be exact")
    dead = NC.unscaled_rows(rec)
    assert float(g[dead].abs().max() if bool(dead.any()) else 0.0) == 0, (label, "rows without a scale must be zero")
    if not a < b:
        fails.append(f"{label}: {a:.3e} >= {b:.3e} at row {r}")


def planes_decode_to(xp, y, n_rows, k, k0=0, n=None):
    """The planes output decodes to the fp32 output within the pair format's own error: 2^-23 relative + f16's subnormal quantum."""
    from str2str_amd import ops

    n = y.shape[1] if n is None else n
    d = ops.unpack_planes(xp, n_rows, k)[:, k0:k0 + n]
    return bool(((d - y).abs() <= 2.0 ** -23 * y.abs() + 2.0 ** -24).all())


def run_forms(layer, kwd, M, arith):
    """{form: fp32 output [M, n_pad]} of one layer through every form of its arithmetic; the planes of each f16x3 form are checked
    against its fp32 output on the way."""
    from str2str_amd import ops

    ep = epilogue_of(kwd)
    K, n = layer["k"], layer["n"]
    if arith == "f32":
        return {"node_linear_f32": ops.node_apply(kwd["x"], layer, M, **ep)[0]}
    xp = ops.pack_planes(kwd["x"])
    out = {}
    forms = [("wide", "w", layer["tg"])] + ([("narrow", "w_s", layer["tg_s"])] if layer["tg_s"] != layer["tg"] else [])
    for form, key, tg in forms:
        y, yxp = ops.node_linear(xp, layer[key], layer["b"], M, K, n, tg, want_xp=True, **ep)
        assert planes_decode_to(yxp, y, M, n), (form, "planes")
        out["node_linear " + form] = y
    y, yxp = ops.node_apply(xp, layer, M, want_xp=True, **ep)
    assert planes_decode_to(yxp, y, M, n), ("node_apply", "planes")
    out["node_apply"] = y
    return out


# ------------------------------------------------------------------------------------------------ single layers, every form
@pytest.mark.parametrize("family", NC.FAMILIES)
@pytest.mark.parametrize("arith", ARITHS)
def test_single_layers_vs_float64(arith, family):
    fails = []
    for fam, kind, ws in NC.layer_table():
        if fam != family:
            continue
        d32 = NC.layer_d32(fam, kind, ws)
        tag = f"{fam} {kind}" + (f" w x {ws:g}" if ws != 1.0 else "")
        for M in NC.ROWS:
            c = NC.layer_case(fam, kind, M, ws)
            kwd = {k: dev(v) for k, v in c["kw"].items()}
            tr = []
            RN.layer(**kwd, trace=tr)
            layer = packed((fam, kind, ws), c["kw"]["w"], c["kw"].get("b"), kwd.get("ln") is not None)
            floor = NC.row_floor(tr) if arith == "f16x3" else None
            for form, y in run_forms(layer, kwd, M, arith).items():
                judge(f"{form} {c['name']}", fam, arith, y, tr[0], d32, floor, fails, margin=f"node {form} vs float64: {tag}")
    assert not fails, fails


def test_node_apply_on_the_far_side_of_each_policy_switch():
    """ops.node_apply at the smallest row count beyond SMALL_ROWS (linear_out, K = 2688: the fused layer instead of narrow GEMM +
    s2s_row_layernorm) and beyond NARROW_MAX_WORK (linear_q, K = 256, 2048 columns: the wide column blocks), and at the last row
    count in front of each."""
    from str2str_amd import ops

    sd, fails = synth_sd(0, 0.02), []
    g = torch.Generator().manual_seed(11)
    wq, bq = RN.lin(sd, T + "ipa_0.linear_q")
    n_q = wq.shape[0]
    d32 = _plain_d32(wq, bq, False)
    for M in (ops.NARROW_MAX_WORK // n_q, ops.NARROW_MAX_WORK // n_q + 1):
        layer = packed("linear_q", wq, bq, False)
        assert layer["tg_s"] != layer["tg"]
        assert ops.node.small_rows_variant(layer, M)[0] == ("w_s" if M * n_q <= ops.NARROW_MAX_WORK else "w")
        x = torch.randn(M, 256, generator=g)
        tr, xd = [], dev(x)
        RN.layer(xd, dev(wq), dev(bq), trace=tr)
        y, _ = ops.node_apply(ops.pack_planes(xd), layer, M)
        judge(f"node_apply linear_q M{M}", "flat", "f16x3", y, tr[0], d32, NC.row_floor(tr), fails,
              margin=f"node node_apply at the packing switch vs float64: flat linear_q M{M}")
        del tr, y
    c = NC.layer_case("flat", "linear_out", NC.ROWS[-1])
    w, b, ln = c["kw"]["w"], c["kw"]["b"], c["kw"]["ln"]
    layer = packed(("flat", "linear_out", 1.0), w, b, True)
    for M in (ops.SMALL_ROWS, ops.SMALL_ROWS + 1):
        x, res = dev(torch.randn(M, 2688, generator=g)), dev(torch.randn(M, 256, generator=g))
        tr = []
        RN.layer(x, dev(w), dev(b), residual=res, ln=dev(ln), trace=tr)
        layer.pop("w_n", None)
        y, _ = ops.node_apply(ops.pack_planes(x), layer, M, residual=res, ln=dev(ln))
        assert ("w_n" in layer) == (M <= ops.SMALL_ROWS)       # the narrow packing is built only where the split form runs
        judge(f"node_apply linear_out M{M}", "flat", "f16x3", y, tr[0], NC.layer_d32("flat", "linear_out"), NC.row_floor(tr), fails,
              margin=f"node node_apply at the LayerNorm split switch vs float64: flat linear_out M{M}")
        del tr, y
    assert not fails, fails


@pytest.mark.parametrize("kind", NC.LN_KINDS)
def test_row_layernorm_alone_on_offset_rows(kind):
    from str2str_amd import ops

    fails, d32 = [], NC.ln_d32(kind)
    for M in NC.ROWS:
        x, ln = NC.ln_case(kind, M)
        xd, lnd = dev(x), dev(ln)
        rec = NC.ln_record(xd, lnd)
        y, yxp = ops.row_layernorm(xd, M, x.shape[1], lnd[0], lnd[1], lnd[2], want_xp=True)
        assert planes_decode_to(yxp, y, M, x.shape[1])
        judge(f"row_layernorm offset {kind} M{M}", "offset", "f32", y, rec, d32, None, fails, margin=f"node row_layernorm vs float64: offset {kind}")
    assert not fails, fails


def _plain_d32(w, b, small, amp=1.0):
    """D32 of x W^T + b on amp x N(0, 1) rows (x the small family's row scales), pooled over the table's row counts."""
    g, worst = torch.Generator().manual_seed(77), 0.0
    for M in NC.ROWS:
        x = amp * torch.randn(M, w.shape[1], generator=g) * (NC.row_scales(M)[:, None] if small else 1.0)
        tr = []
        RN.layer(x, w, b, trace=tr)
        worst = max(worst, NC.nanmax(NC.row_errors(RN.layer(x, w, b, dtype=torch.float32), tr[0])))
    return worst


def decode_vfrag(vf, M, n_out, tph):
    RT = (M + 31) // 32
    fr = vf.view(torch.float16).reshape(RT, n_out // 32 // tph, tph, 2, 2, 2, 32, 8).float().sum(4)   # [RT, H, ct, u, h, c, j]
    u = torch.arange(2)[:, None, None]; h = torch.arange(2)[None, :, None]; j = torch.arange(8)[None, None, :]
    r = 8 * u + j
    row = ((r & 3) + 8 * (r >> 2) + 4 * h).to(vf.device)                                             # [u, h, j]
    y = torch.zeros(RT, 32, n_out, device=vf.device)
    y[:, row.reshape(-1)] = fr.permute(0, 3, 4, 6, 1, 2, 5).reshape(RT, 32, n_out)
    return y.reshape(-1, n_out)


@pytest.mark.parametrize("family", ["flat", "trained-like", "small"])
def test_node_linear_vfrag_vs_float64(family):
    """s2s_node_linear_vfrag (the value projection stored as A fragments), decoded, with and without a padded row map."""
    from str2str_amd import ops

    sd, fails = NC.sd_of(family), []
    amp = NC.AMP_TRAINED if family == "trained-like" else 1.0
    w, b = RN.lin(sd, T + "ipa_0.linear_q")            # 256 -> 2048, 8 heads x 8 column tiles
    wpk = ops.pack_node_weight(dev(w), 8)
    g = torch.Generator().manual_seed(21)
    bb = None if family == "small" else b
    cases = [(M, None) for M in (33, 257)] + [(3 * n_pad, (n_pad, n_src)) for n_pad, n_src in NC.ROW_MAPS.values()]
    d32 = _plain_d32(w, bb, family == "small", amp)
    for rows, rmap in cases:
        m_in = rows if rmap is None else rows // rmap[0] * rmap[1]
        x = amp * torch.randn(m_in, 256, generator=g)
        if family == "small":
            x = x * NC.row_scales(m_in)[:, None]
        idx = torch.arange(rows) if rmap is None else RN.row_map_index(rows, *rmap)
        tr, xd = [], dev(x)
        RN.layer(xd[idx.to(DEV)], dev(w), None if bb is None else dev(bb), trace=tr)
        vf = ops.node_linear_vfrag(ops.pack_planes(xd), wpk, torch.zeros(2048, device=DEV) if bb is None else dev(bb), rows, 256, 2048, 8, row_map=rmap)
        y = decode_vfrag(vf, rows, 2048, 8)
        assert float(y[rows:].abs().max()) == 0 if y.shape[0] > rows else True
        judge(f"node_linear_vfrag {family} rows{rows} map{rmap}", family, "f16x3", y[:rows], tr[0], d32, NC.row_floor(tr), fails,
              margin=f"node node_linear_vfrag vs float64: {family}")
        if rmap is not None:
            v = y[:rows].view(-1, rmap[0], 2048)
            assert torch.equal(v[:, rmap[1]:], v[:, rmap[1] - 1:rmap[1]].expand(-1, rmap[0] - rmap[1], -1))
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ outputs
@pytest.mark.parametrize("kind,M", [("skip", 257), ("bb", 129), ("nt3", 680)])
def test_outputs_land_where_they_are_asked_for(kind, M):
    """out_f32 at out_col0 of a wider sentinel-filled buffer and out_xp at out_xp_k0 of a wider planes buffer: the same values as the
    plain call, every other byte untouched; a padded row map repeats each sample's last row."""
    from str2str_amd import ops

    c = NC.layer_case("flat", kind, M)
    kwd = {k: dev(v) for k, v in c["kw"].items()}
    layer = packed(("flat", kind, 1.0), c["kw"]["w"], c["kw"]["b"], kwd.get("ln") is not None)
    ep, n, K = epilogue_of(kwd), layer["n"], layer["k"]
    xp = ops.pack_planes(kwd["x"])
    y0, yxp0 = ops.node_linear(xp, layer["w"], layer["b"], M, K, n, layer["tg"], want_xp=True, **ep)
    out = torch.full((M, n + 96), -7.0, device=DEV)
    kx = n + 64
    oxp = ops.xp_alloc(M, kx, DEV).fill_(0x5A5A)
    before = oxp.clone()
    ops.node_linear(xp, layer["w"], layer["b"], M, K, n, layer["tg"], out_f32=out, out_col0=32, out_xp=oxp, out_xp_k=kx, out_xp_k0=32, **ep)
    assert torch.equal(out[:, 32:32 + n], y0) and bool((out[:, :32] == -7).all()) and bool((out[:, 32 + n:] == -7).all())
    a, b0 = oxp.view(-1, kx // 16, 1024), before.view(-1, kx // 16, 1024)
    assert torch.equal(a[:, 2:2 + n // 16], yxp0.view(-1, n // 16, 1024))
    assert torch.equal(a[:, :2], b0[:, :2]) and torch.equal(a[:, 2 + n // 16:], b0[:, 2 + n // 16:])
    if kwd.get("ln") is None and not ep:
        for n_pad, n_src in NC.ROW_MAPS.values():
            rows, m_in = 3 * n_pad, 3 * n_src
            if m_in > M:
                continue
            xs = ops.pack_planes(kwd["x"][:m_in].contiguous())
            ym, _ = ops.node_linear(xs, layer["w"], layer["b"], rows, K, n, layer["tg"], row_map=(n_pad, n_src))
            assert torch.equal(ym, y0[RN.row_map_index(rows, n_pad, n_src).to(DEV)])


def test_torsion_head_clamp_and_blend_rows():
    """s2s_torsion_head on given rows: u = 0 (the clamp: 0 / sqrt(eps) = 0, exactly), a row under the clamp, ordinary rows, fixed rows
    (the input torsion, exactly)."""
    from str2str_amd import ops

    u = torch.tensor([[0.0, 0.0], [3e-6, -4e-6], [0.3, -0.4], [-5.0, 12.0], [1.0, 2.0], [0.0, 0.0]])
    gt = torch.nn.functional.normalize(torch.randn(1, 6, 7, 2, generator=torch.Generator().manual_seed(1)), dim=-1)
    fixed = torch.tensor([0.0, 0.0, 0.0, 0.0, 1.0, 1.0])
    up = torch.zeros(6, 32); up[:, :2] = u
    got = ops.torsion_head(dev(up), 6, True, 1e-8, dev(gt)[..., 2, :], dev(fixed)).cpu()
    want = RN.torsion_normalise(u, gt[0, :, 2, :], fixed)
    assert torch.equal(got[0], torch.zeros(2)) and torch.equal(got[4:], gt[0, 4:, 2, :])
    assert float((got.double() - want).abs().max()) < 4 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ several problems, one launch
def _multi_specs(net, which, M, dm):
    """-> (specs for ops.node_apply_multi, refs, getters).  A ref is a float64 layer of the state dict's own weights -- dict(w, b, relu,
    pre = None | "diffuse" (the diffuse mask as row scale) | "x32" (the constant 32)) -- or, for the folded A and B | G layers of the
    EdgeTransition, dict(unfolded=[(output of ref_node.edge_node_parts, first column, last column, factor)])."""
    from str2str_amd import ops

    tr = net.translator
    W = tr._node_weights()
    sd = synth_sd(0, 0.02)
    if which == "skips":          # the four skip_embeds, each into columns 256.. of its block's [M, 320] buffers
        bufs = [(torch.full((M, 320), -7.0, device=DEV), ops.xp_alloc(M, 320, DEV)) for _ in range(4)]
        specs = [(W[b]["skip"], dict(out_f32=bufs[b][0], out_col0=256, out_xp=bufs[b][1], out_xp_k=320, out_xp_k0=256)) for b in range(4)]
        refs = [dict(w=sd[f"{T}skip_embed_{b}.weight"], b=sd[f"{T}skip_embed_{b}.bias"]) for b in range(4)]
        return specs, refs, [lambda o, b=b: bufs[b][0][:, 256:] for b in range(4)]
    et = tr.trunk["edge_transition_0"]
    nl = et.node_layers()
    bb = (W[0]["bb"], dict(pre_scale=dm))
    bb_ref = dict(w=sd[T + "bb_update_0.linear.weight"], b=sd[T + "bb_update_0.linear.bias"], pre="diffuse")
    t1 = (W["tor"]["l1"], dict(relu=True, want_f32=False, want_xp=True))
    t1_ref = dict(w=sd[RN.TORSION + ".linear_1.weight"], b=sd[RN.TORSION + ".linear_1.bias"], relu=True)
    if which == "last-block":     # backbone update + the torsion head's first layer (planes only)
        return [bb, t1], [bb_ref, t1_ref], [lambda o: o[0][0], lambda o: ops.unpack_planes(o[1][1], M, 256)]
    # backbone update + initial_embed + the folded A and (x 32, as a row pre-scale with a x 32 bias) B | G halves + two more widths
    ab, ab_specs = et.ab16_specs(nl, True, M, DEV)
    xf, xa = torch.full((M, 320), -7.0, device=DEV), ops.xp_alloc(M, 320, DEV)
    specs = [bb, (nl["init"], {})] + ab_specs + [t1, (W[0]["skip"], dict(out_f32=xf, out_col0=256, out_xp=xa, out_xp_k=320, out_xp_k0=256))]
    refs = [bb_ref, dict(w=sd[T + "edge_transition_0.initial_embed.weight"], b=sd[T + "edge_transition_0.initial_embed.bias"]),
            dict(unfolded=[("A", 0, 384, 1.0)]), dict(unfolded=[("B", 0, 384, 32.0), ("G", 384, 512, 32.0)]), t1_ref,
            dict(w=sd[T + "skip_embed_0.weight"], b=sd[T + "skip_embed_0.bias"])]
    gets = [lambda o: o[0][0], lambda o: o[1][0], lambda o: ab[:, :384], lambda o: ab[:, 384:], lambda o: ops.unpack_planes(o[4][1], M, 256),
            lambda o: xf[:, 256:]]
    return specs, refs, gets


def _ref_kwargs(ref, d, M, to=lambda t: t):
    kw = {k: (to(v) if torch.is_tensor(v) else v) for k, v in ref.items() if k != "pre"}
    if ref.get("pre"):
        kw["pre_scale"] = to(d["diffuse"] if ref["pre"] == "diffuse" else torch.full((M,), 32.0))
    return kw


_MULTI_D32 = {}


def _multi_d32(family, which, i, ref):
    """D32 of problem ``i``: its float32 layer (for the folded EdgeTransition layers: the float32 unfolded chain, per output) against
    float64 on the family's s' rows, pooled over the table's row counts."""
    key = (family, which, i)
    if key not in _MULTI_D32:
        sd = synth_sd(0, 0.02)
        worst = {}
        for M in NC.ROWS:
            d = NC.stage_inputs(family, M)
            if "unfolded" in ref:
                got, _ = NC.run_stage("edge_node_parts", sd, d, dtype=torch.float32)
                _, tr = NC.run_stage("edge_node_parts", sd, d)
                for name, *_ in ref["unfolded"]:
                    worst[name] = max(worst.get(name, 0.0), NC.nanmax(NC.row_errors(got[name], tr[NC.OUTPUTS["edge_node_parts"][name]])))
            else:
                kw = _ref_kwargs(ref, d, M)
                tr = []
                RN.layer(d["s1"], **kw, trace=tr)
                worst[None] = max(worst.get(None, 0.0), NC.nanmax(NC.row_errors(RN.layer(d["s1"], **kw, dtype=torch.float32), tr[0])))
        _MULTI_D32[key] = worst
    return _MULTI_D32[key]


@pytest.mark.parametrize("family", ["flat", "trained-like", "small", "masked"])
@pytest.mark.parametrize("which", ["last-block", "skips", "edge-parts"])
def test_node_linear_multi_every_problem_vs_float64(net, which, family):
    """s2s_node_linear_multi with 2, 4 and 6 problems of different widths, pre_scale, relu and out_col0 -- the launches of the trunk --
    every problem against the float64 layer of the state dict's weights; the folded A and 32 (B | G) layers of the EdgeTransition
    against the UNFOLDED formula (ref_node.edge_node_parts).  (A planes-only output is judged through its decoded planes: the pair
    format's 2^-23 is inside 3 x D32 + F only because F covers the low plane.)"""
    from str2str_amd import ops

    fails = []
    sdd = {k: dev(v) for k, v in synth_sd(0, 0.02).items() if "edge_transition_0" in k}
    for M in (33, 129, 680):
        d = NC.stage_inputs(family, M)
        s1, dm = dev(d["s1"]), dev(d["diffuse"])
        specs, refs, gets = _multi_specs(net, which, M, dm)
        outs = ops.node_apply_multi(ops.pack_planes(s1), specs, M)
        for i, (ref, get) in enumerate(zip(refs, gets)):
            d32, got = _multi_d32(family, which, i, ref), get(outs)
            if "unfolded" in ref:
                _, tr = NC.run_stage("edge_node_parts", sdd, {"s1": s1})
                for name, c0, c1, mul in ref["unfolded"]:
                    j = NC.OUTPUTS["edge_node_parts"][name]
                    judge(f"node_linear_multi {which}[{i}] {name} {family} M{M}", family, "f16x3", got[:, c0:c1] / mul, tr[j], d32[name],
                          NC.row_floor(tr, j), fails, margin=f"node node_linear_multi vs float64 (unfolded): {which}[{i}] {name} {family}")
                continue
            tr = []
            RN.layer(s1, **_ref_kwargs(ref, d, M, dev), trace=tr)
            judge(f"node_linear_multi {which}[{i}] {family} M{M}", family, "f16x3", got, tr[0], d32[None], NC.row_floor(tr), fails,
                  margin=f"node node_linear_multi vs float64: {which}[{i}] {family}")
        if which != "last-block":
            buf = specs[-1][1]["out_f32"]
            assert bool((buf[:, :256] == -7).all())
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ chains in one launch
def _chain_layers(family, name):
    width, layers, _ = NC.CHAINS[name]
    sd = NC.sd_of(family)
    return [packed((family, p), *RN.lin(sd, p), True) for p, _ in layers]


@pytest.mark.parametrize("name,family", [(n, f) for n in NC.CHAINS for f in NC.CHAIN_FAMILIES if f != "offset" or NC.CHAINS[n][2]])
def test_node_chain_vs_float64(name, family):
    """s2s_node_chain called directly: 2, 3 and 4 layers of width 256 and 320, the last with residual + LayerNorm + mask."""
    from str2str_amd import ops

    width, spec, ln = NC.CHAINS[name]
    sd, fails, d32 = NC.sd_of(family), [], NC.chain_d32(family, name)
    layers = _chain_layers(family, name)
    for M in NC.ROWS:
        x, res, mask = (None if t is None else dev(t) for t in NC.chain_inputs(family, name, M))
        tr = NC.run_chain(name, {k: dev(v) for k, v in sd.items() if any(k.startswith(p) for p, _ in spec) or (ln and k.startswith(ln))}, x, res, mask)
        kw = {}
        if ln:
            g, b, eps = dev(RN.ln_of(sd, ln))
            kw = dict(residual=res, ln_gamma=g, ln_beta=b, ln_eps=eps, post_mask=mask)
        y, yxp = ops.node_chain(ops.pack_planes(x), [L["w_row"] for L in layers], [L["b"] for L in layers], [r for _, r in spec], M, width,
                                want_xp=True, **kw)
        assert planes_decode_to(yxp, y, M, width)
        judge(f"node_chain {name} {family} M{M}", family, "f16x3", y, tr[-1], d32, NC.row_floor(tr), fails,
              margin=f"node node_chain vs float64: {name} {family}")
    assert not fails, fails


def _trunk_chain(net, stage, family, M, arith, fails, direct=False):
    """post_attention (320: out_proj + residual + norm1 -> x1, linear1, linear2 + x1 + norm2) or node_transition (320 -> 256 first layer,
    its fp32 result the last layer's residual) as the trunk calls them."""
    from str2str_amd import ops

    tr_ = net.translator
    W = tr_._node_weights()[0]
    d = NC.stage_inputs(family, M)
    sdd = {k: dev(v) for k, v in NC.sd_of(family).items() if "transformer_0.layers.0" in k or "linear_0" in k or "node_transition_0" in k}
    dd = {k: dev(v) for k, v in d.items()}
    _, tr = NC.run_stage(stage, sdd, dd)
    d32 = NC.stage_d32(family, stage)
    if family == "trained-like":
        pk = lambda p, whole=False: packed((family, p), *RN.lin(NC.sd_of(family), p), whole)  # noqa: E731
    else:
        pk = None
    act = lambda t: ops.to_act(t, arith)  # noqa: E731
    if stage == "post_attention":
        p = T + "transformer_0.layers.0."
        lw = W["layers"][0]
        layers = [lw["o"], lw["l1"], lw["l2"]] if pk is None else [pk(p + "self_attn.out_proj", True), pk(p + "linear1"), pk(p + "linear2", True)]
        n1, n2 = dev(RN.ln_of(NC.sd_of(family), p + "norm1")), dev(RN.ln_of(NC.sd_of(family), p + "norm2"))
        x1 = torch.full((M, 320), float("nan"), device=DEV)
        if direct:
            y, _ = ops.node_chain(act(dd["sa"]), [L_["w_row"] for L_ in layers], [L_["b"] for L_ in layers], [False, True, False], M, 320,
                                  residual=x1, ln_gamma=n2[0], ln_beta=n2[1], ln_eps=n2[2], want_xp=True, mid_residual=dd["x"], mid_out_f32=x1,
                                  mid_ln=n1)
        else:
            y, _ = ops.node_apply_chain(act(dd["sa"]), layers, M, (False, True, False), first_residual=dd["x"], first_out_f32=x1, first_ln=n1,
                                        residual=x1, ln=n2, want_xp=True)
        got = {"x1": x1, "x2": y}
    else:
        p = T + "node_transition_0."
        layers = ([W["lin"], W["nt1"], W["nt2"], W["nt3"]] if pk is None else
                  [pk(T + "linear_0"), pk(p + "linear_1"), pk(p + "linear_2"), pk(p + "linear_3", True)])
        n = torch.full((M, 256), float("nan"), device=DEV)
        y, _ = ops.node_apply_chain(act(dd["x_act"]), layers, M, (False, True, True, False), first_residual=dd["s"], first_out_f32=n,
                                    residual=n, ln=dev(RN.ln_of(NC.sd_of(family), p + "ln")), post_mask=dd["mask"], want_xp=True)
        got = {"n": n, "s1": y}
    for name, i in NC.OUTPUTS[stage].items():
        form = "node_chain direct" if direct else f"trunk chain {arith}"
        judge(f"{stage}.{name} {form} {family} M{M}", family, arith, got[name], tr[i], d32[name], NC.row_floor(tr, i), fails,
              margin=f"node {form} vs float64: {family} {stage}.{name}")


@pytest.mark.parametrize("family", NC.FAMILIES)
@pytest.mark.parametrize("stage", ["post_attention", "node_transition"])
@pytest.mark.parametrize("arith", ARITHS)
def test_trunk_chains_vs_float64(net, arith, stage, family):
    """The trunk's two chains through node_apply_chain (arith f16x3: s2s_node_chain with mid_residual / mid_out_f32 aliased to the last
    residual and mid_ln, or separate launches where the policy says so; arith f32: the layers one after the other)."""
    fails = []
    for M in NC.ROWS:
        _trunk_chain(net, stage, family, M, arith, fails)
    assert not fails, fails


@pytest.mark.parametrize("family", NC.FAMILIES)
def test_node_chain_with_mid_layer_norm_called_directly(net, family):
    """s2s_node_chain itself, width 320, at every table row count (node_apply_chain takes separate launches there): out_proj +
    mid_residual + mid_ln with mid_out_f32 aliased to the last layer's residual, then linear1, linear2 + residual + LayerNorm --
    on every family, the offset rows in front of both LayerNorms included."""
    fails = []
    for M in NC.ROWS:
        _trunk_chain(net, "post_attention", family, M, "f16x3", fails, direct=True)
    assert not fails, fails


def test_node_apply_chain_picks_the_one_launch_form_for_width_320(net, monkeypatch):
    """The 320-wide chain at the smallest row count where node_apply_chain takes s2s_node_chain (64 workgroups of 128 rows): any
    separate launch would go through node_apply, which is made to fail here."""
    from str2str_amd import ops

    M = 63 * 128 + 1
    fails = []

    def no(*a, **k):
        raise AssertionError("node_apply_chain fell back to separate launches")

    monkeypatch.setattr(ops.node, "node_apply", no)
    _trunk_chain(net, "post_attention", "flat", M, "f16x3", fails)
    assert not fails, fails
    with pytest.raises(AssertionError, match="separate launches"):      # one row fewer: 63 workgroups, separate launches
        _trunk_chain(net, "post_attention", "flat", M - 1, "f16x3", [])


# ------------------------------------------------------------------------------------------------ one block, as the trunk runs it
B_BLOCK, N_BLOCK = 2, 37


def _block_reference(sd):
    """Float64 stages of block 0 in the trunk's order on given attention outputs, each stage fed the float32 rounding of the stage in
    front of it (what the kernels are handed).  -> (inputs {name: float32 device tensor}, traces {stage: float64 trace})."""
    B, N = B_BLOCK, N_BLOCK
    M = B * N
    g = torch.Generator().manual_seed(404)
    mask = (torch.rand(M, generator=g) >= 0.25).float()
    mask[0], mask[5:9], mask[N + 3] = 1.0, 0.0, 0.0
    fixed = (torch.rand(M, generator=g) < 0.3).float()
    gt = torch.nn.functional.normalize(torch.randn(B, N, 7, 2, generator=g), dim=-1)
    r32 = lambda t: t.float().to(DEV).contiguous()  # noqa: E731
    sdd = {k: v.to(DEV) for k, v in sd.items() if "_0" in k or "torsion" in k}
    I = dict(mask=r32(mask), fixed=r32(fixed), gt=r32(gt), diffuse=r32((1 - fixed) * mask))
    I["feats"], I["init"] = r32(torch.randn(M, 2688, generator=g)), r32(torch.randn(M, 256, generator=g) * mask[:, None])
    I["s"] = r32(torch.randn(M, 256, generator=g) * mask[:, None])
    I["sa"] = [r32(torch.randn(M, 320, generator=g)) for _ in range(2)]
    R = {}

    def run(name, fn, *a, **kw):
        tr = []
        out = fn(sdd, *a, trace=tr, **kw)
        R[name] = tr
        return out

    x_ln = run("linear_out", RN.linear_out, 0, I["feats"], I["s"], I["mask"])
    skip = run("skip_embed", RN.skip_embed, 0, I["init"])
    I["x0"] = RN.transformer_input(x_ln, skip).float()
    xx = I["x0"]
    I["x"] = []
    for l in range(2):
        I["x"].append(xx)
        run(f"in_proj{l}", RN.in_proj, 0, l, xx)
        _, x2 = run(f"post_attention{l}", RN.post_attention, 0, l, xx, I["sa"][l])
        xx = x2.float()
    I["x2"] = xx
    I["x_ln"] = x_ln.float()
    s1 = run("node_transition", RN.node_transition, 0, I["x_ln"], xx, I["mask"])
    I["s1"] = s1.float()
    run("backbone_update", RN.backbone_update, 0, I["s1"], I["diffuse"])
    run("edge_node_parts", RN.edge_node_parts, 0, I["s1"])
    tr = []
    RN.torsion_head(sdd, I["s1"], trace=tr)
    R["torsion_head"] = tr
    return I, R


@pytest.mark.parametrize("arith", ARITHS)
def test_one_trunk_block_stage_by_stage(net, arith):
    """The node path of block 0 with the ops calls of TranslationIPA.forward, in its order, each stage on the float64 reference's
    rounded input: x_ln | skip, qkv and the post-attention half of both encoder layers, n and s', upd (6 columns, per row),
    n' and A | 32 B | 32 G (arith f32: A | B | G) against the unfolded formula, u and psi."""
    from str2str_amd import ops

    sd = synth_sd(0, 0.02)
    I, R = _block_reference(sd)
    B, N = B_BLOCK, N_BLOCK
    M, C, D = B * N, 256, 320
    tr_ = net.translator
    Tm, W = tr_.trunk, tr_._node_weights()
    w, f16 = W[0], arith == "f16x3"
    fam, fails = "masked", []
    act = lambda t: ops.to_act(t, arith)  # noqa: E731
    lin = lambda x, wl, **kw: ops.node_apply(x, wl, M, **kw)  # noqa: E731
    d32 = {st: NC.stage_d32(fam, st) for st in NC.STAGES}

    def jd(stage, name, got, tr, i, d):
        judge(f"block {arith} {stage}.{name}", fam, arith, got, tr[i], d, NC.row_floor(tr, i), fails, margin=f"node trunk block {arith} vs float64: {stage}.{name}")

    ipa, ln = Tm["ipa_0"], Tm["ipa_ln_0"]
    x_f32 = torch.empty(M, D, device=DEV)
    x_a = ops.xp_alloc(M, D, DEV) if f16 else x_f32
    lin(act(I["feats"]), ipa.node_packs()["out"], pre_mask=I["mask"], residual=I["s"], ln=(ln.weight, ln.bias, ln.eps), out_f32=x_f32, out_xp=x_a, out_xp_k=D)
    lin(act(I["init"]), w["skip"], out_f32=x_f32, out_col0=C, out_xp=x_a, out_xp_k=D, out_xp_k0=C)
    jd("linear_out", "x_ln", x_f32[:, :C], R["linear_out"], 0, d32["linear_out"]["x_ln"])
    jd("skip_embed", "skip", x_f32[:, C:], R["skip_embed"], 0, d32["skip_embed"]["skip"])
    if f16:
        assert planes_decode_to(x_a, x_f32, M, D)
    for l, (layer, lw) in enumerate(zip(Tm["transformer_0"].layers, w["layers"])):
        xin = I["x"][l]
        qkv, _ = lin(act(xin), lw["in"])
        jd(f"in_proj{l}", "qkv", qkv, R[f"in_proj{l}"], 0, d32["in_proj"]["qkv"])
        x1 = torch.empty(M, D, device=DEV)
        xf, _ = ops.node_apply_chain(act(I["sa"][l]), [lw["o"], lw["l1"], lw["l2"]], M, (False, True, False), first_residual=xin, first_out_f32=x1,
                                     first_ln=(layer.norm1.weight, layer.norm1.bias, layer.norm1.eps), residual=x1,
                                     ln=(layer.norm2.weight, layer.norm2.bias, layer.norm2.eps), want_xp=True)
        jd(f"post_attention{l}", "x1", x1, R[f"post_attention{l}"], 0, d32["post_attention"]["x1"])
        jd(f"post_attention{l}", "x2", xf, R[f"post_attention{l}"], 2, d32["post_attention"]["x2"])
    nt = Tm["node_transition_0"]
    n_f32 = torch.empty(M, C, device=DEV)
    s_f32, _ = ops.node_apply_chain(act(I["x2"]), [w["lin"], w["nt1"], w["nt2"], w["nt3"]], M, (False, True, True, False), first_residual=I["x0"],
                                    first_out_f32=n_f32, residual=n_f32, ln=(nt.ln.weight, nt.ln.bias, nt.ln.eps), post_mask=I["mask"], want_xp=True)
    jd("node_transition", "n", n_f32, R["node_transition"], 0, d32["node_transition"]["n"])
    jd("node_transition", "s1", s_f32, R["node_transition"], 3, d32["node_transition"]["s1"])
    s_a = act(I["s1"])
    et = Tm["edge_transition_0"]
    nl = et.node_layers()
    specs = [(w["bb"], dict(pre_scale=I["diffuse"]))]
    if f16:
        node_ab, ab_specs = et.ab16_specs(nl, True, M, DEV)
        specs += [(nl["init"], {})] + ab_specs
    else:
        specs += [(nl["init"], {}), (nl["ab_s"], {})]
    specs += [(W["tor"]["l1"], dict(relu=True, want_f32=False, want_xp=True))]
    outs = ops.node_apply_multi(s_a, specs, M)
    jd("backbone_update", "upd", outs[0][0], R["backbone_update"], 0, d32["backbone_update"]["upd"])
    jd("edge_node_parts", "n_p", outs[1][0], R["edge_node_parts"], 0, d32["edge_node_parts"]["n_p"])
    ab = node_ab if f16 else outs[2][0]
    k = 32.0 if f16 else 1.0
    for name, i, c0, c1, mul in (("A", 1, 0, 384, 1.0), ("B", 2, 384, 768, k), ("G", 3, 768, 896, k)):
        jd("edge_node_parts", name, ab[:, c0:c1] / mul, R["edge_node_parts"], i, d32["edge_node_parts"][name])
    wt = W["tor"]
    t1 = outs[-1][1]
    _, t2 = lin(t1, wt["l2"], residual=I["s1"], want_f32=False, want_xp=True)
    u = lin(t2, wt["fin"])[0]
    trt = R["torsion_head"]
    jd("torsion_head", "u", u, trt, 2, d32["torsion_head"]["u"])
    psi = ops.torsion_head(u, M, True, tr_.torsion_pred.eps, I["gt"][..., 2, :], I["fixed"])
    gt2 = I["gt"][..., 2, :].reshape(M, 2)
    err, fl = NC.psi_errors(psi, trt[2], gt2, I["fixed"], NC.floors(trt)[2] if f16 else None)
    bound = 3 * NC.psi_d32(fam) + fl
    r = int((err / bound).argmax())
    record_margin(f"node trunk block {arith} vs float64: psi", float(err[r]), float(bound[r]))
    print(f"block {arith} psi: {float(err[r]):.3e} (bound {float(bound[r]):.3e}, row {r})")
    assert torch.equal(psi[I["fixed"] == 1], gt2[I["fixed"] == 1])
    if not bool((err < bound).all()):
        fails.append(f"psi: {float(err[r]):.3e} >= {float(bound[r]):.3e} at row {r}")
    assert not fails, fails
