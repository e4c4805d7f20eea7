"""The pair stream on the HIP kernels (csrc/edge_transition_f16.h, csrc/edge_embed_f16.h, csrc/pair_mlp.hip behind EdgeTransition / EmbeddingModule) against the
float64 statement of its formulas (tests/ref_pair.py, evaluated with torch on the device), per pair, at the cases of
tests/pair_cases.py: N below and from 32 (both STAGE instantiations), with and without the fused projection (both PROJ
instantiations), launch splits, more tiles than persistent workgroups with a ragged end; the families flat, trained-like (x 150),
offset-G / offset-W (|channel mean| up to 30 x the pair's channel spread in front of the LayerNorm, planted in G_j and in the final
layer's weights and bias), small (2^-(p mod 16)), masked (exact zeros, projections = their bias) and the block exponents 5, 10, 15.

  both contract levels   the module's forward from (node, edge) and pair_mlp from given per-node vectors, both arithmetics
  outputs                out, attn_bias, pair_z; without the projection; out_layout "none"
  layouts                tiled in / tiled out / mixed against float64 (not against each other), the launch splits included
  one trunk block        s -> the node kernel's [A | 32 B | 32 G] (ab16_specs, node_parts(kernel_form=True)) -> pair_mlp(ab_kernel_form=True,
                         out_layout="tiled"), end to end against float64 from s, F chained through both kernels
  out of bounds          the tiled buffer's padding and a guard band behind a row-major out keep their sentinel
  the edge embedding     its last layer with a common component in rows and bias, per pair against ref_embed.embedding64

Measure and bound: pair_cases (per pair, no floor; 3 x D32 + min(1, 3 x r16) x F for arith "f16x3", 3 x D32 for "f32": F the f16 pair
format's a-priori worst case per pair, r16 the share of it that the CPU emulation of the planes uses in that (family, level, output),
measured on the emulation and never on a kernel: a low plane lost in any one layer leaves the bound, tests/test_pair_parity_cpu.py).
Every figure is printed before it is asserted and recorded (profiles/parity_margins.json), with the largest error of any pair next
to the error of the pair closest to its bound.
"""
import copy

import pytest
import torch

import node_cases as NC
import pair_cases as PC
import ref_embed as RE
import ref_pair as RP
from conftest import record_margin

pytestmark = pytest.mark.gpu

DEV = "cuda"
ARITHS = ("f16x3", "f32")


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
    return None if t is None else t.to(DEV).contiguous()


def modules(net, c, arith, exp=0):
    """Copies of block 0's EdgeTransition and of IPA block 1 carrying the case's weights."""
    et, ipa = copy.deepcopy(net.translator.trunk["edge_transition_0"]), copy.deepcopy(net.translator.trunk["ipa_1"])
    et.load_state_dict({k[len(PC.ET):]: v for k, v in c["sd"].items() if k.startswith(PC.ET)})
    for n in ("linear_b", "down_z"):
        getattr(ipa, n).load_state_dict({k.split(".")[-1]: v for k, v in c["sd"].items() if k.startswith(f"{PC.IPA1}.{n}.")})
    et.arith, et.prescale_exp = arith, exp
    return et, ipa.pair_proj_weights()


def rows(out=None, bias=None, pz=None):
    return (None if out is None else out.reshape(-1, 128)), (None if bias is None else RP.proj_rows(bias, pz))


def judge(label, margin, family, arith, got, traces, output, d, fails):
    assert bool(torch.isfinite(got).all()), (label, "not finite")
    j = PC.judged(got, traces, output, family, d[output], arith)
    a, b, r, exact = j["achieved"], j["bound"], j["pair"], j["exact"]
    record_margin(f"pair {margin} {output}", a, b)
    record_margin(f"pair {margin} {output} [achieved / bound]", a / b, 1.0)
    # (the bound is per pair, so the pair with the largest error / bound is not the one with the largest error)
    record_margin(f"pair {margin} {output} [largest error]", j["largest"], j["largest_bound"])
    print(f"{label} {output}: {a:.3e} (bound {b:.3e}, pair {r}); largest error {j['largest']:.3e} (against {j['largest_bound']:.3e})")
    assert exact, (label, output, "masked pairs must be exact")
    if not a < b:
        fails.append(f"{label} {output}: {a:.3e} >= {b:.3e} at pair {r}")


def judge_all(label, margin, family, arith, res, traces, d, fails):
    out, proj = res
    if out is not None:
        judge(label, margin, family, arith, out, traces, "out", d, fails)
    if proj is not None:
        judge(label, margin, family, arith, proj, traces, "proj", d, fails)


def split_env(monkeypatch, shape):
    if shape in PC.SPLITS:
        monkeypatch.setenv("S2S_ET_MAX_PAIRS", str(PC.SPLITS[shape]))
    else:
        monkeypatch.delenv("S2S_ET_MAX_PAIRS", raising=False)


def inputs(c):
    return dev(c["s"]), dev(c["edge"]), dev(c["mask"]), tuple(dev(t) for t in c["parts"])


# ------------------------------------------------------------------------------------------------ every shape, family, level, arithmetic
@pytest.mark.parametrize("family", [f for f in PC.FAMILIES if not f.startswith("exp")])
def test_edge_transition_vs_float64(net, family, monkeypatch):
    """forward from (node, edge) and pair_mlp from given per-node vectors, with the fused projection, without it, and with out_layout
    "none", in both arithmetics, at every shape: each output of each call against float64, per pair."""
    fails = []
    for level in PC.levels(family):
        d = PC.d32(family, level)
        for shape in PC.SHAPES:
            c = PC.case(family, shape)
            split_env(monkeypatch, shape)
            traces = PC.run(c, level, device=DEV)[2]
            s, edge, mask, (n_p, ab) = inputs(c)
            for arith in ARITHS:
                et, nxt = modules(net, c, arith)
                tag, margin = f"{family} {level} {shape} {arith}", f"edge transition {arith} {level} vs float64: {family}"
                if level == "module":
                    call = lambda proj, **kw: et(s, edge, mask, proj, **kw)  # noqa: E731
                else:
                    call = lambda proj, **kw: et.pair_mlp(edge, ab, n_p, mask, proj, **kw)  # noqa: E731
                judge_all(tag + " proj", margin, family, arith, rows(*call(nxt)), traces, d, fails)
                judge_all(tag + " plain", margin + " (no projection)", family, arith, rows(call(None)), traces, d, fails)
                if arith == "f16x3" and level == "parts":
                    o, bias, pz = call(nxt, out_layout="none")
                    assert o is None
                    judge_all(tag + " out_layout none", margin + " (out_layout none)", family, arith, rows(None, bias, pz), traces, d, fails)
            del traces
    assert not fails, fails


@pytest.mark.parametrize("family", ["flat", "masked", "offset-G"])
def test_pair_layouts_vs_float64(net, family, monkeypatch):
    """The tiled pair layout on either side of the f16x3 kernel (ops.pair_tiled / pair_untiled), the launch splits included: every
    combination against float64, not against the row-major call."""
    from str2str_amd import ops

    fails, d = [], PC.d32(family, "parts")
    for shape in PC.SHAPES:
        c = PC.case(family, shape)
        split_env(monkeypatch, shape)
        traces = PC.run(c, "parts", device=DEV)[2]
        _, edge, mask, (n_p, ab) = inputs(c)
        et, nxt = modules(net, c, "f16x3")
        zt = ops.pair_tiled(edge)
        for name, e_in, lay in (("tiled -> tiled", zt, "tiled"), ("tiled -> rowmajor", zt, "rowmajor"), ("rowmajor -> tiled", edge, "tiled")):
            o, bias, pz = et.pair_mlp(e_in, ab, n_p, mask, nxt, out_layout=lay)
            assert isinstance(o, ops.PairTiled) == (lay == "tiled")
            o = ops.pair_untiled(o) if lay == "tiled" else o
            judge_all(f"{family} {shape} {name}", f"edge transition f16x3 layouts vs float64: {family} {name}", family, "f16x3", rows(o, bias, pz), traces, d, fails)
        o = et.pair_mlp(zt, ab, n_p, mask, None, out_layout="tiled")
        judge_all(f"{family} {shape} tiled -> tiled plain", f"edge transition f16x3 layouts vs float64: {family} tiled -> tiled (no projection)", family,
                  "f16x3", rows(ops.pair_untiled(o)), traces, d, fails)
        del traces
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ the common offset, sharply
def test_a_common_offset_in_g_costs_float32_rounding_only(net, monkeypatch):
    """LayerNorm(y + c 1) = LayerNorm(y): the f16x3 kernel on G_j + c_j (offset-G, |c_j| up to 30 x the channel spread) against the
    same kernel on G_j.  G_j passes through no f16 plane -- it starts the final layer's fp32 accumulators -- so the two runs read
    bit-identical planes and F does not enter: each lies within 3 x D32 (capped) of the same float64 row, and they differ by at most
    twice that.  (With G_j handed to the kernel uncentred the difference is 1.4e-5 .. 1.9e-5 on an MI355X: every one of the 72
    accumulations of the final layer then rounds at the offset's magnitude.)"""
    fails, d = [], PC.d32("offset-G", "parts")["out"]
    bound = 2.0 * min(3.0 * d, NC.CAP)
    for shape in PC.SHAPES:
        c = PC.case("offset-G", shape)
        split_env(monkeypatch, shape)
        _, edge, mask, (n_p, ab) = inputs(c)
        ab0 = dev(c["parts0"][1])
        assert float((ab - ab0)[..., :768].abs().max()) == 0 and float((ab - ab0)[..., 768:].abs().max()) > 0 or shape == (1, 1)
        traces = PC.run(c, "parts", device=DEV)[2]
        scale = torch.cat([PC.out_scale(t[-2]) for t in traces])
        et, nxt = modules(net, c, "f16x3")
        for name, proj in (("proj", nxt), ("plain", None)):
            a, b = et.pair_mlp(edge, ab, n_p, mask, proj), et.pair_mlp(edge, ab0, n_p, mask, proj)
            a, b = (a[0], b[0]) if proj is not None else (a, b)
            e = (a.double() - b.double()).reshape(-1, 128).abs().amax(-1) / scale
            r = int(e.argmax())
            record_margin("pair edge transition f16x3: G_j + c_j against G_j, offset-G", float(e[r]), bound)
            print(f"offset-G {shape} {name}: kernel(G + c) - kernel(G) = {float(e[r]):.3e} (bound {bound:.3e}, pair {r})")
            if not float(e[r]) < bound:
                fails.append(f"{shape} {name}: {float(e[r]):.3e} >= {bound:.3e} at pair {r}")
        del traces
    assert not fails, fails


def test_layers_in_front_of_a_layernorm_are_packed_centred(net):
    """The contract of include/str2str_hip.h: the EdgeTransition's final layer and the edge embedding's last layer reach the kernels
    centred over their output channels (C = I - 1 1^T / 128, in float64 on the host) -- in the f16x3 weight streams, in the fp32
    kernels' packed weights and bias arguments, and in the per-node layers that produce G_j -- whatever common component the module's
    own parameters carry (offset-W: rows and bias with a component of 30 x the channel spread)."""
    from str2str_amd import ops

    c = PC.case("offset-W", (3, 7))
    et, _ = modules(net, c, "f16x3")
    cen = lambda w: (w.double() - w.double().mean(0, keepdim=True)).float()  # noqa: E731
    w1, w2, wf, bf = (dev(c["sd"][PC.ET + k]) for k in ("trunk.0.weight", "trunk.2.weight", "final_layer.weight", "final_layer.bias"))
    assert float(wf.mean(0).abs().max()) > float(cen(wf).abs().max()) and float(bf.mean().abs()) > 100 * float(cen(bf).abs().max())   # the case
    assert torch.equal(et._packed()["wstream_f16"], ops.pack_f16x3_stream(w1[:, :128].contiguous(), w2, cen(wf)))
    assert torch.equal(et._packed_f32()["wfp"], ops.pack_weight(cen(wf), tile_major=True))
    assert torch.equal(et._bf_centred(), cen(bf)) and abs(float(et._bf_centred().double().sum())) < 1e-5 * float(bf.abs().max())
    M = 21
    s_a = ops.pack_planes(dev(c["s"]).reshape(M, -1))
    for kernel_form in (False, True):
        G = et.node_parts(s_a, M, kernel_form=kernel_form)[1][:, 768:].double() / (32.0 if kernel_form else 1.0)
        assert float(G.mean(-1).abs().max()) < 1e-5 * float(G.abs().max()), "G_j must leave the node kernel with channel mean 0"
    ce = PC.embed_offset_case((3, 7))
    emb = copy.deepcopy(net.embedder)
    emb.load_state_dict({k[len("embedder."):]: v for k, v in ce["sd"].items()})
    w = emb._weights()
    e2w, e4w, e4b = (dev(ce["sd"]["embedder.edge_embed." + k]) for k in ("2.weight", "4.weight", "4.bias"))
    assert torch.equal(w["w3p"], ops.pack_weight(cen(e4w))) and torch.equal(w["b3c"], cen(e4b))
    emb.arith = "f16x3"
    emb(residue_idx=ce["residue_idx"], t=ce["t"], fixed_mask=dev(ce["fixed_mask"]), self_conditioning_ca=dev(ce["ca"]))
    assert torch.equal(emb._w16cache.held()[0], ops.pack_f16x3_embed_stream(e2w, cen(e4w)))


# ------------------------------------------------------------------------------------------------ the block exponent
@pytest.mark.parametrize("e", PC.EXPS)
def test_block_exponent_family(net, e, monkeypatch):
    """Hidden activations of 2^(13.5+e) (e = 15: the 2^26 .. 2^27 that admissible inputs reach): with prescale_exp = e the range flag
    stays quiet and every pair is inside the bound (F with the activation term 2^(e-25)); with e - 5 the flag is raised."""
    from str2str_amd import ops

    family, fails = f"exp{e}", []
    for level in PC.LEVELS:
        d = PC.d32(family, level)
        for shape in PC.SHAPES:
            c = PC.case(family, shape)
            split_env(monkeypatch, shape)
            traces = PC.run(c, level, device=DEV)[2]
            s, edge, mask, (n_p, ab) = inputs(c)
            et, nxt = modules(net, c, "f16x3", e)
            call = (lambda: et(s, edge, mask, nxt)) if level == "module" else (lambda: et.pair_mlp(edge, ab, n_p, mask, nxt))
            ops.range_flag_reset()
            res = call()
            assert ops.range_flag_read() == 0, (family, level, shape, ops.range_flag_names(ops.range_flag_read()))
            judge_all(f"{family} {level} {shape}", f"edge transition f16x3 {level} vs float64: {family}", family, "f16x3", rows(*res), traces, d, fails)
            et.prescale_exp = e - 5
            call()
            assert ops.range_flag_read() & 4, (family, level, shape, "the range flag must be raised with e - 5")
            ops.range_flag_reset()
            del traces
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ one trunk block in call order
@pytest.mark.parametrize("family", ["flat", "masked", "small", "offset-W"])
def test_one_trunk_block_in_call_order(net, family):
    """s -> the node kernel's per-node vectors in the pair kernel's form (the folded layers of ab16_specs in one multi launch, as the
    trunk runs them; node_parts(kernel_form=True)) -> pair_mlp(ab_kernel_form=True, out_layout="tiled") with the fused projection: n',
    A | 32 B | 32 G and the three pair outputs against float64 from s; the pair outputs under the module-level rule of pair_cases
    (3 x D32 + min(1, 3 x r16) x F, F chained through both kernels, r16 of the (family, "module") emulation)."""
    from str2str_amd import ops

    fails, d = [], PC.d32(family, "module")
    nfam = "flat" if family.startswith("offset") else family
    dn = NC.stage_d32(nfam, "edge_node_parts") if family != "small" else None
    for shape in ((3, 7), (2, 37)):
        c = PC.case(family, shape)
        B, N = shape
        M = B * N
        traces = PC.run(c, "module", device=DEV)[2]
        s, edge, mask, _ = inputs(c)
        et, nxt = modules(net, c, "f16x3")
        s_a = ops.pack_planes(s.reshape(M, -1))
        nl = et.node_layers()
        ab16, specs = et.ab16_specs(nl, True, M, DEV)
        n_p = ops.node_apply_multi(s_a, [(nl["init"], {})] + specs, M)[0][0]
        n_p2, ab16_2 = et.node_parts(s_a, M, kernel_form=True)
        tr = traces[0]
        if family != "small":      # the node kernel's outputs against the per-node reference (G centred)
            for name, i, c0, c1, mul in (("A", 1, 0, 384, 1.0), ("B", 2, 384, 768, 32.0), ("G", 3, 768, 896, 32.0)):
                for form, got in (("folded", ab16), ("node_parts", ab16_2)):
                    a, b, r = NC.check_rows(got[:, c0:c1] / mul, tr[i], dn[name], NC.row_floor(tr[:4], i), NC.capped(nfam))
                    record_margin(f"pair trunk block vs float64: {family} {name} ({form})", a, b)
                    print(f"{family} {shape} {name} {form}: {a:.3e} (bound {b:.3e}, row {r})")
                    if not a < b:
                        fails.append(f"{family} {shape} {name} {form}: {a:.3e} >= {b:.3e} at row {r}")
        for form, (p_, ab_) in (("folded", (n_p, ab16)), ("node_parts", (n_p2, ab16_2))):
            o, bias, pz = et.pair_mlp(ops.pair_tiled(edge), ab_.view(B, N, -1), p_.view(B, N, -1), mask, nxt, out_layout="tiled", ab_kernel_form=True)
            judge_all(f"{family} {shape} block {form}", f"trunk block f16x3 vs float64 ({form}): {family}", family, "f16x3",
                      rows(ops.pair_untiled(o), bias, pz), traces, d, fails)
        del traces
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ nothing beyond B N N pairs
@pytest.mark.parametrize("shape", [(1, 1), (3, 7), (1, 33), (1, 190)])
def test_out_is_not_touched_beyond_the_pairs(net, shape):
    """A tiled out buffer's padding (B N N rounded up to 32 pairs) and a guard band behind a row-major out keep their sentinel; the
    pairs in front of them are the float64 ones."""
    from str2str_amd import ops

    fails, d = [], PC.d32("flat", "parts")
    c = PC.case("flat", shape)
    B, N = shape
    M = B * N * N
    traces = PC.run(c, "parts", device=DEV)[2]
    _, edge, mask, (n_p, ab) = inputs(c)
    et, nxt = modules(net, c, "f16x3")
    pk = et._packed()
    args = (ab, n_p, pk["wstream_f16"], et.trunk[2].bias, et.layer_norm.weight, et.layer_norm.bias, mask, et.layer_norm.eps)
    stream = torch.cat([pk["wstream_f16"], nxt["wp_f16x2"]])
    S = -7.25
    for with_proj in (False, True):
        proj = (stream, nxt["b64"]) if with_proj else None
        big = torch.full((M * 128 + 4096,), S, device=DEV)
        res = ops.edge_transition_f16x3(edge, *args, out=big[:M * 128].view(B, N, N, 128), proj=proj)
        out = res[0] if with_proj else res
        assert bool((big[M * 128:] == S).all()), "row-major out: the guard band was written"
        judge_all(f"guard band {shape} proj={with_proj}", "edge transition f16x3 into a guarded out vs float64: flat", "flat", "f16x3",
                  rows(out, *(res[1:] if with_proj else ())), traces, d, fails)
        t = ops.PairTiled(B, N, DEV)
        t.buf.fill_(S)
        res = ops.edge_transition_f16x3(ops.pair_tiled(edge), *args, out=t, proj=proj, out_layout="tiled")
        pad = t.buf.view(-1, 16, 2, 32, 4).permute(0, 3, 1, 2, 4).reshape(-1, 128)[M:]
        assert pad.numel() == (-M % 32) * 128 and bool((pad == S).all()), "tiled out: the padding was written"
        judge_all(f"tiled padding {shape} proj={with_proj}", "edge transition f16x3 into a guarded out vs float64: flat", "flat", "f16x3",
                  rows(ops.pair_untiled(t)), traces, d, fails)
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ the edge embedding's LayerNorm
_EMB_D32 = {}


def _emb_errors(got, ref64, beta):
    g, r = got.reshape(-1, 128).double(), ref64.reshape(-1, 128)
    return (g - r).abs().amax(-1) / (r - beta.to(r)).abs().amax(-1)


def emb_d32():
    """D32 of the edge embedding on the offset cases: the float32 chain (oracle.net.embedding) against float64, per pair, pooled."""
    from oracle import net as ON

    if "d" not in _EMB_D32:
        worst = 0.0
        for shape in PC.EMB_SHAPES:
            c = PC.embed_offset_case(shape)
            args = (c["residue_idx"], c["t"], c["fixed_mask"], c["ca"])
            e32 = ON.embedding(c["sd"], *args)[1]
            e64 = RE.embedding64(c["sd"], *args)[1]
            worst = max(worst, float(_emb_errors(e32, e64, c["sd"]["embedder.edge_embed.5.bias"]).max()))
        _EMB_D32["d"] = worst
    return _EMB_D32["d"]


@pytest.mark.parametrize("arith", ARITHS)
def test_edge_embedding_offset_rows_vs_float64(net, arith):
    """The edge embedding's last layer with a common component in its rows and bias (|channel mean| up to 30 x the channel spread in
    front of the LayerNorm): per pair against ref_embed.embedding64, below 32 residues and from 32."""
    fails, d = [], emb_d32()
    for shape in PC.EMB_SHAPES:
        c = PC.embed_offset_case(shape)
        emb = copy.deepcopy(net.embedder)
        emb.load_state_dict({k[len("embedder."):]: v for k, v in c["sd"].items()})
        emb.arith = arith
        _, edge = emb(residue_idx=c["residue_idx"], t=c["t"], fixed_mask=dev(c["fixed_mask"]), self_conditioning_ca=dev(c["ca"]))
        e64 = RE.embedding64(c["sd"], c["residue_idx"], c["t"], c["fixed_mask"], c["ca"], device=DEV)[1]
        e = _emb_errors(edge, e64, c["sd"]["embedder.edge_embed.5.bias"])
        share = min(1.0, 3.0 * PC.embed_r16())      # (F alone was two thirds of this bound; the format uses r16 of it: pair_cases)
        bound = min(3.0 * d, NC.CAP) + (share * PC.embed_floor(c).to(e) if arith == "f16x3" else 0.0)
        bound = bound if torch.is_tensor(bound) else torch.full_like(e, bound)
        r = int((e / bound).argmax())
        record_margin(f"pair edge embedding {arith} vs float64, offset rows", float(e[r]), float(bound[r]))
        record_margin(f"pair edge embedding {arith} vs float64, offset rows [achieved / bound]", float(e[r] / bound[r]), 1.0)
        print(f"edge embedding offset {shape} {arith}: {float(e[r]):.3e} (bound {float(bound[r]):.3e}, pair {r}; D32 {d:.3e})")
        if not bool((e < bound).all()):
            fails.append(f"{shape} {arith}: {float(e[r]):.3e} >= {float(bound[r]):.3e} at pair {r}")
    assert not fails, fails
