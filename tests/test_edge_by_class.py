"""The embedding's pair tensor BY CLASS (ops.PairByClass: s2s_edge_embed_expand in index mode + s2s_edge_transition_f16x3 reading its edge
rows out of the class table, EmbeddingModule.et_by_class = S2S_ET_BY_CLASS) against the materialised tiled tensor from the same table.

Required agreement: the class index of every pair is the host-computed class (pairs whose distance lies within 4 float32 ulps of a bin
edge aside: their bin depends on one rounding); every output of the edge transition -- z', attn_bias, pair_z -- is BIT-IDENTICAL
(compared as int32) where the edge mask m_i m_j is non-zero and equal as numbers where it is zero, and the range words are the same; a
whole evaluation is byte-identical between the two switch values.  The table row is copied in one path and read in place in the other:
there is no tolerance.  Shapes: B = 3, N = 7 (147 pairs: the per-lane-seed instantiation, tiles that span samples, a tail tile of 19
pairs), B = 2, N = 33 (2 178 pairs: the staged instantiation, tiles that cross node rows, a 2-pair tail), B = 2, N = 37 for the network.
"""
import copy
import functools

import pytest
import torch

import attention_cases as AC
import embed_cases as EC
import guarded_alloc as GA
from str2str_amd.arith import use_arith

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(3, 7), (2, 33)]


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module")
def net():
    from str2str_amd.factory import build_synthetic_net

    m = build_synthetic_net(seed=0, sigma_final=0.02, device=DEV)
    m.embedder.ee_classes = "1"
    return m


@functools.lru_cache(maxsize=None)
def inputs(B, N):
    """Both fixed-mask values (four (fa, fb) classes), a gap in the numbering, half of the last sample masked off, CA scaled so that
    several bins and "no bin" occur.  Shared between tests: read-only."""
    g = torch.Generator().manual_seed(8100 + N)
    idx = torch.arange(N)[None].repeat(B, 1)
    idx[:, N // 2:] += 3
    fixed = (torch.rand(B, N, generator=g) > 0.6).float()
    fixed[0, 0], fixed[0, 1] = 0.0, 1.0
    mask = torch.ones(B, N)
    mask[B - 1, N // 2:] = 0.0
    ca = 8.0 * torch.randn(B, N, 3, generator=g)
    return dict(residue_idx=idx, fixed_mask=fixed.to(DEV), ca=ca.to(DEV), node_mask=mask.to(DEV))


def t_img(net):
    from str2str_amd.models.net.denoising_ipa import get_timestep_embedding

    if getattr(net, "_test_t_img", None) is None:   # (once per network: the embedding of t is computed on the host)
        net._test_t_img = net.embedder.time_images(get_timestep_embedding(torch.tensor([0.37]), 32))[0].contiguous()
    return net._test_t_img


def embed(net, ins, layout, ca=None):
    """-> (node activations, pair tensor in ``layout``, (attn_bias, pair_z)) of the embedder with the first IPA block's projection fused"""
    nxt = net.translator.trunk["ipa_0"].pair_proj_weights()
    _, act, edge, proj = net.embedder.embed(ins["residue_idx"], None, ins["fixed_mask"], ins["ca"] if ca is None else ca, ins["node_mask"], nxt,
                                            edge_layout=layout, t_img=t_img(net))
    return act, edge, proj


def transition(net, act, edge, ins, out_layout, fused=True):
    """EdgeTransition 0 on the embedder's pair tensor as the trunk calls it -> [z' row-major | None, attn_bias, pair_z] (+ the range words)"""
    from str2str_amd import ops

    B, N = ins["residue_idx"].shape
    et = net.translator.trunk["edge_transition_0"]
    nxt = net.translator.trunk["ipa_1"].pair_proj_weights() if fused else None
    n_p, node_ab = et.node_parts(act, B * N, kernel_form=True)
    ops.range_flag_reset()
    res = et.pair_mlp(edge, node_ab.view(B, N, -1), n_p.view(B, N, -1), ins["node_mask"], nxt,
                      **({"out_layout": out_layout} if out_layout != "rowmajor" else {}), ab_kernel_form=True)
    z, *pr = res if fused else (res,)
    if isinstance(z, ops.PairTiled):
        z = ops.pair_untiled(z)
    return [z] + pr, ops.range_flag().tolist()


def same_bits(ins, got, ref, label):
    m = ins["node_mask"]
    em = (m[:, :, None] * m[:, None, :]) != 0
    sels = (em[..., None], em[:, None], em[..., None])
    assert len(got) == len(ref)
    for name, g, r, sel in zip(("z", "attn_bias", "pair_z"), got, ref, sels):
        if r is None:
            assert g is None, (label, name)
            continue
        assert g.shape == r.shape and torch.isfinite(r).all(), (label, name)
        diff = (g.view(torch.int32) != r.view(torch.int32)) & sel.expand_as(r)
        assert not diff.any(), (label, name, int(diff.sum()), "entries differ in bits; first at", tuple(int(v) for v in diff.nonzero()[0]))
        assert torch.equal(g, r), (label, name, "differs where the edge mask is zero")


@pytest.mark.parametrize("B,N", SHAPES)
def test_index_is_the_host_class_and_untiling_is_the_expansion(net, B, N):
    from str2str_amd import ops

    ins = inputs(B, N)
    _, edge, proj = embed(net, ins, "by_class")
    assert isinstance(edge, ops.PairByClass) and edge.rec == 168 and edge.M32 == -(-(B * N * N) // 32) * 32
    got = edge.index.cpu()
    # host classes: fa, fb = the fixed-mask values; d = idx_i - idx_j + span, clamped; bin = the edge count rule of the reference's one-hot
    idx, fixed, ca = ins["residue_idx"], ins["fixed_mask"].cpu().long(), ins["ca"].cpu().double()
    span = int(idx.max() - idx.min())
    n_rel, edges = 2 * span + 1, EC.edges64()
    d = (idx[:, :, None] - idx[:, None, :] + span).clamp(0, n_rel - 1)
    dist = torch.linalg.norm(ca[:, :, None] - ca[:, None, :], dim=-1)
    cnt = (edges < dist[..., None]).sum(-1)
    upper = torch.cat([edges[1:], torch.tensor([1e8], dtype=torch.float64)])
    bin_ = torch.where((cnt >= 1) & (dist < upper[(cnt - 1).clamp(min=0)]), cnt - 1, torch.full_like(cnt, -1))
    want = ops.edge_embed_class_row(fixed[:, :, None], fixed[:, None, :], d, bin_, n_rel, len(edges))
    ulp = 2.0 ** (torch.floor(torch.log2(dist.float().double().clamp(min=1e-30))) - 23)      # of the float32 distance
    clear = (dist[..., None] - edges).abs().amin(-1) > 4 * ulp
    m = ins["node_mask"].cpu()
    em = (m[:, :, None] * m[:, None, :]) != 0
    assert em.any() and (~em).any() and clear[em].float().mean() > 0.99
    assert len(torch.unique(bin_[em])) > 4 and (bin_[em] == -1).any() and len(torch.unique(fixed[:, :, None] * 2 + fixed[:, None, :])) == 4
    assert torch.equal(got[em & clear], want[em & clear].int())
    assert (got[~em] == -1).all()
    # the zero record in front of the table, and the materialised tensor = the tiled expansion of the same call
    assert not edge.records[0].any()
    _, tiled, proj_t = embed(net, ins, "tiled")
    assert torch.equal(ops.pair_untiled(edge).view(torch.int32), ops.pair_untiled(tiled).view(torch.int32))
    for a, b in zip(proj, proj_t):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("out_layout", ["tiled", "none"])
@pytest.mark.parametrize("B,N", SHAPES)
def test_transition_by_class_is_the_transition_on_the_tiled_tensor(net, B, N, out_layout):
    ins = inputs(B, N)
    act, edge, _ = embed(net, ins, "by_class")
    _, tiled, _ = embed(net, ins, "tiled")
    ref, words_ref = transition(net, act, tiled, ins, out_layout)
    got, words = transition(net, act, edge, ins, out_layout)
    same_bits(ins, got, ref, f"B={B} N={N} {out_layout}")
    assert words == words_ref == [0] * 8


@pytest.mark.parametrize("out_layout", ["rowmajor", "none"])
@pytest.mark.parametrize("B,N", SHAPES)
def test_split_launches(net, B, N, out_layout, monkeypatch):
    """One sample per launch (S2S_ET_MAX_PAIRS = N^2 + 7): the index pointer moves with the launch, the table does not.  (A tiled tensor
    cannot be split at these odd N^2 -- its launches start on whole blocks -- so the reference runs unsplit and the outputs are row-major.)"""
    ins = inputs(B, N)
    act, edge, _ = embed(net, ins, "by_class")
    _, tiled, _ = embed(net, ins, "tiled")
    ref, words_ref = transition(net, act, tiled, ins, out_layout)
    monkeypatch.setenv("S2S_ET_MAX_PAIRS", str(N * N + 7))
    got, words = transition(net, act, edge, ins, out_layout)
    same_bits(ins, got, ref, f"B={B} N={N} {out_layout} split")
    assert words == words_ref


def test_readers_that_need_a_tensor_materialise(net):
    """Without the fused projection the transition takes the materialised tensor (ops.pair_untiled through the expansion kernel)."""
    from str2str_amd import ops

    B, N = SHAPES[1]
    ins = inputs(B, N)
    act, edge, _ = embed(net, ins, "by_class")
    _, tiled, _ = embed(net, ins, "tiled")
    ref, _ = transition(net, act, ops.pair_untiled(tiled), ins, "rowmajor", fused=False)
    got, _ = transition(net, act, edge, ins, "rowmajor", fused=False)
    assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32))
    with pytest.raises(ops.HipLibraryError):
        ops.pair_untiled(ops.PairByClass(B, N, edge.buf, edge.rec))          # no producer to expand with


@pytest.mark.parametrize("B,N", SHAPES)
def test_records_of_128_floats(net, B, N):
    """io_layout bit 3 without bit 4: the same indices over a table of z-only records (what ``edge_embed_classes_f16x3(proj=None,
    out_layout="by_class")`` makes) -- a wrong record size reads other classes' rows."""
    from str2str_amd import ops

    ins = inputs(B, N)
    act, edge, _ = embed(net, ins, "by_class")
    _, tiled, _ = embed(net, ins, "tiled")
    narrow = ops.PairByClass(B, N, torch.cat([edge.buf[:edge.M32], edge.records[:, :128].reshape(-1)]).contiguous(), 128)
    assert narrow.rec == 128 and torch.equal(narrow.index, edge.index)
    ref, words_ref = transition(net, act, tiled, ins, "tiled")
    got, words = transition(net, act, narrow, ins, "tiled")
    same_bits(ins, got, ref, f"B={B} N={N} rec=128")
    assert words == words_ref
    # ... and from the wrapper itself: no projection -> 128-float records, the same class rows
    emb = net.embedder
    w = emb._weights()
    rel_tab, span, node_pos, idx_dev, rel_cb = emb._tables(ins["residue_idx"], w["w_rel"], w["wn_pos"])
    cls = emb._fixed_terms(ins["fixed_mask"], w, w["b0"].device, node_pos)[3]
    _, a2, b2 = torch.ops.str2str_amd.embed_assemble(t_img(net).reshape(-1).contiguous(), cls["nc2"], cls["fa2"], cls["fb2"], 1, cls["n_fixed"], False, True)
    e2, e4, ln = emb.edge_embed[2], emb.edge_embed[4], emb.edge_embed[5]
    ws = ops.pack_f16x3_embed_stream(e2.weight.float(), w["w3c"])
    plain = ops.edge_embed_classes_f16x3(a2, b2, cls["fixed_cls"], rel_cb, w["bin_tab_cb"], w["bin_lower"], idx_dev, ins["ca"], ws, e2.bias, w["b3c"],
                                         ln.weight, ln.bias, ins["node_mask"], span, ln.eps, out_layout="by_class")
    assert isinstance(plain, ops.PairByClass) and plain.rec == 128 and torch.equal(plain.index, edge.index) and not plain.records[0].any()
    assert torch.equal(plain.records.view(torch.int32), narrow.records.view(torch.int32))
    assert torch.equal(ops.pair_untiled(plain).view(torch.int32), ops.pair_untiled(tiled).view(torch.int32))


def test_trunk_materialises_for_an_exact_first_transition(net):
    """The trunk handed a PairByClass while EdgeTransition 0 runs the exact fp32 kernel: the result is that of the tiled tensor."""
    B, N = SHAPES[1]
    ins = inputs(B, N)
    m = copy.deepcopy(net)
    g = torch.Generator().manual_seed(8300)
    r7 = torch.cat([AC.random_rotations(B * N, g).view(B, N, 4), 10.0 * AC.chain_walk(B, N, g)], -1).float().to(DEV)
    nxt = m.translator.trunk["ipa_0"].pair_proj_weights()
    outs = []
    for layout in ("tiled", "by_class"):
        node, act, edge, proj = m.embedder.embed(ins["residue_idx"], None, ins["fixed_mask"], ins["ca"], ins["node_mask"], nxt, edge_layout=layout,
                                                 t_img=t_img(m))
        batch = dict(residue_idx=ins["residue_idx"], residue_mask=ins["node_mask"], fixed_mask=ins["fixed_mask"], rigids_t=r7, _node_embed_act=act)
        with use_arith(m.translator.trunk["edge_transition_0"], "f32"):
            out = m.translator(node, edge, batch, _first_proj=proj)
        outs.append((out["out_rigids7"].clone(), out["psi"].clone()))
    assert GA.same_bytes(outs[0][0], outs[1][0]) and GA.same_bytes(outs[0][1], outs[1][1]) and torch.isfinite(outs[1][0]).all()


# ---------------------------------------------------------------------------------------------------- the whole evaluation
@functools.lru_cache(maxsize=None)
def batch37():
    B, N, g = 2, 37, torch.Generator().manual_seed(8237)
    mask = torch.ones(B, N)
    mask[1, [3, 20, 36]] = 0.0
    fixed = torch.zeros(B, N)
    fixed[:, 5:9] = 1.0
    r7 = torch.cat([AC.random_rotations(B * N, g).view(B, N, 4), 10.0 * AC.chain_walk(B, N, g)], -1).float()
    return dict(residue_idx=torch.arange(N)[None].repeat(B, 1), t=torch.full((B,), 0.37), fixed_mask=fixed.to(DEV), residue_mask=mask.to(DEV),
                sc_ca_t=r7[..., 4:].to(DEV), rigids_t=r7.to(DEV),
                torsion_angles_sin_cos=torch.nn.functional.normalize(torch.randn(B, N, 7, 2, generator=g), dim=-1).to(DEV))


def evaluate(m, switch, layouts=None, monkeypatch=None):
    from str2str_amd import ops

    if layouts is not None:
        def recorded(*a, _f=ops.edge_embed_classes_f16x3, **kw):
            layouts.append(kw.get("out_layout"))
            return _f(*a, **kw)
        monkeypatch.setattr(ops, "edge_embed_classes_f16x3", recorded)
    m.embedder.et_by_class = switch
    m.backbone_in_forward = False
    out = m(dict(batch37(), t_img=t_img(m)))
    if layouts is not None:
        monkeypatch.undo()
    return out["rigids7"].clone(), out["psi"].clone()


def test_whole_evaluation_is_byte_identical(net, monkeypatch):
    m, seen = copy.deepcopy(net), []
    off = evaluate(m, "0", seen, monkeypatch)
    on = evaluate(m, "1", seen, monkeypatch)
    assert seen == ["tiled", "by_class"]
    assert GA.same_bytes(on[0], off[0]) and GA.same_bytes(on[1], off[1])
    assert torch.isfinite(on[0]).all()


@pytest.mark.parametrize("families", [("edge_transition",), ("edge_embed",), ("node", "edge_transition", "edge_embed", "ipa")])
def test_range_fallback_runs_the_exact_kernels_on_a_real_tensor(net, families, monkeypatch):
    """What the sampler's range guard does to a chunk -- the flagged families on their fp32 kernels -- with the switch on: the embedder
    is no longer asked for the pair tensor by class, and the result is the demoted network's with the switch off."""
    m, seen = copy.deepcopy(net), []
    with use_arith(m, "f32", families=families):
        off = evaluate(m, "0")
        on = evaluate(m, "1", seen, monkeypatch)
    assert "by_class" not in seen
    assert GA.same_bytes(on[0], off[0]) and GA.same_bytes(on[1], off[1])


def test_captured_graph_replay_equals_eager(net):
    """Embedding by class + EdgeTransition 0 captured once, replayed on other CA coordinates: bit for bit the eager result."""
    B, N = SHAPES[1]
    ins = inputs(B, N)
    ca = ins["ca"].clone()

    def run():
        act, edge, _ = embed(net, ins, "by_class", ca=ca)
        return transition(net, act, edge, ins, "tiled")[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                   # warm-up: derived tensors are built outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    et = net.translator.trunk["edge_transition_0"]
    nxt = net.translator.trunk["ipa_1"].pair_proj_weights()

    def captured():   # (transition() reads the range words on the host: the captured region is the launches only)
        act, edge, _ = embed(net, ins, "by_class", ca=ca)
        n_p, node_ab = et.node_parts(act, B * N, kernel_form=True)
        return et.pair_mlp(edge, node_ab.view(B, N, -1), n_p.view(B, N, -1), ins["node_mask"], nxt, out_layout="tiled", ab_kernel_form=True)

    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        z_g, bias_g, pz_g = captured()
    ca.copy_(ins["ca"].flip(0))
    g.replay()
    torch.cuda.synchronize()
    got = [z_g.buf.clone(), bias_g.clone(), pz_g.clone()]
    z_e, bias_e, pz_e = captured()
    from str2str_amd import ops
    # (through pair_untiled: the pairs past the end of the ragged last block are never written)
    for a, b in zip((ops.pair_untiled(ops.PairTiled(B, N, buf=got[0])), got[1], got[2]), (ops.pair_untiled(z_e), bias_e, pz_e)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("B,N", SHAPES)
def test_guarded_and_poisoned_run(net, B, N):
    """The by-class pair under tests/guarded_alloc.py, both poisons: bands intact, results those of the plain run -- the index words past
    the last pair and whatever the buffers held before are never read as data."""
    from str2str_amd import ops

    ins = inputs(B, N)

    def run():
        act, edge, proj = embed(net, ins, "by_class")
        out, words = transition(net, act, edge, ins, "tiled")
        torch.cuda.synchronize()
        return [edge.index.clone(), proj[0].clone(), proj[1].clone()] + out, words

    run()
    plain, words_plain = run()
    keep = {k: v.clone() for k, v in ins.items()}
    for poison in (GA.POISON_A, GA.POISON_B):
        with GA.guarded(poison) as guard:
            got, words = run()
            bands = guard.check_bands()
        assert guard.allocations and not bands, bands
        for k, (x, y) in enumerate(zip(got, plain)):
            assert GA.same_bytes(x, y), (poison, k, GA.first_difference(x, y))
        assert words == words_plain == [0] * 8
        assert all(GA.same_bytes(ins[k], keep[k]) for k in ins), "an input was modified"
    assert ops.range_flag().tolist() == [0] * 8
