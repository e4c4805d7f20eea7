"""What the node-stream parity suite (tests/test_node_parity.py) rests on, checked without a GPU:

  * tests/ref_node.py in float64 is the reference's trunk (oracle/net.py), stage by stage along a whole evaluation of the golden
    network inputs (tests/golden/net_b2n16.npz), and that walk ends at the golden psi;
  * D32 -- the float32 chain's distance from float64 under the per-row measure of tests/node_cases.py -- for every (family, layer)
    and (family, stage), recorded;
  * the CPU emulation of the f16 planes (ref_node.split_f16x3) meets 3 x D32 + F on the whole table, and on the small family exceeds
    3 x D32 alone from some input scale on (recorded): F is needed, attainable, and the measure can tell the difference;
  * the footroom of the network: F / scale_row of every stage along one trunk evaluation at B = 2, N = 24 for both synthetic weight
    styles, each below 5e-6 -- "fp32-equivalent"  holds at every node-stream input of the network, not at one O(1) example;
  * every planted mistake exceeds the bound on some case of the table.
"""
import pytest
import torch
import torch.nn.functional as F

import node_cases as NC
import ref_attention as RA
import ref_node as RN
from conftest import T, golden, record_margin, synth_sd

TR = RN.TRUNK


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def _batch(g):
    return {k[3:]: T(v) for k, v in g.items() if k.startswith("in_")}


def _close(a, b, what, tol=1e-11):
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
    assert err < tol, (what, err)


# ------------------------------------------------------------------------------------------------ the trunk, walked
def walk_trunk(sd32, batch, visit=None, check=True):
    """One evaluation of the trunk in float64 on ref_node's stages (attention sections from ref_attention, frames and the pair MLP
    from the oracle), in the order of oracle.net.translation_ipa; with ``check`` every stage is held to the oracle's own functions on
    the same inputs.  ``visit(stage, block, trace, valid_rows)`` sees every stage's float64 trace.  -> (psi [B, N, 2], rigids7)."""
    from oracle import geometry as OG
    from oracle import net as ON

    sd = {k: v.double() for k, v in sd32.items()}
    node_mask = batch["residue_mask"].double()
    fixed = batch["fixed_mask"].double()
    diffuse = (1 - fixed) * node_mask
    edge_mask = node_mask[..., None] * node_mask[..., None, :]
    node, edge = ON.embedding(sd32, batch["residue_idx"], batch["t"], fixed.float(), batch["sc_ca_t"])
    node, edge = node.double() * node_mask[..., None], edge.double() * edge_mask[..., None]
    B, N, C = node.shape
    M = B * N
    rows = lambda t: t.reshape(M, -1)  # noqa: E731
    nm, dm, valid = node_mask.reshape(M), diffuse.reshape(M), node_mask.reshape(M).bool()
    curr = OG.Frames.from_tensor_7(batch["rigids_t"].double().clone()).scale_translation(0.1)
    init = node
    nb = 0
    while f"{TR}ipa_{nb}.linear_q.weight" in sd:
        nb += 1

    def stage(name, b, fn, *a, **kw):
        tr = []
        out = fn(*a, trace=tr, **kw)
        if visit is not None:
            visit(name, b, tr, valid)
        return out

    for b in range(nb):
        w = RA.ipa_weights(sd, f"{TR}ipa_{b}.")
        bias = F.linear(edge, w["linear_b.weight"], w["linear_b.bias"]).permute(0, 3, 1, 2)
        pz = F.linear(edge, w["down_z.weight"], w["down_z.bias"])
        f = RA.ipa_features(w, node, bias, pz, curr.to_tensor_7(), node_mask)
        feats = torch.cat([f["o"], f["o_pt"], f["o_norm"], f["o_pair"]], dim=-1)
        if visit is not None:
            visit("feats", b, {k: rows(f[k]) for k in ("o", "o_pt", "o_norm", "o_pair")}, valid)
        x_ln = stage("linear_out", b, RN.linear_out, sd, b, rows(feats), rows(node), nm)
        skip = stage("skip_embed", b, RN.skip_embed, sd, b, rows(init))
        x = RN.transformer_input(x_ln, skip)
        if check:
            # (the attention sections are ref_attention's, held to the oracle by the attention suite: here to 1e-6; the node stage
            #  itself is held to the oracle's linear and LayerNorm on the same sections)
            emb = ON.ipa(sd, f"{TR}ipa_{b}", node, edge, curr, node_mask)
            _close(ON._lin(feats, sd, f"{TR}ipa_{b}.linear_out")[node_mask.bool()], emb[node_mask.bool()], ("attention sections", b), 1e-6)
            o_ln = ON._ln(node + ON._lin(feats, sd, f"{TR}ipa_{b}.linear_out") * node_mask[..., None], sd, f"{TR}ipa_ln_{b}")
            _close(x_ln, rows(o_ln), ("linear_out", b))
            _close(skip, rows(ON._lin(init, sd, f"{TR}skip_embed_{b}")), ("skip_embed", b))
            o_tr = ON.transformer_encoder(sd, f"{TR}transformer_{b}", torch.cat([o_ln, ON._lin(init, sd, f"{TR}skip_embed_{b}")], -1).transpose(0, 1),
                                          1.0 - node_mask, 4).transpose(0, 1)
        xx = x
        for l in range(RN.n_encoder_layers(sd, b)):
            qkv = stage("in_proj", b, RN.in_proj, sd, b, l, xx)
            sa = RA.encoder_attention(qkv, 1.0 - node_mask, B, N, 4)[0]
            _, xx = stage("post_attention", b, RN.post_attention, sd, b, l, xx, sa)
        s1 = stage("node_transition", b, RN.node_transition, sd, b, x_ln, xx, nm)
        upd = stage("backbone_update", b, RN.backbone_update, sd, b, s1, dm)
        if check:
            _close(xx[valid], rows(o_tr)[valid], ("transformer_encoder", b), 1e-9)
            o_n = ON.node_transition(sd, f"{TR}node_transition_{b}", o_ln + ON._lin(o_tr, sd, f"{TR}linear_{b}")) * node_mask[..., None]
            _close(s1[valid], rows(o_n)[valid], ("node_transition", b), 1e-9)
            assert bool((s1[~valid] == 0).all())
            _close(upd, rows(ON._lin(s1.view(B, N, C) * diffuse[..., None], sd, f"{TR}bb_update_{b}.linear")), ("backbone_update", b))
        node = s1.view(B, N, C)
        curr = curr.compose_q_update_vec(upd.view(B, N, 6), diffuse[..., None])
        if b < nb - 1:
            n_p, ab = stage("edge_node_parts", b, RN.edge_node_parts, sd, b, s1)
            p = f"{TR}edge_transition_{b}"
            if check:      # the oracle's first layer and final layer on [0 | n'_i | n'_j] and [0 | 0 | n'_j]: A_i + B_j, G_j (centred)
                o_np = ON._lin(node, sd, p + ".initial_embed")
                _close(n_p, rows(o_np), ("initial_embed", b))
                i, j = 3 % N, 7 % N
                z128 = o_np.new_zeros(B, 128)
                pre = ON._lin(torch.cat([z128, o_np[:, i], o_np[:, j]], -1), sd, p + ".trunk.0")
                A, Bc, G = ab.view(B, N, -1)[..., :384], ab.view(B, N, -1)[..., 384:768] / 32, ab.view(B, N, -1)[..., 768:] / 32
                _close(A[:, i] + Bc[:, j], pre, ("edge A_i + B_j", b))
                o_g = ON._lin(torch.cat([z128, z128, o_np[:, j]], -1), sd, p + ".final_layer")
                _close(G[:, j], o_g - o_g.mean(-1, keepdim=True), ("edge G_j, centred over the channels", b))
            edge = ON.edge_transition(sd, p, node, edge) * edge_mask[..., None]
    gt = batch["torsion_angles_sin_cos"][..., 2, :].double()
    u, psi = stage("torsion_head", nb, RN.torsion_head, sd, rows(node), rows(gt), fixed.reshape(M))
    if check:
        o_psi = ON.torsion_head(sd, RN.TORSION, node)
        _close(RN.torsion_normalise(u), rows(o_psi), "torsion_head", 1e-9)
    return psi.view(B, N, 2), curr.unscale_translation(0.1).to_tensor_7()


def test_ref_node_is_the_oracle_trunk_stage_by_stage():
    g = golden("net_b2n16.npz")
    psi, r7 = walk_trunk(synth_sd(0, 0.02), _batch(g))
    assert float((psi - T(g["psi"]).double()).abs().max()) < 2e-4
    assert float((r7 - T(g["rigids7"]).double()).abs().max()) < 2e-4


def test_generic_layer_is_the_written_contract():
    """layer == LayerNorm(residual + mask * relu(scale * x W^T + b)) * mask, against torch's own functions."""
    g = torch.Generator().manual_seed(4)
    M, K, n = 19, 64, 32
    x, w, b = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((M, K), (n, K), (n,)))
    sc, m = torch.rand(M, generator=g).double() + 0.5, (torch.rand(M, generator=g) > 0.3).double()
    res, ga, be = torch.randn(M, n + 8, generator=g).double(), torch.randn(n, generator=g).double(), torch.randn(n, generator=g).double()
    want = F.layer_norm(torch.relu(F.linear(x * sc[:, None], w) + b) * m[:, None] + res[:, :n], (n,), ga, be, 1e-5) * m[:, None]
    got = RN.layer(x, w, b, pre_scale=sc, relu=True, pre_mask=m, residual=res, ln=(ga, be, 1e-5), post_mask=m)
    assert float((got - want).abs().max()) < 1e-12
    assert RN.row_map_index(128, 64, 33).tolist() == [min(i, 32) for i in range(64)] + [33 + min(i, 32) for i in range(64)]


# ------------------------------------------------------------------------------------------------ the table's properties
def test_families_have_the_properties_they_are_named_for():
    hidden = []
    for M in NC.ROWS:
        d = NC.stage_inputs("trained-like", M)
        RN.node_transition(NC.trained_sd(), 0, d["s"], d["x_act"], d["mask"], hidden=hidden)
        tr = []
        RN.post_attention(NC.trained_sd(), 0, 0, d["x"], d["sa"], trace=tr)
        hidden.append(tr[1]["out"])
    amax = max(float(h.abs().max()) for h in hidden)
    print(f"trained-like hidden activations: up to {amax:.0f}")
    assert 1000.0 < amax < 2.0 ** 15
    for kind in NC.LN_KINDS:      # offset: rows c_row + N(0, 1), cancellation up to 30 : 1
        v = NC.layer_ref("offset", kind, 257)[0]["pre_ln"]
        ratio = v.mean(-1).abs() / v.std(-1)
        assert float(ratio.max()) > 20 and 0.8 < float(v.std(-1).mean()) < 1.2
    x = NC.layer_case("small", "skip", 33)["kw"]["x"]
    assert float(x[15].abs().max()) < 2.0 ** -12 and float(x[16].abs().max()) > 1.0
    kinds = set()
    for M in NC.ROWS:
        c, rec = NC.layer_case("masked", "linear_out", M), NC.layer_ref("masked", "linear_out", M)[0]
        m = c["kw"]["pre_mask"]
        kinds.add("all" if not m.any() else ("prefix" if not m[:(M + 1) // 2].any() else "isolated"))
        rows, want = NC.exact_rows(rec)
        assert torch.equal(rows, m == 0) and torch.equal(rec["out"][rows], want[rows])       # a masked linear_out row is beta, exactly
        rec = NC.layer_ref("masked", "nt3", M)[0]
        rows, want = NC.exact_rows(rec)
        assert torch.equal(rec["out"][rows], want[rows]) and float(want.abs().max()) == 0
        r = NC.layer_ref("masked", "l1", M)[0]
        dead = NC.layer_case("masked", "l1", M)["kw"]["x"].abs().amax(-1) == 0
        assert bool((r["out"][dead] == 0).all())      # every value in front of the ReLU negative
    assert kinds == {"all", "prefix", "isolated"}


# ------------------------------------------------------------------------------------------------ D32, the emulation, the crossover
def _emulated(flags=()):
    return RN.f16x3_layer(**{k: True for k in flags})


@pytest.mark.parametrize("family", NC.FAMILIES)
def test_emulated_planes_meet_the_bound_on_single_layers(family):
    E = _emulated()
    fails = []
    for fam, kind, ws in NC.layer_table():
        if fam != family:
            continue
        d32 = NC.layer_d32(fam, kind, ws)
        tag = f"{fam} {kind}" + (f" w x {ws:g}" if ws != 1.0 else "")
        record_margin(f"node D32 (float32 chain vs float64): {tag}", d32, NC.CAP if NC.capped(fam) else d32)
        for M in NC.ROWS:
            c, tr = NC.layer_case(fam, kind, M, ws), NC.layer_ref(fam, kind, M, ws)
            got = E(**c["kw"])
            a, b, r = NC.check_rows(got, tr[0], d32, NC.row_floor(tr), NC.capped(fam))
            record_margin(f"node f16x3 emulation vs float64: {tag}", a, b)
            record_margin(f"node f16x3 emulation vs float64: {tag} [achieved / bound]", a / b, 1.0)
            rows, want = NC.exact_rows(tr[0])
            if not (a < b and torch.equal(got[rows], want[rows])):
                fails.append((c["name"], a, b, r))
    assert not fails, fails


@pytest.mark.parametrize("family", NC.FAMILIES)
def test_emulated_planes_meet_the_bound_on_the_stages(family):
    E = _emulated()
    fails = []
    for stage in NC.STAGES:
        d32 = NC.stage_d32(family, stage)
        for name, i in NC.OUTPUTS[stage].items():
            record_margin(f"node D32 (float32 chain vs float64): {family} {stage}.{name}", d32[name], NC.CAP if NC.capped(family) else d32[name])
        for M in NC.ROWS:
            got, _ = NC.run_stage(stage, NC.sd_of(family), NC.stage_inputs(family, M), L=E)
            _, tr = NC.stage_ref(family, stage, M)
            for name, i in NC.OUTPUTS[stage].items():
                a, b, r = NC.check_rows(got[name], tr[i], d32[name], NC.row_floor(tr, i), NC.capped(family))
                record_margin(f"node f16x3 emulation vs float64: {family} {stage}.{name}", a, b)
                record_margin(f"node f16x3 emulation vs float64: {family} {stage}.{name} [achieved / bound]", a / b, 1.0)
                if not a < b:
                    fails.append((family, stage, name, M, a, b, r))
    assert not fails, fails


def test_small_inputs_need_the_format_floor():
    """On the small family the emulation leaves 3 x D32 from some input scale on -- and stays inside 3 x D32 + F at every scale."""
    E = _emulated()
    cross = {}
    for kind in ("skip", "in_proj", "nt3", "bb"):
        for ws in NC.W_SCALES:
            d32 = NC.layer_d32("small", kind, ws)
            worst = torch.zeros(16, dtype=torch.float64)
            for M in NC.ROWS:
                c, tr = NC.layer_case("small", kind, M, ws), NC.layer_ref("small", kind, M, ws)
                e = NC.row_errors(E(**c["kw"]), tr[0])
                assert bool((e <= 3 * d32 + NC.row_floor(tr)).all()), (c["name"],)
                for r in range(M):
                    worst[r % 16] = max(worst[r % 16], float(e[r]))
            over = [k for k in range(16) if worst[k] > 3 * d32]
            assert over and over[-1] == 15, (kind, ws, worst.tolist(), d32)
            cross[(kind, ws)] = over[0]
            print(f"small {kind} w x {ws:g}: 3 x D32 = {3 * d32:.2e} is exceeded from input scale 2^-{over[0]} on; at 2^-15: {float(worst[15]):.2e}")
            record_margin(f"node f16x3 emulation: first input scale 2^-k beyond 3 x D32: small {kind} w x {ws:g}", over[0], 15)
    assert all(0 < k for (kind, ws), k in cross.items() if ws == 1.0), cross     # O(1) inputs on unscaled weights stay inside 3 x D32


# ------------------------------------------------------------------------------------------------ footroom of the network
FOOTROOM = 5e-6


@pytest.mark.parametrize("style", ["init", "trained_like"])
def test_footroom_of_every_stage_of_the_network(style):
    """F / scale_row along one trunk evaluation at B = 2, N = 24 (the trained-like fixture's inputs), per stage and per plane-format
    input of the stage -- layer i of the stage reads input i as planes; its figure is that layer's own floor over the layer's scale --
    each asserted below 5e-6.  Also recorded, per layer output of a stage, the floor with the earlier layers' floors taken through
    |W| (the F of the parity bound).  That one is not held to 5e-6: it sums absolute values through 256- and 320-wide layers, which
    multiplies ANY relative error of an input -- a float32 rounding as well -- by sum |w| ~ 20 to 30 per layer, and says nothing about
    the format that it does not say about float32."""
    sd = synth_sd(0, 0.002) if style == "init" else NC.trained_sd()
    own, chained, share = {}, {}, {}

    def visit(stage, b, tr, valid):
        if stage == "feats":
            for k, v in tr.items():      # linear_out's input sections: the share of elements below the f16 pair's normal range
                share[k] = max(share.get(k, 0.0), float((v[valid].abs() < NC.X_LOW).double().mean()))
            return
        for i, rec in enumerate(tr):
            scale = NC.record_scale(rec)
            ok = valid & (scale > 0)
            if not bool(ok.any()):
                continue
            key = f"{stage}[{i}]"
            own[key] = max(own.get(key, 0.0), float(NC.row_floor([rec])[ok].max()))
            chained[key] = max(chained.get(key, 0.0), float(NC.row_floor(tr, i)[ok].max()))

    walk_trunk(sd, _batch(golden("net_b2n24_trained_like.npz")), visit, check=False)
    assert set(k.split("[")[0] for k in own) == set(NC.STAGES)
    for k, v in sorted(share.items()):
        print(f"footroom {style}: share of |x| < 0.25 in linear_out's input section {k}: {v:.3f}")
    fails = []
    for key in sorted(own):
        print(f"footroom {style} {key}: own input {own[key]:.3e}, with the stage's earlier layers {chained[key]:.3e}")
        record_margin(f"node footroom F / scale_row ({style}): {key} input", own[key], FOOTROOM)
        record_margin(f"node footroom, earlier layers taken along ({style}): {key}", chained[key], chained[key])
        if not own[key] < FOOTROOM:
            fails.append((key, own[key]))
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ planted mistakes
def _mistaken_layer(mistake):
    """ref_node.layer with one mistake planted in its epilogue."""
    def L(x, w, b=None, pre_scale=None, relu=False, pre_mask=None, residual=None, ln=None, post_mask=None, *, dtype=torch.float64, trace=None,
          matmul=RN.matmul):
        c = lambda t: None if t is None else t.to(dtype)  # noqa: E731
        x, w, b, pre_scale, pre_mask, residual, post_mask = (c(t) for t in (x, w, b, pre_scale, pre_mask, residual, post_mask))
        v = matmul(x, w).to(dtype)
        zero = torch.zeros((), dtype=dtype)
        ps = pre_scale[:, None] if pre_scale is not None else 1.0
        bb = b if b is not None else zero
        if mistake == "scale_after_bias":
            v = (v + bb) * ps
        elif mistake == "relu_before_bias" and relu:
            v = torch.relu(v * ps) + bb
        else:
            v = v * ps + bb
        if relu and mistake != "relu_before_bias":
            v = torch.relu(v)
        if pre_mask is not None and mistake != "pre_mask_after_residual":
            v = v * pre_mask[:, None]
        if residual is not None:
            v = v + residual[:, :w.shape[0]]
        if pre_mask is not None and mistake == "pre_mask_after_residual":
            v = v * pre_mask[:, None]
        if ln is not None:
            g, be, eps = c(ln[0]), c(ln[1]), ln[2]
            n = v.shape[-1]
            mean = v.mean(-1, keepdim=True)
            if mistake == "one_pass_variance":
                var = (v * v).mean(-1, keepdim=True) - mean * mean
            else:
                var = ((v - mean) ** 2).sum(-1, keepdim=True) / (n - 1 if mistake == "variance_over_n_minus_1" else n)
            v = (v - mean) / torch.sqrt(var + (eps * n if mistake == "eps_times_n" else eps)) * g + be
        if post_mask is not None:
            v = v * post_mask[:, None]
        return v
    return L


def _post_attention_wrong(which):
    def fn(sd, b, l, x, sa, dtype=torch.float64, L=RN.layer, trace=None):
        p = f"{TR}transformer_{b}.layers.{l}."
        pre = L(sa, *RN.lin(sd, p + "self_attn.out_proj"), residual=x, dtype=dtype)
        x1 = pre if which == "mid_ln_omitted" else RN.layer_norm(pre, *(t.to(dtype) for t in RN.ln_of(sd, p + "norm1")[:2]), 1e-5)
        h = L(x1, *RN.lin(sd, p + "linear1"), relu=True, dtype=dtype)
        res = pre if which == "norm2_residual_before_norm1" else x1
        return x1, L(h, *RN.lin(sd, p + "linear2"), residual=res, ln=RN.ln_of(sd, p + "norm2"), dtype=dtype)
    return fn


# mistake -> (the arithmetic it is evaluated in, the families it is looked for in)
EPILOGUE_MISTAKES = {"one_pass_variance": (torch.float32, ("offset",)), "variance_over_n_minus_1": (torch.float64, ("flat",)),
                     "eps_times_n": (torch.float64, ("flat", "masked")), "pre_mask_after_residual": (torch.float64, ("masked",)),
                     "scale_after_bias": (torch.float64, ("flat", "masked")), "relu_before_bias": (torch.float64, ("flat", "masked"))}
PLANE_MISTAKES = {"x_l_dropped": ("drop_xl",), "w_l_dropped": ("drop_wl",), "low_plane_subnormals_flushed": ("flush_subnormals",)}


def _exceeds_on_layers(L, dtype, families, floor):
    """Does layer function ``L`` leave the bound on some single-layer case of ``families``?  (The bound of the arithmetic ``L`` stands
    for: 3 x D32, + F where it is the plane arithmetic.)"""
    hits = []
    for fam, kind, ws in NC.layer_table():
        if fam not in families:
            continue
        d32 = NC.layer_d32(fam, kind, ws)
        for M in NC.ROWS:
            c, tr = NC.layer_case(fam, kind, M, ws), NC.layer_ref(fam, kind, M, ws)
            got = L(**c["kw"], dtype=dtype)
            a, b, _ = NC.check_rows(got, tr[0], d32, NC.row_floor(tr) if floor else None, NC.capped(fam))
            rows, want = NC.exact_rows(tr[0])
            if not a < b or not torch.equal(got.double()[rows], want[rows]):
                hits.append((c["name"], a, b))
    return hits


@pytest.mark.parametrize("mistake", list(EPILOGUE_MISTAKES))
def test_planted_epilogue_mistake_exceeds_the_bound(mistake):
    dtype, families = EPILOGUE_MISTAKES[mistake]
    assert not _exceeds_on_layers(RN.layer, dtype, families, False)          # (the same evaluation without the mistake is inside)
    hits = _exceeds_on_layers(_mistaken_layer(mistake), dtype, families, False)
    print(mistake, len(hits), hits[:3])
    assert hits


@pytest.mark.parametrize("mistake", list(PLANE_MISTAKES))
def test_planted_plane_mistake_exceeds_the_bound(mistake):
    hits = _exceeds_on_layers(_emulated(PLANE_MISTAKES[mistake]), torch.float64, NC.FAMILIES, True)
    print(mistake, len(hits), hits[:3])
    assert hits
    if mistake == "low_plane_subnormals_flushed":
        assert any(n.startswith("small") for n, _, _ in hits)


@pytest.mark.parametrize("mistake", ["mid_ln_omitted", "norm2_residual_before_norm1"])
def test_planted_chain_mistake_exceeds_the_bound(mistake):
    fn, hits = _post_attention_wrong(mistake), []
    for family in ("flat", "trained-like"):
        d32 = NC.stage_d32(family, "post_attention")["x2"]
        for M in NC.ROWS:
            d = NC.stage_inputs(family, M)
            _, tr = NC.stage_ref(family, "post_attention", M)
            _, got = fn(NC.sd_of(family), 0, 0, d["x"], d["sa"])
            a, b, _ = NC.check_rows(got, tr[2], d32, NC.row_floor(tr, 2), NC.capped(family))
            if not a < b:
                hits.append((family, M, a, b))
    assert hits


def test_planted_row_map_mistake_exceeds_the_bound():
    """Padded rows taken from the next sample instead of repeating the sample's last row."""
    hits = []
    for N, (n_pad, n_src) in NC.ROW_MAPS.items():
        samples = 3
        c = NC.layer_case("flat", "skip", NC.ROWS[-1])
        x = c["kw"]["x"][:samples * n_src]
        rows = samples * n_pad
        idx = RN.row_map_index(rows, n_pad, n_src)
        r = torch.arange(rows)
        wrong = torch.clamp((r // n_pad) * n_src + r % n_pad, max=samples * n_src - 1)
        tr = []
        RN.layer(x[idx], c["kw"]["w"], c["kw"]["b"], trace=tr)
        got = RN.layer(x[wrong], c["kw"]["w"], c["kw"]["b"])
        a, b, _ = NC.check_rows(got, tr[0], NC.layer_d32("flat", "skip"), NC.row_floor(tr), True)
        assert torch.equal(tr[0]["out"].view(samples, n_pad, -1)[:, n_src:], tr[0]["out"].view(samples, n_pad, -1)[:, n_src - 1:n_src].expand(-1, n_pad - n_src, -1))
        if not a < b:
            hits.append((N, a, b))
    assert len(hits) == len(NC.ROW_MAPS), hits
