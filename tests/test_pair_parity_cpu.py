"""What the pair-stream parity suite (tests/test_pair_parity.py) rests on, checked without a GPU:

  * tests/ref_pair.py in float64 is the reference's EdgeTransition (oracle/net.py::edge_transition) and meets its golden output
    (tests/golden/edge_transition.npz); the per-node-parts form equals the (node, edge) form;
  * the families of tests/pair_cases.py have the properties they are named for, the shapes the tile arithmetic they were chosen for;
  * D32 -- the float32 chain's distance from float64 under the per-pair measure -- for every (family, level), recorded; below the
    cap for flat and offset, so the reference alone stays within it;
  * r16 -- the share of the a-priori floor F that the CPU emulation of the f16 planes uses -- for every (family, level), recorded and
    at most 1 (F does bound the format);
  * the emulation meets 3 x D32 + min(1, 3 x r16) x F on every family at the shapes up to (2, 37), and on the small family exceeds
    3 x D32 alone: the F term is needed;
  * every planted mistake exceeds the bound on some case; a low plane dropped (x_l, W_l) or its subnormals flushed in ANY ONE of the
    eight layers of a module-level evaluation (n', A, B, G, layer 1, layer 2, final, projection) or of the four of a parts-level one
    exceeds it at that level.  (Under 3 x D32 + F, the rule before r16, every one of them passed at the module level: the weakest
    stage's error / bound under both rules is recorded.)
"""
import functools

import pytest
import torch

import node_cases as NC
import pair_cases as PC
import ref_node as RN
import ref_pair as RP
from conftest import T, golden, record_margin, synth_sd
from test_node_parity_cpu import _close


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


# ------------------------------------------------------------------------------------------------ the reference
def test_ref_pair_is_the_oracle_edge_transition_and_meets_the_golden_output():
    from oracle import net as ON

    sd32 = synth_sd(0, 0.02)
    sd = {k: v.double() for k, v in sd32.items() if k.startswith(PC.ET)}
    g = golden("edge_transition.npz")
    node, edge = T(g["node"]).double(), T(g["edge"]).double()
    want = ON.edge_transition(sd, PC.ET[:-1], node, edge)
    got = RP.edge_transition(sd, PC.ET, edge, s=node)
    _close(got, want, "ref_pair from (node, edge) vs the oracle")
    assert float((got - T(g["out"]).double()).abs().max() / T(g["out"]).abs().max()) < 5e-6      # (the golden output is the float32 reference's)
    B, N = node.shape[:2]
    n_p, ab = RN.edge_node_parts(sd, None, node.reshape(B * N, -1), prefix=PC.ET)
    ab = torch.cat([ab[:, :384], ab[:, 384:] / 32.0], dim=-1)
    mask = (torch.rand(B, N, generator=torch.Generator().manual_seed(5)) > 0.3).double()
    from_parts = RP.edge_transition(sd, PC.ET, edge, mask, parts=(n_p.view(B, N, -1), ab.view(B, N, -1)))
    _close(from_parts, want * (mask[:, :, None] * mask[:, None, :])[..., None], "ref_pair from the per-node parts vs the oracle, masked")
    # the parts with an uncentred G_j (the formula of the reference, layers.py:181) give the same result: the LayerNorm removes the mean
    wf, bf = RN.lin(sd, PC.ET + "final_layer")
    ab2 = ab.clone()
    ab2[:, 768:] = n_p @ wf[:, 256:].t() + bf
    assert float((ab2[:, 768:] - ab[:, 768:]).abs().max()) > 1e-4
    _close(RP.edge_transition(sd, PC.ET, edge, parts=(n_p.view(B, N, -1), ab2.view(B, N, -1))), want, "uncentred G_j")


# ------------------------------------------------------------------------------------------------ the table's properties
def test_shapes_have_the_tile_arithmetic_they_were_chosen_for():
    assert PC.tiles(3, 7) == (147, 2, 19, 5, 19)                      # a partial second 128-pair tile, a partial 32-pair block
    assert PC.tiles(1, 190) == (36100, 283, 4, 1129, 4) and 283 > 256   # more tiles than CUs; the last tile holds 4 pairs
    assert [N < 32 for _, N in PC.SHAPES[:4]] == [True] * 4 and [N >= 32 for _, N in PC.SHAPES[4:7]] == [True] * 3
    assert PC.SPLITS[(5, 24)] // (24 * 24) == 2 and PC.SPLITS[(20, 6)] // 36 == 10
    assert PC.tiles(1, 1)[0] == 1 and PC.tiles(1, 2)[0] == 4


def test_families_have_the_properties_they_are_named_for():
    kinds, negative = set(), 0
    for shape in PC.SHAPES:
        B, N = shape
        for level in PC.LEVELS:
            tr = PC.ref("trained-like", shape, level)[2]
            hmax = max(max(float(t[-4]["out"].abs().max()), float(t[-2]["x"].abs().max())) for t in tr)
            if B * N * N >= 147:          # (the largest of a handful of values says little)
                assert 2000.0 <= hmax < 2.0 ** 15, (shape, hmax)
            assert hmax < 2.0 ** 15
        for fam in ("offset-G", "offset-W"):
            r = PC.offset_ratio(PC.case(fam, shape), PC.levels(fam)[0])
            assert float(r.max()) <= NC.OFFSET and float((r >= 20).double().mean()) >= 0.1, (fam, shape, float(r.max()))
        c = PC.case("small", shape)
        M = B * N * N
        assert float(c["sd"][PC.ET + "final_layer.bias"].abs().max()) == 0
        if M > 16:
            assert float(c["edge"].reshape(M, -1)[15].abs().max()) < 2.0 ** -12 and float(c["edge"].reshape(M, -1)[16].abs().max()) > 1.0
        c = PC.case("masked", shape)
        m = c["mask"].reshape(-1)
        kinds.add("all" if not m.any() else ("prefix" if not m[:(B * N + 1) // 2].any() else "isolated"))
        out, proj, tr = PC.ref("masked", shape, "parts")
        dead = torch.cat([PC.masked_rows(t[-2]) for t in tr])
        ii, jj = RP.pair_index(B, N)
        assert torch.equal(dead, (m[ii] * m[jj]) == 0) and float(out[dead].abs().max() if dead.any() else 0.0) == 0
        bias = torch.cat([c["sd"][PC.IPA1 + ".linear_b.bias"], c["sd"][PC.IPA1 + ".down_z.bias"]]).double()
        assert torch.equal(proj[dead], bias.expand(int(dead.sum()), -1))      # the projection of a zero vector: its bias
        for t in tr:      # pairs whose every layer-1 and layer-2 pre-activation is negative: both hidden layers are zero
            negative += int(((t[-4]["out"] == 0).all(-1) & (t[-3]["out"] == 0).all(-1) & ~PC.masked_rows(t[-2])).sum())
        for e in PC.EXPS:
            tr = PC.ref(f"exp{e}", shape, "module")[2]
            hmax = max(max(float(t[-4]["out"].abs().max()), float(t[-2]["x"].abs().max())) for t in tr)
            # (e = 15: inputs below 2^14 and 2^5 w below 2^15.5 leave the hidden maximum near 2^27; still 2^(15 + e - 5) and beyond)
            assert 2.0 ** ((13 if e < 15 else 11) + e) <= hmax < 2.0 ** (15 + e), (e, shape, hmax)
            c = PC.case(f"exp{e}", shape)
            assert max(float(c["edge"].abs().max()), float(c["s"].abs().max()), float(c["parts"][0].abs().max())) <= 2.0 ** 14 + 1
            assert 32.0 * float(c["sd"][PC.ET + "trunk.0.weight"].abs().max()) < 2.0 ** 15.6
            assert tr[0][-2]["exp"] == e and tr[0][-3]["exp"] == e and "exp" not in tr[0][-4]
    assert kinds == {"all", "prefix", "isolated"} and negative > 0


# ------------------------------------------------------------------------------------------------ D32, the emulation
@pytest.mark.parametrize("family", PC.FAMILIES)
def test_d32_is_recorded_and_below_the_cap_where_capped(family):
    for level in PC.levels(family):
        d = PC.d32(family, level)
        for o in PC.OUTPUTS:
            print(f"pair D32 {family} {level} {o}: {d[o]:.3e}")
            record_margin(f"pair D32 (float32 chain vs float64): {family} {level} {o}", d[o], NC.CAP if PC.capped(family) else d[o])
            if PC.capped(family):
                assert d[o] < NC.CAP, (family, level, o, d[o])


@pytest.mark.parametrize("family", PC.FAMILIES)
def test_r16_is_recorded_and_at_most_one(family):
    """r16 = the largest error / F of the plane emulation (three plane products accumulated in float64: the format's loss alone):
    F is an a-priori bound of exactly that, so r16 <= 1; the bound rule takes min(1, 3 x r16) of F."""
    for level in PC.levels(family):
        r = PC.r16(family, level)
        for o in PC.OUTPUTS:
            print(f"pair r16 {family} {level} {o}: {r[o]:.3e} (share of F in the bound: {PC.floor_share(family, level, o):.3e})")
            record_margin(f"pair r16 (plane emulation's error / F): {family} {level} {o}", r[o], 1.0)
            assert 0.0 < r[o] <= 1.0, (family, level, o, r[o])


def test_embed_r16_is_recorded_and_at_most_one():
    """The same share for the edge embedding's last two layers (pair_cases.embed_r16), whose bound takes min(1, 3 x r16) of their F."""
    r = PC.embed_r16()
    print(f"pair r16 edge embedding, offset rows: {r:.3e}")
    record_margin("pair r16 (plane emulation's error / F): edge embedding, offset rows", r, 1.0)
    assert 0.0 < r <= 1.0, r


@pytest.mark.parametrize("family", PC.FAMILIES)
def test_emulated_planes_meet_the_bound(family):
    fails, over = [], 0
    for level in PC.levels(family):
        d = PC.d32(family, level)
        for shape in PC.SMALL_SHAPES:
            out, proj = PC.emulated(family, shape, level)
            traces = PC.ref(family, shape, level)[2]
            for o, got in (("out", out), ("proj", proj)):
                a, b, r, exact = PC.check(got, traces, o, family, d[o])
                record_margin(f"pair f16x3 emulation vs float64: {family} {level} {o}", a, b)
                if not (a < b and exact):
                    fails.append((family, level, shape, o, a, b, r, exact))
                over += int(PC.check(got, traces, o, family, d[o], arith="f32")[0] >= 3 * d[o])
    assert not fails, fails
    if family == "small":
        assert over > 0          # without F the small family exceeds: F is needed


# ------------------------------------------------------------------------------------------------ planted mistakes
def _plain_mean_layer(x, w, b=None, relu=False, ln=None, post_mask=None, *, dtype=torch.float32, trace=None, **kw):
    """ref_node.layer in float32 with the LayerNorm written as the pair kernels write it: the mean from one running sum over the
    channels, left to right, then the variance of the deviations from it -- no correction of the mean."""
    v = RN.layer(x, w, b, relu=relu, dtype=dtype, **kw)
    if ln is not None:
        acc = v[:, 0].clone()
        for k in range(1, v.shape[1]):
            acc = acc + v[:, k]
        d = v - (acc * (1.0 / v.shape[1]))[:, None]
        var = d[:, 0] * d[:, 0]
        for k in range(1, v.shape[1]):
            var = var + d[:, k] * d[:, k]
        v = d * (1.0 / torch.sqrt(var * (1.0 / v.shape[1]) + ln[2]))[:, None] * ln[0].to(dtype) + ln[1].to(dtype)
    if post_mask is not None:
        v = v * post_mask.to(dtype)[:, None]
    return v


# mistake -> (families it is looked for in, keyword arguments of pair_cases.run)
MISTAKES = {"ij_swapped": (("flat",), dict(wrong="ij_swapped")),
            "b2_dropped": (("trained-like", "flat"), dict(wrong="b2_dropped")),
            "residual_from_h1": (("flat",), dict(wrong="residual_from_h1")),
            "j_residual_missing": (("flat",), dict(wrong="j_residual_missing")),
            "mask_i_only": (("masked",), dict(wrong="mask_i_only")),
            "plain_mean_float32": (("offset-G", "offset-W"), dict(dtype=torch.float32, L=_plain_mean_layer)),
            "attn_bias_pair_major": (("flat",), dict(wrong="attn_bias_pair_major")),
            "projection_of_unmasked_row": (("masked",), dict(wrong="projection_of_unmasked_row")),
            "x_l_dropped": (("flat", "trained-like"), "drop_xl"),
            "w_l_dropped": (("flat", "trained-like"), "drop_wl"),
            "low_plane_subnormals_flushed": (("small",), "flush_subnormals"),
            "ragged_last_pair_from_neighbour": (("flat",), dict(wrong="ragged_last_pair_from_neighbour"))}
PLANE_MISTAKES = tuple(m for m, (_, how) in MISTAKES.items() if isinstance(how, str))
MISTAKE_SHAPES = ((3, 7), (2, 37))


@pytest.mark.parametrize("mistake", list(MISTAKES))
def test_planted_mistake_exceeds_the_bound(mistake):
    """The mistake in every layer it can be made in.  A plane mistake must show in every family it is looked for in at BOTH levels (a
    hit at the parts level says nothing about the module level, whose F starts four layers earlier)."""
    families, how = MISTAKES[mistake]
    hits = []
    for family in families:
        for level in PC.levels(family):
            d = PC.d32(family, level)
            n0 = len(hits)
            for shape in MISTAKE_SHAPES:
                c = PC.case(family, shape)
                kw = PC.emulation(c, level, (how,)) if isinstance(how, str) else how
                out, proj, _ = PC.run(c, level, **kw)
                traces = PC.ref(family, shape, level)[2]
                for o, got in (("out", out), ("proj", proj)):
                    a, b, r, exact = PC.check(got, traces, o, family, d[o], arith="f16x3" if isinstance(how, str) else "f32")
                    if not (a < b and exact):
                        hits.append((family, level, shape, o, a, b))
            assert len(hits) > n0 or not isinstance(how, str), (mistake, family, level, "passes the bound")
    print(mistake, len(hits), hits[:3])
    assert hits


@functools.lru_cache(maxsize=None)
def _one_layer_ratio(mistake, family, level, stage):
    """{rule: the largest error / bound over MISTAKE_SHAPES and both outputs} of the plane emulation with ``mistake`` in layer ``stage``
    alone, judged as the GPU tests judge a kernel ("measured"), and with the whole a-priori F as before r16 ("a-priori")."""
    d, best = PC.d32(family, level), {"measured": 0.0, "a-priori": 0.0}
    for shape in MISTAKE_SHAPES:
        c = PC.case(family, shape)
        out, proj, _ = PC.run(c, level, **PC.emulation(c, level, (MISTAKES[mistake][1],), stage))
        traces = PC.ref(family, shape, level)[2]
        for o, got in (("out", out), ("proj", proj)):
            for rule in best:
                j = PC.judged(got, traces, o, family, d[o], rule=rule)
                best[rule] = max(best[rule], j["achieved"] / j["bound"])
    return best


@pytest.mark.parametrize("mistake, level, stage", [(m, lv, st) for m in PLANE_MISTAKES for lv in PC.LEVELS for st in PC.stages(lv)])
def test_plane_mistake_in_one_layer_exceeds_the_bound(mistake, level, stage):
    """A low plane lost in ONE layer (the realistic kernel mistake: one MFMA of one stage without its x_l or W_l operand, one
    conversion that flushes) must leave the bound at the level it is made at, in every family it is looked for in, on (3, 7) or
    (2, 37), in at least one output.  (exp10 is not among the families: its hidden activations of 2^23 dwarf what two of the per-node
    layers lose; that family is there for the block exponent.)"""
    for family in MISTAKES[mistake][0]:
        r = _one_layer_ratio(mistake, family, level, stage)
        print(f"{mistake} in {stage}, {family} {level}: error / bound {r['measured']:.3g} (with the whole F: {r['a-priori']:.3g})")
        assert r["measured"] > 1.0, (mistake, family, level, stage, r)


@pytest.mark.parametrize("mistake, level", [(m, lv) for m in PLANE_MISTAKES for lv in PC.LEVELS])
def test_weakest_stage_of_a_plane_mistake_is_recorded(mistake, level):
    """error / bound of the stage at which the mistake shows least, per family: under the bound rule, and under 3 x D32 + F.  A dropped
    plane is recorded for offset-W and masked as well (not asserted: the per-layer requirement is on flat and trained-like)."""
    required = MISTAKES[mistake][0]
    extra = tuple(f for f in ("offset-W", "masked") if mistake != "low_plane_subnormals_flushed" and level in PC.levels(f))
    for family in required + extra:
        per = {st: _one_layer_ratio(mistake, family, level, st) for st in PC.stages(level)}
        for rule in ("measured", "a-priori"):
            st = min(per, key=lambda s: per[s][rule])
            n_pass = sum(per[s][rule] <= 1.0 for s in per)
            print(f"{mistake} {family} {level}, {rule} F: weakest stage {st} at {per[st][rule]:.3g}; {n_pass} of {len(per)} stages pass")
            # (a mistake: "achieved" above the "bound" of 1 is what is wanted here)
            record_margin(f"pair plane mistake in one layer, weakest stage [error / bound, {rule} F]: {mistake} {family} {level}",
                          per[st][rule], 1.0)
        assert family in extra or min(per[s]["measured"] for s in per) > 1.0


def test_ln_eps_must_follow_the_block_exponent_on_ordinary_magnitudes():
    """The kernel normalises 2^-e y; with ln_eps left unscaled an ordinary row (variance of y around 1) is visibly wrong at e = 5."""
    c = dict(PC.case("flat", (3, 7)), exp=5)
    out, _, _ = PC.run(c, "parts", wrong="ln_eps_unscaled")
    a, b, _, _ = PC.check(out, PC.ref("flat", (3, 7), "parts")[2], "out", "flat", PC.d32("flat", "parts")["out"], arith="f32")
    assert a > 10 * b, (a, b)


def test_embed_offset_case_meets_the_offset_condition():
    for shape in PC.EMB_SHAPES:
        r = PC.embed_offset_case(shape)["ratio"]
        assert float(r.max()) <= NC.OFFSET and float((r >= 20).double().mean()) >= 0.1, (shape, float(r.max()))
