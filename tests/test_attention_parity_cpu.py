"""What the attention parity suite (tests/test_attention_parity.py) rests on, checked without a GPU: the formulas of
tests/ref_attention.py are the reference's (oracle.net.ipa, the ipa.npz fixture, torch.nn.MultiheadAttention), the case table of
tests/attention_cases.py has the properties its families are named for, the bounds are printed with the chain distances they are
3 x of, and each planted mistake of ref_attention.MUTATIONS exceeds the bound on some case of the table.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import attention_cases as AC
import ref_attention as RA
from conftest import T, golden, synth_sd

BLOCK = "translator.trunk.ipa_2."


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module")
def weights():
    return RA.ipa_weights(synth_sd(0, 0.02), BLOCK)


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / max(1.0, float(b.double().abs().max())))


def _pair_proj(w, z):
    return F.linear(z, w["linear_b.weight"], w["linear_b.bias"]).permute(0, 3, 1, 2), F.linear(z, w["down_z.weight"], w["down_z.bias"])


# ------------------------------------------------------------------------------------------------ the formulas are the reference's
def test_float32_features_through_linear_out_reproduce_the_oracle(weights):
    from oracle import geometry as OG
    from oracle import net as ON

    sd = synth_sd(0, 0.02)
    g = torch.Generator().manual_seed(233)
    B, N = 2, 41
    s, z = torch.randn(B, N, 256, generator=g), torch.randn(B, N, N, 128, generator=g)
    q = torch.randn(B, N, 4, generator=g)
    r7 = torch.cat([q / q.norm(dim=-1, keepdim=True), torch.randn(B, N, 3, generator=g)], -1)
    mask = torch.ones(B, N)
    mask[1, 5:9] = 0
    ref = ON.ipa(sd, BLOCK[:-1], s, z, OG.Frames.from_tensor_7(r7), mask)
    bias, pz = _pair_proj(weights, z)
    for dtype, tol in ((torch.float32, 2e-6), (torch.float64, 2e-6)):
        f = RA.ipa_features(weights, s, bias, pz, r7, mask, dtype=dtype)
        err = rel(RA.ipa_linear_out(weights, f, dtype)[mask.bool()], ref[mask.bool()])
        print(f"ipa_features {dtype} -> linear_out vs oracle.net.ipa: {err:.3e}")
        assert err < tol
    assert f["o"].shape == (B, N, 2048) and f["as"].shape == (B, N, 2048) and f["o_pt"].shape == (B, N, 288)
    assert f["o_norm"].shape == (B, N, 96) and f["o_pair"].shape == (B, N, 256) and f["probs"].shape == (B, 8, N, N)


def test_float32_features_through_linear_out_reproduce_the_golden_block():
    g = golden("ipa.npz")
    w = RA.ipa_weights(synth_sd(0, 0.02), "translator.trunk.ipa_0.")
    bias, pz = _pair_proj(w, T(g["z"]))
    f = RA.ipa_features(w, T(g["s"]), bias, pz, T(g["rigids7"]), T(g["mask"]), dtype=torch.float32)
    valid = T(g["mask"]).bool()
    err = rel(RA.ipa_linear_out(w, f)[valid], T(g["out"])[valid])
    print(f"ipa_features float32 -> linear_out vs tests/golden/ipa.npz: {err:.3e}")
    assert err < 2e-6


def test_folded_columns_carry_the_same_information(weights):
    """``as`` is what the folded path hands to linear_out in place of ``o``: W_v (sum_j a_ij s_j) + b_v = o, per head."""
    c = AC.case("peaked", 33)
    f = RA.ipa_features(weights, *AC.ipa_inputs(c))
    B, N = c["B"], c["N"]
    wv = weights["linear_kv.weight"].double().view(8, 2, 256, 256)[:, 1]
    bv = weights["linear_kv.bias"].double().view(8, 2, 256)[:, 1]
    o = torch.einsum("hca,bnha->bnhc", wv, f["as"].view(B, N, 8, 256)) + bv
    assert AC.section_error(o.reshape(B, N, -1), f["o"], c["mask"]) < 1e-12


@pytest.mark.parametrize("kind", ["none", "float", "inf"])
def test_encoder_attention_float64_is_torch_multihead_attention(kind):
    B, N, D, heads = 3, 45, AC.ENC_D, AC.ENC_HEADS
    torch.manual_seed(5)
    mha = torch.nn.MultiheadAttention(D, heads).double()
    mha.in_proj_weight.normal_(0, 0.1)
    mha.in_proj_bias.normal_(0, 0.1)
    mha.out_proj.weight.copy_(torch.eye(D))
    mha.out_proj.bias.zero_()
    x = torch.randn(N, B, D, dtype=torch.float64)
    kb = None
    if kind == "float":
        kb = (torch.rand(B, N) < 0.3).double()
    elif kind == "inf":
        kb = torch.zeros(B, N, dtype=torch.float64)
        kb[0, 40:], kb[1, :32], kb[2, 1:] = float("-inf"), float("-inf"), float("-inf")
    ref = mha(x, x, x, key_padding_mask=kb, need_weights=False)[0].transpose(0, 1).reshape(B * N, D)
    qkv = F.linear(x.transpose(0, 1).reshape(B * N, D), mha.in_proj_weight, mha.in_proj_bias)
    got = RA.encoder_attention(qkv, kb, B, N, heads, torch.float64)[0]
    assert float((got - ref).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------ the table's properties
def _row_stats(weights, c):
    """Over the valid query rows x heads of a case: (row maximum of the probabilities, logit span over the valid keys, arg-max key)."""
    f = RA.ipa_features(weights, *AC.ipa_inputs(c))
    valid = c["mask"].bool()
    p = f["probs"].permute(0, 2, 1, 3)[valid]                          # [rows, H, N]
    lg = f["logits"].permute(0, 2, 1, 3)[valid]
    km = c["mask"][:, None, None, :].expand(-1, c["N"], 8, -1)[valid].bool()
    assert bool(km.any(-1).all()), (c["name"], "a valid row without a valid key")
    assert bool((lg.amax(-1) > -1e4).all())
    big = torch.full_like(lg, 1e30)
    span = torch.where(km, lg, -big).amax(-1) - torch.where(km, lg, big).amin(-1)
    return p.amax(-1).flatten(), span.flatten(), p.argmax(-1).flatten()


def test_table_properties_and_chain_distances(weights):
    for family in AC.FAMILIES:
        d = AC.pooled_chain_distance(weights, family)
        print(f"{family}: pooled float32 chain distance " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
        print(f"{family}: bound                          " + ", ".join(f"{k} {AC.bound(weights, family, k):.2e}" for k in RA.SECTIONS))
        for k in RA.SECTIONS:
            assert 0 < AC.bound(weights, family, k) <= 3.0 * d[k]
            assert AC.base_family(family) != "flat" or AC.bound(weights, family, k) <= AC.CAP
    for family in ("flat", "peaked"):
        rows = []
        for N in AC.LENGTHS:
            c = AC.case(family, N)
            assert len(set(c["kinds"])) == c["B"], "every sample of a batch has a mask of another kind"
            pmax, span, arg = _row_stats(weights, c)
            tiles = sorted(set((arg // AC.TILE).tolist()))
            print(f"{c['name']} masks {c['kinds']}: median row max {float(pmax.median()):.3f}, span > 88 in "
                  f"{float((span > 88).float().mean()):.2f} of the rows, arg-max key tiles {tiles}")
            rows.append((pmax, span))
            if family == "peaked":
                assert tiles == list(range((N + AC.TILE - 1) // AC.TILE)), (c["name"], "the arg-max key misses a key tile", tiles)
                assert float(pmax.median()) > 0.9, c["name"]
            elif N >= 32:
                assert float(pmax.median()) < 0.3, c["name"]
        pmax, span = (torch.cat(x) for x in zip(*rows))
        if family == "peaked":
            assert float(pmax.median()) > 0.9 and float((span > 88).float().mean()) >= 0.25
        else:
            assert float(pmax.median()) < 0.3 and float(span.max()) < 88
    kinds = {k for f in ("flat", "peaked") for N in AC.LENGTHS for k in AC.case(f, N)["kinds"]}
    assert kinds == set(AC.MASK_KINDS)


@pytest.mark.parametrize("base", ["flat", "peaked"])
def test_moved_cases_are_the_same_operation(weights, base):
    """In float64, on the frames before they are rounded to float32: the features of a moved case are those of its base case."""
    worst = 0.0
    for N in AC.LENGTHS:
        c, m = AC.case(base, N), AC.case("moved-" + base, N)
        for k in ("s", "bias", "pz", "mask"):
            assert torch.equal(c[k], m[k])
        centre = m["r7_64"][..., 4:].mean(dim=1).norm(dim=-1)
        assert bool(((centre - AC.MOVE).abs() < 1e-9).all()) and float(c["r7_64"][..., 4:].mean(dim=1).abs().max()) < 1e-12
        f0 = RA.ipa_features(weights, *AC.ipa_inputs(c, r7=c["r7_64"]))
        f1 = RA.ipa_features(weights, *AC.ipa_inputs(m, r7=m["r7_64"]))
        for k in RA.SECTIONS:
            e = AC.section_error(f1[k], f0[k], c["mask"])
            worst = max(worst, 0.0 if math.isnan(e) else e)
    print(f"moved-{base} vs {base}, float64: {worst:.3e}")
    assert worst < 1e-12


def test_encoder_table_properties_and_chain_distances():
    for family in AC.ENC_FAMILIES:
        print(f"encoder {family}: pooled float32 chain distance {AC.encoder_pooled_chain_distance(family):.2e}, bound {AC.encoder_bound(family):.2e}")
        assert 0 < AC.encoder_bound(family) <= 3.0 * AC.encoder_pooled_chain_distance(family)
        for N in AC.ENC_LENGTHS:
            for kind in AC.ENC_BIAS:
                _, lg, p = AC.encoder_ref(family, N, kind, torch.float64)
                assert bool(torch.isfinite(lg).any(-1).all()), "every row keeps a key"
            _, _, p = AC.encoder_ref(family, N, "none", torch.float64)
            last = float((p.argmax(-1) >= (N - 1) // AC.TILE * AC.TILE).float().mean())
            print(f"encoder {family} N={N}: median row max {float(p.amax(-1).median()):.3f}, arg-max in the last key tile for {last:.2f} of the rows")
            if family == "peaked":
                assert float(p.amax(-1).median()) > 0.9 and last >= 0.4
            elif N >= 31:
                assert float(p.amax(-1).median()) < 0.3
    assert AC.encoder_bound("flat") <= AC.CAP
    kb = AC.encoder_case("flat", 130, "inf-prefix")["key_bias"]
    assert bool((kb[1, 64:] == float("-inf")).all()) and bool((kb[2, 1:] == float("-inf")).all())      # whole trailing tiles masked
    assert bool((AC.encoder_case("flat", 130, "inf-first-tile")["key_bias"][:, :32] == float("-inf")).all())


# ------------------------------------------------------------------------------------------------ the bounds catch the mistakes
@pytest.mark.parametrize("mutation", RA.MUTATIONS)
def test_each_planted_mistake_exceeds_the_bound_somewhere(weights, mutation):
    """The reference with one mistake of a pipelined kernel planted, against the unmutated reference, both in float64: on at least
    one case of the table some section is further off than the family's bound (or not finite)."""
    for family in ("peaked", "flat"):
        for N in reversed(AC.LENGTHS):
            c = AC.case(family, N)
            ref = AC.features64(weights, c)
            mut = RA.ipa_features(weights, *AC.ipa_inputs(c), mutate=mutation)
            for k in RA.SECTIONS:
                valid = c["mask"].bool()
                e = AC.section_error(mut[k], ref[k], c["mask"]) if bool(torch.isfinite(mut[k][valid]).all()) else float("inf")
                if e > AC.bound(weights, family, k):
                    print(f"{mutation}: {c['name']} {k} off by {e:.3e} (bound {AC.bound(weights, family, k):.3e})")
                    return
    raise AssertionError(f"{mutation} stays within the bounds on every case of the table")
