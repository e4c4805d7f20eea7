"""The float64 embedder reference (tests/ref_embed.py) and the case table (tests/embed_cases.py) checked on the CPU, before the
MI355X sees them (tests/test_embedding_parity.py): the reference against the reference-generated fixture, the product's first-layer
feature functions against the oracle's bit for bit, the distance e_ref of the float32 chain from float64 that the GPU bound is
3 x of, the edge clearance of every case, the expected-bin table of the exact-edge case, and the proof that the bound separates
right from wrong -- every planted mutation of the reference sits at least 10 x the GPU bound away from the unmutated float32 chain.
"""
import pytest
import torch

import embed_cases as EC
import ref_embed
from conftest import T, golden, record_margin, synth_sd
from oracle import net as ON


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module")
def sd():
    return synth_sd(0, 0.02)


def check(name, achieved, bound):
    record_margin(name, achieved, bound)
    assert achieved < bound, (name, achieved, bound)


def test_embedding64_matches_the_reference_fixture(sd):
    """embedding.npz holds the reference's own node and edge embedding (float32) of B = 2, N = 16 with the synthetic weights;
    bound: the project's per-op 5e-6 of the output scale."""
    g = golden("embedding.npz")
    node, edge = ref_embed.embedding64(sd, T(g["residue_idx"]), T(g["t"]), T(g["fixed_mask"]), T(g["sc_ca"]))
    for name, got, ref in (("node", node, T(g["node"])), ("edge", edge, T(g["edge"]))):
        scale = float(ref.abs().max())
        check(f"embedding64 vs fixture: {name} (scale {scale:.1f})", float((got - ref.double()).abs().max()), 5e-6 * scale)


def test_features32_are_the_oracles_features(sd):
    """The float32 MLP on features32 returns oracle.net.embedding bit for bit: same features, same order."""
    import torch.nn.functional as F

    c = EC.case("n7-gaps")
    node_f, pair_f = ref_embed.features32(*EC.inputs(c))
    assert node_f.shape == (3, 7, 65) and pair_f.shape == (3, 49, 120) and node_f.dtype == pair_f.dtype == torch.float32
    assert ref_embed.features32(*EC.inputs(c), self_conditioning=False)[1].shape == (3, 49, 98)
    node, edge = ON.embedding(sd, *EC.inputs(c))

    def mlp(x, p):
        for k in ("0", "2"):
            x = F.relu(F.linear(x, sd[f"{p}.{k}.weight"], sd[f"{p}.{k}.bias"]))
        x = F.linear(x, sd[p + ".4.weight"], sd[p + ".4.bias"])
        return F.layer_norm(x, (x.shape[-1],), sd[p + ".5.weight"], sd[p + ".5.bias"], 1e-5)

    assert torch.equal(mlp(node_f, "embedder.node_embed"), node)
    assert torch.equal(mlp(pair_f, "embedder.edge_embed").reshape(edge.shape), edge)


@pytest.mark.parametrize("name", EC.NAMES + ["exact-edge-axis0"])
def test_product_feature_functions_equal_the_oracles(name):
    """get_timestep_embedding / get_positional_embedding (what the module builds its tables from) on every case's t, residue
    numbers and relative-position table range arange(-span, span + 1), incl. the 100000 offset: the oracle's bits."""
    from str2str_amd.models.net.denoising_ipa import get_positional_embedding, get_timestep_embedding

    c = EC.exact_edge_case(0) if name.startswith("exact") else EC.case(name)
    idx = c["residue_idx"]
    span = int(idx.max() - idx.min())
    assert torch.equal(get_timestep_embedding(c["t"], 32), ON.timestep_embedding(c["t"], 32))
    for x in (idx, torch.arange(-span, span + 1)):
        assert torch.equal(get_positional_embedding(x, 32), ON.positional_embedding(x, 32))


@pytest.mark.parametrize("name", EC.NAMES)
def test_cases_are_what_they_claim(name):
    c = EC.case(name)
    B, N = c["B"], c["N"]
    if N > 1:
        assert EC.edge_clearance(c["ca"]) >= 1e-4
        assert ((c["fixed_mask"] == 0).any(1) & (c["fixed_mask"] == 1).any(1)).all()
        idx = c["residue_idx"]
        assert all(len(set(idx[b].tolist())) == N for b in range(B))
    assert len(set(c["t"].tolist())) == B
    m = c["node_mask"]
    assert (m[:, 0] == 0).all() and (m[:, -1] == 0).all() and (N < 24 or 0.05 < 1 - float(m.mean()) < 0.3)
    print(f"{name}: {c['redraws']} redraws, clearance {EC.edge_clearance(c['ca']):.2e} A")


def test_case_table_covers_the_inputs_it_promises():
    cs = [EC.case(n) for n in EC.NAMES]
    ts = {round(float(v), 6) for c in cs for v in c["t"]}
    assert 0.01 in ts and 1.0 in ts
    assert any((c["residue_idx"] < 0).any() for c in cs) and any((c["residue_idx"] >= 100000).any() for c in cs)
    rel = lambda c: c["residue_idx"][:, :, None] - c["residue_idx"][:, None, :]  # noqa: E731
    assert any(int(rel(c).max()) >= 1000 for c in cs)
    upper = lambda c: torch.triu(torch.ones(c["N"], c["N"]), 1).bool()  # noqa: E731
    assert any((rel(c)[:, upper(c)] > 0).any() for c in cs)      # d > 0 above the diagonal: descending / permuted order
    assert any(c["max_pairs"] for c in cs)
    # every bin and "no bin" occur off the diagonal somewhere in the table
    seen = torch.zeros(ref_embed.NUM_BINS + 1)
    for c in cs:
        hot = ref_embed.distogram32(c["ca"])
        seen[:-1] += hot.sum((0, 1, 2))
    assert (seen[:-1] > 0).all()


@pytest.mark.parametrize("name", EC.NAMES)
def test_float32_chain_distance_from_float64(sd, name):
    """e_ref: max |oracle.net.embedding (float32) - embedding64| for node and edge, and the same for the pair projection (float32
    F.linear of the float32 edge against pair_projection64).  The GPU bound is 3 x the maximum of these over the table; here each
    is held to the project's per-op 5e-6 of the output scale."""
    e = EC.e_ref(EC.case(name), sd, device="cpu")
    for out in EC.OUTPUTS:
        print(f"{name}: e_ref[{out}] = {e[out][0]:.3e} at scale {e[out][1]:.2f}")
        check(f"embedder float32 chain vs float64 [{name}]: {out}", e[out][0], 5e-6 * e[out][1])


@pytest.mark.parametrize("axis", [0, 1])
def test_oracle_reproduces_the_expected_bins_of_the_exact_edge_case(axis):
    c = EC.exact_edge_case(axis)
    hot = ON.calc_distogram(c["ca"], 1e-5, 20.0, 22)           # [72, 2, 2, 22]
    assert torch.equal(hot, ref_embed.distogram32(c["ca"]))
    n = hot.sum(-1)
    assert (n <= 1).all() and (n[:, 0, 0] == 0).all() and (n[:, 1, 1] == 0).all()
    got = torch.where(n > 0, hot.argmax(-1), torch.full_like(hot.argmax(-1), -1))
    assert torch.equal(got[:, 0, 1], c["bins"]) and torch.equal(got[:, 1, 0], c["bins"])
    assert set(c["bins"].tolist()) == set(range(-1, 22))
    # exact distances: the float32 norm returns the planted number
    d = torch.linalg.norm(c["ca"][:, 1] - c["ca"][:, 0], dim=-1)
    assert torch.equal(d, c["ca"][:, 1, axis])


def test_forced_bins_are_told_apart_by_the_bound(sd):
    """The GPU test reads a kernel's bin off its output row: the 23 forced-bin evaluations of embedding64 must differ from one
    another by far more than the bound, on every sample of the exact-edge case."""
    c = EC.exact_edge_case(0)
    rows = torch.stack([ref_embed.embedding64(sd, *EC.inputs(c), force_bin=k)[1][:, 0, 1] for k in range(-1, 22)])   # [23, 72, 128]
    gap = (rows[:, None] - rows[None]).abs().amax(-1)                                                                 # [23, 23, 72]
    gap = gap + torch.eye(23)[..., None] * 1e9
    assert float(gap.min()) > 10 * EC.rule_bound(sd, "edge"), (float(gap.min()), EC.rule_bound(sd, "edge"))


#  mutation                  case that separates it     output
SEPARATED_BY = [("rel_sign",               "n7-arange",         "edge"),
                ("rel_off_by_one",         "n7-arange",         "edge"),
                ("fixed_row_col_swapped",  "n7-arange",         "edge"),
                ("t_of_previous_sample",   "n7-arange",         "edge"),
                ("t_of_previous_sample",   "n7-arange",         "node"),
                ("bin_plus_one",           "n7-arange",         "edge"),
                ("upper_edge_le",          "exact-edge-axis0",  "edge")]


@pytest.mark.parametrize("mutation,name,output", SEPARATED_BY)
def test_bound_separates_a_mutated_reference(sd, mutation, name, output):
    """The unmutated float32 chain is at least 10 x the GPU bound (the rule's value: a tightened bound is smaller) away from the
    mutated float64 reference on the named case -- so a kernel with that mistake fails the GPU test by an order of magnitude, while
    the right chain passes at a third of the bound."""
    c = EC.exact_edge_case(0) if name.startswith("exact") else EC.case(name)
    got = dict(zip(("node", "edge"), ON.embedding(sd, *EC.inputs(c))))[output]
    ref = dict(zip(("node", "edge"), ref_embed.embedding64(sd, *EC.inputs(c), mutate=mutation)))[output]
    dist, b = float((got.double() - ref).abs().max()), EC.rule_bound(sd, output)
    print(f"{mutation} on {name}: {output} distance {dist:.3e}, bound {b:.3e}")
    record_margin(f"embedder mutation {mutation} [{name}] {output}: bound / distance (<= 0.1)", b / dist if dist else float("inf"), 0.1)
    assert dist >= 10 * b, (mutation, name, dist, b)


@pytest.mark.parametrize("mutation", ref_embed.MUTATIONS)
def test_every_listed_mutation_has_a_separating_case(mutation):
    assert any(m == mutation for m, _, _ in SEPARATED_BY)


def test_pair_projection64_layout(sd):
    """attn_bias is head-major [B, 8, L, L] = linear_b(z) permuted, pair_z [B, L, L, 32] = down_z(z) (oracle.net.ipa)."""
    c = EC.case("n7-gaps")
    _, edge = ref_embed.embedding64(sd, *EC.inputs(c), node_mask=c["node_mask"])
    ab, pz = ref_embed.pair_projection64(sd, EC.IPA0, edge)
    assert ab.shape == (3, 8, 7, 7) and pz.shape == (3, 7, 7, 32)
    m = c["node_mask"]
    dead = (m[:, :, None] * m[:, None, :]) == 0
    assert (edge[dead] == 0).all()
    # a masked pair projects to the bias alone
    assert torch.equal(pz[dead], sd[EC.IPA0 + ".down_z.bias"].double().expand_as(pz[dead]))
