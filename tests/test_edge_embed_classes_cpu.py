"""The host side of the edge embedding by class: the row-index formula and its inverse, the table size, and the eligibility rule."""
import pytest
import torch

from str2str_amd import ops


@pytest.mark.parametrize("n_rel,n_bins", [(1, 1), (3, 2), (7, 22), (12, 5)])
def test_class_row_and_its_decode_are_inverse_over_the_whole_table(n_rel, n_bins):
    rows = ops.edge_embed_class_rows(2, n_rel, n_bins)
    assert rows == 4 * n_rel * (n_bins + 1) and ops.edge_embed_class_rows(1, n_rel, n_bins) == n_rel * (n_bins + 1)
    seen = set()
    for r in range(rows):
        fa, fb, d, b = ops.edge_embed_class_of_row(r, n_rel, n_bins)
        assert fa in (0, 1) and fb in (0, 1) and 0 <= d < n_rel and -1 <= b < n_bins
        assert ops.edge_embed_class_row(fa, fb, d, b, n_rel, n_bins) == r
        seen.add((fa, fb, d, b))
    assert len(seen) == rows
    # one fixed-mask value present: its rows are the first quarter, class (0, 0)
    assert all(ops.edge_embed_class_of_row(r, n_rel, n_bins)[:2] == (0, 0) for r in range(ops.edge_embed_class_rows(1, n_rel, n_bins)))
    # the documented formula
    assert ops.edge_embed_class_row(1, 0, n_rel - 1, n_bins - 1, n_rel, n_bins) == ((1 * 2 + 0) * n_rel + n_rel - 1) * (n_bins + 1) + n_bins
    with pytest.raises(ops.HipLibraryError):
        ops.edge_embed_class_rows(3, n_rel, n_bins)


def test_eligibility_rule():
    ok = dict(mode="auto", arith="f16x3", one_timestep=True, n_fixed=1, mask_is_01=True, n_rel=511, n_bins=22, B=128, N=256)
    el = lambda **kw: ops.edge_embed_classes_eligible(**dict(ok, **kw))  # noqa: E731
    assert el()                                                   # the flagship shape: 11 753 rows against 8.4 M pairs
    assert not el(mode="0") and el(mode="1")
    assert not el(arith="f32") and not el(one_timestep=False) and not el(n_fixed=None) and not el(mask_is_01=False)
    assert not el(mode="1", arith="f32") and not el(mode="1", n_fixed=None)          # forcing never makes an illegal call legal
    # the threshold: rows x R <= B N^2, with the table's rows counted for the fixed-mask values present
    rows1, rows2 = 511 * 23, 4 * 511 * 23
    R = ops.EE_CLASS_R
    assert R >= 1
    assert el(B=1, N=256, R=5) == (rows1 * 5 <= 256 * 256) and el(n_fixed=2, B=1, N=256, R=1) == (rows2 <= 256 * 256)
    b_min = -(-rows1 * R // (256 * 256))
    assert el(B=b_min) and (b_min == 1 or not el(B=b_min - 1))
    assert not el(B=1000, N=35, n_rel=69, n_fixed=2, R=10 ** 6) and el(mode="1", B=1, N=2, n_fixed=2)   # "1" ignores the threshold
    with pytest.raises(ValueError):
        el(mode="yes")


def test_class_terms_of_the_fixed_mask():
    """The per-target build: class terms only for an exact 0/1 mask, the operand rows are the chunk's own products."""
    from str2str_amd.factory import build_synthetic_net

    emb = build_synthetic_net(seed=0, sigma_final=0.02, device="cpu").embedder
    w, cpu = emb._weights(), torch.device("cpu")
    fixed = torch.tensor([[0.0, 1.0, 1.0, 0.0]])
    Fn, Fa, Fb, cls = emb._fixed_terms(fixed, w, cpu, torch.zeros(1, 4, 256))
    assert cls["n_fixed"] == 2 and cls["fixed_cls"].dtype == torch.int32 and cls["fixed_cls"].tolist() == [[0, 1, 1, 0]]
    assert torch.equal(cls["fa2"][0], Fa[0, :2]) and torch.equal(cls["fb2"][0], Fb[0][0, :, :2])
    for value in (0.0, 1.0):
        one = torch.full((2, 3), value)
        _, Fa, Fb, cls = emb._fixed_terms(one, w, cpu, torch.zeros(2, 3, 256))
        assert cls["n_fixed"] == 1 and not cls["fixed_cls"].any() and torch.equal(cls["fa2"][0, 0], Fa[0, 0]) and torch.equal(cls["fb2"][0, :, 0], Fb[0][0, :, 0])
    assert emb._fixed_terms(torch.tensor([[0.0, 0.5]]), w, cpu, torch.zeros(1, 2, 256))[3] is None
    assert emb.ee_classes in ("auto", "0", "1") and "ee_classes" in type(emb).launch_modes
