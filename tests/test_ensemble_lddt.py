"""lDDT on the device (csrc/ensemble_lddt.hip) against the float64 numpy restatement of its definition in tests/ref_lddt.py.

Every case here is a parity input: tests/test_ensemble_lddt_cpu.py asserts that its nearest comparison (a distance difference against a
threshold, a reference distance against the cutoff) is at least 1e-10 A from flipping, and the kernel's squared-bound comparisons differ
from the yardstick's by a few ulp of 15 A ~ 1e-14 A.  Hits and counts are therefore the same integers on both sides, and the score -- one
float64 division of them -- may differ by at most BOUND = 4e-16: two float64 roundings near 1, should the division be done as a
reciprocal and a multiplication.
"""
import functools

import numpy as np
import pytest
import torch

import lddt_cases as cases
import ref_cluster
import ref_lddt as ref
import ref_tm64
from conftest import record_margin
from ensemble_cases import close_4 as _close_4, to_device as _dev

pytestmark = pytest.mark.gpu

DEV = "cuda"
BOUND = 4e-16


@functools.lru_cache(maxsize=None)
def reference(L):
    """(a, b, lDDT_ref [n_a, n_b]) of one chain length, computed once."""
    a, b = cases.ensembles(L)
    want = ref.matrix(a, b)
    want.setflags(write=False)
    return a, b, want


def _held(name, got, want):
    err = float(np.abs(got - want).max())
    record_margin(name, err, BOUND)
    assert err <= BOUND, (name, err)


@pytest.mark.parametrize("L", cases.LENGTHS)
def test_lddt_matrix_against_float64_reference(L):
    from str2str_amd import ops

    a, b, want = reference(L)
    assert ref.margin(a, b) >= ref.MARGIN
    got = ops.ca_lddt_matrix(_dev(a), _dev(b))
    assert got.dtype == torch.float64 and got.shape == want.shape
    got = got.cpu().numpy()
    assert (got >= 0.0).all() and (got <= 1.0).all()
    print(f"L={L} {got.shape}: max |lDDT_gpu - lDDT_ref| = {float(np.abs(got - want).max()):.3e}, lDDT in [{want.min():.4f}, {want.max():.4f}]")
    _held("ensemble_lddt_matrix_abs", got, want)
    if L == 1:
        assert (got == 1.0).all()
    for x in (a, b):                                           # b=None: every structure in its own environment
        own = ops.ca_lddt_matrix(_dev(x))
        assert own.dtype == torch.float64 and bool((own.diagonal() == 1.0).all()) and bool((own >= 0.0).all()) and bool((own <= 1.0).all())
        assert torch.equal(own, ops.ca_lddt_matrix(_dev(x), _dev(x).clone()))   # b == a is not special-cased
        if len(x) <= 9:
            assert ref.margin(x, x) >= ref.MARGIN
            _held("ensemble_lddt_matrix_abs", own.cpu().numpy(), ref.matrix(x, x))


def test_chunking_is_bit_identical(monkeypatch):
    from str2str_amd import ops
    from str2str_amd.ops import ensemble

    a, b, want = reference(65)                                 # 17 x 24
    a, b = _dev(a), _dev(b)
    whole = ops.ca_lddt_matrix(a, b)
    n_b = b.shape[0]
    for max_pairs in (n_b, 5 * n_b, 100):
        assert torch.equal(ops.ca_lddt_matrix(a, b, max_pairs=max_pairs), whole), max_pairs
    out = torch.empty(17, 24, dtype=torch.float64, device=DEV)
    assert ops.ca_lddt_matrix(a, b, out=out) is out and torch.equal(out, whole)
    monkeypatch.setattr(ensemble, "LDDT_WORKSPACE_BYTES", 1)   # one reference structure per launch
    assert torch.equal(ops.ca_lddt_matrix(a, b), whole)
    own = ops.ca_lddt_matrix(a)
    monkeypatch.undo()
    assert torch.equal(ops.ca_lddt_matrix(a), own)
    # 601 x 601 at L = 16: in one launch a staged tile serves runs of five reference structures (the last run is short), in launches of
    # seven rows each serves one
    s = _dev(ref_tm64.make_ensemble(np.random.default_rng(5), 601, 16, ref_tm64.random_walk(np.random.default_rng(6), 16)))
    big = ops.ca_lddt_matrix(s)
    assert torch.equal(ops.ca_lddt_matrix(s, max_pairs=601 * 7), big) and bool((big.diagonal() == 1.0).all())


@pytest.mark.parametrize("L", [31, 65])
def test_orientation(L):
    from str2str_amd import ops

    a, b, want = reference(L)
    ab, ba = ops.ca_lddt_matrix(_dev(a), _dev(b)).cpu().numpy(), ops.ca_lddt_matrix(_dev(b), _dev(a)).cpu().numpy()
    assert ref.margin(b, a) >= ref.MARGIN
    _held("ensemble_lddt_matrix_abs", ab, want)
    _held("ensemble_lddt_matrix_abs", ba, ref.matrix(b, a))
    assert (ab != ba.T).any()                                  # the first argument defines the environment


def test_other_cutoff_and_sequence_separation():
    from str2str_amd import ops

    a, b, want = reference(65)
    cutoff, sep = cases.OTHER_PARAMETERS
    assert ref.margin(a, b, cutoff, sep) >= ref.MARGIN
    want2 = ref.matrix(a, b, cutoff, sep)
    _held("ensemble_lddt_matrix_abs", ops.ca_lddt_matrix(_dev(a), _dev(b), cutoff=cutoff, min_seq_sep=sep).cpu().numpy(), want2)
    assert np.abs(want2 - want).max() > 1e-3
    for c, s in ((cutoff, 1), (15.0, sep)):                    # each parameter alone
        assert ref.margin(a, b, c, s) >= ref.MARGIN
        _held("ensemble_lddt_matrix_abs", ops.ca_lddt_matrix(_dev(a), _dev(b), cutoff=c, min_seq_sep=s).cpu().numpy(), ref.matrix(a, b, c, s))
    # a separation no pair reaches: the empty set everywhere
    assert bool((ops.ca_lddt_matrix(_dev(a), _dev(b), min_seq_sep=65) == 1.0).all())


@pytest.mark.parametrize("L", cases.PER_RESIDUE_LENGTHS)
def test_lddt_per_residue(L):
    from str2str_amd import ops
    from str2str_amd.metrics import metrics

    model, target = cases.per_residue_inputs(L)
    assert ref.margin(target[None], model) >= ref.MARGIN
    want_res, want_total = ref.per_residue(model, target)
    per_res, total = ops.ca_lddt_per_residue(_dev(model), _dev(target))
    assert per_res.dtype == torch.float64 and per_res.shape == (9, L) and total.dtype == torch.float64 and total.shape == (9,)
    assert torch.equal(total, ops.ca_lddt_matrix(_dev(target[None]), _dev(model))[0])
    _held("ensemble_lddt_per_residue_abs", per_res.cpu().numpy(), want_res)
    _held("ensemble_lddt_per_residue_abs", total.cpu().numpy(), want_total)
    assert bool((per_res >= 0.0).all()) and bool((per_res <= 1.0).all()) and float(total[0]) == 1.0    # (the first model is an exact copy)
    assert (metrics.lddt(model, target) == total.cpu().numpy()).all()
    assert (metrics.lddt(model, target, per_residue=True) == per_res.cpu().numpy()).all()
    # a tight cutoff leaves some residues of a random walk without a partner at min_seq_sep = 3: they score 1.0
    assert ref.margin(target[None], model, 5.0, 3) >= ref.MARGIN and (ref.counts(target, model, 5.0, 3)[1] == 0).any()
    w_res, w_total = ref.per_residue(model, target, 5.0, 3)
    g_res, g_total = ops.ca_lddt_per_residue(_dev(model), _dev(target), cutoff=5.0, min_seq_sep=3)
    _held("ensemble_lddt_per_residue_abs", g_res.cpu().numpy(), w_res)
    _held("ensemble_lddt_per_residue_abs", g_total.cpu().numpy(), w_total)


def test_nan_is_neither_included_nor_hit():
    from str2str_amd import ops

    a, b, _ = reference(16)
    a, b = a[:3].copy(), b[:4].copy()
    b[1, 5] = np.nan                                           # a model with a missing residue: its pairs are not hit
    a[2, 7, 0] = np.nan                                        # a reference with a missing residue: its pairs are not included
    got = ops.ca_lddt_matrix(_dev(a), _dev(b)).cpu().numpy()
    want = ref.matrix(a, b)
    assert np.isfinite(got).all() and np.abs(got - want).max() <= BOUND
    assert ref.counts(a[2], b)[1][7] == 0 and ref.counts(a[0], b)[0][1, 5] == 0


def test_diversity_coverage_and_lddt_metrics():
    from str2str_amd.metrics import metrics

    rng = np.random.default_rng(22)
    L = 22
    base = ref_tm64.random_walk(rng, L)
    target, pred = ref_tm64.make_ensemble(rng, 9, L, base), ref_tm64.make_ensemble(rng, 12, L, base, first_kind=1)
    cross = ref.matrix(target, pred)                           # [9, 12]: the reference ensemble's frames are the lDDT references
    got = metrics.pairwise_lddt(target, pred)
    assert min(ref.margin(target, pred), ref.margin(pred, pred), ref.margin(target, target), ref.margin(target, pred, 8.0, 2)) >= ref.MARGIN
    assert got.dtype == np.float64 and np.abs(got - cross).max() <= BOUND
    assert np.abs(metrics.pairwise_lddt(pred) - ref.matrix(pred, pred)).max() <= BOUND
    assert np.abs(metrics.pairwise_lddt(target, pred, cutoff=8.0, min_seq_sep=2) - ref.matrix(target, pred, 8.0, 2)).max() <= BOUND

    div = metrics.diversity_lddt({"target": target, "pred": pred, "one": pred[:1]})
    assert div["one"] == 1.0 and set(div) == {"target", "pred", "one"}
    for k, x in (("target", target), ("pred", pred)):
        m = ref.matrix(x, x)
        assert _close_4(div[k], m[~np.eye(len(x), dtype=bool)].mean()) and div[k] == np.around(div[k], decimals=4) and 0.0 < div[k] < 1.0
    recall, precision = metrics.coverage_lddt({"target": target, "pred": pred})
    assert recall["target"] == 1.0 and precision["target"] == 1.0
    assert _close_4(recall["pred"], cross.max(1).mean()) and _close_4(precision["pred"], cross.max(0).mean())
    # 9 x 12 pairs in chunks of 36 = three row chunks: running maxima, the very same numbers
    assert metrics.coverage_lddt({"target": target, "pred": pred}, chunk_pairs=36) == (recall, precision)
    per_ref, per_sample = metrics._coverage_extrema(metrics.LDDT, _dev(pred), _dev(target), chunk_pairs=36)
    assert np.abs(per_ref.cpu().numpy() - cross.max(1)).max() <= BOUND and np.abs(per_sample.cpu().numpy() - cross.max(0)).max() <= BOUND

    scores = metrics.lddt(pred, target[0])
    assert scores.shape == (12,) and all(_close_4(np.around(s, 4), w) for s, w in zip(scores, cross[0]))
    assert metrics.lddt(pred, target[0], per_residue=True).shape == (12, L)


def test_cluster_lddt_equals_the_yardstick():
    from str2str_amd.metrics import metrics

    x, group = ref_cluster.planted_ensemble()
    assert ref.margin(x, x) >= ref.MARGIN
    sym = ref.symmetrised(x)
    values = np.unique(sym)
    assert len(values) > 4
    for k in (len(values) // 4, len(values) // 2, (3 * len(values)) // 4):
        cutoff = 0.5 * (values[k - 1] + values[k])             # between two adjacent distinct values: no entry sits on it
        assert values[k - 1] < cutoff < values[k]
        want = ref_cluster.gromos(sym >= cutoff)
        got = metrics.cluster_lddt(x, cutoff)
        assert isinstance(got, metrics.ClusterResult)
        for g, w, name in zip(got, want, ("labels", "centres", "sizes")):
            assert g.dtype == np.int32 and g.shape == w.shape and (g == w).all(), (name, cutoff)
    # the four planted chains come back as the four largest clusters at a cutoff between the within- and between-chain scores
    same = group[:, None] == group[None, :]
    lo, hi = sym[~same].max(), sym[same].min()
    assert lo < hi
    res = metrics.cluster_lddt(x, 0.5 * (lo + hi))
    assert res.sizes.tolist() == [40, 25, 12, 3] and all(len(set(group[res.labels == c])) == 1 for c in range(4))

