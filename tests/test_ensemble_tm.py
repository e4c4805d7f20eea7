"""TM-score on the device (csrc/ensemble_tm.hip) against the float64 numpy restatement of its definition in tests/ref_tm64.py.

Bound: |TM_gpu - TM_ref| <= 1e-9 on every pair with L >= 3.  The search is a continuous function of the coordinates (a fixed number of
reweighted Kabsch steps, a maximum over seeds), and perturbing the widened inputs by 1e-15 relative moves the reference by at most a few
1e-14 on this recipe, so a different summation order and a different eigen-route (Jacobi on Horn's 4 x 4 there, SVD here) leave four
orders of headroom.  The yardstick is evaluated a second time on inputs perturbed by 1e-15: a pair on which it moves by more than 1e-10
is ill conditioned and left out, and at most 1 % of the pairs may be.  L = 2 (two tied optima) and an exactly collinear chain are not
parity inputs: finite values in (0, 1] only.
"""
import functools

import numpy as np
import pytest
import torch

import ref_tm64 as ref
from conftest import record_margin
from ensemble_cases import close_4 as _close_4, to_device as _dev

pytestmark = pytest.mark.gpu

DEV = "cuda"
BOUND = 1e-9
# no windows; the duplicate-window case; the d0 floor edge; wave-width edges; several residues per staging lane; above 341 residues the
# tile needs more than the default 64 KiB of dynamic LDS
LENGTHS = (1, 3, 4, 5, 8, 16, 21, 22, 35, 63, 64, 65, 130, 256, 400)


def _sizes(L):
    if L >= 130:
        return ((1, 5), (5, 9)) if L < 400 else ((2, 3),), (1, 5) if L < 400 else (3,)
    return ((1, 5), (17, 24), (5, 33)), (1, 5, 17)


@functools.lru_cache(maxsize=None)
def case(L):
    """The inputs of one chain length and their reference values, computed once: [(a, b or None for a self matrix, TM_ref, TM_ref of
    the perturbed inputs)]."""
    rng = np.random.default_rng(4000 + L)
    base = ref.random_walk(rng, L)
    cross, selfs = _sizes(L)
    out = []
    for n_a, n_b in cross:
        a, b = ref.make_ensemble(rng, n_a, L, base), ref.make_ensemble(rng, n_b, L, base, first_kind=3)
        out.append((a, b, ref.tm_matrix(a, b), ref.tm_matrix(ref.perturbed(a, rng), ref.perturbed(b, rng))))
    for n in selfs:
        a = ref.make_ensemble(rng, n, L, base, first_kind=n)
        p = ref.perturbed(a, rng)
        out.append((a, None, ref.tm_matrix(a, a), ref.tm_matrix(p, p)))
    return out


@pytest.mark.parametrize("L", LENGTHS)
def test_tm_matrix_against_float64_reference(L):
    from str2str_amd import ops

    worst, n_pairs, n_out = 0.0, 0, 0
    for a, b, want, want_p in case(L):
        got = ops.ca_tm_matrix(_dev(a), None if b is None else _dev(b)).cpu().numpy()
        assert got.shape == want.shape and got.dtype == np.float64 and np.isfinite(got).all()
        assert (got > 0.0).all() and (got <= 1.0).all()
        floor = ref.kabsch_tm(a, a if b is None else b)
        assert (got >= floor - BOUND).all(), float((floor - got).max())   # never below the plain minimum-RMSD superposition
        if b is None:
            assert (got == got.T).all() and np.diag(got).min() >= 1.0 - 1e-12
        if L == 1:
            assert (got == 1.0).all()
        keep = np.abs(want - want_p) <= 1e-10
        n_pairs += keep.size
        n_out += int((~keep).sum())
        err = np.abs(got - want)
        print(f"L={L} {got.shape}: max |TM_gpu - TM_ref| = {float(err.max()):.3e} (kept pairs {float(err[keep].max()) if keep.any() else 0.0:.3e}), "
              f"reference moved by {float(np.abs(want - want_p).max()):.3e} under the perturbation, left out {int((~keep).sum())}")
        if keep.any():
            worst = max(worst, float(err[keep].max()))
    record_margin("ensemble_tm_matrix_abs", worst, BOUND)
    assert n_out <= 0.01 * n_pairs, (n_out, n_pairs)
    assert worst <= BOUND, worst


def test_explicit_d0_overrides_the_formula():
    from str2str_amd import ops

    a, b, want, _ = case(35)[2]
    got = ops.ca_tm_matrix(_dev(a), _dev(b), d0=3.0).cpu().numpy()
    want3 = ref.tm_matrix(a, b, d0=3.0)
    record_margin("ensemble_tm_matrix_abs", float(np.abs(got - want3).max()), BOUND)
    assert np.abs(got - want3).max() <= BOUND and np.abs(want3 - want).max() > 1e-3
    # (the library's cbrt and numpy's may differ in the last bit of d0)
    assert (ops.ca_tm_matrix(_dev(a), _dev(b), d0=ref.tm_d0(35)) - ops.ca_tm_matrix(_dev(a), _dev(b))).abs().max() <= 1e-12


def test_chunking_is_bit_identical():
    from str2str_amd import ops

    a, b = _dev(case(35)[1][0]), _dev(case(35)[1][1])          # 17 x 24
    s = _dev(case(35)[5][0])                                   # self, 17
    for x, y, n_b in ((s, None, 17), (a, b, 24)):
        whole = ops.ca_tm_matrix(x, y)
        for max_pairs in (n_b, 5 * n_b, 100):
            assert torch.equal(ops.ca_tm_matrix(x, y, max_pairs=max_pairs), whole), (n_b, max_pairs)
    out = torch.empty(17, 24, dtype=torch.float64, device=DEV)
    assert ops.ca_tm_matrix(a, b, out=out) is out and torch.equal(out, ops.ca_tm_matrix(a, b))
    # the self matrix through explicit b is the cross evaluation of every pair: the same values within the bound, not bit for bit
    assert (ops.ca_tm_matrix(s, s.clone()) - ops.ca_tm_matrix(s)).abs().max() <= BOUND


@pytest.mark.parametrize("L", [22, 65])
def test_transposed_arguments(L):
    from str2str_amd import ops

    a, b, _, _ = case(L)[1]
    d = (ops.ca_tm_matrix(_dev(a), _dev(b)) - ops.ca_tm_matrix(_dev(b), _dev(a)).T).abs().max()
    record_margin("ensemble_tm_transposed_arguments_abs", float(d), BOUND)
    assert d <= BOUND


@pytest.mark.parametrize("L", [16, 35, 80])
def test_planted_half_chain_is_found(L):
    from str2str_amd import ops

    rng = np.random.default_rng(200 + L)
    for _ in range(4):
        a, b, fraction = ref.planted_pair(rng, L)
        got = float(ops.ca_tm_matrix(_dev(a[None]), _dev(b[None]))[0, 0])
        assert fraction <= got <= 1.0, (fraction, got)


def test_ill_conditioned_inputs_stay_finite():
    """L = 2 has two tied local optima and a collinear chain a free rotation about its axis: no parity, finite values in (0, 1]."""
    from str2str_amd import ops

    rng = np.random.default_rng(9)
    for L in (2, 35):
        base = ref.random_walk(rng, L) if L == 2 else np.arange(L)[:, None] * 3.8 * np.array([[0.6, 0.0, 0.8]])
        a, b = ref.make_ensemble(rng, 5, L, base), ref.make_ensemble(rng, 9, L, base, first_kind=2)
        for got in (ops.ca_tm_matrix(_dev(a), _dev(b)), ops.ca_tm_matrix(_dev(b))):
            assert bool(torch.isfinite(got).all()) and bool((got > 0.0).all()) and bool((got <= 1.0).all())
        tm, xform = ops.ca_tm_superpose(_dev(a), _dev(b[0]))
        assert bool(torch.isfinite(tm).all()) and bool(torch.isfinite(xform).all())


@pytest.mark.parametrize("L", [1, 5, 22, 35, 65, 256])
def test_tm_superpose(L):
    from str2str_amd import ops
    from str2str_amd.metrics import metrics

    rng = np.random.default_rng(5000 + L)
    base = ref.random_walk(rng, L)
    mobile = ref.make_ensemble(rng, 9, L, base)
    target = np.asarray(ref.rigid_move(rng, base), dtype=np.float32)
    tm, xform = ops.ca_tm_superpose(_dev(mobile), _dev(target))
    assert torch.equal(tm, ops.ca_tm_matrix(_dev(mobile), _dev(target[None]))[:, 0])
    tm, xf = tm.cpu().numpy(), xform.cpu().numpy()
    rot, trans = xf[:, :9].reshape(-1, 3, 3), xf[:, 9:]
    det = float(np.abs(np.linalg.det(rot) - 1.0).max())
    ortho = float(np.abs(np.swapaxes(rot, 1, 2) @ rot - np.eye(3)).max())
    t64 = np.broadcast_to(target.astype(np.float64), mobile.shape)
    again = ref.score_under(mobile.astype(np.float64), t64, rot, trans, ref.tm_d0(L))[1]
    record_margin("ensemble_tm_superpose_score_of_xform_abs", float(np.abs(again - tm).max()), BOUND)
    record_margin("ensemble_tm_superpose_det", max(det, ortho), 1e-12)
    assert np.abs(again - tm).max() <= BOUND and det <= 1e-12 and ortho <= 1e-12
    if L >= 3:
        want = ref.tm_matrix(mobile, target[None])[:, 0]
        keep = np.abs(want - ref.tm_matrix(ref.perturbed(mobile, rng), ref.perturbed(target[None], rng))[:, 0]) <= 1e-10
        assert keep.all() and np.abs(tm - want).max() <= BOUND
    aligned, tm2 = metrics.tm_superpose(mobile, target)
    assert aligned.dtype == np.float32 and (tm2 == tm).all()
    assert (aligned == ops.apply_xform(_dev(mobile), xform).cpu().numpy()).all()


def test_diversity_and_coverage_metrics():
    from str2str_amd.metrics import metrics

    rng = np.random.default_rng(21)
    L = 22
    base = ref.random_walk(rng, L)
    target, pred = ref.make_ensemble(rng, 9, L, base), ref.make_ensemble(rng, 12, L, base, first_kind=1)
    got = metrics.pairwise_tm(pred, target)
    cross = ref.tm_matrix(pred, target)
    assert got.dtype == np.float64 and np.abs(got - cross).max() <= BOUND
    self_p = metrics.pairwise_tm(pred)
    assert (self_p == self_p.T).all() and np.abs(self_p - ref.tm_matrix(pred, pred)).max() <= BOUND

    div = metrics.diversity_tm({"target": target, "pred": pred, "one": pred[:1]})
    assert div["one"] == 1.0 and set(div) == {"target", "pred", "one"}
    for k, x in (("target", target), ("pred", pred)):
        assert _close_4(div[k], ref.tm_matrix(x, x)[np.triu_indices(len(x), 1)].mean()) and div[k] == np.around(div[k], decimals=4)
    recall, precision = metrics.coverage_tm({"target": target, "pred": pred})
    assert recall["target"] == 1.0 and precision["target"] == 1.0
    assert _close_4(recall["pred"], cross.max(0).mean()) and _close_4(precision["pred"], cross.max(1).mean())
    # 12 x 9 pairs in chunks of 36 = three row chunks: running maxima, the very same numbers
    assert metrics.coverage_tm({"target": target, "pred": pred}, chunk_pairs=36) == (recall, precision)
    per_ref, per_sample = metrics._coverage_extrema(metrics.TM, _dev(pred), _dev(target), chunk_pairs=36)
    assert np.abs(per_ref.cpu().numpy() - cross.max(0)).max() <= BOUND and np.abs(per_sample.cpu().numpy() - cross.max(1)).max() <= BOUND

