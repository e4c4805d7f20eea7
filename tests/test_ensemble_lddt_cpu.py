"""The lDDT feature without a GPU: its yardstick (tests/ref_lddt.py) held to the reference's own ``lddt`` and to cases worked by hand, the
margin that makes every device case a parity input, the C-ABI surface, the evaluation columns, and the argument checks that must fire
before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lddt_cases as cases
import ref_lddt as ref
from conftest import ROOT, golden, record_margin
from ensemble_cases import load_eval_entry
from ref_tm64 import random_walk
from str2str_amd.ops.ensemble import LDDT_MAX_RES, lddt_workspace_bytes   # (the binding's statement of the header's limits, held to it below)

NAMES = ("s2s_ca_lddt_matrix", "s2s_ca_lddt_per_residue")


# ------------------------------------------------------------------------------------------------------------- the yardstick itself
@pytest.mark.parametrize("tag,L", [("a", 5), ("b", 40), ("c", 130)])
def test_yardstick_against_the_reference_lddt(tag, L):
    """tests/golden/lddt.npz: src/models/loss.py ``lddt`` in float64, mask of ones.  Bound 1e-9: the reference's eps = 1e-10 inside the
    square root moves a distance by at most 1e-10 / (2 min d) <= 1e-9 A at min d >= 0.05 A -- far inside the case's margin, so no comparison
    flips -- and in eps / (eps + n) moves the score by less than 1e-10."""
    g = golden("lddt.npz")
    true, pred = g[f"{tag}_true"], g[f"{tag}_pred"]
    assert true.shape == (L, 3) and true.dtype == np.float32
    off = ~np.eye(L, dtype=bool)
    assert min(ref.distances(true)[off].min(), ref.distances(pred)[off].min()) >= 0.05
    assert ref.counts(true, pred[None])[1].sum() > 0 and ref.margin(true[None], pred[None]) >= 1e-6
    per_res, total = ref.per_residue(pred[None], true)
    err = max(float(np.abs(per_res[0] - g[f"{tag}_per_residue"]).max()), abs(float(total[0]) - float(g[f"{tag}_total"])))
    record_margin("ensemble_lddt_ref_vs_reference_abs", err, 1e-9)
    assert err <= 1e-9, err
    assert float(ref.matrix(true[None], pred[None])[0, 0]) == float(total[0])


def _line(*xs):
    return np.array([[x, 0.0, 0.0] for x in xs], dtype=np.float32)


def test_hand_cases():
    rng = np.random.default_rng(1)
    x = np.asarray(random_walk(rng, 12), dtype=np.float32)
    assert ref.matrix(x[None], x[None])[0, 0] == 1.0 and (ref.per_residue(x[None], x)[0] == 1.0).all()       # an identical pair
    far = _line(0.0, 20.0)
    assert ref.matrix(far[None], _line(0.0, 3.0)[None])[0, 0] == 1.0                                          # the empty set
    assert ref.counts(far, far[None])[1].sum() == 0
    one = np.zeros((1, 1, 3), dtype=np.float32)
    assert ref.matrix(one, one + 5.0)[0, 0] == 1.0 and ref.per_residue(one + 5.0, one[0])[0].tolist() == [[1.0]]   # L = 1


def test_three_residues_by_hand():
    """a = 0, 3, 6 on a line: d_a(0,1) = d_a(1,2) = 3, d_a(0,2) = 6.  The models keep residues 0 and 1 and move residue 2 to 6 + s:
    |d_a - d_b| = s for the pairs (1,2) and (0,2), 0 for (0,1).  s = 0.25, 0.75, 1.5, 3, 5 lose 0, 1, 2, 3, 4 of the four thresholds."""
    a = _line(0.0, 3.0, 6.0)
    shifts = (0.25, 0.75, 1.5, 3.0, 5.0)
    b = np.stack([_line(0.0, 3.0, 6.0 + s) for s in shifts])
    hits, n = ref.counts(a, b)
    assert n.tolist() == [2, 2, 2]
    for k, lost in enumerate((0, 1, 2, 3, 4)):
        moved = 4 - lost                                       # hits of a pair that involves residue 2
        assert hits[k].tolist() == [4 + moved, 4 + moved, 2 * moved]
        assert ref.matrix(a[None], b[k:k + 1])[0, 0] == (8 + 4 * moved) / 24.0
        assert ref.per_residue(b[k:k + 1], a)[0][0].tolist() == [(4 + moved) / 8.0, (4 + moved) / 8.0, moved / 4.0]
    # a pair with every count 0 .. 4 in one structure: residue 2 at 6 + s against 0 sits |d| = s off
    assert sorted(set((hits[:, 2] // 2).tolist())) == [0, 1, 2, 3, 4]


def test_asymmetry_and_min_seq_sep():
    # a: residues 0 and 1 are 10 A apart (included); b: 20 A apart (not included).  a -> b scores the pair (lost: 0), b -> a has nothing to score.
    a, b = _line(0.0, 10.0), _line(0.0, 20.0)
    assert ref.matrix(a[None], b[None])[0, 0] == 0.0 and ref.matrix(b[None], a[None])[0, 0] == 1.0
    # min_seq_sep = 3 drops exactly the pairs with |i - j| in (1, 2)
    rng = np.random.default_rng(2)
    x = np.cumsum(rng.normal(size=(9, 3)), 0).astype(np.float32)
    y = (x + rng.normal(size=x.shape)).astype(np.float32)
    n1, n3 = ref.counts(x, y[None], cutoff=100.0)[1], ref.counts(x, y[None], cutoff=100.0, min_seq_sep=3)[1]
    assert n1.tolist() == [8] * 9 and n3.tolist() == [6, 5, 4, 4, 4, 4, 4, 5, 6]
    l1 = np.abs(ref.distances(x) - ref.distances(y))
    near = np.abs(np.subtract.outer(np.arange(9), np.arange(9)))
    want = sum(int(((l1 < t) & (near >= 3)).sum()) for t in ref.THRESHOLDS) / (4.0 * (near >= 3).sum())
    assert ref.matrix(x[None], y[None], cutoff=100.0, min_seq_sep=3)[0, 0] == want
    sym = ref.symmetrised(np.stack([x, y]))
    assert (sym == sym.T).all() and (np.diag(sym) == 1.0).all()


# --------------------------------------------------------------------------------------------------------- the device cases' margin
@pytest.mark.parametrize("L", cases.LENGTHS)
def test_every_device_case_is_a_parity_input(L):
    """The device compares squared distances with squared bounds, a few ulp of 15 A ~ 1e-14 A from the yardstick's comparisons: a case whose
    nearest comparison is >= 1e-10 A from flipping has identical integers on both sides.  A condition on the cases; none is left out."""
    a, b = cases.ensembles(L)
    m = ref.margin(a, b)
    print(f"L={L} {len(a)} x {len(b)}: margin {m:.3e} A")
    assert m >= ref.MARGIN, m
    if L in (31, 65):                                          # the transposed arguments
        assert ref.margin(b, a) >= ref.MARGIN
    if len(b) <= 9:                                            # each ensemble in its own environments
        assert min(ref.margin(a, a), ref.margin(b, b)) >= ref.MARGIN
    if L == 65:
        cutoff, sep = cases.OTHER_PARAMETERS
        assert min(ref.margin(a, b, cutoff, sep), ref.margin(a, b, cutoff, 1), ref.margin(a, b, 15.0, sep)) >= ref.MARGIN
    if L in cases.PER_RESIDUE_LENGTHS:
        model, target = cases.per_residue_inputs(L)
        assert min(ref.margin(target[None], model), ref.margin(target[None], model, 5.0, 3)) >= ref.MARGIN


def test_the_other_device_inputs_are_parity_inputs():
    import ref_cluster
    import ref_tm64

    x, _ = ref_cluster.planted_ensemble()
    assert ref.margin(x, x) >= ref.MARGIN
    rng = np.random.default_rng(22)
    base = ref_tm64.random_walk(rng, 22)
    target, pred = ref_tm64.make_ensemble(rng, 9, 22, base), ref_tm64.make_ensemble(rng, 12, 22, base, first_kind=1)
    assert min(ref.margin(target, pred), ref.margin(pred, pred), ref.margin(target, target), ref.margin(target, pred, 8.0, 2)) >= ref.MARGIN


def test_margin_sees_a_pair_on_the_edge():
    a = _line(0.0, 10.0)
    assert abs(ref.margin(a[None], _line(0.0, 10.5 + 1e-4)[None]) - 1e-4) < 1e-6      # | |d_a - d_b| - 0.5 |
    assert abs(ref.margin(_line(0.0, 15.0 - 1e-3)[None], a[None]) - 1e-3) < 1e-5      # | d_a - cutoff |
    assert ref.margin(np.zeros((1, 1, 3)), np.zeros((1, 1, 3))) == np.inf


# ------------------------------------------------------------------------------------------------------------ header and binding
def test_header_declares_and_ops_exports_the_entry_points():
    from str2str_amd import ops
    from str2str_amd.ops import binding

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "str2str_hip.h")).read(), flags=re.S)
    protos = dict(re.findall(r"^int\s+(s2s_\w+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M))
    for name in NAMES:
        assert name in protos and name in ops.EXPORTS
        args = [a.strip() for a in protos[name].split(",")]
        assert args[-1] == "void* stream" and "double cutoff" in args and "int min_seq_sep" in args and "long long workspace_bytes" in args
        assert len(args) == len(binding._SIGNATURES[name])
    assert int(re.search(r"#define\s+S2S_LDDT_MAX_RES\s+(\d+)", hdr).group(1)) == ops.LDDT_MAX_RES == LDDT_MAX_RES >= 1024
    assert ops.ABI_VERSION >= 37 and callable(ops.ca_lddt_matrix) and callable(ops.ca_lddt_per_residue)
    # the workspace formula of the header, as the binding states it
    for n_a, L in ((1, 1), (3, 2), (5, 7), (2, 1024)):
        slots = (L * (L - 1) // 2 + 1) // 2 * 2
        assert lddt_workspace_bytes(n_a, L) == n_a * (12 * slots + 8 + 4 * L)
    assert "12 * S2S_LDDT_LIST_SLOTS(n_res) + 8 + 4 *" in hdr


def test_bad_sizes_are_invalid_value():
    """Sizes and parameters the kernels cannot take are rejected before any launch (hipErrorInvalidValue = 1), so this needs no device."""
    from str2str_amd import build, ops

    if not os.path.exists(ops.LIB_PATH):
        build.build(verbose=False)
    lib = ops.load_library()
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 40                                                # (a stated size; nothing is touched before the checks)
    nan, inf = float("nan"), float("inf")
    bad = [(0, 4, 8, 15.0, 1), (4, 0, 8, 15.0, 1), (4, 4, 0, 15.0, 1), (4, 4, ops.LDDT_MAX_RES + 1, 15.0, 1), (1 << 16, 1 << 15, 8, 15.0, 1),
           (4, 4, 8, 0.0, 1), (4, 4, 8, -1.0, 1), (4, 4, 8, nan, 1), (4, 4, 8, inf, 1), (4, 4, 8, 15.0, 0), (4, 4, 8, 15.0, -2)]
    for n_a, n_b, L, cutoff, sep in bad:
        assert lib.s2s_ca_lddt_matrix(p, n_a, p, n_b, L, cutoff, sep, p, p, big, None) == 1, (n_a, n_b, L, cutoff, sep)
    for args in ((None, 4, p, 4, 8, 15.0, 1, p, p, big), (p, 4, None, 4, 8, 15.0, 1, p, p, big), (p, 4, p, 4, 8, 15.0, 1, None, p, big),
                 (p, 4, p, 4, 8, 15.0, 1, p, None, big)):
        assert lib.s2s_ca_lddt_matrix(*args, None) == 1
    need = lddt_workspace_bytes(4, 8)
    assert lib.s2s_ca_lddt_matrix(p, 4, p, 4, 8, 15.0, 1, p, p, need - 1, None) == 1
    assert lib.s2s_ca_lddt_matrix(p, 4, p, 4, 8, 15.0, 1, p, p, 0, None) == 1
    for n, L, cutoff, sep in ((0, 8, 15.0, 1), (4, 0, 15.0, 1), (4, ops.LDDT_MAX_RES + 1, 15.0, 1), (4, 8, 0.0, 1), (4, 8, nan, 1), (4, 8, 15.0, 0)):
        assert lib.s2s_ca_lddt_per_residue(p, n, p, L, cutoff, sep, p, p, p, big, None) == 1, (n, L, cutoff, sep)
    for args in ((None, 4, p, 8, 15.0, 1, p, p, p, big), (p, 4, None, 8, 15.0, 1, p, p, p, big), (p, 4, p, 8, 15.0, 1, None, p, p, big),
                 (p, 4, p, 8, 15.0, 1, p, None, p, big), (p, 4, p, 8, 15.0, 1, p, p, None, big)):
        assert lib.s2s_ca_lddt_per_residue(*args, None) == 1
    assert lib.s2s_ca_lddt_per_residue(p, 4, p, 8, 15.0, 1, p, p, p, lddt_workspace_bytes(1, 8) - 1, None) == 1


def test_argument_checks_fire_before_the_device(monkeypatch):
    from str2str_amd import ops
    from str2str_amd.metrics import metrics
    from str2str_amd.ops import ensemble

    def touched(*a, **k):
        raise AssertionError("touched the device")

    monkeypatch.setattr(ensemble, "load_library", touched)
    x = torch.zeros(4, 8, 3)
    bad_matrix = [
        (dict(a=torch.zeros(4, 8)), "coordinates"), (dict(a=torch.zeros(4, 8, 2)), "coordinates"), (dict(a=torch.zeros(0, 8, 3)), "coordinates"),
        (dict(a=torch.zeros(4, 0, 3)), "coordinates"), (dict(a=x, b=torch.zeros(4, 9, 3)), "coordinates"), (dict(a=x, b=torch.zeros(8, 3)), "coordinates"),
        (dict(a=np.zeros((4, 8, 3), dtype=np.float32)), "tensors"), (dict(a=torch.zeros(2, ops.LDDT_MAX_RES + 1, 3)), "residues"),
        (dict(a=x, cutoff=0.0), "cutoff"), (dict(a=x, cutoff=float("nan")), "cutoff"), (dict(a=x, cutoff=float("inf")), "cutoff"),
        (dict(a=x, min_seq_sep=0), "min_seq_sep"), (dict(a=x, min_seq_sep=1.5), "min_seq_sep"), (dict(a=x), "no CPU fallback"),
    ]
    for kwargs, match in bad_matrix:
        with pytest.raises(ops.HipLibraryError, match=match):
            ops.ca_lddt_matrix(**kwargs)
    for model, target in ((torch.zeros(4, 8), torch.zeros(8, 3)), (x, torch.zeros(9, 3)), (x, torch.zeros(1, 8, 3)), (torch.zeros(0, 8, 3), torch.zeros(8, 3)),
                          (x.numpy(), torch.zeros(8, 3)), (x, torch.zeros(8, 3))):
        with pytest.raises(ops.HipLibraryError):
            ops.ca_lddt_per_residue(model, target)
    with pytest.raises(ops.HipLibraryError, match="cutoff"):
        ops.ca_lddt_per_residue(x, torch.zeros(8, 3), cutoff=-1.0)
    with pytest.raises(ops.HipLibraryError, match="min_seq_sep"):
        ops.ca_lddt_per_residue(x, torch.zeros(8, 3), min_seq_sep=0)

    # the metrics reach the device through _dev only: malformed coordinates stop there, a single structure needs no device at all
    monkeypatch.setattr(metrics, "_dev", lambda v: torch.as_tensor(np.asarray(v)).float().reshape((-1,) + np.shape(v)[-2:]))
    assert metrics.diversity_lddt({"one": np.zeros((1, 8, 3))}) == {"one": 1.0}
    for call in (lambda: metrics.pairwise_lddt(np.zeros((4, 8, 3))), lambda: metrics.diversity_lddt({"k": np.zeros((4, 8, 3))}),
                 lambda: metrics.coverage_lddt({"target": np.zeros((4, 8, 3)), "pred": np.zeros((2, 8, 3))}),
                 lambda: metrics.lddt(np.zeros((4, 8, 3)), np.zeros((8, 3))), lambda: metrics.cluster_lddt(np.zeros((4, 8, 3)), 0.5),
                 lambda: metrics.pairwise_lddt(np.zeros((4, 8, 3)), np.zeros((4, 9, 3)))):
        with pytest.raises(ops.HipLibraryError):
            call()
    recall, precision = metrics.coverage_lddt({"target": np.zeros((4, 8, 3))})
    assert recall == {"target": 1.0} and precision == {"target": 1.0}
    monkeypatch.setattr(metrics, "_dev", touched)
    for cutoff in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="cutoff"):
            metrics.cluster_lddt(np.zeros((4, 8, 3)), cutoff)


def test_metric_columns_accept_the_lddt_names():
    entry = load_eval_entry("s2s_eval_entry_lddt_cpu")
    five = ["val_clash", "val_bond", "js_pwd", "js_rg", "js_tica"]
    assert entry.metric_columns(["lddt_precision", "div_lddt", "lddt_recall"]) == five + ["lddt_precision", "div_lddt", "lddt_recall"]
    assert entry.metric_columns(["div_tm", "div_lddt"]) == five + ["div_tm", "div_lddt"]
    assert entry.metric_columns(None) == five
    assert entry.EXTRA_METRICS[-3:] == ("div_lddt", "lddt_recall", "lddt_precision")
    for bad in (["div_lddt", "div_lddt"], ["lddt"], "lddt_score"):
        with pytest.raises(ValueError):
            entry.metric_columns(bad)
