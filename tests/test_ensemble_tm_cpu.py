"""The TM-score feature without a GPU: its yardstick (tests/ref_tm64.py) held to the properties the definition promises, the C-ABI
surface, the evaluation columns, and the argument checks that must fire before any device call."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ref_tm64 as ref
from conftest import ROOT, record_margin
from ensemble_cases import load_eval_entry
from str2str_amd.metrics.metrics import tm_d0   # (the package's d0 drives the yardstick below: the two must be one function of L)

NAMES = ("s2s_ca_tm_matrix", "s2s_ca_tm_superpose")


def _pairs(rng, L, n=8):
    base = ref.random_walk(rng, L)
    return ref.make_ensemble(rng, n, L, base), ref.make_ensemble(rng, n, L, base, first_kind=3)


@pytest.mark.parametrize("L", [3, 5, 16, 22, 35, 80])
def test_every_reweighting_step_raises_the_score(L):
    """f is convex in d^2, so the weighted least-squares step maximises a minorant of the score: no step may lower it (1e-12 of slack
    for the rounding of a converged iteration)."""
    a, b = _pairs(np.random.default_rng(100 + L), L)
    trace = ref.tm_search(a, b, d0=tm_d0(L))["trace"]                      # [seeds, iters, pairs]
    assert trace.shape[1] == 33
    worst = float(np.diff(trace, axis=1).min())
    record_margin("ensemble_tm_ref_most_negative_step", max(-worst, 0.0), 1e-12)
    assert worst >= -1e-12, worst


@pytest.mark.parametrize("L", [3, 5, 22, 35])
def test_moment_form_of_the_yardstick_is_the_direct_one(L):
    """tm_search works from 16 weighted moments of centred coordinates; evaluated with the plain weighted Kabsch on the raw coordinates
    (up to 50 A from the origin) it gives the same values and the same superpositions.  The intermediate scores of a three-point chain move
    by 2e-11 under a 1e-15 perturbation of the inputs; they are held to the 1e-9 of the device parity, the results to 1e-12."""
    a, b = _pairs(np.random.default_rng(150 + L), L)
    fast, slow = ref.tm_search(a, b), ref.tm_search(a, b, direct=True)
    assert np.abs(fast["tm"] - slow["tm"]).max() <= 1e-12 and np.abs(fast["trace"] - slow["trace"]).max() <= 1e-9
    x, y = a.astype(np.float64), b.astype(np.float64)
    for r in (fast, slow):
        assert np.abs(ref.score_under(x, y, r["rot"], r["trans"], tm_d0(L))[1] - r["tm"]).max() <= 1e-12
        assert np.abs(np.linalg.det(r["rot"]) - 1.0).max() <= 1e-12


@pytest.mark.parametrize("L", [16, 35, 80])
def test_planted_half_chain_is_found(L):
    rng = np.random.default_rng(200 + L)
    for _ in range(4):
        a, b, fraction = ref.planted_pair(rng, L)
        got = float(ref.tm_matrix(a[None], b[None], d0=tm_d0(L))[0, 0])
        whole = float(ref.kabsch_tm(a[None], b[None], d0=tm_d0(L))[0, 0])
        print(f"L={L}: planted {fraction:.4f}  search {got:.4f}  whole-chain Kabsch {whole:.4f}")
        assert fraction <= got <= 1.0 and whole <= got + 1e-12


def test_d0():
    for fn in (tm_d0, ref.tm_d0):
        assert all(fn(L) == 0.5 for L in range(1, 22))
        assert all(fn(L) == 1.24 * np.cbrt(L - 15.0) - 1.8 > 0.5 for L in (22, 35, 100, 800))
        assert round(fn(22), 4) == 0.5720 and round(fn(100), 4) == 3.6521


@pytest.mark.parametrize("L", [1, 2, 3, 5, 22, 35])
def test_identical_inputs_score_one(L):
    rng = np.random.default_rng(300 + L)
    a = np.asarray([ref.rigid_move(rng, ref.random_walk(rng, L)) for _ in range(3)], dtype=np.float32)
    assert np.abs(np.diag(ref.tm_matrix(a, a, d0=tm_d0(L))) - 1.0).max() <= 1e-12


def test_seed_list():
    assert tm_d0(4) == ref.tm_d0(4)
    assert [len(ref.tm_seeds(L)) for L in (4, 5, 22, 35)] == [1, 5, 15, 13]
    assert ref.tm_seeds(22)[:6] == [(0, 22), (0, 11), (5, 11), (10, 11), (11, 11), (0, 5)] and ref.tm_seeds(22)[-1] == (17, 5)
    for L in range(1, 900):
        seeds = ref.tm_seeds(L)
        assert seeds[0] == (0, L) and len(seeds) <= 16 and all(0 <= s and n >= 1 and s + n <= L for s, n in seeds)


def test_metric_columns_accept_the_tm_names():
    entry = load_eval_entry("s2s_eval_entry_tm_cpu")
    five = ["val_clash", "val_bond", "js_pwd", "js_rg", "js_tica"]
    assert entry.metric_columns(["tm_precision", "div_tm", "tm_recall"]) == five + ["tm_precision", "div_tm", "tm_recall"]
    assert entry.metric_columns(["div_rmsd", "div_tm"]) == five + ["div_rmsd", "div_tm"]
    assert entry.metric_columns(None) == five
    with pytest.raises(ValueError):
        entry.metric_columns(["div_tm", "div_tm"])


def test_header_declares_and_ops_exports_the_entry_points():
    import re

    from str2str_amd import ops

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "str2str_hip.h")).read(), flags=re.S)
    protos = dict(re.findall(r"^int\s+(s2s_\w+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M))
    for name in NAMES:
        assert name in protos and name in ops.EXPORTS and "void* stream" in protos[name] and "double d0" in protos[name]
    assert int(re.search(r"#define\s+S2S_TM_MAX_RES\s+(\d+)", hdr).group(1)) == ops.TM_MAX_RES
    assert ops.ABI_VERSION >= 35 and callable(ops.ca_tm_matrix) and callable(ops.ca_tm_superpose)


def test_bad_sizes_are_invalid_value():
    """Sizes the kernels cannot take are rejected before any launch (hipErrorInvalidValue = 1), so this needs no device."""
    from str2str_amd import build, ops

    if not os.path.exists(ops.LIB_PATH):
        build.build(verbose=False)
    lib = ops.load_library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for n_a, n_b, L in ((0, 4, 8), (4, 0, 8), (4, 4, 0), (4, 4, ops.TM_MAX_RES + 1), (1 << 16, 1 << 15, 8), (1, 4 * 65535 + 1, 8)):
        assert lib.s2s_ca_tm_matrix(p, n_a, p, n_b, L, 0.0, p, None) == 1, (n_a, n_b, L)
    assert lib.s2s_ca_tm_matrix(None, 4, p, 4, 8, 0.0, p, None) == 1 and lib.s2s_ca_tm_matrix(p, 4, p, 4, 8, 0.0, None, None) == 1
    for n, L in ((0, 8), (4, 0), (4, ops.TM_MAX_RES + 1)):
        assert lib.s2s_ca_tm_superpose(p, n, p, L, 0.0, p, p, None) == 1, (n, L)
    assert lib.s2s_ca_tm_superpose(p, 4, p, 8, 0.0, p, None, None) == 1


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
        (dict(a=np.zeros((4, 8, 3), dtype=np.float32)), "tensors"), (dict(a=torch.zeros(2, ops.TM_MAX_RES + 1, 3)), "no CPU fallback"),
        (dict(a=x), "no CPU fallback"),
    ]
    for kwargs, match in bad_matrix:
        with pytest.raises(ops.HipLibraryError, match=match):
            ops.ca_tm_matrix(**kwargs)
    for mobile, target in ((torch.zeros(4, 8), torch.zeros(8, 3)), (x, torch.zeros(9, 3)), (x, torch.zeros(1, 8, 3)), (torch.zeros(0, 8, 3), torch.zeros(8, 3)),
                           (x.numpy(), torch.zeros(8, 3)), (x, torch.zeros(8, 3))):
        with pytest.raises(ops.HipLibraryError):
            ops.ca_tm_superpose(mobile, target)
    for d0 in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ops.HipLibraryError, match="d0"):
            ensemble._tm_d0(d0)
    assert ensemble._tm_d0(None) == 0.0 and ensemble._tm_d0(2) == 2.0

    # the metrics reach the device through _dev only: malformed coordinates stop there, a single structure needs no device at all
    monkeypatch.setattr(metrics, "_dev", lambda v: torch.as_tensor(np.asarray(v)).float().reshape((-1,) + np.shape(v)[-2:]))
    assert metrics.diversity_tm({"one": np.zeros((1, 8, 3))}) == {"one": 1.0}
    for call in (lambda: metrics.pairwise_tm(np.zeros((4, 8, 3))), lambda: metrics.diversity_tm({"k": np.zeros((4, 8, 3))}),
                 lambda: metrics.coverage_tm({"target": np.zeros((4, 8, 3)), "pred": np.zeros((2, 8, 3))}),
                 lambda: metrics.tm_superpose(np.zeros((4, 8, 3)), np.zeros((8, 3))),
                 lambda: metrics.pairwise_tm(np.zeros((4, 8, 3)), np.zeros((4, 9, 3)))):
        with pytest.raises(ops.HipLibraryError):
            call()
    recall, precision = metrics.coverage_tm({"target": np.zeros((4, 8, 3))})
    assert recall == {"target": 1.0} and precision == {"target": 1.0}


def test_unknown_names_stay_unknown(tmp_path, monkeypatch):
    """``tm_score`` and ``rmsd`` are not column names (the new ones are div_tm / tm_recall / tm_precision), and a bad list is rejected
    before the device."""
    from str2str_amd.metrics import metrics

    entry = load_eval_entry("s2s_eval_entry_tm_cpu")
    monkeypatch.setattr(metrics, "_dev", lambda x: (_ for _ in ()).throw(AssertionError("touched the device")))
    for bad in (["div_tm", "tm_score"], ["tm"], "rmsd", ["tm_recall", "tm_recall"]):
        with pytest.raises(ValueError):
            entry.evaluate_prediction(str(tmp_path), os.path.join(ROOT, "tests", "golden", "pdb"), tag="t", extra_metrics=bad)
