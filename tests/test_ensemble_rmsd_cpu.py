"""The RMSD feature's C-ABI surface, its yardstick and the evaluation option -- no GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, record_margin
from ensemble_cases import load_eval_entry
from test_ensemble_rmsd import LENGTHS, U64, horn, make_ensemble, make_weights, random_walk, ref_msd_matrix

NAMES = ("s2s_ca_rmsd_matrix", "s2s_ca_superpose", "s2s_apply_xform")


@pytest.fixture(scope="module")
def built_library():
    """The shared library is a build artefact (git-ignored): build it with hipcc when it is not there yet (cross-compiles for gfx950
    without a GPU)."""
    from str2str_amd import build, ops

    if not os.path.exists(ops.LIB_PATH):
        build.build(verbose=False)
    return ops.LIB_PATH


def test_header_declares_and_ops_exports_the_entry_points():
    from str2str_amd import ops

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "str2str_hip.h")).read(), flags=re.S)
    protos = dict(re.findall(r"^int\s+(s2s_\w+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M))
    for name in NAMES:
        assert name in protos and name in ops.EXPORTS
        assert "void* stream" in protos[name] and protos[name].count(",") + 1 == len(ops.binding._SIGNATURES[name])
    assert callable(ops.ca_rmsd_matrix) and callable(ops.ca_superpose) and callable(ops.apply_xform)


def test_library_exports_the_entry_points(built_library):
    lib = ctypes.CDLL(built_library)
    for name in NAMES:
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)


def test_bad_sizes_are_invalid_value(built_library):
    """L < 1 or n < 1 is rejected before any launch (hipErrorInvalidValue = 1), so this needs no device."""
    from str2str_amd import ops

    lib = ops.load_library()
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for n_a, n_b, L in ((0, 4, 8), (4, 0, 8), (4, 4, 0)):
        assert lib.s2s_ca_rmsd_matrix(p, n_a, p, n_b, L, None, p, p, 4096, None) == 1
    assert lib.s2s_ca_rmsd_matrix(p, 4, p, 4, 8, None, p, p, 10, None) == 1          # workspace too small
    assert lib.s2s_ca_superpose(p, 0, p, 8, None, p, p, None) == 1 and lib.s2s_ca_superpose(p, 4, p, 0, None, p, p, None) == 1
    assert lib.s2s_apply_xform(p, p, 0, 8, p, None) == 1 and lib.s2s_apply_xform(p, p, 4, 0, p, None) == 1


@pytest.mark.parametrize("wmode", ["none", "third", "two"])
@pytest.mark.parametrize("L", LENGTHS)
def test_svd_reference_agrees_with_eigvalsh(L, wmode):
    """The yardstick of the GPU tests (SVD Kabsch) against an independent float64 evaluation (largest eigenvalue of Horn's 4 x 4),
    within the MSD bound the kernels are held to."""
    rng = np.random.default_rng(1000 + L)
    base = random_walk(rng, L)
    w = make_weights(rng, L, wmode)
    a, _ = make_ensemble(rng, 24, L, base)
    b, _ = make_ensemble(rng, 17, L, base, first_kind=3)
    msd, s_raw, _ = ref_msd_matrix(a, b, w)
    ww = np.ones(L) if w is None else w.astype(np.float64)
    cen = lambda x: x.astype(np.float64) - (ww[:, None] * x).sum(-2, keepdims=True) / ww.sum()  # noqa: E731
    da, db = cen(a), cen(b)
    lam = np.linalg.eigvalsh(horn(np.einsum("ail,bim->ablm", da * ww[:, None], db)))[..., -1]
    g = lambda d: (ww * (d * d).sum(-1)).sum(-1)  # noqa: E731
    msd2 = (g(da)[:, None] + g(db)[None, :] - 2.0 * lam) / ww.sum() if L > 1 else np.zeros_like(msd)
    ratio = float((np.abs(msd - msd2) / (8.0 * U64 * s_raw)).max())
    record_margin("ensemble_rmsd_svd_vs_eigvalsh_msd_over_bound", ratio, 1.0)
    assert ratio <= 1.0, ratio


def test_unknown_extra_metric_is_rejected_before_the_device(tmp_path, monkeypatch):

    entry = load_eval_entry("s2s_eval_entry_cpu")
    assert entry.metric_columns(None) == ["val_clash", "val_bond", "js_pwd", "js_rg", "js_tica"]
    assert entry.metric_columns(["rmsd_recall", "div_rmsd"])[5:] == ["rmsd_recall", "div_rmsd"]
    from str2str_amd.metrics import metrics

    monkeypatch.setattr(metrics, "_dev", lambda x: (_ for _ in ()).throw(AssertionError("touched the device")))
    for bad in (["div_rmsd", "tm_score"], ["div_rmsd", "div_rmsd"], "rmsd"):
        with pytest.raises(ValueError):
            entry.evaluate_prediction(str(tmp_path), os.path.join(ROOT, "tests", "golden", "pdb"), tag="t", extra_metrics=bad)


def test_extra_metrics_parse_from_the_command_line(monkeypatch):
    from str2str_amd.utils import config as C

    monkeypatch.setenv("TEST_DATA", "/nonexistent")
    cfg = C.compose(os.path.join(ROOT, "configs"), "eval.yaml", ["+extra_metrics=[div_rmsd,rmsd_recall,rmsd_precision]"])
    assert list(cfg.get("extra_metrics")) == ["div_rmsd", "rmsd_recall", "rmsd_precision"]
    assert C.compose(os.path.join(ROOT, "configs"), "eval.yaml", []).get("extra_metrics") is None


def test_argument_checks_fire_before_the_library(monkeypatch):
    """``ca_rmsd_matrix`` and ``ca_superpose`` look at their arguments before they load the library: the malformed inputs of
    tests/test_ensemble_tm_cpu.py raise HipLibraryError with ``load_library`` out of reach."""
    import torch

    from str2str_amd import ops
    from str2str_amd.ops import ensemble

    def touched(*a, **k):
        raise AssertionError("loaded the library")

    monkeypatch.setattr(ensemble, "load_library", touched)
    x = torch.zeros(4, 8, 3)
    for kwargs in (dict(a=torch.zeros(4, 8)), dict(a=torch.zeros(4, 8, 2)), dict(a=torch.zeros(0, 8, 3)), dict(a=torch.zeros(4, 0, 3)),
                   dict(a=x, b=torch.zeros(4, 9, 3)), dict(a=x, b=torch.zeros(8, 3)), dict(a=np.zeros((4, 8, 3), dtype=np.float32))):
        with pytest.raises(ops.HipLibraryError):
            ops.ca_rmsd_matrix(**kwargs)
    for mobile, target in ((torch.zeros(4, 8), torch.zeros(8, 3)), (x, torch.zeros(9, 3)), (x, torch.zeros(1, 8, 3)), (torch.zeros(0, 8, 3), torch.zeros(8, 3)),
                           (x.numpy(), torch.zeros(8, 3)), (x, torch.zeros(8, 3))):
        with pytest.raises(ops.HipLibraryError):
            ops.ca_superpose(mobile, target)
