"""Solvent accessibility without a GPU: the sphere table, the yardstick (tests/ref_sasa.py) held to closed forms, the margins that make every
device case a parity input, the C-ABI surface, the argument checks, the numpy tails of the ensemble metrics and the evaluation switch."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import ref_sasa as ref
import sasa_cases as cases
import ss_cases
from conftest import ROOT

ULP = 2.0 ** -52
MARGIN = 1e-9


# ---------------------------------------------------------------------------------------------------------------------- the sphere
@pytest.mark.parametrize("P", (1, 2, 63, 64, 65, 96, 129, 513, 960, 1024))
def test_sphere_table_is_the_bindings_and_has_unit_vectors(P):
    from str2str_amd import ops

    mine, theirs = ref.sphere(P), ops.sphere_points(P)
    assert theirs.dtype == np.float64 and theirs.shape == (P, 3) and mine.tobytes() == theirs.tobytes()
    norm = np.sqrt((mine * mine).sum(1))
    assert np.abs(norm - 1.0).max() <= 4 * ULP
    assert len({row.tobytes() for row in mine}) == P            # P distinct points


def test_sphere_points_rejects_what_the_kernel_cannot_take():
    from str2str_amd import ops

    for bad in (0, -1, ops.SASA_MAX_POINTS + 1, 96.5, True):
        with pytest.raises(ops.HipLibraryError, match="n_points"):
            ops.sphere_points(bad)


# ------------------------------------------------------------------------------------------------------------------ closed forms
def _atoms_of(centres, radii):
    """A one-residue structure whose first len(centres) slots exist -> (atoms [1, 5, 3] float32, exists [1, 5], radii [1, 5])."""
    x, ex, r = np.zeros((1, 5, 3), dtype=np.float32), np.zeros((1, 5), dtype=bool), np.full((1, 5), np.nan)
    for k, (c, rad) in enumerate(zip(centres, radii)):
        x[0, k], ex[0, k], r[0, k] = c, True, rad
    return x, ex, r


@pytest.mark.parametrize("P", (1, 96, 960))
def test_an_isolated_atom_keeps_every_point(P):
    got = ref.sasa(*_atoms_of([(3.0, -2.0, 7.5)], [1.7]), probe=1.4, n_points=P)
    assert got["counts"].tolist() == [[P, 0, 0, 0, 0]] and got["margin"] == np.inf
    want = 4.0 * math.pi * (1.7 + 1.4) ** 2
    assert abs(got["per_residue"][0] - want) <= 4 * ULP * want and got["total"] == got["per_residue"][0]


def test_an_atom_inside_a_larger_one_has_no_surface():
    got = ref.sasa(*_atoms_of([(0.0, 0.0, 0.0), (0.2, 0.1, -0.1)], [1.0, 3.0]), probe=1.4, n_points=96)
    assert got["counts"][0, 0] == 0 and 0 < got["counts"][0, 1] <= 96
    # an atom that does not exist buries nothing and has no surface, wherever its coordinates are
    x, ex, r = _atoms_of([(0.0, 0.0, 0.0), (0.2, 0.1, -0.1)], [1.0, 3.0])
    ex[0, 1] = False
    alone = ref.sasa(x, ex, r, probe=1.4, n_points=96)
    assert alone["counts"].tolist() == [[96, 0, 0, 0, 0]]


@pytest.mark.parametrize("P", (96, 960))
def test_two_spheres_against_the_cap_formula(P):
    ca, cb, ra, rb, probe = (0.0, 0.0, 0.0), (3.5, 0.3, -0.2), 1.7, 1.52, 1.4
    got = ref.sasa(*_atoms_of([ca, cb], [ra, rb]), probe=probe, n_points=P)
    d = math.sqrt(3.5 ** 2 + 0.3 ** 2 + 0.2 ** 2)
    Ra, Rb = ra + probe, rb + probe
    for k, (R1, R2) in enumerate(((Ra, Rb), (Rb, Ra))):
        want = (1.0 + (d * d + R1 * R1 - R2 * R2) / (2.0 * d * R1)) / 2.0
        err = abs(got["counts"][0, k] / P - want)
        print(f"P = {P}, sphere {k}: accessible fraction {got['counts'][0, k] / P:.5f}, cap formula {want:.5f}, error {err * P:.2f} / P")
        assert err <= 4.0 / P


def test_a_helix_is_more_buried_than_the_same_chain_extended():
    L = 20
    exists, radii = np.ones((L, 5), dtype=bool), ref.default_radii(L)
    helix = ref.relative(ss_cases.regular(-57.0, -47.0, L)[None], exists, radii)
    extended = ref.relative(ss_cases.regular(-120.0, 130.0, L)[None], exists, radii)
    print(f"mean relative accessibility: helix {helix.mean():.4f}, extended {extended.mean():.4f}")
    assert helix.shape == (1, L) and (helix >= 0.0).all() and (helix <= 1.0).all() and (extended <= 1.0).all()
    assert helix.mean() < extended.mean()
    assert helix[0, 8:12].mean() < helix[0, [0, L - 1]].mean()  # the middle of a helix is more buried than its ends


# -------------------------------------------------------------------------------------------------------- the device cases' margin
@pytest.mark.parametrize("tag", cases.tags())
def test_every_device_case_is_a_parity_input(tag):
    """The device forms every point and every squared distance as the yardstick does (float64, one rounding per operation): a case whose
    nearest comparison is >= 1e-9 (relative) from flipping has the same counts on both sides.  A condition on the cases; none is left out."""
    c, want = cases.case(tag), cases.reference(tag)
    R, L = c.atoms.shape[:2]
    print(f"{tag}: margin {want['margin']:.3e}")
    assert c.atoms.dtype == np.float32 and c.atoms.shape[2:] == (5, 3) and c.exists.shape == c.radii.shape == (L, 5)
    assert want["counts"].shape == (R, L, 5) and want["counts"].dtype == np.int32 and want["per_residue"].shape == (R, L)
    assert want["margin"] >= MARGIN
    assert (want["counts"][:, ~c.exists] == 0).all() and (want["counts"] <= c.n_points).all()


def test_the_cases_cover_what_they_are_there_for():
    assert set(cases.SHAPES) >= {(1, 2), (2, 1), (4, 3), (13, 17), (31, 9), (64, 3), (65, 17), (129, 4)}
    assert {1, 63, 64, 65, 960} <= set(cases.POINTS) and [c[:2] for c in cases.LONG] == [(257, 2)]
    for L, R in cases.SHAPES:
        c = cases.case(f"L{L}_R{R}")
        assert (c.aatype == ref.GLY).any() and not c.exists[c.aatype == ref.GLY, 4].any() and c.n_points == 96 and c.probe == 1.4
    # the COMPACT members: most atoms are neighbours of each other (more than a list of 64 or 128 entries would hold), almost all buried
    for tag, share in (("L65_R17", 0.5), ("L129_R4", 0.25)):
        c, want = cases.case(tag), cases.reference(tag)
        x = c.atoms[ss_cases.COMPACT].reshape(-1, 3).astype(np.float64)
        near = (np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1)) < 2 * (1.7 + 1.4)).sum(1) - 1
        assert near.mean() > share * len(x) and near.min() > 64 and near.max() > 128, tag
        assert want["total"][ss_cases.COMPACT] < 0.25 * want["total"][ss_cases.MIXED]
    by_residue, plain = cases.case("L31_R9_radii_by_residue"), cases.case("L31_R9")
    assert len(np.unique(by_residue.radii, axis=0)) > 5 and (cases.reference("L31_R9_radii_by_residue")["counts"] != cases.reference("L31_R9")["counts"]).any()
    assert cases.case("L31_R9_probe_0").probe == 0.0 and (cases.reference("L31_R9_probe_0")["total"] < cases.reference("L31_R9")["total"]).all()
    missing = cases.case("L31_R9_missing_residue")
    assert not missing.exists[5].any() and (cases.reference("L31_R9_missing_residue")["per_residue"][:, 5] == 0.0).all()
    assert (plain.exists.sum(), missing.exists.sum()) == (154, 146)


# ------------------------------------------------------------------------------------------------------------ header and binding
def test_abi_and_interface_are_declared():
    from str2str_amd import build, ops
    from str2str_amd.metrics import metrics
    from str2str_amd.ops import binding

    text = open(os.path.join(ROOT, "include", "str2str_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = dict(re.findall(r"^int\s+(s2s_\w+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M))
    name = "s2s_backbone_sasa"
    assert name in protos and name in ops.EXPORTS
    args = [" ".join(a.split()) for a in protos[name].split(",")]
    assert args[-1] == "void* stream" and "int n_res" in args and "double probe" in args and "const double* sphere" in args and "int* counts" in args
    assert len(args) == len(binding._SIGNATURES[name]) == 12
    assert int(re.search(r"#define\s+S2S_SASA_MAX_RES\s+(\d+)", hdr).group(1)) == ops.SASA_MAX_RES >= 512
    assert int(re.search(r"#define\s+S2S_SASA_MAX_POINTS\s+(\d+)", hdr).group(1)) == ops.SASA_MAX_POINTS == 1024
    assert ops.ABI_VERSION == 40
    assert int(re.search(r"return (\d+);", open(os.path.join(ROOT, "str2str_amd", "csrc", "abi.hip")).read()).group(1)) == 40
    assert build.UNITS["ensemble_sasa.hip"] == ["-ffp-contract=off"]
    section = text.split("Solvent accessibility")[1].split("S2S_SASA_MAX_RES")[0]
    assert "no side chains" in section and "Shrake" in section and "Rupley" in section
    assert metrics.SolventAccessibility._fields == ("counts", "per_residue", "total") and metrics.SASA_RADII == ref.RADII
    for fn in ("solvent_accessibility", "relative_accessibility", "mean_sasa", "sasa_mae", "js_sasa"):
        assert callable(getattr(metrics, fn)), fn
    sig = inspect.signature(ops.backbone_sasa).parameters
    assert list(sig) == ["atoms", "atom_exists", "radii", "probe", "n_points", "max_structures"]
    assert (sig["probe"].default, sig["n_points"].default, sig["max_structures"].default) == (1.4, 96, None)


def test_bad_sizes_are_invalid_value():
    """What the kernel cannot take is rejected before any launch (hipErrorInvalidValue = 1), so this needs no device."""
    from str2str_amd import build, ops

    if not os.path.exists(ops.LIB_PATH):
        build.build(verbose=False)
    lib = ops.load_library()
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(n=4, L=8, probe=1.4, P=96, ptrs=(p,) * 7):
        return lib.s2s_backbone_sasa(ptrs[0], n, L, ptrs[1], ptrs[2], probe, ptrs[3], P, ptrs[4], ptrs[5], ptrs[6], None)

    for kwargs in (dict(L=ops.SASA_MAX_RES + 1), dict(L=0), dict(L=-3), dict(n=0), dict(n=-1), dict(P=0), dict(P=-5), dict(P=ops.SASA_MAX_POINTS + 1),
                   dict(probe=-0.1), dict(probe=float("inf")), dict(probe=float("nan"))):
        assert call(**kwargs) == 1, kwargs
    for k in range(7):
        assert call(ptrs=(p,) * k + (None,) + (p,) * (6 - k)) == 1, k


def test_argument_checks_fire_before_the_device(monkeypatch):
    from str2str_amd import ops
    from str2str_amd.metrics import metrics
    from str2str_amd.ops import ensemble

    def touched(*a, **k):
        raise AssertionError("touched the device")

    monkeypatch.setattr(ensemble, "load_library", touched)
    x = torch.zeros(4, 8, 5, 3)
    ok = dict(atom_exists=np.ones((8, 5), dtype=np.uint8), radii=ref.default_radii(8))
    nan_radius, gone = ref.default_radii(8), np.ones((8, 5), dtype=np.uint8)
    nan_radius[3, 4], gone[3, 4] = np.nan, 0
    bad = [(dict(atoms=torch.zeros(4, 8, 3)), "atoms"), (dict(atoms=torch.zeros(4, 8, 14, 3)), "atoms"), (dict(atoms=torch.zeros(0, 8, 5, 3)), "atoms"),
           (dict(atoms=x.numpy()), "tensor"), (dict(atoms=torch.zeros(1, ops.SASA_MAX_RES + 1, 5, 3)), "residues"),
           (dict(atoms=x, max_structures=0), "max_structures"), (dict(atoms=x, max_structures=1.5), "max_structures"),
           (dict(atoms=x, atom_exists=np.ones((7, 5), dtype=np.uint8)), "atom_exists"), (dict(atoms=x, atom_exists=np.ones((8, 5))), "atom_exists"),
           (dict(atoms=x, radii=ref.default_radii(7)), "radii"), (dict(atoms=x, radii=np.zeros((8, 5))), "radii"),
           (dict(atoms=x, radii=-ref.default_radii(8)), "radii"), (dict(atoms=x, radii=nan_radius), "radii"),
           (dict(atoms=x, probe=-1.0), "probe"), (dict(atoms=x, probe=float("nan")), "probe"), (dict(atoms=x, probe=float("inf")), "probe"),
           (dict(atoms=x, n_points=0), "n_points"), (dict(atoms=x, n_points=ops.SASA_MAX_POINTS + 1), "n_points"), (dict(atoms=x, n_points=96.5), "n_points"),
           (dict(atoms=x), "no CPU fallback"), (dict(atoms=x, radii=nan_radius, atom_exists=gone), "no CPU fallback"),
           (dict(atoms=x.double()), "no CPU fallback")]
    for kwargs, match in bad:
        with pytest.raises(ops.HipLibraryError, match=match):
            ops.backbone_sasa(**{**ok, **kwargs})
    monkeypatch.setattr(metrics, "_backbone_dev", lambda a: torch.as_tensor(np.asarray(a)).float())
    with pytest.raises(ValueError, match="aatype"):
        metrics.solvent_accessibility(np.zeros((2, 8, 5, 3)), aatype=np.zeros(7, dtype=int))
    with pytest.raises(ValueError, match="radii"):
        metrics.relative_accessibility(np.zeros((2, 8, 5, 3)), radii=np.ones((8, 4)))
    monkeypatch.undo()
    for shape in ((4, 8, 3), (4, 8, 14, 3), (8, 5)):
        with pytest.raises(ValueError, match="backbone atoms"):
            metrics.solvent_accessibility(np.zeros(shape))


# ------------------------------------------------------------------------------------------------------- the numpy tails of the metrics
def yardstick_as_device(monkeypatch):
    """``ops.backbone_sasa`` answered by the yardstick on host tensors, so that everything after the kernel runs without a device."""
    from str2str_amd import ops
    from str2str_amd.metrics import metrics

    def fake(atoms, atom_exists, radii, probe=1.4, n_points=96, max_structures=None):
        got = ref.ensemble(atoms.numpy(), np.asarray(atom_exists), np.asarray(radii), probe, n_points)
        return torch.from_numpy(got["counts"]), torch.from_numpy(got["per_residue"]), torch.from_numpy(got["total"])

    monkeypatch.setattr(ops, "backbone_sasa", fake)
    monkeypatch.setattr(metrics, "_backbone_dev", lambda a: (torch.as_tensor(np.array(a))[None] if np.ndim(a) == 3 else torch.as_tensor(np.array(a))).float().contiguous())


def test_ensemble_metrics_are_the_plain_numpy_tails(monkeypatch):
    from str2str_amd.metrics import metrics

    yardstick_as_device(monkeypatch)
    c = cases.case("L13_R17")
    both = {"target": c.atoms[:9], "pred": c.atoms[6:]}
    want = {k: ref.ensemble(v, c.exists, c.radii) for k, v in both.items()}
    rel = {k: ref.relative(v, c.exists, c.radii, in_chain=want[k]["per_residue"]) for k, v in both.items()}
    res = metrics.solvent_accessibility(both["pred"], c.aatype)
    assert all((getattr(res, k) == want["pred"][k]).all() for k in res._fields) and res.counts.dtype == np.int32
    got_rel = metrics.relative_accessibility(both["pred"], c.aatype)
    assert got_rel.dtype == np.float64 and (got_rel == rel["pred"]).all() and (got_rel >= 0.0).all() and (got_rel <= 1.0).all()
    one = metrics.solvent_accessibility(both["pred"][2], c.aatype)            # a single structure without the leading axis
    assert (one.per_residue == want["pred"]["per_residue"][2:3]).all()

    mean = metrics.mean_sasa(both, c.aatype)
    assert mean == {k: np.around(float(want[k]["total"].mean()), decimals=4) for k in both} and mean["pred"] != mean["target"]
    mae = metrics.sasa_mae(both, "target", c.aatype)
    assert mae["target"] == 0.0 and mae["pred"] == np.around(float(np.abs(rel["pred"].mean(0) - rel["target"].mean(0)).mean()), decimals=4) > 0.0
    lo, hi = want["target"]["total"].min(), want["target"]["total"].max()
    hist = {k: np.histogram(want[k]["total"], bins=50, range=(lo, hi))[0] + metrics.PSEUDO_C for k in both}
    js = metrics.js_sasa(both, "target", aatype=c.aatype)
    assert js["target"] == 0.0 and js["pred"] == np.around(metrics._js(hist["pred"], hist["target"]), decimals=4) and 0.0 < js["pred"] < 1.0
    w = {"pred": np.linspace(0.5, 2.0, len(both["pred"]))}
    hist_w = np.histogram(want["pred"]["total"], bins=12, weights=w["pred"], range=(lo, hi))[0] + metrics.PSEUDO_C
    hist_t = np.histogram(want["target"]["total"], bins=12, range=(lo, hi))[0] + metrics.PSEUDO_C
    assert metrics.js_sasa(both, "target", n_bins=12, weights=w, aatype=c.aatype)["pred"] == np.around(metrics._js(hist_w, hist_t), decimals=4)

    same = {"target": both["target"], "pred": both["target"].copy()}          # an ensemble against itself
    assert metrics.sasa_mae(same, "target", c.aatype)["pred"] == 0.0 and metrics.js_sasa(same, "target", aatype=c.aatype)["pred"] == 0.0
    # radii of one's own reach the kernel, and the residues are grouped by radii and existing atoms for the denominators
    by_residue = cases.case("L31_R9_radii_by_residue")
    got = metrics.relative_accessibility(by_residue.atoms[:2], by_residue.aatype, radii=by_residue.radii)
    assert (got == ref.relative(by_residue.atoms[:2], by_residue.exists, by_residue.radii)).all()
