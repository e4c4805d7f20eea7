"""The backbone violations without a GPU: the yardstick (tests/ref_violations.py) held to the reference's own functions through
tests/golden/violations.npz and to cases worked by hand, the margin that makes every device case a parity input, the C-ABI surface, the PDB
reader of the five backbone atoms and the evaluation columns."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import torch

import ref_violations as ref
import violations_cases as cases
from conftest import GOLDEN, ROOT, golden, record_margin
from ensemble_cases import load_eval_entry

FIXTURE_BOUND = 5e-7   # x max(1, |value|): the reference works in float32 (2^-23 = 1.2e-7); 1.0e-7 was measured when the fixture was made
TAGS = ("ideal12", "ideal40", "stretched", "o_n", "hairpin")


# ------------------------------------------------------------------------------------------------------------- the yardstick itself
@pytest.mark.parametrize("tag", TAGS)
def test_yardstick_against_the_reference(tag):
    """tests/golden/violations.npz: between_residue_bond_loss, between_residue_clash_loss, extreme_ca_ca_distance_violations and masked_mean
    of the reference in float32.  Every mask is equal (the case's margin, >= 1e-4, is a hundred float32 ulps of a 10 A distance) and every
    loss and fraction is within 5e-7 max(1, |value|)."""
    g = golden("violations.npz")
    atoms, exists, aatype, ri = cases.fixture_cases()[tag]
    assert atoms.dtype == np.float32 and (atoms == g[f"{tag}_atoms"]).all() and (aatype == g[f"{tag}_aatype"]).all()
    assert (ri == g[f"{tag}_residue_index"]).all() and (aatype == ref.GLY).any() and (aatype == ref.PRO).any() and (np.diff(ri) != 1).sum() == 1
    assert ref.margin(atoms, exists, aatype, ri) >= 1e-4
    got = ref.violations(atoms, exists, aatype, ri)
    assert (got["bond_mask"] == g[f"{tag}_bond_mask"]).all() and (got["clash_atom_mask"] == g[f"{tag}_clash_atom_mask"]).all()
    assert got["n_clash_pairs"] >= got["clash_atom_mask"].any(1).sum() / 2
    for k in ref.LOSSES + ref.FRACTIONS + ("per_residue_loss_sum",):
        want = g[f"{tag}_{k}"].astype(np.float64)
        err = float((np.abs(np.asarray(got[k]) - want) / np.maximum(1.0, np.abs(want))).max())
        record_margin("ensemble_violations_ref_vs_reference_rel", err, FIXTURE_BOUND)
        assert err <= FIXTURE_BOUND, (k, err)
    if tag == "stretched":
        assert got["bond_mask"].tolist() == [False] * 4 + [True] * 2 + [False] * 6 and got["c_n_loss_mean"] > 0.02
    if tag == "o_n":
        assert got["clash_atom_mask"][3, 3] and got["clash_atom_mask"][30, 0]
    if tag == "hairpin":
        assert got["n_clash_pairs"] > 20 and got["violations_between_residue_clash"] > 0.9
    if tag.startswith("ideal"):
        assert not got["bond_mask"].any() and max(got[k] for k in ref.LOSSES[:3]) == 0.0


def _two_residues(shift=0.0):
    """An ideal dipeptide, its second residue moved by ``shift`` A along C_0 -> N_1 (the two angles at the bond do not change)."""
    x = cases.build_backbone(np.array([-60.0, -60.0]), np.array([-45.0, -45.0]))
    step = x[1, 0] - x[0, 2]
    x[1] += shift * step / np.linalg.norm(step)
    return x


ALA2 = (np.ones((2, 5), dtype=bool), np.zeros(2, dtype=np.int64))


def test_c_n_bond_at_the_edge_of_its_tolerance():
    width = 12.0 * 0.014
    for side, violated in ((-1e-3, False), (1e-3, True)):
        x = _two_residues(width + side)
        got = ref.violations(x, *ALA2, np.array([4, 5]))
        e = np.sqrt(1e-6 + (np.sqrt(1e-6 + ((x[1, 0] - x[0, 2]) ** 2).sum()) - 1.329) ** 2)
        assert abs(e - (width + side)) < 1e-5
        assert got["bond_mask"].tolist() == [violated, violated]          # a violated connection marks both of its residues
        assert got["violations_between_residue_bond"] == (2.0 if violated else 0.0) / (1e-4 + 2)
        assert abs(got["c_n_loss_mean"] - max(e - width, 0.0) / (1.0 + 1e-6)) < 1e-15
        assert got["ca_c_n_loss_mean"] == 0.0 and got["c_n_ca_loss_mean"] == 0.0
        assert np.abs(got["per_residue_loss_sum"] - 0.5 * max(e - width, 0.0)).max() < 1e-15
        assert abs(ref.margin(x, *ALA2, np.array([4, 5])) - 1e-3) < 1e-5
    # next residue PRO: 1.341 +- 12 x 0.016
    pro = np.array([0, ref.PRO])
    assert not ref.violations(_two_residues(0.012 + 12 * 0.016 - 1e-3), ALA2[0], pro, np.array([4, 5]))["bond_mask"].any()
    assert ref.violations(_two_residues(0.012 + 12 * 0.016 + 1e-3), ALA2[0], pro, np.array([4, 5]))["bond_mask"].all()
    # the CA-C-N cosine is held to the bond length's width 0.014, as the reference has it: an angle 13 degrees off violates (|d cos| >= 0.19 >
    # 0.168), which the cosine's own 0.0311 (12 sigma = 0.37) would let pass
    x = cases.build_backbone(np.array([-60.0, -60.0]), np.array([-45.0, -45.0]))
    c, axis = x[0, 2], np.cross(x[0, 1] - x[0, 2], x[1, 0] - x[0, 2])
    axis /= np.linalg.norm(axis)
    t = np.deg2rad(13.0)
    rot = lambda v: v * np.cos(t) + np.cross(axis, v) * np.sin(t) + axis * (axis @ v) * (1 - np.cos(t))   # noqa: E731
    x[1] = np.array([c + rot(p - c) for p in x[1]])
    got = ref.violations(x, *ALA2, np.array([0, 1]))
    assert got["ca_c_n_loss_mean"] > 0.0 and got["c_n_loss_mean"] == 0.0 and got["c_n_ca_loss_mean"] == 0.0 and got["bond_mask"].all()


def _one_pair(d, ri=(0, 7), slots=(3, 0)):
    """Two residues of which only one atom each exists (default: the O of the first, the N of the second), ``d`` A apart."""
    x = np.zeros((2, 5, 3))
    x[1, slots[1], 0] = d
    exists = np.zeros((2, 5), dtype=bool)
    exists[0, slots[0]] = exists[1, slots[1]] = True
    return x, exists, np.zeros(2, dtype=np.int64), np.array(ri)


def test_atom_pair_at_the_edge_of_its_bound():
    bound = 1.52 + 1.55 - 1.5
    far = ref.violations(*_one_pair(bound + 1e-3))
    assert far["n_clash_pairs"] == 0 and not far["clash_atom_mask"].any() and far["clashes_mean_loss"] == 0.0 and far["n_terms"]["clashes_mean_loss"] == 1
    near = ref.violations(*_one_pair(bound - 1e-3))
    assert near["n_clash_pairs"] == 1 and near["clash_atom_mask"].sum() == 2 and near["clash_atom_mask"][0, 3] and near["clash_atom_mask"][1, 0]
    assert abs(near["clashes_mean_loss"] - 1e-3 / (1.0 + 1e-6)) < 1e-9
    assert near["violations_between_residue_clash"] == near["violations_per_residue"] == 2.0 / (1e-4 + 2) and not near["bond_mask"].any()
    assert abs(ref.margin(*_one_pair(bound + 1e-4)) - 1e-4) < 1e-8 and abs(ref.margin(*_one_pair(bound - 1e-4)) - 1e-4) < 1e-8
    # another clash tolerance moves the bound
    assert ref.violations(*_one_pair(bound + 0.2), clash_tolerance=1.2)["n_clash_pairs"] == 1
    # two residues with one number are no pair at all
    assert ref.violations(*_one_pair(0.5, ri=(3, 3)))["n_terms"]["clashes_mean_loss"] == 0


def test_peptide_bond_is_no_clash_and_a_gap_silences_only_the_connection():
    c_n = dict(slots=(2, 0))
    bonded = ref.violations(*_one_pair(1.33, ri=(4, 5), **c_n))
    assert bonded["n_clash_pairs"] == 0 and bonded["n_terms"]["clashes_mean_loss"] == 0 and bonded["clashes_mean_loss"] == 0.0
    assert ref.violations(*_one_pair(1.33, ri=(4, 6), **c_n))["n_clash_pairs"] == 1          # not consecutive: an ordinary pair
    assert ref.violations(*_one_pair(1.33, ri=(4, 5), slots=(0, 2)))["n_clash_pairs"] == 1   # N_i - C_i+1 is no bond
    assert ref.violations(*_one_pair(1.33, ri=(5, 4), slots=(0, 2)))["n_clash_pairs"] == 0   # the numbers decide, not the positions
    # a dipeptide torn 1 A apart: violated when numbered 4, 5; with a gap in the numbers no connection term counts, but its C and N, still
    # 2.3 A apart, are then an ordinary pair, and pushed together they clash
    x = _two_residues(1.0)
    assert ref.violations(x, *ALA2, np.array([4, 5]))["bond_mask"].all()
    gap = ref.violations(x, *ALA2, np.array([4, 8]))
    assert not gap["bond_mask"].any() and gap["c_n_loss_mean"] == 0.0 and gap["n_terms"]["c_n_loss_mean"] == 0
    assert gap["violations_extreme_ca_ca_distance"] == 0.0 and gap["per_residue_loss_sum"].min() > 0.0          # (the per-residue loss is not masked)
    assert ref.violations(_two_residues(0.0), *ALA2, np.array([4, 8]))["clash_atom_mask"][[0, 1], [2, 0]].all()
    assert ref.violations(_two_residues(0.0), *ALA2, np.array([4, 5]))["n_clash_pairs"] == 0
    # CA atoms 3.802 + 1.5 + 0.2 A apart
    far = _two_residues(1.7 / 0.9)
    step = np.sqrt(1e-6 + ((far[0, 1] - far[1, 1]) ** 2).sum()) - ref.CA_CA
    assert (ref.violations(far, *ALA2, np.array([4, 5]))["violations_extreme_ca_ca_distance"] > 0.99) == (step > 1.5)


def test_absent_cb_of_gly_never_clashes():
    atoms, exists, aatype, ri = cases.ensemble(13, 17)
    k = int(np.nonzero(aatype == ref.GLY)[0][0])
    assert not exists[k, 4] and (atoms[0, k, 4] == atoms[0, k + 1, 0]).all()          # the decoy sits on the next N
    got = ref.violations(atoms[0], exists, aatype, ri)
    assert not got["clash_atom_mask"][k, 4]
    assert ref.violations(atoms[0], np.ones_like(exists), aatype, ri)["clash_atom_mask"][k, 4]   # counted, it would


def test_single_residue():
    got = ref.violations(np.ones((1, 5, 3)), np.ones((1, 5), dtype=bool), np.array([3]), np.array([9]))
    assert all(got[k] == 0.0 for k in ref.LOSSES + ref.FRACTIONS) and got["n_clash_pairs"] == 0 and not got["bond_mask"].any()
    assert got["per_residue_loss_sum"].tolist() == [0.0] and not got["clash_atom_mask"].any()
    assert ref.margin(np.ones((1, 5, 3)), np.ones((1, 5), dtype=bool), np.array([3]), np.array([9])) == np.inf


# --------------------------------------------------------------------------------------------------------- the device cases' margin
@pytest.mark.parametrize("L,R", cases.SHAPES)
def test_every_device_case_is_a_parity_input(L, R):
    """The device forms every term as the yardstick does (float64, one rounding per operation): a case whose nearest comparison is >= 1e-10
    from flipping has identical masks and counts on both sides.  A condition on the cases; none is left out.  Where the ensemble has room
    (three members, a residue pair) it holds a member of which no pair passes the kernel's prefilter and one of which every pair does."""
    atoms, exists, aatype, ri = cases.ensemble(L, R)
    m = ref.margin(atoms, exists, aatype, ri)
    print(f"L={L} R={R}: margin {m:.3e}")
    assert atoms.shape == (R, L, 5, 3) and atoms.dtype == np.float32 and m >= ref.MARGIN
    if L >= 2:
        assert (aatype == ref.GLY).any() and (aatype == ref.PRO).any()
    if L >= 3:
        assert (np.diff(ri) != 1).sum() == 1
    if L >= 2 and R >= 3:
        passed = [ref.prefilter_survivors(x, exists, ri) for x in atoms]
        assert passed[cases.EXTENDED][0] == 0 and passed[cases.COMPACT][0] == passed[cases.COMPACT][1] == L * (L - 1) // 2
        assert 0 < passed[0][0] < passed[0][1] or L < 4


def test_fixture_cases_are_parity_inputs():
    for tag, case in cases.fixture_cases().items():
        assert ref.margin(*case) >= 1e-4, tag


# ------------------------------------------------------------------------------------------------------------ header and binding
def test_header_declares_and_ops_exports_the_entry_point():
    from str2str_amd import ops
    from str2str_amd.ops import binding

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "str2str_hip.h")).read(), flags=re.S)
    protos = dict(re.findall(r"^int\s+(s2s_\w+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M))
    name = "s2s_backbone_violations"
    assert name in protos and name in ops.EXPORTS
    args = [" ".join(a.split()) for a in protos[name].split(",")]
    assert args[-1] == "void* stream" and "double tolerance_factor" in args and "double clash_tolerance" in args and "int n_res" in args
    assert len(args) == len(binding._SIGNATURES[name]) == 15
    assert int(re.search(r"#define\s+S2S_VIOL_MAX_RES\s+(\d+)", hdr).group(1)) == ops.VIOL_MAX_RES >= 1024
    assert ops.ABI_VERSION >= 38 and callable(ops.backbone_violations)
    assert "ensemble_violations.hip" in __import__("str2str_amd.build", fromlist=["UNITS"]).UNITS


def test_bad_sizes_are_invalid_value():
    """Sizes the kernel cannot take are rejected before any launch (hipErrorInvalidValue = 1), so this needs no device."""
    from str2str_amd import build, ops

    if not os.path.exists(ops.LIB_PATH):
        build.build(verbose=False)
    lib = ops.load_library()
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda n, L, tol=12.0, clash=1.5, ptrs=(p,) * 10: lib.s2s_backbone_violations(   # noqa: E731
        ptrs[0], n, L, ptrs[1], ptrs[2], ptrs[3], tol, clash, *ptrs[4:], None)
    for n, L in ((4, ops.VIOL_MAX_RES + 1), (4, 0), (4, -3), (0, 8), (-1, 8)):
        assert call(n, L) == 1, (n, L)
    assert call(4, 8, tol=float("nan")) == 1 and call(4, 8, clash=float("inf")) == 1
    for k in range(10):
        assert call(4, 8, ptrs=(p,) * k + (None,) + (p,) * (9 - k)) == 1, k


def test_argument_checks_fire_before_the_device(monkeypatch):
    from str2str_amd import ops
    from str2str_amd.metrics import metrics
    from str2str_amd.ops import ensemble

    def touched(*a, **k):
        raise AssertionError("touched the device")

    monkeypatch.setattr(ensemble, "load_library", touched)
    x = torch.zeros(4, 8, 5, 3)
    ok = dict(atom_exists=np.ones((8, 5), dtype=bool), aatype=np.zeros(8, dtype=int), residue_index=np.arange(8))
    bad = [(dict(atoms=torch.zeros(4, 8, 3)), "atoms"), (dict(atoms=torch.zeros(4, 8, 14, 3)), "atoms"), (dict(atoms=torch.zeros(0, 8, 5, 3)), "atoms"),
           (dict(atoms=x.numpy()), "tensor"), (dict(atoms=torch.zeros(1, ops.VIOL_MAX_RES + 1, 5, 3)), "residues"),
           (dict(atoms=x, tolerance_factor=float("nan")), "finite"), (dict(atoms=x, clash_tolerance=float("inf")), "finite"),
           (dict(atoms=x, max_structures=0), "max_structures"), (dict(atoms=x), "no CPU fallback")]
    for kwargs, match in bad:
        with pytest.raises(ops.HipLibraryError, match=match):
            ops.backbone_violations(**{**ok, **kwargs})
    monkeypatch.setattr(metrics, "_backbone_dev", lambda a: torch.as_tensor(np.asarray(a)).float())
    with pytest.raises(ValueError, match="aatype"):
        metrics.backbone_violations(np.zeros((2, 8, 5, 3)), aatype=np.zeros(7, dtype=int))
    with pytest.raises(ops.HipLibraryError, match="residue_index"):
        metrics.backbone_violations(np.zeros((2, 8, 5, 3)), residue_index=np.arange(8) * 2.5)
    monkeypatch.undo()
    for shape in ((4, 8, 3), (4, 8, 14, 3), (8, 5)):
        with pytest.raises(ValueError, match="backbone atoms"):
            metrics.backbone_violations(np.zeros(shape))


# ------------------------------------------------------------------------------------------------------------------- the reader
def test_extract_backbone_atoms(tmp_path):
    from str2str_amd.common import residue_constants as rc
    from str2str_amd.common.pdb_utils import extract_backbone_atoms, extract_backbone_coords

    files = sorted(glob.glob(os.path.join(GOLDEN, "pdb", "*.pdb")))
    assert len(files) == 12
    seen_gly = 0
    for f in files:
        atoms, aatype, ri = extract_backbone_atoms(f)
        ca = extract_backbone_coords(f)
        L = ca.shape[1]
        assert atoms.shape == (1, L, 5, 3) and atoms.dtype == np.float32 and aatype.shape == ri.shape == (L,) and aatype.dtype == ri.dtype == np.int64
        assert (atoms[:, :, 1] == ca).all()
        names = [ln[17:20] for ln in open(f) if ln.startswith("ATOM") and ln[12:16] == " CA "]
        assert [rc.restype_1to3[rc.restypes[a]] for a in aatype] == names
        gly = aatype == ref.GLY
        seen_gly += int(gly.sum())
        assert (atoms[0, gly, 4] == 0.0).all() and (np.abs(atoms[0, ~gly]).sum(-1) > 0).all()
        got = ref.violations(atoms[0], ref.exists_from_aatype(aatype), aatype, ri)
        assert got["n_terms"]["c_n_loss_mean"] == L - 1 - int((np.diff(ri) != 1).sum()) and got["violations_extreme_ca_ca_distance"] == 0.0
    assert seen_gly > 10
    two = tmp_path / "two.pdb"
    two.write_text(open(os.path.join(GOLDEN, "io_atom37_two_models.pdb.txt")).read())
    atoms, aatype, ri = extract_backbone_atoms(str(two))
    assert atoms.shape[0] == 2 and atoms.shape[2:] == (5, 3) and (atoms[:, :, 1] == extract_backbone_coords(str(two))).all()
    assert ri[0] == 3 and aatype[0] == 0 and aatype[1] == ref.GLY and (atoms[:, 1, 4] == 0.0).all()
    first = np.array([[1.257, -1.321, 6.404], [1.049, -5.357, 3.616], [13.040, 9.471, -7.037], [-23.250, -2.188, -12.459], [-12.654, -6.233, 0.413]])
    assert (atoms[0, 0] == first.astype(np.float32)).all()                             # N, CA, C, O, CB: the file has CB before O
    assert extract_backbone_atoms(str(two), max_n_model=1)[0].shape[0] == 1
    # a missing atom names its residue
    lines = open(files[0]).read().splitlines(keepends=True)
    for atom in (" CB ", " N  ", " O  "):
        k = next(i for i, ln in enumerate(lines) if ln.startswith("ATOM") and ln[12:16] == atom and ln[17:20] != "GLY")
        broken = tmp_path / f"no{atom.strip()}.pdb"
        broken.write_text("".join(lines[:k] + lines[k + 1:]))
        with pytest.raises(ValueError, match=rf"{lines[k][17:20]} {lines[k][21]}{lines[k][22:26].strip()} has no {atom.strip()}"):
            extract_backbone_atoms(str(broken))
    other = tmp_path / "coords.npy"
    other.write_text("")
    with pytest.raises(ValueError, match="Unrecognized"):
        extract_backbone_atoms(str(other))


# ---------------------------------------------------------------------------------------------------------------------- eval.py
def test_metric_columns_accept_the_backbone_names():
    entry = load_eval_entry("s2s_eval_entry_violations_cpu")
    five = ["val_clash", "val_bond", "js_pwd", "js_rg", "js_tica"]
    names = ["val_bb_bond", "val_bb_clash", "viol_per_residue"]
    assert entry.metric_columns(None) == five and entry.metric_columns([]) == five
    assert entry.metric_columns(names) == five + names and entry.metric_columns(["div_lddt", "val_bb_clash"]) == five + ["div_lddt", "val_bb_clash"]
    assert entry.metric_columns("viol_per_residue") == five + ["viol_per_residue"]
    assert set(names) <= set(entry.EXTRA_METRICS) and tuple(names) == entry.BACKBONE_METRICS and len(set(entry.EXTRA_METRICS)) == 12
    for bad in (["val_bb_bond", "val_bb_bond"], ["val_bb"], "violations"):
        with pytest.raises(ValueError):
            entry.metric_columns(bad)
