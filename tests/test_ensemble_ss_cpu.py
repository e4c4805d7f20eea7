"""Secondary structure and backbone torsions without a GPU: the yardstick (tests/ref_ss.py) held to constructed helices, to the known anatomy
of the fixture proteins and, for its dihedral, to the reference through tests/golden/torsions.npz; the margins that make every device
case a parity input; the C-ABI surface, the numpy tails of the ensemble metrics and the evaluation switch."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import torch

import ref_ss as ref
import ss_cases as cases
from conftest import GOLDEN, ROOT, golden, record_margin

ALA = lambda L: (np.zeros(L, dtype=np.int64), np.arange(L))   # noqa: E731

# Measured against the fixture when it was made: 7.8e-6 (extended65), 1.9e-6 (mixed31), 5.7e-7 (helix13).  The reference's frames are
# float32 whatever the input (its Rigid casts rotations and translations, rigid_utils.py:331, 902), so the difference is 2^-24 of the
# largest coordinate -- the extended chain reaches 200 A -- and not the 1e-8 under its square roots.  The bound is 2.6 x the measured value.
TORSION_FIXTURE_BOUND = 2e-5


# ------------------------------------------------------------------------------------------------------------------- constructions
@pytest.mark.parametrize("phi,psi,L,want", cases.CONSTRUCTIONS)
def test_constructed_chains_give_their_strings(phi, psi, L, want):
    got = ref.secondary_structure(cases.regular(phi, psi, L), *ALA(L))
    assert ref.strings(got["ss"]) == [want]
    assert ref.margin(cases.regular(phi, psi, L), *ALA(L)) >= 1e-2


def test_proline_costs_one_bond_and_a_gap_splits_the_helix():
    x = cases.regular(-57.0, -47.0, 20)
    aatype, ri = ALA(20)
    plain = ref.secondary_structure(x, aatype, ri)
    assert plain["n_hbonds"] == 16 and (plain["hb_partner"][4:] == np.arange(16)).all() and (plain["hb_partner"][:4] == -1).sum() >= 1
    assert (plain["hb_energy"][4:] < -1.0).all() and plain["hb_energy"][0] == 0.0 and plain["hb_partner"][0] == -1
    pro = aatype.copy()
    pro[10] = ref.PRO                                           # no amide hydrogen: the bond 6 -> 10 is gone, the helix stands
    got = ref.secondary_structure(x, pro, ri)
    assert got["n_hbonds"] == 15 and ref.strings(got["ss"]) == ["-" + 18 * "H" + "-"]
    assert got["hb_partner"][10] == -1 and got["hb_energy"][10] == 0.0
    gap = ri.copy()
    gap[10:] += 3                                               # residues 9 and 10 are not connected: no turn spans them
    got = ref.secondary_structure(x, aatype, gap)
    assert ref.strings(got["ss"]) == ["-HHHHHHHH--HHHHHHHH-"] and got["n_hbonds"] < 16
    assert not got["hb"][:, 10].any()                           # residue 10 has no hydrogen to give


def test_hydrogen_bond_conditions():
    """j = i and j = i + 1 are no bonds whatever the energy, a residue pair 9 A apart is none, and below 0.5 A the energy is -9.9."""
    x = cases.regular(-57.0, -47.0, 8).astype(np.float64)
    e, surv, d_ca, r = ref._energies(x, *ALA(8))
    assert not surv[np.arange(8), np.arange(8)].any() and not surv[np.arange(7), np.arange(1, 8)].any() and not surv[:, 0].any()
    assert surv[np.arange(1, 8), np.arange(7)].any()            # j = i - 1 is tested
    far = x.copy()
    far[5:] += np.array([30.0, 0.0, 0.0])
    assert not ref._energies(far, *ALA(8))[1][:5, 5:].any()
    near = x.copy()
    near[6, 0] = near[1, 3] + np.array([0.3, 0.0, 0.0])         # N_6 0.3 A from O_1
    got = ref.secondary_structure(near, *ALA(8))
    assert got["hb"][1, 6] and got["hb_energy"][6] == ref.E_MIN and got["hb_partner"][6] == 1


# ---------------------------------------------------------------------------------------------------------------- fixture proteins
PROTEIN_STRINGS = {
    "CLN025": "-EETTTTEE-",
    "2JOF": "-HHHHHHHTTGGGGSS----",
    "NuG2": "-EEEEEEEETTEEEEEEEE-SSHHHHHHHHHHHHHHTT---EEEEETTTTEEEEE-",
    "bpti": "--GGGGS-----SS---EEEEEEETTTTEEEEEEE-SSS--SS-BSSHHHHHHHH---",
}


def _model_one(name):
    from str2str_amd.common.pdb_utils import extract_backbone_atoms

    atoms, aatype, ri = extract_backbone_atoms(cases.protein_path(name), max_n_model=1)
    return atoms[0], aatype, ri


@pytest.mark.parametrize("name", sorted(PROTEIN_STRINGS))
def test_fixture_proteins_give_their_strings(name):
    x, aatype, ri = _model_one(name)
    assert ref.strings(ref.secondary_structure(x, aatype, ri)["ss"]) == [PROTEIN_STRINGS[name]]
    assert ref.margin(x, aatype, ri) >= 1.2e-4


def test_fixture_proteins_have_their_textbook_content():
    files = sorted(glob.glob(os.path.join(GOLDEN, "pdb", "*.pdb")))
    assert len(files) == 12
    for name in ("A3D", "UVF", "PRB", "lambda"):
        p = ref.propensity(ref.secondary_structure(*_model_one(name))["ss"])
        assert p[:, 0].mean() >= 0.6 and b"E" not in ref.secondary_structure(*_model_one(name))["ss"], name
    got = ref.secondary_structure(*_model_one("GTT"))["ss"]
    assert b"H" not in got and ref.propensity(got)[:, 1].mean() >= 0.3
    for f in files:                                            # every fixture protein keeps the margin the device cases ask for
        x, aatype, ri = _model_one(os.path.basename(f)[:-4])
        assert ref.margin(x, aatype, ri) >= 1.2e-4 and ref.min_bond_sine(x, ri) >= 0.1, f


# ------------------------------------------------------------------------------------------------------------------------ torsions
@pytest.mark.parametrize("tag", ("mixed31", "helix13", "extended65"))
def test_dihedral_against_the_reference(tag):
    """tests/golden/torsions.npz: the reference's atom37_to_torsion_angles, entries 0 - 2 as (sin, cos).  Its quadruples are pre-omega
    (CA_i-1, C_i-1, N_i, CA_i), phi (C_i-1, N_i, CA_i, C_i) and psi as (N_i, CA_i, C_i, O_i) with both components negated; the yardstick's
    dihedral on those quadruples pins its sign and range.  (The public psi ends on N_i+1, not on O_i.)"""
    g = golden("torsions.npz")
    assert str(g["source"]) == "atom37_to_torsion_angles"
    atoms, aatype, ri = cases.torsion_fixture_cases()[tag]
    assert (atoms == g[f"{tag}_atoms"]).all() and (aatype == g[f"{tag}_aatype"]).all() and (ri == g[f"{tag}_residue_index"]).all()
    x = atoms.astype(np.float64)
    n, ca, c, o = x[:, 0], x[:, 1], x[:, 2], x[:, 3]
    L = len(x)
    ang = np.zeros((L, 3))
    ang[1:, 0] = ref.dihedral(ca[:-1], c[:-1], n[1:], ca[1:])
    ang[1:, 1] = ref.dihedral(c[:-1], n[1:], ca[1:], c[1:])
    ang[:, 2] = ref.dihedral(n, ca, c, o)
    mine = np.stack([np.sin(ang), np.cos(ang)], axis=-1)
    mine[:, 2] *= -1.0
    mask = g[f"{tag}_mask"]
    assert mask.sum(0).tolist() == [L - 1, L - 1, L]            # the reference's masks ignore the numbering gap
    err = float(np.abs(mine - g[f"{tag}_sin_cos"])[mask].max())
    print(f"{tag}: max |sin, cos| difference {err:.3e}")
    record_margin("ensemble_ss_dihedral_vs_reference", err, TORSION_FIXTURE_BOUND)
    assert err <= TORSION_FIXTURE_BOUND
    assert (ang > -np.pi).all() and (ang <= np.pi).all()


def test_build_backbone_torsions_come_back():
    from violations_cases import build_backbone

    rng = np.random.default_rng(5)
    L = 40
    phi, psi, omega = rng.uniform(-180.0, 180.0, size=(3, L))
    omega = np.where(rng.random(L) < 0.5, omega, 180.0)        # (exactly pi must come back as +pi)
    ri = np.arange(L) + 3
    ri[17:] += 2
    ang, mask = ref.torsions(build_backbone(phi, psi, omega), ri)
    want = np.deg2rad(np.stack([phi, psi, np.append(0.0, omega[:-1])], axis=1))
    diff = np.abs(np.angle(np.exp(1j * (ang - want))))[mask]
    print(f"build_backbone round trip: {diff.max():.3e} rad")
    assert diff.max() < 1e-12
    assert mask[:, 0].tolist() == mask[:, 2].tolist() == [k not in (0, 17) for k in range(L)]
    assert mask[:, 1].tolist() == [k not in (16, L - 1) for k in range(L)] and (ang[~mask] == 0.0).all()
    flat = ref.dihedral(*np.array([[1.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, -1.0, 0.0]]))   # trans: +pi, never -pi
    assert flat == np.pi


# -------------------------------------------------------------------------------------------------------- the device cases' margin
CASES = {tag: rest for tag, *rest in cases.parity_cases()}


@pytest.mark.parametrize("tag", list(CASES))
def test_every_device_case_is_a_parity_input(tag):
    """The device forms every energy, distance and cosine as the yardstick does (float64, one rounding per operation): a case whose nearest
    comparison is >= 1e-9 from flipping has the same bonds, hence the same letters, on both sides.  A condition on the cases; none is
    left out."""
    atoms, aatype, ri = CASES[tag]
    m, s = ref.margin(atoms, aatype, ri), ref.min_bond_sine(atoms, ri)
    print(f"{tag}: margin {m:.3e}, smallest bond-angle sine {s:.3f}")
    assert atoms.ndim == 4 and atoms.shape[2:] == (5, 3) and atoms.dtype == np.float32
    assert m >= ref.MARGIN and s >= 0.1
    L = atoms.shape[1]
    if L >= 8 and tag.startswith("L"):
        assert (aatype == ref.PRO).any() and (np.diff(ri) != 1).sum() == 1


def test_the_cases_cover_every_letter_and_shape():
    seen = set()
    for atoms, aatype, ri in CASES.values():
        seen |= set("".join(ref.strings(ref.ensemble(atoms, aatype, ri)["ss"])))
    assert seen == set(ref.LETTERS)
    assert set(cases.SHAPES) >= {(1, 2), (2, 1), (4, 3), (5, 3), (6, 2), (13, 17), (31, 9), (64, 3), (65, 17), (129, 4), (300, 3)}
    assert ref.strings(ref.ensemble(*cases.ensemble(5, 3))["ss"])[0] == "-TTT-"              # one turn, no helix
    assert ref.strings(ref.ensemble(*cases.ensemble(6, 2))["ss"])[0] == "-HHHH-"             # the minimal helix
    assert ref.ensemble(*cases.ensemble(4, 3))["n_hbonds"].sum() == 0
    dense = ref.ensemble(*cases.ensemble(65, 17))
    assert dense["n_survivors"][cases.COMPACT] > 0.7 * 65 * 64 and (dense["hb_energy"][cases.COMPACT] == ref.E_MIN).any()
    assert all(len(cases.protein(name)[0]) == 1 + cases.N_COPIES for name in cases.PROTEINS)


# ------------------------------------------------------------------------------------------------------------ header and binding
def test_abi_and_interface_are_declared():
    from str2str_amd import ops
    from str2str_amd.metrics import metrics
    from str2str_amd.ops import binding

    text = open(os.path.join(ROOT, "include", "str2str_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = dict(re.findall(r"^int\s+(s2s_\w+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M))
    name = "s2s_secondary_structure"
    assert name in protos and name in ops.EXPORTS
    args = [" ".join(a.split()) for a in protos[name].split(",")]
    assert args[-1] == "void* stream" and "int n_res" in args and "unsigned char* ss" in args and "double* torsions" in args
    assert len(args) == len(binding._SIGNATURES[name]) == 11
    assert int(re.search(r"#define\s+S2S_SS_MAX_RES\s+(\d+)", hdr).group(1)) == ops.SS_MAX_RES >= 512
    assert ops.ABI_VERSION >= 39 and callable(ops.secondary_structure)
    assert int(re.search(r"return (\d+);", open(os.path.join(ROOT, "str2str_amd", "csrc", "abi.hip")).read()).group(1)) == ops.ABI_VERSION
    assert "ensemble_ss.hip" in __import__("str2str_amd.build", fromlist=["UNITS"]).UNITS
    assert "-ffp-contract=off" in __import__("str2str_amd.build", fromlist=["UNITS"]).UNITS["ensemble_ss.hip"]
    assert "bulge" in text and "two" in text.split("S2S_SS_MAX_RES")[0].split("Secondary structure")[1]      # the departures are stated
    assert metrics.SecondaryStructure._fields == ("ss", "n_hbonds", "hbond_energy", "hbond_partner")
    for fn in ("secondary_structure", "ss_strings", "backbone_torsions", "ss_propensity", "ss_content", "ss_mae", "js_rama"):
        assert callable(getattr(metrics, fn)), fn


def test_bad_sizes_are_invalid_value():
    """Sizes the kernel cannot take are rejected before any launch (hipErrorInvalidValue = 1), so this needs no device."""
    from str2str_amd import build, ops

    if not os.path.exists(ops.LIB_PATH):
        build.build(verbose=False)
    lib = ops.load_library()
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda n, L, ptrs=(p,) * 8: lib.s2s_secondary_structure(ptrs[0], n, L, *ptrs[1:], None)   # noqa: E731
    for n, L in ((4, ops.SS_MAX_RES + 1), (4, 0), (4, -3), (0, 8), (-1, 8)):
        assert call(n, L) == 1, (n, L)
    for k in range(8):
        assert call(4, 8, ptrs=(p,) * k + (None,) + (p,) * (7 - k)) == 1, k


def test_argument_checks_fire_before_the_device(monkeypatch):
    from str2str_amd import ops
    from str2str_amd.metrics import metrics
    from str2str_amd.ops import ensemble

    def touched(*a, **k):
        raise AssertionError("touched the device")

    monkeypatch.setattr(ensemble, "load_library", touched)
    x = torch.zeros(4, 8, 5, 3)
    ok = dict(aatype=np.zeros(8, dtype=int), residue_index=np.arange(8))
    bad = [(dict(atoms=torch.zeros(4, 8, 3)), "atoms"), (dict(atoms=torch.zeros(4, 8, 14, 3)), "atoms"), (dict(atoms=torch.zeros(0, 8, 5, 3)), "atoms"),
           (dict(atoms=x.numpy()), "tensor"), (dict(atoms=torch.zeros(1, ops.SS_MAX_RES + 1, 5, 3)), "residues"),
           (dict(atoms=x, max_structures=0), "max_structures"), (dict(atoms=x, max_structures=1.5), "max_structures"),
           (dict(atoms=x, aatype=np.zeros(7, dtype=int)), "aatype"), (dict(atoms=x, residue_index=np.arange(8) * 0.5), "residue_index"),
           (dict(atoms=x, residue_index=np.arange(8) + 2 ** 31), "32 bits"), (dict(atoms=x), "no CPU fallback")]
    for kwargs, match in bad:
        with pytest.raises(ops.HipLibraryError, match=match):
            ops.secondary_structure(**{**ok, **kwargs})
    monkeypatch.setattr(metrics, "_backbone_dev", lambda a: torch.as_tensor(np.asarray(a)).float())
    with pytest.raises(ValueError, match="aatype"):
        metrics.secondary_structure(np.zeros((2, 8, 5, 3)), aatype=np.zeros(7, dtype=int))
    with pytest.raises(ValueError, match="residue_index"):
        metrics.backbone_torsions(np.zeros((2, 8, 5, 3)), residue_index=np.arange(9))
    monkeypatch.undo()
    for shape in ((4, 8, 3), (4, 8, 14, 3), (8, 5)):
        with pytest.raises(ValueError, match="backbone atoms"):
            metrics.secondary_structure(np.zeros(shape))
        with pytest.raises(ValueError, match="backbone atoms"):
            metrics.backbone_torsions(np.zeros(shape))


# ------------------------------------------------------------------------------------------------------- the numpy tails of the metrics
def test_propensity_strings_and_ramachandran_tails():
    from str2str_amd.metrics import metrics

    ss = np.array([list("-HHGE"), list("BHTIS")], dtype="S1")
    assert metrics.ss_strings(ss) == ["-HHGE", "BHTIS"] and metrics.ss_strings(ss[0]) == ["-HHGE"]
    res = metrics.SecondaryStructure(ss, np.zeros(2, np.int32), np.zeros((2, 5)), np.zeros((2, 5), np.int32))
    assert metrics.ss_strings(res) == ["-HHGE", "BHTIS"]
    p = metrics._propensity(ss)
    assert p.tolist() == [[0.0, 0.5, 0.5], [1.0, 0.0, 0.0], [0.5, 0.0, 0.5], [1.0, 0.0, 0.0], [0.0, 0.5, 0.5]]
    assert (p == ref.propensity(ss)).all() and (p.sum(1) == 1.0).all()
    angles = np.zeros((2, 4, 3))
    angles[0, :, 0], angles[0, :, 1] = [-np.pi, 0.0, np.pi, 1.0], [0.0, np.pi, -np.pi, 1.0]
    mask = np.array([[True, True, True], [True, True, True], [True, True, True], [True, False, True]])
    h = metrics._rama_histogram(angles, mask, 4).reshape(4, 4)
    assert h.sum() == pytest.approx(6.0 + 16 * metrics.PSEUDO_C)
    counts = np.rint(h - metrics.PSEUDO_C).astype(int)
    # structure 0: (-pi, 0) -> bin (0, 2); (0, pi) -> (2, 0): pi wraps to -pi; (pi, -pi) -> (0, 0); structure 1: three times (0, 0) -> (2, 2)
    assert counts[0, 2] == 1 and counts[2, 0] == 1 and counts[0, 0] == 1 and counts[2, 2] == 3
