"""Secondary structure and backbone torsions on the device (csrc/ensemble_ss.hip) against the float64 numpy statement of their definition in
tests/ref_ss.py.

Every case here is a parity input: tests/test_ensemble_ss_cpu.py asserts that its nearest comparison (an energy against -0.5 kcal/mol, a
CA-CA distance against 9 A, an atom distance against 0.5 A, a bend cosine against cos 70) is at least 1e-9 from flipping and that no bond
angle entering a torsion has a sine below 0.1.  The kernel forms every term as the yardstick does, in float64 with one rounding per
operation, so letters, bond counts and partners are compared with ``==``.

A-priori bounds of the two float64 outputs (u = 2^-52):
  * energy.  A distance is 3 differences, 3 products, 2 sums and a square root, its reciprocal one division more: 10 roundings; four of
    them, three sums and the product with 27.888 make 44.  The terms of the sum are 27.888 / r each, so
        |dE| <= 44 u 27.888 (1 / r_ON + 1 / r_CH + 1 / r_OH + 1 / r_CN)          (exact where the 0.5 A rule sets E = -9.9).
  * angle.  atan2(y, x) with x = (b1 x b2) . (b2 x b3), y = |b2| b1 . (b2 x b3): a cross product is 3 roundings per component on terms of
    size |b||b'| while its length is |b||b'| sin(bond angle), so each normal carries a relative error of 3 u / sin; the dot products, the
    differences before them and the length add 13 more roundings on terms no larger than |n1||n2| / sin^2, and (x, y) has the length
    |b2| |n1||n2|.  The angle moves by the relative error of (x, y), and either atan2 adds at most 4 u of its result, |angle| <= pi:
        |d angle| <= u (32 / sin^2 + 8 pi),  sin = the smallest bond-angle sine of the case (asserted >= 0.1).
Achieved values are recorded through ``record_margin`` in units of their bound.
"""
import functools
import glob
import os

import numpy as np
import pytest
import torch

import ref_ss as ref
import ss_cases as cases
from conftest import record_margin
from ensemble_cases import load_eval_entry, to_device as _dev

pytestmark = pytest.mark.gpu

DEV = "cuda"
ULP = 2.0 ** -52
ENERGY_OPS = 44


@functools.lru_cache(maxsize=None)
def reference(tag):
    """(atoms, aatype, residue_index, the yardstick's outputs, the energy bound [R, L], the angle bound) of one case, computed once."""
    atoms, aatype, ri = cases.protein(tag) if tag in cases.PROTEINS else cases.ensemble(*tag)
    want = ref.ensemble(atoms, aatype, ri)
    e_bound = np.zeros(want["hb_energy"].shape)
    for k, x in enumerate(atoms):
        _, _, _, r = ref._energies(x.astype(np.float64), aatype, ri)
        j = np.nonzero(want["hb_partner"][k] >= 0)[0]
        i = want["hb_partner"][k][j]
        with np.errstate(divide="ignore"):
            e_bound[k, j] = np.where(want["hb_energy"][k, j] == ref.E_MIN, 0.0, ENERGY_OPS * ULP * ref.Q * (1.0 / r[:, i, j]).sum(0))
    s = ref.min_bond_sine(atoms, ri)
    a_bound = ULP * (32.0 / s ** 2 + 8.0 * np.pi) if np.isfinite(s) else 0.0
    for v in list(want.values()) + [e_bound]:
        v.setflags(write=False)
    return atoms, aatype, ri, want, e_bound, a_bound


def _held(tag, result, angles, mask):
    atoms, aatype, ri, want, e_bound, a_bound = reference(tag)
    R, L = atoms.shape[:2]
    assert result.ss.dtype == np.dtype("S1") and result.ss.shape == (R, L) and result.n_hbonds.dtype == np.int32
    assert result.hbond_energy.dtype == np.float64 and result.hbond_partner.dtype == np.int32
    if not (result.ss == want["ss"]).all():
        bad = int(np.nonzero((result.ss != want["ss"]).any(1))[0][0])
        raise AssertionError((tag, bad, ref.strings(result.ss[bad]), ref.strings(want["ss"][bad])))
    assert (result.n_hbonds == want["n_hbonds"]).all() and (result.hbond_partner == want["hb_partner"]).all(), tag
    e_err = np.abs(result.hbond_energy - want["hb_energy"])
    a_err = np.abs(angles - want["torsions"])
    with np.errstate(divide="ignore", invalid="ignore"):
        e_rel = float(np.nan_to_num(np.where(e_bound > 0, e_err / e_bound, np.where(e_err > 0, np.inf, 0.0))).max())
    a_rel = float(a_err.max() / a_bound) if a_bound else float(a_err.max())
    print(f"{tag}: energy error {e_err.max():.3e} ({e_rel:.3f} of its bound), angle error {a_err.max():.3e} ({a_rel:.3f} of {a_bound:.3e})")
    record_margin("ensemble_ss_hbond_energy_of_apriori_bound", e_rel, 1.0)
    record_margin("ensemble_ss_torsion_of_apriori_bound", a_rel, 1.0)
    assert (e_err <= e_bound).all(), (tag, float(e_err.max()))
    assert (a_err <= a_bound).all(), (tag, float(a_err.max()))
    assert angles.shape == (R, L, 3) and angles.dtype == np.float64 and (mask == want["torsion_mask"]).all() and (angles[:, ~mask] == 0.0).all()
    assert (angles > -np.pi).all() and (angles <= np.pi).all()
    assert ((result.hbond_partner == -1) == (result.hbond_energy == 0.0)).all()


@pytest.mark.parametrize("L,R", cases.SHAPES)
def test_secondary_structure_against_float64_reference(L, R):
    from str2str_amd.metrics import metrics

    atoms, aatype, ri, want, _, _ = reference((L, R))
    assert ref.margin(atoms, aatype, ri) >= ref.MARGIN
    got = metrics.secondary_structure(atoms, aatype, ri)
    angles, mask = metrics.backbone_torsions(atoms, ri)
    _held((L, R), got, angles, mask)
    assert metrics.ss_strings(got) == ref.strings(want["ss"])
    if L <= 4:
        assert (got.n_hbonds == 0).all() and set(b"".join(got.ss.reshape(-1))) == set(b"-") and (got.hbond_partner[:, 0] == -1).all()
    if (L, R) == (5, 3):
        assert metrics.ss_strings(got)[0] == "-TTT-"
    if (L, R) == (6, 2):
        assert metrics.ss_strings(got)[0] == "-HHHH-"


@pytest.mark.parametrize("name", cases.PROTEINS)
def test_fixture_proteins_and_perturbed_copies(name):
    from str2str_amd.metrics import metrics

    atoms, aatype, ri, want, _, _ = reference(name)
    assert ref.margin(atoms, aatype, ri) >= ref.MARGIN and len(atoms) == 1 + cases.N_COPIES
    got = metrics.secondary_structure(atoms, aatype, ri)
    _held(name, got, *metrics.backbone_torsions(atoms, ri))
    assert b"E" in got.ss[0] or name == "2JOF"


def test_chunking_and_repeats_are_bit_identical():
    from str2str_amd import ops

    atoms, aatype, ri, _, _, _ = reference((65, 17))
    x = _dev(atoms)
    whole = ops.secondary_structure(x, aatype, ri)
    assert all(t.is_cuda for t in whole)
    assert [t.dtype for t in whole] == [torch.uint8, torch.int32, torch.float64, torch.int32, torch.float64]
    again = ops.secondary_structure(x, aatype, ri)
    assert all(torch.equal(a, b) for a, b in zip(whole, again))
    for max_structures in (1, 2, 17):
        part = ops.secondary_structure(x, aatype, ri, max_structures=max_structures)
        assert all(torch.equal(a, b) for a, b in zip(whole, part)), max_structures
    alone = ops.secondary_structure(x[3:4].contiguous(), aatype, ri)       # a structure's results do not depend on its neighbours
    assert all(torch.equal(a[3:4], b) for a, b in zip(whole, alone))


def test_atom37_input_equals_atom14_input():
    from str2str_amd.metrics import metrics

    atoms, aatype, ri, want, _, _ = reference((13, 17))
    atom37 = np.zeros((17, 13, 37, 3), dtype=np.float32)
    atom37[:, :, list(metrics.ATOM37_BACKBONE)] = atoms        # N, CA, C, CB, O, ...: the sampler's layout
    a, b = metrics.secondary_structure(atoms, aatype, ri), metrics.secondary_structure(_dev(atom37), aatype, ri)
    assert all((u == v).all() for u, v in zip(a, b))
    ta, tb = metrics.backbone_torsions(atoms, ri), metrics.backbone_torsions(_dev(atom37), ri)
    assert (ta[0] == tb[0]).all() and (ta[1] == tb[1]).all()
    _held((13, 17), b, *tb)
    one = metrics.secondary_structure(atoms[4], aatype, ri)     # a single structure without the leading axis
    assert all((u[4:5] == v).all() for u, v in zip(a, one))
    # the defaults: all ALA (every connected residue has an amide hydrogen), numbered 0 .. L - 1 (no break)
    plain = metrics.secondary_structure(atoms)
    ala, numbers = np.zeros(13, dtype=np.int64), np.arange(13)
    assert ref.margin(atoms, ala, numbers) >= ref.MARGIN
    w = ref.ensemble(atoms, ala, numbers)
    assert (plain.ss == w["ss"]).all() and (plain.n_hbonds == w["n_hbonds"]).all() and (plain.hbond_partner == w["hb_partner"]).all()
    assert metrics.backbone_torsions(atoms)[1][1:, 0].all()


def test_what_the_kernel_cannot_take_raises():
    from str2str_amd import ops
    from str2str_amd.metrics import metrics

    L = ops.SS_MAX_RES + 1
    with pytest.raises(ops.HipLibraryError, match="residues"):
        metrics.secondary_structure(np.zeros((1, L, 5, 3), dtype=np.float32))
    with pytest.raises(ops.HipLibraryError, match="residues"):
        ops.secondary_structure(torch.zeros(1, L, 5, 3, device=DEV), np.zeros(L, dtype=int), np.arange(L))
    ok = (np.zeros(8, dtype=int), np.arange(8))
    with pytest.raises(ops.HipLibraryError, match="no CPU fallback"):
        ops.secondary_structure(torch.zeros(2, 8, 5, 3), *ok)
    with pytest.raises(ops.HipLibraryError, match="dtype"):
        ops.secondary_structure(torch.zeros(2, 8, 5, 3, device=DEV, dtype=torch.float64), *ok)
    with pytest.raises(ops.HipLibraryError, match="contiguous"):
        ops.secondary_structure(torch.zeros(2, 8, 3, 5, device=DEV).transpose(2, 3), *ok)
    for shape in ((2, 8, 3), (2, 8, 4, 3), (0, 8, 5, 3)):
        with pytest.raises(ops.HipLibraryError, match="atoms"):
            ops.secondary_structure(torch.zeros(shape, device=DEV), *ok)
    # the longest chain the kernel takes: a helix of S2S_SS_MAX_RES residues, every letter as the yardstick's
    x = cases.regular(-57.0, -47.0, ops.SS_MAX_RES)[None]
    got = metrics.secondary_structure(x)
    assert metrics.ss_strings(got) == ["-" + (ops.SS_MAX_RES - 2) * "H" + "-"] and got.n_hbonds.tolist() == [ops.SS_MAX_RES - 4]


def _tails(both, aatype, ri, n_bins=36):
    """The ensemble metrics as the numpy tail of str2str_amd.metrics applied to the yardstick's output."""
    from str2str_amd.metrics import metrics

    out = {k: ref.ensemble(v, aatype, ri) for k, v in both.items()}
    prop = {k: ref.propensity(o["ss"]) for k, o in out.items()}
    binned = {k: metrics._rama_histogram(o["torsions"], o["torsion_mask"], n_bins) for k, o in out.items()}
    return dict(prop=prop, helix={k: np.around(p[:, 0].mean(), decimals=4) for k, p in prop.items()},
                strand={k: np.around(p[:, 1].mean(), decimals=4) for k, p in prop.items()},
                mae={k: np.around((0.5 * np.abs(p - prop["target"]).sum(1)).mean(), decimals=4) if k != "target" else 0.0 for k, p in prop.items()},
                js={k: np.around(metrics._js(b, binned["target"]), decimals=4) if k != "target" else 0.0 for k, b in binned.items()})


def test_ensemble_metrics_against_the_yardsticks_tail():
    from str2str_amd.metrics import metrics

    t_atoms, aatype, ri, _, _, _ = reference((31, 9))
    p_atoms = t_atoms[::-1][:6].copy()                          # another mix of the same sequence's members
    assert ref.margin(p_atoms, aatype, ri) >= ref.MARGIN
    both = {"target": t_atoms, "pred": p_atoms}
    want = _tails(both, aatype, ri)
    prop = metrics.ss_propensity(both, aatype, ri)
    helix, strand = metrics.ss_content(both, aatype, ri)
    mae = metrics.ss_mae(both, "target", aatype, ri)
    js = metrics.js_rama(both, "target", residue_index=ri)
    for k in both:
        assert prop[k].shape == (31, 3) and prop[k].dtype == np.float64 and (prop[k] == want["prop"][k]).all()
        assert helix[k] == want["helix"][k] and strand[k] == want["strand"][k] and mae[k] == want["mae"][k] and js[k] == want["js"][k]
    assert mae["target"] == 0.0 and js["target"] == 0.0 and 0.0 < mae["pred"] < 1.0 and 0.0 < js["pred"] < 1.0
    assert 0.0 < helix["target"] < 1.0 and strand["target"] > 0.0
    assert metrics.js_rama(both, "target", n_bins=12, residue_index=ri)["pred"] == _tails(both, aatype, ri, 12)["js"]["pred"]


def test_eval_secondary_structure_switch(tmp_path):
    """Three targets written with the project's own writer, the last one's target file cut down to its CA trace.  With the switch the ss
    csv and the per-residue tables hold the yardstick's values for what the reader returns (NaN in the target columns of the CA trace);
    without it the output directory holds what it held before, and the metrics csv is the same either way."""
    from str2str_amd.common.pdb_utils import atom37_to_pdb, extract_backbone_atoms
    from str2str_amd.metrics import metrics

    entry = load_eval_entry("s2s_eval_entry_ss")
    target_dir = tmp_path / "targets"
    target_dir.mkdir()
    ensembles = {}
    for name, shape in (("one", (31, 9)), ("two", (13, 17)), ("trace", (13, 17))):
        atoms, aatype, ri, _, _, _ = reference(shape)
        L, R = shape
        atom37 = np.zeros((R, L, 37, 3), dtype=np.float32)
        atom37[:, :, list(metrics.ATOM37_BACKBONE)] = atoms + 10.0   # (away from the origin: the writer takes an atom at 0, 0, 0 for absent)
        atom37[:, aatype == metrics.GLY, 3] = 0.0               # the writer leaves a GLY's CB out
        ensembles[name] = (atom37, aatype, ri)
        atom37_to_pdb(str(target_dir / f"{name}.pdb"), atom37[:5], aatype=aatype, residue_index=ri)
    trace = target_dir / "trace.pdb"
    trace.write_text("".join(ln for ln in open(trace) if not ln.startswith("ATOM") or ln[12:16] == " CA "))
    listing = {}
    for sub, switch in (("plain", None), ("ss", True)):
        pred_dir = tmp_path / sub / "samples" / "all"
        pred_dir.mkdir(parents=True)
        for name, (atom37, aatype, ri) in ensembles.items():
            atom37_to_pdb(str(pred_dir / f"{name}.pdb"), atom37, aatype=aatype, residue_index=ri)
        entry.evaluate_prediction(str(pred_dir), str(target_dir), tag="t", secondary_structure=switch)
        files = glob.glob(str(tmp_path / sub / "metrics_t_*.csv"))
        assert len(files) == 1
        listing[sub] = (sorted(os.listdir(tmp_path / sub)), open(files[0]).read())
    assert len(listing["plain"][0]) == 2 and [f.split("_")[0] for f in listing["plain"][0]] == ["metrics", "samples"]
    assert [f.split("_")[0] for f in listing["ss"][0]] == ["metrics", "samples", "secondary", "ss"]
    assert listing["ss"][1] == listing["plain"][1]                # the metrics csv does not change
    rows = {r[0]: r[1:] for r in (ln.rstrip("\n").split("\t") for ln in open(glob.glob(str(tmp_path / "ss" / "ss_t_*.csv"))[0]))}
    assert rows[""] == list(entry.SS_COLUMNS) and set(rows) == {"", "one", "two", "trace"}
    assert sorted(os.listdir(tmp_path / "ss" / "secondary_structure")) == ["one.csv", "trace.csv", "two.csv"]
    for name in ensembles:
        atoms, aatype, ri = extract_backbone_atoms(str(tmp_path / "ss" / "samples" / "all" / f"{name}.pdb"))   # at the PDB's three decimals
        both = {"pred": atoms}
        if name != "trace":
            both["target"] = extract_backbone_atoms(str(target_dir / f"{name}.pdb"))[0]
        assert all(ref.margin(v, aatype, ri) >= ref.MARGIN for v in both.values())
        w = _tails({"target": both.get("target", atoms), "pred": atoms}, aatype, ri)
        got = [float(v) if v else float("nan") for v in rows[name]]
        if name == "trace":
            assert got[:2] == [float(w["helix"]["pred"]), float(w["strand"]["pred"])] and np.isnan(got[2:]).all()
        else:
            assert got == [float(v) for v in (w["helix"]["pred"], w["strand"]["pred"], w["helix"]["target"], w["strand"]["target"],
                                              w["mae"]["pred"], w["js"]["pred"])], name
        table = [ln.rstrip("\n").split("\t") for ln in open(tmp_path / "ss" / "secondary_structure" / f"{name}.csv")]
        assert table[0] == ["residue_index"] + [f"{k}_{c}" for k in ("pred", "target") for c in entry.SS_CLASSES] and len(table) == 1 + len(ri)
        body = np.array([[float(v) if v else np.nan for v in row] for row in table[1:]])
        assert (body[:, 0] == ri).all() and (body[:, 1:4] == np.around(w["prop"]["pred"], decimals=4)).all()
        if name == "trace":
            assert np.isnan(body[:, 4:]).all()
        else:
            assert (body[:, 4:] == np.around(w["prop"]["target"], decimals=4)).all()
