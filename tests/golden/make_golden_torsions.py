"""Golden values for the dihedral of the secondary-structure yardstick (authoring container only).

    python tests/golden/make_golden_torsions.py   ->  tests/golden/torsions.npz

The REFERENCE's own ``atom37_to_torsion_angles`` (src/common/data_transforms.py:925-1090) is imported from the reference checkout and called
in float64 on the backbones of tests/ss_cases.py ``torsion_fixture_cases`` as atom37 arrays in which N, CA, C, O and CB exist; its entries
0 - 2 (pre-omega, phi, psi as (sin, cos)) and their masks are kept.  Its psi is the torsion N-CA-C-O with both components negated, and its
masks know nothing of numbering gaps; tests/test_ensemble_ss_cpu.py holds the yardstick's ``dihedral`` to all three quadruples as the
reference forms them.  The fixture holds the inputs and the outputs only, and ``source`` names the function that produced them.  If the
module cannot be imported, the reference's ``geo_utils.dihedral`` on the same quadruples is the fallback, and ``source`` says so."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import  # noqa: E402
import ss_cases  # noqa: E402

_ref_import.install()
ATOM37_BACKBONE = (0, 1, 2, 4, 3)   # atom37 slots of N, CA, C, O, CB


def quadruples(pos):
    """atom37 positions [L, 37, 3] -> [L, 3, 4, 3]: the atoms of pre-omega, phi, psi as the reference gathers them (zeros before residue 0)."""
    prev = torch.cat([torch.zeros_like(pos[:1]), pos[:-1]])
    return torch.stack([torch.cat([prev[:, 1:3], pos[:, :2]], dim=1), torch.cat([prev[:, 2:3], pos[:, :3]], dim=1),
                        torch.cat([pos[:, :3], pos[:, 4:5]], dim=1)], dim=1)


def main():
    out = {}
    try:
        from src.common.data_transforms import atom37_to_torsion_angles
        source = "atom37_to_torsion_angles"
    except ImportError as e:
        print(f"data_transforms does not import ({e}); using geo_utils.dihedral")
        from src.common.geo_utils import dihedral
        source = "geo_utils.dihedral"
    for tag, (atoms, aatype, ri) in ss_cases.torsion_fixture_cases().items():
        L = len(aatype)
        pos = torch.zeros(L, 37, 3, dtype=torch.float64)
        pos[:, list(ATOM37_BACKBONE)] = torch.as_tensor(np.array(atoms), dtype=torch.float64)
        mask = torch.zeros(L, 37, dtype=torch.float64)
        mask[:, list(ATOM37_BACKBONE)] = 1.0
        if source == "atom37_to_torsion_angles":
            protein = {"aatype": torch.as_tensor(np.array(aatype)), "all_atom_positions": pos, "all_atom_mask": mask}
            res = atom37_to_torsion_angles()(protein)
            sin_cos, m = res["torsion_angles_sin_cos"][:, :3], res["torsion_angles_mask"][:, :3]
        else:
            ang = dihedral(quadruples(pos))
            sin_cos = torch.stack([torch.sin(ang), torch.cos(ang)], dim=-1) * torch.tensor([1.0, 1.0, -1.0])[None, :, None]
            m = torch.ones(L, 3)
            m[0, :2] = 0.0
        assert sin_cos.dtype == torch.float64 and sin_cos.shape == (L, 3, 2)
        out[f"{tag}_atoms"], out[f"{tag}_aatype"], out[f"{tag}_residue_index"] = np.asarray(atoms), np.asarray(aatype), np.asarray(ri)
        out[f"{tag}_sin_cos"], out[f"{tag}_mask"] = sin_cos.numpy(), m.numpy() > 0
    out["source"] = np.array(source)
    path = os.path.join(HERE, "torsions.npz")
    np.savez_compressed(path, **out)
    print(f"torsions.npz: {os.path.getsize(path) / 1024:.1f} KiB, from {source}")


if __name__ == "__main__":
    main()
