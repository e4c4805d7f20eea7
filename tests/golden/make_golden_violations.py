"""Golden values for the backbone-violation yardstick (authoring container only).

    python tests/golden/make_golden_violations.py   ->  tests/golden/violations.npz

The REFERENCE's own ``between_residue_bond_loss``, ``between_residue_clash_loss`` (one structure per call) and
``extreme_ca_ca_distance_violations`` (src/models/loss.py:714-1017, 1237-1271) are imported from the reference checkout and called in float32,
its working precision, on the cases of tests/violations_cases.py ``fixture_cases`` as atom14 arrays whose slots 5 .. 13 do not exist; the
radii are those of ``find_structural_violations`` (:1126-1137) and the per-residue fractions go through the reference's ``masked_mean`` with
a sequence mask of ones, as ``compute_violation_metrics`` (:1274-1314) forms them.  The fixture holds the inputs and the outputs only.
``ml_collections`` (imported by loss.py, not used here) is stubbed as a bare module when it is not installed."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import  # noqa: E402
import violations_cases  # noqa: E402

_ref_import.install()
if importlib.util.find_spec("ml_collections") is None:
    sys.modules["ml_collections"] = types.ModuleType("ml_collections")
    sys.modules["ml_collections"].ConfigDict = dict   # (named in an annotation of loss.py)
from src.common import residue_constants as rc  # noqa: E402
from src.models import loss as RL  # noqa: E402
from src.utils.tensor_utils import masked_mean  # noqa: E402


def main():
    out = {}
    for tag, (atoms, exists, aatype, ri) in violations_cases.fixture_cases().items():
        L = len(aatype)
        pos = torch.zeros(L, 14, 3)
        pos[:, :5] = torch.as_tensor(np.array(atoms))
        mask = torch.zeros(L, 14)
        mask[:, :5] = torch.as_tensor(np.array(exists)).float()
        elements = "NCCOC" + "C" * 9                              # N, CA, C, O, CB; the other slots do not exist
        radius = mask * torch.tensor([rc.van_der_waals_radius[e] for e in elements])
        ri_t, aa_t = torch.as_tensor(np.array(ri)), torch.as_tensor(np.array(aatype))
        bond = RL.between_residue_bond_loss(pos, mask, ri_t, aa_t)                      # tolerance factors 12.0: the function's defaults
        clash = RL.between_residue_clash_loss(pos, mask, radius, ri_t)                  # overlap tolerances 1.5: the function's defaults
        ones = torch.ones(L)
        per_res_clash = torch.max(clash["per_atom_clash_mask"], dim=-1)[0]
        union = torch.maximum(bond["per_residue_violation_mask"], per_res_clash)
        out[f"{tag}_atoms"], out[f"{tag}_aatype"], out[f"{tag}_residue_index"] = np.asarray(atoms), np.asarray(aatype), np.asarray(ri)
        for k in ("c_n_loss_mean", "ca_c_n_loss_mean", "c_n_ca_loss_mean", "per_residue_loss_sum"):
            out[f"{tag}_{k}"] = bond[k].numpy()
        out[f"{tag}_clashes_mean_loss"] = clash["mean_loss"].numpy()
        out[f"{tag}_bond_mask"] = bond["per_residue_violation_mask"].numpy() > 0
        out[f"{tag}_clash_atom_mask"] = clash["per_atom_clash_mask"].numpy()[:, :5] > 0
        assert not clash["per_atom_clash_mask"][:, 5:].any()
        out[f"{tag}_violations_between_residue_bond"] = masked_mean(ones, bond["per_residue_violation_mask"], dim=-1).numpy()
        out[f"{tag}_violations_between_residue_clash"] = masked_mean(ones, per_res_clash, dim=-1).numpy()
        out[f"{tag}_violations_per_residue"] = masked_mean(ones, union, dim=-1).numpy()
        out[f"{tag}_violations_extreme_ca_ca_distance"] = RL.extreme_ca_ca_distance_violations(pos, mask, ri_t).numpy()
        assert out[f"{tag}_c_n_loss_mean"].dtype == np.float32 and out[f"{tag}_per_residue_loss_sum"].shape == (L,)
    path = os.path.join(HERE, "violations.npz")
    np.savez_compressed(path, **out)
    print(f"violations.npz: {os.path.getsize(path) / 1024:.1f} KiB", {k: float(v) for k, v in out.items() if k.endswith("mean_loss")})


if __name__ == "__main__":
    main()
