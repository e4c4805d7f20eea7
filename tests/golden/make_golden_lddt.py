"""Golden values for the lDDT yardstick (authoring container only).

    python tests/golden/make_golden_lddt.py   ->  tests/golden/lddt.npz

The REFERENCE's own ``lddt`` (src/models/loss.py:384-437) is imported from the reference checkout and called in float64 with a mask of
ones, ``per_residue`` both ways, on three small pairs (L = 5, 40, 130): a random-walk chain as the true structure, a noisy copy
under a rigid move as the prediction.  The fixture holds the inputs and the outputs only.  ``ml_collections`` (imported by loss.py, not
used by ``lddt``) is stubbed as a bare module (with the one name an annotation mentions) when it is not installed."""
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
import ref_tm64  # noqa: E402

_ref_import.install()
if importlib.util.find_spec("ml_collections") is None:
    sys.modules["ml_collections"] = types.ModuleType("ml_collections")
    sys.modules["ml_collections"].ConfigDict = dict   # (named in an annotation of loss.py)
from src.models import loss as RL  # noqa: E402

CASES = {"a": (5, 0.3), "b": (40, 1.0), "c": (130, 2.0)}   # tag: (L, sigma of the prediction's noise in A)


def main():
    rng = np.random.default_rng(8)
    out = {}
    for tag, (L, sigma) in CASES.items():
        true = ref_tm64.random_walk(rng, L)
        pred = ref_tm64.rigid_move(rng, true + rng.normal(size=true.shape) * sigma)
        true, pred = np.asarray(true, dtype=np.float32), np.asarray(pred, dtype=np.float32)   # (what the device is given)
        t, p = torch.as_tensor(true).double(), torch.as_tensor(pred).double()
        mask = torch.ones(L, 1, dtype=torch.float64)
        out[f"{tag}_true"], out[f"{tag}_pred"] = true, pred
        out[f"{tag}_per_residue"] = RL.lddt(p, t, mask, per_residue=True).numpy()
        out[f"{tag}_total"] = RL.lddt(p, t, mask, per_residue=False).numpy()
        assert out[f"{tag}_per_residue"].dtype == np.float64 and out[f"{tag}_per_residue"].shape == (L,)
    path = os.path.join(HERE, "lddt.npz")
    np.savez_compressed(path, **out)
    print(f"lddt.npz: {os.path.getsize(path) / 1024:.1f} KiB", {k: float(v) for k, v in out.items() if k.endswith("_total")})


if __name__ == "__main__":
    main()
