"""What the ensemble test files share: the move to the device, the four-decimal comparison, the multi-model PDB writer and the loader of
the repository's eval.py."""
import importlib.util
import os

import numpy as np
import torch

from conftest import ROOT


def to_device(x):
    """An array, list or tensor on the device in its own dtype (None stays None)."""
    return None if x is None else torch.as_tensor(x if torch.is_tensor(x) else np.asarray(x)).to("cuda")


def close_4(got, want):
    """``got`` (rounded to four decimals by the metrics) against the unrounded yardstick value ``want``."""
    return abs(float(got) - float(np.around(want, decimals=4))) <= 1e-4 + 1e-12   # (+- 1e-4: a value on a rounding edge)


def write_models(path, template, coords):
    """A multi-model PDB with the CA-bearing residues of ``template`` (one model) moved to ``coords`` [R, L, 3] (all atoms of a residue
    shifted with its CA)."""
    atoms = [ln for ln in open(template) if ln.startswith("ATOM")]
    ca = np.array([[float(ln[30:38]), float(ln[38:46]), float(ln[46:54])] for ln in atoms if ln[12:16].strip() == "CA"])
    res_of = np.cumsum([ln[12:16].strip() == "N" for ln in atoms]) - 1
    with open(path, "w") as f:
        for m, x in enumerate(coords):
            f.write(f"MODEL     {m + 1:4d}\n")
            for ln, r in zip(atoms, res_of):
                p = np.array([float(ln[30:38]), float(ln[38:46]), float(ln[46:54])]) - ca[r] + x[r]
                f.write(f"{ln[:30]}{p[0]:8.3f}{p[1]:8.3f}{p[2]:8.3f}{ln[54:]}")
            f.write("ENDMDL\n")
        f.write("END\n")


def load_eval_entry(name):
    """The repository's eval.py as a module of its own called ``name`` (it is a script, not part of the package)."""
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "eval.py"))
    entry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(entry)
    return entry
