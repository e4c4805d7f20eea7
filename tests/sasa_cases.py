"""The deterministic inputs of the solvent-accessibility tests, shared by the CPU test (which asserts their margins) and the device test:
the ensembles of ``ss_cases`` (helices, mixed chains, strands and the COMPACT members shrunk to 0.15, where nearly every atom is a
neighbour of every other) and its fixture proteins with perturbed copies, under several spheres, radii, probes and existence patterns.
The yardstick's result of a case is computed once (``reference``) and shared read-only."""
import functools
from typing import NamedTuple

import numpy as np

import ref_sasa as ref
import ss_cases

# (L, R) at 96 points: one residue; one structure; fewer atoms than a wave; general cases; 320 atoms, a whole number of sweeps of 64, and
# five more; 645 atoms with a COMPACT member
SHAPES = ((1, 2), (2, 1), (4, 3), (13, 17), (31, 9), (64, 3), (65, 17), (129, 4))
# one residue past the chain length at which the kernel changes its block shape (512 threads up to 256 residues, 1024 above), at 64 points
LONG = ((257, 2, 64),)
# points on (13, 17): one lane's worth; around a wave's worth; one past the two slots per lane of the small-sphere kernel; the usual fine
# setting (two passes of the large-sphere kernel) and one point past its single pass
POINTS = (1, 63, 64, 65, 129, 513, 960)
VARIANTS = ("radii_by_residue", "probe_0", "missing_residue")   # on (31, 9)
PROTEINS = ss_cases.PROTEINS


class Case(NamedTuple):
    atoms: np.ndarray      # float32 [R, L, 5, 3]
    aatype: np.ndarray     # [L]
    exists: np.ndarray     # bool [L, 5]
    radii: np.ndarray      # float64 [L, 5]
    probe: float
    n_points: int


def tags():
    return ([f"L{L}_R{R}" for L, R in SHAPES] + [f"L{L}_R{R}_P{P}" for L, R, P in LONG] + list(PROTEINS) + [f"L13_R17_P{P}" for P in POINTS]
            + [f"L31_R9_{v}" for v in VARIANTS])


@functools.lru_cache(maxsize=None)
def case(tag) -> Case:
    if tag in PROTEINS:
        atoms, aatype, _ = ss_cases.protein(tag)
        return _frozen(Case(atoms, aatype, ref.exists_from_aatype(aatype), ref.default_radii(len(aatype)), 1.4, 96))
    parts = tag.split("_", 2)
    L, R = int(parts[0][1:]), int(parts[1][1:])
    atoms, aatype, _ = ss_cases.ensemble(L, R)
    exists, radii, probe, P = ref.exists_from_aatype(aatype), ref.default_radii(L), 1.4, 96
    rest = parts[2] if len(parts) > 2 else ""
    if rest.startswith("P"):
        P = int(rest[1:])
    elif rest == "radii_by_residue":            # the CB radius a function of aatype, the N radius of the position: a wrong index shows
        radii = radii.copy()
        radii[:, 4] = 1.7 + 0.03 * (aatype % 7)
        radii[:, 0] = 1.55 + 0.01 * (np.arange(L) % 5)
    elif rest == "probe_0":
        probe = 0.0
    elif rest == "missing_residue":             # a whole residue missing, and single atoms of others
        exists = exists.copy()
        exists[5] = False
        exists[9, 3] = exists[20, 0] = exists[0, 1] = False
    elif rest:
        raise KeyError(tag)
    return _frozen(Case(atoms, aatype, exists, radii, probe, P))


def _frozen(c):
    for a in (c.exists, c.radii):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(tag):
    """The yardstick's outputs of a case (counts, per_residue, total, margin), read-only."""
    c = case(tag)
    want = ref.ensemble(c.atoms, c.exists, c.radii, c.probe, c.n_points)
    for v in want.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return want
