"""The deterministic inputs of the secondary-structure tests, shared by the CPU test (which asserts their margins), the device test and the
fixture script: backbones built from chosen torsions with ideal geometry (``violations_cases.build_backbone``) and the fixture proteins of
tests/golden/pdb with perturbed copies."""
import functools
import os

import numpy as np

from ref_ss import PRO
from violations_cases import build_backbone, sequence

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (L, R) of the device parity cases: no hydrogen bond possible (1, 2, 4 residues); one turn and no helix; the minimal helix; general
# cases; one word of bond bits and one past it; three words; the long-chain launch (above 256 residues)
SHAPES = ((1, 2), (2, 1), (4, 3), (5, 3), (6, 2), (13, 17), (31, 9), (64, 3), (65, 17), (129, 4), (300, 3))
HELIX, MIXED, EXTENDED, COMPACT, PI_HELIX = 0, 1, 2, 3, 4      # kinds of ensemble members, see ``ensemble``
PROTEINS = ("CLN025", "2JOF", "NuG2", "bpti")      # the fixture proteins of the device test
N_COPIES = 3                                       # perturbed copies of each
BASINS = ((-60.0, -45.0), (-120.0, 130.0), (-70.0, 145.0), (55.0, 45.0))   # alpha, beta, polyproline II, left-handed alpha

# the constructions of the CPU test: (phi, psi, L, the string they must give); all ALA, numbered consecutively
CONSTRUCTIONS = ((-57.0, -47.0, 5, "-TTT-"), (-57.0, -47.0, 6, "-HHHH-"), (-57.0, -47.0, 20, "-" + 18 * "H" + "-"),
                 (-49.0, -26.0, 12, "-" + 10 * "G" + "-"), (-57.0, -70.0, 14, "-" + 12 * "I" + "-"), (-120.0, 130.0, 12, 12 * "-"))


def regular(phi, psi, L):
    """A chain of L residues with one phi / psi, ideal geometry -> float32 [L, 5, 3]."""
    return build_backbone(np.full(L, phi), np.full(L, psi)).astype(np.float32)


def kind_of(r, R):
    """A single structure is the mixed-basin chain."""
    return r % 5 if R > 1 else MIXED


def mixed_torsions(rng, L, noise=12.0):
    """Runs of 3 .. 8 residues in one basin each, with noise -> (phi, psi) in degrees."""
    phi, psi = np.zeros(L), np.zeros(L)
    k = 0
    while k < L:
        run = int(rng.integers(3, 9))
        phi[k:k + run], psi[k:k + run] = BASINS[int(rng.integers(0, len(BASINS)))]
        k += run
    return phi + rng.normal(size=L) * noise, psi + rng.normal(size=L) * noise


@functools.lru_cache(maxsize=None)
def ensemble(L, R):
    """-> (atoms [R, L, 5, 3] float32, aatype [L], residue_index [L]), read-only.  The sequence has a GLY, a PRO and one numbering gap
    (``violations_cases.sequence``); below 8 residues, where a gap or a PRO in the middle would leave no room for the one turn and the
    minimal helix these lengths are there for, the numbering has no gap and the PRO is the first residue.  Member r is of kind
    ``kind_of(r, R)``: HELIX an alpha-helix with 4 degrees of noise on its torsions, MIXED a chain of runs in the four basins, EXTENDED a
    noisy beta-strand, COMPACT a mixed chain shrunk to 0.15 of its size: most residue pairs pass the 9 A prefilter and many atoms are
    closer than 0.5 A, where the energy is -9.9 by rule and the bond relation is dense, PI_HELIX a pi-helix with 2 degrees of noise."""
    rng = np.random.default_rng(31000 + 7 * L + R)
    aatype, ri = sequence(rng, L, with_break=L >= 8)
    if 4 <= L < 8:
        aatype[aatype == PRO] = 0
        aatype[0] = PRO
    out = np.zeros((R, L, 5, 3))
    for r in range(R):
        kind = kind_of(r, R)
        if kind == HELIX:
            x = build_backbone(-57.0 + rng.normal(size=L) * 4.0, -47.0 + rng.normal(size=L) * 4.0)
        elif kind == PI_HELIX:
            x = build_backbone(-57.0 + rng.normal(size=L) * 2.0, -70.0 + rng.normal(size=L) * 2.0)
        elif kind == EXTENDED:
            x = build_backbone(-120.0 + rng.normal(size=L) * 10.0, 130.0 + rng.normal(size=L) * 10.0)
        else:
            x = build_backbone(*mixed_torsions(rng, L))
            if kind == COMPACT:
                x *= 0.15
        out[r] = x
    out = out.astype(np.float32)
    for a in (out, aatype, ri):
        a.setflags(write=False)
    return out, aatype, ri


def protein_path(name):
    return os.path.join(GOLDEN, "pdb2010" if name == "bpti" else "pdb", f"{name}.pdb")


@functools.lru_cache(maxsize=None)
def protein(name):
    """Model 1 of a fixture protein and N_COPIES copies with 0.05, 0.15 and 0.3 A of noise on every atom
    -> (atoms [1 + N_COPIES, L, 5, 3] float32, aatype, residue_index), read-only."""
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from str2str_amd.common.pdb_utils import extract_backbone_atoms

    atoms, aatype, ri = extract_backbone_atoms(protein_path(name), max_n_model=1)
    rng = np.random.default_rng(sum(map(ord, name)))
    x = np.concatenate([atoms] + [atoms + rng.normal(size=atoms.shape) * s for s in (0.05, 0.15, 0.3)[:N_COPIES]]).astype(np.float32)
    for a in (x, aatype, ri):
        a.setflags(write=False)
    return x, aatype, ri


def parity_cases():
    """Every device parity case -> [(tag, atoms [R, L, 5, 3], aatype, residue_index)]."""
    return [(f"L{L}_R{R}", *ensemble(L, R)) for L, R in SHAPES] + [(name, *protein(name)) for name in PROTEINS]


def torsion_fixture_cases():
    """The backbones of tests/golden/torsions.npz -> {tag: (atoms [L, 5, 3] float32, aatype, residue_index)}."""
    return {"mixed31": (ensemble(31, 9)[0][1],) + ensemble(31, 9)[1:], "helix13": (ensemble(13, 17)[0][0],) + ensemble(13, 17)[1:],
            "extended65": (ensemble(65, 17)[0][2],) + ensemble(65, 17)[1:]}
